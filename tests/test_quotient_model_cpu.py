"""tests/quotient_model.py against the mathematics, on the CPU: for a satisfied permutation + lookup + gate instance at k = 4 (built with
the oracle's permutation_product, lookup_permute and lookup_product), with every column a polynomial of degree below n evaluated on the
extended domain by Python integers, the model's numerator is divisible by X^n - 1 — interpolated from its 4 n values and evaluated at
the n-th roots of unity it is zero everywhere —, it stops being so when one cell is altered, and the streaming splits of the prover
(head only, chaining and product terms over blocks of sets, joined with powers of y) add up to the monolithic call."""
import numpy as np
import pytest

import quotient_model as M

R = M.R
K, EXT, N, NE = 4, 2, 16, 64
USABLE = N - 6
N_COLS, CHUNK = 5, 2            # three sets, the last one short; degree (CHUNK + 2)(n - 1) < 4 n: the 4 n values determine the numerator


def _powers(w, m):
    out = [1] * m
    for i in range(1, m):
        out[i] = out[i - 1] * w % R
    return out


@pytest.fixture(scope="module")
def dom(O):
    w = M.scalar(O.root_of_unity(K))
    return {"w": _powers(w, N), "nat": M.Natural(K, EXT)}


def to_coset(dom, rows):
    """the values on the n rows -> the interpolant's values on the 4 n points, as Montgomery words"""
    w = dom["w"]
    ninv = pow(N, -1, R)
    coeff = [ninv * sum(v * w[(-i * r) % N] for r, v in enumerate(rows)) % R for i in range(N)]
    out = []
    for x in dom["nat"].X:
        acc = 0
        for c in reversed(coeff):
            acc = (acc * x + c) % R
        out.append(acc)
    return M.words(out)


def cosets_of(dom, cols):
    return np.stack([to_coset(dom, c) for c in cols])


def at_roots(dom, values):
    """the polynomial of degree below 4 n with these values (Montgomery words) on the 4 n points, evaluated at the n-th roots of unity"""
    v = M.O.fr_to_ints(values)
    X = dom["nat"].X
    w4 = X[1] * pow(X[0], -1, R) % R
    wp = _powers(w4, NE)
    zinv = _powers(pow(X[0], -1, R), NE)
    einv = pow(NE, -1, R)
    coeff = [einv * zinv[i] * sum(vj * wp[(-i * j) % NE] for j, vj in enumerate(v)) % R for i in range(NE)]
    # modulo X^n - 1 the coefficient i folds onto i mod n; the n values at the roots of unity are the transform of the folded ones
    folded = [sum(coeff[i::N]) % R for i in range(N)]
    return [sum(c * dom["w"][(i * r) % N] for i, c in enumerate(folded)) % R for r in range(N)]


@pytest.fixture(scope="module")
def instance(O, dom):
    rng = np.random.default_rng(20261126)
    rnd = lambda: int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) % R
    adv = [[rnd() for _ in range(N)] for _ in range(N_COLS)]
    # copy constraints among the usable rows: cycles of equal cells; every other cell maps to itself
    mapping = np.array([[(c << 32) | r for r in range(N)] for c in range(N_COLS)], dtype=np.uint64)
    cells = [(c, r) for c in range(N_COLS) for r in range(USABLE)]
    order = rng.permutation(len(cells))
    pos, in_cycles = 0, []
    for size in (2, 3, 5, 2, 7):
        cyc = [cells[i] for i in order[pos: pos + size]]
        pos += size
        in_cycles += cyc
        for (c, r), (c2, r2) in zip(cyc, cyc[1:] + cyc[:1]):
            mapping[c, r] = (c2 << 32) | r2
            adv[c][r] = adv[cyc[0][0]][cyc[0][1]]
    beta, gamma, y = (O.fr_from_ints([rnd()])[0] for _ in range(3))
    delta = O.fr_from_ints([O.DELTA_INT])[0]
    cols_m = np.stack([O.fr_from_ints(c) for c in adv])
    sigma_m = O.permutation_sigma(mapping, K)
    z_m = O.permutation_product(cols_m, sigma_m, USABLE, CHUNK, beta, gamma)
    z = [O.fr_to_ints(c) for c in z_m]
    assert z[-1][USABLE] == 1 and z[0][0] == 1
    for c in z:
        c[USABLE + 1:] = [rnd() for _ in range(N - USABLE - 1)]              # blinding rows
    # lookup: a 2-bit range table, one input column
    table = [i if i < 4 else 0 for i in range(N)]
    inp = [int(rng.integers(0, 4)) for _ in range(USABLE)] + [rnd() for _ in range(N - USABLE)]
    pa, ps = O.lookup_permute(inp[:USABLE], table[:USABLE])
    pa, ps = pa + [rnd() for _ in range(N - USABLE)], ps + [rnd() for _ in range(N - USABLE)]
    wrap = lambda v: O.fr_from_ints(v).reshape(1, N, 4)
    zl = O.fr_to_ints(O.lookup_product(wrap(inp), O.fr_from_ints(table), wrap(pa), wrap(ps), USABLE, beta, gamma)[0])
    assert zl[USABLE] == 1
    zl[USABLE + 1:] = [rnd() for _ in range(N - USABLE - 1)]
    # gates: cells [a, b, c, d] with d = a + b c where the selector is on
    gate = [rnd() for _ in range(N)]
    sel = [0] * N
    for r in (0, 3, 6):
        gate[r + 3] = (gate[r] + gate[r + 1] * gate[r + 2]) % R
        sel[r] = 1
    l0 = [1] + [0] * (N - 1)
    l_last = [1 if r == USABLE else 0 for r in range(N)]
    l_active = [1 if r < USABLE else 0 for r in range(N)]
    rows = {"adv": adv, "sigma": [O.fr_to_ints(c) for c in sigma_m], "z": z, "inp": [inp], "table": [table], "pa": [pa], "ps": [ps], "zl": [zl],
            "gate": [gate], "sel": [sel], "l": [l0, l_last, l_active]}
    return {"rows": rows, "ch": (beta, gamma, delta, y), "in_cycles": in_cycles}


def numerator(dom, rows, ch, acc0=None):
    beta, gamma, delta, y = ch
    E = {name: cosets_of(dom, cols) for name, cols in rows.items()}
    acc = np.zeros((NE, 4), dtype=np.uint64) if acc0 is None else acc0
    acc = M.gate_eval_dev(E["gate"], E["sel"], 1, K, EXT, y, acc)
    acc = M.permutation_eval_dev(E["adv"], E["sigma"], E["z"], N_COLS, CHUNK, K, EXT, USABLE, *E["l"], beta, gamma, delta, y, acc)
    return M.lookup_eval_dev(E["inp"], E["table"][0], E["pa"], E["ps"], E["zl"], 1, K, EXT, *E["l"], beta, gamma, y, acc), E


def test_numerator_of_a_satisfied_instance_vanishes_on_the_rows(dom, instance):
    num, _ = numerator(dom, instance["rows"], instance["ch"])
    assert num.any()
    assert at_roots(dom, num) == [0] * N


# (an advice cell outside every cycle is free: "adv" takes the i-th cell that a copy constraint binds)
ALTERED = [("adv", 0, None), ("adv", 11, None), ("adv", 18, None), ("z", 0, 0), ("z", 2, USABLE), ("z", 1, 5), ("sigma", 3, 4), ("inp", 0, 1), ("pa", 0, 3), ("ps", 0, USABLE - 1),
           ("zl", 0, 0), ("zl", 0, 7), ("gate", 0, 4), ("table", 0, 2)]


@pytest.mark.parametrize("name,col,row", ALTERED)
def test_one_altered_cell_breaks_divisibility(dom, instance, name, col, row):
    rows = {k: [list(c) for c in v] for k, v in instance["rows"].items()}
    if name == "adv":
        col, row = instance["in_cycles"][col]
    rows[name][col][row] = (rows[name][col][row] + 1) % R
    num, _ = numerator(dom, rows, instance["ch"])
    res = at_roots(dom, num)
    assert any(res), (name, col, row)


def test_blinding_rows_do_not_matter(dom, instance):
    """cells above the usable rows are free (product columns above row usable, advice and lookup columns from row usable on)"""
    rows = {k: [list(c) for c in v] for k, v in instance["rows"].items()}
    for name, col, row in (("adv", 2, USABLE), ("z", 1, USABLE + 1), ("pa", 0, N - 1), ("zl", 0, USABLE + 2), ("inp", 0, USABLE + 1)):
        rows[name][col][row] = (rows[name][col][row] + 12345) % R
    num, _ = numerator(dom, rows, instance["ch"])
    assert at_roots(dom, num) == [0] * N


def _pow_words(O, y, e):
    return O.fr_from_ints([pow(M.scalar(y), e, R)])[0]


@pytest.mark.parametrize("layout", ["natural", "cosets3", "cosets4"])
@pytest.mark.parametrize("head2", [0, 2])
def test_streaming_splits_join_to_the_monolithic_call(O, dom, instance, layout, head2):
    """head only, then per block of sets a chaining call and a product call (block buffers that start one set early, as the prover's do),
    into accumulators of their own, joined as (A2 y^n3 + A3) y^n4 + A4 — on arbitrary arrays, in both layouts"""
    rng = np.random.default_rng(7 + head2)
    beta, gamma, delta, y = instance["ch"]
    n_sets, n_lk = 3, 2
    if layout == "natural":
        pts, shape = NE, (NE,)
        perm = lambda *a: M.permutation_eval_parts_dev(*a[:9], K, EXT, *a[9:])
        look = lambda *a: M.lookup_eval_dev(*a[:6], K, EXT, *a[6:])
    else:
        slots = int(layout[-1])
        pts, shape = slots * N, (slots, N)
        perm = lambda *a: M.permutation_eval_parts_cosets_dev(*a[:9], K, slots, *a[9:])
        look = lambda *a: M.lookup_eval_cosets_dev(*a[:6], K, slots, *a[6:])
    arr = lambda m: O.random_fr(rng, m * pts).reshape((m,) + shape + (4,))
    adv, sig, z, lsel, tab, pa, ps, zl, inp = (arr(m) for m in (N_COLS, N_COLS, n_sets, 3, 1, n_lk, n_lk, n_lk, n_lk))
    if head2:
        sig_in = O.fr_mul(sig.reshape(-1, 4), np.broadcast_to(beta, (N_COLS * pts, 4)).copy()).reshape(sig.shape)
    else:
        sig_in = sig
    zero = np.zeros(shape + (4,), dtype=np.uint64)
    tail = (USABLE, lsel[0], lsel[1], lsel[2], beta, gamma, delta, y)
    mono = perm(adv, 0, sig, z, 0, z[0], z[n_sets - 1], N_COLS, CHUNK, *tail, zero, 1, 1, n_sets, 0, n_sets)
    mono = look(inp, tab[0], pa, ps, zl, n_lk, lsel[0], lsel[1], lsel[2], beta, gamma, y, mono)
    a2 = perm(None, 0, None, None, 0, z[0], z[n_sets - 1], N_COLS, CHUNK, *tail, zero, 1, 0, 0, 0, 0)
    a3, a4 = zero, zero
    for set_lo, set_hi in ((0, 2), (2, 3)):
        z0 = max(set_lo - 1, 0)
        if max(set_lo, 1) < set_hi:
            a2 = perm(None, 0, None, z[z0:], z0, None, None, N_COLS, CHUNK, *tail, a2, 0, max(set_lo, 1), set_hi, 0, 0)
        c_lo = z0 * CHUNK                                 # the advice block starts one set early, the sigma block at the first set asked for
        a3 = perm(adv[c_lo:], c_lo, sig_in[set_lo * CHUNK:], z[z0:], z0, None, None, N_COLS, CHUNK, *tail, a3, head2, 0, 0, set_lo, set_hi)
    for j0 in (0, 1):
        a4 = look(inp[j0: j0 + 1], tab[0], pa[j0: j0 + 1], ps[j0: j0 + 1], zl[j0: j0 + 1], 1, lsel[0], lsel[1], lsel[2], beta, gamma, y, a4)
    n3, n4 = n_sets, 5 * n_lk
    a3 = M.poly_axpy_dev(a3.reshape(-1, 4), _pow_words(O, y, n3), a2.reshape(-1, 4), pts)
    a4 = M.poly_axpy_dev(a4.reshape(-1, 4), _pow_words(O, y, n4), a3, pts)
    assert np.array_equal(a4, mono.reshape(-1, 4))


def test_cosets_are_the_natural_order_points_taken_four_apart(O, dom, instance):
    rng = np.random.default_rng(99)
    beta, gamma, delta, y = instance["ch"]
    arr = lambda m: O.random_fr(rng, m * NE).reshape(m, NE, 4)
    adv, sig, z, lsel, acc = arr(N_COLS), arr(N_COLS), arr(3), arr(3), arr(1)[0]
    slots = lambda a, s: np.ascontiguousarray(np.stack([a[..., M.SLOT_POINT[t]::4, :] for t in range(s)], axis=-3))
    nat = M.permutation_eval_parts_dev(adv, 0, sig, z, 0, z[0], z[2], N_COLS, CHUNK, K, EXT, 3, *lsel, beta, gamma, delta, y, acc, 1, 1, 3, 0, 3)
    for s in (1, 3, 4):
        got = M.permutation_eval_parts_cosets_dev(slots(adv, s), 0, slots(sig, s), slots(z, s), 0, slots(z[0], s), slots(z[2], s), N_COLS, CHUNK, K, s, 3,
                                                  *(slots(l, s) for l in lsel), beta, gamma, delta, y, slots(acc, s), 1, 1, 3, 0, 3)
        assert np.array_equal(got, slots(nat, s))
    g_nat = M.gate_eval_sub_dev(adv, 2, slots(sig, 2).transpose(0, 2, 1, 3).reshape(N_COLS, 2 * N, 4), N_COLS, K, 1, y, acc[: 2 * N])
    g_cos = M.gate_eval_cosets_dev(slots(adv, 3), 3, slots(sig, 2), N_COLS, K, 2, y, np.ascontiguousarray(np.stack([acc[0: 2 * N: 2], acc[1: 2 * N: 2]])))
    assert np.array_equal(g_cos[0], g_nat[0::2]) and np.array_equal(g_cos[1], g_nat[1::2])


def test_the_others(O):
    rng = np.random.default_rng(3)
    x, acc = O.random_fr(rng, 9), O.random_fr(rng, 9)
    a = O.random_fr(rng, 1)[0]
    ax = O.fr_mul(x, np.broadcast_to(a, (9, 4)).copy())
    assert np.array_equal(M.poly_scale_dev(x, a, 9), ax)
    assert np.array_equal(M.poly_axpy_dev(acc, a, x, 9), O.fr_add(acc, ax))
    idx = np.array([8, 0, 0, 3], dtype=np.int64)
    assert np.array_equal(M.gather_fr_dev(x, idx, 4), x[[8, 0, 0, 3]])


def test_gpu_cases_put_every_edge_word_into_every_role():
    """the case generator of tests/test_gpu_quotient_pointwise.py, checked without a GPU: every word of its edge set W occurs in every
    input role of every kernel at least once over the cases"""
    import test_gpu_quotient_pointwise as G
    G.test_every_edge_word_reaches_every_role()
