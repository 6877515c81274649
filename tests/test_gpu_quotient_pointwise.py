"""The pointwise kernels of the quotient numerator (k_perm_eval, k_lookup_eval, k_gate_eval, k_poly_axpy, k_poly_scale, k_gather_fr) and
the product columns' production route, held bit for bit to the Python-integer restatement of tests/quotient_model.py — on arbitrary
arrays of canonical memory words, uploaded raw: seeded-random words mixed with the edge set W below (the limb patterns the kernels'
hand-derived bounds are about), constant arrays, a satisfied shape (left == right) and left factors r - 1 against right factors 0;
at the smallest shapes where the index arithmetic can go wrong (a partial workgroup, two workgroups, two workgroups a slot; 1..4 slots;
usable rows 0, 1, n - 6, n - 1; chunks of 1, 3, 7 and 9 of 7 columns), through every streaming split the prover makes.

Every device array is allocated at twice its size with other words behind it: a kernel that indexes a block buffer from the wrong
origin then computes a wrong value, which these tests catch, instead of leaving its allocation.

The integer model's share of the run time is added up in MODEL_SECONDS and printed when the module is done (pytest -s)."""
import ctypes
import time

import numpy as np
import pytest

import quotient_model as M

pytestmark = pytest.mark.gpu

R = M.R
ONE = (1 << 256) % R                       # the memory word of one
LOW232 = ((R >> 232) << 232) - 1           # the largest word below r whose low 232 bits are all ones
W = [0, 1, 2, R - 1, R - 2, (R + 1) // 2, (R - 1) // 2, ONE, R - ONE, 1 << 253, (1 << 253) - 1, LOW232]
assert len(set(W)) == 12 and all(0 <= w < R for w in W) and LOW232 & ((1 << 232) - 1) == (1 << 232) - 1 and LOW232 + (1 << 232) >= R
sz = ctypes.c_size_t
MODEL_SECONDS = [0.0]


def timed(fn, *a):
    t = time.perf_counter()
    out = fn(*a)
    MODEL_SECONDS[0] += time.perf_counter() - t
    return out


# ---- inputs: raw memory words ---------------------------------------------------------------------------------------------------------
class Seen:
    """which words of W reached which input role"""
    def __init__(self):
        self.roles = {}

    def note(self, role, vals):
        self.roles.setdefault(role, set()).update(v for v in vals if v in W_SET)

    def missing(self):
        return {role: sorted(W_SET - s) for role, s in self.roles.items() if s != W_SET}


W_SET = set(W)


def raw(vals):
    return M.O.ints_to_limbs(vals)


def mixed(rng, seen, role, *shape):
    """seeded-random words below r, a third of the positions (at least one) taken by words of W, starting at a random one"""
    count = int(np.prod(shape))
    vals = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(count)]
    start = int(rng.integers(0, 12))
    for i, pos in enumerate(rng.permutation(count)[: max(1, count // 3)]):
        vals[int(pos)] = W[(start + i) % 12]
    seen.note(role, vals)
    return raw(vals).reshape(shape + (4,))


def const(seen, role, w, *shape):
    seen.note(role, [w])
    return np.ascontiguousarray(np.broadcast_to(raw([w])[0], shape + (4,)))


def challenge(rng, seen, role, i, step):
    """odd cases draw from W (walking through all of it), even ones at random"""
    v = W[(i // 2 * step + step) % 12] if i % 2 else int.from_bytes(rng.bytes(32), "little") % R
    seen.note(role, [v])
    return raw([v])[0]


class Layout:
    """slots == 0: the natural order of 4 n points (rotations by four); otherwise `slots` cosets of n points"""
    def __init__(self, k, slots):
        self.k, self.slots, self.n = k, slots, 1 << k
        self.pts = (4 << k) if slots == 0 else slots << k

    def __repr__(self):
        return f"k={self.k} " + ("natural" if self.slots == 0 else f"{self.slots} slots")


def perm_inputs(rng, seen, lay, n_cols, n_sets, i, kind="mixed", pair=None):
    p = lay.pts
    d = {}
    if kind == "const":             # every array one constant word; z and adv take every pair
        wz, wa = pair
        names = ("sigma", "l0", "l_last", "l_active", "acc2", "acc3")
        d = {name: const(seen, "perm." + name, W[(i + 5 * j + 1) % 12], *((n_cols, p) if name == "sigma" else (p,))) for j, name in enumerate(names)}
        d["adv"], d["z"] = const(seen, "perm.adv", wa, n_cols, p), const(seen, "perm.z", wz, n_sets, p)
        d["beta"], d["gamma"], d["y"] = (const(seen, "perm." + name, W[(m * i + i // 12 + off) % 12]) for name, m, off in (("beta", 1, 0), ("gamma", 5, 1), ("y", 7, 2)))
        return d
    for name, m in (("adv", n_cols), ("sigma", n_cols), ("z", n_sets)):
        d[name] = mixed(rng, seen, "perm." + name, m, p)
    for name in ("l0", "l_last", "l_active", "acc2", "acc3"):
        d[name] = mixed(rng, seen, "perm." + name, p)
    d["beta"], d["gamma"], d["y"] = (challenge(rng, seen, "perm." + name, i, step) for name, step in (("beta", 1), ("gamma", 5), ("y", 7)))
    if kind in ("satisfied", "left r-1 right 0"):
        dom = M.Natural(lay.k, 2) if lay.slots == 0 else M.Cosets(lay.k, lay.slots)
        beta, gamma = (M.scalar(d[x]) or 1 for x in ("beta", "gamma"))
        d["beta"], d["gamma"] = M.words([beta])[0], M.words([gamma])[0]
        dpow = [pow(M.O.DELTA_INT, c, R) for c in range(n_cols)]
        if kind == "satisfied":     # z == 1 and sigma the identity permutation: left == right at every point
            d["z"] = const(seen, "perm.z", ONE, n_sets, p)
            d["sigma"] = np.stack([M.words([dpow[c] * x % R for x in dom.X]) for c in range(n_cols)])
        else:                       # a = -(gamma + delta^c beta X): right factors 0; sigma = (-1 - a - gamma) / beta: left factors r - 1
            a = [[-(gamma + dpow[c] * beta * x) % R for x in dom.X] for c in range(n_cols)]
            d["adv"] = np.stack([M.words(col) for col in a])
            d["sigma"] = np.stack([M.words([(-1 - v - gamma) * pow(beta, -1, R) % R for v in col]) for col in a])
    return d


# ---- device side ----------------------------------------------------------------------------------------------------------------------
class Dev:
    def __init__(self, api):
        self.api, self.bufs = api, []

    def put(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        b = self.api.DeviceBuffer(2 * max(arr.nbytes, 32))
        b.upload(arr)
        b.upload(np.ascontiguousarray(arr.reshape(-1, 4)[::-1]), offset=arr.nbytes)      # the guard: other canonical words
        self.bufs.append(b)
        return b

    def free(self):
        for b in self.bufs:
            b.free()


def at(buf, elems):
    return ctypes.c_void_p(buf.ptr.value + 32 * elems)


@pytest.fixture(scope="module")
def env(O):
    from halo2_vectordb_amd import api
    from halo2_vectordb_amd._lib import check
    lib = api.init(0)
    yield {"api": api, "lib": lib, "check": check, "delta": api.fr_delta(), "O": O}
    print(f"\ninteger model: {MODEL_SECONDS[0]:.1f} s")


class Perm:
    """one case's arrays on the host and on the device, and the two ways to make a call: the kernel's and the model's"""
    def __init__(self, env, lay, n_cols, chunk, usable, d):
        self.env, self.lay, self.n_cols, self.chunk, self.usable, self.d = env, lay, n_cols, chunk, usable, d
        self.n_sets = -(-n_cols // chunk)
        self.dev = Dev(env["api"])
        self.b = {name: self.dev.put(d[name]) for name in ("adv", "sigma", "z", "l0", "l_last", "l_active")}

    def kernel(self, acc_buf, adv_col0, sig_col0, z_set0, zfl, head, clo, chi, slo, shi, with_cols=True, with_z=True, n_slots=None):
        lib, api, lay, p = self.env["lib"], self.env["api"], self.lay, self.lay.pts
        fn = lib.vdb_permutation_eval_parts_dev if lay.slots == 0 else lib.vdb_permutation_eval_parts_cosets_dev
        return fn(at(self.b["adv"], adv_col0 * p) if with_cols else None, sz(adv_col0), at(self.b["sigma"], sig_col0 * p) if with_cols else None,
                  at(self.b["z"], z_set0 * p) if with_z else None, sz(z_set0), at(self.b["z"], 0) if zfl else None,
                  at(self.b["z"], (self.n_sets - 1) * p) if zfl else None, sz(self.n_cols), sz(self.chunk), lay.k,
                  (lay.slots or 2) if n_slots is None else n_slots, sz(self.usable), self.b["l0"].ptr, self.b["l_last"].ptr, self.b["l_active"].ptr, api._p(self.d["beta"]), api._p(self.d["gamma"]), api._p(self.env["delta"]),
                  api._p(self.d["y"]), acc_buf.ptr, head, sz(clo), sz(chi), sz(slo), sz(shi))

    def model(self, acc, adv_col0, sig_col0, z_set0, zfl, head, clo, chi, slo, shi, with_cols=True, with_z=True):
        d, lay = self.d, self.lay
        fn = M.permutation_eval_parts_dev if lay.slots == 0 else M.permutation_eval_parts_cosets_dev
        return timed(fn, d["adv"][adv_col0:] if with_cols else None, adv_col0, d["sigma"][sig_col0:] if with_cols else None, d["z"][z_set0:] if with_z else None,
                     z_set0, d["z"][0] if zfl else None, d["z"][self.n_sets - 1] if zfl else None, self.n_cols, self.chunk, lay.k, lay.slots or 2, self.usable,
                     d["l0"], d["l_last"], d["l_active"], d["beta"], d["gamma"], self.env["delta"], d["y"], acc, head, clo, chi, slo, shi).reshape(-1, 4)

    def both(self, acc_buf, acc, *a, **kw):
        """the same call on the device (into acc_buf) and in the model (from acc) -> the model's new accumulator, after comparing"""
        self.env["check"](self.kernel(acc_buf, *a, **kw))
        want = self.model(acc, *a, **kw)
        got = acc_buf.download((self.lay.pts, 4))
        assert np.array_equal(got, want), (self.lay, self.n_cols, self.chunk, self.usable, a, kw, int((got != want).any(axis=1).sum()))
        return want

    def production(self, head2, early):
        """rounds.py's pattern: head only (null column pointers); per block of 2 chunk_len columns a chaining-only call with
        z_set0 = max(set_lo - 1, 0) and a product call on block buffers; the accumulators joined with vdb_poly_axpy_dev by y^n3.
        -> the joined accumulator (kernel == model asserted at every call)"""
        env, d, p, chunk = self.env, self.d, self.lay.pts, self.chunk
        a2_buf, a3_buf = self.dev.put(d["acc2"]), self.dev.put(d["acc3"])
        a2 = self.both(a2_buf, d["acc2"], 0, 0, 0, True, 1, 0, 0, 0, 0, with_cols=False, with_z=False)
        a3 = d["acc3"]
        for c0 in range(0, self.n_cols, 2 * chunk):
            nb = min(2 * chunk, self.n_cols - c0)
            set_lo, set_hi = c0 // chunk, -(-(c0 + nb) // chunk)
            z0 = max(set_lo - 1, 0)
            if max(set_lo, 1) < set_hi:
                a2 = self.both(a2_buf, a2, 0, 0, z0, False, 0, max(set_lo, 1), set_hi, 0, 0, with_cols=False)
            adv_col0 = c0 - chunk if early and c0 >= chunk else c0
            a3 = self.both(a3_buf, a3, adv_col0, c0, z0, False, head2, 0, 0, set_lo, set_hi)
        yn3 = M.words([pow(M.scalar(d["y"]), self.n_sets, R)])[0]
        env["check"](env["lib"].vdb_poly_axpy_dev(a3_buf.ptr, env["api"]._p(yn3), a2_buf.ptr, sz(p)))
        joined = a3_buf.download((p, 4))
        assert np.array_equal(joined, timed(M.poly_axpy_dev, a3, yn3, a2, p))
        return joined

    def monolithic(self, head2):
        """the model's value of all terms in one call from acc2, times nothing, plus acc3 y^n3: what the joined accumulators must be"""
        mono = self.model(self.d["acc2"], 0, 0, 0, True, 1 | head2, 1, self.n_sets, 0, self.n_sets)
        yn3 = M.words([pow(M.scalar(self.d["y"]), self.n_sets, R)])[0]
        return mono, timed(M.poly_axpy_dev, mono, yn3, self.d["acc3"], self.lay.pts)


# (k, slots — 0: natural order —, usable as an offset from n when negative, chunk_len); n_cols = 7 throughout
N_COLS = 7
PERM_SHAPES = [(3, 0, -6, 3), (3, 0, 0, 1), (3, 0, 1, 7), (3, 0, -1, 9), (7, 0, -6, 1), (7, 0, 0, 3),
               (3, 1, 0, 3), (3, 2, 1, 1), (3, 3, -6, 7), (3, 4, -1, 9), (7, 1, -1, 1), (7, 2, -6, 9), (7, 3, 0, 3), (7, 4, 1, 7),
               (9, 1, 1, 3), (9, 3, -6, 3), (9, 2, 0, 1)]
STRUCTURED = [("satisfied", 3, 3, -6, 3), ("satisfied", 7, 0, 1, 1), ("left r-1 right 0", 3, 2, 0, 3), ("left r-1 right 0", 7, 3, -6, 9), ("left r-1 right 0", 3, 0, -1, 1)]


def perm_case_inputs(seen):
    """every permutation case's inputs, in a fixed order: (kind, layout, usable, chunk, arrays)"""
    out = []
    for i, (k, slots, usable, chunk) in enumerate(PERM_SHAPES):
        lay = Layout(k, slots)
        rng = np.random.default_rng(1000 + i)
        out.append(("mixed", lay, usable % lay.n, chunk, perm_inputs(rng, seen, lay, N_COLS, -(-N_COLS // chunk), i)))
    for i, (kind, k, slots, usable, chunk) in enumerate(STRUCTURED):
        lay = Layout(k, slots)
        rng = np.random.default_rng(2000 + i)
        out.append((kind, lay, usable % lay.n, chunk, perm_inputs(rng, seen, lay, N_COLS, -(-N_COLS // chunk), i, kind)))
    return out


def perm_const_inputs(seen):
    lay = Layout(3, 1)
    return [(lay, perm_inputs(None, seen, lay, 3, 1, i, "const", (wz, wa))) for i, (wz, wa) in enumerate((wz, wa) for wz in W for wa in W)]


def lookup_inputs(rng, seen, lay, n_lk, i, w=None):
    p = lay.pts
    d = {}
    names = (("inp", (n_lk, p)), ("pa", (n_lk, p)), ("ps", (n_lk, p)), ("z", (n_lk, p)), ("table", (p,)), ("l0", (p,)), ("l_last", (p,)), ("l_active", (p,)),
             ("acc", (p,)), ("acc3", (p,)))
    for j, (name, shape) in enumerate(names):
        d[name] = mixed(rng, seen, "lookup." + name, *shape) if w is None else const(seen, "lookup." + name, W[(w + 5 * j) % 12], *shape)
    for j, name in enumerate(("beta", "gamma", "y")):
        d[name] = challenge(rng, seen, "lookup." + name, i, (1, 5, 7)[j]) if w is None else const(seen, "lookup." + name, W[(w + 7 * j + 3) % 12])
    return d


LOOKUP_SHAPES = [(3, 0), (7, 0), (3, 1), (3, 2), (3, 3), (3, 4), (7, 1), (7, 2), (7, 3), (7, 4), (9, 2), (9, 3)]


def lookup_case_inputs(seen):
    out = []
    for i, (k, slots) in enumerate(LOOKUP_SHAPES):
        out.append((Layout(k, slots), lookup_inputs(np.random.default_rng(3000 + i), seen, Layout(k, slots), 2, i)))
    for w in range(12):
        out.append((Layout(3, 1 + w % 4), lookup_inputs(None, seen, Layout(3, 1 + w % 4), 2, w, w)))
    return out


# (k, natural: (e, sub) / cosets: None)
GATE_SHAPES = [(3, (1, 0)), (3, (1, 1)), (3, (2, 0)), (3, (2, 1)), (7, (1, 1)), (7, (2, 0)), (7, (2, 1)), (7, (1, 0)), (3, None), (7, None), (9, None), (3, None)]
GATE_COLS = 3


def gate_case_inputs(seen):
    out = []
    for i, (k, nat) in enumerate(GATE_SHAPES):
        rng = np.random.default_rng(4000 + i)
        n = 1 << k
        pa, ps = ((n << (nat[0] + nat[1]), n << nat[0]) if nat else (3 * n, 2 * n))
        d = {"adv": mixed(rng, seen, "gate.adv", GATE_COLS, pa), "sel": mixed(rng, seen, "gate.sel", GATE_COLS, ps), "acc": mixed(rng, seen, "gate.acc", ps),
             "y": challenge(rng, seen, "gate.y", 2 * i + 1 if i < 12 else i, 1)}
        out.append((k, nat, d))
    return out


def test_every_edge_word_reaches_every_role():
    """CPU side: over the cases of this file, every word of W occurs in every input role of every kernel"""
    seen = Seen()
    perm_case_inputs(seen)
    perm_const_inputs(seen)
    lookup_case_inputs(seen)
    gate_case_inputs(seen)
    roles = set(seen.roles)
    assert roles == {"perm." + x for x in ("adv", "sigma", "z", "l0", "l_last", "l_active", "acc2", "acc3", "beta", "gamma", "y")} | \
        {"lookup." + x for x in ("inp", "pa", "ps", "z", "table", "l0", "l_last", "l_active", "acc", "acc3", "beta", "gamma", "y")} | \
        {"gate." + x for x in ("adv", "sel", "acc", "y")}
    assert seen.missing() == {}


# ---- permutation ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def perm_cases():
    return perm_case_inputs(Seen())


@pytest.mark.parametrize("idx", range(len(PERM_SHAPES) + len(STRUCTURED)))
def test_permutation_terms_through_every_split(env, perm_cases, idx):
    """the production pattern into accumulators of their own (head 0 and 2; block buffers that start one set early and exactly), every
    call against the model with the same arguments and the join against the model's monolithic value; in the natural order also
    vdb_permutation_eval_dev and vdb_permutation_eval_range_dev over [0, 1), [1, n_sets)"""
    kind, lay, usable, chunk, d = perm_cases[idx]
    lib, api, check = env["lib"], env["api"], env["check"]
    c = Perm(env, lay, N_COLS, chunk, usable, d)
    try:
        variants = [(0, True), (2, False)] if lay.k >= 9 else [(0, True), (0, False), (2, True), (2, False)]
        want = {}
        for head2, early in variants:
            if head2 not in want:
                want[head2] = c.monolithic(head2)
            assert np.array_equal(c.production(head2, early), want[head2][1]), (kind, lay, head2, early)
        if lay.slots == 0:
            p, b = lay.pts, c.b
            tail = (sz(N_COLS), sz(chunk), lay.k, 2, sz(usable), b["l0"].ptr, b["l_last"].ptr, b["l_active"].ptr, api._p(d["beta"]), api._p(d["gamma"]),
                    api._p(env["delta"]), api._p(d["y"]))
            acc = c.dev.put(d["acc2"])
            check(lib.vdb_permutation_eval_dev(b["adv"].ptr, b["sigma"].ptr, b["z"].ptr, *tail, acc.ptr))
            assert np.array_equal(acc.download((p, 4)), want[0][0])
            mono = timed(M.permutation_eval_dev, d["adv"], d["sigma"], d["z"], N_COLS, chunk, lay.k, 2, usable, d["l0"], d["l_last"], d["l_active"], d["beta"],
                         d["gamma"], env["delta"], d["y"], d["acc2"])
            assert np.array_equal(mono, want[0][0])
            if c.n_sets > 1:
                acc.upload(d["acc2"])
                cur = d["acc2"]
                for lo, hi in ((0, 1), (1, c.n_sets)):
                    check(lib.vdb_permutation_eval_range_dev(b["adv"].ptr, at(b["sigma"], lo * chunk * p), b["z"].ptr, *tail, acc.ptr, sz(lo), sz(hi)))
                    cur = timed(M.permutation_eval_range_dev, d["adv"], d["sigma"][lo * chunk:], d["z"], N_COLS, chunk, lay.k, 2, usable, d["l0"], d["l_last"],
                                d["l_active"], d["beta"], d["gamma"], env["delta"], d["y"], cur, lo, hi)
                    assert np.array_equal(acc.download((p, 4)), cur), (lo, hi)
                assert np.array_equal(cur, want[0][0])
    finally:
        c.dev.free()


def test_permutation_terms_on_constant_arrays(env):
    """every array one constant word of W; the product column and the advice take every pair (one set of three columns, one slot of 8 rows)"""
    for i, (lay, d) in enumerate(perm_const_inputs(Seen())):
        c = Perm(env, lay, 3, 3, 2, d)
        try:
            acc = c.dev.put(d["acc2"])
            c.both(acc, d["acc2"], 0, 0, 0, True, 1 | (2 if i % 2 else 0), 1, 1, 0, 1)
        finally:
            c.dev.free()


def test_permutation_argument_checks(env):
    """each refused call returns VDB_ERR_ARG and leaves the accumulator bit-identical"""
    lay = Layout(3, 3)
    seen = Seen()
    d = perm_inputs(np.random.default_rng(5), seen, lay, N_COLS, 3, 0)
    c = Perm(env, lay, N_COLS, 3, 2, d)
    nat = Perm(env, Layout(3, 0), N_COLS, 3, 2, perm_inputs(np.random.default_rng(6), seen, Layout(3, 0), N_COLS, 3, 0))
    try:
        for case in (c, nat):
            acc = case.dev.put(case.d["acc2"])
            #          adv_col0, sig_col0, z_set0, z_first/last, head, chain_lo, chain_hi, set_lo, set_hi
            refused = [(0, 0, 0, False, 0, 0, 2, 0, 0),        # chain_lo = 0: the chaining term of set 0 does not exist
                       (0, 0, 2, False, 0, 2, 3, 0, 0),        # chain_lo - 1 < z_set0
                       (0, 3, 2, False, 0, 0, 0, 1, 2),        # set_lo < z_set0
                       (4, 3, 0, False, 0, 0, 0, 1, 2),        # set_lo chunk_len < adv_col0
                       (0, 0, 0, False, 1, 0, 0, 0, 0),        # head & 1 without the first / last product coset
                       (0, 0, 0, True, 1, 1, 3, 0, 4)]         # set_hi beyond the sets
            for a in refused:
                assert case.kernel(acc, *a) == -3, a
                assert np.array_equal(acc.download((case.lay.pts, 4)), case.d["acc2"]), a
            env["check"](case.kernel(acc, 0, 0, 0, True, 1, 1, 3, 0, 3))          # (the same buffers are fine in an allowed call)
            assert not np.array_equal(acc.download((case.lay.pts, 4)), case.d["acc2"])
        acc = c.dev.put(d["acc2"])
        for slots in (0, 5):
            assert c.kernel(acc, 0, 0, 0, True, 1, 1, 3, 0, 3, n_slots=slots) == -3, slots
            assert np.array_equal(acc.download((lay.pts, 4)), d["acc2"]), slots
    finally:
        c.dev.free()
        nat.dev.free()


# ---- lookup ---------------------------------------------------------------------------------------------------------------------------
def test_lookup_terms(env):
    """vdb_lookup_eval_dev / _cosets_dev: two columns in one call and column by column (the prover's thirds of a block), then joined by
    y^n4 onto an arbitrary accumulator with vdb_poly_axpy_dev"""
    lib, api, check = env["lib"], env["api"], env["check"]
    for lay, d in lookup_case_inputs(Seen()):
        dev = Dev(api)
        try:
            b = {name: dev.put(d[name]) for name in ("inp", "pa", "ps", "z", "table", "l0", "l_last", "l_active")}
            p, n_lk = lay.pts, 2
            fn = lib.vdb_lookup_eval_dev if lay.slots == 0 else lib.vdb_lookup_eval_cosets_dev
            mfn = M.lookup_eval_dev if lay.slots == 0 else M.lookup_eval_cosets_dev

            def run(acc_buf, j0, m):
                return fn(at(b["inp"], j0 * p), b["table"].ptr, at(b["pa"], j0 * p), at(b["ps"], j0 * p), at(b["z"], j0 * p), sz(m), lay.k, lay.slots or 2, b["l0"].ptr,
                          b["l_last"].ptr, b["l_active"].ptr, api._p(d["beta"]), api._p(d["gamma"]), api._p(d["y"]), acc_buf.ptr)

            def model(acc, j0, m):
                return timed(mfn, d["inp"][j0:], d["table"], d["pa"][j0:], d["ps"][j0:], d["z"][j0:], m, lay.k, lay.slots or 2, d["l0"], d["l_last"], d["l_active"],
                             d["beta"], d["gamma"], d["y"], acc).reshape(-1, 4)
            a1, a2 = dev.put(d["acc"]), dev.put(d["acc"])
            check(run(a1, 0, n_lk))
            whole = model(d["acc"], 0, n_lk)
            assert np.array_equal(a1.download((p, 4)), whole), lay
            cur = d["acc"]
            for j0 in range(n_lk):
                check(run(a2, j0, 1))
                cur = model(cur, j0, 1)
                assert np.array_equal(a2.download((p, 4)), cur), (lay, j0)
            assert np.array_equal(cur, whole)
            a3 = dev.put(d["acc3"])
            yn4 = M.words([pow(M.scalar(d["y"]), 5 * n_lk, R)])[0]
            check(lib.vdb_poly_axpy_dev(a2.ptr, api._p(yn4), a3.ptr, sz(p)))
            assert np.array_equal(a2.download((p, 4)), timed(M.poly_axpy_dev, whole, yn4, d["acc3"], p)), lay
            if lay.slots:
                for slots in (0, 5):
                    assert fn(b["inp"].ptr, b["table"].ptr, b["pa"].ptr, b["ps"].ptr, b["z"].ptr, sz(1), lay.k, slots, b["l0"].ptr, b["l_last"].ptr, b["l_active"].ptr,
                              api._p(d["beta"]), api._p(d["gamma"]), api._p(d["y"]), a1.ptr) == -3
                assert np.array_equal(a1.download((p, 4)), whole)
        finally:
            dev.free()


# ---- gates ----------------------------------------------------------------------------------------------------------------------------
def test_gate_terms(env):
    """natural order with e in {1, 2} on advice cosets of the same size (sub = 0, both entry points) and of twice the size (sub = 1);
    coset by coset: two slots on three-slot advice"""
    lib, api, check = env["lib"], env["api"], env["check"]
    for k, nat, d in gate_case_inputs(Seen()):
        dev = Dev(api)
        try:
            adv, sel, acc = dev.put(d["adv"]), dev.put(d["sel"]), dev.put(d["acc"])
            pts = d["acc"].shape[0]
            if nat:
                e, sub = nat
                check(lib.vdb_gate_eval_sub_dev(adv.ptr, e + sub, sel.ptr, sz(GATE_COLS), k, e, api._p(d["y"]), acc.ptr))
                want = timed(M.gate_eval_sub_dev, d["adv"], e + sub, d["sel"], GATE_COLS, k, e, d["y"], d["acc"])
                assert np.array_equal(acc.download((pts, 4)), want), (k, nat)
                if sub == 0:
                    acc.upload(d["acc"])
                    check(lib.vdb_gate_eval_dev(adv.ptr, sel.ptr, sz(GATE_COLS), k, e, api._p(d["y"]), acc.ptr))
                    assert np.array_equal(acc.download((pts, 4)), want), (k, nat)
                    assert np.array_equal(timed(M.gate_eval_dev, d["adv"], d["sel"], GATE_COLS, k, e, d["y"], d["acc"]), want)
            else:
                check(lib.vdb_gate_eval_cosets_dev(adv.ptr, 3, sel.ptr, sz(GATE_COLS), k, 2, api._p(d["y"]), acc.ptr))
                want = timed(M.gate_eval_cosets_dev, d["adv"], 3, d["sel"], GATE_COLS, k, 2, d["y"], d["acc"]).reshape(-1, 4)
                assert np.array_equal(acc.download((pts, 4)), want), k
        finally:
            dev.free()


# ---- axpy, scale, gather --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_axpy_scale_gather(env, n):
    lib, api, check = env["lib"], env["api"], env["check"]
    rng = np.random.default_rng(n)
    seen = Seen()
    dev = Dev(api)
    try:
        for a_w in W[: 12 if n <= 257 else 4] + [int.from_bytes(rng.bytes(32), "little") % R]:
            a = raw([a_w])[0]
            x, acc = mixed(rng, seen, "x", n), mixed(rng, seen, "acc", n)
            bx, bacc = dev.put(x), dev.put(acc)
            check(lib.vdb_poly_axpy_dev(bacc.ptr, api._p(a), bx.ptr, sz(n)))
            assert np.array_equal(bacc.download((n, 4)), timed(M.poly_axpy_dev, acc, a, x, n))
            assert np.array_equal(bx.download((2 * n, 4))[n:], x[::-1]) and np.array_equal(bacc.download((2 * n, 4))[n:], acc[::-1])     # nothing past n
            check(lib.vdb_poly_scale_dev(bx.ptr, api._p(a), sz(n)))
            assert np.array_equal(bx.download((2 * n, 4)), np.concatenate([timed(M.poly_scale_dev, x, a, n), x[::-1]]))
        src = mixed(rng, seen, "src", 1000)
        idx = rng.integers(0, 1000, size=n).astype(np.int64)
        idx[0], idx[-1] = 999, 0
        bs, bo = dev.put(src), dev.put(np.zeros((n, 4), dtype=np.uint64))
        bi = api.DeviceBuffer(max(idx.nbytes, 32))
        dev.bufs.append(bi)
        bi.upload(idx)
        check(lib.vdb_gather_fr_dev(bs.ptr, bi.ptr, sz(n), bo.ptr))
        assert np.array_equal(bo.download((n, 4)), M.gather_fr_dev(src, idx, n))
    finally:
        dev.free()


# ---- the product columns, the production route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,usable", [(4, 0), (4, 10), (8, 0), (8, 250)])
def test_product_columns_block_by_block(env, k, usable):
    """vdb_permutation_product_range_dev over blocks of columns, vdb_permutation_chain_dev over all sets: api.permutation_product and the
    oracle's, bit for bit; two ranges chained separately and joined with vdb_poly_scale_dev (the sharded join) give the single chain"""
    lib, api, check, O = env["lib"], env["api"], env["check"], env["O"]
    n, chunk, n_sets = 1 << k, 3, 3
    rng = np.random.default_rng(50 + k + usable)
    seen = Seen()
    cols, sigma = mixed(rng, seen, "cols", N_COLS, n), mixed(rng, seen, "sigma", N_COLS, n)
    beta, gamma = O.random_fr(rng, 2)
    want = O.permutation_product(cols, sigma, usable, chunk, beta, gamma)
    assert np.array_equal(api.permutation_product(cols, sigma, usable, chunk, beta, gamma), want)
    dev = Dev(api)
    try:
        bc, bs = dev.put(cols), dev.put(sigma)
        args = (k, sz(usable), sz(chunk), api._p(beta), api._p(gamma), api._p(env["delta"]))
        for blocks in (((0, 3), (3, 7)), ((0, 6), (6, 7))):
            bz = dev.put(np.full((n_sets, n, 4), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64))
            for lo, hi in blocks:
                check(lib.vdb_permutation_product_range_dev(at(bc, lo * n), at(bs, lo * n), sz(hi - lo), sz(lo), *args, at(bz, lo // chunk * n)))
            separate = bz.download((n_sets, n, 4))
            check(lib.vdb_permutation_chain_dev(bz.ptr, sz(n_sets), k, sz(usable)))
            assert np.array_equal(bz.download((n_sets, n, 4)), want), blocks
            # the sharded join: sets [0, 2) and [2, 3) chained on their own, the second range scaled by the first one's last product
            bz.upload(separate)
            check(lib.vdb_permutation_chain_dev(bz.ptr, sz(2), k, sz(usable)))
            check(lib.vdb_permutation_chain_dev(at(bz, 2 * n), sz(1), k, sz(usable)))
            end = bz.download((n_sets, n, 4))[1, usable].copy()
            check(lib.vdb_poly_scale_dev(at(bz, 2 * n), api._p(end), sz(n)))
            assert np.array_equal(bz.download((n_sets, n, 4)), want), blocks
            assert lib.vdb_permutation_product_range_dev(at(bc, 4 * n), at(bs, 4 * n), sz(3), sz(4), *args, at(bz, n)) == -3      # not a chunk boundary
            assert np.array_equal(bz.download((n_sets, n, 4)), want)
    finally:
        dev.free()


def test_chain_of_more_sets_than_lanes(env):
    """vdb_permutation_chain_dev with 1027 sets of 8 rows — more than the one workgroup of k_chain_factors has lanes —, a zero end value
    in set 500: every later set is zero up to the last usable row"""
    lib, api, check, O = env["lib"], env["api"], env["check"], env["O"]
    n_sets, k, usable = 1027, 3, 5
    n = 1 << k
    z = O.random_fr(np.random.default_rng(1027), n_sets * n).reshape(n_sets, n, 4)
    z[500, usable] = 0
    vals = [O.fr_to_ints(c) for c in z]
    f, want = 1, []
    for c in range(n_sets):
        want.append([v * f % R if row <= usable else v for row, v in enumerate(vals[c])])
        f = f * vals[c][usable] % R
    want = np.stack([O.fr_from_ints(c) for c in want])
    assert not want[501:, : usable + 1].any() and want[500, :usable].all() and np.array_equal(want[501:, usable + 1:], z[501:, usable + 1:])
    dev = Dev(api)
    try:
        bz = dev.put(z)
        check(lib.vdb_permutation_chain_dev(bz.ptr, sz(n_sets), k, sz(usable)))
        assert np.array_equal(bz.download((n_sets, n, 4)), want)
    finally:
        dev.free()


