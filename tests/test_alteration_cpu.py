"""Every cell of every circuit the project proves, altered alone, on the host-built constraint maps and the oracle's witnesses
(no GPU).  The suite shows elsewhere that the maps accept every honest witness; here tests/alteration_model.py asks the opposite
question of each map: which cells could a prover replace without one gate, copy, constant, lookup or public value noticing?  For
each circuit: (a) the honest witness violates nothing, (b) every unnoticed cell is free in the reference's circuit too — today
that is the inverse witness of an is_zero whose operand is zero, and nothing else —, (c) such cells are at most 1 % of the circuit
(the reference alone stays at 0.2 .. 0.6 % on inputs like these: uniform vectors with one pair of equal elements, no zero vector),
(d) every lookup cell altered alone is noticed.  Where a whole-circuit trace and a block-built map exist, both are swept and must
leave the same cells free.  The model's verdicts are themselves held against a recount of the altered witness on samples of both
kinds of cell.  Each sweep prints one line: cells, unnoticed cells and their share, the reasons with counts."""
import re

import numpy as np
import pytest

import alteration_model as AM
import topk_model as TM
from halo2_vectordb_amd import circuit_sym as CS
from test_circuit_sym_cpu import to_ints
from test_gpu_fp_ops import BINARY, UNARY
from test_merkle_map_cpu import mark_constants, merkle_spans, oracle_merkle
from test_merkle_update_cpu import fetchers, kernel_like_flags, model as update_model
from test_topk_cpu import separated_inputs

CAP = 0.01


def sweep(name, cm, vals, lk, public, L, flags=None):
    """(a) .. (d) on one map and one witness; -> the unnoticed cells"""
    vals, lk, public = np.asarray(vals, dtype=object), np.asarray(lk, dtype=object), [int(c) for c in public]
    assert cm.n_cells == len(vals) and len(cm.lookup_src) == len(lk), name
    if flags is not None:
        assert np.array_equal(np.asarray(flags, dtype=np.uint8) & 1, np.asarray(cm.gate, dtype=np.uint8)), name
    inst = [vals[c] for c in public]
    honest = AM.recount(cm, vals, lk, L, public, inst)
    assert AM.violations(honest) == 0, (name, honest)                                   # (a)
    free = AM.unnoticed(cm, vals, lk, public)
    reasons = [AM.explain(cm, vals, c) for c in free]
    print(AM.summary(name, cm, free, reasons))
    unexplained = [c for c, r in zip(free, reasons) if r is None]
    assert not unexplained, f"{name}: cells {unexplained[:8]} ({len(unexplained)} in all) are tied to nothing and no gate notices them"   # (b)
    assert len(free) <= CAP * cm.n_cells, (name, len(free), cm.n_cells)                  # (c)
    assert AM.unnoticed_lookups(cm, lk) == [], name                                      # (d)
    # the model's verdicts against a recount of the altered witness, on seeded samples: lookup cells, free cells, bound cells
    rng = np.random.default_rng(cm.n_cells)
    for j in rng.choice(len(lk), size=min(8, len(lk)), replace=False).tolist():
        alt = lk.copy()
        alt[j] = (alt[j] + 1) % AM.R
        assert AM.recount(cm, vals, alt, L, public, inst, touched=([], [j]))["lookup_copies_unequal"] == 1, (name, j)
    is_free = np.zeros(cm.n_cells, dtype=bool)
    is_free[free] = True
    bound = np.flatnonzero(~is_free)
    sample = [(c, 0) for c in rng.choice(free, size=min(16, len(free)), replace=False).tolist()] if free else []
    sample += [(c, 1) for c in rng.choice(bound, size=min(48, len(bound)), replace=False).tolist()]
    for i, (c, want) in enumerate(sample):
        alt = vals.copy()
        alt[c] = (alt[c] + 1) % AM.R if i % 2 else int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) % AM.R
        if alt[c] == vals[c]:
            continue
        rep = AM.recount(cm, alt, lk, L, public, inst, touched=([c], []))
        assert (AM.violations(rep) >= 1) == bool(want), (name, c, want, rep)
        if i < 4:
            assert rep == AM.recount(cm, alt, lk, L, public, inst), (name, c)             # the short recount is the whole one
    return free


def both_forms(name, traced, built, vals, lk, L, flags=None):
    """a whole-circuit trace and a block-built map, (map, public cells) each: the same cells stay free"""
    a = sweep(name + " traced", traced[0], vals, lk, traced[1], L, flags)
    b = sweep(name + " built", built[0], vals, lk, built[1], L, flags)
    assert a == b, name


def flat(cells):
    return [int(c) for c in np.asarray(cells).reshape(-1)]


def uniform_pair(rng, shape, lo, hi, equal=True):
    """uniform rows with one pair of equal elements (the first two rows agree in place 0)"""
    v = rng.uniform(lo, hi, size=shape)
    if equal and shape[0] > 1:
        v[1, 0] = v[0, 0]
    return v


# ---------------------------------------------------------------------------------------------------------------- distances
@pytest.mark.parametrize("P,L", [(48, 11), (32, 9)])
@pytest.mark.parametrize("dim", [1, 2, 5])
@pytest.mark.parametrize("metric", ["euclidean", "cosine", "manhattan", "hamming"])
def test_distance(O, metric, dim, P, L):
    rng = np.random.default_rng([dim, L])
    # a and b agree in place 0 — except where that is the whole vector and the distance a square root: the reference's qsqrt(0)
    # violates its own asserted constants (tests/test_circuit_sym_cpu.py::test_sqrt_of_zero_violates_its_asserted_constant)
    v = uniform_pair(rng, (2, dim), -3.0, 3.0, equal=not (metric == "euclidean" and dim == 1))
    qa, qb = O.quantize(v[0], P), O.quantize(v[1], P)
    c = O.Ctx(store=True, keygen=True)
    c.assign_witnesses(qa)
    c.assign_witnesses(qb)
    c.distance(metric, qa, qb, P=P, L=L)
    assert c.err == 0
    cm, outs = CS.trace_distance(metric, dim, P, L)
    sweep(f"distance {metric} dim {dim} P {P} L {L}", cm, to_ints(O, c.advice()), to_ints(O, c.lookup()), outs, L, c.selectors())


# ---------------------------------------------------------------------------------------------------------------- fixed-point operations
def trace_binary(name, P, L):
    """x, y = two loaded witnesses, then one FixedPointInstructions call of two operands; public: x, y and the result.  The calls
    circuit_sym names are its own; qadd / qsub are the gate's add / sub (fixed_point.rs:213-239), qmax is qmin with the select's
    arms exchanged (:918-934) and qpow(x, e) = qexp(qmul(e, qlog(x))) (:441-456), as the oracle states them."""
    s = CS.Sym(P, L)
    x, y = s.assign_witnesses(2)
    call = dict(qadd=s.g_add, qsub=s.g_sub, qmul=s.qmul, qdiv=s.qdiv, qmin=s.qmin, bit_xor=s.bit_xor, cond_neg=s.cond_neg, qmod=s.qmod,
                qmax=lambda a, b: s.g_select(b, a, s.is_neg(s.g_sub(a, b))), qpow=lambda a, e: s.qexp(s.qmul(e, s.qlog(a))))[name]
    out = call(x, y)
    return CS._whole(s, 2), [x, y, out]


def operands(O, op, P):
    """two operand sets per operation: a generic one, and one at zero or one (one where zero is outside the domain)"""
    q = lambda v: O.quantize(np.asarray([v], dtype=np.float64), P)[0]
    bit = lambda v: O.fr_from_ints([v])[0]
    if op in ("qsqrt", "qlog2", "qlog"):
        return [(q(1.375), None), (q(1.0), None)]
    if op == "signed_div_scale":                                  # its operand is a product: twice the scale
        return [(O.fr_mul(q(1.375).reshape(1, 4), q(-2.25).reshape(1, 4))[0], None), (q(0.0), None)]
    if op in UNARY:
        return [(q(-2.25), None), (q(0.0), None)]
    if op == "bit_xor":
        # both pairs have xor = 0: with xor = 1 the closing is_equal has a zero operand, and its one free inverse is 2.6 % of this
        # circuit of 38 cells (the cap is stated for circuits of hundreds of cells and more).  The map does not depend on the
        # operands; with these, every one of its cells has to be noticed.
        return [(bit(1), bit(1)), (bit(0), bit(0))]
    if op == "cond_neg":
        return [(q(-2.25), bit(1)), (q(0.0), bit(0))]
    if op == "qpow":
        return [(q(1.375), q(-0.75)), (q(1.0), q(0.0))]
    if op in ("qdiv", "qmod"):                                    # the divisor is not zero
        return [(q(-2.25), q(0.625)), (q(0.0), q(1.0))]
    return [(q(-2.25), q(0.625)), (q(0.0), q(1.0))]


@pytest.mark.parametrize("op", UNARY + BINARY)
def test_fixed_point_operation(O, op):
    P, L = 48, 11
    cm, outs = CS.trace_fixed_point((op,), P, L) if op in UNARY else trace_binary(op, P, L)
    for i, (a, b) in enumerate(operands(O, op, P)):
        c = O.Ctx(store=True, keygen=True)
        c.assign_witnesses(np.stack([a] if b is None else [a, b]))
        res = c.op(op, a, b, P=P, L=L)
        assert c.err == 0, (op, i)
        vals = to_ints(O, c.advice())
        assert vals[outs[-1]] == to_ints(O, res)[0], (op, i)
        sweep(f"{op} operands {i}", cm, vals, to_ints(O, c.lookup()), outs, L, c.selectors())


# ---------------------------------------------------------------------------------------------------------------- nearest vector, batch, top-k
def oracle_queries(O, metric, queries, db, P, L):
    c = O.Ctx(store=True, keygen=True)
    c.assign_witnesses(queries)
    c.assign_witnesses(db)
    for qq in queries:
        c.nearest_vector(metric, qq, db, P=P, L=L)
    assert c.err == 0
    return to_ints(O, c.advice()), to_ints(O, c.lookup()), c.selectors()


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_nearest_with_a_tie(O, metric):
    n, dim, P, L = 5, 4, 48, 13
    # two equal database vectors, away from the query: their distances tie, the minimum is the first vector's alone.  (A tie AT the
    # minimum sets two indicators, and halo2-base's select_by_indicator assigns the last selected value, not the sum its gates
    # state: the reference's own witness violates its gates there, as the oracle's does.)
    v = uniform_pair(np.random.default_rng(54), (1 + n, dim), 0.25, 3.0)
    v[4] = v[2]
    v[0] = 1.01 * v[1] + np.linspace(0.01, 0.02, dim)
    qv = O.quantize(v, P)
    vals, lk, sel = oracle_queries(O, metric, qv[:1], qv[1:], P, L)
    (tm, (_i, tres)), (bm, (_j, bres)) = CS.trace_nearest(metric, n, dim, P, L), CS.build_nearest(metric, n, dim, P, L)
    both_forms(f"nearest {metric} n {n} dim {dim} L {L}", (tm, flat(tres)), (bm, flat(bres)), vals, lk, L, sel)


def test_batch_of_two_queries(O):
    metric, q, n, dim, P, L = "euclidean", 2, 5, 4, 48, 11
    qv = O.quantize(uniform_pair(np.random.default_rng(25), (q + n, dim), 0.25, 3.0), P)
    vals, lk, sel = oracle_queries(O, metric, qv[:q], qv[q:], P, L)
    (tm, (_i, tres)), (bm, (_j, bres)) = CS.trace_nearest_batch(metric, q, n, dim, P, L), CS.build_nearest_batch(metric, q, n, dim, P, L)
    both_forms(f"batch {metric} q {q} n {n} dim {dim} L {L}", (tm, flat(tres)), (bm, flat(bres)), vals, lk, L, sel)


def test_topk(O):
    metric, q, n, dim, topk, P, L = "euclidean", 2, 4, 3, 2, 48, 11
    qv = O.quantize(separated_inputs(metric, q, n, dim, topk, seed=21), P)
    m = TM.topk_model(O, metric, qv[:q], qv[q:], topk, P, L)
    vals, lk = to_ints(O, m["advice"]), to_ints(O, m["lookup"])
    (tm, (_i, tres)), (bm, (_j, bres)) = CS.trace_nearest_topk(metric, q, n, dim, topk, P, L), CS.build_nearest_topk(metric, q, n, dim, topk, P, L)
    both_forms(f"top-k {metric} q {q} n {n} dim {dim} t {topk} L {L}", (tm, flat(tres)), (bm, flat(bres)), vals, lk, L, m["selectors"])


def test_query_circuit_with_its_commitment(O):
    """build_nearest_topk(finish=False), then place_merkle, on the numpy builder, as tests/test_merkle_map_cpu.py assembles what
    TopKQueryHotPath.constraint_map(on_device=False) does; public: every result vector, then the root"""
    metric, q, n, dim, topk, P, L = "euclidean", 2, 3, 2, 2, 48, 11
    rng = np.random.default_rng(41)
    queries, db = O.quantize(rng.random((q, dim)) + 0.1, P), O.quantize(rng.random((n, dim)) + 0.1, P)
    m = TM.topk_model(O, metric, queries, db, topk, P, L, merkle=True)
    vals, sel = TM.to_ints(m["advice"]), m["selectors"].astype(np.uint8) & 1
    base = m["regions"]["merkle"]
    spans, _leaves, _zero, _levels, end = merkle_spans(n, dim, base)
    flags = sel.copy()
    mark_constants(vals, flags, spans)
    B, (_ind, res), used = CS.build_nearest_topk(metric, q, n, dim, topk, P, L, extra_cells=end - base, finish=False)
    root_cell, stop = CS.place_merkle(B, n, dim, used, q * dim, lambda lo, hi: flags[lo:hi], lambda lo, hi: vals[lo:hi])
    assert used == base and stop == end
    sweep(f"query circuit {metric} q {q} n {n} dim {dim} t {topk} L {L}", B.finish(), vals, TM.to_ints(m["lookup"]), flat(res) + [root_cell], L, sel)


# ---------------------------------------------------------------------------------------------------------------- k-means
def test_kmeans_cosine(O):
    """(Euclidean k-means does not satisfy its own asserts: tests/test_gpu_copymap.py::test_kmeans_cosine_is_satisfied_and_euclidean_is_not)"""
    metric, n, dim, K, I, P, L = "cosine", 5, 2, 2, 1, 48, 13
    qv = O.quantize(uniform_pair(np.random.default_rng(52), (n, dim), 0.05, 1.05), P)
    c = O.Ctx(store=True, keygen=True)
    c.assign_witnesses(qv)
    c.kmeans(metric, qv, K, I, P=P, L=L)
    assert c.err == 0
    (tm, (tcent, _i)), (bm, (bcent, _j)) = CS.trace_kmeans(metric, n, dim, K, I, P, L), CS.build_kmeans(metric, n, dim, K, I, P, L)
    both_forms(f"k-means {metric} n {n} dim {dim} K {K} I {I} L {L}", (tm, flat(tcent)), (bm, flat(bcent)), to_ints(O, c.advice()), to_ints(O, c.lookup()),
               L, c.selectors())


# ---------------------------------------------------------------------------------------------------------------- Merkle commitment, path updates
@pytest.mark.parametrize("n,dim", [(3, 3), (2, 4)])
def test_merkle_commitment(O, n, dim):
    """(3, 3): a padding leaf and a permutation that absorbs one word; (2, 4): a full sponge's padding-only permutation"""
    _db, vals, flags, _sel, _root = oracle_merkle(O, n, dim)
    cm, root_cell = CS.build_merkle(n, dim, lambda lo, hi: flags[lo:hi], lambda lo, hi: vals[lo:hi])
    sweep(f"merkle n {n} dim {dim}", cm, vals, [], [root_cell], 8, flags)


def test_merkle_update(O):
    n, dim, indices = 2, 3, [1]
    m, levels = update_model(O, n, dim, indices)
    depth, k = len(levels) - 1, len(indices)
    m["flags"] = kernel_like_flags(m, dim, depth, k)
    ff, fv, vals = fetchers(m)
    both_forms(f"merkle update n {n} dim {dim} m {k}", CS.trace_merkle_update(k, dim, depth, ff, fv), CS.build_merkle_update(k, dim, depth, ff, fv), vals, [], 8,
               m["flags"])


# ---------------------------------------------------------------------------------------------------------------- the check itself
def test_a_dropped_tie_is_found_and_named(O, monkeypatch):
    """is_zero without the copy of its operand into the second gate [0, a', z, 0]: wherever a != 0, z = 0 and a' is bound by nothing —
    the honest witness still passes, and the sweep names such cells instead of passing.  (The copy of z into that gate, dropped alone,
    is beyond a sweep of single cells: z' then sits beside a = 0 or is held by the cells that copy it.  The splice sweep finds it:
    tests/test_splice_cpu.py::test_a_dropped_copy_of_z_is_found_and_named.)"""
    def g_is_zero(self, a):
        z = self.push(None, True)
        self.push(a); self.push(None); self.push(CS.C(1))
        self.push(CS.C(0), True); self.push(None)                # (push(a) in the product)
        z2 = self.push(z)
        self.push(CS.C(0))
        return z2
    monkeypatch.setattr(CS.Sym, "g_is_zero", g_is_zero)
    P, L, dim = 48, 11, 2
    v = uniform_pair(np.random.default_rng(3), (2, dim), -3.0, 3.0)
    qa, qb = O.quantize(v[0], P), O.quantize(v[1], P)
    c = O.Ctx(store=True, keygen=True)
    c.assign_witnesses(qa)
    c.assign_witnesses(qb)
    c.distance("hamming", qa, qb, P=P, L=L)
    cm, outs = CS.trace_distance("hamming", dim, P, L)
    vals = to_ints(O, c.advice())
    with pytest.raises(AssertionError, match=r"cells \[\d+") as e:
        sweep("hamming without is_zero's second copy of its operand", cm, vals, to_ints(O, c.lookup()), outs, L, c.selectors())
    named = [int(x) for x in re.search(r"cells \[([\d, ]+)\]", str(e.value)).group(1).split(",")]
    assert all(cm.gate[x - 1] and vals[x + 1] == 0 and vals[x] != 0 for x in named)          # offset 1 of [0, a', 0, 0]
