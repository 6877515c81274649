"""The MSM driver's planner — msm_window and msm_plan of halo2_vectordb_amd/csrc/msm_plan.hpp, what vdb_srs_load_window shapes a table
with and msm_batch_dev (msm.hip) plans every job with — on the host, through `tools/msm_plan_probe.hip --host`, held with no tolerance
to tests/msm_plan_model.py, and what the kernels rely on stated on the model the probe has been held to:

  probe == model   every field of every plan and every refusal with its code and message, over the product of: windows c 2..14, given
                   and through the VDB_MSM_C knob; k 1..24 and the first k whose table index leaves 31 bits; columns of 1, 2, 3,
                   2^k - 37, 2^k - 1 and 2^k scalars; 1, 2, 7, 600, 8,146, 20,000 and 2^20 columns; 0, 1, 8 GiB - 1, 16 GiB and
                   200 GiB free, nothing or 1 GiB held, no cap, a cap of one byte and of 4 GiB; the default windows, knob values outside
                   2..14, and shapes no table has, for the planner's own refusals
  layout           the ten regions in order, disjoint, aligned to their elements and inside the buffer
  batches          1 <= nb <= min(n_cols, 16384); segment and range capacities of a batch below 2^31
  sort and scatter lcap a power of two in [32, 256]; fine_bits 0 or in [2, c - 1], non-zero only from c = 13, sharing 31 bits with the
                   table index; LDS within 160 KiB (the sort) and 64 KiB (the second scatter); the combine pass count
  the benchmark    the k-means job goes through in one batch"""
import pytest

import l9_model as L
import msm_plan_model as M

GIB = M.GIB
CS = range(2, 15)
N_COLS = (1, 2, 7, 600, 8146, 20000, 1 << 20)
MEMS = [M.Mem(f, h, c) for f in (0, 1, 8 * GIB - 1, 16 * GIB, 200 * GIB) for h in (0, GIB) for c in (0, 1, 4 * GIB)]
NAMES = ["msm_plan by window", "msm_plan by shape"]

# shapes msm_window never gives, for what msm_plan itself refuses (and two it accepts beside them)
HUGE = M.Shape(13, 20, 1 << 12, 1 << 40)
SHAPE_CASES = [
    ("msm: a kernel needs more than 160 KiB of LDS", M.Shape(15, 17, 1 << 14, 1 << 10), 4, 1 << 10),
    ("msm: table index and fine bucket number do not fit an entry's 31 bits", HUGE, 4, 1 << 10),
    ("msm: the job does not fit the loaded table", M.Shape(11, 24, 1 << 10, 1 << 10), 0, 1 << 10),
    ("msm: the job does not fit the loaded table", M.Shape(11, 24, 1 << 10, 1 << 10), 4, 0),
    ("msm: the job does not fit the loaded table", M.Shape(11, 24, 1 << 10, 1 << 10), 4, (1 << 10) + 1),
    ("msm: the job does not fit the loaded table", HUGE, 0, 1),                     # the first refusal in the planner's order
    ("", M.Shape(11, 24, 1 << 10, 1 << 10), 4, 1 << 10),
    ("", M.Shape(14, 19, 1 << 13, 1 << 26), 4, 1 << 26),                            # fine_bits cut from 5 to 0 by a 31-bit table index
]


def ks(c):
    """1..24 and the first k at which the table index of this window does not fit 31 bits"""
    W = (254 + c - 1) // c
    first_bad = next(k for k in range(1, 40) if W << k > 0x7FFFFFFF)
    assert first_bad > 24
    return list(range(1, 25)) + [first_bad]


def ns(k):
    return sorted({v for v in (1, 2, 3, (1 << k) - 37, (1 << k) - 1, 1 << k) if 1 <= v <= 1 << k})


def product_block(knob, window_bits, k_list):
    cases = [((k, window_bits, n, nc, mem), M.case_words(k, window_bits, n, nc, mem))
             for k in k_list for n in ns(k) for nc in N_COLS for mem in MEMS]
    return L.Block(0, knob, cases, nin=M.NIN, names=NAMES)


def gen():
    """-> blocks; a case's tag is its inputs"""
    blocks = [product_block(0, c, ks(c)) for c in CS]                       # the window given, the knob unset
    blocks += [product_block(c, 0, ks(c)) for c in CS]                      # the window from the knob
    # the default windows (8 up to k = 8, then 11), knob values that are ignored, a given window beside a knob, a refused window
    for knob in (0, 1, 15, 7):
        cases = [((k, wb, n, 7, M.Mem(16 * GIB)), M.case_words(k, wb, n, 7, M.Mem(16 * GIB)))
                 for k in range(1, 27) for wb in (0, 9, 1, 15) for n in ns(k)[-2:]]
        blocks.append(L.Block(0, knob, cases, nin=M.NIN, names=NAMES))
    blocks.append(L.Block(1, 0, [((why, s, nc, n), M.shape_case_words(s, n, nc, M.Mem(16 * GIB))) for why, s, nc, n in SHAPE_CASES], nin=M.NIN, names=NAMES))
    return blocks


def model_answer(b, tag):
    """-> (msm_window's rc, why, shape, plan or None) for a case"""
    if b.op == 1:
        why, s, nc, n = tag
        return M.OK, "", s, M.plan(s, nc, n, M.Mem(16 * GIB))
    k, wb, n, nc, mem = tag
    rc, why, s = M.window(k, wb, b.mod)
    return rc, why, s, (M.plan(s, nc, n, mem) if rc == M.OK else None)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """-> [(block, tag, msm_window's rc and why, shape, model plan or None)], after the probe's words have been held to the model's for
    every one of them (one run of the probe per block: a block's results are compared and dropped)"""
    d = tmp_path_factory.mktemp("msm_plan")
    exe = L.compile_probe(d, "msm_plan_probe")
    out = []
    for b in gen():
        (res,) = L.run_probe(exe, "--host", [b], d, 600, [M.NOUT, M.NOUT], NAMES, M.MAGIC)
        for (tag, _), got in zip(b.cases, res):
            rc, why, s, P = model_answer(b, tag)
            assert got == M.expect_words(rc, why, s, P), (b.op, b.mod, tag)
            out.append((b, tag, rc, why, s, P))
    return out


@pytest.fixture(scope="module")
def ok(plans):
    """the distinct plans (the 30 states of the memory are six budgets, and the knob's windows are the given ones), each with the first
    case that asked for it"""
    first = {}
    for _, tag, rc, _, _, P in plans:
        if rc == M.OK and P.rc == M.OK:
            first.setdefault(id(P), (tag, P))
    return list(first.values())


def test_probe_equals_model(plans, ok):
    planned = sum(rc == M.OK and P.rc == M.OK for _, _, rc, _, _, P in plans)
    print("cases", len(plans), "planned", planned, "distinct plans", len(ok))
    # 26 blocks of the product: 141 (k, n) pairs, 135 of them planned, times 7 column counts and 30 states of the memory
    assert len(plans) > 26 * 141 * 210 and planned > 26 * 135 * 210 and len(ok) > 13 * 135 * 7 * 6
    by_window = {(b.mod, tag[1]): s.c for b, tag, rc, _, s, _ in plans if b.op == 0 and rc == M.OK}
    assert {c for (knob, wb), c in by_window.items() if knob == 0 and wb} == set(CS)             # given
    assert {c for (knob, wb), c in by_window.items() if wb == 0 and knob in CS} == set(CS)       # from the knob
    assert by_window[7, 9] == 9 and by_window[7, 0] == 7                                         # a given window goes before the knob
    for b, tag, rc, _, s, _ in plans:
        if b.op == 0 and rc == M.OK:
            assert (s.W, s.B, s.table_n) == (-(-254 // s.c), 1 << (s.c - 1), 1 << tag[0])
            if tag[1] == 0 and b.mod not in CS:
                assert s.c == (8 if tag[0] <= 8 else 11)                                         # no knob, or one outside 2..14


def test_every_refusal_with_its_code_and_message(plans):
    seen = {}
    for b, tag, rc, why, s, P in plans:
        if rc != M.OK or P.rc != M.OK:
            assert (rc if rc != M.OK else P.rc) == M.REFUSED == -3
            seen.setdefault(why if rc != M.OK else P.why, []).append((b.op, tag))
    assert set(seen) == {"window_bits must be 0 (default) or 2..14", "srs: table index does not fit 31 bits"} | {w for w, *_ in SHAPE_CASES if w}
    # a table index above 31 bits is refused at exactly the first such k of every window; no shape msm_window gives is refused by msm_plan
    bad = {(tag[1], tag[0]) for _, tag in seen["srs: table index does not fit 31 bits"] if tag[1] in CS}
    assert bad == {(c, ks(c)[-1]) for c in CS}
    assert all(op == 1 for w, *_ in SHAPE_CASES if w for op, _ in seen[w])
    assert {tag[1] for _, tag in seen["window_bits must be 0 (default) or 2..14"]} == {1, 15}


def test_regions_are_disjoint_aligned_and_inside(ok):
    worst_pad = 0
    for tag, P in ok:
        at = 0
        for name in M.REGIONS:
            off = P.off[name]
            assert off >= at and off % M.ALIGN[name] == 0, (tag, name)                            # in order, after the one before, aligned
            assert off - at < M.ALIGN[name]
            at = off + P.region_bytes(name)
        assert at == P.end <= P.bytes, tag
        # the old sum: a column's bytes times the batch, the counters, and what is left of the 512 for padding
        pad = P.end - P.nb * P.per_col - 4 * M.COUNTER_WORDS
        assert 0 <= pad <= M.SLACK - 4 * M.COUNTER_WORDS
        worst_pad = max(worst_pad, pad)
    print("largest padding", worst_pad, "of", M.SLACK - 4 * M.COUNTER_WORDS)
    assert 0 < worst_pad <= 15 + 7


def test_raw_is_aligned_where_the_entries_end_off_a_16_byte_boundary():
    rc, _, s = M.window(3, 7)
    assert rc == M.OK and (s.c, s.W) == (7, 37)
    P = M.plan(s, 1, 1)
    assert P.nb == 1 and P.region_bytes("entries") == 148 and P.off["raw"] == 160 and P.off["raw"] % 16 == 0
    P = M.plan(s, 1, 3)
    assert P.region_bytes("entries") == 444 and P.off["raw"] == 448


def test_batches_and_capacities(ok):
    many = 0
    for tag, P in ok:
        assert 1 <= P.nb <= min(P.n_cols, 16384), tag
        assert P.nb * P.seg_cap_col == P.seg_cap < 1 << 31 and P.nb * P.range_cap_col == P.range_cap < 1 << 31, tag
        assert P.range_cap_col < P.seg_cap_col                                                    # why bounding the segments bounds the ranges
        assert P.n_batches == -(-P.n_cols // P.nb) and (P.n_batches - 1) * P.nb < P.n_cols
        many += P.n_batches > 1
    assert many > 1000


def test_sort_and_scatter_parameters(ok):
    two_phase = set()
    for tag, P in ok:
        c, W, B, table_n = P.shape
        assert P.lcap in (32, 64, 128, 256), tag
        assert P.ent_cap == P.n * W and P.range_cap_col == -(-P.ent_cap // P.lcap) and P.seg_cap_col == B + P.range_cap_col
        assert 1 << P.idx_bits >= W * table_n and (P.idx_bits == 1 or 1 << (P.idx_bits - 1) < W * table_n)
        assert P.fine_bits == 0 or 2 <= P.fine_bits <= c - 1, tag
        assert P.fine_bits == 0 or c >= 13
        assert P.fine_bits + P.idx_bits <= 31, tag
        assert P.sort_lds == (3 * B + 32) * 4 <= 160 * 1024
        assert P.scatter2_lds == ((P.bin_cap + (1 << P.fine_bits)) * 4 if P.fine_bits else 0) and P.scatter2_lds <= 64 * 1024
        assert P.bin_cap == 6 * 1024 and P.scatter2_bins_x == (min(B >> P.fine_bits, 64) if P.fine_bits else 0)
        assert (1 << P.combine_passes) >= P.range_cap_col + 1 > (1 << P.combine_passes) // 2      # ceil(log2(range_cap_col + 1))
        if P.fine_bits:
            two_phase.add((c, P.fine_bits))
    assert {c for c, _ in two_phase} == {13, 14} and (13, 4) in two_phase and (14, 5) in two_phase and len(two_phase) > 2
    assert max(P.sort_lds for _, P in ok) == 98432                                                # c = 14
    # the prover's window: 12 KB, what lets two workgroups of k_msm_sort share a CU
    assert {P.sort_lds for _, P in ok if P.shape.c == 11} == {12416}


def test_the_benchmark_job_is_one_batch(plans):
    rc, _, s = M.window(16, 11)
    tag = (16, 11, 1 << 16, 8146, M.Mem(200 * GIB, 0, 0))
    assert any(b.op == 0 and b.mod == 0 and t == tag for b, t, *_ in plans)                       # the probe has answered this job
    P = M.plan(s, 8146, 1 << 16, M.Mem(200 * GIB))
    assert rc == M.OK and P.rc == M.OK and (P.nb, P.n_batches, P.lcap, P.combine_passes) == (8146, 1, 256, 13)
    assert P.bytes == 67800983216                                                                 # 67.8 GB
