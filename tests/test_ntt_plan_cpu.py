"""The NTT driver's planner — ntt_plan and NttPlan::chunk_cols of halo2_vectordb_amd/csrc/ntt_plan.hpp, what ntt_dev (ntt.hip) plans every
transform with — on the host, through `tools/ntt_plan_probe.hip --host`, held with no tolerance to tests/ntt_plan_model.py, and what the
kernels rely on stated on the model the probe has been held to:

  probe == model   every field of every plan, and every refusal with its code and message, over log_n 1..26, the input lengths n, n/2,
                   n/4, n/8 and 1, max_s 4..9 (and values outside), the 16 settings of shoup / spec / shoup_all / blk0, 0, 1, 3 and 4
                   virtual slots and the flag combinations of the entry points of ntt.hip
  safe schedule    every limb bound that enters a product is below 6.1 units of 2^29, no bound reaches 8, no carry pass in front of
                   the step at stage 0, and no comparison of the walk lies within 1e-9 of its threshold (so the header's doubles and the
                   model's fractions take the same branches)
  fast kernels     the prover's sizes plan the specialised instantiations
  SA shapes        an SA instantiation is only ever planned with the shape and Shoup table its template constants say
  LDS, chunking    at most 55,332 B of dynamic LDS (so no launch needs a raised limit); chunks are whole groups of virtual columns
                   within 2 GiB of scratch — but for 3 or 4 slots at 2^25 and 2^26, where one group alone is larger and is the chunk
                   (no entry point takes slots above 2^24)"""
import itertools

import pytest

import l9_model as L
import ntt_plan_model as M

KNOBS = [M.Knobs(ms, sh, sp, sa, b0) for ms in range(4, 10) for sh, sp, sa, b0 in itertools.product((True, False), repeat=4)]
ODD_KNOBS = [M.Knobs(max_s=ms) for ms in (0, 3, 10, 255)]
LOGS = range(1, 27)

REFUSALS = [
    ("ntt: log_n > 26 unsupported", M.Job(27, in_place=True)),
    ("ntt: log_n > 26 unsupported", M.Job(31, in_len=5, vslots=9)),
    ("ntt: in-place transform needs in_len == n", M.Job(12, in_len=1 << 10, in_place=True)),
    ("ntt: in-place transform needs in_len == n", M.Job(12, in_len=1 << 10, in_place=True, vslots=2, has_srcs=True)),
    ("ntt: virtual columns need an output buffer and their input tables", M.Job(12, vslots=2, has_in_tabs=True, in_place=True)),
    ("ntt: virtual columns need an output buffer and their input tables", M.Job(12, vslots=2)),
    ("ntt: virtual columns need an output buffer and their input tables", M.Job(12, n_cols=10, vslots=5, has_in_tabs=True)),
    ("ntt: virtual columns need an output buffer and their input tables", M.Job(12, vslots=2, has_in_tabs=True, has_srcs=True)),
    ("ntt: virtual columns need an output buffer and their input tables", M.Job(12, vslots=2, has_in_tabs=True, coset_in=True)),
    ("ntt: virtual columns need an output buffer and their input tables", M.Job(12, n_cols=7, vslots=2, has_in_tabs=True)),
    ("ntt: column sources need an output buffer and a multi-pass size", M.Job(12, has_srcs=True, in_place=True)),
    ("ntt: column sources need an output buffer and a multi-pass size", M.Job(12, has_srcs=True, in_len=1 << 11)),
    ("ntt: column sources need an output buffer and a multi-pass size", M.Job(10, has_srcs=True)),
]


def gen():
    blocks = []
    for kn in KNOBS + ODD_KNOBS:
        cases = [(f"2^{k} {tag}", M.job_words(j)) for k in LOGS for tag, j in M.caller_jobs(k)]
        if kn == M.Knobs():
            cases += [(f"refusal: {why}", M.job_words(j)) for why, j in REFUSALS]
            cases += [(f"2^{k} chunking, {nc} columns", M.job_words(M.Job(k, n_cols=nc, vslots=v, has_in_tabs=v > 0)))
                      for k in LOGS for v in (0, 1, 3, 4) for nc in (12, 60, 600, 12 << 16)]
        blocks.append(L.Block(0, M.knob_word(kn), cases, nin=[M.NIN], names=["ntt_plan"]))
    return blocks


def job_of(words):
    f = words[6]
    return M.Job(words[0], words[1] | words[2] << 32, words[3] | words[4] << 32, words[5], *[bool(f >> i & 1) for i in range(7)])


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """-> [(knobs, tag, job, model plan)], after the probe's words have been held to the model's for every one of them"""
    d = tmp_path_factory.mktemp("ntt_plan")
    exe = L.compile_probe(d, "ntt_plan_probe")
    blocks = gen()
    results = L.run_probe(exe, "--host", blocks, d, 600, [M.NOUT], ["ntt_plan"], M.MAGIC)
    out = []
    for kn, b, res in zip(KNOBS + ODD_KNOBS, blocks, results):
        assert b.mod == M.knob_word(kn)
        for (tag, w), got in zip(b.cases, res):
            j = job_of(w)
            P = M.plan(j, kn)
            assert got == M.expect_words(P), (kn, tag, j, got, M.expect_words(P))
            out.append((kn, tag, j, P))
    return out


def test_probe_equals_model(plans):
    ok = [P for _, _, _, P in plans if P.rc == M.OK]
    kernels = {p["kernel"] for P in ok for p in P.passes}
    print("plans", len(plans), "refused", len(plans) - len(ok), "instantiations planned", len(kernels))
    assert len(plans) > 90000 and {P.L for P in ok} == {1, 2, 3, 4}
    assert kernels == {name for name, _ in M.KERNELS}                     # every line of the driver's switch is reached
    assert {P.job.vslots for P in ok} == {0, 1, 3, 4}
    assert M.CKP == L.offset_limbs(14, L.R) and float(M.CMAX) == pytest.approx(1.58929, abs=1e-5)


def test_every_refusal_with_its_code_and_message(plans):
    seen = {}
    for kn, tag, j, P in plans:
        if P.rc != M.OK:
            assert P.rc == M.REFUSED == -3
            seen.setdefault(P.why, []).append(tag)
    for why, j in REFUSALS:
        assert M.plan(j).why == why and any(t == f"refusal: {why}" for t in seen[why]), why
    # three refusals no job reaches, and none can be provoked through ntt_plan: the carry pass in front of the step at stage 0 and the SA
    # plan that does not match its instantiation (the schedule and the LDS plan never ask for them: test_schedule_is_safe,
    # test_specialised_kernels_get_their_constants) and a pass above 64 KiB of LDS (test_lds_and_chunking)
    assert set(seen) == {why for why, _ in REFUSALS}
    # what the callers ask for at sizes the driver refuses: column sources at single-pass sizes and short inputs, nothing else
    for why, tags in seen.items():
        for t in tags:
            assert t.startswith("refusal:") or ("lagrange_to_coeff_src" in t and "column sources" in why), (why, t)


def test_schedule_is_safe(plans):
    worst_product = worst = 0
    closest = 1
    shapes = set()
    for _, tag, j, P in plans:
        for p in P.passes:
            w = p["walk"]
            shapes.add((p["S"], p["s0"]))
            fed = list(w.products)
            if p["out_mul"]:
                closest = min(closest, abs(w.final - M.PRODUCT_MAX))
                fed.append(M.RENORMED if p["ren_out"] else w.final)
            assert all(x < M.PRODUCT_MAX for x in fed), (tag, p)
            assert all(x < 8 for x in w.bounds + (w.final,)), (tag, p)
            assert not (p["s0"] == 0 and p["ren_mask"] & 1), (tag, p)
            worst_product = max([worst_product] + fed)
            worst = max((worst,) + w.bounds)
            closest = min((closest,) + w.margins)
    print("pass shapes", len(shapes), "worst product operand", float(worst_product), "worst bound", float(worst), "closest comparison",
          float(closest))
    assert {(s, 0) for s in range(1, 11)} <= shapes and {(s, 2) for s in range(4, 10)} <= shapes
    assert worst == M.RENORMED + 4 * M.CMAX and float(worst) == pytest.approx(7.357, abs=1e-3)
    assert closest > 1e-9


def kernels_of(log_n, kn=M.Knobs(), **kw):
    P = M.plan(M.Job(log_n, **kw), kn)
    assert P.rc == M.OK
    return [p["kernel"] for p in P.passes]


def test_fast_kernels_are_chosen(plans):
    planned = {(kn, j): P for kn, _, j, P in plans}
    inv = dict(in_place=True, scale_ninv=True)
    ext = dict(in_len=1 << 16, coset_in=True)
    # every job below is one the probe has answered
    for kn in (M.Knobs(), M.Knobs(shoup_all=False), M.Knobs(spec=False)):
        for j in [M.Job(k, n_cols=12, **inv) for k in (16, 17, 18)] + [M.Job(18, n_cols=12, **ext)]:
            assert (kn, j) in planned
    assert kernels_of(16, n_cols=12, **inv) == ["256_SA", "LAST_256_SA"]
    assert kernels_of(17, n_cols=12, **inv) == ["512_SA", "LAST_256_SA"]
    assert kernels_of(18, n_cols=12, **inv) == ["512_SA", "LAST_512_SA"]
    assert kernels_of(18, n_cols=12, **ext) == ["512_PAD_SA", "LAST_512_SA"]
    no_sa = M.Knobs(shoup_all=False)
    assert kernels_of(16, no_sa, **inv) == ["256", "LAST_256"]
    assert kernels_of(17, no_sa, **inv) == ["512", "LAST_256"]
    assert kernels_of(18, no_sa, **inv) == ["512", "LAST_512"]
    assert kernels_of(18, no_sa, **ext) == ["512_PAD", "LAST_512"]
    for k, kw in ((16, inv), (17, inv), (18, inv), (18, ext)):
        assert kernels_of(k, M.Knobs(spec=False), **kw) == ["GENERIC", "LAST"]
    assert (M.Knobs(), M.Job(16, in_len=1 << 16, n_cols=12, vslots=3, has_in_tabs=True)) in planned
    assert kernels_of(16, n_cols=12, vslots=3, has_in_tabs=True) == ["VS_256", "LAST_256_SA"]
    # the template constants of the names above
    shape = dict(M.KERNELS)
    assert shape["256_SA"] == (0, 0, 8, 0, 4, 1) and shape["LAST_256_SA"] == (1, 0, 8, 0, 4, 1)
    assert shape["512_SA"] == (0, 0, 9, 0, 20, 1) and shape["LAST_512_SA"] == (1, 0, 9, 0, 20, 1)
    assert shape["512_PAD_SA"] == (0, 0, 9, 2, 4, 1) and shape["VS_256"] == (0, 1, 8, 0, 4, 0)


def test_specialised_kernels_get_their_constants(plans):
    shape = dict(M.KERNELS)
    sa_shapes = set()
    for kn, tag, j, P in plans:
        for l, p in enumerate(P.passes):
            last, vs, cs, cs0, cren, sa = shape[p["kernel"]]
            assert last == p["last"] and vs == (l == 0 and j.vslots > 0) and sa == p["sa"], (tag, p)
            if not cs:
                continue
            # a specialised instantiation reads none of these from its argument: they have to be what it was compiled with
            rl = M.spec_sh_res_log(cs, sa)
            assert (p["S"], p["s0"], p["ren_mask"], p["logG"], p["blk0"]) == (cs, cs0, cren, 10 - cs, 1), (tag, p)
            assert p["has_sh_tab"] and (p["sh_res_log"], p["sh_ns"], p["sh_max_s"]) == (rl, (1 << (cs - 1)) >> rl, cs - 2 - rl), (tag, p)
            if sa:
                sa_shapes.add((cs, cs0, cren))
                assert p["needs_sh2_tab"] == (cs == 9) and p["needs_tw_rec"] == (not last) and j.log_n <= 22
    assert sa_shapes == {(8, 0, 4), (9, 0, 20), (9, 2, 4)}


def test_lds_and_chunking(plans):
    single = multi = groups_over = slots_at_24 = 0
    for kn, tag, j, P in plans:
        if P.rc != M.OK:
            continue
        for p in P.passes:
            if P.L == 1:
                single = max(single, p["lds_bytes"])
            else:
                multi = max(multi, p["lds_bytes"])
        chunk = P.chunk_cols(j.n_cols)
        assert chunk >= 1 and (P.L == 1 or chunk <= max(j.n_cols, j.vslots))
        if j.vslots:
            assert chunk % j.vslots == 0
        col = 32 << j.log_n
        assert col <= 2 << 30                       # one column always fits (log_n <= 26)
        if P.L > 1 and j.vslots * col > 2 << 30:
            # the one exception: a single group of virtual columns is larger than 2 GiB and the chunk is that group.  No entry point
            # asks for it: vdb_coeff_to_cosets_dev, the only caller with slots, takes k <= 24
            assert j.log_n >= 25 and j.vslots >= 3 and chunk == j.vslots, (tag, chunk)
            groups_over += 1
        elif P.L > 1:
            assert chunk * col <= 2 << 30, (tag, chunk)
            slots_at_24 += j.vslots > 0 and j.log_n == 24
    print("largest dynamic LDS: single pass", single, "multi-pass", multi, "groups above 2 GiB", groups_over)
    assert groups_over > 0 and slots_at_24 > 0
    assert single == 55332 and multi == 50832       # below 64 KiB: no launch needs hipFuncAttributeMaxDynamicSharedMemorySize
