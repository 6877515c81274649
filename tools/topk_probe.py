#!/usr/bin/env python3
"""What the t nearest vectors cost beside the nearest one, measured on the device (writes profiles/topk_query.json).
Method of tools/batch_query_probe.py: HIP events, warm, five alternating repeats, the spread recorded; per-kernel times and launch
counts from the library's own event profiler in a pass of their own.  Euclidean, 64 x 128, P = 48, L = 13, k = 14:

1. cells — vdb_wit_nearest_topk_size for t = 1 and 10 beside vdb_wit_nearest_size;
2. witness — vdb_wit_nearest_topk_dev for (q, t) in {(1, 1), (1, 10), (8, 10), (1, 64)} (the batch entry point is this call at
   t = 1: tools/batch_query_probe.py times it);
3. whole proof — TopKQueryHotPath(topk = 10) against QueryHotPath in one process, alternating, both verified: ms, proof bytes,
   column counts, prover stages.

    python tools/topk_probe.py [--out profiles/topk_query.json] [--skip-proof]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x1234567890ABCDEF1234567
METRIC, N, DIM, P, L, K = "euclidean", 64, 128, 48, 13, 14
REPEATS = 5


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), spread=max(xs) - min(xs), runs=xs)


def sizes(api):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    m = api.METRICS[METRIC]
    c, l = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.vdb_wit_nearest_size(m, P, L, N, DIM, ctypes.byref(c), ctypes.byref(l)))
    out = dict(nearest_vector=dict(cells=c.value, lookup_cells=l.value))
    for t in (1, 10, 64):
        check(lib.vdb_wit_nearest_topk_size(m, P, L, 1, N, DIM, t, ctypes.byref(c), ctypes.byref(l)))
        out[f"topk_{t}"] = dict(cells=c.value, lookup_cells=l.value)
    base = out["nearest_vector"]["cells"]
    out["cells_per_further_round"] = (out["topk_10"]["cells"] - base) // 9
    out["further_round_over_nearest_vector"] = out["cells_per_further_round"] / base
    out["topk_10_over_nearest_vector"] = out["topk_10"]["cells"] / base
    return out


def witness_probe(api, q, t):
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import sift_like_vectors
    lib = api.init()
    m = api.METRICS[METRIC]
    db, seed = sift_like_vectors(20260002, N, DIM)
    queries, _ = sift_like_vectors(seed + 1000, q, DIM)
    qq, qdb = api.quantize(queries, P), api.quantize(db, P)
    c, l = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.vdb_wit_nearest_topk_size(m, P, L, q, N, DIM, t, ctypes.byref(c), ctypes.byref(l)))
    cells, lks = c.value, l.value
    bufs = [api.DeviceBuffer(x) for x in (qq.nbytes, qdb.nbytes, cells * 32, lks * 32, q * t * N * 32, q * t * DIM * 32)]
    d_q, d_db, d_adv, d_lk, d_ind, d_res = bufs
    d_q.upload(qq)
    d_db.upload(qdb)

    def topk():
        check(lib.vdb_wit_nearest_topk_dev(m, P, L, d_q.ptr, d_db.ptr, q, N, DIM, t, d_adv.ptr, d_lk.ptr, None, d_ind.ptr, d_res.ptr))

    def timed(fn):
        api.sync()
        api.timer_start()
        fn()
        return api.timer_stop()

    try:
        topk()                                                             # warm
        times = [timed(topk) for _ in range(REPEATS)]
        api.sync()                                                         # per-kernel times and launch counts, a pass of its own
        api.profile_begin(deferred=True)
        topk()
        api.sync()
        kernels = api.profile_end()
        return dict(q=q, topk=t, cells=cells, lookup_cells=lks, topk_ms=stats(times), kernels_ms=dict(topk=kernels),
                    launches=int(sum(v["launches"] for v in kernels.values())),
                    stream_write_GBps=(cells + lks) * 32 / (float(np.median(times)) * 1e-3) / 1e9)
    finally:
        for x in bufs:
            x.free()


def proof_probe(api):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import QueryHotPath, TopKQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    hps, made = {}, {}
    for name, ctor in (("query", lambda: QueryHotPath(n=N, dim=DIM, k=K, P=P, L=L, metric=METRIC, tau=TAU)),
                       ("topk_10", lambda: TopKQueryHotPath(topk=10, q=1, n=N, dim=DIM, k=K, P=P, L=L, metric=METRIC, tau=TAU))):
        t0 = time.perf_counter()
        hp = ctor().setup()
        pr = ProverRounds(hp).keygen()
        hps[name] = (hp, pr, time.perf_counter() - t0)
    try:
        for name, (hp, pr, _s) in hps.items():
            out = pr.prove(None)                                           # warm
            ok = bool(verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"])))
            made[name] = dict(verified=ok, times=[], proof_bytes=len(out["proof"]), instances=len(out["instances"]))
        for _ in range(REPEATS):                                            # alternating
            for name, (hp, pr, _s) in hps.items():
                api.sync()
                t0 = time.perf_counter()
                pr.prove(None)
                api.sync()
                made[name]["times"].append((time.perf_counter() - t0) * 1e3)
        rep = {}
        for name, (hp, pr, setup_s) in hps.items():
            stages = {}
            pr.prove(None, timings=stages)
            rep[name] = dict(k=hp.k, lookup_bits=hp.L, cells=hp.n_cells, lookup_cells=hp.n_lookup, advice_columns=hp.n_adv_cols, lookup_columns=hp.n_lk_cols,
                             public_values=made[name]["instances"], setup_and_keygen_s=setup_s, proof_ms=stats(made[name]["times"]),
                             proof_bytes=made[name]["proof_bytes"], verified=made[name]["verified"], stage_ms=stages)
        a, b = rep["query"], rep["topk_10"]
        rep["proof_ms_ratio"] = b["proof_ms"]["median"] / a["proof_ms"]["median"]
        rep["cell_ratio"] = b["cells"] / a["cells"]
        rep["spread_ms"] = max(a["proof_ms"]["spread"], b["proof_ms"]["spread"])
        rep["stages_grown_ms"] = {s: b["stage_ms"][s] - a["stage_ms"][s] for s in b["stage_ms"] if s in a["stage_ms"]}
        return rep
    finally:
        for hp, pr, _s in hps.values():
            pr.free()
            hp.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_query.json"))
    ap.add_argument("--skip-proof", action="store_true")
    args = ap.parse_args()
    from halo2_vectordb_amd import api
    api.init(0)
    doc = dict(shape=dict(metric=METRIC, n=N, dim=DIM, P=P, L=L, k=K), repeats=REPEATS,
               timing="HIP events on the library's stream (witness); wall clock around prove() with device syncs (proof)", cells=sizes(api),
               witness=[witness_probe(api, q, t) for q, t in ((1, 1), (1, 10), (8, 10), (1, 64))])
    doc["launches_equal_in_every_row"] = len({w["launches"] for w in doc["witness"]}) == 1
    if not args.skip_proof:
        doc["proof"] = proof_probe(api)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    brief = dict(cells=doc["cells"], launches_equal=doc["launches_equal_in_every_row"],
                 witness=[dict(q=w["q"], topk=w["topk"], ms=w["topk_ms"]["median"], spread=w["topk_ms"]["spread"], launches=w["launches"])
                          for w in doc["witness"]])
    if "proof" in doc:
        pf = doc["proof"]
        brief["proof"] = {name: dict(ms=pf[name]["proof_ms"]["median"], spread=pf[name]["proof_ms"]["spread"], bytes=pf[name]["proof_bytes"],
                                     advice_columns=pf[name]["advice_columns"], lookup_columns=pf[name]["lookup_columns"], verified=pf[name]["verified"])
                          for name in ("query", "topk_10")}
        brief["proof"]["ratio"] = pf["proof_ms_ratio"]
        brief["proof"]["cell_ratio"] = pf["cell_ratio"]
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
