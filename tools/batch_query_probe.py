#!/usr/bin/env python3
"""What a batch of queries in one circuit buys, measured on the device (DESIGN "Batch of queries"; writes profiles/batch_query.json):

1. witness only — vdb_wit_nearest_batch_dev against q successive vdb_wit_nearest_dev calls into the same buffers (the only way to
   produce that stream without the batch entry point), Euclidean, 64 x 128, P = 48, L = 13, q in {1, 8, 32}: HIP-event times, warm,
   five alternating repeats, and the per-kernel times of both ways (the library's own event profiler, a pass of its own);
2. whole proof — BatchQueryHotPath(q = 8) at the smallest k that holds it against one QueryHotPath proof at k = 14: proof time per
   query, the ratio beside the cell ratio, and the stage times of both.

    python tools/batch_query_probe.py [--out profiles/batch_query.json] [--skip-proof]
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
METRIC, N, DIM, P, L = "euclidean", 64, 128, 48, 13
REPEATS = 5


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), spread=max(xs) - min(xs), runs=xs)


def witness_probe(api, q):
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import sift_like_vectors
    lib = api.init()
    m = api.METRICS[METRIC]
    db, seed = sift_like_vectors(20260002, N, DIM)
    queries, _ = sift_like_vectors(seed + 1000, q, DIM)
    qq, qdb = api.quantize(queries, P), api.quantize(db, P)
    c1, l1 = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.vdb_wit_nearest_size(m, P, L, N, DIM, ctypes.byref(c1), ctypes.byref(l1)))
    c1, l1 = c1.value, l1.value
    bufs = [api.DeviceBuffer(x) for x in (qq.nbytes, qdb.nbytes, q * c1 * 32, q * l1 * 32, q * N * 32, q * DIM * 32)]
    d_q, d_db, d_adv, d_lk, d_ind, d_res = bufs
    d_q.upload(qq)
    d_db.upload(qdb)

    def batch():
        check(lib.vdb_wit_nearest_batch_dev(m, P, L, d_q.ptr, d_db.ptr, q, N, DIM, d_adv.ptr, d_lk.ptr, None, d_ind.ptr, d_res.ptr))

    def singles():
        for i in range(q):
            check(lib.vdb_wit_nearest_dev(m, P, L, d_q.at(i * DIM * 32), d_db.ptr, N, DIM, d_adv.at(i * c1 * 32), d_lk.at(i * l1 * 32), None,
                                          d_ind.at(i * N * 32), d_res.at(i * DIM * 32)))

    def timed(fn):
        api.sync()
        api.timer_start()
        fn()
        return api.timer_stop()

    try:
        outs = {}
        for name, fn in (("batch", batch), ("singles", singles)):      # warm, and the two ways must leave the same bytes
            fn()
            api.sync()
            outs[name] = (d_adv.download((q * c1, 4)), d_lk.download((q * l1, 4)), d_res.download((q * DIM, 4)))
        same = all(np.array_equal(a, b) for a, b in zip(outs["batch"], outs["singles"]))
        del outs
        t = {"batch": [], "singles": []}
        for _ in range(REPEATS):                                         # alternating
            t["batch"].append(timed(batch))
            t["singles"].append(timed(singles))
        kernels = {}
        for name, fn in (("batch", batch), ("singles", singles)):      # per-kernel times, a pass of its own
            api.sync()
            api.profile_begin(deferred=True)
            fn()
            api.sync()
            kernels[name] = api.profile_end()
        b, s = stats(t["batch"]), stats(t["singles"])
        spread = max(b["spread"], s["spread"])
        return dict(q=q, cells=q * c1, lookup_cells=q * l1, same_bytes=bool(same), batch_ms=b, singles_ms=s, speedup=s["median"] / b["median"],
                    spread_ms=spread, batch_not_slower=bool(b["median"] <= s["median"] + spread), batch_faster_beyond_spread=bool(s["median"] - b["median"] > spread),
                    stream_write_GBps=q * (c1 + l1) * 32 / (b["median"] * 1e-3) / 1e9, kernels_ms=kernels)
    finally:
        for x in bufs:
            x.free()


def proof_probe(api):
    from halo2_vectordb_amd.pipeline import BatchQueryHotPath, QueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    from halo2_vectordb_amd import verifier
    q = 8
    made = {}
    hps = {}
    # both at k = 14 with the same lookup table (LOOKUP_BITS = 13 needs k >= 14, and 2^14 rows hold the batch: 39.3 M cells are ~2,400
    # advice columns, a fraction of what the k-means circuits put through the same rounds): the smallest k, the same cells as in DESIGN
    for name, ctor in (("single", lambda: QueryHotPath(n=N, dim=DIM, k=14, P=P, L=L, metric=METRIC, tau=TAU)),
                       ("batch", lambda: BatchQueryHotPath(q=q, n=N, dim=DIM, k=14, P=P, L=L, metric=METRIC, tau=TAU))):
        t0 = time.perf_counter()
        hp = ctor().setup()
        pr = ProverRounds(hp).keygen()
        hps[name] = (hp, pr, time.perf_counter() - t0)
    try:
        for name, (hp, pr, _s) in hps.items():
            out = pr.prove(None)                                          # warm
            ok = bool(verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"])))
            made[name] = dict(verified=ok, times=[], stages=None, proof_bytes=len(out["proof"]))
        for _ in range(REPEATS):                                           # alternating
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
            nq = q if name == "batch" else 1
            st = stats(made[name]["times"])
            rep[name] = dict(queries=nq, k=hp.k, lookup_bits=hp.L, cells=hp.n_cells, lookup_cells=hp.n_lookup, advice_columns=hp.n_adv_cols, lookup_columns=hp.n_lk_cols,
                             setup_and_keygen_s=setup_s, proof_ms=st, proof_ms_per_query=st["median"] / nq, proof_bytes=made[name]["proof_bytes"],
                             verified=made[name]["verified"], stage_ms=stages)
        spread = max(rep["single"]["proof_ms"]["spread"], rep["batch"]["proof_ms"]["spread"] / q)
        rep["per_query_ratio"] = rep["single"]["proof_ms_per_query"] / rep["batch"]["proof_ms_per_query"]
        rep["cell_ratio"] = q * rep["single"]["cells"] / rep["batch"]["cells"]
        rep["spread_ms_per_query"] = spread
        rep["batch_per_query_below_single_beyond_spread"] = bool(rep["single"]["proof_ms_per_query"] - rep["batch"]["proof_ms_per_query"] > spread)
        return rep
    finally:
        for hp, pr, _s in hps.values():
            pr.free()
            hp.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_query.json"))
    ap.add_argument("--skip-proof", action="store_true")
    args = ap.parse_args()
    from halo2_vectordb_amd import api
    api.init(0)
    doc = dict(shape=dict(metric=METRIC, n=N, dim=DIM, P=P, L=L), repeats=REPEATS, timing="HIP events on the library's stream (witness); wall clock around prove() with device syncs (proof)",
               witness=[witness_probe(api, q) for q in (1, 8, 32)])
    if not args.skip_proof:
        doc["proof"] = proof_probe(api)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    brief = dict(witness=[{k: w[k] for k in ("q", "same_bytes", "speedup", "spread_ms", "batch_not_slower", "batch_faster_beyond_spread")} | dict(batch_ms=w["batch_ms"]["median"], singles_ms=w["singles_ms"]["median"])
                          for w in doc["witness"]])
    if "proof" in doc:
        pf = doc["proof"]
        brief["proof"] = dict(single_ms=pf["single"]["proof_ms_per_query"], batch_ms_per_query=pf["batch"]["proof_ms_per_query"], ratio=pf["per_query_ratio"],
                              cell_ratio=pf["cell_ratio"], ok=pf["batch_per_query_below_single_beyond_spread"], verified=[pf["single"]["verified"], pf["batch"]["verified"]])
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
