#!/usr/bin/env python3
"""What routing rows to their clusters costs, measured on the device (writes profiles/ann_assign.json).  Method of
tools/ann_update_probe.py: warm, alternating repeats, the spread recorded; per-kernel times and launch counts from the library's own
event profiler in a pass of their own.  n = 1,024 vectors of dim 128 in K = 32 clusters, 1,024 rows to route:

1. AnnIndex.assign over the 1,024 rows (one vdb_nearest_values_dev against the resident centroids; wall clock, the quantisation, the
   upload of the rows and the download of the ids included) against 1,024 AnnIndex.probe calls, the only way before it (each emits
   nearest_vector's stream over the K centroids and reads the indicator off);
2. the device call alone, by HIP events.

The two must agree on every row before anything is timed.

    python tools/ann_assign_probe.py [--out profiles/ann_assign.json] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, DIM, ROWS, P = 1024, 32, 128, 1024, 48


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), spread=max(xs) - min(xs), runs=xs)


def probe(api, repeats):
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import AnnIndex, sift_like_vectors
    lib = api.init()
    db, seed = sift_like_vectors(20260007, N, DIM)
    rows, _ = sift_like_vectors(seed + 3000, ROWS, DIM)
    ids = (np.arange(N) % K).astype(np.uint32)
    index = AnnIndex(N, DIM, K, db, ids, db[:K], P=P)
    q_rows = api.quantize(rows, P)
    bufs = [api.DeviceBuffer(x) for x in (q_rows.nbytes, ROWS * 4, ROWS * 32)]
    bufs[0].upload(q_rows)

    def wall(fn):
        api.sync()
        t0 = time.time()
        out = fn()
        api.sync()
        return (time.time() - t0) * 1e3, out

    def device_call():
        check(lib.vdb_nearest_values_dev(P, index.L, api.METRICS[index.metric_name], bufs[0].ptr, index.d_cent.ptr, ROWS, K, DIM, bufs[1].ptr, bufs[2].ptr))

    def timed(fn):
        api.sync()
        api.timer_start()
        fn()
        return api.timer_stop()

    try:
        ways = dict(assign=lambda: index.assign(rows), probe_calls=lambda: np.asarray([index.probe(r) for r in rows]))
        answers = {name: fn() for name, fn in ways.items()}                # warm
        assert np.array_equal(answers["assign"], answers["probe_calls"]), "assign and probe disagree"
        device_call()
        assert np.array_equal(bufs[1].download((ROWS,), dtype=np.uint32), answers["assign"])
        times = {name: [] for name in ways}
        dev = []
        for _ in range(repeats):                                           # alternating
            for name, fn in ways.items():
                times[name].append(wall(fn)[0])
            dev.append(timed(device_call))
        api.sync()
        api.profile_begin(deferred=True)
        device_call()
        api.sync()
        kernels = api.profile_end()
        out = dict(wall_ms={k: stats(v) for k, v in times.items()}, device_call_ms=stats(dev), kernels_ms=kernels,
                   clusters_hit=int(np.unique(answers["assign"]).size))
        out["probe_calls_over_assign"] = out["wall_ms"]["probe_calls"]["median"] / out["wall_ms"]["assign"]["median"]
        return out
    finally:
        for x in bufs:
            x.free()
        index.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ann_assign.json"))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from halo2_vectordb_amd import api
    api.init(0)
    doc = dict(shape=dict(n=N, K=K, dim=DIM, rows=ROWS, P=P), repeats=args.repeats,
               timing="wall clock for assign and the probe calls (host work included); HIP events on the library's stream for the device call",
               run=probe(api, args.repeats))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    r = doc["run"]
    print(json.dumps(dict(assign_ms=round(r["wall_ms"]["assign"]["median"], 3), probe_calls_ms=round(r["wall_ms"]["probe_calls"]["median"], 1),
                          device_call_ms=round(r["device_call_ms"]["median"], 4), probe_calls_over_assign=round(r["probe_calls_over_assign"], 1),
                          spreads={k: round(v["spread"], 3) for k, v in r["wall_ms"].items()})))


if __name__ == "__main__":
    main()
