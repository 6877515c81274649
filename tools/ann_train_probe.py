#!/usr/bin/env python3
"""What training the index on the device costs (writes profiles/ann_train.json).  Method of tools/ann_assign_probe.py: warm,
alternating repeats, median and spread, HIP events on the library's stream; per-kernel times from the library's own event profiler in a
pass of their own.

1. vdb_ann_assign_dev against vdb_nearest_values_dev at (1,024 rows, K = 32, dim = 128), the one shape both serve (§4g): the two must
   agree on every row and every distance before anything is timed.
2. One Lloyd iteration at a shape the old path cannot run (by default n = 262,144, K = 1,024, dim = 128): vdb_ann_train_dev capped at one
   iteration, and its per-kernel split.

    python tools/ann_train_probe.py [--out profiles/ann_train.json] [--repeats 5] [--n 262144] [--K 1024] [--dim 128]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = 48, 13


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), spread=max(xs) - min(xs), runs=xs)


def timed(api, fn):
    api.sync()
    api.timer_start()
    fn()
    return api.timer_stop()


def kernels_of(api, fn):
    api.sync()
    api.profile_begin(deferred=True)
    fn()
    api.sync()
    return api.profile_end()


def rows_of(api, seed, n, dim):
    return api.quantize(np.random.default_rng(seed).integers(0, 219, size=(n, dim)).astype(np.float64), P)


def shared_shape(api, repeats, metric):
    from halo2_vectordb_amd._lib import check
    lib, (n, K, dim) = api.init(), (1024, 32, 128)
    q_rows, q_cent = rows_of(api, 1, n, dim), rows_of(api, 2, K, dim)
    bufs = [api.DeviceBuffer(x) for x in (q_rows.nbytes, q_cent.nbytes, n * 4, n * 32)]
    try:
        bufs[0].upload(q_rows)
        bufs[1].upload(q_cent)
        calls = {name: (lambda fn=fn: check(fn(P, L, api.METRICS[metric], bufs[0].ptr, bufs[1].ptr, n, K, dim, bufs[2].ptr, bufs[3].ptr)))
                 for name, fn in (("nearest_values", lib.vdb_nearest_values_dev), ("ann_assign", lib.vdb_ann_assign_dev))}
        answers = {}
        for name, call in calls.items():                                   # warm, and the agreement
            call()
            answers[name] = (bufs[2].download((n,), dtype=np.uint32), bufs[3].download((n, 4)))
        assert all(np.array_equal(a, b) for a, b in zip(*answers.values())), "the two entry points disagree"
        times = {name: [] for name in calls}
        for _ in range(repeats):                                           # alternating
            for name, call in calls.items():
                times[name].append(timed(api, call))
        out = dict(shape=dict(n=n, K=K, dim=dim), device_ms={k: stats(v) for k, v in times.items()},
                   kernels_ms={name: kernels_of(api, call) for name, call in calls.items()})
        out["ann_assign_over_nearest_values"] = out["device_ms"]["ann_assign"]["median"] / out["device_ms"]["nearest_values"]["median"]
        return out
    finally:
        for b in bufs:
            b.free()


def lloyd_iteration(api, repeats, metric, n, K, dim):
    q_rows = rows_of(api, 3, n, dim)
    bufs = [api.DeviceBuffer(x) for x in (q_rows.nbytes, K * dim * 32, n * 4)]
    try:
        bufs[0].upload(q_rows)

        def one():
            bufs[1].upload(q_rows[:K])
            return api.ann_train_dev(metric, bufs[0], n, K, dim, bufs[1], bufs[2], 1, P, L)
        sizes, run = one()                                                 # warm
        assert run == 1 and sizes.sum() == n
        out = dict(shape=dict(n=n, K=K, dim=dim), iteration_ms=stats([timed(api, one) for _ in range(repeats)]), kernels_ms=kernels_of(api, one),
                   clusters_hit=int((sizes > 0).sum()))
        out["ns_per_pair"] = out["iteration_ms"]["median"] * 1e6 / (n * K)
        return out
    finally:
        for b in bufs:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ann_train.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--metric", default="euclidean")
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--K", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=128)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from halo2_vectordb_amd import api
    api.init(0)
    doc = dict(P=P, L=L, metric=args.metric, repeats=args.repeats, timing="HIP events on the library's stream, warm, alternating repeats",
               plan=api.ann_assign_plan(args.metric, args.n, args.K, args.dim), shared=shared_shape(api, args.repeats, args.metric),
               lloyd=lloyd_iteration(api, args.repeats, args.metric, args.n, args.K, args.dim))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    s, ll = doc["shared"], doc["lloyd"]
    print(json.dumps(dict(shared_ms={k: round(v["median"], 4) for k, v in s["device_ms"].items()},
                          shared_spread={k: round(v["spread"], 4) for k, v in s["device_ms"].items()},
                          ratio=round(s["ann_assign_over_nearest_values"], 3), iteration_ms=round(ll["iteration_ms"]["median"], 2),
                          iteration_spread=round(ll["iteration_ms"]["spread"], 2), ns_per_pair=round(ll["ns_per_pair"], 3),
                          kernels_ms={k: round(v["ms"], 3) for k, v in ll["kernels_ms"].items()})))


if __name__ == "__main__":
    main()
