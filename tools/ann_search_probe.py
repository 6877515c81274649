#!/usr/bin/env python3
"""What the batch search costs (writes profiles/ann_search.json).  Method of tools/ann_train_probe.py: warm, alternating
repeats, median and spread, HIP events on the library's stream, one session; per-kernel times from the library's own event profiler in
a pass of their own.  Every pair of calls that is compared must first agree on its answer.

1. ns a pair at Q = 4,096, n = 65,536, dim = 128, t = 10 against vdb_ann_assign_dev on the same two arrays (the same tile at t = 1).
2. Q = 16, n = 262,144, t = 10: the plan's span against span = n (one piece a tile) — what the split over the database axis buys.
3. Q = 64, t = 16 against vdb_nearest_topk_values_dev at the largest n of 16,384, 8,192, 4,096, 2,048 that call accepts.
4. AnnIndex.search at n = 262,144, K = 1,024, probes = 8, topk = 10, Q = 1,024 over clustered rows: the two stages, and recall@10
   against search_exact.

    python tools/ann_search_probe.py [--out profiles/ann_search.json] [--repeats 3] [--metric euclidean] [--skip-index]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from ann_train_probe import P, L, kernels_of, rows_of, stats, timed  # noqa: E402


def compare(api, repeats, calls, answer):
    """calls: name -> thunk; answer(name) -> arrays after that call.  Warm and hold the agreement, then alternate."""
    answers = {}
    for name, call in calls.items():
        call()
        answers[name] = answer(name)
    first = next(iter(answers.values()))
    assert all(all(np.array_equal(a, b) for a, b in zip(first, other)) for other in answers.values()), "the calls disagree"
    times = {name: [] for name in calls}
    for _ in range(repeats):
        for name, call in calls.items():
            times[name].append(timed(api, call))
    return dict(device_ms={k: stats(v) for k, v in times.items()}, kernels_ms={name: kernels_of(api, call) for name, call in calls.items()})


def dense(api, repeats, metric, Q, n, dim, t, others):
    """api.ann_search_dev at the plan's span against `others`: name -> (thunk factory over the buffers, columns of the answer compared)"""
    qq, qv = rows_of(api, 11, Q, dim), rows_of(api, 12, n, dim)
    bufs = [api.DeviceBuffer(x) for x in (qq.nbytes, qv.nbytes, Q * t * 4, Q * t * 32)]
    try:
        bufs[0].upload(qq)
        bufs[1].upload(qv)
        calls = dict(ann_search=lambda: api.ann_search_dev(metric, bufs[0], bufs[1], Q, n, dim, t, bufs[2], bufs[3], 0, P, L))
        cols = dict(ann_search=t)
        for name, (make, c) in others.items():
            calls[name], cols[name] = make(bufs), c
        width = min(cols.values())
        answer = lambda name: (bufs[2].download((Q, cols[name]), dtype=np.uint32)[:, :width], bufs[3].download((Q, cols[name], 4))[:, :width])
        out = dict(shape=dict(Q=Q, n=n, dim=dim, t=t), plan={k: v for k, v in api.ann_search_plan(metric, Q, dim, t, n=n, cus=256).items() if np.isscalar(v)},
                   **compare(api, repeats, calls, answer))
        out["ns_per_pair"] = out["device_ms"]["ann_search"]["median"] * 1e6 / (Q * n)
        for name in others:
            out[f"ann_search_over_{name}"] = out["device_ms"]["ann_search"]["median"] / out["device_ms"][name]["median"]
        return out
    finally:
        for b in bufs:
            b.free()


def index_search(api, repeats, metric, n, K, dim, Q, probes, topk):
    from halo2_vectordb_amd.pipeline import AnnIndex
    rng = np.random.default_rng(13)
    centres = rng.integers(30, 190, size=(K, dim)).astype(np.float64)
    rows = centres[rng.integers(0, K, size=n)] + rng.integers(-25, 26, size=(n, dim))
    queries = centres[rng.integers(0, K, size=Q)] + rng.integers(-25, 26, size=(Q, dim))
    qrows, qcent = api.quantize(rows, P), api.quantize(centres, P)
    ids, _ = api.ann_assign(metric, qrows, qcent, P, L)
    ix = AnnIndex(n, dim, K, qrows, ids, qcent, P=P, L=L, metric=metric)
    bufs = [api.DeviceBuffer(x) for x in (Q * dim * 32, Q * probes * 4, Q * topk * 4, Q * topk * 32)]
    try:
        bufs[0].upload(api.quantize(queries, P))
        stage1 = lambda: api.ann_search_dev(metric, bufs[0], ix.d_cent, Q, K, dim, probes, bufs[1], None, 0, P, L)
        stage1()
        clusters = bufs[1].download((Q, probes), dtype=np.uint32)
        stage2 = lambda: api.ann_search_probed_dev(metric, bufs[0], ix.d_grouped, ix.offsets, clusters, dim, topk, bufs[2], bufs[3], 0, P, L)
        exact = lambda: api.ann_search_dev(metric, bufs[0], ix.d_grouped, Q, n, dim, topk, bufs[2], bufs[3], 0, P, L)
        calls = dict(stage1_centroids=stage1, stage2_probed=stage2, exact=exact)
        for call in calls.values():
            call()
        times = {name: [] for name in calls}
        for _ in range(repeats):
            for name, call in calls.items():
                times[name].append(timed(api, call))
        got = ix.search(queries, probes=probes, topk=topk)
        want_slots, want_dist = ix.search_exact(queries, topk)
        # recall on distances: a neighbour counts if its distance is among the exact answer's (rows at equal distance are interchangeable)
        hits = sum(len({d.tobytes() for d in got["dist"][j]} & {d.tobytes() for d in want_dist[j]}) for j in range(Q))
        pairs = int(ix.sizes[got["clusters"]].sum())
        return dict(shape=dict(n=n, K=K, dim=dim, Q=Q, probes=probes, topk=topk), device_ms={k: stats(v) for k, v in times.items()},
                    kernels_ms={name: kernels_of(api, call) for name, call in calls.items()}, probed_pairs=pairs,
                    stage2_ns_per_pair=float(np.median(times["stage2_probed"])) * 1e6 / pairs, recall_at_topk=hits / (Q * topk),
                    largest_cluster=int(ix.sizes.max()), smallest_cluster=int(ix.sizes.min()))
    finally:
        for b in bufs:
            b.free()
        ix.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ann_search.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--metric", default="euclidean")
    ap.add_argument("--skip-index", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from halo2_vectordb_amd import api
    from halo2_vectordb_amd._lib import check
    lib, m, code = api.init(0), args.metric, api.METRICS[args.metric]
    doc = dict(P=P, L=L, metric=m, repeats=args.repeats, timing="HIP events on the library's stream, warm, alternating repeats, one session")

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)

    Q, n, dim = 4096, 65536, 128
    doc["at_scale"] = dense(api, args.repeats, m, Q, n, dim, 10, dict(ann_assign=(
        lambda b: lambda: check(lib.vdb_ann_assign_dev(P, L, code, b[0].ptr, b[1].ptr, Q, n, dim, b[2].ptr, b[3].ptr)), 1)))
    save()
    Q2, n2 = 16, 262144
    doc["few_queries"] = dense(api, max(args.repeats - 1, 1), m, Q2, n2, dim, 10, dict(one_piece=(
        lambda b: lambda: api.ann_search_dev(m, b[0], b[1], Q2, n2, dim, 10, b[2], b[3], n2, P, L), 10)))
    save()
    Q3, shared = 64, None
    for n3 in (16384, 8192, 4096, 2048):                                   # the largest of these the existing call accepts (its cell limit)
        try:
            shared = dense(api, args.repeats, m, Q3, n3, dim, 16, dict(nearest_topk_values=(
                lambda b: lambda: check(lib.vdb_nearest_topk_values_dev(P, L, code, b[0].ptr, b[1].ptr, Q3, n3, dim, 16, b[2].ptr, b[3].ptr)), 16)))
            break
        except api.VdbError as e:
            doc.setdefault("shared_shape_refused", []).append(dict(n=n3, error=str(e)))
    doc["shared_shape"] = shared
    save()
    if not args.skip_index:
        doc["index"] = index_search(api, args.repeats, m, 262144, 1024, dim, 1024, 8, 10)
        save()
    brief = {k: dict(ms={c: round(v["median"], 3) for c, v in doc[k]["device_ms"].items()},
                     spread={c: round(v["spread"], 3) for c, v in doc[k]["device_ms"].items()},
                     **{x: round(y, 4) for x, y in doc[k].items() if isinstance(y, float)}) for k in doc if isinstance(doc[k], dict)}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
