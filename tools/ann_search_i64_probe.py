#!/usr/bin/env python3
"""What the batch search over packed rows costs against the field form (writes profiles/ann_search_i64.json).  Method and
shapes of tools/ann_search_probe.py (§4r's 1, 2 and 4): warm, the two forms first held to one answer, then alternating repeats, HIP
events on the library's stream, one session; per-kernel times from the library's event profiler in a pass of their own.

1. Q = 4,096, n = 65,536, dim = 128, t = 10: ns a pair of vdb_ann_search_dev and vdb_ann_search_i64_dev, every metric.
2. Q = 16, n = 262,144, t = 10, the plan's span: the same, every metric.
4. AnnIndex.search at n = 262,144, K = 1,024, probes = 8, topk = 10, Q = 1,024: both stages in both forms, and the pack of the index.

    python tools/ann_search_i64_probe.py [--out profiles/ann_search_i64.json] [--repeats 3] [--metrics euclidean,cosine,...] [--skip-index]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from ann_search_probe import compare  # noqa: E402
from ann_train_probe import P, L, kernels_of, rows_of, stats, timed  # noqa: E402

FIELD_PRODUCT_INSTRUCTIONS = 250                                           # vector instructions of one Montgomery product, about


def model(metric, dim, head_instr):
    """the issue's per-pair model: field products of the head (3 a term) and of the tail, and the packed head's instructions"""
    tail = dict(euclidean=100, cosine=100, manhattan=0, hamming=100)[metric]
    return dict(field_products_field_form=3 * dim + tail, field_products_packed=tail + 1, packed_head_instructions=head_instr[metric] * dim)


def dense(api, repeats, metric, Q, n, dim, t, head_instr):
    qq, qv = rows_of(api, 11, Q, dim), rows_of(api, 12, n, dim)
    bufs = [api.DeviceBuffer(x) for x in (qq.nbytes, qv.nbytes, Q * t * 4, Q * t * 32, Q * dim * 8, n * dim * 8)]
    try:
        bufs[0].upload(qq)
        bufs[1].upload(qv)
        api.pack_i64_dev(bufs[0], Q * dim, bufs[4])
        pack_ms = timed(api, lambda: api.pack_i64_dev(bufs[1], n * dim, bufs[5]))
        calls = dict(field=lambda: api.ann_search_dev(metric, bufs[0], bufs[1], Q, n, dim, t, bufs[2], bufs[3], 0, P, L),
                     packed=lambda: api.ann_search_i64_dev(metric, bufs[4], bufs[5], Q, n, dim, t, bufs[2], bufs[3], 0, P, L))
        answer = lambda name: (bufs[2].download((Q, t), dtype=np.uint32), bufs[3].download((Q, t, 4)))
        out = dict(shape=dict(Q=Q, n=n, dim=dim, t=t), pack_vectors_ms=pack_ms, model=model(metric, dim, head_instr), **compare(api, repeats, calls, answer))
        for k in calls:
            out[f"ns_per_pair_{k}"] = out["device_ms"][k]["median"] * 1e6 / (Q * n)
        out["packed_over_field"] = out["device_ms"]["packed"]["median"] / out["device_ms"]["field"]["median"]
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
    bufs = [api.DeviceBuffer(x) for x in (Q * dim * 32, Q * dim * 8, Q * probes * 4, Q * topk * 4, Q * topk * 32)]
    try:
        bufs[0].upload(api.quantize(queries, P))
        api.pack_i64_dev(bufs[0], Q * dim, bufs[1])
        api.sync()
        api.timer_start()
        pg, pc = ix._packed()
        pack_ms = api.timer_stop()
        api.ann_search_dev(metric, bufs[0], ix.d_cent, Q, K, dim, probes, bufs[2], None, 0, P, L)
        clusters = bufs[2].download((Q, probes), dtype=np.uint32)
        calls = dict(stage1_field=lambda: api.ann_search_dev(metric, bufs[0], ix.d_cent, Q, K, dim, probes, bufs[2], None, 0, P, L),
                     stage1_packed=lambda: api.ann_search_i64_dev(metric, bufs[1], pc, Q, K, dim, probes, bufs[2], None, 0, P, L),
                     stage2_field=lambda: api.ann_search_probed_dev(metric, bufs[0], ix.d_grouped, ix.offsets, clusters, dim, topk, bufs[3], bufs[4], 0, P, L),
                     stage2_packed=lambda: api.ann_search_probed_i64_dev(metric, bufs[1], pg, ix.offsets, clusters, dim, topk, bufs[3], bufs[4], 0, P, L))
        for call in calls.values():
            call()
        got, want = ix.search(queries[:64], probes=probes, topk=topk, packed=True), ix.search(queries[:64], probes=probes, topk=topk)
        assert all(np.array_equal(got[k], want[k]) for k in want), "the two forms disagree"
        times = {name: [] for name in calls}
        for _ in range(repeats):
            for name, call in calls.items():
                times[name].append(timed(api, call))
        pairs = int(ix.sizes[clusters.astype(np.int64)].sum())
        ms = {k: stats(v) for k, v in times.items()}
        return dict(shape=dict(n=n, K=K, dim=dim, Q=Q, probes=probes, topk=topk), device_ms=ms, pack_index_ms=pack_ms, probed_pairs=pairs,
                    kernels_ms={name: kernels_of(api, call) for name, call in calls.items()},
                    stage2_ns_per_pair_field=ms["stage2_field"]["median"] * 1e6 / pairs, stage2_ns_per_pair_packed=ms["stage2_packed"]["median"] * 1e6 / pairs,
                    stage1_packed_over_field=ms["stage1_packed"]["median"] / ms["stage1_field"]["median"],
                    stage2_packed_over_field=ms["stage2_packed"]["median"] / ms["stage2_field"]["median"])
    finally:
        for b in bufs:
            b.free()
        ix.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ann_search_i64.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--metrics", default="euclidean,cosine,manhattan,hamming")
    ap.add_argument("--skip-index", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from halo2_vectordb_amd import api
    api.init(0)
    # instructions a term of the packed head in the gfx950 code object
    head_instr = dict(euclidean=36, cosine=37, manhattan=22, hamming=15)
    doc = dict(P=P, L=L, repeats=args.repeats, timing="HIP events on the library's stream, warm, alternating repeats, one session",
               field_product_instructions=FIELD_PRODUCT_INSTRUCTIONS)

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)

    for m in args.metrics.split(","):
        doc[f"at_scale_{m}"] = dense(api, args.repeats, m, 4096, 65536, 128, 10, head_instr)
        save()
        doc[f"few_queries_{m}"] = dense(api, args.repeats, m, 16, 262144, 128, 10, head_instr)
        save()
    if not args.skip_index:
        doc["index"] = index_search(api, args.repeats, "euclidean", 262144, 1024, 128, 1024, 8, 10)
        save()
    brief = {k: dict(ms={c: round(v["median"], 3) for c, v in doc[k]["device_ms"].items()},
                     spread={c: round(v["spread"], 3) for c, v in doc[k]["device_ms"].items()},
                     **{x: round(y, 4) for x, y in doc[k].items() if isinstance(y, float)}) for k in doc if isinstance(doc[k], dict)}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
