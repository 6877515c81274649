#!/usr/bin/env python3
"""What a linked write costs beside the plain write and beside what it replaces, the plain write plus a fresh cover of the new pair of
roots, measured on the device (writes profiles/ann_write.json).  Method of tools/ann_move_probe.py: HIP events, warm, five
alternating repeats, median and spread; per-kernel times and launch counts from the library's own event profiler in a pass of their
own; proofs by wall clock, the median of `--proofs`.  §4h's probe shape: n = 1,024 vectors of dim 128 in K = 32 clusters of 32 members,
m = 8 writes into cluster 0, four replacements and four appends (32 -> 36 members: g_c = 1; 1,024 -> 1,028 rows: g_db = 1):

1. the witness call vdb_wit_ann_write_dev against vdb_wit_ann_update_dev on the same batch;
2. vdb_ann_index_write_dev against vdb_ann_index_apply_dev + vdb_ann_index_db_tree_dev over the index it leaves;
3. the proof of AnnWriteHotPath against the proofs of AnnUpdateHotPath and of AnnCoverHotPath over the new pair of roots.

    python tools/ann_write_probe.py [--out profiles/ann_write.json] [--proofs 3] [--skip-proofs]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, DIM, M, P, REPEATS = 1024, 32, 128, 8, 48, 5


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), spread=max(xs) - min(xs), runs=xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ann_write.json"))
    ap.add_argument("--proofs", type=int, default=3)
    ap.add_argument("--skip-proofs", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from halo2_vectordb_amd import api
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import AnnCoverHotPath, AnnIndex, AnnUpdateHotPath, AnnWriteHotPath, sift_like_vectors
    from halo2_vectordb_amd.rounds import ProverRounds
    lib = api.init(0)
    db, seed = sift_like_vectors(20260007, N, DIM)
    rows = sift_like_vectors(seed + 2000, M, DIM)[0]
    ids = (np.arange(N) % K).astype(np.uint32)
    index = AnnIndex(N, DIM, K, db, ids, db[:K], P=P)
    c, n_c = 0, int(index.sizes[0])
    slots = np.asarray([0, 1, 2, 3] + [n_c + i for i in range(M - 4)], dtype=np.uint64)
    made = [index]
    try:
        wr = AnnWriteHotPath(index, c, (slots, rows), k=15).setup()
        made.append(wr)
        up = AnnUpdateHotPath(index, c, (slots, rows), grow=None, k=15).setup()
        made.append(up)
        for h in (wr, up):
            h._witness()
        api.sync()
        written, applied = index.written(wr), index.updated(up)
        made += [written, applied]
        assert (wr.grow, wr.grow_db, up.grow, wr.appends) == (1, 1, 1, M - 4)
        n2 = written.n
        lp2 = 2 * api.merkle_levels(n2)[0]
        assert np.array_equal(written.roots(), applied.roots()), "the linked write reaches the plain write's index"
        assert np.array_equal(written.database_tree().download((lp2, 4)), applied.database_tree().download((lp2, 4))), "and the database tree a fresh build gives"
        assert np.array_equal(wr.results()[7], written.database_tree().download((lp2, 4))[-2]) and np.array_equal(wr.results()[8], written.roots()[-1])
        cover = AnnCoverHotPath(written, k=15).setup()
        made.append(cover)
        cover._witness()
        api.sync()
        assert np.array_equal(np.stack(cover.results()[:2]), np.stack(wr.results()[7:])), "the fresh cover publishes the pair the write published"
        sizes0 = np.ascontiguousarray(index.sizes, dtype=np.uint64)
        sizes2 = np.ascontiguousarray(written.sizes, dtype=np.uint64)
        out_bytes = (n2 * DIM * 32, n2 * 4, (K + 1) * 8, written.n_digests * 32, (K + 2) * 32)
        bufs = {name: [api.DeviceBuffer(x) for x in out_bytes] for name in ("write", "apply")}
        bufs["write"].append(api.DeviceBuffer(lp2 * 32))
        d_tree = api.DeviceBuffer(lp2 * 32)
        app_slots = np.arange(N, N + M - 4, dtype=np.uint32)

        def timed(fn):
            api.sync()
            api.timer_start()
            fn()
            return api.timer_stop()

        def index_write():
            check(lib.vdb_ann_index_write_dev(index.d_grouped.ptr, index.d_slots.ptr, index.d_forest.ptr, index.d_roots.ptr, api._p(sizes0), K, DIM, c, wr.grow,
                                              wr.grow_db, wr.d_levels.ptr, wr.d_levels_db.ptr, wr.d_vec.ptr, api._p(wr.indices), M, *[x.ptr for x in bufs["write"]]))

        def apply_db_tree():
            check(lib.vdb_ann_index_apply_dev(index.d_grouped.ptr, index.d_slots.ptr, index.d_forest.ptr, index.d_roots.ptr, api._p(sizes0), K, DIM, c, up.grow,
                                              up.d_levels.ptr, up.d_vec.ptr, api._p(up.indices), api._p(app_slots), M, *[x.ptr for x in bufs["apply"]]))
            check(lib.vdb_ann_index_db_tree_dev(bufs["apply"][3].ptr, api._p(sizes2), bufs["apply"][1].ptr, K, n2, d_tree.ptr))

        ways = dict(update_witness=up._witness, witness=wr._witness, index_write=index_write, apply_db_tree=apply_db_tree)
        order = ("update_witness", "witness", "index_write", "apply_db_tree")           # the index calls read the trees the witness calls left
        for name in order:                                                              # warm
            ways[name]()
        api.sync()
        x, y = bufs["write"][5], d_tree
        assert np.array_equal(x.download((x.nbytes,), dtype=np.uint8), y.download((y.nbytes,), dtype=np.uint8)), "the two database trees differ"
        times = {name: [] for name in ways}
        for _ in range(REPEATS):                                                        # alternating
            for name in order:
                times[name].append(timed(ways[name]))
        kernels = {}
        for name in order:                                                              # per-kernel times and launch counts, a pass of its own
            api.sync()
            api.profile_begin(deferred=True)
            ways[name]()
            api.sync()
            kernels[name] = api.profile_end()
        out = dict(shape=dict(n=N, K=K, dim=DIM, m=M, appends=M - 4, P=P, n_c=n_c, d_c=wr.depth, g_c=wr.grow, d_db=wr.depth_db, g_db=wr.grow_db), repeats=REPEATS,
                   timing="HIP events on the library's stream; proofs by wall clock",
                   cells=dict(ann_write=wr.n_cells, ann_update=up.n_cells, e_db=wr.n_cells - up.n_cells, ann_cover_new_pair=cover.n_cells),
                   columns=dict(ann_write=wr.n_cols, ann_update=up.n_cols, ann_cover_new_pair=cover.n_cols),
                   ms={k: stats(v) for k, v in times.items()}, kernels_ms=kernels)
        out["witness_over_update"] = out["ms"]["witness"]["median"] / out["ms"]["update_witness"]["median"]
        out["index_write_over_apply_db_tree"] = out["ms"]["index_write"]["median"] / out["ms"]["apply_db_tree"]["median"]
        if not args.skip_proofs:
            pw = {}
            for name, h in (("ann_write", wr), ("ann_update", up), ("ann_cover_new_pair", cover)):
                pr = ProverRounds(h).keygen()
                assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
                walls = []
                for _ in range(args.proofs + 1):                                        # the first proof warms
                    t0 = time.time()
                    pr.prove(None)
                    api.sync()
                    walls.append((time.time() - t0) * 1e3)
                pw[name] = dict(columns=h.n_cols, cells=h.n_cells, proof_wall_ms=stats(walls[1:]))
                pr.free()
            out["proof"] = pw
            pair = pw["ann_update"]["proof_wall_ms"]["median"] + pw["ann_cover_new_pair"]["proof_wall_ms"]["median"]
            out["proof_over_update"] = pw["ann_write"]["proof_wall_ms"]["median"] / pw["ann_update"]["proof_wall_ms"]["median"]
            out["proof_over_update_plus_cover"] = pw["ann_write"]["proof_wall_ms"]["median"] / pair
        for group in bufs.values():
            for x in group:
                x.free()
        d_tree.free()
    finally:
        for x in reversed(made):
            x.free()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(cells=out["cells"], **{k: round(v["median"], 4) for k, v in out["ms"].items()},
                          spreads={k: round(v["spread"], 4) for k, v in out["ms"].items()}, witness_over_update=round(out["witness_over_update"], 4),
                          index_write_over_apply_db_tree=round(out["index_write_over_apply_db_tree"], 4),
                          proof={k: round(v["proof_wall_ms"]["median"], 1) for k, v in out.get("proof", {}).items()},
                          proof_over_update=round(out.get("proof_over_update", 0.0), 4),
                          proof_over_update_plus_cover=round(out.get("proof_over_update_plus_cover", 0.0), 4))))


if __name__ == "__main__":
    main()
