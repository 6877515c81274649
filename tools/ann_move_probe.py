#!/usr/bin/env python3
"""What proving a move against the index root costs beside the delete and the write it replaces, measured on the device (DESIGN §4o;
writes profiles/ann_move.json).  Method of tools/ann_delete_probe.py: HIP events, warm, five alternating repeats, median and spread;
per-kernel times and launch counts from the library's own event profiler in a pass of their own; proofs by wall clock, the median of
`--proofs`.  n = 1,024 vectors of dim 128 in K = 32 clusters of 32 members, m = 8 moves from cluster 0 (32 -> 24 members: s = 0) to
cluster 1 (32 -> 40: its tree doubles, g = 1):

1. the witness call vdb_wit_ann_move_dev against vdb_wit_ann_delete_dev (the 8 deletes from cluster 0) and vdb_wit_ann_update_dev (the 8
   appends of the same vectors to cluster 1 of the removed index) run back to back;
2. vdb_ann_index_move_dev against vdb_ann_index_remove_dev + vdb_ann_index_apply_dev, and against rebuilding the index with
   vdb_ann_index_build_dev over the same database with the moved ids;
3. the proof of AnnMoveHotPath against the proofs of AnnDeleteHotPath and AnnUpdateHotPath.

    python tools/ann_move_probe.py [--out profiles/ann_move.json] [--proofs 3] [--skip-proofs]
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
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ann_move.json"))
    ap.add_argument("--proofs", type=int, default=3)
    ap.add_argument("--skip-proofs", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from halo2_vectordb_amd import api
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import AnnDeleteHotPath, AnnIndex, AnnMoveHotPath, AnnUpdateHotPath, sift_like_vectors
    from halo2_vectordb_amd.rounds import ProverRounds
    lib = api.init(0)
    db, _ = sift_like_vectors(20260007, N, DIM)
    ids = (np.arange(N) % K).astype(np.uint32)
    index = AnnIndex(N, DIM, K, db, ids, db[:K], P=P)
    a, b, n_a, n_b = 0, 1, int(index.sizes[0]), int(index.sizes[1])
    slots = np.arange(M) * 3 % (n_a - M)                             # every slot stays below the fill at its turn
    made = [index]
    try:
        mv = AnnMoveHotPath(index, a, b, slots, k=15).setup()
        made.append(mv)
        dl = AnnDeleteHotPath(index, a, slots, k=15).setup()
        made.append(dl)
        for h in (mv, dl):
            h._witness()
        api.sync()
        moved, removed = index.moved(mv), index.removed(dl)
        made += [moved, removed]
        # the write of the pair: the vectors the deletes took, appended to cluster 1 of the removed index
        rows = db[np.flatnonzero(ids == a)[np.asarray(mv.moved_from)]]
        up = AnnUpdateHotPath(removed, b, (np.arange(n_b, n_b + M), rows), grow=None, k=15).setup()
        made.append(up)
        up._witness()
        api.sync()
        applied = removed.updated(up)
        made.append(applied)
        assert (mv.shrink, mv.grow, up.grow) == (0, 1, 1)
        assert np.array_equal(applied.roots()[-1], moved.roots()[-1]), "the pair reaches the move's index root"
        assert not np.array_equal(applied.database_tree().download((2 * N, 4)), index.database_tree().download((2 * N, 4))), "the pair renumbers the database"
        assert np.array_equal(moved.database_tree().download((2 * N, 4)), index.database_tree().download((2 * N, 4))), "the move does not"
        sizes0 = np.ascontiguousarray(index.sizes, dtype=np.uint64)
        sizes1 = np.ascontiguousarray(removed.sizes, dtype=np.uint64)
        out_bytes = lambda ix: (ix.n * DIM * 32, ix.n * 4, (K + 1) * 8, ix.n_digests * 32, (K + 2) * 32)
        bufs = {name: [api.DeviceBuffer(x) for x in out_bytes(ix)] for name, ix in (("move", moved), ("remove", removed), ("apply", applied), ("rebuild", moved))}
        d_db = api.DeviceBuffer(moved.qvec.nbytes)
        d_db.upload(moved.qvec)
        ids2 = np.ascontiguousarray(moved.cluster_ids, dtype=np.uint32)
        app_slots = np.arange(removed.n, removed.n + M, dtype=np.uint32)

        def timed(fn):
            api.sync()
            api.timer_start()
            fn()
            return api.timer_stop()

        def move():
            check(lib.vdb_ann_index_move_dev(index.d_grouped.ptr, index.d_slots.ptr, index.d_forest.ptr, index.d_roots.ptr, api._p(sizes0), K, DIM, a, b, mv.grow,
                                             mv.d_levels_a.ptr, mv.d_levels_b.ptr, api._p(mv.slots), M, *[x.ptr for x in bufs["move"]]))

        def remove_apply():
            check(lib.vdb_ann_index_remove_dev(index.d_grouped.ptr, index.d_forest.ptr, index.d_roots.ptr, api._p(sizes0), K, DIM, a, dl.d_levels.ptr,
                                               api._p(dl.slots), M, *[x.ptr for x in bufs["remove"]]))
            check(lib.vdb_ann_index_apply_dev(removed.d_grouped.ptr, removed.d_slots.ptr, removed.d_forest.ptr, removed.d_roots.ptr, api._p(sizes1), K, DIM, b,
                                              up.grow, up.d_levels.ptr, up.d_vec.ptr, api._p(up.indices), api._p(app_slots), M, *[x.ptr for x in bufs["apply"]]))

        def rebuild():
            check(lib.vdb_ann_index_build_dev(d_db.ptr, api._p(ids2), index.d_cent.ptr, N, K, DIM, *[x.ptr for x in bufs["rebuild"]]))

        def pair_witness():
            dl._witness()
            up._witness()

        ways = dict(pair_witness=pair_witness, witness=mv._witness, move=move, remove_apply=remove_apply, rebuild=rebuild)
        order = ("pair_witness", "witness", "move", "remove_apply", "rebuild")          # the index calls read the trees the witness calls left
        for name in order:                                                              # warm
            ways[name]()
        api.sync()
        # the moved index and the rebuild have the same offsets (a build over the moved database orders a cluster by database slot, the
        # move by swap-with-last, so the two differ inside clusters a and b: tests/test_gpu_ann_move.py holds the move to a build over its own rows)
        x, y = bufs["move"][2], bufs["rebuild"][2]
        assert np.array_equal(x.download((x.nbytes,), dtype=np.uint8), y.download((y.nbytes,), dtype=np.uint8)), "offsets differ"
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
        out = dict(shape=dict(n=N, K=K, dim=DIM, m=M, P=P, n_a=n_a, n_b=n_b, d_a=mv.depth, s=mv.shrink, d_b=mv.depth_b, g=mv.grow), repeats=REPEATS,
                   timing="HIP events on the library's stream; proofs by wall clock",
                   cells=dict(ann_move=mv.n_cells, ann_delete=dl.n_cells, ann_update_appends=up.n_cells), columns=dict(ann_move=mv.n_cols, ann_delete=dl.n_cols,
                                                                                                                     ann_update_appends=up.n_cols),
                   ms={k: stats(v) for k, v in times.items()}, kernels_ms=kernels)
        out["witness_over_pair"] = out["ms"]["witness"]["median"] / out["ms"]["pair_witness"]["median"]
        out["move_over_remove_apply"] = out["ms"]["move"]["median"] / out["ms"]["remove_apply"]["median"]
        out["move_over_rebuild"] = out["ms"]["move"]["median"] / out["ms"]["rebuild"]["median"]
        if not args.skip_proofs:
            pw = {}
            for name, h in (("ann_move", mv), ("ann_delete", dl), ("ann_update_appends", up)):
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
            pair = pw["ann_delete"]["proof_wall_ms"]["median"] + pw["ann_update_appends"]["proof_wall_ms"]["median"]
            out["proof_over_pair"] = pw["ann_move"]["proof_wall_ms"]["median"] / pair
        for group in bufs.values():
            for x in group:
                x.free()
        d_db.free()
    finally:
        for x in reversed(made):
            x.free()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(cells=out["cells"], **{k: round(v["median"], 4) for k, v in out["ms"].items()},
                          spreads={k: round(v["spread"], 4) for k, v in out["ms"].items()}, witness_over_pair=round(out["witness_over_pair"], 4),
                          move_over_remove_apply=round(out["move_over_remove_apply"], 4), move_over_rebuild=round(out["move_over_rebuild"], 4),
                          proof={k: round(v["proof_wall_ms"]["median"], 1) for k, v in out.get("proof", {}).items()},
                          proof_over_pair=round(out.get("proof_over_pair", 0.0), 4))))


if __name__ == "__main__":
    main()
