#!/usr/bin/env python3
"""What proving deletes against the index root costs, measured on the device (writes profiles/ann_delete.json).  Method of
tools/ann_update_probe.py: HIP events, warm, five alternating repeats, the spread recorded; per-kernel times and launch counts from the
library's own event profiler in a pass of their own.  n = 1,024 vectors of dim 128 in K = 32 clusters of 32 members, m = 8 deletes from
cluster 0 (32 -> 24 members: the tree keeps its 32 leaves, s = 0), then on the removed index a second batch of 8 (24 -> 16: the tree
halves, s = 1).  Per batch:

1. the witness call vdb_wit_ann_delete_dev against vdb_wit_ann_update_dev over 2 m replacements of the same cluster (as many path
   updates, each with a leaf sponge the delete does not have);
2. vdb_ann_index_remove_dev against rebuilding the index with vdb_ann_index_build_dev over the compacted database, in the same run;
3. the proof (ProverRounds.prove, wall clock, best of `--proofs`) of AnnDeleteHotPath against AnnUpdateHotPath over those replacements.

The plain update call against the parent commit's library is tools/merkle_ops_probe.py --parent-tree.

    python tools/ann_delete_probe.py [--out profiles/ann_delete.json] [--proofs 3] [--skip-proofs]
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


def probe(api, index, proofs):
    """one batch of M deletes from cluster 0 of `index` -> (the figures, the removed index)"""
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import AnnDeleteHotPath, AnnUpdateHotPath, sift_like_vectors
    from halo2_vectordb_amd.rounds import ProverRounds
    lib = api.init()
    c, n_c, n = 0, int(index.sizes[0]), index.n
    slots = np.arange(M) * 3 % (n_c - M)                         # every slot stays below the fill at its turn
    hp = AnnDeleteHotPath(index, c, slots, k=15).setup()
    new, _ = sift_like_vectors(20260009, 2 * M, DIM)
    up = AnnUpdateHotPath(index, c, (np.arange(2 * M) % n_c, new), grow=0, k=15).setup()
    hp._witness()
    api.sync()
    removed = index.removed(hp)
    sizes = np.ascontiguousarray(index.sizes, dtype=np.uint64)
    n2 = n - M
    index_bytes = (n2 * DIM * 32, n2 * 4, (K + 1) * 8, removed.n_digests * 32, (K + 2) * 32)
    bufs = [api.DeviceBuffer(x) for x in (n2 * DIM * 32,) + index_bytes + index_bytes]
    d_db2, rebuilt, again = bufs[0], bufs[1:6], bufs[6:11]
    d_db2.upload(removed.qvec)
    ids2 = np.ascontiguousarray(removed.cluster_ids, dtype=np.uint32)

    def timed(fn):
        api.sync()
        api.timer_start()
        fn()
        return api.timer_stop()

    def remove():
        check(lib.vdb_ann_index_remove_dev(index.d_grouped.ptr, index.d_forest.ptr, index.d_roots.ptr, api._p(sizes), K, DIM, c, hp.d_levels.ptr,
                                           api._p(hp.slots), M, *[b.ptr for b in again]))

    def rebuild():
        check(lib.vdb_ann_index_build_dev(d_db2.ptr, api._p(ids2), index.d_cent.ptr, n2, K, DIM, *[b.ptr for b in rebuilt]))

    try:
        ways = dict(update_witness_2m_replacements=up._witness, witness=hp._witness, remove=remove, rebuild=rebuild)
        order = ("update_witness_2m_replacements", "witness", "remove", "rebuild")      # remove reads the tree the witness call left
        for name in order:                                                 # warm
            ways[name]()
        api.sync()
        for a, b in zip(again, rebuilt):
            assert np.array_equal(a.download((a.nbytes,), dtype=np.uint8), b.download((b.nbytes,), dtype=np.uint8)), "the removed index is not the rebuilt one"
        times = {name: [] for name in ways}
        for _ in range(REPEATS):                                           # alternating
            for name in order:
                times[name].append(timed(ways[name]))
        kernels = {}
        for name in order:                                                 # per-kernel times and launch counts, a pass of its own
            api.sync()
            api.profile_begin(deferred=True)
            ways[name]()
            api.sync()
            kernels[name] = api.profile_end()
        out = dict(n_c=n_c, depth=hp.depth, shrink=hp.shrink, cells=dict(ann_delete=hp.n_cells, ann_update_2m_replacements=up.n_cells),
                   ms={k: stats(v) for k, v in times.items()}, kernels_ms=kernels)
        out["remove_over_rebuild"] = out["ms"]["remove"]["median"] / out["ms"]["rebuild"]["median"]
        out["witness_over_update"] = out["ms"]["witness"]["median"] / out["ms"]["update_witness_2m_replacements"]["median"]
        if proofs:
            pw = {}
            for name, h in (("ann_delete", hp), ("ann_update_2m_replacements", up)):
                pr = ProverRounds(h).keygen()
                assert pr.keygen_report.violations() == 0, pr.keygen_report.as_dict()
                walls = []
                for _ in range(proofs + 1):                                # the first proof warms
                    t0 = time.time()
                    pr.prove(None)
                    api.sync()
                    walls.append((time.time() - t0) * 1e3)
                pw[name] = dict(columns=h.n_cols, cells=h.n_cells, proof_wall_ms=stats(walls[1:]))
                pr.free()
            out["proof"] = pw
            out["proof_over_update"] = pw["ann_delete"]["proof_wall_ms"]["median"] / pw["ann_update_2m_replacements"]["proof_wall_ms"]["median"]
        return out, removed
    except Exception:
        removed.free()
        raise
    finally:
        for x in bufs:
            x.free()
        up.free()
        hp.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ann_delete.json"))
    ap.add_argument("--proofs", type=int, default=3)
    ap.add_argument("--skip-proofs", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from halo2_vectordb_amd import api
    from halo2_vectordb_amd.pipeline import AnnIndex, sift_like_vectors
    api.init(0)
    db, _ = sift_like_vectors(20260007, N, DIM)
    ids = (np.arange(N) % K).astype(np.uint32)
    index = AnnIndex(N, DIM, K, db, ids, db[:K], P=P)
    proofs = 0 if args.skip_proofs else args.proofs
    first, index1 = probe(api, index, proofs)                    # 32 -> 24: s = 0
    second, index2 = probe(api, index1, proofs)                  # 24 -> 16: s = 1
    assert first["shrink"] == 0 and second["shrink"] == 1
    for ix in (index2, index1, index):
        ix.free()
    doc = dict(shape=dict(n=N, K=K, dim=DIM, m=M, P=P), repeats=REPEATS, timing="HIP events on the library's stream; proofs by wall clock", runs=[first, second])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps([dict(shrink=r["shrink"], cells=r["cells"], **{k: round(v["median"], 4) for k, v in r["ms"].items()},
                           spreads={k: round(v["spread"], 4) for k, v in r["ms"].items()}, remove_over_rebuild=round(r["remove_over_rebuild"], 4),
                           witness_over_update=round(r["witness_over_update"], 4),
                           proof={k: round(v["proof_wall_ms"]["median"], 1) for k, v in r.get("proof", {}).items()}) for r in doc["runs"]]))


if __name__ == "__main__":
    main()
