#!/usr/bin/env python3
"""What proving writes against the index root costs, measured on the device (writes profiles/ann_update.json).  Method of
tools/merkle_ops_probe.py: HIP events, warm, five alternating repeats, the spread recorded; per-kernel times and launch counts from the
library's own event profiler in a pass of their own.  n = 1,024 vectors of dim 128 in K = 32 clusters of 32 members, m = 8 writes into
cluster 0: eight replacements (g = 0), and eight appends, which double its tree (g = 1).  Per g:

1. the witness call vdb_wit_ann_update_dev against vdb_wit_merkle_update_ops_dev on the same cluster's tree alone;
2. vdb_ann_index_apply_dev against rebuilding the index with vdb_ann_index_build_dev over the updated database, timed in the same run;
3. the proof (ProverRounds.prove, wall clock, best of `--proofs`) of AnnUpdateHotPath against UpdateHotPath on the same cluster alone.

The plain call against the parent commit's library is tools/merkle_ops_probe.py --parent-tree.

    python tools/ann_update_probe.py [--out profiles/ann_update.json] [--proofs 3] [--skip-proofs]
"""
import argparse
import ctypes
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


def probe(api, grow, proofs):
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnUpdateHotPath, UpdateHotPath, sift_like_vectors
    from halo2_vectordb_amd.rounds import ProverRounds
    lib = api.init()
    db, seed = sift_like_vectors(20260007, N, DIM)
    new, _ = sift_like_vectors(seed + 2000, M, DIM)
    ids = (np.arange(N) % K).astype(np.uint32)
    c, n_c = 0, N // K
    slots = np.arange(M) * 3 % n_c if grow == 0 else n_c + np.arange(M)
    index = AnnIndex(N, DIM, K, db, ids, db[:K], P=P)
    hp = AnnUpdateHotPath(index, c, (slots, new), grow=grow, k=15).setup()
    assert hp.grow == grow
    # the index a rebuild would make: the updated database on the device
    members = np.flatnonzero(ids == c)
    db2, ids2 = db.copy(), ids.copy()
    if grow == 0:
        db2[members[slots]] = new
    else:
        db2, ids2 = np.concatenate([db, new]), np.concatenate([ids, np.full(M, c, dtype=np.uint32)])
    q2 = api.quantize(db2, P)
    n2 = db2.shape[0]
    digests, _ = api.ann_forest_layout(ids2, K)
    cells_plain, n_in = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.vdb_wit_merkle_update_ops_size(n_c, DIM, M, None, grow, ctypes.byref(cells_plain), ctypes.byref(n_in)))
    sizes = np.ascontiguousarray(index.sizes, dtype=np.uint64)
    appends, digests_a, _ = api.ann_index_apply_layout(sizes, c, grow, hp.indices)
    assert digests_a == digests and appends == n2 - N
    db_slots = np.arange(N, n2, dtype=np.uint32)
    index_bytes = (q2.nbytes, n2 * 4, (K + 1) * 8, digests * 32, (K + 2) * 32)
    bufs = [api.DeviceBuffer(x) for x in (q2.nbytes,) + index_bytes + index_bytes + ((3 * M + 2) * 32, cells_plain.value * 32)]
    d_db2, rebuilt, applied, (d_pub, d_adv) = bufs[0], bufs[1:6], bufs[6:11], bufs[11:]
    d_db2.upload(q2)

    def timed(fn):
        api.sync()
        api.timer_start()
        fn()
        return api.timer_stop()

    def reset():
        check(lib.vdb_memcpy_d2d(hp.d_levels.ptr, hp.d_levels0.ptr, ctypes.c_size_t(2 * hp.lp * 32)))

    def witness():
        hp._witness()

    def plain():
        check(lib.vdb_wit_merkle_update_ops_dev(hp.d_levels.ptr, n_c, DIM, grow, hp.d_vec.ptr, api._p(hp.indices), None, M, d_adv.ptr, None, d_pub.ptr))

    def apply():
        check(lib.vdb_ann_index_apply_dev(index.d_grouped.ptr, index.d_slots.ptr, index.d_forest.ptr, index.d_roots.ptr, api._p(sizes), K, DIM, c, grow,
                                          hp.d_levels.ptr, hp.d_vec.ptr, api._p(hp.indices), api._p(db_slots) if appends else None, M,
                                          *[b.ptr for b in applied]))

    def rebuild():
        check(lib.vdb_ann_index_build_dev(d_db2.ptr, api._p(ids2), index.d_cent.ptr, n2, K, DIM, *[b.ptr for b in rebuilt]))

    try:
        ways = dict(witness=witness, plain_update_witness=plain, apply=apply, rebuild=rebuild)
        order = ("plain_update_witness", "witness", "apply", "rebuild")     # apply reads the tree the witness call left
        for name in order:                                                 # warm
            if name != "apply":
                reset()
            ways[name]()
        api.sync()
        for a, b in zip(applied, rebuilt):
            assert np.array_equal(a.download((a.nbytes,), dtype=np.uint8), b.download((b.nbytes,), dtype=np.uint8)), "the applied index is not the rebuilt one"
        times = {name: [] for name in ways}
        for _ in range(REPEATS):                                           # alternating
            for name in order:
                if name != "apply":
                    reset()
                times[name].append(timed(ways[name]))
        kernels = {}
        for name in order:                                                 # per-kernel times and launch counts, a pass of its own
            if name != "apply":
                reset()
            api.sync()
            api.profile_begin(deferred=True)
            ways[name]()
            api.sync()
            kernels[name] = api.profile_end()
        out = dict(grow=grow, n_c=n_c, depth=hp.depth, cells=dict(ann_update=hp.n_cells, plain_update=cells_plain.value),
                   ms={k: stats(v) for k, v in times.items()}, kernels_ms=kernels)
        out["apply_over_rebuild"] = out["ms"]["apply"]["median"] / out["ms"]["rebuild"]["median"]
        out["extra_cells_over_plain"] = hp.n_cells - cells_plain.value
        if proofs:
            pw = {}
            plain_hp = UpdateHotPath(n=n_c, dim=DIM, m=M, k=15, P=P, vectors=db[members], updates=(slots, new), grow=grow).setup()
            for name, h in (("ann_update", hp), ("plain_update", plain_hp)):
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
            plain_hp.free()
            out["proof"] = pw
            out["proof_over_plain"] = pw["ann_update"]["proof_wall_ms"]["median"] / pw["plain_update"]["proof_wall_ms"]["median"]
        return out
    finally:
        for x in bufs:
            x.free()
        hp.free()
        index.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ann_update.json"))
    ap.add_argument("--proofs", type=int, default=3)
    ap.add_argument("--skip-proofs", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from halo2_vectordb_amd import api
    api.init(0)
    doc = dict(shape=dict(n=N, K=K, dim=DIM, m=M, P=P), repeats=REPEATS, timing="HIP events on the library's stream; proofs by wall clock",
               runs=[probe(api, g, 0 if args.skip_proofs else args.proofs) for g in (0, 1)])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps([dict(grow=r["grow"], cells=r["cells"], **{k: round(v["median"], 4) for k, v in r["ms"].items()},
                           spreads={k: round(v["spread"], 4) for k, v in r["ms"].items()}, apply_over_rebuild=round(r["apply_over_rebuild"], 4),
                           proof={k: round(v["proof_wall_ms"]["median"], 1) for k, v in r.get("proof", {}).items()}) for r in doc["runs"]]))


if __name__ == "__main__":
    main()
