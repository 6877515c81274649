#!/usr/bin/env python3
"""What the committed index buys, measured on the device (writes profiles/ann_query.json), by the method of
tools/batch_query_probe.py (HIP events on the library's stream, warm, five alternating repeats, per-kernel times and launch counts from
the library's event profiler in a pass of their own):

1. index build — vdb_ann_index_build_dev against the K + 1 vdb_merkle_tree_build_dev calls that give the same trees one by one (the
   members of every cluster gathered on the host beforehand, not timed), n = 1,024, K = 32, dim = 128: times, launch counts, and the
   roots of both ways compared;
2. whole proof — AnnQueryHotPath on that index against one QueryHotPath proof over the whole database at the same k and LOOKUP_BITS:
   cells, proof time, the ratio beside the cell ratio, both proofs checked by the verifier.

    python tools/ann_probe.py [--out profiles/ann_query.json] [--skip-proof]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x1234567890ABCDEF1234567
METRIC, N, K, DIM, P, L, LOG_ROWS = "euclidean", 1024, 32, 128, 48, 13, 15
REPEATS = 5


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), spread=max(xs) - min(xs), runs=xs)


def inputs():
    """the database, ids by one assignment step to the first K vectors as centroids (no cluster is empty), a query"""
    from halo2_vectordb_amd.pipeline import sift_like_vectors
    db, seed = sift_like_vectors(20260002, N, DIM)
    query = sift_like_vectors(seed + 1000, 1, DIM)[0][0]
    ids = np.argmin(((db[:, None, :] - db[None, :K, :]) ** 2).sum(axis=2), axis=1)
    ids[:K] = np.arange(K)
    return db, ids.astype(np.uint32), db[:K].copy(), query


def timed(api, fn):
    api.sync()
    api.timer_start()
    fn()
    return api.timer_stop()


def launches(api, fn):
    api.sync()
    api.profile_begin(deferred=True)
    fn()
    api.sync()
    prof = api.profile_end()
    return prof, int(sum(v["launches"] for v in prof.values()))


def build_probe(api, db, ids, cent):
    from halo2_vectordb_amd._lib import check
    lib = api.init()
    qdb, qcent = api.quantize(db, P), api.quantize(cent, P)
    digests, seg = api.ann_forest_layout(ids, K)
    parts = [np.ascontiguousarray(qdb[ids == c]) for c in range(K)] + [qcent]
    bufs = [api.DeviceBuffer(x) for x in (qdb.nbytes, qcent.nbytes, qdb.nbytes, N * 4, (K + 1) * 8, digests * 32, (K + 2) * 32, digests * 32)]
    d_vec, d_cent, d_grouped, d_slots, d_off, d_forest, d_roots, d_single = bufs
    d_parts = [api.DeviceBuffer(p.nbytes) for p in parts]
    try:
        d_vec.upload(qdb)
        d_cent.upload(qcent)
        for d, p in zip(d_parts, parts):
            d.upload(p)

        def index():
            check(lib.vdb_ann_index_build_dev(d_vec.ptr, api._p(ids), d_cent.ptr, N, K, DIM, d_grouped.ptr, d_slots.ptr, d_off.ptr, d_forest.ptr, d_roots.ptr))

        def singles():
            for s, (d, p) in enumerate(zip(d_parts, parts)):
                check(lib.vdb_merkle_tree_build_dev(d.ptr, api._sz(p.shape[0]), api._sz(DIM), d_single.at(int(seg[s]) * 32)))

        index()
        singles()
        api.sync()
        same = bool(np.array_equal(d_forest.download((digests, 4)), d_single.download((digests, 4))))
        t = {"index": [], "singles": []}
        for _ in range(REPEATS):
            t["index"].append(timed(api, index))
            t["singles"].append(timed(api, singles))
        (ki, ni), (ks, ns) = launches(api, index), launches(api, singles)
        a, b = stats(t["index"]), stats(t["singles"])
        return dict(n=N, K=K, dim=DIM, cluster_sizes=np.bincount(ids, minlength=K).tolist(), forest_digests=int(digests), same_forest=same, index_ms=a,
                    singles_ms=b, speedup=b["median"] / a["median"], spread_ms=max(a["spread"], b["spread"]), index_launches=ni, singles_launches=ns,
                    index_kernels_ms=ki, singles_kernels_ms=ks,
                    note="the index call also groups the rows and hashes the sponge; the K + 1 single calls are given the members already gathered")
    finally:
        for x in bufs + d_parts:
            x.free()


def proof_probe(api, db, ids, cent, query):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnQueryHotPath, QueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    index = AnnIndex(N, DIM, K, db, ids, cent, P=P, L=L, metric=METRIC)
    hps, made, rep = {}, {}, {}
    try:
        for name, ctor in (("whole", lambda: QueryHotPath(n=N, dim=DIM, k=LOG_ROWS, P=P, L=L, metric=METRIC, tau=TAU, vectors=np.concatenate([query[None], db]))),
                           ("ann", lambda: AnnQueryHotPath(index, query, k=LOG_ROWS, P=P, L=L, metric=METRIC, tau=TAU))):
            t0 = time.perf_counter()
            hp = ctor().setup()
            pr = ProverRounds(hp).keygen()
            hps[name] = (hp, pr, time.perf_counter() - t0)
        for name, (hp, pr, _s) in hps.items():
            out = pr.prove(None)                                          # warm
            ok = bool(verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"])))
            made[name] = dict(verified=ok, mock=pr.keygen_report.as_dict(), times=[], proof_bytes=len(out["proof"]))
        for _ in range(REPEATS):                                           # alternating
            for name, (hp, pr, _s) in hps.items():
                api.sync()
                t0 = time.perf_counter()
                pr.prove(None)
                api.sync()
                made[name]["times"].append((time.perf_counter() - t0) * 1e3)
        for name, (hp, pr, setup_s) in hps.items():
            stages = {}
            pr.prove(None, timings=stages)
            prof, n_launch = launches(api, hp._witness)
            rep[name] = dict(k=hp.k, lookup_bits=hp.L, cells=hp.n_cells, lookup_cells=hp.n_lookup, advice_columns=hp.n_adv_cols, lookup_columns=hp.n_lk_cols,
                             setup_and_keygen_s=setup_s, proof_ms=stats(made[name]["times"]), proof_bytes=made[name]["proof_bytes"], verified=made[name]["verified"],
                             mock_report_on_keygen_witness=made[name]["mock"], stage_ms=stages, witness_launches=n_launch, witness_kernels_ms=prof)
        rep["ann"].update(cluster=hps["ann"][0].cluster, cluster_size=hps["ann"][0].n)
        rep["proof_ratio"] = rep["whole"]["proof_ms"]["median"] / rep["ann"]["proof_ms"]["median"]
        rep["cell_ratio"] = rep["whole"]["cells"] / rep["ann"]["cells"]
        rep["spread_ms"] = max(rep["whole"]["proof_ms"]["spread"], rep["ann"]["proof_ms"]["spread"])
        return rep
    finally:
        for hp, pr, _s in hps.values():
            pr.free()
            hp.free()
        index.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ann_query.json"))
    ap.add_argument("--skip-proof", action="store_true")
    args = ap.parse_args()
    from halo2_vectordb_amd import api
    api.init(0)
    db, ids, cent, query = inputs()
    doc = dict(shape=dict(metric=METRIC, n=N, K=K, dim=DIM, P=P, L=L, k=LOG_ROWS), repeats=REPEATS,
               timing="HIP events on the library's stream (index build); wall clock around prove() with device syncs (proof)", index_build=build_probe(api, db, ids, cent))
    if not args.skip_proof:
        doc["proof"] = proof_probe(api, db, ids, cent, query)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    b = doc["index_build"]
    brief = dict(index_build=dict(index_ms=b["index_ms"]["median"], singles_ms=b["singles_ms"]["median"], spread_ms=b["spread_ms"], index_launches=b["index_launches"],
                                  singles_launches=b["singles_launches"], same_forest=b["same_forest"]))
    if "proof" in doc:
        pf = doc["proof"]
        brief["proof"] = dict(whole_ms=pf["whole"]["proof_ms"]["median"], ann_ms=pf["ann"]["proof_ms"]["median"], ratio=pf["proof_ratio"], cell_ratio=pf["cell_ratio"],
                              spread_ms=pf["spread_ms"], verified=[pf["whole"]["verified"], pf["ann"]["verified"]])
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
