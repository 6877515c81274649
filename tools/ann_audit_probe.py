#!/usr/bin/env python3
"""What the routing audit costs, measured on the device (writes profiles/ann_audit.json), by the method of tools/ann_probe.py
(HIP events on the library's stream, warm, five alternating repeats, median and spread; per-kernel times and launch counts from the
library's event profiler in a pass of their own; proofs by wall clock):

1. witness — vdb_wit_ann_audit_dev on one cluster of a resident index (n = 1,024, K = 32, dim = 128, every cluster 32 members) against the
   witness call of the only way to state routing with what existed: BatchQueryHotPath(q = n_c, n = K), nearest_vector of every member
   over the centroids (which commits to the centroids alone: no member, no index root);
2. whole proof — AnnAuditHotPath against that BatchQueryHotPath at the same k and LOOKUP_BITS, both checked by the verifier; cells and
   columns of both, and whether DESIGN §4j's expectation held.

    python tools/ann_audit_probe.py [--out profiles/ann_audit.json] [--skip-proof]
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
EXPECTED = dict(cells=68621752, routed_block_cells=58910752, tree_cells=9663948, baseline_cells=59325440, columns=2095, baseline_columns=1811,
                proof_ratio_at_most=1.25, witness_ratio_at_most=1.6)


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), spread=max(xs) - min(xs), runs=xs)


def inputs():
    """K SIFT-like centroids and N / K members within 3 of each, a word at a time: every row's nearest centroid is its own"""
    from halo2_vectordb_amd.pipeline import sift_like_vectors
    cent, _ = sift_like_vectors(20260002, K, DIM)
    rng = np.random.default_rng(20260003)
    per = N // K
    db = np.concatenate([np.clip(cent[c] + rng.integers(-3, 4, (per, DIM)), 0, 218) for c in range(K)]).astype(np.float64)
    return db, np.repeat(np.arange(K), per).astype(np.uint32), cent


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ann_audit.json"))
    ap.add_argument("--cluster", type=int, default=7)
    ap.add_argument("--skip-proof", action="store_true")
    args = ap.parse_args()
    from halo2_vectordb_amd import api, verifier
    from halo2_vectordb_amd.pipeline import AnnAuditHotPath, AnnIndex, BatchQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    api.init(0)
    db, ids, cent = inputs()
    index = AnnIndex(N, DIM, K, db, ids, cent, P=P, L=L, metric=METRIC)
    c = args.cluster
    members = db[ids == c]
    rep = dict(n=N, K=K, dim=DIM, metric=METRIC, P=P, lookup_bits=L, k=LOG_ROWS, cluster=c, n_c=int(members.shape[0]), expected=EXPECTED,
               assign_agrees_with_the_ids=bool(np.array_equal(index.assign(db), ids)))
    hps = {}
    try:
        ctors = (("audit", lambda: AnnAuditHotPath(index, c, k=LOG_ROWS, P=P, L=L, metric=METRIC, tau=TAU)),
                 ("nearest_vector_baseline", lambda: BatchQueryHotPath(q=members.shape[0], n=K, dim=DIM, k=LOG_ROWS, P=P, L=L, metric=METRIC, tau=TAU,
                                                                       vectors=np.concatenate([members, cent]))))
        for name, ctor in ctors:
            t0 = time.perf_counter()
            hp = ctor().setup()
            pr = None if args.skip_proof else ProverRounds(hp).keygen()
            hps[name] = (hp, pr, time.perf_counter() - t0)
        wit = {name: [] for name in hps}
        for hp, _pr, _s in hps.values():
            hp._witness()                                                  # warm
        for _ in range(REPEATS):                                           # alternating
            for name, (hp, _pr, _s) in hps.items():
                wit[name].append(timed(api, hp._witness))
        made = {}
        if not args.skip_proof:
            for name, (hp, pr, _s) in hps.items():
                out = pr.prove(None)                                       # warm
                ok = bool(verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"])))
                made[name] = dict(verified=ok, mock=pr.keygen_report.as_dict(), times=[], proof_bytes=len(out["proof"]), n_instances=len(out["instances"]))
            for _ in range(REPEATS):
                for name, (hp, pr, _s) in hps.items():
                    api.sync()
                    t0 = time.perf_counter()
                    pr.prove(None)
                    api.sync()
                    made[name]["times"].append((time.perf_counter() - t0) * 1e3)
        for name, (hp, pr, setup_s) in hps.items():
            prof, n_launch = launches(api, hp._witness)
            rep[name] = dict(cells=hp.n_cells, lookup_cells=hp.n_lookup, advice_columns=hp.n_adv_cols, lookup_columns=hp.n_lk_cols, columns=hp.n_cols,
                             setup_and_keygen_s=setup_s, witness_ms=stats(wit[name]), witness_launches=n_launch, witness_kernels_ms=prof)
            if pr is not None:
                stages = {}
                pr.prove(None, timings=stages)
                rep[name].update(proof_ms=stats(made[name]["times"]), proof_bytes=made[name]["proof_bytes"], n_instances=made[name]["n_instances"],
                                 verified=made[name]["verified"], mock_report_on_keygen_witness=made[name]["mock"], stage_ms=stages)
        a, b = rep["audit"], rep["nearest_vector_baseline"]
        rep["audit"]["routed"] = int(hps["audit"][0].results()[2].sum())
        rep["cell_ratio"] = a["cells"] / b["cells"]
        rep["witness_ratio"] = a["witness_ms"]["median"] / b["witness_ms"]["median"]
        held = dict(cells=a["cells"] == EXPECTED["cells"], baseline_cells=b["cells"] == EXPECTED["baseline_cells"],
                    witness=rep["witness_ratio"] <= EXPECTED["witness_ratio_at_most"])
        if not args.skip_proof:
            rep["proof_ratio"] = a["proof_ms"]["median"] / b["proof_ms"]["median"]
            rep["spread_ms"] = max(a["proof_ms"]["spread"], b["proof_ms"]["spread"])
            held["proof"] = rep["proof_ratio"] <= EXPECTED["proof_ratio_at_most"]
        rep["expectation_held"] = held
    finally:
        for hp, pr, _s in hps.values():
            if pr is not None:
                pr.free()
            hp.free()
        index.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps({k: rep[k] for k in ("cell_ratio", "witness_ratio", "proof_ratio", "expectation_held") if k in rep}))


if __name__ == "__main__":
    main()
