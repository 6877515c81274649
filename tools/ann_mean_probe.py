#!/usr/bin/env python3
"""What the mean audit costs, measured on the device (writes profiles/ann_mean.json), by the method of tools/ann_audit_probe.py
(HIP events on the library's stream, warm, five alternating repeats, median and spread; per-kernel times and launch counts from the
library's event profiler in a pass of their own; proofs by wall clock):

1. values — vdb_ann_cluster_means_dev over the resident index (n = 1,024, K = 32, dim = 128, every cluster 32 members): the one launch of
   k_ann_means behind AnnIndex.means(), and the index AnnIndex.recentred() builds from it;
2. witness — vdb_wit_ann_mean_dev on one cluster of the recentred index against vdb_wit_ann_audit_dev on the same cluster of the same
   index, re-run in the same session;
3. whole proof — AnnMeanHotPath against AnnAuditHotPath at the same k and LOOKUP_BITS, both checked by the verifier; cells and columns
   of both, and whether DESIGN §4k's expectation held.

    python tools/ann_mean_probe.py [--out profiles/ann_mean.json] [--skip-proof]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ann_audit_probe import DIM, K, L, LOG_ROWS, METRIC, N, P, REPEATS, TAU, inputs, launches, stats, timed  # noqa: E402

# stated in DESIGN §4k before anything was measured: the counted cells; the witness call between 0.8 and 1.0 of the routing audit's (the
# two trees' and the header's serial leaf chains are in both and dominate both); the proof at most 0.45 of the audit's (a seventh of
# the cells, but the per-proof floor of a small circuit stays)
EXPECTED = dict(cells=9835545, tree_cells=9663948, select_cells=12416, mean_cells=112129, lookup_cells=24704, audit_cells=68621752,
                witness_ratio_between=[0.8, 1.0], proof_ratio_at_most=0.45)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ann_mean.json"))
    ap.add_argument("--cluster", type=int, default=7)
    ap.add_argument("--skip-proof", action="store_true")
    args = ap.parse_args()
    from halo2_vectordb_amd import api, verifier
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import AnnAuditHotPath, AnnIndex, AnnMeanHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    api.init(0)
    db, ids, cent = inputs()
    built = AnnIndex(N, DIM, K, db, ids, cent, P=P, L=L, metric=METRIC)
    c = args.cluster
    rep = dict(n=N, K=K, dim=DIM, metric=METRIC, P=P, lookup_bits=L, k=LOG_ROWS, cluster=c, n_c=int(built.sizes[c]), expected=EXPECTED)
    hps = {}
    index = None
    try:
        # 1. the values: the raw call into a buffer of its own, then the recentred index
        d_means = api.DeviceBuffer(K * DIM * 32)
        call = lambda: check(built.lib.vdb_ann_cluster_means_dev(P, L, built.d_grouped.ptr, built.d_offsets.ptr, N, K, DIM, d_means.ptr))
        call()
        prof, n_launch = launches(api, call)
        rep["means"] = dict(call_ms=stats([timed(api, call) for _ in range(REPEATS)]), launches=n_launch, kernels_ms=prof)
        d_means.free()
        t0 = time.perf_counter()
        index = built.recentred()
        rep["means"]["recentred_wall_ms"] = (time.perf_counter() - t0) * 1e3
        rep["means"]["recentred_means_are_its_centroids"] = bool(np.array_equal(index.means(), index.qcent))
        rep["assign_agrees_with_the_ids_after_recentring"] = bool(np.array_equal(index.assign(db), ids))
        # 2. and 3.
        ctors = (("mean", lambda: AnnMeanHotPath(index, c, k=LOG_ROWS, P=P, L=L, tau=TAU)),
                 ("routing_audit", lambda: AnnAuditHotPath(index, c, k=LOG_ROWS, P=P, L=L, metric=METRIC, tau=TAU)))
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
        a, b = rep["mean"], rep["routing_audit"]
        rep["mean"]["words_ok"] = int(hps["mean"][0].results()[2].sum())
        rep["routing_audit"]["routed"] = int(hps["routing_audit"][0].results()[2].sum())
        rep["cell_ratio"] = a["cells"] / b["cells"]
        rep["witness_ratio"] = a["witness_ms"]["median"] / b["witness_ms"]["median"]
        lo, hi = EXPECTED["witness_ratio_between"]
        held = dict(cells=a["cells"] == EXPECTED["cells"], lookup_cells=a["lookup_cells"] == EXPECTED["lookup_cells"],
                    audit_cells=b["cells"] == EXPECTED["audit_cells"], witness=lo <= rep["witness_ratio"] <= hi)
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
        if index is not None:
            index.free()
        built.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps({k: rep[k] for k in ("cell_ratio", "witness_ratio", "proof_ratio", "expectation_held") if k in rep}))
    print(json.dumps({"means_call_ms": rep["means"]["call_ms"]["median"], "mean_witness_ms": rep["mean"]["witness_ms"]["median"],
                      "audit_witness_ms": rep["routing_audit"]["witness_ms"]["median"]}))


if __name__ == "__main__":
    main()
