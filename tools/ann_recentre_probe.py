#!/usr/bin/env python3
"""What the recentre of one cluster costs, measured on the device (writes profiles/ann_recentre.json), by the method of
tools/ann_mean_probe.py (HIP events on the library's stream, warm, five alternating repeats, median and spread; per-kernel times and
launch counts from the library's event profiler in a pass of their own; proofs by wall clock):

1. witness — vdb_wit_ann_recentre_dev on one cluster of the index (n = 1,024, K = 32, dim = 128, every cluster 32 members) against
   vdb_wit_ann_mean_dev on the same cluster of the same rows, re-run in the same session (the mean audit runs on the recentred index, where
   its centroid is the mean: the two circuits have the same (K, n_c, dim));
2. whole proof — AnnRecentreHotPath against AnnMeanHotPath at the same k and LOOKUP_BITS, both checked by the verifier; cells and columns
   of both, and whether DESIGN §4l's expectation held;
3. the index after it — AnnIndex.recentred_with(hp) against the full rebuild of AnnIndex.recentred(), by wall clock, with launch counts.

No time is asserted.  What has not run is written as "not measured".

    python tools/ann_recentre_probe.py [--out profiles/ann_recentre.json] [--skip-proof]
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

# stated in DESIGN §4l before anything was measured: the counted cells (0.53 of the mean audit's); the witness call between 0.9 and 1.25 of
# the mean audit's (MC's serial leaf chain goes, the new leaf's chain of the same length, G's chain and five path levels come); the proof
# between 0.55 and 0.95 of the mean audit's; recentred_with at most 0.2 of the rebuild
EXPECTED = dict(cells=5217434, lookup_cells=24704, update_cells=192026, members_tree_cells=4831974, mean_cells=9835545,
                witness_ratio_between=[0.9, 1.25], proof_ratio_between=[0.55, 0.95], recentred_with_over_rebuild_at_most=0.2)
NOT_MEASURED = "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ann_recentre.json"))
    ap.add_argument("--cluster", type=int, default=7)
    ap.add_argument("--skip-proof", action="store_true")
    args = ap.parse_args()
    from halo2_vectordb_amd import api, verifier
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnMeanHotPath, AnnRecentreHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    api.init(0)
    db, ids, cent = inputs()
    built = AnnIndex(N, DIM, K, db, ids, cent, P=P, L=L, metric=METRIC)
    c = args.cluster
    rep = dict(n=N, K=K, dim=DIM, metric=METRIC, P=P, lookup_bits=L, k=LOG_ROWS, cluster=c, n_c=int(built.sizes[c]), expected=EXPECTED)
    hps, made_ix = {}, []
    try:
        t0 = time.perf_counter()
        target = built.recentred()
        made_ix.append(target)
        rebuild_first_ms = (time.perf_counter() - t0) * 1e3
        ctors = (("recentre", lambda: AnnRecentreHotPath(built, c, k=LOG_ROWS, P=P, L=L, tau=TAU)),
                 ("mean", lambda: AnnMeanHotPath(target, c, k=LOG_ROWS, P=P, L=L, tau=TAU)))
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
            else:
                rep[name].update(proof_ms=NOT_MEASURED, verified=NOT_MEASURED)
        # 3. the index after the proof against the rebuild, alternating, by wall clock (both end in a synchronisation of their own)
        hp = hps["recentre"][0]
        hp._witness()
        api.sync()
        with_ms, rebuild_ms = [], []
        for _ in range(REPEATS):
            api.sync()
            t0 = time.perf_counter()
            ix = built.recentred_with(hp)
            api.sync()
            with_ms.append((time.perf_counter() - t0) * 1e3)
            ix.free()
            t0 = time.perf_counter()
            ix = built.recentred()
            api.sync()
            rebuild_ms.append((time.perf_counter() - t0) * 1e3)
            ix.free()
        keep = []
        prof_with, n_with = launches(api, lambda: keep.append(built.recentred_with(hp)))
        prof_re, n_re = launches(api, lambda: keep.append(built.recentred()))
        made_ix += keep
        rep["index_after"] = dict(recentred_with_wall_ms=stats(with_ms), recentred_wall_ms=stats(rebuild_ms), recentred_first_wall_ms=rebuild_first_ms,
                                  recentred_with_launches=n_with, recentred_with_kernels_ms=prof_with, recentred_launches=n_re, recentred_kernels_ms=prof_re,
                                  root_is_the_proofs_new_root=bool(np.array_equal(keep[0].roots()[-1], hp.results()[2])),
                                  ratio=stats(with_ms)["median"] / stats(rebuild_ms)["median"])
        # the chain over all K clusters ends on recentred()'s root (witness only)
        cur, chain = built, []
        for j in range(K):
            hj = AnnRecentreHotPath(cur, j, k=LOG_ROWS, P=P, L=L, tau=TAU)
            hj._load_inputs()                                              # the streams and the trees alone: no key is needed for a witness
            hj._witness()
            api.sync()
            nxt = cur.recentred_with(hj)
            hj.free()
            chain.append(nxt)
            cur = nxt
        rep["chain_of_K_ends_on_recentred_root"] = bool(np.array_equal(cur.roots(), target.roots()))
        made_ix += chain
        a, b = rep["recentre"], rep["mean"]
        rep["mean"]["words_ok"] = int(hps["mean"][0].results()[2].sum())
        rep["cell_ratio"] = a["cells"] / b["cells"]
        rep["witness_ratio"] = a["witness_ms"]["median"] / b["witness_ms"]["median"]
        lo, hi = EXPECTED["witness_ratio_between"]
        held = dict(cells=a["cells"] == EXPECTED["cells"], lookup_cells=a["lookup_cells"] == EXPECTED["lookup_cells"], mean_cells=b["cells"] == EXPECTED["mean_cells"],
                    witness=lo <= rep["witness_ratio"] <= hi, index_after=rep["index_after"]["ratio"] <= EXPECTED["recentred_with_over_rebuild_at_most"])
        if not args.skip_proof:
            rep["proof_ratio"] = a["proof_ms"]["median"] / b["proof_ms"]["median"]
            rep["spread_ms"] = max(a["proof_ms"]["spread"], b["proof_ms"]["spread"])
            lo, hi = EXPECTED["proof_ratio_between"]
            held["proof"] = lo <= rep["proof_ratio"] <= hi
        else:
            rep["proof_ratio"] = NOT_MEASURED
        rep["expectation_held"] = held
    finally:
        for hp, pr, _s in hps.values():
            if pr is not None:
                pr.free()
            hp.free()
        for ix in made_ix:
            ix.free()
        built.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps({k: rep[k] for k in ("cell_ratio", "witness_ratio", "proof_ratio", "expectation_held", "chain_of_K_ends_on_recentred_root") if k in rep}))
    print(json.dumps({"recentre_witness_ms": rep["recentre"]["witness_ms"]["median"], "mean_witness_ms": rep["mean"]["witness_ms"]["median"],
                      "recentred_with_ms": rep["index_after"]["recentred_with_wall_ms"]["median"], "recentred_ms": rep["index_after"]["recentred_wall_ms"]["median"]}))


if __name__ == "__main__":
    main()
