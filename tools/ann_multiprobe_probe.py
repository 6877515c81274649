#!/usr/bin/env python3
"""What the two knobs of the index query cost and save, measured on the device (writes profiles/ann_multiprobe.json), by the
method of tools/ann_probe.py (warm, alternating repeats, median and spread; proofs by wall clock around prove() with device syncs;
per-kernel launch counts from the library's event profiler in a pass of their own), at n = 1,024, K = 32, dim = 128, p = 4, t = 10:

1. one AnnProbeQueryHotPath proof (the 10 nearest over the 4 nearest clusters) against four AnnQueryHotPath proofs of the same four
   clusters: what four single-probe circuits cost.  Only the first of them can be accepted — the single-probe circuit ties the cluster
   searched to the NEAREST centroid, so the other three break that copy — and each returns one neighbour of its cluster;
2. the same proof against one TopKQueryHotPath(topk = 10) proof over all 1,024 rows, the exact answer;
3. AnnIndex.probe_many(query, 4) against four AnnIndex.probe calls (which give the nearest centroid four times: the only values-only
   way to the later rounds without it is the witness call of a whole top-k block).

    python tools/ann_multiprobe_probe.py [--out profiles/ann_multiprobe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ann_probe import DIM, K, L, LOG_ROWS, METRIC, N, P, TAU, inputs, launches, stats  # noqa: E402

PROBES, TOPK, REPEATS = 4, 10, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ann_multiprobe.json"))
    args = ap.parse_args()
    from halo2_vectordb_amd import api, verifier
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnProbeQueryHotPath, AnnQueryHotPath, TopKQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    api.init(0)
    db, ids, cent, query = inputs()
    index = AnnIndex(N, DIM, K, db, ids, cent, P=P, L=L, metric=METRIC)
    made = {}
    try:
        clusters = index.probe_many(query, PROBES).tolist()
        ctors = [("multi", lambda: AnnProbeQueryHotPath(index, query, probes=PROBES, topk=TOPK, k=LOG_ROWS, P=P, L=L, metric=METRIC, tau=TAU))]
        ctors += [(f"single_{r}", lambda c=c: AnnQueryHotPath(index, query, cluster=c, k=LOG_ROWS, P=P, L=L, metric=METRIC, tau=TAU)) for r, c in enumerate(clusters)]
        ctors += [("topk_all", lambda: TopKQueryHotPath(topk=TOPK, q=1, n=N, dim=DIM, k=LOG_ROWS, P=P, L=L, metric=METRIC, tau=TAU,
                                                        vectors=np.concatenate([query[None], db])))]
        for name, ctor in ctors:
            t0 = time.perf_counter()
            hp = ctor().setup()
            pr = ProverRounds(hp).keygen()
            out = pr.prove(None)                                          # warm
            ok = bool(verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"])))
            made[name] = dict(hp=hp, pr=pr, setup_and_keygen_s=time.perf_counter() - t0, verified=ok, proof_bytes=len(out["proof"]),
                              instances=len(out["instances"]), times=[])
        for _ in range(REPEATS):                                           # alternating
            for name, m in made.items():
                api.sync()
                t0 = time.perf_counter()
                m["pr"].prove(None)
                api.sync()
                m["times"].append((time.perf_counter() - t0) * 1e3)
        rep = {}
        for name, m in made.items():
            hp = m["hp"]
            prof, n_launch = launches(api, hp._witness)
            rep[name] = dict(cells=hp.n_cells, lookup_cells=hp.n_lookup, advice_columns=hp.n_adv_cols, lookup_columns=hp.n_lk_cols, k=hp.k,
                             setup_and_keygen_s=m["setup_and_keygen_s"], proof_ms=stats(m["times"]), proof_bytes=m["proof_bytes"], instances=m["instances"],
                             verified=m["verified"], mock_report_on_keygen_witness=m["pr"].keygen_report.as_dict(), witness_launches=n_launch,
                             witness_kernels_ms=prof)
        multi = made["multi"]["hp"]
        rep["multi"].update(clusters=multi.clusters, sizes=multi.sizes.tolist(), candidates=multi.n, neighbours=multi.neighbours().tolist())
        singles = [rep[f"single_{r}"] for r in range(PROBES)]
        four = dict(cells=sum(s["cells"] for s in singles), proof_ms_sum_of_medians=sum(s["proof_ms"]["median"] for s in singles),
                    proof_ms_per_repeat=[sum(s["proof_ms"]["runs"][i] for s in singles) for i in range(REPEATS)],
                    proof_bytes=sum(s["proof_bytes"] for s in singles))
        four["spread_ms"] = max(four["proof_ms_per_repeat"]) - min(four["proof_ms_per_repeat"])
        four["accepted_by_the_verifier"] = [s["verified"] for s in singles]
        four["note"] = ("AnnQueryHotPath ties the cluster searched to the NEAREST centroid: of the four proofs only the first round's can be accepted, "
                        "the other three break the sel = mroot copy (one Mock violation each) — they are timed as what four such circuits cost")
        # the exact answer's slots against the probed answer's: the recall of this one query
        exact = made["topk_all"]["hp"].results()
        rep["four_single_proofs"] = four
        rep["multi_over_four_singles"] = dict(cells=rep["multi"]["cells"] / four["cells"], proof_ms=rep["multi"]["proof_ms"]["median"] / four["proof_ms_sum_of_medians"])
        rep["multi_over_topk_all"] = dict(cells=rep["multi"]["cells"] / rep["topk_all"]["cells"],
                                          proof_ms=rep["multi"]["proof_ms"]["median"] / rep["topk_all"]["proof_ms"]["median"])
        got_rows = multi.results()[2]
        exact_rows = np.asarray(exact[1]).reshape(-1, DIM, 4)[:TOPK]
        rep["results_also_in_the_exact_top_10"] = int(sum(any(np.array_equal(g, e) for e in exact_rows) for g in got_rows))
        # values-only probing
        t = {"probe_many": [], "probes": []}
        index.probe_many(query, PROBES)
        index.probe(query)
        for _ in range(REPEATS):
            for name, fn in (("probe_many", lambda: index.probe_many(query, PROBES)), ("probes", lambda: [index.probe(query) for _ in range(PROBES)])):
                api.sync()
                t0 = time.perf_counter()
                fn()
                api.sync()
                t[name].append((time.perf_counter() - t0) * 1e3)
        prof, n_launch = launches(api, lambda: index.probe_many(query, PROBES))
        rep["probing"] = dict(probe_many_ms=stats(t["probe_many"]), four_probe_calls_ms=stats(t["probes"]), probe_many_launches=n_launch,
                              probe_many_kernels_ms=prof, clusters=clusters,
                              note="probe() is the witness call of a whole nearest_vector block on host arrays; four calls state the nearest centroid four times")
        doc = dict(shape=dict(metric=METRIC, n=N, K=K, dim=DIM, P=P, L=L, k=LOG_ROWS, probes=PROBES, topk=TOPK), repeats=REPEATS,
                   timing="wall clock around prove() with device syncs, warm, alternating repeats", **rep)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
        print(json.dumps(dict(multi_cells=rep["multi"]["cells"], four_cells=four["cells"], topk_all_cells=rep["topk_all"]["cells"],
                              multi_ms=rep["multi"]["proof_ms"], four_ms=four["proof_ms_per_repeat"], topk_all_ms=rep["topk_all"]["proof_ms"],
                              probe_many_ms=rep["probing"]["probe_many_ms"], four_probes_ms=rep["probing"]["four_probe_calls_ms"],
                              verified=[rep[n]["verified"] for n in made], in_exact_top=rep["results_also_in_the_exact_top_10"],
                              sizes=rep["multi"]["sizes"], mock=rep["multi"]["mock_report_on_keygen_witness"])))
    finally:
        for m in made.values():
            m["pr"].free()
            m["hp"].free()
        index.free()


if __name__ == "__main__":
    main()
