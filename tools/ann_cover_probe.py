#!/usr/bin/env python3
"""What the cover of the database by the index costs, measured on the device (writes profiles/ann_cover.json), by the method of
tools/ann_audit_probe.py (HIP events on the library's stream, warm, five alternating repeats, median and spread; per-kernel times and
launch counts from the library's event profiler in a pass of their own; proofs by wall clock):

1. witness — vdb_wit_ann_cover_dev on the resident index (n = 1,024, K = 32, dim = 128, every cluster 32 members) against
   vdb_wit_merkle_dev over the same database, re-run in the same session;
2. whole proof — AnnCoverHotPath against MerkleHotPath at the same k, the cover checked by the verifier; cells and columns of both, and
   whether DESIGN §4n's expectation held;
3. the database tree — AnnIndex.database_tree()'s call (vdb_ann_index_db_tree_dev: digests copied, levels hashed) against
   vdb_merkle_tree_build_dev over the rows, by HIP events, and that the two trees are equal.

No time is asserted.  What has not run is written as "not measured".

    python tools/ann_cover_probe.py [--out profiles/ann_cover.json] [--skip-proof]
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

# stated in DESIGN §4n before anything was measured: the counted cells (0.059 of the Merkle circuit's); the witness call at most 0.25 of
# the Merkle circuit's (no leaf sponge: the serial chain is D's 17 permutations and G's 2 against a leaf's 65); the proof between 0.05
# and 0.30 of the Merkle circuit's (the cell ratio, above a floor that does not shrink with the columns)
EXPECTED = dict(cells=9140902, merkle_cells=154893926, cell_ratio=9140902 / 154893926, witness_ratio_at_most=0.25, proof_ratio_between=[0.05, 0.30])
NOT_MEASURED = "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ann_cover.json"))
    ap.add_argument("--skip-proof", action="store_true")
    args = ap.parse_args()
    from halo2_vectordb_amd import api, verifier
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import AnnCoverHotPath, AnnIndex, MerkleHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    api.init(0)
    db, ids, cent = inputs()
    index = AnnIndex(N, DIM, K, db, ids, cent, P=P, L=L, metric=METRIC)
    rep = dict(n=N, K=K, dim=DIM, P=P, k=LOG_ROWS, cluster_sizes=[int(x) for x in index.sizes], expected=EXPECTED)
    hps = {}
    try:
        ctors = (("cover", lambda: AnnCoverHotPath(index, k=LOG_ROWS, tau=TAU)),
                 ("merkle", lambda: MerkleHotPath(n=N, dim=DIM, k=LOG_ROWS, P=P, tau=TAU, vectors=db)))
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
            rep[name] = dict(cells=hp.n_cells, advice_columns=hp.n_adv_cols, columns=hp.n_cols, setup_and_keygen_s=setup_s, witness_ms=stats(wit[name]),
                             witness_launches=n_launch, witness_kernels_ms=prof)
            if pr is not None:
                stages = {}
                pr.prove(None, timings=stages)
                rep[name].update(proof_ms=stats(made[name]["times"]), proof_bytes=made[name]["proof_bytes"], n_instances=made[name]["n_instances"],
                                 verified=made[name]["verified"], mock_report_on_keygen_witness=made[name]["mock"], stage_ms=stages)
            else:
                rep[name].update(proof_ms=NOT_MEASURED, verified=NOT_MEASURED)
        cover, merkle = hps["cover"][0], hps["merkle"][0]
        rep["database_root_is_the_merkle_circuits_root"] = bool(np.array_equal(cover.results()[0], merkle.results()))
        rep["index_root_is_the_indexs"] = bool(np.array_equal(cover.results()[1], index.roots()[-1]))
        # 3. the database tree from the forest against the tree builder over the rows
        lp, _ = api.merkle_levels(N)
        d_a, d_b = api.DeviceBuffer(2 * lp * 32), api.DeviceBuffer(2 * lp * 32)
        sizes64 = np.ascontiguousarray(index.sizes, dtype=np.uint64)
        from_forest = lambda: check(index.lib.vdb_ann_index_db_tree_dev(index.d_forest.ptr, api._p(sizes64), index.d_slots.ptr, K, N, d_a.ptr))
        from_rows = lambda: check(index.lib.vdb_merkle_tree_build_dev(index.d_vec.ptr, N, DIM, d_b.ptr))
        from_forest(), from_rows()
        t_f, t_r = [], []
        for _ in range(REPEATS):
            t_f.append(timed(api, from_forest))
            t_r.append(timed(api, from_rows))
        rep["database_tree"] = dict(from_forest_ms=stats(t_f), from_rows_ms=stats(t_r), equal=bool(np.array_equal(d_a.download((2 * lp, 4)), d_b.download((2 * lp, 4)))),
                                    from_forest_launches=launches(api, from_forest)[1], from_rows_launches=launches(api, from_rows)[1])
        d_a.free()
        d_b.free()
        a, b = rep["cover"], rep["merkle"]
        rep["cell_ratio"] = a["cells"] / b["cells"]
        rep["witness_ratio"] = a["witness_ms"]["median"] / b["witness_ms"]["median"]
        held = dict(cells=a["cells"] == EXPECTED["cells"], merkle_cells=b["cells"] == EXPECTED["merkle_cells"],
                    witness=rep["witness_ratio"] <= EXPECTED["witness_ratio_at_most"])
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
        index.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps({k: rep[k] for k in ("cell_ratio", "witness_ratio", "proof_ratio", "expectation_held", "database_root_is_the_merkle_circuits_root") if k in rep}))
    print(json.dumps({"cover_witness_ms": rep["cover"]["witness_ms"]["median"], "merkle_witness_ms": rep["merkle"]["witness_ms"]["median"],
                      "cover_proof_ms": rep["cover"]["proof_ms"] if args.skip_proof else rep["cover"]["proof_ms"]["median"],
                      "merkle_proof_ms": rep["merkle"]["proof_ms"] if args.skip_proof else rep["merkle"]["proof_ms"]["median"],
                      "database_tree_from_forest_ms": rep["database_tree"]["from_forest_ms"]["median"],
                      "database_tree_from_rows_ms": rep["database_tree"]["from_rows_ms"]["median"]}))


if __name__ == "__main__":
    main()
