#!/usr/bin/env python3
"""What a proved insert / replacement costs beside recommitting the database, measured on the device (writes
profiles/merkle_update.json).  Method of tools/batch_query_probe.py: HIP events, warm, five alternating repeats, the spread recorded;
per-kernel times and launch counts from the library's own event profiler in a pass of their own.  dim = 128:

1. witness — vdb_wit_merkle_update_dev for m in {1, 8, 64, 512} at depth 10 (n = 1,024) and 14 (n = 16,384), in alternation with
   vdb_wit_merkle_dev over the same database on the same card (the existing entry point: what a write costs without the feature),
   and vdb_merkle_tree_build_dev (what keeping the tree resident saves per batch);
2. whole proof — UpdateHotPath(m = 8) against MerkleHotPath of the same 1,024 x 128 database in one process, alternating, both
   verified: ms, proof bytes, column counts, prover stages.

    python tools/merkle_update_probe.py [--out profiles/merkle_update.json] [--skip-proof] [--skip-depth14]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAU = 0x1234567890ABCDEF1234567
DIM, P = 128, 32
REPEATS = 5
VALUE_KERNELS = ("k_mku_touchers", "k_mk_leaf_states", "k_mku_level", "k_mku_writeback")


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), spread=max(xs) - min(xs), runs=xs)


def witness_probe(api, n, ms):
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import sift_like_vectors
    lib = api.init()
    lp, depth = api.merkle_levels(n)
    db, seed = sift_like_vectors(20260005, n, DIM)
    qdb = api.quantize(db, P)
    c = ctypes.c_uint64()
    check(lib.vdb_wit_merkle_size(n, DIM, 0, ctypes.byref(c)))
    merkle_cells = c.value
    sizes = {}
    for m in ms:
        n_in = ctypes.c_uint64()
        check(lib.vdb_wit_merkle_update_size(n, DIM, m, ctypes.byref(c), ctypes.byref(n_in)))
        sizes[m] = c.value
    m_max = max(ms)
    new, _ = sift_like_vectors(seed + 2000, m_max, DIM)
    qnew = api.quantize(new, P)
    rng = np.random.default_rng(seed)
    idx_all = np.ascontiguousarray(rng.integers(0, n, size=m_max), dtype=np.uint64)
    bufs = [api.DeviceBuffer(x) for x in (qdb.nbytes, qnew.nbytes, max(merkle_cells, max(sizes.values())) * 32, 2 * lp * 32, 2 * lp * 32,
                                          (3 * m_max + 2) * 32, 32)]
    d_db, d_new, d_adv, d_lv0, d_lv, d_pub, d_root = bufs
    d_db.upload(qdb)
    d_new.upload(qnew)

    def timed(fn):
        api.sync()
        api.timer_start()
        fn()
        return api.timer_stop()

    def build():
        check(lib.vdb_merkle_tree_build_dev(d_db.ptr, n, DIM, d_lv0.ptr))

    def recommit():
        check(lib.vdb_wit_merkle_dev(d_db.ptr, n, DIM, 0, d_adv.ptr, None, d_root.ptr))

    def update(m):
        def run():
            check(lib.vdb_wit_merkle_update_dev(d_lv.ptr, n, DIM, d_new.ptr, api._p(idx_all[:m]), m, d_adv.ptr, None, d_pub.ptr))
        return run

    def reset():
        check(lib.vdb_memcpy_d2d(d_lv.ptr, d_lv0.ptr, ctypes.c_size_t(2 * lp * 32)))

    try:
        build()
        recommit()
        api.sync()
        same_root = bool(np.array_equal(d_root.download((4,)), d_lv0.download((2 * lp, 4))[2 * lp - 2]))
        ways = dict(recommit=recommit, tree_build=build, **{f"update_{m}": update(m) for m in ms})
        for name, fn in ways.items():                                      # warm
            reset()
            fn()
        api.sync()
        times = {name: [] for name in ways}
        for _ in range(REPEATS):                                           # alternating
            for name, fn in ways.items():
                reset()
                times[name].append(timed(fn))
        kernels = {}
        for name, fn in ways.items():                                      # per-kernel times and launch counts, a pass of its own
            reset()
            api.sync()
            api.profile_begin(deferred=True)
            fn()
            api.sync()
            kernels[name] = api.profile_end()
        rows = []
        rec = stats(times["recommit"])
        for m in ms:
            k = kernels[f"update_{m}"]
            t = stats(times[f"update_{m}"])
            value_ms = sum(k[x]["ms"] for x in VALUE_KERNELS if x in k)
            rows.append(dict(m=m, cells=sizes[m], update_ms=t, kernels_ms=k, launches=int(sum(v["launches"] for v in k.values())),
                             value_pass_ms=value_ms, leaf_states_ms=k.get("k_mk_leaf_states", {}).get("ms"), levels_ms=k.get("k_mku_level", {}).get("ms"),
                             stream_write_GBps=sizes[m] * 32 / (t["median"] * 1e-3) / 1e9, recommit_over_update=rec["median"] / t["median"],
                             recommit_cells_over_update_cells=merkle_cells / sizes[m]))
        return dict(n=n, depth=depth, dim=DIM, recommit=dict(cells=merkle_cells, ms=rec, kernels_ms=kernels["recommit"],
                                                             launches=int(sum(v["launches"] for v in kernels["recommit"].values()))),
                    tree_build=dict(ms=stats(times["tree_build"]), kernels_ms=kernels["tree_build"]), tree_build_root_is_the_commitment=same_root,
                    updates=rows, launches_equal_in_every_row=len({r["launches"] for r in rows}) == 1)
    finally:
        for x in bufs:
            x.free()


def proof_probe(api):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import MerkleHotPath, UpdateHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    hps, made = {}, {}
    for name, ctor in (("merkle", lambda: MerkleHotPath(n=1024, dim=DIM, k=15, P=P, tau=TAU, seed=20260005)),
                       ("update_8", lambda: UpdateHotPath(n=1024, dim=DIM, m=8, k=15, P=P, tau=TAU, seed=20260005))):
        t0 = time.perf_counter()
        hp = ctor().setup()
        pr = ProverRounds(hp).keygen()
        hps[name] = (hp, pr, time.perf_counter() - t0)
    try:
        for name, (hp, pr, _s) in hps.items():
            out = pr.prove(None)                                           # warm
            ok = bool(verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"])))
            made[name] = dict(verified=ok, times=[], proof_bytes=len(out["proof"]), instances=out["instances"])
        for _ in range(REPEATS):                                            # alternating
            for name, (hp, pr, _s) in hps.items():
                api.sync()
                t0 = time.perf_counter()
                pr.prove(None)
                api.sync()
                made[name]["times"].append((time.perf_counter() - t0) * 1e3)
        rep = {}
        for name, (hp, pr, setup_s) in hps.items():
            stages = {}
            pr.prove(None, timings=stages)
            rep[name] = dict(k=hp.k, cells=hp.n_cells, advice_columns=hp.n_adv_cols, public_values=len(made[name]["instances"]), setup_and_keygen_s=setup_s,
                             mock_violations_at_keygen=int(pr.keygen_report.violations()), proof_ms=stats(made[name]["times"]),
                             proof_bytes=made[name]["proof_bytes"], verified=made[name]["verified"], stage_ms=stages)
        a, b = rep["merkle"], rep["update_8"]
        rep["old_root_of_the_update_is_the_commitment"] = bool(made["update_8"]["instances"][0] == made["merkle"]["instances"][0])
        rep["merkle_over_update_proof_ms"] = a["proof_ms"]["median"] / b["proof_ms"]["median"]
        rep["merkle_over_update_cells"] = a["cells"] / b["cells"]
        rep["spread_ms"] = max(a["proof_ms"]["spread"], b["proof_ms"]["spread"])
        return rep
    finally:
        for hp, pr, _s in hps.values():
            pr.free()
            hp.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_update.json"))
    ap.add_argument("--skip-proof", action="store_true")
    ap.add_argument("--skip-depth14", action="store_true")
    args = ap.parse_args()
    from halo2_vectordb_amd import api
    api.init(0)
    doc = dict(shape=dict(dim=DIM, P=P), repeats=REPEATS,
               timing="HIP events on the library's stream (witness); wall clock around prove() with device syncs (proof)",
               witness=[witness_probe(api, n, (1, 8, 64, 512)) for n in ((1024,) if args.skip_depth14 else (1024, 16384))])
    if not args.skip_proof:
        doc["proof"] = proof_probe(api)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    brief = dict(witness=[dict(depth=w["depth"], recommit_ms=w["recommit"]["ms"]["median"], recommit_spread=w["recommit"]["ms"]["spread"],
                               tree_build_ms=w["tree_build"]["ms"]["median"], launches_equal=w["launches_equal_in_every_row"],
                               updates=[dict(m=r["m"], ms=r["update_ms"]["median"], spread=r["update_ms"]["spread"], launches=r["launches"],
                                             value_pass_ms=r["value_pass_ms"], leaf_states_ms=r["leaf_states_ms"], levels_ms=r["levels_ms"],
                                             recommit_over_update=r["recommit_over_update"]) for r in w["updates"]]) for w in doc["witness"]])
    if "proof" in doc:
        pf = doc["proof"]
        brief["proof"] = {name: dict(ms=pf[name]["proof_ms"]["median"], spread=pf[name]["proof_ms"]["spread"], bytes=pf[name]["proof_bytes"],
                                     advice_columns=pf[name]["advice_columns"], verified=pf[name]["verified"]) for name in ("merkle", "update_8")}
        brief["proof"]["merkle_over_update_proof_ms"] = pf["merkle_over_update_proof_ms"]
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
