#!/usr/bin/env python3
"""What a proved read costs beside a proved write and beside recommitting the database, measured on the device (writes
profiles/merkle_read.json).  Method of tools/merkle_update_probe.py: HIP events, warm, five alternating repeats, the spread recorded;
per-kernel times and launch counts from the library's own event profiler in a pass of their own.  n = 16,384 (depth 14), dim = 128:

1. witness — vdb_wit_merkle_open_dev for m in {1, 64, 4096} in both modes, in alternation with vdb_wit_merkle_update_dev at the same m
   on the same card (the existing entry point, the yardstick): ms, launches, ns per cell;
2. whole proof — ReadHotPath(m = 64) at 2^18 rows, verified; with --with-merkle also MerkleHotPath over the same 16,384 x 128 database
   (2.40 G cells: minutes of set-up), alternating.

    python tools/merkle_read_probe.py [--out profiles/merkle_read.json] [--skip-proof] [--with-merkle] [--ms 1,64,4096]
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
N, DIM, P = 16384, 128, 32
REPEATS = 5


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), spread=max(xs) - min(xs), runs=xs)


def witness_probe(api, ms):
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import sift_like_vectors
    lib = api.init()
    lp, depth = api.merkle_levels(N)
    db, seed = sift_like_vectors(20260006, N, DIM)
    qdb = api.quantize(db, P)
    m_max = max(ms)
    idx_all = np.ascontiguousarray(np.random.default_rng(seed).integers(0, N, size=m_max), dtype=np.uint64)
    qread = np.ascontiguousarray(qdb[idx_all.astype(np.int64)])
    c, n_in = ctypes.c_uint64(), ctypes.c_uint64()
    sizes = {}
    for m in ms:
        for mode in ("vector", "leaf"):
            check(lib.vdb_wit_merkle_open_size(N, DIM, m, int(mode == "vector"), ctypes.byref(c), ctypes.byref(n_in)))
            sizes[f"read_{mode}_{m}"] = c.value
        check(lib.vdb_wit_merkle_update_size(N, DIM, m, ctypes.byref(c), ctypes.byref(n_in)))
        sizes[f"update_{m}"] = c.value
    bufs = [api.DeviceBuffer(x) for x in (qdb.nbytes, qread.nbytes, max(sizes.values()) * 32, 2 * lp * 32, 2 * lp * 32, (3 * m_max + 2 + m_max * DIM) * 32)]
    d_db, d_read, d_adv, d_lv0, d_lv, d_pub = bufs
    d_db.upload(qdb)
    d_read.upload(qread)

    def timed(fn):
        api.sync()
        api.timer_start()
        fn()
        return api.timer_stop()

    def read(m, mode):
        return lambda: check(lib.vdb_wit_merkle_open_dev(d_lv0.ptr, N, DIM, d_read.ptr if mode == "vector" else None, api._p(idx_all[:m]), m, d_adv.ptr, None,
                                                         d_pub.ptr))

    def update(m):                                            # the rows read serve as the new vectors: the cells' kinds do not depend on the values
        return lambda: check(lib.vdb_wit_merkle_update_dev(d_lv.ptr, N, DIM, d_read.ptr, api._p(idx_all[:m]), m, d_adv.ptr, None, d_pub.ptr))

    def reset():
        check(lib.vdb_memcpy_d2d(d_lv.ptr, d_lv0.ptr, ctypes.c_size_t(2 * lp * 32)))

    try:
        check(lib.vdb_merkle_tree_build_dev(d_db.ptr, N, DIM, d_lv0.ptr))
        ways = {}
        for m in ms:
            ways.update({f"read_vector_{m}": read(m, "vector"), f"read_leaf_{m}": read(m, "leaf"), f"update_{m}": update(m)})
        for fn in ways.values():                                           # warm
            reset()
            fn()
        api.sync()
        times = {name: [] for name in ways}
        for _ in range(REPEATS):                                           # alternating
            for name, fn in ways.items():
                reset()
                times[name].append(timed(fn))
        rows = {}
        for name, fn in ways.items():                                      # per-kernel times and launch counts, a pass of its own
            reset()
            api.sync()
            api.profile_begin(deferred=True)
            fn()
            api.sync()
            k = api.profile_end()
            t = stats(times[name])
            rows[name] = dict(cells=sizes[name], ms=t, ns_per_cell=t["median"] * 1e6 / sizes[name], ns_per_cell_spread=t["spread"] * 1e6 / sizes[name],
                              launches={x: int(v["launches"]) for x, v in k.items()}, kernels_ms={x: v["ms"] for x, v in k.items()})
        return dict(n=N, depth=depth, dim=DIM, rows=rows,
                    read_over_update_ns_per_cell={f"{mode}_{m}": rows[f"read_{mode}_{m}"]["ns_per_cell"] / rows[f"update_{m}"]["ns_per_cell"]
                                                  for m in ms for mode in ("vector", "leaf")})
    finally:
        for x in bufs:
            x.free()


def proof_probe(api, with_merkle):
    from halo2_vectordb_amd import verifier
    from halo2_vectordb_amd.pipeline import MerkleHotPath, ReadHotPath
    from halo2_vectordb_amd.rounds import ProverRounds
    ctors = [("read_64", lambda: ReadHotPath(n=N, dim=DIM, m=64, k=18, P=P, tau=TAU, seed=20260006))]
    if with_merkle:
        ctors.append(("merkle", lambda: MerkleHotPath(n=N, dim=DIM, k=18, P=P, tau=TAU, seed=20260006)))
    hps, made = {}, {}
    try:
        for name, ctor in ctors:
            t0 = time.perf_counter()
            hp = ctor().setup()
            hps[name] = (hp, ProverRounds(hp).keygen(), time.perf_counter() - t0)
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
            rep[name] = dict(k=hp.k, cells=hp.n_cells, advice_columns=hp.n_adv_cols, public_values=len(made[name]["instances"]), setup_and_keygen_s=setup_s,
                             mock_violations_at_keygen=int(pr.keygen_report.violations()), proof_ms=stats(made[name]["times"]),
                             proof_bytes=made[name]["proof_bytes"], verified=made[name]["verified"])
        if with_merkle:
            rep["root_of_the_read_is_the_commitment"] = bool(made["read_64"]["instances"][0] == made["merkle"]["instances"][0])
            rep["merkle_over_read_proof_ms"] = rep["merkle"]["proof_ms"]["median"] / rep["read_64"]["proof_ms"]["median"]
        else:
            rep["merkle"] = "not measured (--with-merkle)"
        return rep
    finally:
        for hp, pr, _s in hps.values():
            pr.free()
            hp.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_read.json"))
    ap.add_argument("--skip-proof", action="store_true")
    ap.add_argument("--with-merkle", action="store_true")
    ap.add_argument("--ms", default="1,64,4096")
    args = ap.parse_args()
    from halo2_vectordb_amd import api
    api.init(0)
    doc = dict(shape=dict(n=N, dim=DIM, P=P), repeats=REPEATS,
               timing="HIP events on the library's stream (witness); wall clock around prove() with device syncs (proof)",
               witness=witness_probe(api, tuple(int(x) for x in args.ms.split(","))))
    if not args.skip_proof:
        doc["proof"] = proof_probe(api, args.with_merkle)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    brief = dict(witness={name: dict(cells=r["cells"], ms=round(r["ms"]["median"], 3), spread=round(r["ms"]["spread"], 3), ns_per_cell=round(r["ns_per_cell"], 4),
                                     launches=sum(r["launches"].values())) for name, r in doc["witness"]["rows"].items()},
                 read_over_update_ns_per_cell=doc["witness"]["read_over_update_ns_per_cell"])
    if "proof" in doc:
        pf = doc["proof"]["read_64"]
        brief["proof_read_64"] = dict(ms=pf["proof_ms"]["median"], spread=pf["proof_ms"]["spread"], bytes=pf["proof_bytes"], advice_columns=pf["advice_columns"],
                                      verified=pf["verified"], mock_violations=pf["mock_violations_at_keygen"])
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
