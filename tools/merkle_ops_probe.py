#!/usr/bin/env python3
"""What deletes and tree growth cost in the update witness, measured on the device (writes profiles/merkle_ops.json).
Method of tools/merkle_update_probe.py: HIP events, warm, five alternating repeats, the spread recorded; per-kernel times and launch
counts from the library's own event profiler in a pass of their own.  dim = 128, depth 10 (n = 1,024) and 14 (n = 16,384):

1. the plain call vdb_wit_merkle_update_dev (m = 64) on this tree, and — with `--parent-tree PATH`, a built checkout of the parent
   commit — the same call there: a child process per tree (`--plain-only`), the two trees' children alternating, their runs pooled;
2. an all-delete batch against an all-write batch of the same m through vdb_wit_merkle_update_ops_dev (expectation: a delete costs
   about what the levels cost, since the leaf hash is gone);
3. vdb_merkle_tree_grow_dev at g = 1 against vdb_merkle_tree_build_dev of the same database.

    python tools/merkle_ops_probe.py [--out profiles/merkle_ops.json] [--parent-tree PATH] [--skip-depth14]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM, P, M, REPEATS, ROUNDS = 128, 32, 64, 5, 3


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), spread=max(xs) - min(xs), runs=xs)


def probe(api, n, plain_only):
    from halo2_vectordb_amd._lib import check
    from halo2_vectordb_amd.pipeline import sift_like_vectors
    lib = api.init()
    lp, depth = api.merkle_levels(n)
    db, seed = sift_like_vectors(20260005, n, DIM)
    new, _ = sift_like_vectors(seed + 2000, M, DIM)
    qdb, qnew = api.quantize(db, P), api.quantize(new, P)
    idx = np.ascontiguousarray(np.random.default_rng(seed).integers(0, n, size=M), dtype=np.uint64)
    writes, deletes = np.zeros(M, dtype=np.uint8), np.ones(M, dtype=np.uint8)
    c, n_in = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.vdb_wit_merkle_update_size(n, DIM, M, ctypes.byref(c), ctypes.byref(n_in)))
    cells = dict(plain=c.value)
    bufs = [api.DeviceBuffer(x) for x in (qdb.nbytes, qnew.nbytes, c.value * 32, 2 * lp * 32, 2 * lp * 32, 4 * lp * 32, (3 * M + 2) * 32)]
    d_db, d_new, d_adv, d_lv0, d_lv, d_grown, d_pub = bufs
    d_db.upload(qdb)
    d_new.upload(qnew)

    def timed(fn):
        api.sync()
        api.timer_start()
        fn()
        return api.timer_stop()

    def build():
        check(lib.vdb_merkle_tree_build_dev(d_db.ptr, n, DIM, d_lv0.ptr))

    def plain():
        check(lib.vdb_wit_merkle_update_dev(d_lv.ptr, n, DIM, d_new.ptr, api._p(idx), M, d_adv.ptr, None, d_pub.ptr))

    def ops(kinds):
        return lambda: check(lib.vdb_wit_merkle_update_ops_dev(d_lv.ptr, n, DIM, 0, d_new.ptr, api._p(idx), api._p(kinds), M, d_adv.ptr, None, d_pub.ptr))

    def grow():
        check(lib.vdb_merkle_tree_grow_dev(d_lv0.ptr, n, 1, d_grown.ptr))

    def reset():
        check(lib.vdb_memcpy_d2d(d_lv.ptr, d_lv0.ptr, ctypes.c_size_t(2 * lp * 32)))

    try:
        build()
        ways = dict(plain=plain)
        if not plain_only:
            ways.update(all_writes=ops(writes), all_deletes=ops(deletes), tree_build=build, tree_grow_1=grow)
            for name, kinds in (("all_writes", writes), ("all_deletes", deletes)):
                check(lib.vdb_wit_merkle_update_ops_size(n, DIM, M, api._p(kinds), 0, ctypes.byref(c), ctypes.byref(n_in)))
                cells[name] = c.value
        for fn in ways.values():                                           # warm
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
        return dict(n=n, depth=depth, dim=DIM, m=M, cells=cells, ms={k: stats(v) for k, v in times.items()}, kernels_ms=kernels)
    finally:
        for x in bufs:
            x.free()


def child(tree, ns):
    """the plain call alone, in a fresh process whose package (and library) is the one of the checkout `tree`"""
    cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--package-root", tree, "--n", ",".join(str(n) for n in ns)]
    return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "merkle_ops.json"))
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its plain call is measured beside this one's")
    ap.add_argument("--skip-depth14", action="store_true")
    ap.add_argument("--plain-only", action="store_true", help="(child) only vdb_wit_merkle_update_dev; one JSON line on stdout")
    ap.add_argument("--package-root", default=HERE, help="(child) the checkout whose package is imported")
    ap.add_argument("--n", default=None, help="(child) database sizes, comma separated")
    args = ap.parse_args()
    ns = [int(x) for x in args.n.split(",")] if args.n else ([1024] if args.skip_depth14 else [1024, 16384])
    if args.plain_only:
        sys.path.insert(0, args.package_root)
        from halo2_vectordb_amd import api
        api.init(0)
        print(json.dumps([dict(n=n, runs=probe(api, n, True)["ms"]["plain"]["runs"]) for n in ns]))
        return
    doc = dict(shape=dict(dim=DIM, P=P, m=M), repeats=REPEATS, timing="HIP events on the library's stream")
    if args.parent_tree:                                                   # before this process opens the device: one process on it at a time
        pooled = {tree: {n: [] for n in ns} for tree in ("parent", "this")}
        for _ in range(ROUNDS):                                            # alternating children
            for tree, path in (("parent", args.parent_tree), ("this", HERE)):
                for row in child(path, ns):
                    pooled[tree][row["n"]] += row["runs"]
        rows = []
        for n in ns:
            a, b = stats(pooled["parent"][n]), stats(pooled["this"][n])
            rows.append(dict(n=n, parent_ms=a, this_ms=b, this_minus_parent_median=b["median"] - a["median"], spread=max(a["spread"], b["spread"]),
                             not_slower_beyond_the_spread=bool(b["median"] - a["median"] <= max(a["spread"], b["spread"]))))
        doc["plain_call_against_parent"] = dict(rounds=ROUNDS, rows=rows)
    sys.path.insert(0, HERE)
    from halo2_vectordb_amd import api
    api.init(0)
    doc["witness"] = [probe(api, n, False) for n in ns]
    for w in doc["witness"]:
        ms, k = w["ms"], w["kernels_ms"]
        w["delete_over_write_ms"] = ms["all_deletes"]["median"] / ms["all_writes"]["median"]
        w["levels_share_of_a_write_batch"] = 1 - (k["all_writes"]["k_mk_leaf_states"]["ms"] + k["all_writes"]["k_mk_leaf_trace"]["ms"]) / \
            sum(v["ms"] for v in k["all_writes"].values())
        w["grow_over_build_ms"] = ms["tree_grow_1"]["median"] / ms["tree_build"]["median"]
        w["ops_all_writes_minus_plain_ms"] = ms["all_writes"]["median"] - ms["plain"]["median"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    brief = dict(plain_call_against_parent=[dict(n=r["n"], parent=r["parent_ms"]["median"], this=r["this_ms"]["median"], spread=r["spread"],
                                                 ok=r["not_slower_beyond_the_spread"]) for r in doc.get("plain_call_against_parent", {}).get("rows", [])],
                 witness=[dict(depth=w["depth"], **{k: round(v["median"], 4) for k, v in w["ms"].items()},
                               spreads={k: round(v["spread"], 4) for k, v in w["ms"].items()}, delete_over_write=w["delete_over_write_ms"],
                               levels_share=w["levels_share_of_a_write_batch"], grow_over_build=w["grow_over_build_ms"]) for w in doc["witness"]])
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
