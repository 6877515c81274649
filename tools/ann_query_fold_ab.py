#!/usr/bin/env python3
"""The single-cluster query at another commit and at this tree (DESIGN §4g "One path"; writes profiles/ann_query_fold_ab.json), at
tools/ann_probe.py's shape and by its method: one process per tree, each with its AnnQueryHotPath set up, keyed and warm; then REPEATS
measurements taken in turn, the other commit first — (a) _witness() between HIP events on the library's stream, (b) wall clock around
prove() with device syncs — and per-kernel times and launch counts from the library's profiler in a pass of their own.  Margin: this
tree's median at most the other's median plus its max - min.  SHA-256 of the stream, the lookup stream and the public values of both.

    python tools/ann_query_fold_ab.py --parent DIR [--out profiles/ann_query_fold_ab.json]      (DIR: a built checkout of the other commit)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPEATS = 5


def worker(root):
    """one tree's side: a JSON line when ready, then one per command read from stdin (run, prof; quit ends)"""
    sys.path[:0] = [root, os.path.join(root, "tools")]
    import ann_probe as AP
    from halo2_vectordb_amd import api, verifier
    from halo2_vectordb_amd.pipeline import AnnIndex, AnnQueryHotPath
    from halo2_vectordb_amd.rounds import ProverRounds

    def say(d):
        print(json.dumps(d), flush=True)

    api.init(0)
    db, ids, cent, query = AP.inputs()
    index = AnnIndex(AP.N, AP.DIM, AP.K, db, ids, cent, P=AP.P, L=AP.L, metric=AP.METRIC)
    hp = AnnQueryHotPath(index, query, k=AP.LOG_ROWS, P=AP.P, L=AP.L, metric=AP.METRIC, tau=AP.TAU).setup()
    pr = ProverRounds(hp).keygen()
    out = pr.prove(None)
    ok = bool(verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"])))
    for _ in range(3):
        hp._witness()
    api.sync()
    sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()[:16]
    say(dict(verified=ok, violations=int(pr.keygen_report.violations()), cells=hp.n_cells, lookups=hp.n_lookup, cluster=int(hp.cluster), n_c=int(hp.n),
             stream=sha(hp.d_stream.download((hp.n_cells, 4))), lookup=sha(hp.d_lookup.download((hp.n_lookup, 4))),
             public=sha(hp.d_pub.download((hp.dim + 1, 4))), proof_bytes=len(out["proof"])))
    for line in sys.stdin:
        if line.strip() == "run":
            w = AP.timed(api, hp._witness)
            api.sync()
            t0 = time.perf_counter()
            pr.prove(None)
            api.sync()
            say(dict(witness_ms=w, proof_ms=(time.perf_counter() - t0) * 1e3))
        elif line.strip() == "prof":
            prof, n = AP.launches(api, hp._witness)
            say(dict(launches=n, kernels=prof))
        else:
            break
    pr.free()
    hp.free()
    index.free()


def ask(p, cmd=None):
    if cmd:
        p.stdin.write(cmd + "\n")
        p.stdin.flush()
    line = p.stdout.readline()
    if not line:
        raise SystemExit(f"a worker ended (exit status {p.wait()})")
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the commit to compare with")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "ann_query_fold_ab.json"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.worker))
    if not args.parent:
        raise SystemExit("--parent DIR is needed")
    from ann_probe import DIM, K, L, LOG_ROWS, METRIC, N, P, stats
    roots = dict(parent=os.path.abspath(args.parent), head=os.path.dirname(HERE))
    procs = {}
    try:
        for name, root in roots.items():
            procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        doc = dict(shape=dict(metric=METRIC, n=N, K=K, dim=DIM, P=P, L=L, k=LOG_ROWS), repeats=REPEATS,
                   timing="two processes on one device, each warm, one measurement each in turn, parent first; witness: HIP events on the library's "
                          "stream around AnnQueryHotPath._witness(); proof: wall clock around prove() with device syncs")
        for name, p in procs.items():
            doc[name] = ask(p)
        runs = {name: [] for name in procs}
        for _ in range(REPEATS):
            for name, p in procs.items():
                runs[name].append(ask(p, "run"))
        for name, p in procs.items():
            prof = ask(p, "prof")
            doc[name].update(witness_ms=stats([r["witness_ms"] for r in runs[name]]), proof_ms=stats([r["proof_ms"] for r in runs[name]]),
                             witness_launches=prof["launches"], witness_kernels_ms=prof["kernels"])
            p.stdin.write("quit\n")
            p.stdin.flush()
        for key in ("witness_ms", "proof_ms"):
            doc[key + "_within_margin"] = bool(doc["head"][key]["median"] <= doc["parent"][key]["median"] + doc["parent"][key]["spread"])
        doc["same_bytes"] = all(doc["parent"][k] == doc["head"][k] for k in ("stream", "lookup", "public", "cells", "lookups", "cluster"))
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
        print(json.dumps({k: doc[k] for k in ("witness_ms_within_margin", "proof_ms_within_margin", "same_bytes")}
                         | {name: {k: doc[name][k]["median"] for k in ("witness_ms", "proof_ms")} | dict(launches=doc[name]["witness_launches"]) for name in procs}))
        if any(p.wait(timeout=60) for p in procs.values()):
            raise SystemExit("a worker failed on its way out")
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()


if __name__ == "__main__":
    main()
