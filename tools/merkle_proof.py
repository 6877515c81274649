#!/usr/bin/env python3
"""merkle_commitment over n x dim vectors at 2^k rows as a whole proof on one MI355X: the Poseidon trace's constraint map (placed on the
device) in the permutation argument, the root public, fresh blinds, Fiat-Shamir transcript, SHPLONK.  Defaults: BASELINE C3
(1,024 x 128, k = 15); `--n 10000 --k 18 --block-cols 126 --ext-block-cols 64` is the database Merkle circuit of BASELINE C5
(1.54 G cells, 5,881 columns: 49 GB of columns, the cosets streamed).
`--circuit query` proves the reference's query circuit instead (examples/query.rs: nearest_vector + merkle_commitment over the same n
vectors, result vector and root public; `--lookup-bits`, `--metric`): e.g. the in-cluster query of BASELINE C5's demo,
`--circuit query --n 5000 --k 18 --lookup-bits 17 --block-cols 126 --ext-block-cols 64`.  With `--queries Q` (Q > 1) the query circuit
holds Q queries against the one database — nearest_vector per query, one merkle_commitment, the Q result vectors and the root public
(pipeline.BatchQueryHotPath); with `--topk T` (T > 1) every query asks for its T nearest vectors, nearest first
(pipeline.TopKQueryHotPath).
`--circuit update --updates M` proves M inserts / replacements against the committed root of the n x dim database instead
(pipeline.UpdateHotPath: M Merkle path updates, [old root | idx, old leaf, new leaf per update | new root] public); `--deletes K` makes
the last K of them deletes (new leaf 0), `--grow G` doubles the padded leaf count G times before the first update (the old root stays
the root before the growth).
`--circuit read --reads M` proves M reads of the committed n x dim database (pipeline.ReadHotPath: M Merkle openings, [root | idx, leaf
per read | the vectors read] public; `--leaf-only`: the leaf digests instead of the vectors, a padding slot showing leaf 0), and has
the verifier check the proof.
`--circuit ann --K C` proves one approximate-nearest-neighbour query against a committed index of the n x dim database
(pipeline.AnnIndex, AnnQueryHotPath: the first C vectors are the centroids, every vector belongs to its nearest one; nearest_vector over
the centroids and over the winning cluster, both commitments, the selected cluster root tied to the members' root, [result | index_root]
public), and has the verifier check the proof.  The circuit's size follows the cluster searched, not n.
With `--probes p` and / or `--topk t` above 1 it proves the t nearest vectors over the p nearest clusters in one proof instead
(pipeline.AnnProbeQueryHotPath: top-k with p rounds over the centroids, with t rounds over the probed clusters' members, one commitment
and one tied root selection per probed cluster, [t results nearest first | index_root] public); the defaults, 1 and 1, are the circuit
above — AnnQueryHotPath is AnnProbeQueryHotPath at these.
`--circuit ann-update --K C --updates M [--grow G]` proves M writes into one cluster of that index against its root
(pipeline.AnnUpdateHotPath: the first write replaces member 0 of the largest cluster, the others append to it; [index_root_old | c | idx, old
leaf, new leaf per write | index_root_new] public; `--grow` defaults to the smallest number of doublings that fits the appends), has the
verifier check the proof and applies the batch to the resident index (AnnIndex.updated), whose root must be the public index_root_new.
`--circuit ann-write --K C --updates M [--appends A]` proves a linked write: M writes into the largest cluster of that index AND the same
M leaf changes in the database tree, in one proof (pipeline.AnnWriteHotPath: the first M - A writes replace members 0, 1, .., the last A
append — default: all but the first; [database_root_old | index_root_old | c | idx, db idx, old leaf, new leaf per write |
database_root_new | index_root_new] public), has the verifier check the proof and writes the batch to the resident index
(AnnIndex.written), whose root must be the public index_root_new and whose database tree must be the tree builder's over the updated
rows with the public database_root_new.  Exit status 0 when all of that holds.
`--circuit ann-delete --K C --deletes M` proves M deletes from the largest cluster of that index (pipeline.AnnDeleteHotPath: slot 0 again and
again, so every delete but the first removes the member the one before moved there; the last member moves into the slot and the cluster's
tree halves when the fill drops to a power of two; [index_root_old | c | slot, removed leaf, last, moved leaf per delete | index_root_new]
public), has the verifier check the proof and removes the batch from the resident index (AnnIndex.removed), whose root must be the
public index_root_new.
`--circuit ann-move --K C --moves M [--src a --dst b]` proves M moves from cluster a (default: the largest) to cluster b (default: the
next one) of that index (pipeline.AnnMoveHotPath: slots 0, 1, .. of a; [index_root_old | a | b | slot, leaf, last, moved leaf, dest, dest old leaf per
move | index_root_new] public; no vector enters the circuit), has the verifier check the proof and moves the batch in the resident
index (AnnIndex.moved), whose root must be the public index_root_new and whose database tree must be the old one.
`--circuit ann-audit --K C [--cluster c]` proves the routing of one cluster of that index (pipeline.AnnAuditHotPath: the database is routed
with AnnIndex.assign, the circuit's own fixed-point rule; every member of cluster c — default: the largest — is at least as close to
centroid c as to any other centroid; [index_root | c] public) and has the verifier check the proof.  Exit status 0 when it is accepted.
`--circuit ann-mean --K C [--cluster c]` proves that centroid c of that index, recentred with AnnIndex.recentred (its centroids are then
AnnIndex.means(), the circuit's own fixed-point means), is the mean of cluster c — default: the largest — (pipeline.AnnMeanHotPath;
[index_root | c] public) and has the verifier check the proof.  Exit status 0 when it is accepted.
`--circuit ann-recentre --K C [--cluster c]` proves the recentre of cluster c of that index — default: the largest — from the old index
root to the new one (pipeline.AnnRecentreHotPath: the centroids' tree with leaf c replaced by the leaf of the members' mean, the cluster
roots carried over; [index_root_old | c | index_root_new] public), has the verifier check the proof and recentres the resident index
(AnnIndex.recentred_with), whose root must be the public index_root_new.  Exit status 0 when both hold.
`--circuit ann-cover --K C` proves that that index holds exactly the committed database (pipeline.AnnCoverHotPath: the multiset of the
database's leaf digests equals the union of the clusters'; [database_root | index_root] public; the cluster sizes are circuit shape),
has the verifier check the proof and holds database_root against the root of the tree builder over the rows.  Exit status 0 when the
proof is accepted and the roots agree."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from halo2_vectordb_amd import api  # noqa: E402
from halo2_vectordb_amd.pipeline import AnnAuditHotPath, AnnCoverHotPath, AnnDeleteHotPath, AnnMeanHotPath, AnnMoveHotPath, AnnRecentreHotPath, AnnIndex, AnnProbeQueryHotPath, AnnUpdateHotPath, AnnWriteHotPath, BatchQueryHotPath, MerkleHotPath, QueryHotPath, ReadHotPath, TopKQueryHotPath, UpdateHotPath  # noqa: E402
from halo2_vectordb_amd.rounds import ProverRounds, quotient_identity_holds  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--k", type=int, default=15)
ap.add_argument("--seed", type=int, default=20260003)
ap.add_argument("--block-cols", type=int, default=510)
ap.add_argument("--ext-block-cols", type=int, default=None)
ap.add_argument("--proofs", type=int, default=2)
ap.add_argument("--circuit", default="merkle", choices=["merkle", "query", "update", "read", "ann", "ann-update", "ann-write", "ann-delete", "ann-move", "ann-audit", "ann-mean", "ann-recentre", "ann-cover"])
ap.add_argument("--lookup-bits", type=int, default=13)
ap.add_argument("--metric", default="euclidean")
ap.add_argument("--queries", type=int, default=1, help="--circuit query: queries proved against the one database in this proof")
ap.add_argument("--topk", type=int, default=1, help="--circuit query / ann: nearest vectors proved per query, nearest first")
ap.add_argument("--probes", type=int, default=1, help="--circuit ann: clusters searched, the nearest centroids' in the order the top-k rounds state them")
ap.add_argument("--updates", type=int, default=8, help="--circuit update: inserts / replacements proved in this proof")
ap.add_argument("--appends", type=int, default=None, help="--circuit ann-write: the last A writes append (default: all but the first)")
ap.add_argument("--deletes", type=int, default=0, help="--circuit update: the last K updates empty their slot instead of writing it; --circuit ann-delete: deletes proved")
ap.add_argument("--moves", type=int, default=8, help="--circuit ann-move: members moved in this proof")
ap.add_argument("--src", type=int, default=None, help="--circuit ann-move: the cluster the members leave (default: the largest)")
ap.add_argument("--dst", type=int, default=None, help="--circuit ann-move: the cluster they arrive in (default: the one after --src)")
ap.add_argument("--grow", type=int, default=None, help="--circuit update / ann-update: doublings of the padded leaf count before the first update")
ap.add_argument("--reads", type=int, default=8, help="--circuit read: slots opened in this proof")
ap.add_argument("--leaf-only", action="store_true", help="--circuit read: reveal the leaf digests, not the vectors")
ap.add_argument("--K", type=int, default=32, help="--circuit ann: clusters of the index")
ap.add_argument("--cluster", type=int, default=None, help="--circuit ann-audit / ann-mean / ann-recentre: the cluster audited or recentred (default: the largest)")
ap.add_argument("--out", default=None, help="write the proof (io.write_snark) and the verifying key beside it")
args = ap.parse_args()

api.init(0)
t0 = time.time()
if args.queries < 1 or (args.queries > 1 and args.circuit != "query"):
    raise SystemExit("--queries needs --circuit query and at least one query")
if args.deletes and args.circuit not in ("update", "ann-delete") or args.grow is not None and args.circuit not in ("update", "ann-update"):
    raise SystemExit("--deletes needs --circuit update or ann-delete, --grow --circuit update or ann-update")
ann_grow, args.grow = args.grow, args.grow or 0
if args.topk < 1 or (args.topk > 1 and args.circuit not in ("query", "ann")):
    raise SystemExit("--topk needs --circuit query or ann and at least one neighbour")
if args.probes < 1 or (args.probes > 1 and args.circuit != "ann"):
    raise SystemExit("--probes needs --circuit ann and at least one cluster")
multi_probe = args.circuit == "ann" and (args.probes > 1 or args.topk > 1)
if args.circuit == "query" and args.topk > 1:
    hp = TopKQueryHotPath(topk=args.topk, q=args.queries, n=args.n, dim=args.dim, k=args.k, L=args.lookup_bits, metric=args.metric, seed=args.seed)
elif args.circuit == "query" and args.queries > 1:
    hp = BatchQueryHotPath(q=args.queries, n=args.n, dim=args.dim, k=args.k, L=args.lookup_bits, metric=args.metric, seed=args.seed)
elif args.circuit == "update":
    if not 0 <= args.deletes <= args.updates or args.grow < 0:
        raise SystemExit("--deletes is between 0 and --updates, --grow is not negative")
    kinds = [0] * (args.updates - args.deletes) + [1] * args.deletes
    hp = UpdateHotPath(n=args.n, dim=args.dim, m=args.updates, k=args.k, seed=args.seed, kinds=kinds, grow=args.grow)
elif args.circuit in ("ann", "ann-update", "ann-write", "ann-delete", "ann-move", "ann-audit", "ann-mean", "ann-recentre", "ann-cover"):
    from halo2_vectordb_amd.pipeline import sift_like_vectors
    if not 1 <= args.K <= args.n:
        raise SystemExit("--K is between 1 and --n")
    db, seed = sift_like_vectors(args.seed, args.n, args.dim)
    query = sift_like_vectors(seed + 1000, 1, args.dim)[0][0]
    ids = np.argmin(((db[:, None, :] - db[None, :args.K, :]) ** 2).sum(axis=2), axis=1)
    ids[:args.K] = np.arange(args.K)                           # (a duplicate of an earlier centroid still keeps its own cluster)
    index = AnnIndex(args.n, args.dim, args.K, db, ids, db[:args.K], L=args.lookup_bits, metric=args.metric)
    if args.circuit == "ann-audit":
        # the clusters the audit can prove are the circuit's own: every row goes where AnnIndex.assign sends it.  The centroids are the
        # first K vectors moved by one in their first word: a member EQUAL to a centroid has distance 0, and the reference's qsqrt(0)
        # violates its own asserted constants, as a query equal to a vector does in the query circuits
        cent = db[:args.K].copy()
        cent[:, 0] += np.where(cent[:, 0] < 218, 1.0, -1.0)
        index.free()
        index = AnnIndex(args.n, args.dim, args.K, db, ids, cent, L=args.lookup_bits, metric=args.metric)
        routed = index.assign(db)
        index.free()
        index = AnnIndex(args.n, args.dim, args.K, db, routed, cent, L=args.lookup_bits, metric=args.metric)
        c = int(np.argmax(index.sizes)) if args.cluster is None else args.cluster
        hp = AnnAuditHotPath(index, c, k=args.k, L=args.lookup_bits, metric=args.metric)
    elif args.circuit == "ann-mean":
        index, built = index.recentred(), index
        built.free()
        c = int(np.argmax(index.sizes)) if args.cluster is None else args.cluster
        hp = AnnMeanHotPath(index, c, k=args.k, L=args.lookup_bits)
    elif args.circuit == "ann-recentre":
        if args.K < 2:
            raise SystemExit("--K is at least 2: a centroids' tree of one leaf has no path")
        c = int(np.argmax(index.sizes)) if args.cluster is None else args.cluster
        hp = AnnRecentreHotPath(index, c, k=args.k, L=args.lookup_bits)
    elif args.circuit == "ann-cover":
        hp = AnnCoverHotPath(index, k=args.k)
    elif args.circuit == "ann":
        hp = AnnProbeQueryHotPath(index, query, probes=args.probes, topk=args.topk, k=args.k, L=args.lookup_bits, metric=args.metric)
    elif args.circuit == "ann-move":
        a = int(np.argmax(index.sizes)) if args.src is None else args.src
        b = (a + 1) % args.K if args.dst is None else args.dst
        if args.K < 2 or not (0 <= a < args.K and 0 <= b < args.K and a != b) or not 1 <= args.moves < int(index.sizes[a]):
            raise SystemExit("--K is at least 2, --src and --dst are two clusters of the index, --moves is at least 1 and leaves --src a member")
        hp = AnnMoveHotPath(index, a, b, list(range(args.moves)), k=args.k)
    elif args.circuit == "ann-delete":
        c = int(np.argmax(index.sizes))
        if not 1 <= args.deletes < int(index.sizes[c]):
            raise SystemExit("--deletes is at least 1 and leaves the largest cluster a member")
        hp = AnnDeleteHotPath(index, c, [0] * args.deletes, k=args.k)
    elif args.circuit == "ann-write":
        c = int(np.argmax(index.sizes))
        app = args.updates - 1 if args.appends is None else args.appends
        if not 0 <= app <= args.updates or args.updates - app > int(index.sizes[c]) or args.updates < 1:
            raise SystemExit("--appends is between 0 and --updates, and the replacements fit the largest cluster")
        slots = list(range(args.updates - app)) + [int(index.sizes[c]) + i for i in range(app)]
        hp = AnnWriteHotPath(index, c, (slots, sift_like_vectors(seed + 2000, args.updates, args.dim)[0]), k=args.k)
    else:
        c = int(np.argmax(index.sizes))
        slots = [0] + [int(index.sizes[c]) + i for i in range(args.updates - 1)]
        hp = AnnUpdateHotPath(index, c, (slots, sift_like_vectors(seed + 2000, args.updates, args.dim)[0]), grow=ann_grow, k=args.k)
elif args.circuit == "read":
    hp = ReadHotPath(n=args.n, dim=args.dim, m=args.reads, k=args.k, seed=args.seed, reveal="leaf" if args.leaf_only else "vector")
elif args.circuit == "query":
    hp = QueryHotPath(n=args.n, dim=args.dim, k=args.k, L=args.lookup_bits, metric=args.metric, seed=args.seed)
else:
    hp = MerkleHotPath(n=args.n, dim=args.dim, k=args.k, seed=args.seed)
hp.ext_block_cols = args.ext_block_cols
hp.setup()
t1 = time.time()
print(json.dumps({"setup_s": round(t1 - t0, 1), "cells": hp.n_cells, "columns": hp.n_cols, "free_GB": round(api.mem_info()[0] / 2**30, 1)}), file=sys.stderr, flush=True)
pr = ProverRounds(hp, block_cols=args.block_cols).keygen()
t2 = time.time()
print(json.dumps({"keygen_s": round(t2 - t1, 1), "mock": pr.keygen_report.as_dict(), "free_GB": round(api.mem_info()[0] / 2**30, 1)}), file=sys.stderr, flush=True)
best = None
for _ in range(args.proofs):
    t3 = time.time()
    out = pr.prove(None)
    api.sync()
    wall = (time.time() - t3) * 1e3
    print(json.dumps({"proof_wall_ms": round(wall, 1)}), file=sys.stderr, flush=True)
    if best is None or wall < best[0]:
        best = (wall, dict(pr.host_ms), out)
wall, host_ms, out = best
T = {}
pr.prove(None, timings=T)
ok = quotient_identity_holds(pr, out["challenges"], out["evals"], out["instances"])
# a read, the audits and the cover (its database root) state the root first, the recentre its new root third, the other circuits last
root_at = 0 if args.circuit in ("read", "ann-audit", "ann-mean", "ann-cover") else 2 if args.circuit == "ann-recentre" else -1
root = api.fr_to_canonical(np.asarray(hp.results() if args.circuit == "merkle" else hp.results()[root_at]).reshape(1, 4))[0]
root_int = int(root[0]) | int(root[1]) << 64 | int(root[2]) << 128 | int(root[3]) << 192
if args.out:
    from halo2_vectordb_amd.io import write_snark
    write_snark(args.out, out["proof"], out["instances"])
    pr.save_verifying_key(args.out + ".vk.npz", opened=out["opened"])
accepted = {}
if args.circuit in ("read", "ann", "ann-update", "ann-write", "ann-delete", "ann-move", "ann-audit", "ann-mean", "ann-recentre", "ann-cover"):
    from halo2_vectordb_amd import verifier
    accepted = {"proof_accepted": bool(verifier.verify(out["proof"], out["instances"], verifier.VerifyingKey.from_prover(pr, out["opened"])))}
if args.circuit == "ann-update":
    index2 = index.updated(hp)
    accepted["applied_index_root_is_the_public_new_root"] = bool(np.array_equal(index2.roots()[-1], hp.results()[-1]))
    index2.free()
if args.circuit == "ann-write":
    index2 = index.written(hp)
    tree2 = index2.database_tree().download((2 * api.merkle_levels(index2.n)[0], 4))
    accepted["written_index_root_is_the_public_new_root"] = bool(np.array_equal(index2.roots()[-1], hp.results()[-1]))
    accepted["database_tree_is_the_tree_builders"] = bool(np.array_equal(tree2, api.merkle_tree_build(index2.qvec)))
    accepted["database_root_is_the_public_new_root"] = bool(np.array_equal(tree2[-2], hp.results()[-2]))
    accepted["old_roots_are_the_indexs"] = bool(np.array_equal(hp.results()[1], index.roots()[-1]) and
                                                np.array_equal(hp.results()[0], api.poseidon_merkle_root(index.qvec)))
    index2.free()
if multi_probe:
    accepted["neighbours"] = hp.neighbours().tolist()
if args.circuit == "ann-audit":
    accepted["members_routed"] = int(hp.results()[2].sum())
if args.circuit == "ann-mean":
    accepted["words_at_the_mean"] = int(hp.results()[2].sum())
if args.circuit == "ann-recentre":
    index2 = index.recentred_with(hp)
    accepted["recentred_root_is_public_root"] = bool(np.array_equal(index2.roots()[-1], hp.results()[2]))
    accepted["root_moved"] = not np.array_equal(hp.results()[0], hp.results()[2])
    index2.free()
if args.circuit == "ann-cover":
    accepted["database_root_is_the_tree_builders"] = bool(np.array_equal(hp.results()[0], api.poseidon_merkle_root(index.qvec)))
    accepted["index_root_is_the_indexs"] = bool(np.array_equal(hp.results()[1], index.roots()[-1]))
if args.circuit == "ann-move":
    index2 = index.moved(hp)
    lp2 = 2 * api.merkle_levels(index.n)[0]
    accepted["moved_index_root_is_the_public_new_root"] = bool(np.array_equal(index2.roots()[-1], hp.results()[-1]))
    accepted["database_tree_is_unchanged"] = bool(np.array_equal(index2.database_tree().download((lp2, 4)), index.database_tree().download((lp2, 4))))
    index2.free()
if args.circuit == "ann-delete":
    index2 = index.removed(hp)
    accepted["removed_index_root_is_the_public_new_root"] = bool(np.array_equal(index2.roots()[-1], hp.results()[-1]))
    index2.free()
what = f"merkle_commitment {args.n}x{args.dim} k={args.k}" if args.circuit == "merkle" else \
    f"{args.updates} Merkle path updates ({args.deletes} deletes, tree grown {args.grow} times) against the root of {args.n}x{args.dim}, k={args.k}" if args.circuit == "update" else \
    f"{args.reads} Merkle openings ({'leaves' if args.leaf_only else 'vectors'} public) against the root of {args.n}x{args.dim}, k={args.k}" if args.circuit == "read" else \
    f"ann query (K={args.K}, the {args.topk} nearest of the {hp.n} vectors of clusters {hp.clusters}, {args.metric}) against the index of {args.n}x{args.dim}, k={args.k}, LOOKUP_BITS={args.lookup_bits}" if multi_probe else \
    f"ann query (K={args.K}, cluster {hp.clusters[0]} of {hp.n} vectors, {args.metric}) against the index of {args.n}x{args.dim}, k={args.k}, LOOKUP_BITS={args.lookup_bits}" if args.circuit == "ann" else \
    f"{args.updates} writes into cluster {hp.cluster} ({hp.n} members, tree grown {hp.grow} times) against the index root (K={args.K}) of {args.n}x{args.dim}, k={args.k}" if args.circuit == "ann-update" else \
    f"{args.updates} linked writes ({hp.appends} appends) into cluster {hp.cluster} ({hp.n} members, tree grown {hp.grow} times) and the database tree (grown {hp.grow_db} times) against both roots (K={args.K}) of {args.n}x{args.dim}, k={args.k}" if args.circuit == "ann-write" else \
    f"routing audit of cluster {hp.cluster} ({hp.n} members, {args.metric}) against the index root (K={args.K}) of {args.n}x{args.dim}, k={args.k}, LOOKUP_BITS={args.lookup_bits}" if args.circuit == "ann-audit" else \
    f"recentre of cluster {hp.cluster} ({hp.n} members) from the old index root to the new (K={args.K}) of {args.n}x{args.dim}, k={args.k}, LOOKUP_BITS={args.lookup_bits}" if args.circuit == "ann-recentre" else \
    f"cover of the database by the index (K={args.K}, cluster sizes {int(index.sizes.min())} .. {int(index.sizes.max())}) of {args.n}x{args.dim}, k={args.k}" if args.circuit == "ann-cover" else \
    f"mean audit of cluster {hp.cluster} ({hp.n} members) against the index root (K={args.K}) of {args.n}x{args.dim}, k={args.k}, LOOKUP_BITS={args.lookup_bits}" if args.circuit == "ann-mean" else \
    f"{args.moves} moves from cluster {hp.src} ({hp.n} members, tree halved {hp.shrink} times) to cluster {hp.dst} ({hp.n_b} members, tree grown {hp.grow} times) against the index root (K={args.K}) of {args.n}x{args.dim}, k={args.k}" if args.circuit == "ann-move" else \
    f"{args.deletes} deletes from cluster {hp.cluster} ({hp.n} members, tree halved {hp.shrink} times) against the index root (K={args.K}) of {args.n}x{args.dim}, k={args.k}" if args.circuit == "ann-delete" else \
    f"query circuit ({str(args.queries) + ' x ' if args.queries > 1 else ''}{'top-' + str(args.topk) + ' ' if args.topk > 1 else ''}nearest_vector {args.metric} + merkle_commitment) over {args.n}x{args.dim}, k={args.k}, LOOKUP_BITS={args.lookup_bits}"
print(json.dumps({"workload": what + ": whole constraint map, public outputs in the instance column, transcript, fresh blinds, SHPLONK", "lookup_cells": hp.n_lookup,
                  "cells": hp.n_cells, "columns": hp.n_cols, "product_sets": pr.n_sets, "mock_report_on_keygen_witness": pr.keygen_report.as_dict(),
                  "setup_s": round(t1 - t0, 1), "keygen_s": round(t2 - t1, 1), "quotient_identity_at_x_holds": bool(ok),
                  "public_root_is_the_hash_only_kernels_root": out["instances"][root_at] == root_int, **accepted, "n_instances": len(out["instances"]), "proof_bytes": len(out["proof"]), "proof_wall_ms": round(wall, 1),
                  "constraints_per_s": round(hp.n_cells / (wall * 1e-3)), "host_transcript_ms": round(host_ms["transcript"], 1),
                  "device_ms": {k: round(v, 2) for k, v in T.items()}, "device_ms_total": round(sum(T.values()), 1),
                  "block_cols": args.block_cols, "ext_cols_held": hp.ext_cols}))
pr.free()
hp.free()
if args.circuit in ("ann", "ann-update", "ann-write", "ann-delete", "ann-move", "ann-audit", "ann-mean", "ann-recentre", "ann-cover"):
    index.free()
if args.circuit == "ann-cover" and not (accepted["database_root_is_the_tree_builders"] and accepted["index_root_is_the_indexs"]):
    sys.exit(1)
if args.circuit in ("ann-audit", "ann-mean", "ann-recentre", "ann-cover") and not accepted["proof_accepted"]:
    sys.exit(1)
if args.circuit == "ann-recentre" and not accepted["recentred_root_is_public_root"]:
    sys.exit(1)
if args.circuit == "ann-write" and not all(accepted.values()):
    sys.exit(1)
if args.circuit == "ann-move" and not (accepted["proof_accepted"] and accepted["moved_index_root_is_the_public_new_root"] and accepted["database_tree_is_unchanged"]):
    sys.exit(1)
