"""What a shape reaches in witness.hip's path-update kernels, index-root frame and chain folds: the lane-to-work maps of those kernels and
the grids of their launches restated in Python, so that a test can assert on the host that its shape runs the block, the wavefront,
the LDS trip or the prefetch chunk it is there for, and fails when a later change of a block size takes that away.  Nothing here
computes a cell: the cells are the models' (merkle_update_model, merkle_ops_model, ann_update_model, ann_delete_model) and the oracle's."""
import numpy as np

import topk_model as TM

MAX_UPDATES = 4096            # include/vdb.h VDB_MERKLE_UPDATE_MAX_UPDATES: the entries of k_mku_touchers' LDS table
KM_PF = 8                     # the steps a lane of chain_fold_wave loads ahead of its stores
SMALL_INV = 260               # signed_small_inv: |v| below it comes from the table, from it on through the inverse list


def _blocks(n, size):
    return (n + size - 1) // size


def sponge_perms(words):
    """the permutations of merkle_commitment's sponge over one vector of `words` words"""
    return words // 2 + 1


def path_update_facts(indices, kinds, depth, dim):
    """mku_emit's launches for a batch (kinds None: all writes; 0 a write, anything else an update without a sponge):
    index_blocks / index_last: k_mku_index's blocks of 64 and the updates its last block holds
    level_mixed_waves: the wavefronts of k_mku_level (lane t: update t % m, side t / m) that hold lanes of both sides
    touchers_blocks / fill_trips: k_mku_touchers' blocks of 256 over m * depth lanes, and the trips of its LDS fill (i += 256)
    leaf_blocks / leaf_states_blocks: k_mk_leaf_trace over w * nperm lanes, k_mk_leaf_states over w lanes, blocks of 64
    leaf_straddles: the writes whose permutations lie in two blocks of k_mk_leaf_trace
    from_batch[j]: update j takes its old leaf (prev_same) or its level-0 sibling (sib_from) from an earlier update of the batch
    late_deletes: the updates without a sponge among k_mku_index's lanes of block 1 and up"""
    idx = [int(i) for i in indices]
    m = len(idx)
    kinds = [0] * m if kinds is None else [int(k) for k in kinds]
    w, nperm = kinds.count(0), sponge_perms(dim)
    waves = _blocks(2 * m, 64)
    mixed = [v for v in range(waves) if len({t // m for t in range(64 * v, min(64 * v + 64, 2 * m))}) == 2]
    straddles = [v for v in range(w) if (v * nperm) // 64 != (v * nperm + nperm - 1) // 64]
    from_batch = [any(idx[i] == idx[j] or idx[i] == idx[j] ^ 1 for i in range(j)) for j in range(m)]
    index_blocks = _blocks(m, 64)
    return dict(m=m, w=w, nperm=nperm, index_blocks=index_blocks, index_last=list(range(64 * (index_blocks - 1), m)), level_waves=waves,
                level_mixed_waves=mixed, touchers_blocks=_blocks(m * depth, 256), fill_trips=_blocks(m, 256), leaf_blocks=_blocks(w * nperm, 64) + (w == 0),
                leaf_states_blocks=max(1, _blocks(w, 64)), leaf_straddles=straddles, level_trace_blocks=_blocks(m * depth, 64), from_batch=from_batch,
                late_deletes=[j for j in range(64, m) if kinds[j]])


def frame_facts(K, c, n_public):
    """AnnFrame's launches at K clusters for cluster c, and the public kernel's over n_public values (blocks of 256):
    header_blocks (K + 2 lanes, blocks of 256); indicator_blocks = new_roots_blocks (K lanes, blocks of 64) and the block lane c lies in;
    sponge_perms / sponge_blocks: k_mk_leaf_trace over the permutations of one sponge of K + 1 words"""
    perms = sponge_perms(K + 1)
    return dict(header_blocks=_blocks(K + 2, 256), indicator_blocks=_blocks(K, 64), c_block=c // 64, sponge_perms=perms, sponge_blocks=_blocks(perms, 64),
                public_blocks=_blocks(n_public, 256), public_last_block=(n_public - 1) // 256)


def indicator_off(j):
    """the first cell of indicator j inside block B: indicator 0 is the 8-cell is_zero, every other one the 12-cell is_equal"""
    return 0 if j == 0 else 8 + 12 * (j - 1)


def indicator_inverse(j):
    """the inverse witness of indicator j inside block B: [z, x, inv, ...] of its is_zero"""
    return indicator_off(j) + (2 if j == 0 else 6)


def chain_facts(N):
    """chain_fold_wave over N values: per = ceil(N / 64) steps a lane, lane l owns [lo, hi); chunks[l]: the sizes of the KM_PF-chunks it
    walks; last_live: the last lane that owns a step"""
    per = _blocks(N, 64)
    lanes = [(min(l * per, N), min(l * per + per, N)) for l in range(64)]
    chunks = [[min(KM_PF, hi - v0) for v0 in range(lo, hi, KM_PF)] for lo, hi in lanes]
    return dict(per=per, lanes=lanes, chunks=chunks, last_live=max(l for l, (lo, hi) in enumerate(lanes) if hi > lo))


def sizes_chain(advice, selectors, N, K, P):
    """the first cell of k-means' cluster-size chain in a stream (the first iteration's): the first run of four-cell qadd rows
    [s, x, 1, s + x] with x an indicator (0 or quantization(1.0)), row r >= K continuing row r - K.  It lies behind the per-vector
    blocks; its length must be (N - 1) * K rows exactly"""
    sel = np.asarray(selectors, dtype=np.uint8) & 1
    one = TM.to_limbs([1])[0]
    n = advice.shape[0]
    is_one = (advice == one).all(axis=1)
    rows = np.zeros(n, dtype=bool)
    rows[:n - 3] = (sel[:n - 3] == 1) & (sel[1:n - 2] == 0) & (sel[2:n - 1] == 0) & (sel[3:] == 0) & is_one[2:n - 1]
    want = (N - 1) * K

    def run_from(p):
        """the rows from cell p on that continue the chain"""
        got, prev = 0, []
        while p + 4 <= n and rows[p]:
            s, x, _, t = TM.to_ints(advice[p:p + 4])
            if x not in (0, 1 << P) or t != (s + x) % TM.R or (got >= K and s != prev[got - K]) or (got < K and s not in (0, 1 << P)):
                break
            prev.append(t)
            got += 1
            p += 4
        return got

    behind = 0
    for p in np.flatnonzero(rows):
        if p < behind:
            continue                                             # inside a run already walked
        got = run_from(int(p))
        if got >= min(want, 2 * K):                              # (a stray qadd row of a distance block is a run of one)
            assert got == want, f"the chain at cell {p} has {got} rows, not (N - 1) K = {want}"
            return int(p)
        behind = int(p) + max(1, 4 * got)
    raise AssertionError("no cluster-size chain in the stream")
