"""The Merkle opening circuit as a checker (pipeline.ReadHotPath; include/vdb.h vdb_wit_merkle_open), cell for cell: the old-path half of
merkle_update_model.update_model — the oracle's `merkle_commitment` of one vector for every hash block, the GateChip templates of that
module between them — per read, with the top of every read after the first tied to the top of read 0 (a copy, no cells).

The reads are walked one after the other on build_tree's Python lists, which they leave as they are: nothing here knows how the GPU
batches them.  tests/test_merkle_open_cpu.py holds the model against the oracle.
"""
import numpy as np

from merkle_update_model import _hash_ctx, assert_bit, inner_product_const
from topk_model import row_walk, select, to_ints, to_limbs


def open_model(O, levels, indices, vectors=None, plan_k=None):
    """The closure on the tree `levels` (merkle_update_model.build_tree): slot indices[j] is opened; `vectors` (m, dim, 4): the vectors
    read (vector mode), None: leaf mode, the leaf digest assigned and public.
    -> dict(advice, selectors, break_points, n_in, public: [root | idx, leaf per read | the vectors' words], regions: per read
    dict(block, levels: first cell of every level, index, top: the cell of the path's top), inputs: dict(lead, bits, sibs) first cells,
    ties: [(top of read j, top of read 0)])"""
    m = len(indices)
    lp, depth = len(levels[0]), len(levels) - 1
    assert depth >= 1 and m >= 1 and all(0 <= i < lp for i in indices)
    dim = None if vectors is None else vectors.shape[1]
    n_lead = m if vectors is None else m * dim
    n_in = n_lead + 2 * m * depth
    at = n_in
    leaves, bits_all, sibs_all, blocks, regions, pub = [], [], [], [], [], []
    for j in range(m):
        idx = int(indices[j])
        adv, sel = [], []

        def ctx(c):
            adv.append(c.advice())
            sel.append(c.selectors().astype(np.uint8) & 1)

        def ints(cells, gates):
            adv.append(to_limbs(cells))
            sel.append(np.asarray(gates, dtype=np.uint8))

        reg = dict(block=at, levels=[])
        if vectors is None:
            cur = levels[0][idx].copy()
        else:
            c, cur = _hash_ctx(O, list(vectors[j]))
            ctx(c)
            assert np.array_equal(cur, levels[0][idx]), "the vector read must be the one committed at its slot"
        leaves.append(cur)
        bits, sibs = [], []
        for l in range(depth):
            reg["levels"].append(at + sum(a.shape[0] for a in adv))
            node = idx >> l
            b, sib = node & 1, levels[l][node ^ 1].copy()
            bits.append(b)
            sibs.append(sib)
            (si,), (cu,) = to_ints(sib), to_ints(cur)
            ints(*assert_bit(b))
            cells, gates, lo = select(si, cu, b)
            ints(cells, gates)
            cells, gates, ro = select(cu, si, b)
            ints(cells, gates)
            c, cur = _hash_ctx(O, list(to_limbs([lo, ro])))
            ctx(c)
            assert np.array_equal(cur, levels[l + 1][node >> 1])
        reg["index"] = at + sum(a.shape[0] for a in adv)
        cells, gates, idx_val = inner_product_const(bits, [1 << l for l in range(depth)])
        ints(cells, gates)
        assert idx_val == idx
        bits_all += bits
        sibs_all += sibs
        pub += [to_limbs([idx])[0], leaves[-1]]
        blocks.append((np.concatenate(adv), np.concatenate(sel)))
        # the top: the last hash's squeeze is the last cell of the levels that holds the digest (nothing reads it afterwards)
        top = np.flatnonzero((blocks[-1][0][: reg["index"] - at] == cur).all(axis=1))[-1]
        reg["top"] = at + int(top)
        at += blocks[-1][0].shape[0]
        regions.append(reg)
    lead = np.stack(leaves) if vectors is None else np.ascontiguousarray(vectors).reshape(-1, 4)
    advice = np.concatenate([lead, to_limbs(bits_all), np.stack(sibs_all)] + [b[0] for b in blocks])
    selectors = np.concatenate([np.zeros(n_in, dtype=np.uint8)] + [b[1] for b in blocks])
    assert advice.shape[0] == selectors.shape[0] == at
    public = [levels[depth][0]] + pub + ([] if vectors is None else list(lead))
    return dict(advice=advice, selectors=selectors, break_points=row_walk(selectors, plan_k) if plan_k is not None else None, n_in=n_in,
                public=np.stack(public), regions=regions, inputs=dict(lead=0, bits=n_lead, sibs=n_lead + m * depth),
                ties=[(regions[j]["top"], regions[0]["top"]) for j in range(1, m)])
