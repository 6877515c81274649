"""The plan of the batch search (halo2_vectordb_amd/csrc/ann_search_plan.hpp through vdb_ann_search_plan, which needs no device): what
k_ann_search and k_ann_search_merge rely on.  Every (query, candidate) pair lies in exactly one task, a task's reported index plus the
base of its partial list is the candidate's place in the query's candidate list, every query's CSR lists are exactly its tasks'
slots, `last` and the (R, C) rule hold — for the dense form over a small grid of (Q, n, t, span) and for the index form with uneven
clusters, an empty one and a cluster several queries share — and every refusal is returned."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def plan():
    from halo2_vectordb_amd import api
    return api.ann_search_plan


def check(pl, Q, t, cand, longest):
    """cand[j]: the rows of the vectors array that are query j's candidates, in candidate-list order; longest: the longest range searched"""
    R, C = pl["R"], pl["C"]
    assert C == next(c for c in (16, 32, 64) if c >= max(t, min(longest, 64))) and R * C == 1024 and R * t <= 1024 and pl["span"] % C == 0
    assert pl["lds_bytes"] >= (R + C) * 16 * 32 + R * t * 36 + R * 8 and pl["lds_bytes"] <= 80 * 1024       # two workgroups a CU
    seen, slots = [dict() for _ in range(Q)], [[] for _ in range(Q)]
    base_of = dict(zip(pl["list_slots"].tolist(), pl["list_base"].tolist()))
    for q_start, q_count, v_lo, v_hi, idx_base, slot0 in pl["tasks"].tolist():
        assert 1 <= q_count <= R and v_lo < v_hi and v_hi - v_lo <= pl["span"]
        for i in range(q_count):
            j = int(pl["order"][q_start + i])
            slots[j].append(slot0 + i)
            for v in range(v_lo, v_hi):
                at = base_of[slot0 + i] + idx_base + (v - v_lo)
                assert at not in seen[j]                                       # one task per (query, candidate)
                seen[j][at] = v
    for j in range(Q):
        assert [seen[j].get(i) for i in range(len(cand[j]))] == list(cand[j]) and len(seen[j]) == len(cand[j])
        assert sorted(pl["list_slots"][pl["list_off"][j]:pl["list_off"][j + 1]].tolist()) == sorted(slots[j])
        assert int(pl["last"][j]) == len(cand[j]) - 1
    assert sorted(sum(slots, [])) == list(range(len(pl["list_slots"])))
    assert pl["work_bytes"] == len(pl["list_slots"]) * (t * 36 + 4) + pl["norm_words"] * 32


@pytest.mark.parametrize("Q", (1, 17, 70))
@pytest.mark.parametrize("n", (1, 16, 17, 65, 130))
def test_dense_tasks_cover_every_pair_once(plan, Q, n):
    for t in sorted({1, min(n, 17), min(n, 64)}):
        for span in (0, 1, 48, n):
            for cus in (1, 256):
                pl = plan("cosine", Q, 3, t, n=n, span=span, cus=cus)
                check(pl, Q, t, [range(n)] * Q, n)
                assert pl["norm_words"] == Q + n and plan("euclidean", Q, 3, t, n=n)["norm_words"] == 0
                if span:
                    assert pl["span"] == -(-max(span, 1) // pl["C"]) * pl["C"]
    many = plan("euclidean", 16, 3, 10, n=1 << 18)                             # few queries, a large database: the split fills the machine
    assert 512 <= len(many["tasks"]) <= 520 and many["span"] >= many["C"]
    assert len(plan("euclidean", 1 << 14, 3, 10, n=1 << 18)["tasks"]) == 1 << 10    # tiles enough: one piece each


def test_probed_tasks_follow_the_clusters(plan):
    sizes = [5, 0, 70, 1, 33, 2]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    rng = np.random.default_rng(5)
    clusters = np.array([rng.permutation([0, 2, 3, 4, 5])[:3] for _ in range(40)] + [[1, 2, 0], [3, 1, 5]])
    cand = [[v for k in row for v in range(offsets[k], offsets[k + 1])] for row in clusters]
    for t, span in ((1, 0), (3, 0), (3, 16), (3, 32), (64, 0)):
        if min(map(len, cand)) < t:
            with pytest.raises(Exception) as e:
                plan("euclidean", len(cand), 3, t, offsets=offsets, clusters=clusters, span=span)
            assert e.value.code == -3
            continue
        pl = plan("cosine", len(cand), 3, t, offsets=offsets, clusters=clusters, span=span, cus=4)
        check(pl, len(cand), t, cand, 70)
        assert pl["norm_words"] == len(cand) + int(offsets[-1])
        for q_start, q_count, v_lo, v_hi, _, _ in pl["tasks"].tolist():        # a task stays inside one cluster, which its queries probe
            k = int(np.searchsorted(offsets, v_lo, side="right")) - 1
            assert v_hi <= offsets[k + 1] and all(k in clusters[j] for j in pl["order"][q_start:q_start + q_count])


def test_refusals(plan):
    from halo2_vectordb_amd.api import VdbError
    big = 1 << 32
    dense = [dict(Q=0, n=2), dict(Q=1, n=0), dict(Q=1, n=2, dim=0), dict(Q=1, n=2, t=0), dict(Q=1, n=100, t=65), dict(Q=1, n=2, t=3),
             dict(Q=big, n=2), dict(Q=1, n=big), dict(Q=1, n=2, dim=(1 << 24) + 1), dict(Q=1 << 20, n=big - 1, span=16)]
    for kw in dense:
        kw = dict(dict(dim=3, t=1), **kw)
        with pytest.raises(VdbError) as e:
            plan("euclidean", kw.pop("Q"), kw.pop("dim"), kw.pop("t"), **kw)
        assert e.value.code == -3, kw
    off = np.array([0, 2, 2, 5])
    for clusters, t, offsets in (([[0, 3]], 1, off), ([[1, 1]], 1, off), ([[0, 1]], 3, off), ([[0, 1, 2, 0]], 1, off), ([[0, 2]], 1, off[::-1])):
        with pytest.raises(VdbError) as e:
            plan("euclidean", 1, 3, t, offsets=offsets, clusters=np.array(clusters))
        assert e.value.code == -3, clusters
    assert plan("hamming", 1, 1 << 24, 64, n=big - 1, span=big)["tasks"].tolist() == [[0, 1, 0, big - 1, 0, 0]]
