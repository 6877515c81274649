"""The tile plan of the fused assign (halo2_vectordb_amd/csrc/ann_assign_plan.hpp through vdb_ann_assign_plan, which needs no device): what
k_ann_assign relies on for every dim in 1 .. 4,096 and a few larger ones — the LDS of a workgroup within a CU's 160 KiB, tiles of at
least one row, centroid and word, a grid that covers the n rows exactly once — and the refusals."""
import pytest

DIMS = list(range(1, 4097)) + [4097, 65535, (1 << 20) + 1, 1 << 24]
KS = (1, 2, 15, 16, 17, 32, 33, 64, 65, 1024, 1 << 24)


@pytest.fixture(scope="module")
def plan():
    from halo2_vectordb_amd import api
    return api.ann_assign_plan


def test_tiles_fit_and_the_grid_covers_every_row_once(plan):
    for K in KS:
        for dim in DIMS if K in (2, 1024) else DIMS[:40] + DIMS[-4:]:
            p = plan("cosine", 1000, K, dim)
            R, C, DC = p["R"], p["C"], p["DC"]
            assert p["lds_bytes"] <= 160 * 1024 and R >= 1 and C >= 1 and 1 <= DC <= dim, (K, dim, p)
            assert (R + C) * DC * 32 + R * 36 <= p["lds_bytes"] and R * C * 32 <= p["lds_bytes"]       # the stage, the sums of a chunk, the row minima
            assert C in (16, 32, 64) and R * C == 1024 and (C == 64 or C >= K)                           # a lane's four pairs; few centroids idle few lanes
            assert (p["chunks"] - 1) * C < K <= p["chunks"] * C and (p["dchunks"] - 1) * DC < dim <= p["dchunks"] * DC
            assert p["work_bytes"] == (1000 + K) * 32 and plan("euclidean", 1000, K, dim)["work_bytes"] == 0
    for K in (2, 17, 33):
        R = plan("euclidean", 1, K, 3)["R"]
        for n in (1, 2, R - 1, R, R + 1, 2 * R + 1, (1 << 32) - 1):
            grid = plan("euclidean", n, K, 3)["grid"]
            assert (grid - 1) * R < n <= grid * R and grid < 1 << 31, (n, K)                             # the last tile holds a row, none lies past it


def test_refusals(plan):
    from halo2_vectordb_amd.api import VdbError
    for n, K, dim in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1 << 32, 1, 1), (1, (1 << 24) + 1, 1), (1, 1, (1 << 24) + 1)):
        with pytest.raises(VdbError) as e:
            plan("euclidean", n, K, dim)
        assert e.value.code == -3, (n, K, dim)
    assert plan("hamming", (1 << 32) - 1, 1 << 24, 1 << 24)["grid"] == 1 << 28
