"""The maps of the index-root frame placed on the device (circuit_dev.DeviceBuilder) against the numpy builder's, for the three circuits
whose GPU tests do not make that comparison: build_ann_update, build_ann_delete, build_ann_move.  The six arrays, the public cells and
the info dict are equal.  Shapes: K = 3 (is_equal placed for two j at once; the delete and the move leave the last cluster), dim 1,
m = 1; the update appends to a cluster of 2 (depth 2 after one doubling), the delete takes one of 3 members (depth 2, one halving),
the move takes one of 3 members into a cluster of 2 (d_a = 2, s = 1, d_b = 2, g = 1)."""
import functools

import numpy as np
import pytest

from test_gpu_rounds import TAU

pytestmark = pytest.mark.gpu
P, SIZES = 48, (2, 1, 3)


def _rows(seed, n):
    return np.random.default_rng(seed).integers(0, 219, size=(n, 1)).astype(np.float64)


@pytest.fixture(scope="module")
def index():
    from halo2_vectordb_amd import api
    from halo2_vectordb_amd.pipeline import AnnIndex
    api.init(0)
    ix = AnnIndex(sum(SIZES), 1, len(SIZES), _rows(90, sum(SIZES)), np.repeat(np.arange(len(SIZES)), SIZES), _rows(91, len(SIZES)), P=P, L=13)
    yield ix
    ix.free()


def _update(pl, index):
    return pl.AnnUpdateHotPath(index, 0, ([2], _rows(92, 1)), grow=None, k=13, tau=TAU), "build_ann_update", (3, 1, 1, 2), dict(grow=1)


def _delete(pl, index):
    return pl.AnnDeleteHotPath(index, 2, [1], k=13, tau=TAU), "build_ann_delete", (3, 1, 1, 2), dict(shrink=1)


def _move(pl, index):
    return pl.AnnMoveHotPath(index, 2, 0, [1], k=13, tau=TAU), "build_ann_move", (3, 1, 2, 1, 2, 1), {}


@pytest.mark.parametrize("make", [_update, _delete, _move])
def test_device_built_map_is_the_host_built_map(index, make):
    from halo2_vectordb_amd import api, circuit_sym as CS, pipeline
    from halo2_vectordb_amd.circuit_dev import DeviceBuilder
    hp, name, want_shape, want_kw = make(pipeline, index)
    dev = None
    try:
        hp.setup()
        build, shape, kw = hp._map_builder(CS)
        assert (build, tuple(shape), kw) == (getattr(CS, name), want_shape, want_kw)
        d_flags = hp.keygen_flags()
        hp._witness()
        api.sync()
        readers = (functools.partial(hp._fetch_flags, d_flags), hp._fetch)
        host, pub_h, info_h = build(*shape, *readers, builder=None, **kw)
        dev, pub_d, info_d = build(*shape, *readers, builder=DeviceBuilder, **kw)
        d_flags.free()
        assert pub_h == pub_d and info_h == info_d
        assert dev.n_cells == host.n_cells == hp.n_cells and dev.consts == host.consts
        for field in ("copy_of", "const_idx", "gate", "asserted", "lookup_src"):
            assert np.array_equal(getattr(dev, field), getattr(host, field)), field
    finally:
        if dev is not None:
            dev.free()
        hp.free()
