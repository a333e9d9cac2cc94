"""CPU: the argument checks of ndt_align_pairs* (done before any device work, so they hold with or without a GPU) and the
Python side of alignPairs."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def call_pairs(L, h, pts, offsets, n_clouds, pairs, n_pairs, stride=16):
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
    pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
    T = np.zeros((max(n_pairs, 1), 16), np.float32)
    return L.ndt_align_pairs(h, None if pts is None else pts.ctypes.data,
                             None if off is None else off.ctypes.data_as(C.POINTER(C.c_size_t)), n_clouds, stride, 1,
                             None if pr is None else pr.ctypes.data_as(C.POINTER(C.c_int)), n_pairs, None,
                             T.ctypes.data_as(C.POINTER(C.c_float)), None, None, None)


def test_invalid_arguments_are_refused_before_any_device_work(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    pts = np.zeros((30, 4), np.float32)
    ok_off, ok_pairs = [0, 10, 20, 30], [0, 1, 1, 2]
    bad = [
        (pts, None, 3, ok_pairs, 2),               # NULL offsets with clouds
        (pts, ok_off, 3, None, 2),                 # NULL pairs with pairs
        (pts, [0, 10, 5, 30], 3, ok_pairs, 2),     # offsets not monotone
        (pts, ok_off, 3, [0, 1, 1, 3], 2),         # a pair index of n_clouds
        (pts, ok_off, 3, [0, 1, -1, 2], 2),        # ... or below zero
    ]
    for args in bad:
        assert call_pairs(L, g._h, *args) == _lib.NDT_ERR_INVALID, args
    assert call_pairs(L, g._h, pts, ok_off, 3, ok_pairs, 2, stride=10) == _lib.NDT_ERR_INVALID
    T = np.zeros(16, np.float32)
    pr = np.array([0, 1], np.int32)
    assert L.ndt_align_pairs_clouds(g._h, None, 2, 1, pr.ctypes.data_as(C.POINTER(C.c_int)), 1, None,
                                    T.ctypes.data_as(C.POINTER(C.c_float)), None, None, None) == _lib.NDT_ERR_INVALID
    nulls = (C.c_void_p * 2)(None, None)
    assert L.ndt_align_pairs_clouds(g._h, nulls, 2, 1, pr.ctypes.data_as(C.POINTER(C.c_int)), 1, None,
                                    T.ctypes.data_as(C.POINTER(C.c_float)), None, None, None) == _lib.NDT_ERR_INVALID
    # a handle with an all-reduce hook (pairs are not sharded)
    g.setAllreduce(lambda buf, n, on_device: 0)
    assert call_pairs(L, g._h, pts, ok_off, 3, ok_pairs, 2) == _lib.NDT_ERR_INVALID
    # the inspection of a grid no pairs call built
    n = C.c_size_t(0)
    assert L.ndt_pairs_grid_size(g._h, 0, C.byref(n), C.byref(n)) == _lib.NDT_ERR_NO_INPUT


def test_valid_arguments_need_a_device(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    pts = np.random.default_rng(0).uniform(-5, 5, (30, 4)).astype(np.float32)
    st = call_pairs(L, g._h, pts, [0, 10, 20, 30], 3, [0, 1, 1, 2], 2)
    assert st == (_lib.NDT_OK if L.ndt_device_count() >= 1 else _lib.NDT_ERR_NO_DEVICE)
    assert call_pairs(L, g._h, pts, [0, 10, 20, 30], 3, None, 0) == _lib.NDT_OK  # nothing to do


def test_align_pairs_defaults_to_consecutive_pairs(mods):
    L, _lib, ndt = mods
    assert ndt.pairs_array(4).tolist() == [[0, 1], [1, 2], [2, 3]]
    assert ndt.pairs_array(1).shape == (0, 2) and ndt.pairs_array(0).shape == (0, 2)
    assert ndt.pairs_array(3, [(2, 0), (1, 1)]).tolist() == [[2, 0], [1, 1]]
    assert ndt.pairs_array(3).dtype == np.int32 and ndt.pairs_array(3).flags["C_CONTIGUOUS"]
    # what alignPairs hands the library: without a device the consecutive pairs are valid arguments (NO_DEVICE), an index
    # beyond the clouds is not (INVALID)
    if L.ndt_device_count() >= 1:
        return
    g = ndt.NormalDistributionsTransform()
    cl = [np.zeros((5, 3), np.float32) for _ in range(3)]
    with pytest.raises(_lib.NdtError) as e:
        g.alignPairs(cl)
    assert e.value.status == _lib.NDT_ERR_NO_DEVICE
    with pytest.raises(_lib.NdtError) as e:
        g.alignPairs(cl, [(0, 3)])
    assert e.value.status == _lib.NDT_ERR_INVALID


def test_align_pairs_refuses_a_mix_of_resident_and_host_clouds(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    fake = ndt.DeviceCloud(g, None)  # (never handed to the library: the mix is refused first)
    with pytest.raises(ValueError, match="not a mix"):
        g.alignPairs([np.zeros((5, 3), np.float32), fake])
