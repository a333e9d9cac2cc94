"""CPU: the accumulating target (ndt_target_accumulate*) -- its entries are declared, exported and wrapped; every refusal
that precedes device work returns its code and message with no device present; the zero-size calls are NDT_OK and need no
device; the key of the voxel table round-trips at the corners of the lattice and refuses one cell outside."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("ndt_target_accumulate", "ndt_target_accumulate_device", "ndt_target_accumulate_cloud", "ndt_target_accumulate_clouds",
       "ndt_target_accumulate_reset", "ndt_target_accumulated", "ndt_diag_target_accumulate", "ndt_host_acc_pack_cell",
       "ndt_host_acc_unpack_cell")
METHODS = ("targetAccumulate", "targetAccumulateDevice", "targetAccumulateCloud", "targetAccumulateClouds", "targetAccumulateReset",
           "targetAccumulated", "targetAccumulateDiag")
LIM = 1 << 20


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def last_error(L):
    return L.ndt_last_error().decode()


def test_entries_are_declared_exported_and_wrapped(mods):
    L, _lib, ndt = mods
    with open(os.path.join(ROOT, "include", "ndt_mi355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\(" % name, header), name + " is not declared in include/ndt_mi355.h"
    for method in METHODS:
        assert callable(getattr(ndt.NormalDistributionsTransform, method))


def test_null_handle_is_refused(mods):
    L, _lib, ndt = mods
    pts = np.zeros((4, 4), np.float32)
    one = (C.c_void_p * 1)(None)
    n = C.c_size_t(0)
    calls = (lambda: L.ndt_target_accumulate(None, pts.ctypes.data, 4, 16, 1, None),
             lambda: L.ndt_target_accumulate_device(None, pts.ctypes.data, 4, 16, 1, None),
             lambda: L.ndt_target_accumulate_cloud(None, None, 1, None),
             lambda: L.ndt_target_accumulate_clouds(None, one, 1, 1, None),
             lambda: L.ndt_target_accumulate_reset(None),
             lambda: L.ndt_target_accumulated(None, C.byref(n), C.byref(n), C.byref(n)),
             lambda: L.ndt_diag_target_accumulate(None, None, None, None, None, None))
    for call in calls:
        assert call() == _lib.NDT_ERR_INVALID
        assert "null handle" in last_error(L)


def test_null_points_and_clouds_are_refused_without_a_device(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    assert L.ndt_target_accumulate(g._h, None, 5, 16, 1, None) == _lib.NDT_ERR_INVALID
    assert "null point buffer" in last_error(L)
    assert L.ndt_target_accumulate_device(g._h, None, 5, 16, 1, None) == _lib.NDT_ERR_INVALID
    assert "null point buffer" in last_error(L)
    assert L.ndt_target_accumulate_clouds(g._h, None, 3, 1, None) == _lib.NDT_ERR_INVALID
    assert "null clouds" in last_error(L)
    entries = (C.c_void_p * 2)(None, None)
    assert L.ndt_target_accumulate_clouds(g._h, entries, 2, 1, None) == _lib.NDT_ERR_INVALID
    assert "null cloud" in last_error(L)
    assert L.ndt_target_accumulate_cloud(g._h, None, 1, None) == _lib.NDT_ERR_INVALID
    assert "null cloud" in last_error(L)
    assert g.targetAccumulated() == dict(points=0, voxels=0, updates=0)


def test_more_than_int_max_points_is_refused_without_a_device(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    pts = np.zeros((4, 4), np.float32)   # never read: the count is refused first
    for call in (L.ndt_target_accumulate, L.ndt_target_accumulate_device):
        assert call(g._h, pts.ctypes.data, (1 << 31), 16, 1, None) == _lib.NDT_ERR_INVALID
        assert "INT_MAX" in last_error(L)
    assert g.targetAccumulated() == dict(points=0, voxels=0, updates=0)


def test_zero_size_calls_are_ok_and_change_nothing(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()   # no device is asked for
    pts = np.zeros((4, 4), np.float32)
    assert L.ndt_target_accumulate(g._h, pts.ctypes.data, 0, 16, 1, None) == _lib.NDT_OK
    assert L.ndt_target_accumulate(g._h, None, 0, 16, 0, None) == _lib.NDT_OK
    assert L.ndt_target_accumulate_device(g._h, None, 0, 16, 1, None) == _lib.NDT_OK
    assert L.ndt_target_accumulate_clouds(g._h, None, 0, 1, None) == _lib.NDT_OK
    assert g.targetAccumulate(np.zeros((0, 3), np.float32)) == dict(points=0, voxels=0, updates=0)
    assert g.targetAccumulateClouds([]) == dict(points=0, voxels=0, updates=0)
    g.targetAccumulateReset()
    assert g.targetAccumulateDiag() == dict(touched_voxels=0, new_voxels=0, relinked=False, table_grown=False, launches=0)
    n = C.c_size_t(7)
    assert L.ndt_grid_size(g._h, C.byref(n), C.byref(n)) == _lib.NDT_ERR_NO_INPUT   # still no target


def test_key_round_trip_at_the_corners(mods):
    L, _lib, ndt = mods
    keys = set()
    for i, j, k in itertools.product((-LIM, -1, 0, 1, LIM - 1), repeat=3):
        key = ndt.host_acc_pack_cell(i, j, k)
        assert key < (1 << 63)                      # all-ones stays free for "no key"
        assert ndt.host_acc_unpack_cell(key) == (i, j, k)
        keys.add(key)
    assert len(keys) == 125
    # keys ascend with the reference's linear voxel index: z outermost, then y, then x
    assert ndt.host_acc_pack_cell(LIM - 1, LIM - 1, 0) < ndt.host_acc_pack_cell(-LIM, -LIM, 1)
    assert ndt.host_acc_pack_cell(LIM - 1, 0, 0) < ndt.host_acc_pack_cell(-LIM, 1, 0)
    assert ndt.host_acc_pack_cell(0, 0, 0) < ndt.host_acc_pack_cell(1, 0, 0)


def test_key_refuses_one_cell_outside(mods):
    L, _lib, ndt = mods
    key = C.c_uint64(123)
    for axis in range(3):
        for v in (LIM, -LIM - 1):
            c = [0, 0, 0]
            c[axis] = v
            assert L.ndt_host_acc_pack_cell(c[0], c[1], c[2], C.byref(key)) == _lib.NDT_ERR_INVALID
            assert "2^20" in last_error(L)
            assert key.value == 123
            with pytest.raises(_lib.NdtError):
                ndt.host_acc_pack_cell(*c)
    assert L.ndt_host_acc_pack_cell(0, 0, 0, None) == _lib.NDT_ERR_INVALID
