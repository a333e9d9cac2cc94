"""CPU: the entry points of GICP's voxel target (gicp_set_input_target_grid, gicp_target_grid_voxels, gicp_diag_target_grid) are
exported with the header's enum values, and every refusal that comes before any device work holds with or without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

NEW = ("gicp_set_input_target_grid", "gicp_target_grid_voxels", "gicp_diag_target_grid")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gicp_mi355.h")


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, gicp, ndt
    return built_lib, _lib, gicp, ndt


def status_of(fn, *args):
    from toyslam_amd import _lib
    try:
        fn(*args)
    except _lib.NdtError as e:
        return e.status, str(e)
    return _lib.NDT_OK, ""


def test_symbols_are_exported_and_listed(mods):
    L, _lib, _, _ = mods
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None


def test_enum_values_match_the_header(mods):
    _, _lib, gicp, _ = mods
    text = open(HEADER).read()
    m = re.search(r"enum\s*\{\s*GICP_VOXEL_COV_PLANE\s*=\s*(\d+)\s*,\s*GICP_VOXEL_COV_RAW\s*=\s*(\d+)\s*\}", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 1)
    assert (_lib.GICP_VOXEL_COV_PLANE, _lib.GICP_VOXEL_COV_RAW) == (0, 1)
    assert gicp.GeneralizedIterativeClosestPoint.VOXEL_COV_MODES == {"plane": 0, "raw": 1}
    for word in ("ascending linear voxel index", "GICP_VOXEL_COV_RAW", "BORROWS", "I - (1 - gicp_epsilon) n n^T"):
        assert word in text, word                                          # the definitions are the contract: they are in the header


def test_binding_refusals_before_any_device_work(mods):
    L, _lib, gicp, ndt = mods
    g = gicp.GeneralizedIterativeClosestPoint()
    m = ndt.NormalDistributionsTransform()
    assert L.gicp_set_input_target_grid(None, m._h, 0) == _lib.NDT_ERR_INVALID            # NULL h
    for mode in (-1, 2, 99):
        assert L.gicp_set_input_target_grid(g._h, m._h, mode) == _lib.NDT_ERR_INVALID     # an unknown cov_mode
    other = ndt.NormalDistributionsTransform(device=1)                                     # (a handle opens no device before it is used)
    assert L.gicp_set_input_target_grid(g._h, other._h, 0) == _lib.NDT_ERR_INVALID
    assert "different devices" in L.ndt_last_error().decode()
    for mode in (_lib.GICP_VOXEL_COV_PLANE, _lib.GICP_VOXEL_COV_RAW):
        assert L.gicp_set_input_target_grid(g._h, m._h, mode) == _lib.NDT_OK               # binding needs neither a device nor a target
    assert L.gicp_set_input_target_grid(g._h, None, 77) == _lib.NDT_OK                     # NULL map drops it, whatever the mode says


def test_refusals_on_a_grid_target(mods):
    L, _lib, gicp, ndt = mods
    g = gicp.GeneralizedIterativeClosestPoint()
    m = ndt.NormalDistributionsTransform()
    g.setInputTargetGrid(m, "raw")
    cov = np.tile(np.eye(3), (4, 1, 1))
    st, msg = status_of(g.setTargetCovariances, cov)
    assert st == _lib.NDT_ERR_INVALID and "grid target" in msg
    buf = np.zeros((4, 9))
    idx, d2 = np.zeros((4, 20), np.int32), np.zeros((4, 20), np.float32)
    dp, ip, fp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_float)
    for a, b in ((idx.ctypes.data_as(ip), d2.ctypes.data_as(fp)), (idx.ctypes.data_as(ip), None), (None, d2.ctypes.data_as(fp))):
        assert L.gicp_covariances(g._h, 0, buf.ctypes.data_as(dp), a, b) == _lib.NDT_ERR_INVALID
        assert "neighbour" in L.ndt_last_error().decode()
    # a source is not needed to be refused: the target is checked first
    T = np.eye(4, dtype=np.float32).reshape(1, 16)
    out = [np.zeros(16, np.float32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1)]
    st = L.gicp_align_guesses(g._h, T.ctypes.data_as(fp), 1, 1.0, out[0].ctypes.data_as(fp), out[1].ctypes.data_as(ip),
                              out[2].ctypes.data_as(ip), out[3].ctypes.data_as(ip), out[4].ctypes.data_as(dp))
    assert st == _lib.NDT_ERR_INVALID and "batch forms take cloud targets" in L.ndt_last_error().decode()
    # use without a target on the map handle: NDT_ERR_NO_INPUT, and no source is an NDT_ERR_NO_INPUT of its own
    st, msg = status_of(g.align)
    assert st == _lib.NDT_ERR_NO_INPUT
    n = C.c_size_t(5)
    assert L.gicp_target_grid_voxels(g._h, None, None, None, 0, C.byref(n)) == _lib.NDT_ERR_NO_INPUT and n.value == 0
    assert "no input target" in L.ndt_last_error().decode()
    assert L.gicp_target_grid_voxels(g._h, None, None, None, 0, None) == _lib.NDT_ERR_INVALID
    assert L.gicp_target_grid_voxels(None, None, None, None, 0, C.byref(n)) == _lib.NDT_ERR_INVALID
    d = g.diagTargetGrid()
    assert d == dict(refreshes=0, voxels=0, excursion=0.0, correspond_blocks=0)
    assert L.gicp_diag_target_grid(None, None, None, None, None) == _lib.NDT_ERR_INVALID
    # dropping the binding: the handle has no target, and the cloud-target calls are as before
    g.setInputTargetGrid(None)
    assert L.gicp_target_grid_voxels(g._h, None, None, None, 0, C.byref(n)) == _lib.NDT_ERR_NO_INPUT
    assert "not a grid target" in L.ndt_last_error().decode()
    st, _ = status_of(g.setTargetCovariances, cov)
    assert st == _lib.NDT_ERR_NO_INPUT                                                     # (set the cloud first: the old message)
