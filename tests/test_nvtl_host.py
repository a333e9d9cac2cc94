"""CPU: the nearest-voxel transformation likelihood entries (ndt_calculate_nvtl, ndt_get_nvtl, ndt_nvtl_poses,
ndt_source_point_count, ndt_source_point_nvtl, ndt_diag_nvtl) -- declared, exported and bound; every refusal that precedes
device work leaves sentinel-filled outputs untouched, so it holds with or without a GPU; no poses is NDT_OK without one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("ndt_calculate_nvtl", "ndt_get_nvtl", "ndt_nvtl_poses", "ndt_source_point_count", "ndt_source_point_nvtl", "ndt_diag_nvtl")
SENTINEL = 7.5


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def szp(a):
    return a.ctypes.data_as(C.POINTER(C.c_size_t))


def eye_table(n):
    return np.ascontiguousarray(np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1)))


def test_entries_are_declared_exported_and_wrapped(mods):
    L, _lib, ndt = mods
    with open(os.path.join(ROOT, "include", "ndt_mi355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\(" % name, header), name + " is not declared in include/ndt_mi355.h"
    for method in ("calculateNVTL", "getNVTL", "nvtlPoses", "sourcePointNVTL", "sourcePointCount", "nvtlLaunches"):
        assert callable(getattr(ndt.NormalDistributionsTransform, method))
    # the accumulated target's equivalence list names the calls
    eq = header[header.index("- Equivalence."):header.index("- _clouds:")]
    for name in ("ndt_calculate_nvtl", "ndt_get_nvtl", "ndt_nvtl_poses", "ndt_source_point_nvtl"):
        assert name in eq


def test_refusals_before_device_work_write_nothing(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    INV = _lib.NDT_ERR_INVALID
    pts = np.zeros((4, 4), np.float32)
    v, nf = C.c_double(SENTINEL), C.c_size_t(99)
    # ndt_calculate_nvtl: NULL handle, NULL nvtl, NULL cloud with points, bad strides
    assert L.ndt_calculate_nvtl(None, pts.ctypes.data, 4, 16, C.byref(v), C.byref(nf)) == INV
    assert L.ndt_calculate_nvtl(g._h, pts.ctypes.data, 4, 16, None, C.byref(nf)) == INV
    assert L.ndt_calculate_nvtl(g._h, None, 4, 16, C.byref(v), C.byref(nf)) == INV
    for stride in (0, 8, 14, 18):
        assert L.ndt_calculate_nvtl(g._h, pts.ctypes.data, 4, stride, C.byref(v), C.byref(nf)) == INV, stride
    # ndt_get_nvtl
    assert L.ndt_get_nvtl(None, C.byref(v), C.byref(nf)) == INV
    assert L.ndt_get_nvtl(g._h, None, C.byref(nf)) == INV
    # ndt_source_point_nvtl / _count
    out, dptr = np.full(4, SENTINEL), C.c_void_p(1234)
    assert L.ndt_source_point_nvtl(None, None, dp(out), C.byref(dptr), C.byref(v), C.byref(nf)) == INV
    assert L.ndt_source_point_count(None, C.byref(nf)) == INV
    assert L.ndt_source_point_count(g._h, None) == INV
    # ndt_nvtl_poses: the handle whatever n_poses is, NULL tables with poses, an all-reduce hook
    T, vals, cnt = eye_table(2), np.full(2, SENTINEL), np.full(2, 99, np.uintp)
    assert L.ndt_nvtl_poses(None, fp(T), 2, dp(vals), szp(cnt)) == INV
    assert L.ndt_nvtl_poses(None, fp(T), 0, dp(vals), szp(cnt)) == INV
    assert L.ndt_nvtl_poses(g._h, None, 2, dp(vals), szp(cnt)) == INV
    assert L.ndt_nvtl_poses(g._h, fp(T), 2, None, szp(cnt)) == INV
    # ndt_diag_nvtl
    a = C.c_size_t(99)
    assert L.ndt_diag_nvtl(None, C.byref(a), C.byref(a)) == INV
    assert L.ndt_diag_nvtl(g._h, None, C.byref(a)) == INV
    assert L.ndt_diag_nvtl(g._h, C.byref(a), None) == INV
    g.setAllreduce(lambda buf, n, on_device: 0)
    assert L.ndt_nvtl_poses(g._h, fp(T), 2, dp(vals), szp(cnt)) == INV
    assert v.value == SENTINEL and nf.value == 99 and a.value == 99 and dptr.value == 1234
    assert list(out) == [SENTINEL] * 4 and list(vals) == [SENTINEL] * 2 and list(cnt) == [99, 99]


def test_no_poses_is_ok_without_a_device(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()   # no target, no source, no device: none is needed
    T, vals, cnt = eye_table(2), np.full(2, SENTINEL), np.full(2, 99, np.uintp)
    assert L.ndt_nvtl_poses(g._h, fp(T), 0, dp(vals), szp(cnt)) == _lib.NDT_OK
    assert L.ndt_nvtl_poses(g._h, None, 0, None, None) == _lib.NDT_OK
    assert list(vals) == [SENTINEL] * 2 and list(cnt) == [99, 99]
    assert g.nvtlPoses([]).shape == (0,)
    v, c = g.nvtlPoses([], counts=True)
    assert v.shape == (0,) and c.shape == (0,)
    assert g.nvtlLaunches() == (0, 0) and g.sourcePointCount() == 0
    r = g.alignMultistart([], 3, metric="nvtl")
    assert r["picked"].shape == (0,) and r["best"] == -1 and r["T"].shape == (0, 4, 4)
    with pytest.raises(ValueError):
        g.alignMultistart([], 3, metric="fitness")


def test_a_valid_call_needs_a_device_then_inputs(mods):
    L, _lib, ndt = mods
    if L.ndt_device_count() >= 1:
        return  # (with a GPU the same calls are tests/test_gpu_nvtl.py's business)
    g = ndt.NormalDistributionsTransform()
    pts = np.zeros((4, 4), np.float32)
    v, nf = C.c_double(SENTINEL), C.c_size_t(99)
    T, vals = eye_table(2), np.full(2, SENTINEL)
    out = np.full(4, SENTINEL)
    assert L.ndt_calculate_nvtl(g._h, pts.ctypes.data, 4, 16, C.byref(v), C.byref(nf)) == _lib.NDT_ERR_NO_DEVICE
    assert L.ndt_get_nvtl(g._h, C.byref(v), C.byref(nf)) == _lib.NDT_ERR_NO_DEVICE
    assert L.ndt_nvtl_poses(g._h, fp(T), 2, dp(vals), None) == _lib.NDT_ERR_NO_DEVICE
    assert L.ndt_source_point_nvtl(g._h, None, dp(out), None, C.byref(v), C.byref(nf)) == _lib.NDT_ERR_NO_DEVICE
    assert v.value == SENTINEL and nf.value == 99 and list(vals) == [SENTINEL] * 2 and list(out) == [SENTINEL] * 4
    with pytest.raises(ndt.NdtError) as e:
        g.nvtlPoses([np.eye(4)])
    assert e.value.status == _lib.NDT_ERR_NO_DEVICE
