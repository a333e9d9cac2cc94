"""CPU: the centroid cloud and the centroid fitness (ndt_grid_centroids*, ndt_get_centroid_fitness_score,
ndt_batch_centroid_fitness_scores*, ndt_diag_centroid_fitness) -- the entries are declared, exported, in SIGNATURES and wrapped;
every device-free refusal comes with its code on a handle that never asks for a device, and changes nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("ndt_grid_centroids", "ndt_grid_centroids_cloud", "ndt_get_centroid_fitness_score", "ndt_batch_centroid_fitness_scores",
       "ndt_batch_centroid_fitness_scores_device", "ndt_diag_centroid_fitness")
METHODS = ("gridCentroids", "gridCentroidsCloud", "centroidFitnessScore", "batchCentroidFitness", "centroidFitnessDiag")
INVALID, NO_INPUT = 1, 5
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


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
    assert (_lib.NDT_ERR_INVALID, _lib.NDT_ERR_NO_INPUT) == (INVALID, NO_INPUT)


def batch_args(n_scans=2, pts_per=3):
    pts = np.arange(n_scans * pts_per * 4, dtype=np.float32).reshape(-1, 4)
    off = (np.arange(n_scans + 1) * pts_per).astype(np.uintp)
    T = np.tile(np.eye(4, dtype=np.float32).reshape(16), (max(n_scans, 1), 1))
    out = np.full(max(n_scans, 1), SENTINEL)
    return pts, off, T, out


def call_batch(L, fn, h, pts, off, n_scans, stride, T, out, max_range=1.0):
    szp, fp, dp = C.POINTER(C.c_size_t), C.POINTER(C.c_float), C.POINTER(C.c_double)
    return fn(h, pts.ctypes.data if pts is not None else None, off.ctypes.data_as(szp) if off is not None else None, n_scans, stride,
              T.ctypes.data_as(fp) if T is not None else None, max_range, out.ctypes.data_as(dp) if out is not None else None)


@pytest.mark.parametrize("entry", ["ndt_batch_centroid_fitness_scores", "ndt_batch_centroid_fitness_scores_device"])
def test_batch_refusals_need_no_device_and_change_nothing(mods, entry):
    L, _lib, ndt = mods
    fn = getattr(L, entry)
    g = ndt.NormalDistributionsTransform()
    h = g._h
    before = g.centroidFitnessDiag()
    pts, off, T, out = batch_args()
    assert call_batch(L, fn, None, pts, off, 2, 16, T, out) == INVALID                    # null handle
    assert call_batch(L, fn, h, pts, None, 2, 16, T, out) == INVALID                      # null offsets
    assert call_batch(L, fn, h, pts, off, 2, 16, T, None) == INVALID                      # null fitness
    assert call_batch(L, fn, h, pts, off, 2, 16, None, out) == INVALID                    # null transforms
    assert call_batch(L, fn, h, pts, off[::-1].copy(), 2, 16, T, out) == INVALID          # offsets decrease
    for stride in (8, 14, 0):
        assert call_batch(L, fn, h, pts, off, 2, stride, T, out) == INVALID               # bad stride
    assert call_batch(L, fn, h, None, off, 2, 16, T, out) == INVALID                      # null points with a count
    big = np.zeros(65537, dtype=np.uintp)
    assert call_batch(L, fn, h, pts, big, 65536, 16, T, out) == INVALID                   # more than 65535 scans
    assert "65535" in L.ndt_last_error().decode()
    assert call_batch(L, fn, h, pts, off, 2, 16, T, out) == NO_INPUT                      # no target
    assert "target" in L.ndt_last_error().decode()
    assert call_batch(L, fn, h, pts, off[:1], 0, 16, None, None) == NO_INPUT              # ... even without a scan, as batchFitness
    assert (out == SENTINEL).all()
    assert g.centroidFitnessDiag() == before == dict(launches=0, excursion_passes=0, excursion=0.0, max_blocks=0)


def test_the_other_refusals(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    h = g._h
    n = C.c_size_t(77)
    xyz1 = np.full((4, 4), SENTINEL, dtype=np.float32)
    idx = np.full(4, -9, dtype=np.int64)
    fp, ip64 = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    assert L.ndt_grid_centroids(None, xyz1.ctypes.data_as(fp), idx.ctypes.data_as(ip64), 4, C.byref(n)) == INVALID
    assert L.ndt_grid_centroids(h, xyz1.ctypes.data_as(fp), idx.ctypes.data_as(ip64), 4, None) == INVALID
    assert L.ndt_grid_centroids(h, xyz1.ctypes.data_as(fp), idx.ctypes.data_as(ip64), 4, C.byref(n)) == NO_INPUT
    assert n.value == 77 and (xyz1 == np.float32(SENTINEL)).all() and (idx == -9).all()
    c = C.c_void_p(0x1234)
    assert L.ndt_grid_centroids_cloud(None, C.byref(c)) == INVALID
    assert L.ndt_grid_centroids_cloud(h, None) == INVALID
    assert L.ndt_grid_centroids_cloud(h, C.byref(c)) == NO_INPUT and not c.value          # no cloud comes back
    f = C.c_double(SENTINEL)
    assert L.ndt_get_centroid_fitness_score(None, 1.0, C.byref(f)) == INVALID
    assert L.ndt_get_centroid_fitness_score(h, 1.0, None) == INVALID
    assert L.ndt_get_centroid_fitness_score(h, 1.0, C.byref(f)) == NO_INPUT and f.value == SENTINEL
    assert L.ndt_diag_centroid_fitness(None, None, None, None, None) == INVALID
    assert L.ndt_diag_centroid_fitness(h, None, None, None, None) == 0                    # any pointer may be null
    with pytest.raises(ndt.NdtError) as e:
        g.centroidFitnessScore()
    assert e.value.status == NO_INPUT
    with pytest.raises(ValueError):
        g.batchCentroidFitness([np.zeros((1, 4), np.float32)])                            # one transform per scan
    assert g.targetAccumulated() == dict(points=0, voxels=0, updates=0)
