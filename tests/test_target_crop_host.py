"""CPU: cropping the accumulating target (ndt_target_accumulate_crop) -- the two entries are declared, exported and wrapped;
every refusal comes with its code and message and without a device; crop_cell_range (the numpy f32 restatement of the cell
range) agrees with brute force on bounds on a cell face and one ulp either side, at the ends of the lattice and at +-inf;
and the float a cropped target carries for a corner cell of its box, (cell + 0.5f) * leaf, floors back to that cell over
the whole lattice, in numpy and through ndt_host_lattice."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

NEW = ("ndt_target_accumulate_crop", "ndt_diag_target_crop")
METHODS = ("targetAccumulateCrop", "targetCropDiag")
LIM = 1 << 20
RESOLUTIONS = (1.0, 0.5, 0.3, 0.1)


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def last_error(L):
    return L.ndt_last_error().decode()


def f3(*v):
    return (C.c_float * 3)(*v)


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
    assert callable(ndt.crop_cell_range)


def test_refusals_come_without_a_device(mods):
    L, _lib, ndt = mods
    lo, hi = f3(0, 0, 0), f3(1, 1, 1)
    assert L.ndt_target_accumulate_crop(None, lo, hi) == _lib.NDT_ERR_INVALID
    assert "null handle" in last_error(L)
    assert L.ndt_diag_target_crop(None, None, None, None, None, None) == _lib.NDT_ERR_INVALID
    assert "null handle" in last_error(L)
    g = ndt.NormalDistributionsTransform()   # no device is asked for
    for a, b in ((None, hi), (lo, None), (None, None)):
        assert L.ndt_target_accumulate_crop(g._h, a, b) == _lib.NDT_ERR_INVALID
        assert "null bounds" in last_error(L)
    nan = float("nan")
    for axis in range(3):
        for which in range(2):
            v = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
            v[which][axis] = nan
            assert L.ndt_target_accumulate_crop(g._h, f3(*v[0]), f3(*v[1])) == _lib.NDT_ERR_INVALID
            assert "NaN" in last_error(L)
        v = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
        v[0][axis] = 2.0
        assert L.ndt_target_accumulate_crop(g._h, f3(*v[0]), f3(*v[1])) == _lib.NDT_ERR_INVALID
        assert "min > max" in last_error(L)
    # well-formed bounds, infinite ones included, but no accumulated target
    inf = float("inf")
    for a, b in ((lo, hi), (f3(-inf, -inf, -inf), f3(inf, inf, inf)), (f3(1, 1, 1), f3(1, 1, 1))):
        assert L.ndt_target_accumulate_crop(g._h, a, b) == _lib.NDT_ERR_NO_INPUT
        assert "no accumulated target" in last_error(L)
    with pytest.raises(_lib.NdtError) as e:
        g.targetAccumulateCrop([0, 0, 0], [1, 1, 1])
    assert e.value.status == _lib.NDT_ERR_NO_INPUT
    assert g.targetCropDiag() == dict(kept_voxels=0, removed_voxels=0, kept_points=0, relinked=False, launches=0)
    assert g.targetAccumulated() == dict(points=0, voxels=0, updates=0)


def brute_cell(bound, resolution):
    """floor of the f32-rounded product bound * (1.0f / resolution), in exact rational arithmetic, saturated"""
    inv = np.float32(1.0) / np.float32(resolution)
    if np.isinf(bound):
        return -LIM if bound < 0 else LIM - 1
    exact = Fraction(float(np.float32(bound))) * Fraction(float(inv))
    # round the exact product to f32 (nearest even): via f64 is safe -- a product of two 24-bit significands is exact in f64
    with np.errstate(over="ignore"):
        p = np.float32(float(exact))
    assert Fraction(float(float(exact))) == exact
    if np.isinf(p):
        return -LIM if p < 0 else LIM - 1
    c = int(np.floor(float(p)))   # floor of a finite f32: exact in Python
    return max(-LIM, min(LIM - 1, c))


@pytest.mark.parametrize("resolution", RESOLUTIONS)
def test_crop_cell_range_agrees_with_brute_force(mods, resolution):
    L, _lib, ndt = mods
    leaf = np.float32(resolution)
    faces = [0, 1, -1, 2, -2, 7, -7, 1000, -1000, 123457, -123457, LIM - 1, -(LIM - 1), LIM, -LIM, LIM + 1, -LIM - 1, 3 * LIM, -3 * LIM]
    bounds = []
    for c in faces:
        on = np.float32(c) * leaf                                   # (about) on the face of cell c
        bounds += [on, np.nextafter(on, np.float32(-np.inf)), np.nextafter(on, np.float32(np.inf))]
        mid = (np.float32(c) + np.float32(0.5)) * leaf
        bounds.append(mid)
    bounds += [np.float32(-np.inf), np.float32(np.inf), np.float32(3e38), np.float32(-3e38), np.float32(1e-45), np.float32(-1e-45)]
    bounds = np.array(bounds, np.float32)
    want = np.array([brute_cell(b, resolution) for b in bounds], np.int64)
    lo, hi = ndt.crop_cell_range(resolution, bounds, bounds)
    assert np.array_equal(lo, want) and np.array_equal(hi, want)
    assert lo.min() == -LIM and lo.max() == LIM - 1                   # both ends of the lattice are reached and saturate
    if resolution in (1.0, 0.5):   # powers of two: the face itself is exact, one ulp below lies in the cell before
        k = bounds.tolist().index(float(np.float32(7) * leaf))
        assert (want[k], want[k + 1], want[k + 2]) == (7, 6, 7)
    # three axes at once, as the entry takes them
    lo3, hi3 = ndt.crop_cell_range(resolution, bounds[:3], bounds[3:6])
    assert np.array_equal(lo3, want[:3]) and np.array_equal(hi3, want[3:6])


@pytest.mark.parametrize("resolution", RESOLUTIONS)
def test_cell_centres_floor_back_to_their_cells(mods, resolution):
    """a cropped target carries its box as (cell + 0.5f) * leaf: lattice_geometry must floor that back to the cell"""
    L, _lib, ndt = mods
    cells = np.arange(-LIM, LIM, dtype=np.int64)
    centre = ndt.crop_cell_centre(resolution, cells)
    assert centre.dtype == np.float32
    inv = np.float32(1.0) / np.float32(resolution)
    prod = centre * inv
    assert prod.dtype == np.float32
    assert np.array_equal(np.floor(prod).astype(np.int64), cells)     # the whole cell range, in the arithmetic that bins a point
    frac = prod.astype(np.float64) - cells
    print("resolution %g: (cell + 0.5) * leaf * inv_leaf - cell within [%.4f, %.4f]" % (resolution, frac.min(), frac.max()))
    assert frac.min() > 0.3 and frac.max() < 0.7                      # the two roundings stay under 0.2 of a cell
    # ... and through the library's own lattice: the ends, the origin and a stride over the range, three cells per call
    rng = np.random.default_rng(3)
    some = np.concatenate([[-LIM, -LIM + 1, -1, 0, 1, LIM - 2, LIM - 1], rng.integers(-LIM, LIM, 1493)])
    for k in range(0, len(some) - 2, 3):
        lo = np.sort(some[k:k + 3])
        hi = np.minimum(lo + [0, 1, 5], LIM - 1)
        got = ndt.host_lattice(resolution, ndt.crop_cell_centre(resolution, lo), ndt.crop_cell_centre(resolution, hi))
        assert got["status"] == _lib.NDT_OK
        assert np.array_equal(got["min_b"], lo) and np.array_equal(got["max_b"], hi), (lo, hi)
