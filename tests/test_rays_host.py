"""CPU: the host side of ndt_target_accumulate_clear_rays* -- the entries are declared, exported and wrapped; every device-free
refusal comes with its code and message; ndt_host_ray_cells (the body the kernel walks with) equals the reference of
tests/ray_cases.py cell for cell on the hand cases, ties included, and on every fixture; the spec check at each bound; the
plan of the ray kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ray_cases as rc
from conftest import ROOT

NEW = ("ndt_target_accumulate_clear_rays", "ndt_target_accumulate_clear_rays_clouds", "ndt_target_accumulate_ray_counts",
       "ndt_diag_target_clear_rays", "ndt_host_ray_spec_check", "ndt_host_ray_cells", "ndt_host_ray_plan")
METHODS = ("targetClearRays", "targetRayCounts", "targetClearRaysDiag")


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
    assert "typedef struct ndt_ray_spec" in header
    for method in METHODS:
        assert callable(getattr(ndt.NormalDistributionsTransform, method))
    assert callable(ndt.ray_cells) and callable(ndt.ray_spec_check) and callable(ndt.host_ray_plan)


@pytest.mark.parametrize("case", range(len(rc.HAND)))
def test_host_ray_cells_on_the_hand_cases(mods, case):
    L, _lib, ndt = mods
    o, p, margin, want = rc.HAND[case]
    got = ndt.ray_cells(o, p, 1.0, margin)
    assert got.dtype == np.int32 and [tuple(int(v) for v in c) for c in got] == (want or [])


@pytest.mark.parametrize("leaf,centre", [(1.0, (0, 0, 0)), (0.3, (0, 0, 0)), (0.7, (0, 0, 0)), (1.5, (0, 0, 0)), (1.0, (1e5, -1e5, 0)), (0.7, (1e5, -1e5, 0))])
def test_host_ray_cells_on_the_fixtures(mods, leaf, centre):
    L, _lib, ndt = mods
    origin, pts = rc.random_rays(5, 1200, leaf, reach=40.0, centre=centre)
    for margin in (0.0, leaf):
        keep = rc.clear_points(pts, origin, leaf, margin=margin)
        w = rc.walk_many(origin, keep, leaf, margin)
        starts = np.concatenate([[0], np.cumsum(w["n"])])
        order = np.argsort(w["ray"], kind="stable")                     # a ray's cells in the order of its steps
        flat = w["cells"][order]
        for i in range(len(keep)):
            got = ndt.ray_cells(origin, keep[i], leaf, margin, capacity=int(w["n"][i]))
            assert np.array_equal(got, flat[starts[i]:starts[i + 1]]), i
    print("leaf %g centre %s: %d rays, %.1f cells per ray, smallest clearance %.3g m" % (leaf, centre, len(keep), w["n"].mean(), w["clearance"].min()))


def test_host_ray_cells_arguments(mods):
    L, _lib, ndt = mods
    f3 = lambda *v: (C.c_float * 3)(*v)   # noqa: E731
    n = C.c_size_t(7)
    cells = (C.c_int * 6)()
    o, p = f3(0.5, 0.5, 0.5), f3(3.5, 0.5, 0.5)
    assert L.ndt_host_ray_cells(None, p, 1.0, 0.0, cells, 2, C.byref(n)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_ray_cells(o, p, 1.0, 0.0, cells, 2, None) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_ray_cells(o, f3(np.nan, 0, 0), 1.0, 0.0, cells, 2, C.byref(n)) == _lib.NDT_ERR_INVALID and "finite" in last_error(L)
    assert L.ndt_host_ray_cells(o, p, 0.0, 0.0, cells, 2, C.byref(n)) == _lib.NDT_ERR_INVALID and "resolution" in last_error(L)
    assert L.ndt_host_ray_cells(o, p, 1.0, -1.0, cells, 2, C.byref(n)) == _lib.NDT_ERR_INVALID and "margin" in last_error(L)
    assert L.ndt_host_ray_cells(o, p, 1.0, 0.0, None, 0, C.byref(n)) == _lib.NDT_OK and n.value == 4      # the count alone
    assert L.ndt_host_ray_cells(o, p, 1.0, 0.0, cells, 2, C.byref(n)) == _lib.NDT_ERR_INVALID and n.value == 4   # too small: the count all the same
    assert "more cells" in last_error(L) and list(cells) == [0, 0, 0, 1, 0, 0]


def test_spec_check_at_each_bound(mods):
    L, _lib, ndt = mods
    ok = dict(min_rays=2, margin=1.0, min_range=0.0, max_range=100.0)

    def check(res=1.0, **kw):
        return ndt.ray_spec_check(res, **dict(ok, **kw))

    assert check() == (True, "")
    assert L.ndt_host_ray_spec_check(None, 1.0) == _lib.NDT_ERR_INVALID and "null ray spec" in last_error(L)
    for name in ("min_range", "max_range", "margin"):
        for bad in (np.nan, np.inf, -np.inf):
            good, why = check(**{name: bad})
            assert not good and "finite" in why, (name, bad)
    assert check(min_range=0.0)[0] and check(min_range=-1e-30) == (False, "a ray spec needs min_range >= 0")
    assert check(min_range=100.0)[0] and check(min_range=np.nextafter(np.float32(100), np.float32(200))) == (False, "a ray spec needs min_range <= max_range")
    assert check(max_range=1e-30)[0] and check(max_range=0.0) == (False, "a ray spec needs max_range > 0")
    assert check(margin=0.0)[0] and check(margin=-1e-30) == (False, "a ray spec needs margin >= 0")
    assert check(min_rays=1)[0] and check(min_rays=0) == (False, "a ray spec needs min_rays >= 1") and not check(min_rays=-3)[0]
    for res in (1.0, 0.5, 0.3, 0.7):
        top = np.float32(65536.0) * np.float32(res)
        if float(top) / float(np.float32(res)) <= 65536.0:
            assert check(res, max_range=top)[0]
        assert ndt.ray_spec_check(res)[0]                                    # the wrapper's default max_range is valid
        beyond = top
        while float(beyond) / float(np.float32(res)) <= 65536.0:
            beyond = np.nextafter(beyond, np.float32(np.inf))
        assert check(res, max_range=beyond) == (False, "a ray spec needs max_range / resolution <= 65536")
    for res in (0.0, -1.0, np.nan, np.inf):
        assert check(res) == (False, "the resolution must be finite and positive")


def test_plan(mods, monkeypatch):
    L, _lib, ndt = mods
    monkeypatch.delenv("NDT_RAYS_MAX_BLOCKS", raising=False)
    assert ndt.host_ray_plan(0) == (0, 0)
    cap = 1024
    for n in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 256 * cap - 1, 256 * cap, 256 * cap + 1, 2 * 256 * cap, 2 * 256 * cap + 1, 2 ** 31 - 1):
        blocks, passes = ndt.host_ray_plan(n)
        assert blocks == min(-(-n // 256), cap) and passes == -(-n // (blocks * 256))
        assert blocks * 256 * passes >= n > blocks * 256 * (passes - 1)
    b, p = C.c_int(0), C.c_int(0)
    assert L.ndt_host_ray_plan(2 ** 31, C.byref(b), C.byref(p)) == _lib.NDT_ERR_INVALID and "INT_MAX" in last_error(L)
    assert L.ndt_host_ray_plan(5, None, C.byref(p)) == _lib.NDT_ERR_INVALID
    monkeypatch.setenv("NDT_RAYS_MAX_BLOCKS", "3")                          # read per call
    assert ndt.host_ray_plan(256 * 3 + 1) == (3, 2) and ndt.host_ray_plan(700) == (3, 1)
    monkeypatch.setenv("NDT_RAYS_MAX_BLOCKS", "100000")                     # never above the built-in cap
    assert ndt.host_ray_plan(256 * 5000) == (cap, 5)


def test_refusals_come_without_a_device(mods):
    L, _lib, ndt = mods
    spec = ndt.ray_spec(1.0)
    one = (C.c_void_p * 1)(None)
    nv = C.c_size_t(9)
    assert L.ndt_target_accumulate_clear_rays(None, None, None, None, C.byref(spec)) == _lib.NDT_ERR_INVALID and "null handle" in last_error(L)
    assert L.ndt_target_accumulate_clear_rays_clouds(None, one, 1, None, None, C.byref(spec)) == _lib.NDT_ERR_INVALID and "null handle" in last_error(L)
    assert L.ndt_target_accumulate_ray_counts(None, one, 1, None, None, C.byref(spec), None, None, None, 0, C.byref(nv)) == _lib.NDT_ERR_INVALID
    assert "null handle" in last_error(L)
    assert L.ndt_diag_target_clear_rays(None, None, None, None, None, None, None, None, None, None) == _lib.NDT_ERR_INVALID and "null handle" in last_error(L)
    g = ndt.NormalDistributionsTransform()   # no device is asked for
    calls = (lambda c, n, P, O, s: L.ndt_target_accumulate_clear_rays_clouds(g._h, c, n, P, O, s),
             lambda c, n, P, O, s: L.ndt_target_accumulate_ray_counts(g._h, c, n, P, O, s, None, None, None, 0, C.byref(nv)))
    for call in calls:
        assert call(one, 1, None, None, None) == _lib.NDT_ERR_INVALID and "null ray spec" in last_error(L)
        assert call(None, 1, None, None, C.byref(spec)) == _lib.NDT_ERR_INVALID and "null clouds" in last_error(L)
        assert call(one, 1, None, None, C.byref(spec)) == _lib.NDT_ERR_INVALID and "null cloud" in last_error(L)
        for bad in (np.nan, np.inf):
            pose = np.eye(4, dtype=np.float32).reshape(16)
            pose[13] = bad
            assert call(one, 1, pose.ctypes.data_as(C.POINTER(C.c_float)), None, C.byref(spec)) == _lib.NDT_ERR_INVALID
            assert "pose" in last_error(L) and "not finite" in last_error(L)
            origin = np.array([0, bad, 0], np.float32)
            assert call(one, 1, None, origin.ctypes.data_as(C.POINTER(C.c_float)), C.byref(spec)) == _lib.NDT_ERR_INVALID
            assert "origin" in last_error(L) and "not finite" in last_error(L)
        # well-formed, but no accumulated target: also for zero clouds
        assert call(None, 0, None, None, C.byref(spec)) == _lib.NDT_ERR_NO_INPUT and "no accumulated target" in last_error(L)
    assert L.ndt_target_accumulate_clear_rays(g._h, None, None, None, C.byref(spec)) == _lib.NDT_ERR_INVALID and "null cloud" in last_error(L)
    with pytest.raises(_lib.NdtError) as e:
        g.targetClearRays([])
    assert e.value.status == _lib.NDT_ERR_NO_INPUT
    with pytest.raises(ValueError):
        g.targetClearRays([np.zeros((3, 3), np.float32)])
    assert g.targetClearRaysDiag() == dict(rays_cast=0, rays_skipped=0, cells_visited=0, touched_voxels=0, removed_voxels=0, kept_voxels=0,
                                           kept_points=0, relinked=False, launches=0)
    assert g.targetAccumulated() == dict(points=0, voxels=0, updates=0)
