"""CPU: the selection entries (ndt_cloud_select, ndt_cloud_select_clouds, ndt_source_select_by_nvtl, ndt_diag_select,
ndt_host_select_point, ndt_host_select_plan) -- declared, exported and wrapped; the host predicate against the numpy
restatement (tests/select_cases.py); the launch plan; every refusal done before any device work, with its outputs untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import select_cases as sc
from conftest import ROOT

NEW = ("ndt_cloud_select", "ndt_cloud_select_clouds", "ndt_source_select_by_nvtl", "ndt_diag_select", "ndt_host_select_point",
       "ndt_host_select_plan")
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def host_keep(L, _lib, s, p, k=0.0):
    keep = C.c_int(-7)
    xyz = np.ascontiguousarray(p, np.float32)
    st = L.ndt_host_select_point(C.byref(sc.to_ctypes(s, _lib.SelectSpec)), xyz.ctypes.data_as(C.POINTER(C.c_float)), float(k), C.byref(keep))
    return st, keep.value


def test_entries_are_declared_exported_and_wrapped(mods):
    L, _lib, ndt = mods
    with open(os.path.join(ROOT, "include", "ndt_mi355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\(" % name, header), name + " is not declared in include/ndt_mi355.h"
    for method in ("selectCloud", "selectClouds", "sourceSelectByNVTL", "selectDiag", "selectPlan", "selectPoint"):
        assert callable(getattr(ndt.NormalDistributionsTransform, method))
    assert re.search(r"NDT_BOX_ROUTE_SELECT = 9\b", header) and _lib.BOX_ROUTES[9] == "select"
    for name, bit in (("FINITE", 1), ("BOX", 2), ("BOX_NEGATE", 4), ("RANGE", 8), ("RANGE_NEGATE", 16), ("KEY", 32), ("KEY_NEGATE", 64)):
        assert re.search(r"NDT_SELECT_%s = %d\b" % (name, bit), header) and getattr(_lib, "SELECT_" + name) == bit
    assert C.sizeof(_lib.SelectSpec) == 64 and _lib.SelectSpec.key_lo.offset == 48


def test_host_predicate_equals_the_restatement(mods):
    L, _lib, ndt = mods
    rng = np.random.default_rng(20)
    xyz, keys = sc.random_cloud(40, 3, odd_every=3)
    edge_xyz, edge_keys = sc.edge_cloud()
    n_checked = 0
    specs = sc.edge_specs() + [sc.random_spec(rng) for _ in range(60)]
    for s in specs:
        for pts, ks in ((edge_xyz, edge_keys), (xyz, keys)):
            want = sc.keep_mask(s, pts, ks)
            for i in range(pts.shape[0]):
                st, keep = host_keep(L, _lib, s, pts[i], ks[i])
                assert st == _lib.NDT_OK and keep == int(want[i]), (s, pts[i], ks[i])
                n_checked += 1
    assert n_checked > 5000
    # the wrapper, keyword form
    g = ndt.NormalDistributionsTransform
    s = g.selectSpec(finite=True, range=(1, 5))
    assert s.flags == 9 and g.selectPoint(s, (3, 4, 0)) and not g.selectPoint(s, (sc.up(3), 4, 0)) and not g.selectPoint(s, (0, 0, 0))
    s = g.selectSpec(box=sc.BOX_UNIT, box_negate=True, key_range=(0, 1), key_negate=True)
    assert s.flags == 2 | 4 | 32 | 64 and g.selectPoint(s, (9, 9, 9), 2.0) and not g.selectPoint(s, (9, 9, 9), 0.5)


def test_invalid_specs_are_refused(mods):
    L, _lib, ndt = mods
    for s in sc.invalid_specs():
        st, keep = host_keep(L, _lib, s, (0, 0, 0))
        assert st == _lib.NDT_ERR_INVALID and keep == -7, s
    keep = C.c_int(-7)
    p = np.zeros(3, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    ok = sc.to_ctypes(sc.spec(0), _lib.SelectSpec)
    assert L.ndt_host_select_point(None, p, 0.0, C.byref(keep)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_select_point(C.byref(ok), None, 0.0, C.byref(keep)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_select_point(C.byref(ok), p, 0.0, None) == _lib.NDT_ERR_INVALID
    assert keep.value == -7


def plan_steps(cap, block):
    """n = 0, 1, the edges of a wave and a block, and both sides of every point count up to 300 k at which the plan changes"""
    ns = {0, 1, 63, 64, 65, block - 1, block, block + 1, 2 * block, 2 * block + 1, cap * block - 1, cap * block, cap * block + 1}
    for ppb in range(block, 300000 // cap + 2):
        ns |= {cap * ppb, cap * ppb + 1}
    return sorted(ns)


def test_plan_tiles_the_points(mods):
    L, _lib, ndt = mods
    plan = ndt.NormalDistributionsTransform.selectPlan
    cap, block = 1024, 256
    assert plan(0) == (0, block) and plan(1) == (1, block) and plan(block) == (1, block) and plan(block + 1) == (2, block)
    assert plan(cap * block) == (cap, block) and plan(cap * block + 1) == (1021, block + 1)
    last = 0
    for n in plan_steps(cap, block) + [2 ** 31 - 1]:
        blocks, ppb = plan(n)
        assert 0 <= blocks <= cap and ppb >= block and ppb >= last
        last = ppb
        # block b owns [b * ppb, min(n, (b + 1) * ppb)): no block is empty, the last one ends at n
        assert (blocks - 1) * ppb < n <= blocks * ppb or (n == 0 and blocks == 0)
    b, p = C.c_int(-3), C.c_int(-3)
    assert L.ndt_host_select_plan(2 ** 31, C.byref(b), C.byref(p)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_select_plan(5, None, C.byref(p)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_select_plan(5, C.byref(b), None) == _lib.NDT_ERR_INVALID
    assert (b.value, p.value) == (-3, -3)


class Args:
    """sentinel-filled outputs of the three device entries"""

    def __init__(self, n=4):
        self.out = C.c_void_p(SENTINEL)
        self.outs = (C.c_void_p * n)(*([SENTINEL] * n))
        self.idx = np.full(n, -7, np.int32)
        self.n_kept = C.c_size_t(SENTINEL)
        self.n_kepts = (C.c_size_t * n)(*([SENTINEL] * n))
        self.n_found = C.c_size_t(SENTINEL)

    def idx_p(self):
        return self.idx.ctypes.data_as(C.POINTER(C.c_int32))

    def untouched(self, out_null=False, outs_null=0):
        return ((self.out.value is None if out_null else self.out.value == SENTINEL)
                and all(self.outs[k] is None for k in range(outs_null)) and all(self.outs[k] == SENTINEL for k in range(outs_null, len(self.outs)))
                and (self.idx == -7).all() and self.n_kept.value == SENTINEL and all(v == SENTINEL for v in self.n_kepts)
                and self.n_found.value == SENTINEL)


def test_refusals_leave_the_outputs_untouched(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    ok = sc.to_ctypes(sc.spec(sc.FINITE), _lib.SelectSpec)
    keyed = sc.to_ctypes(sc.spec(sc.KEY, key_lo=0, key_hi=1), _lib.SelectSpec)
    keys = np.zeros(4)
    kp = C.c_void_p(keys.ctypes.data)
    # ndt_cloud_select: NULL handle / out / in / spec
    a = Args()
    assert L.ndt_cloud_select(None, None, C.byref(ok), None, 0, C.byref(a.out), a.idx_p(), C.byref(a.n_kept)) == _lib.NDT_ERR_INVALID
    assert a.untouched(out_null=True)
    a = Args()
    assert L.ndt_cloud_select(g._h, None, C.byref(ok), None, 0, None, a.idx_p(), C.byref(a.n_kept)) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    a = Args()
    assert L.ndt_cloud_select(g._h, None, C.byref(ok), None, 0, C.byref(a.out), a.idx_p(), C.byref(a.n_kept)) == _lib.NDT_ERR_INVALID
    assert a.untouched(out_null=True)
    # ndt_cloud_select_clouds: NULL handle / out / in / spec / entry, too many clouds, an invalid spec, KEY
    a = Args()
    null_entries = (C.c_void_p * 4)()
    assert L.ndt_cloud_select_clouds(None, null_entries, 4, C.byref(ok), a.outs, a.n_kepts) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    assert L.ndt_cloud_select_clouds(g._h, null_entries, 4, C.byref(ok), None, a.n_kepts) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    assert L.ndt_cloud_select_clouds(g._h, null_entries, 65536, C.byref(ok), a.outs, a.n_kepts) == _lib.NDT_ERR_INVALID
    assert a.untouched()                        # (refused before the 65 536 outputs it does not have are written)
    for spec_p, in_p in ((C.byref(ok), None), (None, null_entries), (C.byref(ok), null_entries), (C.byref(keyed), null_entries)):
        a = Args()
        assert L.ndt_cloud_select_clouds(g._h, in_p, 4, spec_p, a.outs, a.n_kepts) == _lib.NDT_ERR_INVALID
        assert a.untouched(outs_null=4)
    for s in sc.invalid_specs():
        a = Args()
        bad = sc.to_ctypes(s, _lib.SelectSpec)
        assert L.ndt_cloud_select_clouds(g._h, null_entries, 0, C.byref(bad), a.outs, a.n_kepts) == _lib.NDT_ERR_INVALID
        assert a.untouched()
    # ndt_source_select_by_nvtl: NULL handle / out, a NaN threshold
    a = Args()
    assert L.ndt_source_select_by_nvtl(None, None, 0.5, 1, C.byref(a.out), C.byref(a.n_kept), C.byref(a.n_found)) == _lib.NDT_ERR_INVALID
    assert a.untouched(out_null=True)
    a = Args()
    assert L.ndt_source_select_by_nvtl(g._h, None, 0.5, 1, None, C.byref(a.n_kept), C.byref(a.n_found)) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    a = Args()
    assert L.ndt_source_select_by_nvtl(g._h, None, float("nan"), 1, C.byref(a.out), C.byref(a.n_kept), C.byref(a.n_found)) == _lib.NDT_ERR_INVALID
    assert a.untouched(out_null=True)
    n = C.c_size_t(SENTINEL)
    assert L.ndt_diag_select(None, C.byref(n), C.byref(n), C.byref(n)) == _lib.NDT_ERR_INVALID
    assert L.ndt_diag_select(g._h, None, C.byref(n), C.byref(n)) == _lib.NDT_ERR_INVALID and n.value == SENTINEL
    assert kp.value  # (keys stay alive to here)


def test_no_clouds_is_ok_without_a_device(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    ok = sc.to_ctypes(sc.spec(sc.FINITE), _lib.SelectSpec)
    a = Args()
    assert L.ndt_cloud_select_clouds(g._h, None, 0, C.byref(ok), a.outs, a.n_kepts) == _lib.NDT_OK
    assert a.untouched()
    assert g.selectClouds([], finite=True) == []
    assert g.selectDiag() == dict(launches=0, blocks=0, clouds=0)


def test_device_calls_need_a_device(mods):
    L, _lib, ndt = mods
    have = L.ndt_device_count() > 0
    g = ndt.NormalDistributionsTransform()
    a = Args()
    st = L.ndt_source_select_by_nvtl(g._h, None, 0.5, 1, C.byref(a.out), C.byref(a.n_kept), C.byref(a.n_found))
    # behind the argument checks comes the device, behind the device the inputs (this handle has none)
    assert st == (_lib.NDT_ERR_NO_INPUT if have else _lib.NDT_ERR_NO_DEVICE) and a.untouched(out_null=True)
    if not have:
        with pytest.raises(ndt.NdtError) as e:
            g.uploadCloud(np.zeros((3, 3), np.float32))  # no cloud can exist here, so ndt_cloud_select has nothing to take
        assert e.value.status == _lib.NDT_ERR_NO_DEVICE
