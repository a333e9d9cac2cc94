"""CPU: the outlier entries (ndt_cloud_neighbor_values, ndt_cloud_remove_outliers, ndt_cloud_remove_outliers_clouds,
ndt_diag_outliers, ndt_host_outlier_spec_check, ndt_host_outlier_plan) -- declared, exported and wrapped; the validity of a
spec field by field; the block plan at its boundaries; every refusal done before any device work, with its outputs untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("ndt_cloud_neighbor_values", "ndt_cloud_remove_outliers", "ndt_cloud_remove_outliers_clouds", "ndt_diag_outliers",
       "ndt_host_outlier_spec_check", "ndt_host_outlier_plan")
SENTINEL = 0x5A5A5A5A
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def spec_of(_lib, **kw):
    base = dict(method=2, negate=0, radius=0.5, min_neighbors=2, mean_k=8, stddev_mul=1.0)
    base.update(kw)
    return _lib.OutlierSpec(**base)


def invalid_specs(_lib):
    bad = [dict(method=0), dict(method=3), dict(method=-1)]
    bad += [dict(method=1, radius=r) for r in (0.0, -1.0, NAN, INF, -INF)]
    bad += [dict(method=1, min_neighbors=-1)]
    bad += [dict(method=2, mean_k=k) for k in (0, -1, 257, 2 ** 31 - 1)]
    bad += [dict(method=2, stddev_mul=m) for m in (NAN, INF, -INF)]
    return [spec_of(_lib, **b) for b in bad]


def test_entries_are_declared_exported_and_wrapped(mods):
    L, _lib, ndt = mods
    with open(os.path.join(ROOT, "include", "ndt_mi355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\(" % name, header), name + " is not declared in include/ndt_mi355.h"
    for method in ("neighborValues", "removeOutliers", "removeOutliersClouds", "outlierDiag", "outlierPlan", "outlierSpecCheck", "outlierSpec"):
        assert callable(getattr(ndt.NormalDistributionsTransform, method))
    assert re.search(r"NDT_OUTLIER_RADIUS = 1\b", header) and _lib.OUTLIER_RADIUS == 1
    assert re.search(r"NDT_OUTLIER_STATISTICAL = 2\b", header) and _lib.OUTLIER_STATISTICAL == 2
    assert C.sizeof(_lib.OutlierSpec) == 32 and _lib.OutlierSpec.stddev_mul.offset == 24 and _lib.OutlierSpec.mean_k.offset == 16
    assert C.sizeof(_lib.OutlierStats) == 40 and _lib.OutlierStats.threshold.offset == 32
    assert "no bit parity with pcl" in header.lower()


def test_spec_check_field_by_field(mods):
    L, _lib, ndt = mods
    check = ndt.NormalDistributionsTransform.outlierSpecCheck
    for s in invalid_specs(_lib):
        assert not check(s), [getattr(s, f) for f, _ in s._fields_]
    assert L.ndt_host_outlier_spec_check(None) == _lib.NDT_ERR_INVALID
    # each method looks at its own fields only
    assert check(spec_of(_lib, method=1, radius=1e-30, min_neighbors=0, mean_k=-5, stddev_mul=NAN))
    assert check(spec_of(_lib, method=1, radius=3e38, min_neighbors=2 ** 31 - 1))
    assert check(spec_of(_lib, method=2, mean_k=1, stddev_mul=-3.0, radius=NAN, min_neighbors=-9))
    assert check(spec_of(_lib, method=2, mean_k=256, stddev_mul=0.0, negate=1))
    g = ndt.NormalDistributionsTransform
    s = g.outlierSpec(radius=0.5, min_neighbors=2, negate=True)
    assert (s.method, s.negate, s.radius, s.min_neighbors) == (1, 1, 0.5, 2) and check(s)
    s = g.outlierSpec(mean_k=20, stddev_mul=1.5)
    assert (s.method, s.negate, s.mean_k, s.stddev_mul) == (2, 0, 20, 1.5) and check(s)
    with pytest.raises(ValueError):
        g.outlierSpec()
    with pytest.raises(ValueError):
        g.outlierSpec(radius=1.0, mean_k=3)


def test_plan_at_its_boundaries(mods):
    L, _lib, ndt = mods
    plan = ndt.NormalDistributionsTransform.outlierPlan
    team, cap = 8, 4096
    assert plan(0) == (0, 0)
    for n, want in ((1, (1, 8)), (7, (1, 8)), (8, (1, 8)), (9, (2, 8)), (16, (2, 8)), (17, (3, 8)),
                    (team * cap - 1, (cap, 8)), (team * cap, (cap, 8)), (team * cap + 1, (cap, 16)), (2 * team * cap, (cap, 16)),
                    (2 * team * cap + 1, (cap, 24)), (2 ** 31 - 1, (cap, 8 * -(-(2 ** 28) // cap)))):
        assert plan(n) == want, (n, plan(n), want)
    for n in list(range(1, 70)) + [team * cap + d for d in range(-9, 10)] + [100000, 2000000, 2 ** 31 - 1]:
        blocks, qpb = plan(n)
        passes = -(-n // team)
        # block b takes the passes b, b + blocks, ...: every pass is taken, no block is idle, and qpb is the busiest block's share
        assert 1 <= blocks <= cap and blocks == min(passes, cap) and qpb == team * -(-passes // blocks)
    b, q = C.c_int(-3), C.c_int(-3)
    assert L.ndt_host_outlier_plan(2 ** 31, C.byref(b), C.byref(q)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_outlier_plan(5, None, C.byref(q)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_outlier_plan(5, C.byref(b), None) == _lib.NDT_ERR_INVALID
    assert (b.value, q.value) == (-3, -3)


class Args:
    """sentinel-filled outputs of the three device entries"""

    def __init__(self, _lib, n=4):
        self.out = C.c_void_p(SENTINEL)
        self.outs = (C.c_void_p * n)(*([SENTINEL] * n))
        self.idx = np.full(n, -7, np.int32)
        self.values = np.full(n, -7.0)
        self.n_kept = C.c_size_t(SENTINEL)
        self.n_kepts = (C.c_size_t * n)(*([SENTINEL] * n))
        self.stats = (_lib.OutlierStats * n)()
        for s in self.stats:
            s.n_finite, s.n_valid, s.mean, s.stddev, s.threshold = SENTINEL, SENTINEL, -7.0, -7.0, -7.0

    def idx_p(self):
        return self.idx.ctypes.data_as(C.POINTER(C.c_int32))

    def val_p(self):
        return C.c_void_p(self.values.ctypes.data)

    def untouched(self, out_null=False, outs_null=0):
        return ((self.out.value is None if out_null else self.out.value == SENTINEL)
                and all(self.outs[k] is None for k in range(outs_null)) and all(self.outs[k] == SENTINEL for k in range(outs_null, len(self.outs)))
                and (self.idx == -7).all() and (self.values == -7.0).all() and self.n_kept.value == SENTINEL
                and all(v == SENTINEL for v in self.n_kepts)
                and all((s.n_finite, s.n_valid, s.mean, s.stddev, s.threshold) == (SENTINEL, SENTINEL, -7.0, -7.0, -7.0) for s in self.stats))


def test_refusals_leave_the_outputs_untouched(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    ok = spec_of(_lib)
    # ndt_cloud_neighbor_values: NULL handle / in / spec / values
    for h, spec_p, values in ((None, C.byref(ok), True), (g._h, C.byref(ok), True), (g._h, None, True), (g._h, C.byref(ok), False)):
        a = Args(_lib)
        st = L.ndt_cloud_neighbor_values(h, None, spec_p, a.val_p() if values else None, 0, a.stats)
        assert st == _lib.NDT_ERR_INVALID and a.untouched()
    # ndt_cloud_remove_outliers: NULL handle / out / in
    a = Args(_lib)
    assert L.ndt_cloud_remove_outliers(None, None, C.byref(ok), C.byref(a.out), a.idx_p(), C.byref(a.n_kept), a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched(out_null=True)
    a = Args(_lib)
    assert L.ndt_cloud_remove_outliers(g._h, None, C.byref(ok), None, a.idx_p(), C.byref(a.n_kept), a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    a = Args(_lib)
    assert L.ndt_cloud_remove_outliers(g._h, None, C.byref(ok), C.byref(a.out), a.idx_p(), C.byref(a.n_kept), a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched(out_null=True)
    # ndt_cloud_remove_outliers_clouds: NULL handle / out / in / spec / entry, too many clouds, an invalid spec
    null_entries = (C.c_void_p * 4)()
    a = Args(_lib)
    assert L.ndt_cloud_remove_outliers_clouds(None, null_entries, 4, C.byref(ok), a.outs, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    assert L.ndt_cloud_remove_outliers_clouds(g._h, null_entries, 4, C.byref(ok), None, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    assert L.ndt_cloud_remove_outliers_clouds(g._h, null_entries, 65536, C.byref(ok), a.outs, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched()                        # (refused before the 65 536 outputs it does not have are written)
    for spec_p, in_p in ((C.byref(ok), None), (None, null_entries), (C.byref(ok), null_entries)):
        a = Args(_lib)
        assert L.ndt_cloud_remove_outliers_clouds(g._h, in_p, 4, spec_p, a.outs, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
        assert a.untouched(outs_null=4)
    for bad in invalid_specs(_lib):
        a = Args(_lib)
        assert L.ndt_cloud_remove_outliers_clouds(g._h, null_entries, 0, C.byref(bad), a.outs, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
        assert a.untouched()
        assert L.ndt_cloud_remove_outliers_clouds(g._h, null_entries, 4, C.byref(bad), a.outs, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
        assert a.untouched(outs_null=4)
    n = C.c_size_t(SENTINEL)
    assert L.ndt_diag_outliers(None, C.byref(n), C.byref(n), C.byref(n), C.byref(n)) == _lib.NDT_ERR_INVALID
    for hole in range(4):
        ptrs = [C.byref(n)] * 4
        ptrs[hole] = None
        assert L.ndt_diag_outliers(g._h, *ptrs) == _lib.NDT_ERR_INVALID and n.value == SENTINEL


def test_no_clouds_is_ok_without_a_device(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    a = Args(_lib)
    assert L.ndt_cloud_remove_outliers_clouds(g._h, None, 0, C.byref(spec_of(_lib)), a.outs, a.n_kepts, a.stats) == _lib.NDT_OK
    assert a.untouched()
    assert g.removeOutliersClouds([], mean_k=8, stddev_mul=1.0) == ([], [])
    assert g.outlierDiag() == dict(index_builds=0, value_launches=0, value_blocks=0, scanned_queries=0)
    assert g.selectDiag() == dict(launches=0, blocks=0, clouds=0)


def test_device_calls_need_a_device(mods):
    L, _lib, ndt = mods
    if L.ndt_device_count() > 0:
        return  # (with a device no cloud-free call gets past the argument checks: tests/test_gpu_outliers.py takes over)
    g = ndt.NormalDistributionsTransform()
    with pytest.raises(ndt.NdtError) as e:
        g.uploadCloud(np.zeros((3, 3), np.float32))  # no cloud can exist here, so the single-cloud entries have nothing to take
    assert e.value.status == _lib.NDT_ERR_NO_DEVICE
