"""CPU: the normals entries (ndt_cloud_estimate_normals / _clouds, ndt_cloud_select_by_normals / _clouds, ndt_diag_normals,
ndt_host_normal_spec_check / _filter_check / _plan / _from_sums / _keep) -- declared, exported and wrapped; the validity of a spec
and of a filter at each bound; the kernel's plan at its boundaries; every refusal done before any device work, with its outputs
untouched; ndt_host_normal_from_sums, the definition itself, on hand-made inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import normal_cases as nc
from conftest import ROOT

NEW = ("ndt_cloud_estimate_normals", "ndt_cloud_estimate_normals_clouds", "ndt_cloud_select_by_normals", "ndt_cloud_select_by_normals_clouds",
       "ndt_diag_normals", "ndt_host_normal_spec_check", "ndt_host_normal_filter_check", "ndt_host_normal_plan", "ndt_host_normal_from_sums",
       "ndt_host_normal_keep")
SENTINEL = 0x5A5A5A5A
NAN, INF = float("nan"), float("inf")
F = np.float32
fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def spec_of(_lib, method=nc.KNN, k=10, radius=0.5, min_neighbors=3, viewpoint=(0.0, 0.0, 0.0)):
    s = _lib.NormalSpec()
    s.method, s.k, s.radius, s.min_neighbors = method, k, radius, min_neighbors
    s.viewpoint[:] = viewpoint
    return s


def filter_of(_lib, flags=0, curvature=(0.0, 1.0), axis=(0.0, 0.0, 1.0), cos=(0.0, 1.0)):
    f = _lib.NormalFilter()
    f.flags, f.curvature_lo, f.curvature_hi, f.cos_lo, f.cos_hi = flags, curvature[0], curvature[1], cos[0], cos[1]
    f.axis[:] = axis
    return f


def invalid_specs(_lib):
    bad = [dict(method=m) for m in (0, 3, -1)]
    bad += [dict(k=k) for k in (2, 0, -1, 257, 2 ** 31 - 1)]
    bad += [dict(method=nc.RADIUS, radius=r) for r in (0.0, -0.0, -1.0, NAN, INF, -INF)]
    bad += [dict(min_neighbors=m) for m in (2, 0, -5)] + [dict(method=nc.RADIUS, min_neighbors=2)]
    bad += [dict(viewpoint=v) for v in ((NAN, 0, 0), (0, INF, 0), (0, 0, -INF))]
    return [spec_of(_lib, **b) for b in bad]


def invalid_filters(_lib):
    cu, an, ng = nc.KEEP_CURVATURE, nc.KEEP_ANGLE, nc.KEEP_NEGATE
    bad = [dict(flags=8), dict(flags=cu | 16), dict(flags=0x80000000)]
    bad += [dict(flags=cu, curvature=c) for c in ((NAN, 1.0), (0.0, NAN), (0.5, 0.25))]
    bad += [dict(flags=an | ng, cos=c) for c in ((NAN, 1.0), (0.0, NAN), (0.5, 0.25), (-1e-9, 1.0), (0.0, 1.0 + 1e-9))]
    bad += [dict(flags=an, axis=a) for a in ((0, 0, 0), (0, 0, 1.0 + 1e-11), (0, 0, 1.0 - 1e-11), (NAN, 0, 1), (1, 1, 0), (INF, 0, 0))]
    return [filter_of(_lib, **b) for b in bad]


def test_entries_are_declared_exported_and_wrapped(mods):
    L, _lib, ndt = mods
    with open(os.path.join(ROOT, "include", "ndt_mi355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\(" % name, header), name + " is not declared in include/ndt_mi355.h"
    g = ndt.NormalDistributionsTransform
    for method in ("normalSpec", "estimateNormals", "estimateNormalsClouds", "selectByNormals", "selectByNormalsClouds", "normalDiag", "normalPlan",
                   "normalSpecCheck", "normalFilter", "normalFilterCheck"):
        assert callable(getattr(g, method))
    S, T, Fl = _lib.NormalSpec, _lib.NormalStats, _lib.NormalFilter
    assert C.sizeof(S) == 40 and (S.method.offset, S.k.offset, S.radius.offset, S.min_neighbors.offset, S.viewpoint.offset) == (0, 4, 8, 12, 16)
    assert C.sizeof(T) == 32 and (T.n_finite.offset, T.n_valid.offset, T.n_collinear.offset, T.max_neighbors.offset) == (0, 8, 16, 24)
    assert C.sizeof(Fl) == 56 and (Fl.flags.offset, Fl.curvature_lo.offset, Fl.curvature_hi.offset, Fl.axis.offset, Fl.cos_lo.offset, Fl.cos_hi.offset) == (
        0, 4, 8, 16, 40, 48)
    assert (_lib.NORMAL_KNN, _lib.NORMAL_RADIUS) == (1, 2) and (_lib.NORMAL_KEEP_CURVATURE, _lib.NORMAL_KEEP_ANGLE, _lib.NORMAL_KEEP_NEGATE) == (1, 2, 4)
    for const in ("NDT_NORMAL_KNN = 1", "NDT_NORMAL_RADIUS = 2", "NDT_NORMAL_KEEP_CURVATURE = 1", "NDT_NORMAL_KEEP_ANGLE = 2", "NDT_NORMAL_KEEP_NEGATE = 4"):
        assert const in header
    section = re.sub(r"[\s*]+", " ", header[header.index("surface normals and curvature of resident clouds"):header.index("accumulating target: posed scans")])
    assert "no bit parity with pcl" in section.lower() and "the definitions below are the contract" in section


def test_spec_check_at_each_bound(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform
    for s in invalid_specs(_lib):
        assert not g.normalSpecCheck(s), (s.method, s.k, s.radius, s.min_neighbors, list(s.viewpoint))
    assert L.ndt_host_normal_spec_check(None) == _lib.NDT_ERR_INVALID
    tiny = float(np.nextafter(F(0), F(1)))
    for ok in (spec_of(_lib), spec_of(_lib, k=3), spec_of(_lib, k=256), spec_of(_lib, k=3, min_neighbors=2 ** 31 - 1),
               spec_of(_lib, nc.RADIUS, k=0, radius=tiny), spec_of(_lib, nc.RADIUS, k=-7, radius=3e38), spec_of(_lib, nc.KNN, radius=NAN),
               spec_of(_lib, viewpoint=(1e300, -1e300, 5e-324))):
        assert g.normalSpecCheck(ok), (ok.method, ok.k, ok.radius, ok.min_neighbors)
    s = g.normalSpec(k=20)
    assert (s.method, s.k, s.min_neighbors, list(s.viewpoint)) == (1, 20, 3, [0.0, 0.0, 0.0]) and g.normalSpecCheck(s)
    s = g.normalSpec(radius=0.1, min_neighbors=5, viewpoint=(1, 2, 3))
    assert (s.method, s.radius, s.min_neighbors, list(s.viewpoint)) == (2, float(F(0.1)), 5, [1.0, 2.0, 3.0]) and g.normalSpecCheck(s)
    assert not g.normalSpecCheck(g.normalSpec(k=2)) and not g.normalSpecCheck(g.normalSpec(radius=1.0, min_neighbors=2))
    with pytest.raises(ValueError):
        g.normalSpec()
    with pytest.raises(ValueError):
        g.normalSpec(k=5, radius=1.0)


def test_filter_check_at_each_bound(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform
    for f in invalid_filters(_lib):
        assert not g.normalFilterCheck(f), (f.flags, f.curvature_lo, f.curvature_hi, list(f.axis), f.cos_lo, f.cos_hi)
    assert L.ndt_host_normal_filter_check(None) == _lib.NDT_ERR_INVALID
    cu, an, ng = nc.KEEP_CURVATURE, nc.KEEP_ANGLE, nc.KEEP_NEGATE
    ok = [filter_of(_lib), filter_of(_lib, ng), filter_of(_lib, cu, curvature=(0.3, 0.3)), filter_of(_lib, cu, curvature=(-INF, INF)),
          filter_of(_lib, an, cos=(0.0, 1.0)), filter_of(_lib, an, cos=(0.5, 0.5)), filter_of(_lib, an, axis=(0, 0, 1.0 + 5e-13)),
          filter_of(_lib, an, axis=(0.6, 0.0, -0.8)), filter_of(_lib, cu | an | ng),
          # the bounds of a test that is not enabled are not looked at
          filter_of(_lib, 0, curvature=(NAN, NAN), axis=(0, 0, 0), cos=(NAN, 7.0)), filter_of(_lib, cu, axis=(0, 0, 0), cos=(2.0, -1.0)),
          filter_of(_lib, an, curvature=(1.0, 0.0))]
    for f in ok:
        assert g.normalFilterCheck(f), (f.flags, f.curvature_lo, f.curvature_hi, list(f.axis), f.cos_lo, f.cos_hi)
    f = g.normalFilter(curvature=(0.0, 0.02), axis=(0, 0, 1), cos=(0.9, 1.0), negate=True)
    assert (f.flags, f.curvature_hi, list(f.axis), f.cos_lo, f.cos_hi) == (7, float(F(0.02)), [0.0, 0.0, 1.0], 0.9, 1.0) and g.normalFilterCheck(f)
    assert g.normalFilter().flags == 0


def test_plan_at_its_boundaries(mods):
    L, _lib, ndt = mods
    assert "NDT_NORMAL_MAX_BLOCKS" not in os.environ
    plan = ndt.NormalDistributionsTransform.normalPlan
    team, cap = 8, 4096
    assert plan(0) == (0, 0)
    for n, want in ((1, (1, 8)), (7, (1, 8)), (8, (1, 8)), (9, (2, 8)), (16, (2, 8)), (17, (3, 8)), (64, (8, 8)), (65, (9, 8)),
                    (team * cap - 1, (cap, 8)), (team * cap, (cap, 8)), (team * cap + 1, (cap, 16)), (2 * team * cap, (cap, 16)),
                    (2 * team * cap + 1, (cap, 24)), (2 ** 31 - 1, (cap, 8 * -(-(2 ** 28) // cap)))):
        assert plan(n) == want, (n, plan(n), want)
    for n in list(range(1, 70)) + [team * cap + d for d in range(-9, 10)] + [100000, 2000000, 2 ** 31 - 1]:
        blocks, qpb = plan(n)
        passes = -(-n // team)
        assert 1 <= blocks <= cap and blocks == min(passes, cap) and qpb == team * -(-passes // blocks)
    b, q = C.c_int(-3), C.c_int(-3)
    assert L.ndt_host_normal_plan(2 ** 31, C.byref(b), C.byref(q)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_normal_plan(5, None, C.byref(q)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_normal_plan(5, C.byref(b), None) == _lib.NDT_ERR_INVALID
    assert (b.value, q.value) == (-3, -3)


class Args:
    """sentinel-filled outputs of the four device entries"""

    def __init__(self, _lib, n=4):
        self.out = C.c_void_p(SENTINEL)
        self.outs = (C.c_void_p * n)(*([SENTINEL] * n))
        self.idx = np.full(n, -7, np.int32)
        self.normals = np.full(4 * n, -7, F)
        self.counts = np.full(n, -7, np.int32)
        self.n_kept = C.c_size_t(SENTINEL)
        self.n_kepts = (C.c_size_t * n)(*([SENTINEL] * n))
        self.stats = (_lib.NormalStats * n)()
        for s in self.stats:
            s.n_finite = s.n_valid = s.n_collinear = s.max_neighbors = SENTINEL

    def vp(self, a):
        return C.c_void_p(a.ctypes.data)

    def p32(self, a):
        return a.ctypes.data_as(C.POINTER(C.c_int32))

    def untouched(self, out_null=False, outs_null=0):
        return ((self.out.value is None if out_null else self.out.value == SENTINEL)
                and all(self.outs[k] is None for k in range(outs_null)) and all(self.outs[k] == SENTINEL for k in range(outs_null, len(self.outs)))
                and all((a == -7).all() for a in (self.idx, self.normals, self.counts)) and self.n_kept.value == SENTINEL
                and all(v == SENTINEL for v in self.n_kepts)
                and all((s.n_finite, s.n_valid, s.n_collinear, s.max_neighbors) == (SENTINEL,) * 4 for s in self.stats))


def test_refusals_leave_the_outputs_untouched(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    ok, flt = spec_of(_lib), filter_of(_lib)
    # ndt_cloud_estimate_normals: NULL handle / in / spec / normals
    for h, spec_p, normals in ((None, C.byref(ok), True), (g._h, C.byref(ok), True), (g._h, None, True), (g._h, C.byref(ok), False)):
        a = Args(_lib)
        st = L.ndt_cloud_estimate_normals(h, None, spec_p, a.vp(a.normals) if normals else None, a.vp(a.counts), 0, a.stats)
        assert st == _lib.NDT_ERR_INVALID and a.untouched()
    # ndt_cloud_estimate_normals_clouds: NULL handle / normals / in / spec / entry, too many clouds, an invalid spec
    null_entries = (C.c_void_p * 4)()
    a = Args(_lib)
    assert L.ndt_cloud_estimate_normals_clouds(None, null_entries, 4, C.byref(ok), a.vp(a.normals), a.vp(a.counts), 0, a.stats) == _lib.NDT_ERR_INVALID
    assert L.ndt_cloud_estimate_normals_clouds(g._h, null_entries, 4, C.byref(ok), None, a.vp(a.counts), 0, a.stats) == _lib.NDT_ERR_INVALID
    assert L.ndt_cloud_estimate_normals_clouds(g._h, null_entries, 65536, C.byref(ok), a.vp(a.normals), a.vp(a.counts), 0, a.stats) == _lib.NDT_ERR_INVALID
    for spec_p, in_p in ((C.byref(ok), None), (None, null_entries), (C.byref(ok), null_entries)):
        assert L.ndt_cloud_estimate_normals_clouds(g._h, in_p, 4, spec_p, a.vp(a.normals), a.vp(a.counts), 0, a.stats) == _lib.NDT_ERR_INVALID
    for bad in invalid_specs(_lib):
        for n in (0, 4):
            assert L.ndt_cloud_estimate_normals_clouds(g._h, null_entries, n, C.byref(bad), a.vp(a.normals), a.vp(a.counts), 0, a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    # ndt_cloud_select_by_normals: NULL handle / out / in
    a = Args(_lib)
    assert L.ndt_cloud_select_by_normals(None, None, C.byref(ok), C.byref(flt), C.byref(a.out), a.p32(a.idx), C.byref(a.n_kept), a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched(out_null=True)
    a = Args(_lib)
    assert L.ndt_cloud_select_by_normals(g._h, None, C.byref(ok), C.byref(flt), None, a.p32(a.idx), C.byref(a.n_kept), a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    a = Args(_lib)
    assert L.ndt_cloud_select_by_normals(g._h, None, C.byref(ok), C.byref(flt), C.byref(a.out), a.p32(a.idx), C.byref(a.n_kept), a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched(out_null=True)
    # ndt_cloud_select_by_normals_clouds: NULL handle / out / in / spec / filter / entry, too many clouds, an invalid spec or filter
    a = Args(_lib)
    assert L.ndt_cloud_select_by_normals_clouds(None, null_entries, 4, C.byref(ok), C.byref(flt), a.outs, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    assert L.ndt_cloud_select_by_normals_clouds(g._h, null_entries, 4, C.byref(ok), C.byref(flt), None, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    assert L.ndt_cloud_select_by_normals_clouds(g._h, null_entries, 65536, C.byref(ok), C.byref(flt), a.outs, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
    assert a.untouched()                        # (refused before the 65 536 outputs it does not have are written)
    for spec_p, flt_p, in_p in ((C.byref(ok), C.byref(flt), None), (None, C.byref(flt), null_entries), (C.byref(ok), None, null_entries),
                                (C.byref(ok), C.byref(flt), null_entries)):
        a = Args(_lib)
        assert L.ndt_cloud_select_by_normals_clouds(g._h, in_p, 4, spec_p, flt_p, a.outs, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
        assert a.untouched(outs_null=4)
    for bad_s, bad_f in [(s, flt) for s in invalid_specs(_lib)] + [(ok, f) for f in invalid_filters(_lib)]:
        a = Args(_lib)
        assert L.ndt_cloud_select_by_normals_clouds(g._h, null_entries, 0, C.byref(bad_s), C.byref(bad_f), a.outs, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
        assert a.untouched()
        assert L.ndt_cloud_select_by_normals_clouds(g._h, null_entries, 4, C.byref(bad_s), C.byref(bad_f), a.outs, a.n_kepts, a.stats) == _lib.NDT_ERR_INVALID
        assert a.untouched(outs_null=4)
    n = C.c_size_t(SENTINEL)
    assert L.ndt_diag_normals(None, *([C.byref(n)] * 4)) == _lib.NDT_ERR_INVALID
    for hole in range(4):
        ptrs = [C.byref(n)] * 4
        ptrs[hole] = None
        assert L.ndt_diag_normals(g._h, *ptrs) == _lib.NDT_ERR_INVALID and n.value == SENTINEL


def test_no_clouds_is_ok_without_a_device(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    a = Args(_lib)
    ok, flt = spec_of(_lib), filter_of(_lib)
    assert L.ndt_cloud_select_by_normals_clouds(g._h, None, 0, C.byref(ok), C.byref(flt), a.outs, a.n_kepts, a.stats) == _lib.NDT_OK
    assert L.ndt_cloud_estimate_normals_clouds(g._h, None, 0, C.byref(ok), a.vp(a.normals), a.vp(a.counts), 0, a.stats) == _lib.NDT_OK
    assert L.ndt_cloud_estimate_normals_clouds(g._h, None, 0, C.byref(ok), None, None, 1, None) == _lib.NDT_OK
    assert a.untouched()
    assert g.estimateNormalsClouds([], k=5) == ([], [], []) and g.selectByNormalsClouds([], g.normalSpec(k=5)) == ([], [])
    assert g.normalDiag() == dict(index_builds=0, launches=0, blocks=0, scanned_queries=0)
    assert g.selectDiag() == dict(launches=0, blocks=0, clouds=0)
    assert g.outlierDiag() == dict(index_builds=0, value_launches=0, value_blocks=0, scanned_queries=0)


def test_device_calls_need_a_device(mods):
    L, _lib, ndt = mods
    if L.ndt_device_count() > 0:
        return  # (with a device no cloud-free call gets past the argument checks: tests/test_gpu_normals.py takes over)
    g = ndt.NormalDistributionsTransform()
    with pytest.raises(ndt.NdtError) as e:
        g.uploadCloud(np.zeros((3, 3), np.float32))  # no cloud can exist here, so the single-cloud entries have nothing to take
    assert e.value.status == _lib.NDT_ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------- the definition itself
def from_sums(L, _lib, sp, p, pts):
    """the record of the query p with the neighbours pts (rows of f32 coordinates, the query among them)"""
    p, pts = np.asarray(p, F), np.asarray(pts, F)
    e = pts.astype(np.float64) - p.astype(np.float64)
    S1 = np.ascontiguousarray(e.sum(axis=0))
    S2 = np.array([(e[:, a] * e[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
    return from_raw(L, _lib, sp, p, len(pts), S1, S2)


def from_raw(L, _lib, sp, p, m, S1, S2):
    out, line = np.full(4, -7, F), C.c_int(-1)
    p, S1, S2 = np.ascontiguousarray(p, F), np.ascontiguousarray(S1, np.float64), np.ascontiguousarray(S2, np.float64)
    assert L.ndt_host_normal_from_sums(C.byref(sp), p.ctypes.data_as(fp), m, S1.ctypes.data_as(dp), S2.ctypes.data_as(dp), out.ctypes.data_as(fp),
                                       C.byref(line)) == _lib.NDT_OK
    return out, line.value


def is_nan_record(r):
    return (r.view(np.uint32) == nc.QNAN_BITS).all()


def test_from_sums_on_hand_made_inputs(mods):
    L, _lib, ndt = mods
    sp = spec_of(_lib, viewpoint=(0.0, 0.0, 10.0))
    g5 = np.arange(5)
    plane = np.array([(x, y, 2.0) for x in g5 for y in g5], F)
    # a plane: l0 == 0, the curvature exactly 0, the normal towards the viewpoint -- on either side
    rec, line = from_sums(L, _lib, sp, plane[12], plane)
    assert list(rec) == [0.0, 0.0, 1.0, 0.0] and line == 0
    rec, line = from_sums(L, _lib, spec_of(_lib, viewpoint=(2.0, 2.0, -3.0)), plane[12], plane)
    assert list(rec) == [0.0, 0.0, -1.0, 0.0] and line == 0
    # a tilted plane x + z = const: the normal (1, 0, 1) / sqrt 2 to f32 rounding, curvature under 1e-15
    tilted = np.array([(x, y, 8.0 - x) for x in g5 for y in g5], F)
    rec, line = from_sums(L, _lib, sp, tilted[7], tilted)
    assert np.abs(rec[:3] - np.array([1, 0, 1]) / np.sqrt(2)).max() <= 2.0 ** -24 and 0.0 <= rec[3] < 1e-15 and line == 0
    # a line: a valid record orthogonal to it, flagged collinear
    pts = np.array([(t, 2 * t, 5.0) for t in range(9)], F)
    rec, line = from_sums(L, _lib, sp, pts[4], pts)
    assert line == 1 and not np.isnan(rec).any() and abs(float(rec[:3].astype(np.float64) @ np.array([1.0, 2.0, 0.0]))) <= 1e-6
    assert abs(np.linalg.norm(rec[:3].astype(np.float64)) - 1.0) <= 2.0 ** -22 and rec[3] == 0.0
    # one point repeated: t == 0, no normal
    rec, line = from_sums(L, _lib, sp, plane[0], np.tile(plane[0], (6, 1)))
    assert is_nan_record(rec) and line == 0
    # fewer members than min_neighbors: no normal -- and exactly min_neighbors: one
    tri = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0.5)], F)
    rec, line = from_sums(L, _lib, spec_of(_lib, min_neighbors=5, viewpoint=(0, 0, 9)), tri[0], tri)
    assert is_nan_record(rec) and line == 0
    rec, line = from_sums(L, _lib, spec_of(_lib, min_neighbors=4, viewpoint=(0, 0, 9)), tri[0], tri)
    assert not np.isnan(rec).any() and rec[2] > 0 and 0 < rec[3] < 1.0 / 3 + 1e-6
    rec, line = from_raw(L, _lib, sp, tri[0], 0, np.zeros(3), np.zeros(6))
    assert is_nan_record(rec)
    # the viewpoint at the point itself: s == 0, the component of largest magnitude is made positive (the first on ties)
    for p, pts, want in ((plane[12], plane, (0, 0, 1)), (tilted[7], tilted, None)):
        rec, line = from_sums(L, _lib, spec_of(_lib, viewpoint=tuple(float(v) for v in p)), p, pts)
        big = int(np.argmax(np.abs(rec[:3])))
        assert rec[big] > 0 and (want is None or list(rec[:3]) == list(want))
    # the viewpoint in the plane of the neighbourhood: s == 0 as well
    rec, line = from_sums(L, _lib, spec_of(_lib, viewpoint=(40.0, -3.0, 2.0)), plane[12], plane)
    assert list(rec) == [0.0, 0.0, 1.0, 0.0]
    # a sum that is not finite: no normal
    e = plane.astype(np.float64) - plane[12].astype(np.float64)
    S1 = e.sum(axis=0)
    S2 = np.array([(e[:, a] * e[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
    for hole in range(9):
        for v in (NAN, INF, -INF):
            a, b = S1.copy(), S2.copy()
            (a if hole < 3 else b)[hole % 3 if hole < 3 else hole - 3] = v
            rec, line = from_raw(L, _lib, sp, plane[12], len(plane), a, b)
            assert is_nan_record(rec) and line == 0, (hole, v)
    # bad arguments and an invalid spec are refused, the outputs untouched
    out = np.full(4, -7, F)
    p = np.zeros(3, F)
    for bad in invalid_specs(_lib)[:3]:
        assert L.ndt_host_normal_from_sums(C.byref(bad), p.ctypes.data_as(fp), 5, S1.ctypes.data_as(dp), S2.ctypes.data_as(dp), out.ctypes.data_as(fp),
                                           None) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_normal_from_sums(None, p.ctypes.data_as(fp), 5, S1.ctypes.data_as(dp), S2.ctypes.data_as(dp), out.ctypes.data_as(fp), None) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_normal_from_sums(C.byref(sp), p.ctypes.data_as(fp), 5, S1.ctypes.data_as(dp), S2.ctypes.data_as(dp), None, None) == _lib.NDT_ERR_INVALID
    assert (out == -7).all()
    assert L.ndt_host_normal_from_sums(C.byref(sp), p.ctypes.data_as(fp), 25, S1.ctypes.data_as(dp), S2.ctypes.data_as(dp), out.ctypes.data_as(fp), None) == _lib.NDT_OK


def test_keep_on_hand_made_records(mods):
    L, _lib, ndt = mods
    cu, an, ng = nc.KEEP_CURVATURE, nc.KEEP_ANGLE, nc.KEEP_NEGATE

    def keep(f, rec):
        k = C.c_int(-1)
        assert L.ndt_host_normal_keep(C.byref(f), np.ascontiguousarray(rec, F).ctypes.data_as(fp), C.byref(k)) == _lib.NDT_OK
        return k.value

    up, side, nanrec = (0, 0, 1, 0.01), (1, 0, 0, 0.2), nc.nan_record()
    assert keep(filter_of(_lib), up) == 1 and keep(filter_of(_lib), nanrec) == 0 and keep(filter_of(_lib, ng), nanrec) == 0 and keep(filter_of(_lib, ng), up) == 0
    c = filter_of(_lib, cu, curvature=(float(F(0.01)), float(F(0.2))))
    assert keep(c, up) == 1 and keep(c, side) == 1 and keep(c, (0, 0, 1, np.nextafter(F(0.01), F(0)))) == 0 and keep(c, (0, 0, 1, np.nextafter(F(0.2), F(1)))) == 0
    a = filter_of(_lib, an, axis=(0, 0, -1), cos=(0.5, 1.0))
    assert keep(a, up) == 1 and keep(a, (0, 0, -1, 0)) == 1 and keep(a, side) == 0 and keep(a, (0.8, 0.0, 0.6, 0.0)) == 1 and keep(a, (0.9, 0.0, 0.4, 0.0)) == 0
    both = filter_of(_lib, cu | an | ng, curvature=(0.0, 0.05), axis=(0, 0, 1), cos=(0.9, 1.0))
    assert keep(both, up) == 0 and keep(both, side) == 1 and keep(both, (0, 0, 1, 0.5)) == 1 and keep(both, nanrec) == 0
    assert keep(both, (NAN, 0, 1, 0.01)) == 0 and keep(filter_of(_lib), (0, 0, 1, NAN)) == 0
    k = C.c_int(-1)
    rec = np.zeros(4, F)
    assert L.ndt_host_normal_keep(None, rec.ctypes.data_as(fp), C.byref(k)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_normal_keep(C.byref(both), None, C.byref(k)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_normal_keep(C.byref(both), rec.ctypes.data_as(fp), None) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_normal_keep(C.byref(invalid_filters(_lib)[0]), rec.ctypes.data_as(fp), C.byref(k)) == _lib.NDT_ERR_INVALID and k.value == -1
