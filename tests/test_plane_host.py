"""CPU: the plane entries (ndt_cloud_plane_counts, ndt_cloud_segment_plane, ndt_cloud_segment_plane_clouds,
ndt_cloud_plane_distances, ndt_diag_plane and the ndt_host_plane_* ones) -- declared, exported and wrapped; the host functions
against tests/plane_cases.py bit for bit; ndt_host_plane_fit against numpy.linalg.eigh; the validity of a spec at each bound;
the count kernel's plan; every refusal done before any device work, with its outputs untouched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import plane_cases as pc
from conftest import ROOT

NEW = ("ndt_cloud_plane_counts", "ndt_cloud_segment_plane", "ndt_cloud_segment_plane_clouds", "ndt_cloud_plane_distances", "ndt_diag_plane",
       "ndt_host_plane_spec_check", "ndt_host_plane_sample", "ndt_host_plane_model", "ndt_host_plane_distance", "ndt_host_plane_fit",
       "ndt_host_plane_plan")
SENTINEL = 0x5A5A5A5A
NAN, INF = float("nan"), float("inf")
F = np.float32


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def lib_spec(ndt, sp):
    return ndt.plane_spec(sp["T"], sp["H"], seed=sp["seed"], axis=sp["axis"], eps_angle=sp["eps"], refine=sp["refine"])


def test_entries_are_declared_exported_and_wrapped(mods):
    L, _lib, ndt = mods
    with open(os.path.join(ROOT, "include", "ndt_mi355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\(" % name, header), name + " is not declared in include/ndt_mi355.h"
    for method in ("planeCounts", "segmentPlane", "segmentPlaneClouds", "planeDistances", "planeDiag"):
        assert callable(getattr(ndt.NormalDistributionsTransform, method))
    for fn in ("host_plane_sample", "host_plane_model", "host_plane_distance", "host_plane_fit", "host_plane_plan", "plane_spec", "plane_spec_check"):
        assert callable(getattr(ndt, fn))
    assert C.sizeof(_lib.PlaneSpec) == 40 and _lib.PlaneSpec.seed.offset == 8 and _lib.PlaneSpec.refine.offset == 36
    assert C.sizeof(_lib.PlaneResult) == 88 and _lib.PlaneResult.coeff.offset == 8 and _lib.PlaneResult.n_rejected.offset == 80
    for text in ("0x9e3779b97f4a7c15", "0xbf58476d1ce4e5b9", "0x94d049bb133111eb", ">> 30", ">> 27", ">> 31", "no bit parity with pcl"):
        assert text in header.lower(), text


def test_spec_check_at_each_bound(mods):
    L, _lib, ndt = mods
    ok = lambda **kw: ndt.plane_spec_check(_lib.PlaneSpec(**{**dict(distance_threshold=0.1, n_hypotheses=8, seed=1, use_axis=0, axis=(F(0),) * 3,
                                                                     eps_angle=0.0, refine=0), **kw}))
    assert ok() and ok(seed=2 ** 64 - 1) and ok(n_hypotheses=1) and ok(n_hypotheses=65536) and ok(refine=1)
    assert ok(distance_threshold=1e-30) and ok(distance_threshold=3e38)
    for t in (0.0, -0.1, NAN, INF, -INF):
        assert not ok(distance_threshold=t)
    for h in (0, -1, 65537, 2 ** 31 - 1):
        assert not ok(n_hypotheses=h)
    for v in (2, -1):
        assert not ok(use_axis=v) and not ok(refine=v)
    # the axis and the angle count only with use_axis
    assert ok(axis=(F(NAN), F(0), F(0)), eps_angle=NAN) and ok(axis=(F(0),) * 3, eps_angle=-1.0)
    z = (F(0), F(0), F(1))
    half_pi_below = float(np.nextafter(F(math.pi / 2), F(0)))        # the largest f32 not above pi / 2
    assert float(F(math.pi / 2)) > math.pi / 2 > half_pi_below
    assert ok(use_axis=1, axis=z, eps_angle=0.0) and ok(use_axis=1, axis=z, eps_angle=half_pi_below) and ok(use_axis=1, axis=(F(0), F(-1e-30), F(0)))
    for e in (float(F(math.pi / 2)), -1e-6, NAN, INF, 2.0):
        assert not ok(use_axis=1, axis=z, eps_angle=e)
    for a in ((0, 0, 0), (NAN, 0, 1), (0, INF, 1), (0, 0, -INF)):
        assert not ok(use_axis=1, axis=tuple(F(v) for v in a), eps_angle=0.1)
    assert L.ndt_host_plane_spec_check(None) == _lib.NDT_ERR_INVALID
    s = ndt.plane_spec(0.1, 256, seed=-1, axis=(0, 0, 1), eps_angle=0.25, refine=True)
    assert (s.n_hypotheses, s.seed, s.use_axis, s.refine, tuple(s.axis)) == (256, 2 ** 64 - 1, 1, 1, (0.0, 0.0, 1.0)) and ndt.plane_spec_check(s)


def test_sample_bit_for_bit(mods):
    L, _lib, ndt = mods
    assert int(ndt.host_plane_sample(0, 0, 2 ** 31 - 1)[0]) == pc.SPLITMIX64_SEED0[0] % (2 ** 31 - 1)
    assert int(ndt.host_plane_sample(pc.GOLDEN, 0, 1000)[0]) == pc.SPLITMIX64_SEED0[1] % 1000      # x + golden = the second state
    assert int(ndt.host_plane_sample(2 * pc.GOLDEN, 0, 997)[0]) == pc.SPLITMIX64_SEED0[2] % 997
    rng = np.random.default_rng(0)
    for _ in range(300):
        seed, h, n = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 65536)), int(rng.integers(1, 2 ** 31 - 1))
        assert ndt.host_plane_sample(seed, h, n).tolist() == pc.sample(seed, h, n), (seed, h, n)
    assert ndt.host_plane_sample(2 ** 64 - 1, 3, 5).tolist() == pc.sample(2 ** 64 - 1, 3, 5)
    assert ndt.host_plane_sample(1, 0, 1).tolist() == [0, 0, 0]
    idx = (C.c_int32 * 3)(7, 7, 7)
    for args in ((0, 0, 0, idx), (0, -1, 10, idx), (0, 0, 10, None), (0, 0, 2 ** 31, idx)):
        assert L.ndt_host_plane_sample(*args) == _lib.NDT_ERR_INVALID and list(idx) == [7, 7, 7]


def test_model_and_distance_bit_for_bit(mods):
    L, _lib, ndt = mods
    seen = set()
    for name, (xyz, sp) in sorted({**pc.gpu_cases(), **pc.refine_cases()}.items()):
        s = lib_spec(ndt, sp)
        co, st, cn, tri, aux = pc.counts(xyz, sp)
        for h in range(0, sp["H"], 3):
            a, b, c = (xyz[tri[h, j]] for j in range(3))
            got, state = ndt.host_plane_model(s, a, b, c, len(set(tri[h].tolist())) < 3)
            assert state == st[h] and got.tobytes() == co[h].tobytes(), (name, h)
            seen.add(state)
        best = int(np.argmax(cn))
        want = pc.distances(co[best], xyz)
        for i in range(0, len(xyz), 7):
            got = ndt.host_plane_distance(co[best], xyz[i])
            assert np.float64(got).tobytes() == want[i].tobytes() or (np.isnan(got) and np.isnan(want[i])), (name, i)
    assert seen == {0, 1, 2}
    # the hand cases
    s = ndt.plane_spec(0.1, 1)
    assert ndt.host_plane_model(s, (0, 0, 1), (1, 0, 1), (0, 1, 1))[0].tolist() == [0, 0, 1, -1]
    assert ndt.host_plane_model(s, (0, 0, 1), (1, 0, 1), (0, 1, 1), same_index=True)[1] == 1
    assert ndt.host_plane_model(s, (0, 0, 0), (1, 1, 1), (2, 2, 2))[1] == 1 and ndt.host_plane_model(s, (0, 0, NAN), (1, 0, 1), (0, 1, 1))[1] == 1
    ax = ndt.plane_spec(0.1, 1, axis=(0, 0, 1), eps_angle=math.radians(10.0))
    for deg, want in ((11.0, 2), (9.0, 0)):
        tri = ((0, 0, 0), (1, 0, math.tan(math.radians(deg))), (0, 1, 0))
        got, state = ndt.host_plane_model(ax, *tri)
        ref, rstate = pc.model(pc.spec(0.1, 1, axis=(0, 0, 1), eps=math.radians(10.0)), *tri)
        assert state == want == rstate and got.tobytes() == ref.tobytes()
    for tri, want in ((((0, 0, 0), (0, 1, 0), (1, 0, 0)), [0, 0, 1]), (((0, 0, 0), (0, 0, 1), (1, 0, 0)), [0, 1, 0]), (((0, 0, 0), (0, 0, 1), (0, 1, 0)), [1, 0, 0])):
        assert ndt.host_plane_model(s, *tri)[0][:3].tolist() == want
    assert np.isnan(ndt.host_plane_distance([0, 0, 1, 0], (NAN, 0, 0))) and ndt.host_plane_distance([0, 0, 1, 0], (0, 0, INF)) == INF
    bad = ndt.plane_spec(0.1, 1)
    bad.n_hypotheses = 0
    co, st = (C.c_double * 4)(7, 7, 7, 7), C.c_int(7)
    p = (C.c_float * 3)(0, 0, 0)
    assert L.ndt_host_plane_model(C.byref(bad), p, p, p, 0, co, C.byref(st)) == _lib.NDT_ERR_INVALID and list(co) == [7] * 4 and st.value == 7
    assert L.ndt_host_plane_model(None, p, p, p, 0, co, C.byref(st)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_plane_distance(None, p, co) == _lib.NDT_ERR_INVALID


def test_fit_against_eigh(mods):
    L, _lib, ndt = mods
    rng = np.random.default_rng(5)
    for trial in range(40):
        k = int(rng.integers(3, 400))
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        basis = np.linalg.svd(n[None])[2][1:]
        centre = rng.uniform(-50, 50, 3) * (1000.0 if trial % 4 == 0 else 1.0)
        pts = centre + rng.uniform(-10, 10, (k, 2)) @ basis + rng.normal(0, 0.02, (k, 1)) * n
        a = pts[0]
        sp = pc.spec(0.1, 1, axis=(0, 0, 1), eps=0.3) if trial % 2 else pc.spec(0.1, 1)
        taken_ref, ref, lam_ref, sums = pc.fit(sp, pts, a)
        taken, got, lam = ndt.host_plane_fit(lib_spec(ndt, sp), k, sums["S1"], sums["S2"], a)
        assert taken == taken_ref
        if not taken:
            continue
        dn, dd = pc.refine_bound(sums, lam_ref, float(np.linalg.norm(a + sums["S1"] / k)))
        assert np.abs(got[:3] - ref[:3]).max() <= dn and abs(got[3] - ref[3]) <= dd, (trial, got - ref, dn, dd)
        assert abs(np.linalg.norm(got[:3]) - 1.0) < 1e-15 and np.abs(lam - lam_ref).max() <= 1e-12 * max(lam_ref[2], 1.0)
        assert np.abs(got[:3] - np.sign(got[:3] @ n) * n).max() < 0.05
    # rank 1 (a line) and too few points: refused, the coefficients untouched
    line = np.array([[k, 2.0 * k, -3.0 * k] for k in range(12)])
    sp = pc.spec(0.1, 1)
    sums = pc.fit(sp, line, line[0])[3]
    s = lib_spec(ndt, sp)
    co, tk = (C.c_double * 4)(7, 7, 7, 7), C.c_int(7)
    dp = lambda v: (C.c_double * len(v))(*v)
    assert L.ndt_host_plane_fit(C.byref(s), 12.0, dp(sums["S1"]), dp(sums["S2"]), dp(line[0]), co, None, C.byref(tk)) == _lib.NDT_OK
    assert tk.value == 0 and list(co) == [7] * 4
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.0]])
    sums = pc.fit(sp, tri, tri[0])[3]
    assert ndt.host_plane_fit(s, 3, sums["S1"], sums["S2"], tri[0])[0] and not ndt.host_plane_fit(s, 2, sums["S1"], sums["S2"], tri[0])[0]
    assert not ndt.host_plane_fit(s, 3, [NAN, 0, 0], sums["S2"], tri[0])[0] and not ndt.host_plane_fit(s, 3, sums["S1"], [INF] * 6, tri[0])[0]
    assert ndt.host_plane_fit(s, 3, sums["S1"], sums["S2"], tri[0])[1].tolist() == [0, 0, 1, 0]


def test_plan(mods):
    L, _lib, ndt = mods
    plan = ndt.host_plane_plan
    p = plan(1, 1)
    tile, hpb = p["tile_points"], p["hyp_per_block"]
    assert p == dict(tile_points=tile, hyp_per_block=hpb, tiles=1, hyp_blocks=1, tile_blocks=1) and tile % 64 == 0 and hpb % 64 == 0
    assert plan(0, 5)["tiles"] == 0 and plan(0, 5)["tile_blocks"] == 0
    for n, t in ((tile, 1), (tile + 1, 2), (2 * tile, 2), (2 * tile + 1, 3)):
        assert plan(n, 7)["tiles"] == t == plan(n, 7)["tile_blocks"]
    for H, hb in ((hpb, 1), (hpb + 1, 2), (65536, 65536 // hpb)):
        assert plan(10, H)["hyp_blocks"] == hb
    cap = plan(2 ** 31 - 1, 1)["tile_blocks"]            # the blocks of one cloud at most
    assert plan(cap * tile, 1)["tile_blocks"] == cap == plan(cap * tile, 1)["tiles"] and plan(cap * tile + 1, 1)["tiles"] == cap + 1
    assert plan(cap * tile + 1, 1)["tile_blocks"] == cap
    q = plan(cap * tile, 3 * hpb)
    assert q["tile_blocks"] == cap // 3 and q["tile_blocks"] * q["hyp_blocks"] <= cap
    assert plan(50 * tile, 65536)["tile_blocks"] == max(1, cap // (65536 // hpb)) < 50 and plan(5 * tile, 65536)["tile_blocks"] == 5
    v = [C.c_int(7) for _ in range(5)]
    for n, H in ((2 ** 31, 1), (10, 0), (10, 65537)):
        assert L.ndt_host_plane_plan(n, H, *[C.byref(x) for x in v]) == _lib.NDT_ERR_INVALID and [x.value for x in v] == [7] * 5
    assert L.ndt_host_plane_plan(10, 1, None, *[C.byref(x) for x in v[1:]]) == _lib.NDT_ERR_INVALID


class Args:
    """sentinel-filled outputs of the device entries"""

    def __init__(self, _lib, n=4):
        self.ci, self.co = C.c_void_p(SENTINEL), C.c_void_p(SENTINEL)
        self.cis, self.cos = (C.c_void_p * n)(*([SENTINEL] * n)), (C.c_void_p * n)(*([SENTINEL] * n))
        self.res = (_lib.PlaneResult * n)()
        for r in self.res:
            r.found, r.best, r.best_count = 7, 7, SENTINEL
        self.counts = (C.c_uint32 * 8)(*([7] * 8))
        self.values = np.full(8, -7.0)

    def untouched(self, null=False, nulls=0):
        want = None if null else SENTINEL
        return (self.ci.value == want and self.co.value == want
                and all(a[k] is None for a in (self.cis, self.cos) for k in range(nulls))
                and all(a[k] == SENTINEL for a in (self.cis, self.cos) for k in range(nulls, len(self.cis)))
                and all((r.found, r.best, r.best_count) == (7, 7, SENTINEL) for r in self.res)
                and list(self.counts) == [7] * 8 and (self.values == -7.0).all())


def test_refusals_leave_the_outputs_untouched(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    ok = ndt.plane_spec(0.1, 8)
    bad = ndt.plane_spec(0.1, 8)
    bad.distance_threshold = 0.0
    a = Args(_lib)
    # counts: NULL handle / cloud / counts
    assert L.ndt_cloud_plane_counts(None, None, C.byref(ok), None, None, None, a.counts) == _lib.NDT_ERR_INVALID and a.untouched()
    assert L.ndt_cloud_plane_counts(g._h, None, C.byref(ok), None, None, None, a.counts) == _lib.NDT_ERR_INVALID and a.untouched()
    assert L.ndt_cloud_plane_counts(g._h, None, C.byref(ok), None, None, None, None) == _lib.NDT_ERR_INVALID and a.untouched()
    # segmentation of one cloud: NULL handle / result / cloud; the output clouds become NULL
    for h, res in ((None, a.res), (g._h, None), (g._h, a.res)):
        a = Args(_lib)
        assert L.ndt_cloud_segment_plane(h, None, C.byref(ok), None, res, C.byref(a.ci), C.byref(a.co)) == _lib.NDT_ERR_INVALID
        assert a.untouched(null=True)
    # of many: NULL handle, too many clouds (refused before the outputs it does not have are written), NULL in / results / entry / spec
    entries = (C.c_void_p * 4)()
    a = Args(_lib)
    assert L.ndt_cloud_segment_plane_clouds(None, entries, 4, C.byref(ok), a.res, a.cis, a.cos) == _lib.NDT_ERR_INVALID and a.untouched()
    assert L.ndt_cloud_segment_plane_clouds(g._h, entries, 65536, C.byref(ok), a.res, a.cis, a.cos) == _lib.NDT_ERR_INVALID and a.untouched()
    for in_p, spec_p, res in ((None, C.byref(ok), a.res), (entries, C.byref(ok), None), (entries, C.byref(ok), a.res), (entries, None, a.res),
                              (entries, C.byref(bad), a.res)):
        a2 = Args(_lib)
        assert L.ndt_cloud_segment_plane_clouds(g._h, in_p, 4, spec_p, a2.res if res is not None else None, a2.cis, a2.cos) == _lib.NDT_ERR_INVALID
        assert a2.untouched(nulls=4)
    a = Args(_lib)
    assert L.ndt_cloud_segment_plane_clouds(g._h, entries, 0, C.byref(bad), a.res, a.cis, a.cos) == _lib.NDT_ERR_INVALID and a.untouched()
    # distances: NULL handle / cloud / coeff / values
    co = (C.c_double * 4)(0, 0, 1, 0)
    vp = C.c_void_p(a.values.ctypes.data)
    for args in ((None, None, co, vp), (g._h, None, co, vp), (g._h, None, None, vp), (g._h, None, co, None)):
        assert L.ndt_cloud_plane_distances(*args, 0) == _lib.NDT_ERR_INVALID and a.untouched()
    n = C.c_size_t(SENTINEL)
    assert L.ndt_diag_plane(None, *[C.byref(n)] * 4) == _lib.NDT_ERR_INVALID
    for hole in range(4):
        ptrs = [C.byref(n)] * 4
        ptrs[hole] = None
        assert L.ndt_diag_plane(g._h, *ptrs) == _lib.NDT_ERR_INVALID and n.value == SENTINEL


def test_no_clouds_is_ok_without_a_device(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    a = Args(_lib)
    assert L.ndt_cloud_segment_plane_clouds(g._h, None, 0, C.byref(ndt.plane_spec(0.1, 8)), None, a.cis, a.cos) == _lib.NDT_OK and a.untouched()
    assert g.segmentPlaneClouds([], ndt.plane_spec(0.1, 8)) == ([], [], [])
    assert g.planeDiag() == dict(launches=0, select_launches=0, count_blocks=0, clouds=0)
    assert g.selectDiag() == dict(launches=0, blocks=0, clouds=0)


def test_device_calls_need_a_device(mods):
    L, _lib, ndt = mods
    if L.ndt_device_count() > 0:
        return  # (with a device no cloud-free call gets past the argument checks: tests/test_gpu_plane.py takes over)
    g = ndt.NormalDistributionsTransform()
    with pytest.raises(ndt.NdtError) as e:
        g.uploadCloud(np.zeros((3, 3), np.float32))  # no cloud can exist here, so the single-cloud entries have nothing to take
    assert e.value.status == _lib.NDT_ERR_NO_DEVICE
