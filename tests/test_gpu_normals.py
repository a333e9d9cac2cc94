"""GPU: surface normals and curvature of resident clouds (ndt_cloud_estimate_normals / _clouds, ndt_cloud_select_by_normals /
_clouds) against the numpy restatement of the contract, tests/normal_cases.py, by the comparison rules stated there (derived, not
measured): counts, n_finite, n_valid, max_neighbors and which records are NaN exactly; directions to 2^-24 on well-conditioned
points; on every valid point the unit length, the eigen-residual, the orientation and the curvature; n_collinear exactly on the cases
built to be collinear or clearly not.  The same bits: the single and the list call, host and device outputs, and -- in a child --
NDT_NORMAL_MAX_BLOCKS=3.  The selections: the kept set is ndt_host_normal_keep's on the call's own records, exactly, and the
reference's where its values keep clear of the bounds (tests/test_normal_cases.py holds that)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import normal_cases as nc
from test_gpu_centroid_fitness import app_settings
from test_gpu_pairs import build_app
from test_gpu_select import check_selection, raw
from test_normal_cases import SELECTIONS

pytestmark = pytest.mark.gpu

F = np.float32
CASES = nc.gpu_cases()
PAIRS = [(name, j) for name in sorted(CASES) for j in range(len(CASES[name][1]))]
_REFS = {}


def ref_of(name, sp):
    key = (name, nc.tag_of(sp))
    if key not in _REFS:
        _REFS[key] = nc.reference(CASES[name][0], sp)
    return _REFS[key]


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import _lib, ndt
    return ndt, _lib, built_lib


@pytest.fixture(scope="module")
def g(mods):
    return mods[0].NormalDistributionsTransform()


def c_filter(g, flt):
    f = g.normalFilter()
    f.flags, f.curvature_lo, f.curvature_hi, f.cos_lo, f.cos_hi = flt["flags"], flt["curvature_lo"], flt["curvature_hi"], flt["cos_lo"], flt["cos_hi"]
    f.axis[:] = flt["axis"]
    return f


def same(a, b):
    """records, counts and stats of two calls: the same bits"""
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def check_stats(st, ref, what):
    want = ref["stats"]
    assert (st["n_finite"], st["n_valid"], st["max_neighbors"]) == (want["n_finite"], want["n_valid"], want["max_neighbors"]), (what, st, want)
    assert abs(st["n_collinear"] - want["n_collinear"]) <= int(ref["near_line"].sum()), (what, st, want)


def check_case(g, name, sp, directions):
    what = (name, nc.tag_of(sp))
    xyz = CASES[name][0]
    ref = ref_of(name, sp)
    dc = g.uploadCloud(xyz)
    got = g.estimateNormals(dc, **nc.kw_of(sp))
    d = g.normalDiag()
    some = 1 if len(xyz) else 0
    assert d["index_builds"] == some and d["launches"] == some and d["blocks"] == g.normalPlan(len(xyz))[0], (what, d)
    route = nc.ROUTES.get(what)
    if route is not None:
        assert (d["scanned_queries"] > 0) == (route == "scan"), (what, d)
    rec, cnt, st = got
    assert rec.shape == (len(xyz), 4) and rec.dtype == F and cnt.shape == (len(xyz),) and cnt.dtype == np.int32
    bad = nc.compare(rec, cnt, ref, sp, xyz, directions)
    assert not bad, (what, bad)
    check_stats(st, ref, what)
    # the list call of one cloud, and a call without counts: the same bits
    recs, cnts, sts = g.estimateNormalsClouds([dc], **nc.kw_of(sp))
    assert same((recs[0], cnts[0], sts[0]), got), what
    only = g.estimateNormals(dc, counts=False, **nc.kw_of(sp))
    assert only[1] is None and only[0].tobytes() == rec.tobytes() and only[2] == st, what
    return dc, got


@pytest.mark.parametrize("name,j", PAIRS, ids=["%s, %s" % (n, nc.tag_of(CASES[n][1][j][0])) for n, j in PAIRS])
def test_every_case_against_the_definitions(mods, g, name, j):
    sp, directions = CASES[name][1][j]
    check_case(g, name, sp, directions)


def test_exact_content(mods, g):
    """what the cases built for it must give exactly"""
    rec, cnt, st = g.estimateNormals(g.uploadCloud(CASES["an exact plane"][0]), k=9)
    assert (rec[:, 3] == 0).all() and (rec[:, 2] == -1).all() and (rec[:, :2] == 0).all() and st["n_collinear"] == 0  # (the sensor is below z = 3)
    for kw in (dict(k=5), dict(radius=7.0)):
        rec, cnt, st = g.estimateNormals(g.uploadCloud(CASES["an exact line"][0]), **kw)
        assert st["n_collinear"] == st["n_valid"] == 40 and not np.isnan(rec).any() and (rec[:, 3] == 0).all(), (kw, st)
    rec, cnt, st = g.estimateNormals(g.uploadCloud(CASES["every point equal"][0]), radius=1.0)
    assert (rec.view(np.uint32) == nc.QNAN_BITS).all() and (cnt == 70).all() and st == dict(n_finite=70, n_valid=0, n_collinear=0, max_neighbors=70)
    rec, cnt, st = g.estimateNormals(g.uploadCloud(CASES["|F| < min_neighbors"][0]), k=10, min_neighbors=8)
    assert (rec.view(np.uint32) == nc.QNAN_BITS).all() and sorted(set(cnt)) == [0, 5] and st == dict(n_finite=5, n_valid=0, n_collinear=0, max_neighbors=5)
    rec, cnt, st = g.estimateNormals(g.uploadCloud(np.full((20, 3), np.nan, F)), k=5)
    assert (rec.view(np.uint32) == nc.QNAN_BITS).all() and (cnt == 0).all() and st == dict(n_finite=0, n_valid=0, n_collinear=0, max_neighbors=0)
    assert g.normalDiag() == dict(index_builds=1, launches=1, blocks=3, scanned_queries=0)
    rec, cnt, st = g.estimateNormals(g.uploadCloud(np.zeros((0, 3), F)), k=5)
    assert rec.shape == (0, 4) and cnt.shape == (0,) and g.normalDiag() == dict(index_builds=0, launches=0, blocks=0, scanned_queries=0)


@pytest.mark.parametrize("k", nc.NEAR_K)
def test_clouds_of_k_to_k_plus_9_points(mods, g, k):
    """the eight-lane gather's tails and the LDS row's end; k = 3: the property checks alone (its conditioning is out of the cap)"""
    clouds = nc.near_k_clouds(k)
    sp = nc.spec(k=k)
    dcs = [g.uploadCloud(x) for x in clouds]
    recs, cnts, sts = g.estimateNormalsClouds(dcs, **nc.kw_of(sp))
    d = g.normalDiag()
    assert d["index_builds"] == 10 and d["launches"] == 1 and d["blocks"] == sum(g.normalPlan(len(x))[0] for x in clouds), d
    for x, dc, rec, cnt, st in zip(clouds, dcs, recs, cnts, sts):
        ref = nc.reference(x, sp)
        bad = nc.compare(rec, cnt, ref, sp, x, directions=k != 3)
        assert not bad and (cnt == k).all(), (k, len(x), bad)
        check_stats(st, ref, (k, len(x)))
        assert same(g.estimateNormals(dc, **nc.kw_of(sp)), (rec, cnt, st)), (k, len(x))


def test_either_side_of_the_block_cap(mods, g):
    """the point counts at which the plan reaches its cap and first strides; the reference on a sample of the rows"""
    plan = g.normalPlan
    cap = plan(10 ** 6)[0]
    n_cap = 8 * cap
    assert plan(n_cap) == (cap, 8) and plan(n_cap + 1) == (cap, 16)
    full = nc.surface(n_cap + 1, 11, scale=40.0)
    for n in (n_cap, n_cap + 1):
        xyz = full[:n]
        rows = np.unique(np.concatenate([np.arange(0, 24), np.arange(n - 24, n), np.arange(n_cap // 2 - 8, n_cap // 2 + 8),
                                         np.random.default_rng(n).integers(0, n, 200)]))
        dc = g.uploadCloud(xyz)
        for sp in (nc.spec(k=10), nc.spec(radius=0.8)):
            rec, cnt, st = g.estimateNormals(dc, **nc.kw_of(sp))
            assert g.normalDiag()["blocks"] == cap and st["n_finite"] == n and st["n_valid"] <= n
            ref = nc.reference(xyz, sp, rows)
            assert nc.ill_fraction(ref) <= nc.ILL_CAP
            bad = nc.compare(rec, cnt, ref, sp, xyz)
            assert not bad, (n, nc.tag_of(sp), bad)
            assert st["n_valid"] == int((~np.isnan(rec).any(axis=1)).sum()) and st["max_neighbors"] == cnt.max()


def test_the_strided_regime_in_a_child(mods, g, tmp_path):
    """NDT_NORMAL_MAX_BLOCKS=3: three blocks stride over the passes of small clouds (tests/normals_child.py), the same bits"""
    from normals_child import PICKS
    assert "NDT_NORMAL_MAX_BLOCKS" not in os.environ
    mine = {}
    flt = g.normalFilter(curvature=(0.0, 0.02))
    for j, (name, sp) in enumerate(PICKS):
        dc = g.uploadCloud(CASES[name][0])
        rec, cnt, st = g.estimateNormals(dc, **nc.kw_of(sp))
        assert g.normalDiag()["blocks"] == -(-len(dc) // 8)
        mine["rec%d" % j], mine["cnt%d" % j] = rec, cnt
        mine["st%d" % j] = np.array([st[k] for k in ("n_finite", "n_valid", "n_collinear", "max_neighbors")], np.int64)
        mine["idx%d" % j] = g.selectByNormals(dc, g.normalSpec(**nc.kw_of(sp)), flt, indices=True)[2]
    path = str(tmp_path / "parent.npz")
    np.savez(path, **mine)
    env = dict(os.environ, NDT_NORMAL_MAX_BLOCKS="3")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "normals_child.py")
    r = subprocess.run([sys.executable, child, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["cases"] == len(PICKS) and res["max_blocks_seen"] == 3, res


def test_outputs_to_device_memory_are_the_same_bits(mods, g):
    from test_gpu_parity import _DeviceCopies
    ndt, _lib, L = mods
    xyz = CASES["non-finite rows"][0]
    n = len(xyz)
    dc = g.uploadCloud(xyz)
    with _DeviceCopies() as dev:
        for kw in (dict(k=8), dict(radius=1.2)):
            rec, cnt, st = g.estimateNormals(dc, **kw)
            buf = dev.put(np.full(5 * n, -7.0, F))  # 4 n floats, then n int32
            p_rec, p_cnt, st_d = g.estimateNormals(dc, device=buf, **kw)
            assert p_rec == buf and p_cnt == buf + 16 * n and st_d == st
            back = np.zeros(5 * n, F)
            assert dev.hip.hipMemcpy(back.ctypes.data, buf, back.nbytes, 2) == 0  # hipMemcpyDeviceToHost
            assert back[:4 * n].tobytes() == rec.tobytes() and back[4 * n:].view(np.int32).tobytes() == cnt.tobytes()
            # the list call into device memory, and without counts
            buf2 = dev.put(np.full(5 * 2 * n, -7.0, F))
            arr = (C.c_void_p * 2)(dc._c, dc._c)
            sts = (_lib.NormalStats * 2)()
            assert L.ndt_cloud_estimate_normals_clouds(g._h, arr, 2, C.byref(g.normalSpec(**kw)), C.c_void_p(buf2), None, 1, sts) == _lib.NDT_OK
            back2 = np.zeros(10 * n, F)
            assert dev.hip.hipMemcpy(back2.ctypes.data, buf2, back2.nbytes, 2) == 0
            assert back2[:4 * n].tobytes() == rec.tobytes() and back2[4 * n:8 * n].tobytes() == rec.tobytes() and (back2[8 * n:] == -7.0).all()
            assert g._normal_stats(sts[0]) == st and g._normal_stats(sts[1]) == st
        # records that are not aligned to 16 bytes are refused
        buf = dev.put(np.zeros(5 * n + 4, F))
        assert L.ndt_cloud_estimate_normals(g._h, dc._c, C.byref(g.normalSpec(k=8)), C.c_void_p(buf + 4), None, 1, None) == _lib.NDT_ERR_INVALID


# ---------------------------------------------------------------------------------------------------- many clouds
@pytest.mark.parametrize("sp", (nc.spec(k=8), nc.spec(radius=1.2), nc.spec(k=64, min_neighbors=10, viewpoint=nc.ABOVE)), ids=nc.tag_of)
def test_many_clouds_match_the_single_calls(mods, g, sp):
    """ragged clouds, empty clouds among them, in one normals launch: every cloud's bits are those of its own call, in any order"""
    clouds = [CASES[name][0] for name in nc.RAGGED]
    dcs = [g.uploadCloud(x) for x in clouds]
    singles = [g.estimateNormals(dc, **nc.kw_of(sp)) for dc in dcs]
    recs, cnts, sts = g.estimateNormalsClouds(dcs, **nc.kw_of(sp))
    d = g.normalDiag()
    assert d["index_builds"] == sum(1 for x in clouds if len(x)) and d["launches"] == 1 and d["blocks"] == sum(g.normalPlan(len(x))[0] for x in clouds), d
    for j in range(len(dcs)):
        assert same((recs[j], cnts[j], sts[j]), singles[j]), (j, nc.RAGGED[j])
    order = [8, 0, 5, 2, 7, 4, 3, 1, 6]
    recs, cnts, sts = g.estimateNormalsClouds([dcs[j] for j in order], **nc.kw_of(sp))
    for at, j in enumerate(order):
        assert same((recs[at], cnts[at], sts[at]), singles[j]), (at, j)
    # the selections of the list: every cloud what its own call gives
    flt = g.normalFilter(curvature=(0.0, 0.05), axis=(0, 0, 1), cos=(0.5, 1.0))
    spec = g.normalSpec(**nc.kw_of(sp))
    outs, sts2 = g.selectByNormalsClouds(dcs, spec, flt)
    assert g.normalDiag() == d
    host_flt = nc.keep_filter(nc.KEEP_CURVATURE | nc.KEEP_ANGLE, (0.0, 0.05), (0, 0, 1), (0.5, 1.0))
    for j, dc in enumerate(dcs):
        one, st1, idx = g.selectByNormals(dc, spec, flt, indices=True)
        assert st1 == singles[j][2] == sts2[j], j
        mask = nc.keep_by(host_flt, singles[j][0])
        check_selection(g, raw(g, dc), mask, one, idx, (j, nc.tag_of(sp)))
        check_selection(g, raw(g, dc), mask, outs[j], None, (j, nc.tag_of(sp)))
    only_empty = g.estimateNormalsClouds([dcs[1], dcs[7]], **nc.kw_of(sp))
    assert [len(r) for r in only_empty[0]] == [0, 0] and g.normalDiag() == dict(index_builds=0, launches=0, blocks=0, scanned_queries=0)


# ---------------------------------------------------------------------------------------------------- the selections
@pytest.mark.parametrize("which", sorted(SELECTIONS))
def test_selections_of_the_golden_scan(mods, g, which):
    """the kept set: ndt_host_normal_keep on the call's OWN records, exactly -- and the reference's where it keeps clear of the bounds"""
    ndt, _lib, L = mods
    flt = SELECTIONS[which]
    xyz = CASES["golden scan"][0]
    dc = g.uploadCloud(xyz)
    records = raw(g, dc)
    for sp in (nc.spec(k=10), nc.spec(radius=1.5)):
        rec, cnt, st = g.estimateNormals(dc, **nc.kw_of(sp))
        d = g.normalDiag()
        f = c_filter(g, flt)
        mask = np.zeros(len(xyz), bool)
        for i in range(len(xyz)):
            k = C.c_int(-1)
            assert L.ndt_host_normal_keep(C.byref(f), rec[i].ctypes.data_as(C.POINTER(C.c_float)), C.byref(k)) == _lib.NDT_OK
            mask[i] = bool(k.value)
        assert np.array_equal(mask, nc.keep_by(flt, rec))
        sel_before = g.selectDiag()
        got, st2, idx = g.selectByNormals(dc, g.normalSpec(**nc.kw_of(sp)), f, indices=True)
        assert st2 == st and g.normalDiag() == d and g.selectDiag() == sel_before, (which, nc.tag_of(sp))
        check_selection(g, records, mask, got, idx, (which, nc.tag_of(sp)))
        if sp["method"] == nc.KNN and which in ("curvature", "angle to z"):
            assert np.array_equal(mask, nc.keep_by(flt, ref_of("golden scan", sp)["records"])), which
        if which == "every normal":
            assert mask.sum() == st["n_valid"] and np.array_equal(idx, g.selectByNormals(dc, g.normalSpec(**nc.kw_of(sp)), None, indices=True)[2])


def test_refusals_with_a_cloud_in_hand(mods, g):
    ndt, _lib, L = mods
    dc = g.uploadCloud(CASES["size n=65"][0])
    bad = g.normalSpec(k=8)
    bad.k = 257
    ok, flt = g.normalSpec(k=8), g.normalFilter()
    bad_flt = g.normalFilter(curvature=(0.5, 0.25))
    out, nk = C.c_void_p(0x5A5A), C.c_size_t(77)
    for s, f in ((bad, flt), (ok, bad_flt), (None, flt), (ok, None)):
        out = C.c_void_p(0x5A5A)
        st = L.ndt_cloud_select_by_normals(g._h, dc._c, C.byref(s) if s else None, C.byref(f) if f else None, C.byref(out), None, C.byref(nk), None)
        assert st == _lib.NDT_ERR_INVALID and out.value is None and nk.value == 77
    rec = np.full(4 * len(dc), -7.0, F)
    assert L.ndt_cloud_estimate_normals(g._h, dc._c, C.byref(bad), C.c_void_p(rec.ctypes.data), None, 0, None) == _lib.NDT_ERR_INVALID
    assert L.ndt_cloud_estimate_normals(g._h, dc._c, C.byref(ok), None, None, 0, None) == _lib.NDT_ERR_INVALID
    assert (rec == -7.0).all()
    outs, arr = (C.c_void_p * 2)(0x5A5A, 0x5A5A), (C.c_void_p * 2)(dc._c, None)
    assert L.ndt_cloud_select_by_normals_clouds(g._h, arr, 2, C.byref(ok), C.byref(flt), outs, None, None) == _lib.NDT_ERR_INVALID
    assert outs[0] is None and outs[1] is None
    assert L.ndt_cloud_estimate_normals_clouds(g._h, arr, 2, C.byref(ok), C.c_void_p(rec.ctypes.data), None, 0, None) == _lib.NDT_ERR_INVALID
    assert (rec == -7.0).all()
    # an empty cloud: an empty result, never NULL
    empty, st = g.selectByNormals(g.uploadCloud(np.zeros((0, 3), F)), ok)
    assert len(empty) == 0 and empty.bounds()[1] == "none" and st == dict(n_finite=0, n_valid=0, n_collinear=0, max_neighbors=0)
    assert g.normalDiag() == dict(index_builds=0, launches=0, blocks=0, scanned_queries=0)


def test_the_calls_change_nothing_of_the_handle(mods, pair):
    ndt = mods[0]
    t, s = pair
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(t)
    g.setInputSource(s)
    g.align()
    g.mapUpdate(s[:3000], leaf_size=0.5)
    dc = g.uploadCloud(s[:8000])
    g.selectCloud(dc, finite=True)
    g.neighborValues(dc, radius=0.5, min_neighbors=3)
    g.extractClusters(dc, 0.5, 5)

    def state():
        return (g.getFinalTransformation().tobytes(), g.hasConverged(), g.getFinalNumIteration(), g.getTransformationProbability(),
                repr(g.stats()), g.grid_counts(), g.inputBounds("source")[0].tobytes(), g.inputBounds("source")[1], g.inputBounds("target")[0].tobytes(),
                g.mapSize(), repr(g.selectDiag()), repr(g.outlierDiag()), repr(g.diagClusters()), repr(g.planeDiag()))
    before = state()
    for kw in (dict(k=10), dict(radius=0.5)):
        g.estimateNormals(dc, **kw)
        assert state() == before
        g.selectByNormals(dc, g.normalSpec(**kw), g.normalFilter(curvature=(0.0, 0.05)), indices=True)
        assert state() == before
        g.selectByNormalsClouds([dc, g.uploadCloud(s[:100])], g.normalSpec(**kw))
        g.estimateNormalsClouds([dc, g.uploadCloud(s[:100])], **kw)
        assert state() == before
    T0 = g.getFinalTransformation().tobytes()
    g.align()
    assert g.getFinalTransformation().tobytes() == T0


# ---------------------------------------------------------------------------------------------------- the app
def test_map_sequence_flat(mods, pair, tmp_path):
    """apps/map_sequence --scan-to-map --flat <k> <curvature_max> on two synthetic PCD files against the same loop in Python: kept
    counts exact, the registration's transform within 1e-5 (the bound of the other app tests)"""
    ndt = mods[0]
    d = tmp_path / "pcd"
    d.mkdir()
    scans = []
    for k, x in enumerate(pair, 1):
        path = str(d / ("cloud_%d.pcd" % k))
        ndt.pcd_write_xyz(path, np.ascontiguousarray(x[::2]))
        scans.append(np.ascontiguousarray(ndt.pcd_read_xyz(path)[0][:, :3], dtype=F))
    exe = build_app(tmp_path, "map_sequence")
    plain = subprocess.check_output([exe, "--scan-to-map", str(d)], text=True)
    assert "flat kept:" not in plain
    for args in (["--flat", "10", "0.05", str(d)], ["--scan-to-map", "--flat", "2", "0.05", str(d)], ["--scan-to-map", "--flat", "257", "0.05", str(d)],
                 ["--scan-to-map", "--flat", "10", "-0.1", str(d)], ["--scan-to-map", "--flat", "10", "nan", str(d)], ["--scan-to-map", "--flat", "10"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage: map_sequence" in r.stderr, args
    out = subprocess.check_output([exe, "--scan-to-map", "--flat", "10", "0.05", str(d)], text=True)
    g = ndt.NormalDistributionsTransform()
    app_settings(g)
    want, kept, prev = [], [], np.eye(4, dtype=F)
    for k, x in enumerate(scans):
        dc = g.uploadCloud(x)
        n = len(dc)
        dc = g.selectByNormals(dc, g.normalSpec(k=10), g.normalFilter(curvature=(0.0, 0.05)))[0]
        kept.append((len(dc), n))
        g.voxelGridFilterBegin(dc, 0.5)
        dc, _ = g.voxelGridFilterEnd()
        if k == 0:
            g.targetAccumulateCloud(dc)
            continue
        g.setInputSourceCloud(dc)
        g.align(prev)
        assert g.hasConverged()
        prev = g.getFinalTransformation().astype(F)
        want.append(prev)
    got_kept = [tuple(int(v) for v in m) for m in re.findall(r"^flat kept: (\d+)/(\d+)$", out, re.M)]
    print("kept: app", got_kept, "python", kept)
    assert got_kept == kept and all(0 < a < b for a, b in kept)
    lines = out.splitlines()
    got = [np.array([[float(v) for v in lines[i + 1 + r].split()] for r in range(4)]) for i, ln in enumerate(lines) if ln.startswith("Transform ")]
    print("app", got, "python", want)
    assert len(got) == len(want) == 1 and np.abs(got[0] - want[0]).max() <= 1e-5
