"""GPU: ndt_cloud_plane_counts / ndt_cloud_segment_plane / ndt_cloud_segment_plane_clouds / ndt_cloud_plane_distances against
the numpy restatement of the definitions (tests/plane_cases.py).

Bounds (derived, not measured):
  models                  1e-12 relative (normal entries against 1, d against max(|d|, 1)): both sides round every operation
                          on its own, so they differ only where the device's f64 division or square root would
  states, counts, best, best_count, n_inliers, n_finite, n_degenerate, n_rejected: exact -- tests/test_plane_cases.py holds
                          every fixture's distances 1e-9 m clear of the threshold, its angles 1e-9 clear of cos_eps
  inlier / other clouds   records, order, boxes exact (check_selection: cloud_box_cases.reference_boxes)
  refined coefficients    plane_cases.refine_bound: from n, 2^-53, the sums' magnitudes and the eigen-gap
  distances               the same bits as the host function
  single call, many-clouds call, either merge form, any block cap: the same bits"""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import plane_cases as pc
from test_gpu_centroid_fitness import app_settings
from test_gpu_pairs import build_app
from test_gpu_select import check_selection, raw, xyz_of

pytestmark = pytest.mark.gpu

F = np.float32
CASES = pc.gpu_cases()
REFINE = pc.refine_cases()


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import _lib, ndt
    return ndt, _lib, built_lib


@pytest.fixture(scope="module")
def g(mods):
    return mods[0].NormalDistributionsTransform()


def lib_spec(ndt, sp, **kw):
    sp = dict(sp, **kw)
    return ndt.plane_spec(sp["T"], sp["H"], seed=sp["seed"], axis=sp["axis"], eps_angle=sp["eps"], refine=sp["refine"])


def check_counts(mods, g, xyz, sp, triples=None, what=None):
    """models, states and counts of one call against the restatement, and the launches it states"""
    ndt = mods[0]
    co, st, cn, tri, aux = pc.counts(xyz, sp, triples)
    dc = g.uploadCloud(xyz)
    got_co, got_st, got_cn = g.planeCounts(dc, lib_spec(ndt, sp), triples)
    assert np.array_equal(got_st, st), what
    err = np.abs(got_co - co) / np.maximum(np.abs(co), 1.0)
    assert (err <= 1e-12).all(), (what, err.max())
    assert np.array_equal(got_cn, cn), (what, np.flatnonzero(got_cn != cn)[:8])
    plan = ndt.host_plane_plan(len(xyz), sp["H"])
    d = g.planeDiag()
    assert d == dict(launches=3 if len(xyz) else 2, select_launches=0, count_blocks=plan["tile_blocks"] * plan["hyp_blocks"], clouds=1), (what, d)
    return dc, (co, st, cn, tri)


def same_result(a, b):
    return all(a[k] == b[k] for k in a if k != "coeff") and a["coeff"].tobytes() == b["coeff"].tobytes()


def check_segment(mods, g, xyz, sp, triples=None, what=None):
    """segmentPlane against the restatement: the result row, both clouds, the many-clouds form of one"""
    ndt = mods[0]
    ref = pc.segment(xyz, sp, triples)
    dc = g.uploadCloud(xyz)
    records = raw(g, dc)
    res, inl, oth = g.segmentPlane(dc, lib_spec(ndt, sp), triples)
    d = g.planeDiag()
    for k in ("found", "best", "best_count", "n_inliers", "n_finite", "n_degenerate", "n_rejected"):
        assert res[k] == ref[k], (what, k, res[k], ref[k])
    if not sp["refine"]:
        assert not res["refined"] and res["n_inliers"] == res["best_count"]
        err = np.abs(res["coeff"] - ref["coeff"]) / np.maximum(np.abs(ref["coeff"]), 1.0)
        assert (err <= 1e-12).all(), (what, err)
    check_selection(g, records, ref["inliers"], inl, None, (what, "inliers"))
    check_selection(g, records, ref["others"], oth, None, (what, "others"))
    want = (5 if sp["refine"] else 4) if len(xyz) else 2       # (no point: the model and the choice launch alone)
    assert d["launches"] == want and d["select_launches"] == (4 if len(xyz) else 0) and d["clouds"] == 1, (what, d)
    if triples is None:
        many, inls, oths = g.segmentPlaneClouds([dc], lib_spec(ndt, sp))
        assert same_result(many[0], res), what
        assert np.array_equal(raw(g, inls[0]), raw(g, inl)) and np.array_equal(raw(g, oths[0]), raw(g, oth)), what
        assert np.array_equal(inls[0].bounds()[0], inl.bounds()[0]) and np.array_equal(oths[0].bounds()[0], oth.bounds()[0]), what
    return dc, res, inl, oth, ref


# ---------------------------------------------------------------------------------------------------- counts
def test_counts_at_every_plan_boundary(mods, g):
    """n = 3, 4, 63 | 64 | 65, 255 | 256 | 257, either side of every tile step up to two tiles + 1; hypotheses 1, 63 | 64 | 65,
    255 | 256 | 257, either side of two hypothesis blocks"""
    ndt = mods[0]
    p = ndt.host_plane_plan(1, 1)
    assert (p["tile_points"], p["hyp_per_block"]) == (1024, 256), "plane_cases.SHAPE_N / SHAPE_H follow the plan: move them with it"
    for n in (1024, 1025, 2048, 2049):
        assert ndt.host_plane_plan(n, 1)["tiles"] == (n + 1023) // 1024
    for n, sp in pc.shape_cases():
        check_counts(mods, g, pc.shape_cloud(n), sp, None, (n, sp))


def test_the_strided_regime_in_a_child(mods):
    """NDT_PLANE_MAX_BLOCKS=3: at most three blocks stride over the tiles, in both merge forms (tests/plane_child.py)"""
    env = dict(os.environ, NDT_PLANE_MAX_BLOCKS="3")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plane_child.py")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["cases"] >= 10 and res["max_tile_blocks_seen"] == 3 and res["strided"] >= 3, res


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_against_the_definitions(mods, g, name):
    """at the origin and at 100 km, with and without an axis, with rows that are not finite"""
    xyz, sp = CASES[name]
    check_counts(mods, g, xyz, sp, None, name)
    dc, res, inl, oth, ref = check_segment(mods, g, xyz, sp, None, name)
    co, st, cn = g.planeCounts(dc, lib_spec(mods[0], sp))
    valid = np.flatnonzero(st == 0)
    assert res["best"] == int(valid[np.argmax(cn[valid])]) and res["best_count"] == int(cn[res["best"]])
    assert res["coeff"].tobytes() == co[res["best"]].tobytes()
    assert len(inl) + len(oth) == res["n_finite"] == int(np.isfinite(xyz).all(1).sum())


def test_caller_triples_with_degenerate_and_rejected_rows(mods, g):
    ndt = mods[0]
    xyz, sp = CASES["non-finite rows"]
    n = len(xyz)
    tri = pc.triples_of(99, 70, n)
    bad_row = int(np.flatnonzero(~np.isfinite(xyz).all(1))[0])
    tri[3] = [5, 5, 9]                      # a repeated index
    tri[11] = [bad_row, 1, 2]               # a point that is not finite
    tri[64] = [7, 9, 7]
    wall = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1]], F) + F(3.0)
    xyz = xyz.copy()
    xyz[20:23] = wall                        # three points of a vertical plane: rejected under the z axis
    tri[40] = [20, 21, 22]
    sp = dict(sp, H=70)
    c = pc.clearances(xyz, sp, tri)
    assert c["distance"] >= 1e-9 and c["angle"] >= 1e-9 and c["degeneracy"] <= 0.5, c
    dc, (co, st, cn, _) = check_counts(mods, g, xyz, sp, tri, "caller triples")
    assert st[3] == st[11] == st[64] == pc.DEGENERATE and st[40] == pc.REJECTED and (st == pc.VALID).sum() > 30
    assert cn[3] == cn[11] == cn[40] == 0
    check_segment(mods, g, xyz, sp, tri, "caller triples")
    # an index outside the cloud: refused before any device work
    for v in (-1, n):
        t2 = tri.copy()
        t2[69, 2] = v
        with pytest.raises(ndt.NdtError) as e:
            g.planeCounts(dc, lib_spec(ndt, sp), t2)
        assert e.value.status == mods[1].NDT_ERR_INVALID
        with pytest.raises(ndt.NdtError):
            g.segmentPlane(dc, lib_spec(ndt, sp), t2)


def test_all_points_on_one_plane(mods, g):
    """coordinates that are multiples of 1/8 on z = 1: every product is exact, s == 0 under every valid hypothesis"""
    rng = np.random.default_rng(3)
    xyz = np.column_stack([rng.integers(-400, 400, (1500, 2)) / 8.0, np.ones(1500)]).astype(F)
    for axis in (None, (0.0, 0.0, 1.0)):
        sp = pc.spec(0.01, 100, seed=8, axis=axis, eps=0.1)
        dc, (co, st, cn, tri) = check_counts(mods, g, xyz, sp, None, "one plane")
        assert (cn[st == 0] == 1500).all() and (st == 0).sum() > 80 and (cn[st != 0] == 0).all()
        dc, res, inl, oth, ref = check_segment(mods, g, xyz, sp, None, "one plane")
        assert res["best"] == int(np.flatnonzero(st == 0)[0]) and len(inl) == 1500 and len(oth) == 0
        assert res["coeff"].tolist() == [0.0, 0.0, 1.0, -1.0]


def test_two_parallel_planes_with_equal_counts(mods, g):
    rng = np.random.default_rng(4)
    xy = rng.integers(-200, 200, (300, 2)) / 8.0
    xyz = np.concatenate([np.column_stack([xy, np.zeros(300)]), np.column_stack([xy, np.full(300, 2.0)])]).astype(F)
    tri = np.array([[0, 0, 1], [300, 301, 302], [0, 1, 2], [303, 304, 305], [3, 4, 5]], np.int32)
    sp = pc.spec(0.05, 5)
    assert pc.models(xyz, sp, tri)[1].tolist() == [1, 0, 0, 0, 0]
    dc, (co, st, cn, _) = check_counts(mods, g, xyz, sp, tri, "parallel planes")
    assert cn.tolist() == [0, 300, 300, 300, 300]
    dc, res, inl, oth, ref = check_segment(mods, g, xyz, sp, tri, "parallel planes")
    assert res["best"] == 1 and res["coeff"].tolist() == [0.0, 0.0, 1.0, -2.0]
    assert np.array_equal(xyz_of(raw(g, inl)), xyz[300:]) and np.array_equal(xyz_of(raw(g, oth)), xyz[:300])


def test_no_plane(mods, g):
    """n < 3, and no valid hypothesis: found = 0, the coefficients 0, an empty inlier cloud (never NULL), every finite point in
    the other cloud"""
    base = CASES["non-finite rows"][0]
    for n in (0, 1, 2):
        dc, res, inl, oth, ref = check_segment(mods, g, base[1:1 + n], pc.spec(0.1, 9, seed=2), None, ("n", n))
        assert not res["found"] and res["best"] == -1 and not res["coeff"].any() and res["n_degenerate"] == 9
        assert len(inl) == 0 and inl.bounds()[1] == "none" and len(oth) == n
    line = np.array([[k, 2 * k, -k] for k in range(50)], F)
    line[7] = np.nan
    for sp in (pc.spec(0.1, 64, seed=1), pc.spec(0.1, 64, seed=1, refine=True)):
        dc, res, inl, oth, ref = check_segment(mods, g, line, sp, None, "a line")
        assert not res["found"] and not res["refined"] and res["n_degenerate"] == 64 and len(inl) == 0 and len(oth) == 49
    wall = np.column_stack([np.zeros(40), np.arange(40.0) % 7, np.arange(40.0) // 7]).astype(F)     # x = 0 under the z axis: all rejected
    dc, res, inl, oth, ref = check_segment(mods, g, wall, pc.spec(0.1, 32, seed=1, axis=(0, 0, 1), eps=0.2), None, "a wall")
    assert not res["found"] and res["n_rejected"] > 0 and res["n_rejected"] + res["n_degenerate"] == 32 and len(oth) == 40


# ---------------------------------------------------------------------------------------------------- refinement
@pytest.mark.parametrize("name", sorted(REFINE))
def test_refinement(mods, g, name):
    xyz, sp = REFINE[name]
    ref = pc.reference_of(name)
    dc, res, inl, oth, _ = check_segment(mods, g, xyz, sp, None, name)            # (the refined inlier set, exactly)
    assert res["refined"] and ref["refined"]
    dn, dd = pc.refine_bound(ref["sums"], ref["lam"], float(np.linalg.norm(ref["a"] + ref["sums"]["S1"] / ref["sums"]["count"])))
    en, ed = np.abs(res["coeff"][:3] - ref["coeff"][:3]).max(), abs(res["coeff"][3] - ref["coeff"][3])
    print(name, "refined normal error %.3g (bound %.3g), d error %.3g (bound %.3g)" % (en, dn, ed, dd))
    assert en <= dn and ed <= dd
    plain = g.segmentPlane(dc, lib_spec(mods[0], sp, refine=False))[0]
    assert plain["best"] == res["best"] and plain["best_count"] == res["best_count"] and not plain["refined"]
    assert plain["coeff"].tobytes() != res["coeff"].tobytes()


# ---------------------------------------------------------------------------------------------------- distances
def test_distances_are_the_host_function(mods, g):
    ndt = mods[0]
    from test_gpu_parity import _DeviceCopies
    for name in ("non-finite rows", "ground 4099 at 100 km, any plane"):
        xyz, sp = CASES[name]
        ref = pc.reference_of(name)
        dc = g.uploadCloud(xyz)
        got = g.planeDistances(dc, ref["coeff"])
        assert g.planeDiag() == dict(launches=1, select_launches=0, count_blocks=0, clouds=1)
        fin = np.isfinite(xyz).all(1)
        assert np.isnan(got[~fin]).all() and got[fin].tobytes() == pc.distances(ref["coeff"], xyz)[fin].tobytes()
        for i in range(0, len(xyz), 41):
            if fin[i]:
                assert np.float64(ndt.host_plane_distance(ref["coeff"], xyz[i])).tobytes() == got[i].tobytes()
        assert np.array_equal(got[fin], ref["keys"][fin])
        with _DeviceCopies() as dev:             # to device memory: the same bits, ready as the keys of a height band
            buf = dev.put(np.full(2 * len(xyz), -7.0, F))
            assert g.planeDistances(dc, ref["coeff"], device=buf) == buf
            back = np.zeros(len(xyz))
            assert dev.hip.hipMemcpy(back.ctypes.data, buf, back.nbytes, 2) == 0
            assert back.tobytes() == got.tobytes()
            band, idx = g.selectCloud(dc, keys=buf, key_range=(0.5, 2.0), indices=True)
            assert np.array_equal(idx, np.flatnonzero(fin & (got >= 0.5) & (got <= 2.0))) and 0 < len(idx)
    dc = g.uploadCloud(CASES["ground 1000"][0])
    for bad in ([0, 0, 0, 1], [np.nan, 0, 1, 0], [0, 0, 1, np.inf]):
        with pytest.raises(ndt.NdtError) as e:
            g.planeDistances(dc, bad)
        assert e.value.status == mods[1].NDT_ERR_INVALID
    assert len(g.planeDistances(g.uploadCloud(np.zeros((0, 3), F)), [0, 0, 1, 0])) == 0


# ---------------------------------------------------------------------------------------------------- many clouds
def test_many_clouds_match_the_single_calls(mods, g):
    """ragged clouds (an empty one, one of two points, rows that are not finite, 100 km) in either order"""
    ndt = mods[0]
    base = [CASES["ground 1000"][0], np.zeros((0, 3), F), CASES["non-finite rows"][0], CASES["ground 1000"][0][:2],
            CASES["ground 4099 at 100 km, any plane"][0], CASES["ground 1000 at 100 km"][0][:257]]
    for refine in (False, True):
        s = ndt.plane_spec(0.1, 300, seed=13, axis=(0, 0, 1), eps_angle=math.radians(10.0), refine=refine)
        clouds = [g.uploadCloud(x) for x in base]
        single = [g.segmentPlane(dc, s) for dc in clouds]
        for order in (list(range(len(base))), list(range(len(base)))[::-1]):
            res, inls, oths = g.segmentPlaneClouds([clouds[k] for k in order], s)
            d = g.planeDiag()
            assert d["launches"] == (5 if refine else 4) and d["select_launches"] == 4 and d["clouds"] == len(base), d
            assert d["count_blocks"] == sum(p["tile_blocks"] * p["hyp_blocks"] for p in (ndt.host_plane_plan(len(x), 300) for x in base))
            for j, k in enumerate(order):
                r1, i1, o1 = single[k]
                assert same_result(res[j], r1), (refine, k, res[j], r1)
                assert np.array_equal(raw(g, inls[j]), raw(g, i1)) and np.array_equal(raw(g, oths[j]), raw(g, o1)), (refine, k)
                for a, b in ((inls[j], i1), (oths[j], o1)):
                    assert np.array_equal(a.bounds()[0], b.bounds()[0]) and a.bounds()[1] == b.bounds()[1], (refine, k)
        assert single[0][0]["found"] and not single[1][0]["found"] and not single[3][0]["found"] and single[0][0]["refined"] == refine
        res, inls, oths = g.segmentPlaneClouds(clouds, s, inliers=False)
        assert inls is None and g.planeDiag()["select_launches"] == 2 and all(same_result(res[k], single[k][0]) for k in range(len(base)))
        res, inls, oths = g.segmentPlaneClouds(clouds, s, inliers=False, others=False)
        assert oths is None and g.planeDiag()["select_launches"] == 0 and all(same_result(res[k], single[k][0]) for k in range(len(base)))


# ---------------------------------------------------------------------------------------------------- consumers
def test_outputs_feed_every_consumer(mods, pair):
    """the other cloud (the scan without its ground) as source, target, filter input and accumulated scan: the same results as
    the upload of the host-selected rows"""
    ndt = mods[0]
    t, s = pair
    s = np.ascontiguousarray(s[:20000])
    sp = pc.spec(0.2, 128, seed=3)
    ref = pc.segment(s, sp)
    mask = ref["others"]
    assert ref["found"] and 0 < mask.sum() < len(s)

    def both(make):
        res = []
        for form in ("plane", "upload"):
            h = ndt.NormalDistributionsTransform()
            dc = h.segmentPlane(h.uploadCloud(s), lib_spec(ndt, sp), inliers=False)[2] if form == "plane" else h.uploadCloud(s[mask])
            res.append(make(h, dc))
        return res
    a, b = both(lambda h, dc: (raw(h, dc), dc.bounds()[0]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    def as_source(h, dc):
        h.setInputTarget(t)
        h.setInputSourceCloud(dc)
        h.align()
        return h.getFinalTransformation().tobytes(), h.getFinalNumIteration(), h.hasConverged()
    a, b = both(as_source)
    assert a == b

    def as_target(h, dc):
        h.setInputTargetCloud(dc)
        return h.grid()
    a, b = both(as_target)
    assert set(a) == set(b) and len(a["idx"]) > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k

    def through_filter(h, dc):
        h.voxelGridFilterBegin(dc, 0.5)
        out, ov = h.voxelGridFilterEnd()
        return raw(h, out), ov
    a, b = both(through_filter)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and len(a[0]) > 0

    def through_accumulate(h, dc):
        h.targetAccumulateCloud(dc)
        return bytes(h.targetAccumulateExport())
    a, b = both(through_accumulate)
    assert a == b and len(a) > 0


# ---------------------------------------------------------------------------------------------------- refusals, untouched state
def test_refusals_with_a_cloud_in_hand(mods, g):
    ndt, _lib, L = mods
    dc = g.uploadCloud(CASES["ground 1000"][0])
    ok, bad = ndt.plane_spec(0.1, 8), ndt.plane_spec(0.1, 8)
    bad.n_hypotheses = 65537
    res, ci, co = _lib.PlaneResult(), C.c_void_p(0x5A5A), C.c_void_p(0x5A5A)
    res.best = 77
    for spec_p in (C.byref(bad), None):
        ci, co = C.c_void_p(0x5A5A), C.c_void_p(0x5A5A)
        assert L.ndt_cloud_segment_plane(g._h, dc._c, spec_p, None, C.byref(res), C.byref(ci), C.byref(co)) == _lib.NDT_ERR_INVALID
        assert ci.value is None and co.value is None and res.best == 77
    counts = (C.c_uint32 * 8)(*([7] * 8))
    assert L.ndt_cloud_plane_counts(g._h, dc._c, C.byref(bad), None, None, None, counts) == _lib.NDT_ERR_INVALID and list(counts) == [7] * 8
    assert L.ndt_cloud_plane_counts(g._h, dc._c, C.byref(ok), None, None, None, None) == _lib.NDT_ERR_INVALID
    outs, arr = (C.c_void_p * 2)(0x5A5A, 0x5A5A), (C.c_void_p * 2)(dc._c, None)
    ress = (_lib.PlaneResult * 2)()
    assert L.ndt_cloud_segment_plane_clouds(g._h, arr, 2, C.byref(ok), ress, outs, None) == _lib.NDT_ERR_INVALID
    assert outs[0] is None and outs[1] is None
    # neither output cloud asked for: the result alone
    r = g.segmentPlane(dc, ok, inliers=False, others=False)
    assert r[1] is None and r[2] is None and r[0]["found"] and g.planeDiag()["select_launches"] == 0


def test_the_calls_change_nothing_of_the_handle(mods, pair):
    ndt = mods[0]
    t, s = pair
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(t)
    g.setInputSource(s)
    g.align()
    g.mapUpdate(s[:3000], leaf_size=0.5)
    g.getNVTL()
    g.scorePoses([np.eye(4)])
    dc = g.uploadCloud(s[:8000])
    g.selectCloud(dc, finite=True)
    g.removeOutliers(dc, radius=0.5, min_neighbors=2)
    pending = g.uploadCloud(s[:5000])
    ref_filtered = raw(g, g.voxelGridFilterCloud(s[:5000], 0.5)[0])
    g.voxelGridFilterBegin(pending, 0.5)

    def state():
        return (g.getFinalTransformation().tobytes(), g.hasConverged(), g.getFinalNumIteration(), g.getTransformationProbability(),
                repr(g.stats()), g.grid_counts(), g.inputBounds("source")[0].tobytes(), g.inputBounds("source")[1], g.inputBounds("target")[0].tobytes(),
                g.mapSize(), g.scorePosesLaunches(), g.nvtlLaunches(), repr(g.selectDiag()), repr(g.outlierDiag()))
    before = state()
    for refine in (False, True):
        spec = ndt.plane_spec(0.2, 64, seed=1, refine=refine)
        g.planeCounts(dc, spec)
        assert state() == before
        res = g.segmentPlane(dc, spec)[0]
        assert state() == before and res["found"]
        g.segmentPlaneClouds([dc, g.uploadCloud(s[:100])], spec)
        assert state() == before
        g.planeDistances(dc, res["coeff"])
        assert state() == before
    g.planeDiag()
    out, ov = g.voxelGridFilterEnd()
    assert np.array_equal(raw(g, out), ref_filtered) and not ov
    T0 = g.getFinalTransformation().tobytes()
    g.align()
    assert g.getFinalTransformation().tobytes() == T0


# ---------------------------------------------------------------------------------------------------- the app
def test_map_sequence_ground_flags(mods, pair, tmp_path):
    """apps/map_sequence --scan-to-map --ground ... [--ground-remove] on two synthetic PCD files against the same loop in Python:
    printed counts exact, the registration's transform within 1e-5 (the bound of the other app tests)"""
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
    assert "ground:" not in plain
    for args in (["--ground", "0.2", "128", "15", str(d)], ["--scan-to-map", "--ground-remove", str(d)], ["--scan-to-map", "--ground", "0", "128", "15", str(d)],
                 ["--scan-to-map", "--ground", "0.2", "0", "15", str(d)], ["--scan-to-map", "--ground", "0.2", "65537", "15", str(d)],
                 ["--scan-to-map", "--ground", "0.2", "128", "91", str(d)], ["--scan-to-map", "--ground", "0.2", "128", "-1", str(d)],
                 ["--scan-to-map", "--ground", "0.2", "128"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage: map_sequence" in r.stderr, args

    def transforms(out):
        lines = out.splitlines()
        return [np.array([[float(x) for x in lines[i + 1 + r].split()] for r in range(4)]) for i, ln in enumerate(lines) if ln.startswith("Transform ")]
    spec = ndt.plane_spec(0.2, 128, seed=0, axis=(0, 0, 1), eps_angle=float(F(15.0 * math.pi / 180.0)))
    for remove in (False, True):
        out = subprocess.check_output([exe, "--scan-to-map", "--ground", "0.2", "128", "15"] + (["--ground-remove"] if remove else []) + [str(d)], text=True)
        g = ndt.NormalDistributionsTransform()
        app_settings(g)
        want, grounds, prev = [], [], np.eye(4, dtype=F)
        for k, x in enumerate(scans):
            dc = g.uploadCloud(x)
            res, _, rest = g.segmentPlane(dc, spec, inliers=False, others=remove)
            grounds.append((res["n_inliers"], len(x)) + tuple(float("%.9g" % v) for v in res["coeff"]))
            if remove:
                dc = rest
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
        got_grounds = [(int(m[0]), int(m[1])) + tuple(float(v) for v in m[2:]) for m in
                       re.findall(r"^ground: (\d+)/(\d+) normal (\S+) (\S+) (\S+) d (\S+)$", out, re.M)]
        print(remove, "ground: app", got_grounds, "python", grounds)
        assert got_grounds == grounds and all(0 < a[0] < a[1] for a in grounds), remove
        got = transforms(out)
        assert len(got) == len(want) == 1
        for a, b in zip(got, want):
            assert np.abs(a - b).max() <= 1e-5, (remove, a, b)
