"""GPU: ndt_cloud_neighbor_values / ndt_cloud_remove_outliers / ndt_cloud_remove_outliers_clouds against the numpy restatement of
the definitions (tests/outlier_cases.py).

Bounds (derived, not measured):
  per-point values        relative 1e-12: (mean_k + 2) f64 roundings <= 3e-14 at mean_k = 256 (test_gpu_fitness_edges' bound)
  RADIUS counts, n_finite, n_valid, kept indices / records / order / boxes: exact
  mean 1e-11, stddev 1e-9 relative; stddev of equal values exactly 0
  kept set == {i in F : value_i <= threshold} under the call's OWN values and threshold, exactly; and == the reference's kept
  set on every cloud of outlier_cases.gpu_cases (tests/test_outlier_cases.py holds their values clear of the threshold)
  single call, many-clouds call, values to the host / to device memory: the same bits
The index leaf follows the radius (RADIUS), so "a radius many leaves wide" arises only where the leaf is clamped by the cell
budget or the index slack is large: the 100 km cloud, which takes the whole-cloud scan with radius 0.05."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import outlier_cases as oc
from test_gpu_centroid_fitness import app_settings
from test_gpu_pairs import build_app
from test_gpu_select import check_selection, raw, xyz_of

pytestmark = pytest.mark.gpu

F = np.float32
CASES = oc.gpu_cases()


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import _lib, ndt
    return ndt, _lib, built_lib


@pytest.fixture(scope="module")
def g(mods):
    return mods[0].NormalDistributionsTransform()


def kw_of(spec):
    """the wrapper's keywords of an outlier_cases spec (negate apart)"""
    if spec["method"] == oc.RADIUS:
        return dict(radius=spec["radius"], min_neighbors=spec["min_neighbors"])
    return dict(mean_k=spec["mean_k"], stddev_mul=spec["stddev_mul"])


def rel_close(got, want, tol):
    return abs(got - want) <= tol * abs(want)


def check_values(values, stats, ref, spec, what):
    """values and statistics of one call against the reference"""
    want = ref["values"]
    assert values.shape == want.shape and np.array_equal(np.isnan(values), np.isnan(want)), what
    fin = ~np.isnan(want)
    if spec["method"] == oc.RADIUS:
        assert np.array_equal(values[fin], want[fin]), what
        assert stats == dict(n_finite=ref["n_finite"], n_valid=ref["n_finite"], mean=0.0, stddev=0.0, threshold=float(spec["min_neighbors"])), what
        return
    err = np.abs(values[fin] - want[fin])
    print(what, "max relative value error %.3g" % (err / np.maximum(want[fin], 1e-300)).max() if fin.any() else "no finite row")
    assert (err <= 1e-12 * np.abs(want[fin])).all(), what
    assert stats["n_finite"] == ref["n_finite"] and stats["n_valid"] == ref["n_valid"], what
    print(what, "mean", stats["mean"], ref["mean"], "stddev", stats["stddev"], ref["stddev"], "threshold", stats["threshold"], ref["threshold"])
    assert rel_close(stats["mean"], ref["mean"], 1e-11), what
    if ref["stddev"] == 0.0:
        assert stats["stddev"] == 0.0, what
    else:
        assert rel_close(stats["stddev"], ref["stddev"], 1e-9), what
    if ref["n_valid"] == 0:
        assert (stats["mean"], stats["stddev"], stats["threshold"]) == (0.0, 0.0, 0.0) and (values[fin] == 0.0).all(), what
    assert stats["threshold"] == stats["mean"] + spec["stddev_mul"] * stats["stddev"], what


def same_stats(a, b):
    return all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in ("mean", "stddev", "threshold")) and a["n_finite"] == b["n_finite"] and a["n_valid"] == b["n_valid"]


def check_case(g, name, xyz, spec, route=None):
    """one (cloud, spec): values, statistics, the kept cloud, the many-clouds form of one"""
    what = (name, spec)
    ref = oc.reference_of(name, xyz, spec)
    dc = g.uploadCloud(xyz)
    records = raw(g, dc)
    values, stats = g.neighborValues(dc, **kw_of(spec))
    d = g.outlierDiag()
    plan_blocks = g.outlierPlan(len(xyz))[0]
    assert d["index_builds"] == (1 if len(xyz) else 0) and d["value_launches"] == (1 if len(xyz) else 0) and d["value_blocks"] == plan_blocks, (what, d)
    if route is not None:
        assert (d["scanned_queries"] > 0) == (route == "scan"), (what, d)
    check_values(values, stats, ref, spec, what)
    got, st2, idx = g.removeOutliers(dc, negate=spec["negate"], indices=True, **kw_of(spec))
    assert same_stats(st2, stats), what
    assert g.outlierDiag() == d, what
    # the kept set is what the call's own values and threshold say, exactly ...
    mask = oc.keep_by(values, st2["threshold"], spec["method"], spec["negate"])
    check_selection(g, records, mask, got, idx, what)
    # ... and the reference's: its values keep clear of its threshold, or all equal it (then the device's must too)
    fin = ~np.isnan(ref["values"])
    if spec["method"] == oc.STATISTICAL and fin.any() and (ref["values"][fin] == ref["threshold"]).all():
        assert np.array_equal(values[fin], ref["values"][fin]) and stats["stddev"] == 0.0, what
    assert np.array_equal(mask, ref["keep"]), what
    outs, sts = g.removeOutliersClouds([dc], negate=spec["negate"], **kw_of(spec))
    assert same_stats(sts[0], stats) and np.array_equal(raw(g, outs[0]), raw(g, got)), what
    assert np.array_equal(outs[0].bounds()[0], got.bounds()[0]) and outs[0].bounds()[1] == got.bounds()[1], what
    return dc, got, values, stats


ROUTES = {("far points", "STATISTICAL"): "scan", ("surface, no stray point", "STATISTICAL"): "shells", ("surface, no stray point", "RADIUS"): "shells",
          ("100 km from the origin", "RADIUS 0.05"): "scan", ("cells of 1 ... 129 points", "STATISTICAL"): "scan", ("a plane", "RADIUS"): "shells"}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_against_the_definitions(mods, g, name):
    xyz, specs = CASES[name]
    for spec in specs:
        tag = "STATISTICAL" if spec["method"] == oc.STATISTICAL else "RADIUS"
        route = ROUTES.get((name, tag)) or ROUTES.get((name, "%s %g" % (tag, spec.get("radius") or 0)))
        if name == "surface, no stray point" and spec.get("mean_k", 8) != 8:
            route = None
        check_case(g, name, xyz, spec, route)


def test_either_side_of_the_block_cap(mods, g):
    """the point counts at which the plan reaches its cap and first strides; the reference on a sample of the rows"""
    plan = g.outlierPlan
    cap = plan(10 ** 6)[0]
    n_cap = 8 * cap
    assert plan(n_cap) == (cap, 8) and plan(n_cap + 1) == (cap, 16)
    full = oc.surface(n_cap + 1, 11, scale=40.0)
    for n in (n_cap, n_cap + 1):
        xyz = full[:n]
        rows = np.unique(np.concatenate([np.arange(0, 24), np.arange(n - 24, n), np.arange(n_cap // 2 - 8, n_cap // 2 + 8),
                                         np.random.default_rng(n).integers(0, n, 300)]))
        d2 = oc._d2_rows(xyz, rows)
        dc = g.uploadCloud(xyz)
        counts, st = g.neighborValues(dc, radius=0.4, min_neighbors=6)
        assert g.outlierDiag()["value_blocks"] == cap and st["n_finite"] == n
        assert np.array_equal(counts[rows], (d2 <= F(0.4) * F(0.4)).sum(axis=1))
        vals, st = g.neighborValues(dc, mean_k=8, stddev_mul=1.0)
        want = np.cumsum(np.sqrt(np.sort(np.partition(d2, 7, axis=1)[:, :8], axis=1).astype(np.float64)), axis=1)[:, -1] / 8
        assert (np.abs(vals[rows] - want) <= 1e-12 * want).all() and not np.isnan(vals).any()
        v = vals
        assert rel_close(st["mean"], float(np.mean(v)), 1e-11) and rel_close(st["stddev"], float(np.std(v, ddof=1)), 1e-9)
        got, st2, idx = g.removeOutliers(dc, radius=0.4, min_neighbors=6, indices=True)
        check_selection(g, raw(g, dc), counts >= 6, got, idx, n)


def test_the_strided_regime_in_a_child(mods):
    """NDT_OUTLIER_MAX_BLOCKS=3: three blocks stride over the passes of small clouds (tests/outliers_child.py)"""
    env = dict(os.environ, NDT_OUTLIER_MAX_BLOCKS="3")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "outliers_child.py")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["cases"] >= 6 and res["max_blocks_seen"] == 3, res


def test_values_to_device_memory_are_the_same_bits(mods, g):
    from test_gpu_parity import _DeviceCopies
    xyz = CASES["non-finite rows"][0]
    dc = g.uploadCloud(xyz)
    with _DeviceCopies() as dev:
        for kw in (dict(mean_k=8, stddev_mul=1.0), dict(radius=0.3, min_neighbors=3)):
            host, st = g.neighborValues(dc, **kw)
            buf = dev.put(np.full(2 * len(xyz), -7.0, F))          # room for len(xyz) doubles
            ptr, st_d = g.neighborValues(dc, device=buf, **kw)
            assert ptr == buf and same_stats(st, st_d)
            back = np.zeros(len(xyz))
            assert dev.hip.hipMemcpy(back.ctypes.data, buf, back.nbytes, 2) == 0  # hipMemcpyDeviceToHost
            assert back.tobytes() == host.tobytes()
            # ... and straight into a selection as its keys: the kept set of removeOutliers
            by_keys, idx = g.selectCloud(dc, keys=buf, key_range=(float("-inf"), st["threshold"]) if "mean_k" in kw else (st["threshold"], float("inf")),
                                         indices=True)
            assert np.array_equal(idx, g.removeOutliers(dc, indices=True, **kw)[2])


# ---------------------------------------------------------------------------------------------------- many clouds
@pytest.mark.parametrize("spec", oc.RAGGED_SPECS, ids=("stat", "stat negated", "radius", "radius negated"))
def test_many_clouds_match_the_single_calls(mods, g, spec):
    parts = oc.ragged()
    kw = dict(negate=spec["negate"], **kw_of(spec))
    for order in (list(range(len(parts))), list(range(len(parts)))[::-1]):
        ins = [g.uploadCloud(parts[j]) for j in order]
        outs, sts = g.removeOutliersClouds(ins, **kw)
        d = g.outlierDiag()
        assert d["value_launches"] == 1 and d["index_builds"] == sum(1 for j in order if len(parts[j]))
        assert d["value_blocks"] == sum(g.outlierPlan(len(parts[j]))[0] for j in order)
        for j, dc, out, st in zip(order, ins, outs, sts):
            one, st1, idx = g.removeOutliers(dc, indices=True, **kw)
            assert same_stats(st, st1), (j, st, st1)
            assert np.array_equal(raw(g, one), raw(g, out)) and np.array_equal(one.bounds()[0], out.bounds()[0]) and one.bounds()[1] == out.bounds()[1], j
            ref = oc.reference(parts[j], **spec)
            check_selection(g, raw(g, dc), ref["keep"], out, None, (j, spec))
            assert np.array_equal(idx, np.flatnonzero(ref["keep"]))
        for out in outs[::2]:                     # the slices are clouds of their own
            out.release()
        for j, out in list(zip(order, outs))[1::2]:
            assert len(raw(g, out)) == int(oc.reference(parts[j], **spec)["keep"].sum())
    assert g.removeOutliersClouds([], **kw) == ([], [])


# ---------------------------------------------------------------------------------------------------- producers and consumers
def test_every_kind_of_input_cloud(mods, g):
    pts = oc.with_nonfinite(oc.surface(12000, 21, outliers=30, scale=20.0), every=97)
    filt, _ = g.voxelGridFilterCloud(pts, 0.15, is_dense=False)
    slices = g.selectClouds([g.uploadCloud(pts[:7000]), g.uploadCloud(pts[7000:])], finite=True, range=(0, 25))
    first, _ = g.removeOutliers(g.uploadCloud(pts), radius=0.5, min_neighbors=4)
    for what, dc in (("uploaded", g.uploadCloud(pts)), ("filter output", filt), ("slice of a selection", slices[0]), ("slice of a selection", slices[1]),
                     ("output of removeOutliers", first)):
        records = raw(g, dc)
        xyz = np.ascontiguousarray(xyz_of(records))
        for spec in (oc.stat(10, 1.0), oc.rad(0.5, 6)):
            ref = oc.reference(xyz, **spec)
            assert oc.threshold_margin(ref) > 1e-9 or spec["method"] == oc.RADIUS
            assert 0 < ref["keep"].sum() < len(xyz), what
            got, st, idx = g.removeOutliers(dc, indices=True, **kw_of(spec))
            check_selection(g, records, ref["keep"], got, idx, (what, spec))
            assert np.array_equal(raw(g, dc), records), what             # the input is left as it was


def test_the_result_is_the_cloud_an_upload_of_the_kept_rows_would_be(mods, pair):
    ndt = mods[0]
    t, s = pair
    s = np.ascontiguousarray(s[:20000])
    spec = oc.stat(12, 0.8)
    ref = oc.reference(s, **spec)
    mask = ref["keep"]
    assert 0 < mask.sum() < len(s) and oc.threshold_margin(ref) > 1e-9

    def both(make):
        res = []
        for form in ("filter", "upload"):
            h = ndt.NormalDistributionsTransform()
            dc = h.removeOutliers(h.uploadCloud(s), **kw_of(spec))[0] if form == "filter" else h.uploadCloud(s[mask])
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

    def through_map(h, dc):
        h.mapUpdateCloud(dc, leaf_size=0.5)
        return h.mapGet()
    a, b = both(through_map)
    assert a.tobytes() == b.tobytes() and len(a) > 0

    def through_accumulate(h, dc):
        h.targetAccumulateCloud(dc)
        return bytes(h.targetAccumulateExport())
    a, b = both(through_accumulate)
    assert a == b and len(a) > 0


# ---------------------------------------------------------------------------------------------------- refusals, untouched state
def test_refusals_with_a_cloud_in_hand(mods, g):
    ndt, _lib, L = mods
    dc = g.uploadCloud(CASES["a line"][0])
    bad = g.outlierSpec(mean_k=8, stddev_mul=1.0)
    bad.mean_k = 257
    out, nk = C.c_void_p(0x5A5A), C.c_size_t(77)
    assert L.ndt_cloud_remove_outliers(g._h, dc._c, C.byref(bad), C.byref(out), None, C.byref(nk), None) == _lib.NDT_ERR_INVALID
    assert out.value is None and nk.value == 77
    out = C.c_void_p(0x5A5A)
    assert L.ndt_cloud_remove_outliers(g._h, dc._c, None, C.byref(out), None, C.byref(nk), None) == _lib.NDT_ERR_INVALID and out.value is None
    vals = np.full(len(dc), -7.0)
    assert L.ndt_cloud_neighbor_values(g._h, dc._c, C.byref(bad), C.c_void_p(vals.ctypes.data), 0, None) == _lib.NDT_ERR_INVALID
    assert L.ndt_cloud_neighbor_values(g._h, dc._c, C.byref(g.outlierSpec(mean_k=8)), None, 0, None) == _lib.NDT_ERR_INVALID
    assert (vals == -7.0).all()
    ok = g.outlierSpec(radius=0.5, min_neighbors=1)
    outs, arr = (C.c_void_p * 2)(0x5A5A, 0x5A5A), (C.c_void_p * 2)(dc._c, None)
    assert L.ndt_cloud_remove_outliers_clouds(g._h, arr, 2, C.byref(ok), outs, None, None) == _lib.NDT_ERR_INVALID
    assert outs[0] is None and outs[1] is None
    # an empty cloud: an empty result, never NULL
    empty, st = g.removeOutliers(g.uploadCloud(np.zeros((0, 3), F)), mean_k=8, stddev_mul=1.0)
    assert len(empty) == 0 and empty.bounds()[1] == "none" and st == dict(n_finite=0, n_valid=0, mean=0.0, stddev=0.0, threshold=0.0)
    assert g.outlierDiag() == dict(index_builds=0, value_launches=0, value_blocks=0, scanned_queries=0)


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
    pending = g.uploadCloud(s[:5000])
    ref_filtered = raw(g, g.voxelGridFilterCloud(s[:5000], 0.5)[0])
    g.voxelGridFilterBegin(pending, 0.5)

    def state():
        return (g.getFinalTransformation().tobytes(), g.hasConverged(), g.getFinalNumIteration(), g.getTransformationProbability(),
                repr(g.stats()), g.grid_counts(), g.inputBounds("source")[0].tobytes(), g.inputBounds("source")[1], g.inputBounds("target")[0].tobytes(),
                g.mapSize(), g.scorePosesLaunches(), g.nvtlLaunches(), repr(g.selectDiag()))
    before = state()
    for kw in (dict(mean_k=8, stddev_mul=1.0), dict(radius=0.5, min_neighbors=3)):
        g.neighborValues(dc, **kw)
        assert state() == before
        g.removeOutliers(dc, indices=True, **kw)
        assert state() == before
        g.removeOutliersClouds([dc, g.uploadCloud(s[:100])], **kw)
        assert state() == before
    g.outlierDiag()
    out, ov = g.voxelGridFilterEnd()
    assert np.array_equal(raw(g, out), ref_filtered) and not ov
    T0 = g.getFinalTransformation().tobytes()
    g.align()
    assert g.getFinalTransformation().tobytes() == T0


# ---------------------------------------------------------------------------------------------------- the app
def test_map_sequence_outlier_flags(mods, pair, tmp_path):
    """apps/map_sequence --scan-to-map --outliers-radius / --outliers-stat on two synthetic PCD files against the same loop in
    Python: removed counts exact, the registration's transform within 1e-5 (the bound of the other app tests)"""
    ndt = mods[0]
    d = tmp_path / "pcd"
    d.mkdir()
    scans = []
    for k, x in enumerate(pair, 1):
        path = str(d / ("cloud_%d.pcd" % k))
        ndt.pcd_write_xyz(path, np.ascontiguousarray(x[::2]))
        scans.append(np.ascontiguousarray(ndt.pcd_read_xyz(path)[0][:, :3], dtype=F))
    exe = build_app(tmp_path, "map_sequence")
    runs = {"radius": (["--outliers-radius", "0.5", "2"], [dict(radius=0.5, min_neighbors=2)]),
            "stat": (["--outliers-stat", "20", "1.0"], [dict(mean_k=20, stddev_mul=1.0)]),
            "both": (["--outliers-stat", "20", "1.0", "--outliers-radius", "0.5", "2"], [dict(radius=0.5, min_neighbors=2), dict(mean_k=20, stddev_mul=1.0)])}
    plain = subprocess.check_output([exe, "--scan-to-map", str(d)], text=True)
    assert "outliers removed:" not in plain
    for args in (["--outliers-radius", "0.5", "2", str(d)], ["--scan-to-map", "--outliers-radius", "0", "2", str(d)], ["--scan-to-map", "--outliers-radius", "0.5", "-1", str(d)],
                 ["--scan-to-map", "--outliers-stat", "0", "1.0", str(d)], ["--scan-to-map", "--outliers-stat", "257", "1.0", str(d)],
                 ["--scan-to-map", "--outliers-stat", "20", "nan", str(d)], ["--scan-to-map", "--outliers-stat", "20"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage: map_sequence" in r.stderr, args

    def transforms(out):
        lines = out.splitlines()
        return [np.array([[float(x) for x in lines[i + 1 + r].split()] for r in range(4)]) for i, ln in enumerate(lines) if ln.startswith("Transform ")]
    for name, (flags, steps) in runs.items():
        out = subprocess.check_output([exe, "--scan-to-map"] + flags + [str(d)], text=True)
        g = ndt.NormalDistributionsTransform()
        app_settings(g)
        want, removed, prev = [], [], np.eye(4, dtype=F)
        for k, x in enumerate(scans):
            dc = g.uploadCloud(x)
            for kw in steps:
                n = len(dc)
                dc = g.removeOutliers(dc, **kw)[0]
                removed.append((n - len(dc), n))
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
        got_removed = [tuple(int(x) for x in m) for m in re.findall(r"^outliers removed: (\d+)/(\d+)$", out, re.M)]
        print(name, "removed: app", got_removed, "python", removed)
        assert got_removed == removed and all(0 < a < b for a, b in removed), name
        got = transforms(out)
        print(name, "app", got, "python", want)
        assert len(got) == len(want) == 1 and np.abs(got[0] - want[0]).max() <= 1e-5, name
