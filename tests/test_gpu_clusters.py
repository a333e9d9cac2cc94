"""GPU: ndt_cloud_cluster / ndt_cloud_extract_clusters / ndt_cloud_extract_clusters_clouds against the numpy restatement of the
definitions (tests/cluster_cases.py).

Bounds (derived, not measured):
  labels, roots, sizes, the table's root / size / first / boxes, indices, the summary, kept indices / records / order / boxes:
  EXACT on every cloud -- the device and the reference compute the same f32 d2 with the same operation order, so no case needs
  clearance from tol2 and none is left out
  centroids: within size * 2^-53 * sum|x| per axis of the math.fsum value (a sum of `size` f64 terms in any order), and the
  same bits in two calls, whatever the capacity and whatever else the call is asked for
  single call, many-clouds call, labels to the host / to device memory: the same bits
cas_retries varies from run to run and is only ever printed or compared with >= 0."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cluster_cases as cc
from test_gpu_centroid_fitness import app_settings
from test_gpu_pairs import build_app
from test_gpu_select import check_selection, raw, xyz_of

pytestmark = pytest.mark.gpu

F = np.float32
CASES = cc.gpu_cases()
NO_DIAG = dict(index_builds=0, launches=0, link_blocks=0, scanned_queries=0, cas_retries=0)


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import _lib, ndt
    return ndt, _lib, built_lib


@pytest.fixture(scope="module")
def g(mods):
    return mods[0].NormalDistributionsTransform()


def fixed(d):
    """a diag without the one field that varies from run to run"""
    return {k: v for k, v in d.items() if k != "cas_retries"}


def check_table(xyz, table, ref, rows, what):
    want = ref["table"][:rows]
    assert table.dtype == cc.CLUSTER_DTYPE and len(table) == len(want), what
    for f in ("root", "size", "first", "box_min", "box_max"):
        assert np.array_equal(table[f], want[f]), (what, f)
    for c in range(len(want)):
        run = ref["indices"][want["first"][c]:want["first"][c] + want["size"][c]]
        err = np.abs(table["centroid"][c] - want["centroid"][c])
        assert (err <= cc.centroid_bound(xyz, run)).all(), (what, c, err)


def check_case(g, name, xyz, sp, scan=None):
    """one (cloud, spec): the labelling call, the extraction in both senses, the many-clouds form of one"""
    what = (name, sp)
    ref = cc.reference_of(name, xyz, sp)
    n, s = len(xyz), ref["summary"]
    dc = g.uploadCloud(xyz)
    records = raw(g, dc)
    labels, table, indices, summary, roots = g.clusterCloud(dc, roots=True, **sp)
    d = g.diagClusters()
    C_ = s["n_clusters"]
    front = 3 + (1 if s["n_finite"] else 0)  # parents, link (only with a finite point), flatten, keys
    assert fixed(d) == dict(index_builds=1, launches=front + 1 + (3 if C_ else 0), link_blocks=g.clusterPlan(n)[0] if s["n_finite"] else 0,
                            scanned_queries=d["scanned_queries"]), (what, d)
    if scan is not None:
        assert (d["scanned_queries"] > 0) == scan, (what, d)
    assert summary == s, (what, summary, s)
    assert labels.dtype == np.int32 and np.array_equal(labels, ref["labels"]), what
    assert np.array_equal(roots, ref["roots"]) and np.array_equal(indices, ref["indices"]) and indices.dtype == np.int32, what
    check_table(xyz, table, ref, C_, what)
    # the same call again: byte for byte
    again = g.clusterCloud(dc, roots=True, **sp)
    assert again[0].tobytes() == labels.tobytes() and again[1].tobytes() == table.tobytes() and again[2].tobytes() == indices.tobytes(), what
    assert again[3] == summary and again[4].tobytes() == roots.tobytes(), what
    # the extraction: the clustered points, and with negate the finite points of no cluster
    for negate, mask in ((False, ref["keep"]), (True, ref["others"])):
        got, s2, idx = g.extractClusters(dc, negate=negate, indices=True, **sp)
        d2 = g.diagClusters()
        assert s2 == s and fixed(d2) == dict(fixed(d), launches=front), (what, negate, d2)
        check_selection(g, records, mask, got, idx, (what, negate))
        outs, sums = g.extractClustersClouds([dc], negate=negate, **sp)
        assert sums == [s] and np.array_equal(raw(g, outs[0]), raw(g, got)) and outs[0].bounds()[1] == got.bounds()[1], (what, negate)
        assert np.array_equal(outs[0].bounds()[0], got.bounds()[0]), (what, negate)
    assert np.array_equal(raw(g, dc), records), what  # the input is left as it was


# The index leaf follows the tolerance, so a query leaves the shell walk only where the index slack is large against the leaf:
# the 100 km cloud under a tolerance of 0.05, whose queries take the whole-cloud scan (the RADIUS filter's case of the same kind)
SCANS = {("100 km from the origin", float(F(0.05))): True, ("100 km from the origin", 0.5): False, ("components over many cells", 0.5): False}


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_against_the_definitions(mods, g, name):
    xyz, specs = CASES[name]
    for sp in specs:
        check_case(g, name, xyz, sp, SCANS.get((name, sp["tolerance"])))


def test_the_chain_is_one_component_in_any_order(mods, g):
    """4 096 points on a line at 0.9 tolerance: one component, deep union-find paths, the most contention a small case gives"""
    for order in ("shuffled", "ascending", "descending"):
        xyz = CASES["chain, %s" % order][0]
        labels, table, indices, summary, roots = g.clusterCloud(g.uploadCloud(xyz), 0.5, roots=True)
        print(order, g.diagClusters())
        assert summary == dict(n_finite=4096, n_components=1, n_clusters=1, n_clustered=4096, largest=4096)
        assert not labels.any() and not roots.any() and np.array_equal(indices, np.arange(4096))
        assert (table["root"][0], table["size"][0], table["first"][0]) == (0, 4096, 0)


def test_either_side_of_the_block_cap(mods, g):
    """the point counts at which the plan reaches its cap and first strides, on a cloud whose components are known by
    construction: blobs inside cubes of 0.4, 20 apart"""
    plan = g.clusterPlan
    cap = plan(10 ** 6)[0]
    n_cap = 8 * cap
    assert plan(n_cap) == (cap, 8) and plan(n_cap + 1) == (cap, 16)
    # n_cap + 1 points in blobs of 41 inside cubes of 0.4, 20 apart on a line, rows shuffled: every blob one component at 0.8
    sizes = [41] * (n_cap // 41) + [n_cap + 1 - 41 * (n_cap // 41)]
    rng = np.random.default_rng(5)
    blob_of = np.repeat(np.arange(len(sizes)), sizes)
    full = (np.column_stack([20.0 * blob_of, np.zeros(n_cap + 1), np.zeros(n_cap + 1)]) + 0.4 * rng.random((n_cap + 1, 3))).astype(F)
    perm = rng.permutation(n_cap + 1)
    full, blob_of = full[perm], blob_of[perm]
    for n in (n_cap, n_cap + 1):
        xyz, blob = full[:n], blob_of[:n]
        first = np.full(len(sizes), n, np.int64)
        np.minimum.at(first, blob, np.arange(n))
        dc = g.uploadCloud(xyz)
        labels, table, indices, summary, roots = g.clusterCloud(dc, 0.8, min_size=41, roots=True, capacity=16)
        assert g.diagClusters()["link_blocks"] == cap
        assert np.array_equal(roots, first[blob].astype(np.int32))
        count = np.bincount(blob, minlength=len(sizes))
        assert summary == dict(n_finite=n, n_components=int((count > 0).sum()), n_clusters=int((count == 41).sum()),
                               n_clustered=41 * int((count == 41).sum()), largest=41)
        assert np.array_equal(labels >= 0, count[blob] == 41) and len(table) == 16 and (table["size"] == 41).all()
        assert (np.diff(table["root"]) > 0).all() and np.array_equal(np.flatnonzero(labels == 3), indices[table["first"][3]:table["first"][3] + 41])
        got, s2, idx = g.extractClusters(dc, 0.8, min_size=41, indices=True)
        check_selection(g, raw(g, dc), count[blob] == 41, got, idx, n)


def test_the_strided_regime_in_a_child(mods):
    """NDT_CLUSTER_MAX_BLOCKS=3: three blocks stride over the passes of small clouds (tests/clusters_child.py)"""
    env = dict(os.environ, NDT_CLUSTER_MAX_BLOCKS="3")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clusters_child.py")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["cases"] >= 6 and res["max_blocks_seen"] == 3, res


def test_capacity_and_optional_outputs(mods, g):
    name, sp = "blobs of 1 ... 59 points", cc.spec(0.8, 10, 50)
    xyz = CASES[name][0]
    ref = cc.reference_of(name, xyz, sp)
    n_cl = ref["summary"]["n_clusters"]
    assert n_cl == 41
    dc = g.uploadCloud(xyz)
    full = g.clusterCloud(dc, **sp)
    for cap in (0, 1, n_cl - 1, n_cl, n_cl + 5):
        for want_idx in (True, False):
            labels, table, indices, summary = g.clusterCloud(dc, capacity=cap, indices=want_idx, **sp)
            what = (cap, want_idx)
            assert summary == ref["summary"] and np.array_equal(labels, ref["labels"]), what
            assert (indices is None) if not want_idx else np.array_equal(indices, ref["indices"]), what
            check_table(xyz, table, ref, min(cap, n_cl), what)
            assert table.tobytes() == full[1][:min(cap, n_cl)].tobytes(), what  # the centroids do not depend on what else is asked for
    # the table is written up to the capacity and no further
    L, _lib = mods[2], mods[1]
    rows = np.full(3 * 16, -7, np.int32)
    lab = np.zeros(len(xyz), np.int32)
    st = _lib.ClusterSummary()
    spec = g.clusterSpec(**sp)
    assert L.ndt_cloud_cluster(g._h, dc._c, C.byref(spec), C.c_void_p(lab.ctypes.data), 0, None, rows.ctypes.data_as(C.POINTER(_lib.ClusterInfo)), 2,
                               None, C.byref(st)) == 0
    assert (rows[32:] == -7).all() and rows[:32].tobytes() == full[1][:2].tobytes() and st.n_clusters == n_cl
    # one cluster's cloud is a selection by label
    one, idx = g.selectCloud(dc, keys=labels.astype(np.float64), key_range=(3, 3), indices=True)
    assert np.array_equal(idx, np.flatnonzero(ref["labels"] == 3)) and len(one) == ref["table"]["size"][3]


def test_labels_to_device_memory_are_the_same_bits(mods, g):
    from test_gpu_parity import _DeviceCopies
    xyz = CASES["non-finite rows"][0]
    sp = cc.spec(0.5, 5)
    dc = g.uploadCloud(xyz)
    n = len(xyz)
    host = g.clusterCloud(dc, roots=True, **sp)
    with _DeviceCopies() as dev:
        buf = dev.put(np.full(2 * n, -7.0, F))  # room for n labels and n roots
        ptr, table, indices, summary, rptr = g.clusterCloud(dc, roots=True, device=buf, **sp)
        assert ptr == buf and rptr == buf + 4 * n and summary == host[3] and table.tobytes() == host[1].tobytes() and np.array_equal(indices, host[2])
        back = np.zeros(2 * n, np.int32)
        assert dev.hip.hipMemcpy(back.ctypes.data, buf, back.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        assert back[:n].tobytes() == host[0].tobytes() and back[n:].tobytes() == host[4].tobytes()


# ---------------------------------------------------------------------------------------------------- many clouds
@pytest.mark.parametrize("sp", cc.RAGGED_SPECS, ids=("min 5", "at most 4"))
@pytest.mark.parametrize("negate", (False, True), ids=("clusters", "negated"))
def test_many_clouds_match_the_single_calls(mods, g, sp, negate):
    parts = cc.ragged()
    for order in (list(range(len(parts))), list(range(len(parts)))[::-1]):
        ins = [g.uploadCloud(parts[j]) for j in order]
        outs, sums = g.extractClustersClouds(ins, negate=negate, **sp)
        d = g.diagClusters()
        with_finite = [j for j in order if cc.finite_rows(parts[j]).any()]
        assert fixed(d) == dict(index_builds=sum(1 for j in order if len(parts[j])), launches=4, scanned_queries=d["scanned_queries"],
                                link_blocks=sum(g.clusterPlan(len(parts[j]))[0] for j in with_finite)), d
        for j, dc, out, sm in zip(order, ins, outs, sums):
            one, sm1, idx = g.extractClusters(dc, negate=negate, indices=True, **sp)
            assert sm == sm1, (j, sm, sm1)
            assert np.array_equal(raw(g, one), raw(g, out)) and np.array_equal(one.bounds()[0], out.bounds()[0]) and one.bounds()[1] == out.bounds()[1], j
            ref = cc.reference_of("ragged %d" % j, parts[j], sp)
            assert sm == ref["summary"], (j, sm)
            mask = ref["others"] if negate else ref["keep"]
            check_selection(g, raw(g, dc), mask, out, None, (j, sp))
            assert np.array_equal(idx, np.flatnonzero(mask))
        for out in outs[::2]:                     # the slices are clouds of their own
            out.release()
        for j, out in list(zip(order, outs))[1::2]:
            ref = cc.reference_of("ragged %d" % j, parts[j], sp)
            assert len(raw(g, out)) == int((ref["others"] if negate else ref["keep"]).sum())
    assert g.extractClustersClouds([], negate=negate, **sp) == ([], [])


# ---------------------------------------------------------------------------------------------------- producers and consumers
def test_nothing_and_everything_clustered(mods, g):
    xyz = CASES["components over many cells"][0]
    dc = g.uploadCloud(xyz)
    largest = cc.reference_of("components over many cells", xyz, cc.spec(0.5))["summary"]["largest"]
    none, sm = g.extractClusters(dc, 0.5, min_size=3001)
    assert len(none) == 0 and none.bounds()[1] == "none" and sm["n_clusters"] == 0 and sm["n_clustered"] == 0 and sm["largest"] == largest
    labels, table, indices, sm2 = g.clusterCloud(dc, 0.5, min_size=3001)
    assert (labels == -1).all() and len(table) == 0 and len(indices) == 0 and sm2 == sm
    every, sm, idx = g.extractClusters(dc, 0.5, indices=True)
    assert sm["n_clustered"] == 3000 and np.array_equal(idx, np.arange(3000)) and np.array_equal(raw(g, every), raw(g, dc))
    rest, _ = g.extractClusters(dc, 0.5, negate=True)
    assert len(rest) == 0 and rest.bounds()[1] == "none"
    # an empty cloud: an empty result, never NULL
    empty = g.uploadCloud(np.zeros((0, 3), F))
    out, sm = g.extractClusters(empty, 0.5)
    assert len(out) == 0 and out.bounds()[1] == "none" and sm == dict(n_finite=0, n_components=0, n_clusters=0, n_clustered=0, largest=0)
    assert g.diagClusters() == NO_DIAG
    labels, table, indices, sm = g.clusterCloud(empty, 0.5, roots=False)
    assert len(labels) == 0 and len(table) == 0 and len(indices) == 0 and g.diagClusters() == NO_DIAG


def test_every_kind_of_input_cloud(mods, g):
    import outlier_cases as oc
    pts = oc.with_nonfinite(oc.surface(6000, 21, outliers=30, scale=20.0), every=97)
    filt, _ = g.voxelGridFilterCloud(pts, 0.15, is_dense=False)
    slices = g.selectClouds([g.uploadCloud(pts[:3500]), g.uploadCloud(pts[3500:])], finite=True, range=(0, 25))
    first, _ = g.extractClusters(g.uploadCloud(pts), 0.5, min_size=3)
    for what, dc in (("uploaded", g.uploadCloud(pts)), ("filter output", filt), ("slice of a selection", slices[0]), ("slice of a selection", slices[1]),
                     ("output of extractClusters", first)):
        records = raw(g, dc)
        xyz = np.ascontiguousarray(xyz_of(records))
        sp = cc.spec(0.4, 4)
        ref = cc.reference(xyz, **sp)
        assert 0 < ref["keep"].sum() < len(xyz), what
        got, sm, idx = g.extractClusters(dc, indices=True, **sp)
        assert sm == ref["summary"], what
        check_selection(g, records, ref["keep"], got, idx, (what, sp))
        assert np.array_equal(g.clusterCloud(dc, **sp)[0], ref["labels"]), what
        assert np.array_equal(raw(g, dc), records), what


def test_the_result_is_the_cloud_an_upload_of_the_kept_rows_would_be(mods, pair):
    """the consumers of test_gpu_outliers' test of the same name, fed with the extraction's output"""
    ndt = mods[0]
    t, s = pair
    s = np.ascontiguousarray(s[:8000])
    sp = cc.spec(0.4, 10)
    mask = cc.reference(s, **sp)["keep"]
    assert 0 < mask.sum() < len(s)

    def both(make):
        res = []
        for form in ("clusters", "upload"):
            h = ndt.NormalDistributionsTransform()
            dc = h.extractClusters(h.uploadCloud(s), **sp)[0] if form == "clusters" else h.uploadCloud(s[mask])
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
    dc = g.uploadCloud(CASES["equal sizes"][0])
    n = len(dc)
    bad = g.clusterSpec(0.5, 3, 2)
    out, nk = C.c_void_p(0x5A5A), C.c_size_t(77)
    assert L.ndt_cloud_extract_clusters(g._h, dc._c, C.byref(bad), 0, C.byref(out), None, C.byref(nk), None) == _lib.NDT_ERR_INVALID
    assert out.value is None and nk.value == 77
    out = C.c_void_p(0x5A5A)
    assert L.ndt_cloud_extract_clusters(g._h, dc._c, None, 0, C.byref(out), None, C.byref(nk), None) == _lib.NDT_ERR_INVALID and out.value is None
    lab = np.full(n, -7, np.int32)
    ok = g.clusterSpec(0.8)
    for spec_p, lab_p, cap in ((C.byref(bad), C.c_void_p(lab.ctypes.data), 0), (C.byref(ok), None, 0), (C.byref(ok), C.c_void_p(lab.ctypes.data), 4)):
        assert L.ndt_cloud_cluster(g._h, dc._c, spec_p, lab_p, 0, None, None, cap, None, None) == _lib.NDT_ERR_INVALID
    assert (lab == -7).all()
    outs, arr = (C.c_void_p * 2)(0x5A5A, 0x5A5A), (C.c_void_p * 2)(dc._c, None)
    assert L.ndt_cloud_extract_clusters_clouds(g._h, arr, 2, C.byref(ok), 0, outs, None, None) == _lib.NDT_ERR_INVALID
    assert outs[0] is None and outs[1] is None
    # every optional output left out
    assert L.ndt_cloud_cluster(g._h, dc._c, C.byref(ok), C.c_void_p(lab.ctypes.data), 0, None, None, 0, None, None) == 0
    assert np.array_equal(lab, cc.reference(CASES["equal sizes"][0], 0.8)["labels"])


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
    g.removeOutliers(dc, radius=0.5, min_neighbors=3)
    g.segmentPlane(dc, ndt.plane_spec(0.2, 64))
    pending = g.uploadCloud(s[:5000])
    ref_filtered = raw(g, g.voxelGridFilterCloud(s[:5000], 0.5)[0])
    g.voxelGridFilterBegin(pending, 0.5)

    def state():
        return (g.getFinalTransformation().tobytes(), g.hasConverged(), g.getFinalNumIteration(), g.getTransformationProbability(),
                repr(g.stats()), g.grid_counts(), g.inputBounds("source")[0].tobytes(), g.inputBounds("source")[1], g.inputBounds("target")[0].tobytes(),
                g.mapSize(), g.scorePosesLaunches(), g.nvtlLaunches(), repr(g.selectDiag()), repr(g.outlierDiag()), repr(g.planeDiag()))
    before = state()
    g.clusterCloud(dc, 0.4, min_size=10, roots=True)
    assert state() == before
    g.extractClusters(dc, 0.4, min_size=10, indices=True)
    assert state() == before
    g.extractClustersClouds([dc, g.uploadCloud(s[:100])], 0.4, min_size=10, negate=True)
    assert state() == before
    g.diagClusters()
    out, ov = g.voxelGridFilterEnd()
    assert np.array_equal(raw(g, out), ref_filtered) and not ov
    T0 = g.getFinalTransformation().tobytes()
    g.align()
    assert g.getFinalTransformation().tobytes() == T0


# ---------------------------------------------------------------------------------------------------- the app
def test_map_sequence_clusters_flag(mods, pair, tmp_path):
    """apps/map_sequence --scan-to-map --ground ... --ground-remove --clusters 0.5 10 on two PCD files of the golden pair against
    the same loop in Python: printed counts exact, the registration's transform within 1e-5 (the bound of the other app tests)"""
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
    assert "clusters:" not in plain
    for args in (["--clusters", "0.5", "10", str(d)], ["--scan-to-map", "--clusters", "0", "10", str(d)], ["--scan-to-map", "--clusters", "0.5", "0", str(d)],
                 ["--scan-to-map", "--clusters", "0.5", "10", "9", str(d)], ["--scan-to-map", "--clusters", "nan", "10", str(d)],
                 ["--scan-to-map", "--clusters", "0.5"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage: map_sequence" in r.stderr and "--clusters <tolerance> <min_size> [<max_size>]" in r.stderr, args

    def transforms(out):
        lines = out.splitlines()
        return [np.array([[float(x) for x in lines[i + 1 + r].split()] for r in range(4)]) for i, ln in enumerate(lines) if ln.startswith("Transform ")]
    ground = ndt.plane_spec(0.2, 128, seed=0, axis=(0, 0, 1), eps_angle=float(F(15.0 * math.pi / 180.0)))
    for flags, kw in ((["--clusters", "0.5", "10"], dict(tolerance=0.5, min_size=10)), (["--clusters", "0.5", "10", "400"], dict(tolerance=0.5, min_size=10, max_size=400))):
        out = subprocess.check_output([exe, "--scan-to-map", "--ground", "0.2", "128", "15", "--ground-remove"] + flags + [str(d)], text=True)
        g = ndt.NormalDistributionsTransform()
        app_settings(g)
        want, lines, prev = [], [], np.eye(4, dtype=F)
        for k, x in enumerate(scans):
            dc = g.uploadCloud(x)
            dc = g.segmentPlane(dc, ground, inliers=False, others=True)[2]
            n = len(dc)
            dc, sm = g.extractClusters(dc, **kw)
            lines.append((sm["n_clusters"], len(dc), n))
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
        got_lines = [tuple(int(v) for v in m) for m in re.findall(r"^clusters: (\d+) kept (\d+)/(\d+)$", out, re.M)]
        print(flags, "clusters: app", got_lines, "python", lines)
        assert got_lines == lines and all(c > 0 and 0 < k < n for c, k, n in lines), flags
        got = transforms(out)
        assert len(got) == len(want) == 1 and np.abs(got[0] - want[0]).max() <= 1e-5, flags
