"""GPU: the centroid cloud of a target (ndt_grid_centroids*) and getFitnessScore against it (ndt_get_centroid_fitness_score,
ndt_batch_centroid_fitness_scores*), on cloud targets and accumulated ones, dense and sparse.

The lever is test_gpu_fitness_edges': a scan of ONE point through the batch call returns that query's squared nearest distance
(f32 widened to f64), compared BIT FOR BIT with tests/fitness_cases.nearest_d2 over the expected cloud
(tests/centroid_fitness_cases.centroid_cloud).  Means of multi-point scans are compared at 1e-12 relative, the bound the
project's fitness tests hold for means (the block sums may be ordered differently).

Sizes that follow from the search as implemented (ndt_centroid_fitness.hip): shells 0..2 by a team of 8 lanes, 3.. by the wave;
shells are walked while (2r+1)^3 <= table entries / 4, at least 3 (cc.shell_limit) -- the small targets here have a limit of 3,
the 40 x 40 plane one of 6; edge_queries reaches 8 shells off every box, so both sides of the hand-off (2 | 3) and of each
limit (3 | 4, 6 | 7) are queried."""
import subprocess

import numpy as np
import pytest

import centroid_fitness_cases as cc
import fitness_cases as fc
from test_gpu_pairs import build_app

pytestmark = pytest.mark.gpu

F = np.float32
DBL_MAX = fc.DBL_MAX
I4 = np.eye(4, dtype=F)
MEAN_REL = 1e-12
FORMS = [("cloud", 1), ("cloud", 2), ("acc", 1), ("acc", 2)]   # (target kind, voxel index: 1 dense table, 2 sparse hash)
FORM_IDS = ["%s-%s" % (k, "dense" if i == 1 else "sparse") for k, i in FORMS]


@pytest.fixture(scope="module")
def ndt(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import ndt
    return ndt


def make(ndt, updates, form, res=1.0, min_pts=6):
    kind, index = form
    g = ndt.NormalDistributionsTransform()
    g.setResolution(res)
    g.setMinPointPerVoxel(min_pts)
    g.setVoxelIndex(index)
    if kind == "acc":
        for u in updates:
            g.targetAccumulate(u)
    else:
        g.setInputTarget(np.concatenate(updates), is_dense=True)
    return g


def members(g, scans, T=I4, max_range=DBL_MAX):
    return g.batchCentroidFitness(scans, transforms=[T] * len(scans), max_range=max_range)


def per_query(g, q, T=I4, max_range=DBL_MAX):
    return np.concatenate([members(g, [q[i:i + 1] for i in range(a, min(a + 65535, len(q)))], T, max_range) for a in range(0, len(q), 65535)])


def assert_exact(got, d2, what, max_range=DBL_MAX):
    want = fc.one_point_values(d2, max_range)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: %d of %d queries differ, first %d: got %r want %r" % (what, len(bad), len(got), bad[0], got[bad[:3]], want[bad[:3]])


def assert_mean(got, d2, what, max_range=DBL_MAX):
    want = fc.member_value(d2, max_range)
    if want == DBL_MAX:
        assert got == DBL_MAX, what
        return
    print("DEV %-40s n=%-7d rel=%.3g" % (what, len(d2), abs(got - want) / want if want else abs(got)))
    assert got == pytest.approx(want, rel=MEAN_REL, abs=0.0), what


def check_cloud(g, want_xyz, what):
    """gridCentroids and the cloud form against the expected cloud, indices against the dump -> the (V, 3) cloud"""
    xyz1, idx = g.gridCentroids()
    grid = g.grid()
    in_c = (grid["n"] >= g_min_pts(g)) | (grid["n"] == -1)
    assert np.array_equal(idx, grid["idx"][in_c]), what
    assert xyz1.shape == (len(want_xyz), 4) and np.array_equal(xyz1[:, :3], want_xyz), what
    assert (xyz1[:, 3] == 1.0).all()
    dc = g.gridCentroidsCloud()
    assert len(dc) == len(want_xyz)
    if len(want_xyz):
        assert np.array_equal(dc.numpy(), xyz1[:, :3]), what
    return xyz1[:, :3]


def g_min_pts(g):
    return g._test_min_pts if hasattr(g, "_test_min_pts") else 6


# ------------------------------------------------------------------------------------------------ 1. the centroid cloud
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_centroid_cloud_of_every_form(ndt, form):
    u = cc.mixed_target()
    want, _ = cc.centroid_cloud(np.concatenate(u), 1.0, 6)
    g = make(ndt, u, form)
    grid = g.grid()
    assert ((grid["n"] > 0) & (grid["n"] < 6)).any()             # a voxel under min_pts (the rejected voxel: the next test)
    got = check_cloud(g, want, str(form))
    q = cc.edge_queries(want, np.concatenate(u), 1.0, np.random.default_rng(11), 60)
    assert_exact(per_query(g, q), fc.nearest_d2(got, q)[0], "mixed " + str(form))
    if form[0] == "acc":
        # a voxel crosses min_pts on the later update: the cloud after the first update alone lacks it
        g0 = make(ndt, u[:1], form)
        w0, _ = cc.centroid_cloud(u[0], 1.0, 6)
        assert len(w0) < len(want)
        check_cloud(g0, w0, "first update " + str(form))
        bx, _ = cc.centroids_from_blob(g.targetAccumulateExport(), 6)
        assert np.array_equal(bx, want)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_a_rejected_voxel_is_in_the_cloud(ndt, form):
    pts, cell = cc.rejected_target()
    want, _ = cc.centroid_cloud(pts, 1.0, 6)
    g = make(ndt, [pts], form)
    grid = g.grid()
    assert (grid["n"] == -1).sum() == 1 and ((grid["n"] > 0) & (grid["n"] < 6)).sum() == 1 and len(want) == 15
    got = check_cloud(g, want, "rejected " + str(form))
    rng = np.random.default_rng(16)
    q = (np.asarray(cell, np.float64) + [-6, -6, -3] + rng.random((300, 3)) * [12, 12, 6]).astype(F)
    q = np.concatenate([q, want[(cc.cloud_cells(pts, 1.0, 6) == np.asarray(cell)).all(axis=1)] + F(0.01)])    # beside the rejected voxel's centroid
    assert_exact(per_query(g, q), fc.nearest_d2(got, q)[0], "rejected " + str(form))


def test_equivalence_with_the_point_fitness_of_a_second_handle(ndt):
    u = cc.mixed_target()
    g = make(ndt, u, ("acc", 1))
    dc = g.gridCentroidsCloud()
    b = ndt.NormalDistributionsTransform()
    b.setResolution(1.0)
    b.setInputTargetCloud(dc, is_dense=True)
    want, _ = cc.centroid_cloud(np.concatenate(u), 1.0, 6)
    q = cc.edge_queries(want, np.concatenate(u), 1.0, np.random.default_rng(12), 200)
    a = per_query(g, q)
    p = b.batchFitness([q[i:i + 1] for i in range(len(q))], transforms=[I4] * len(q))
    assert np.array_equal(a, p)


def test_bucket_form_before_its_records_are_compacted(ndt):
    rng = np.random.default_rng(13)
    pts = (rng.random((66000, 3)) * [60, 60, 4]).astype(F)      # ~4.6 points a cell: voxels either side of min_pts
    g = ndt.NormalDistributionsTransform()
    g.setResolution(1.0)
    g.setVoxelIndex(1)
    g.setInputTarget(pts, is_dense=True)
    gb = g.gridBuild()
    assert gb["form"] == "buckets" and gb["compact_pending"], gb
    want, _ = cc.centroid_cloud(pts, 1.0, 6)
    xyz1, idx = g.gridCentroids()
    assert g.gridBuild()["compact_pending"]
    assert 1000 < len(want) < 14400 and np.array_equal(xyz1[:, :3], want)
    q = (rng.random((400, 3)) * [70, 70, 14] - [5, 5, 5]).astype(F)
    assert_exact(per_query(g, q), fc.nearest_d2(want, q)[0], "uncompacted")        # (the table scan meets the same records)
    assert g.gridBuild()["compact_pending"]


def test_one_launch_build_and_empty_clouds(ndt):
    rng = np.random.default_rng(14)
    pts = cc.voxel_points([(i, j, 0) for i in range(5) for j in range(4)], rng, pts=7)
    g = make(ndt, [pts], ("cloud", 0))
    print("build form:", g.gridBuild()["form"])
    check_cloud(g, cc.centroid_cloud(pts, 1.0, 6)[0], "small")
    for form in FORMS:                                           # every voxel under min_pts: an empty cloud, DBL_MAX everywhere
        e = make(ndt, cc.under_target(), form)
        check_cloud(e, np.zeros((0, 3), F), "empty " + str(form))
        q = np.array([[0.5, 0.5, 0.5], [30, 2, 1]], dtype=F)
        assert (members(e, [q, q[:1], q[:0]]) == DBL_MAX).all()
        assert (members(e, [q], max_range=np.inf) == DBL_MAX).all()      # (no centroid: nothing to accept, whatever the range)
        e.setInputSource(q)
        assert e.centroidFitnessScore() == DBL_MAX
        assert members(e, []).shape == (0,)


def test_accumulated_after_crop_import_and_growth(ndt, monkeypatch):
    monkeypatch.setenv("NDT_ACC_SLOTS", "16")
    monkeypatch.setenv("NDT_ACC_HASH_BITS", "2")
    rng = np.random.default_rng(15)
    u = [cc.voxel_points([(i, j, k) for i in range(6 * n, 6 * n + 6) for j in range(5) for k in (0, 1)], rng, pts=5 + n) for n in range(3)]
    g = make(ndt, u[:1], ("acc", 0))
    grown = []
    for x in u[1:]:
        g.targetAccumulate(x)
        grown.append(g.targetAccumulateDiag()["table_grown"])
    assert all(grown)                                            # 60 slots a update against 16: the slot arrays were doubled and copied
    cat = np.concatenate(u)
    want, _ = cc.centroid_cloud(cat, 1.0, 6)
    assert len(want) == 120                                      # the first update's voxels hold 5 points: under min_pts
    got = check_cloud(g, want, "grown")
    assert np.array_equal(cc.centroids_from_blob(g.targetAccumulateExport(), 6)[0], want)
    q = cc.edge_queries(want, cat, 1.0, rng, 80)
    assert_exact(per_query(g, q), fc.nearest_d2(got, q)[0], "grown")
    # crop: the cells x <= 13 stay; the indices are over the new box
    blob_all = g.targetAccumulateExport()
    g.targetAccumulateCrop([-np.inf] * 3, [13.5, np.inf, np.inf])
    keep = cc.cells_of(cat, 1.0)[:, 0] <= 13
    wc, _ = cc.centroid_cloud(cat[keep], 1.0, 6)
    assert 0 < len(wc) < len(want)
    check_cloud(g, wc, "cropped")
    assert_exact(per_query(g, q), fc.nearest_d2(wc, q)[0], "cropped")
    # import into a fresh handle
    b = ndt.NormalDistributionsTransform()
    b.setResolution(1.0)
    b.targetAccumulateImport(blob_all)
    check_cloud(b, want, "imported")
    assert_exact(per_query(b, q), fc.nearest_d2(want, q)[0], "imported")


# ------------------------------------------------------------------------------------------------ 2. the search edges
@pytest.fixture(scope="module")
def shapes():
    rng = np.random.default_rng(21)
    out = {}
    for name, cells in cc.shape_targets().items():
        pts = cc.voxel_points(cells, rng)
        xyz, _ = cc.centroid_cloud(pts, 1.0, 6)
        q = cc.edge_queries(xyz, pts, 1.0, np.random.default_rng(22))
        out[name] = (pts, xyz, q, fc.nearest_d2(xyz, q)[0])
    return out


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", list(cc.shape_targets()))
def test_search_edges(ndt, shapes, name, form):
    pts, xyz, q, d2 = shapes[name]
    g = make(ndt, [pts], form)
    got = per_query(g, q)
    assert_exact(got, d2, "%s %s" % (name, form))
    assert np.array_equal(got, per_query(g, q))                  # run to run
    assert_mean(members(g, [q])[0], d2, "%s %s mean" % (name, form))
    if form == FORMS[0]:
        lim = cc.shell_limit(g.grid()["div_b"])
        assert lim == min(3, int(max(g.grid()["div_b"]))) and np.sqrt(d2[np.isfinite(d2)].astype(np.float64)).max() > lim + 2     # both sides of the bound are queried


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_plane_with_a_larger_shell_limit_transforms_ties_and_ranges(ndt, form):
    rng = np.random.default_rng(23)
    pts = cc.voxel_points([(i, j, 0) for i in range(40) for j in range(40)], rng, pts=6)
    xyz, _ = cc.centroid_cloud(pts, 1.0, 6)
    g = make(ndt, [pts], form)
    if form[1] == 1:
        assert cc.shell_limit(g.grid()["div_b"]) == 6
    q = np.concatenate([np.c_[rng.random((40, 2)) * 40, np.full(40, h + 0.5)] for h in range(1, 10)] +
                       [np.c_[rng.random((40, 2)) * 40, np.full(40, -h - 0.5)] for h in (2, 3, 6, 7)]).astype(F)   # h shells above / below the plane
    assert_exact(per_query(g, q), fc.nearest_d2(xyz, q)[0], "plane " + str(form))
    for T in cc.transforms():                                     # non-identity transforms
        moved = fc.se3_f32(T, q[::3])
        assert_exact(per_query(g, q[::3], T), fc.nearest_d2(xyz, moved)[0], "plane moved " + str(form))
    # max_range at, one ulp under and one ulp over a query's d2
    d2 = fc.nearest_d2(xyz, q[:12])[0]
    for k in range(12):
        d = float(d2[k])
        for r in (d, np.nextafter(d, 0.0), np.nextafter(d, np.inf)):
            assert_exact(per_query(g, q[k:k + 1], max_range=r), d2[k:k + 1], "range", r)
    assert_mean(members(g, [q], max_range=float(np.median(d2)))[0], fc.nearest_d2(xyz, q)[0], "plane ranged", float(np.median(d2)))
    t, tq = cc.tie_target()                                       # ties between two centroids
    gt = make(ndt, [t], form)
    assert_exact(per_query(gt, tq), fc.nearest_d2(cc.centroid_cloud(t, 1.0, 6)[0], tq)[0], "tie " + str(form))


# ------------------------------------------------------------------------------------------------ 3. the excursion
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_excursion(ndt, form):
    pts, big = cc.excursion_target()
    xyz, _ = cc.centroid_cloud(pts, 1.0, 6)
    own = cc.excursion_of(xyz, cc.cloud_cells(pts, 1.0, 6))
    assert own >= 2.0
    g = make(ndt, [pts], form)
    got = check_cloud(g, xyz, "excursion " + str(form))
    q = cc.excursion_queries(pts, big)
    assert_exact(per_query(g, q), fc.nearest_d2(got, q)[0], "excursion " + str(form))
    d = g.centroidFitnessDiag()
    print("excursion: fixture %.6g, reported %.6g" % (own, d["excursion"]))
    assert d["excursion"] >= own
    near, nbig = cc.excursion_target(base=1000.0)
    gn = make(ndt, [near], form)
    nq = cc.excursion_queries(near, nbig)
    assert_exact(per_query(gn, nq), fc.nearest_d2(cc.centroid_cloud(near, 1.0, 6)[0], nq)[0], "1 km " + str(form))
    assert gn.centroidFitnessDiag()["excursion"] == 0.0


def test_excursion_cache(ndt):
    rng = np.random.default_rng(31)
    u0 = cc.voxel_points([(i, j, 0) for i in range(6) for j in range(6)], rng)
    u1 = cc.voxel_points([(i, 7, 1) for i in range(3, 12)], rng)
    q = cc.edge_queries(cc.centroid_cloud(u0, 1.0, 6)[0], u0, 1.0, rng, 60)
    scans = [q[i:i + 1] for i in range(len(q))]
    for form in (("cloud", 1), ("acc", 1), ("acc", 2)):
        g = make(ndt, [u0], form)
        a = members(g, scans)
        da = g.centroidFitnessDiag()
        b = members(g, scans)
        db = g.centroidFitnessDiag()
        assert da["excursion_passes"] == 1 and da["launches"] == 3 and db["excursion_passes"] == 0 and db["launches"] == 2
        assert np.array_equal(a, b)
        assert_exact(a, fc.nearest_d2(cc.centroid_cloud(u0, 1.0, 6)[0], q)[0], "cache " + str(form))
        if form[0] != "acc":
            continue
        g.targetAccumulate(u1)                                   # one more update
        cat = np.concatenate([u0, u1])
        c = members(g, scans)
        assert g.centroidFitnessDiag()["excursion_passes"] == 1
        assert_exact(c, fc.nearest_d2(cc.centroid_cloud(cat, 1.0, 6)[0], q)[0], "after update")
        assert members(g, scans[:3]) is not None and g.centroidFitnessDiag()["excursion_passes"] == 0
        blob = g.targetAccumulateExport()
        g.targetAccumulateCrop([-np.inf] * 3, [np.inf, 6.5, np.inf])    # the second update's voxels go
        c = members(g, scans)
        assert g.centroidFitnessDiag()["excursion_passes"] == 1
        assert_exact(c, fc.nearest_d2(cc.centroid_cloud(u0, 1.0, 6)[0], q)[0], "after crop")
        g.targetAccumulateCrop([-np.inf] * 3, [2.5, np.inf, np.inf])
        g.targetAccumulateImport(cc_subset(ndt, blob, lambda r: r["i"] > 2))   # the rest comes back through an import
        c = members(g, scans)
        assert g.centroidFitnessDiag()["excursion_passes"] == 1
        assert_exact(c, fc.nearest_d2(cc.centroid_cloud(cat, 1.0, 6)[0], q)[0], "after import")


def cc_subset(ndt, blob, pick):
    """the rows of an export that `pick` keeps, exported again from a scratch handle (a well-formed blob)"""
    s = ndt.NormalDistributionsTransform()
    s.setResolution(1.0)
    s.targetAccumulateImport(blob)
    rows = ndt.acc_blob_rows(blob)
    lo = [int(rows[c][pick(rows)].min()) for c in ("i", "j", "k")]
    hi = [int(rows[c][pick(rows)].max()) for c in ("i", "j", "k")]
    assert all(pick(r) == all(lo[a] <= r[c] <= hi[a] for a, c in enumerate("ijk")) for r in rows)
    return s.targetAccumulateExport(np.asarray(lo, F) + 0.5, np.asarray(hi, F) + 0.5)


# ------------------------------------------------------------------------------------------------ 4. the launch plan
PLAN_SIZES = [1, 8, 9, 31, 32, 33, 511, 512, 513, 65504, 65505, 65536, 65537]   # a block per 32 queries, 2048 blocks at most


@pytest.fixture(scope="module")
def plan(ndt):
    rng = np.random.default_rng(41)
    pts = cc.voxel_points([(i, j, k) for i in range(0, 10, 2) for j in range(6) for k in (0, 2)], rng)
    xyz, _ = cc.centroid_cloud(pts, 1.0, 6)
    q = (rng.random((max(PLAN_SIZES), 3)) * [16, 12, 8] - [3, 3, 3]).astype(F)
    q[5::97] = np.nan
    return make(ndt, [pts], ("acc", 1)), xyz, q, fc.nearest_d2(xyz, q)[0]


@pytest.mark.parametrize("n", PLAN_SIZES)
def test_plan_boundaries(plan, n):
    g, xyz, q, d2 = plan
    got = members(g, [q[:n]])[0]
    d = g.centroidFitnessDiag()
    assert d["max_blocks"] == fc.fitness_blocks(n) == min(2048, -(-n // 32)) and d["launches"] - d["excursion_passes"] == 2
    assert_mean(got, d2[:n], "plan n=%d" % n)
    assert got == members(g, [q[:n]])[0]
    if n <= 513:
        assert_exact(per_query(g, q[:n]), d2[:n], "plan n=%d" % n)
        g.setInputSource(q[:n])                                   # the single-handle call: the batch member's bits
        g.setMaximumIterations(0)
        g.align()
        T = g.getFinalTransformation().astype(F)
        assert g.centroidFitnessScore() == members(g, [q[:n]], T=T)[0]
        assert_mean(g.centroidFitnessScore(), fc.nearest_d2(xyz, fc.se3_f32(T, q[:n]))[0], "single handle n=%d" % n)


@pytest.mark.parametrize("m", [1, 2, 300])
def test_members(plan, m):
    g, xyz, q, d2 = plan
    rng = np.random.default_rng(m)
    scans, want = [], []
    for k in range(m):
        kind = k % 5
        a = int(rng.integers(0, 60000))
        n = 0 if kind == 1 else int(rng.integers(1, 90))
        s = q[a:a + n].copy()
        if kind == 3:
            s[:] = np.nan                                         # a member without a finite point
        scans.append(s)
        want.append(fc.member_value(fc.nearest_d2(xyz, s)[0]) if n else DBL_MAX)
    got = members(g, scans)
    assert g.centroidFitnessDiag()["max_blocks"] == sum(fc.fitness_blocks(len(s)) for s in scans if len(s))
    for k in range(m):
        if want[k] == DBL_MAX:
            assert got[k] == DBL_MAX, k
        else:
            assert got[k] == pytest.approx(want[k], rel=MEAN_REL, abs=0.0), k
    assert np.array_equal(got, members(g, scans))
    solo = [members(g, [s])[0] for s in scans[:7]]                # a member's value does not depend on the members around it
    assert np.array_equal(got[:7], solo)


# ------------------------------------------------------------------------------------------------ 5. state
def test_the_calls_change_nothing(ndt):
    u = cc.mixed_target()
    src = (np.concatenate(u)[::3] + F(0.02)).astype(F)
    g = make(ndt, u, ("acc", 1))
    g.setInputSource(src)
    g.setMaximumIterations(5)
    g.align()
    T0, conv0, it0 = g.getFinalTransformation().copy(), g.hasConverged(), g.getFinalNumIteration()
    grid0, acc0 = g.grid(), g.targetAccumulated()
    g.gridCentroids()
    g.gridCentroidsCloud()
    g.centroidFitnessScore(2.0)
    members(g, [src[:40], src[:0], src[40:90]])
    g.centroidFitnessDiag()
    assert np.array_equal(g.getFinalTransformation(), T0) and g.hasConverged() == conv0 and g.getFinalNumIteration() == it0
    grid1 = g.grid()
    for k in ("idx", "n", "mean", "cov", "icov", "evals", "min_b", "max_b", "div_b"):
        assert np.array_equal(grid0[k], grid1[k]), k
    assert g.targetAccumulated() == acc0
    g.align()                                                     # a following registration: the same result
    assert np.array_equal(g.getFinalTransformation(), T0) and g.hasConverged() == conv0 and g.getFinalNumIteration() == it0
    with pytest.raises(ndt.NdtError):                             # the point fitness keeps refusing an accumulated target
        g.getFitnessScore()


# ------------------------------------------------------------------------------------------------ 6. the app
def test_map_sequence_prints_the_map_fitness(ndt, tmp_path):
    from toyslam_amd import clouds
    rng = np.random.default_rng(61)
    world = clouds.target_surfaces(24000, seed=62, extent=30.0)[:, :3].astype(F)
    pose, scans = np.eye(4), []
    for k in range(4):
        if k:
            pose = pose @ clouds.make_T(rng.uniform(-0.3, 0.3, 3) * [1, 1, 0.05], np.deg2rad(rng.uniform(-1, 1, 3) * [0.2, 0.2, 1]))
        pick = world[rng.choice(len(world), 9000, replace=False)]
        scans.append((clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(F))
    d = tmp_path / "pcd"
    d.mkdir()
    for k, sc in enumerate(scans, 1):
        ndt.pcd_write_xyz(str(d / ("cloud_%d.pcd" % k)), sc)
    exe = build_app(tmp_path, "map_sequence")
    plain = subprocess.check_output([exe, "--scan-to-map", str(d)], text=True)
    flagged = subprocess.check_output([exe, "--scan-to-map", "--map-fitness", str(d)], text=True)
    timed = lambda ln: ln.startswith("time:") or ln.startswith("start-up") or " ms" in ln
    fit = [ln for ln in flagged.splitlines() if ln.startswith("map fitness: ")]
    assert len(fit) == 3 and "registrations 3" in flagged
    assert "map fitness" not in plain
    assert [ln for ln in plain.splitlines() if not timed(ln)] == [ln for ln in flagged.splitlines() if not timed(ln) and not ln.startswith("map fitness: ")]
    assert subprocess.run([exe, "--map-fitness", str(d)], capture_output=True).returncode == 2     # goes with --scan-to-map
    assert subprocess.run([exe, "--scan-to-map", "--map-fitness", str(d), "0.5", "-", "rosbag"], capture_output=True).returncode == 2
    # the same loop in Python, with the app's settings
    g = ndt.NormalDistributionsTransform()
    app_settings(g)
    want, prev = [], np.eye(4, dtype=F)
    for k, sc in enumerate(scans):
        dc, _ = g.voxelGridFilterCloud(sc, 0.5)
        if k == 0:
            g.targetAccumulateCloud(dc)
            continue
        g.setInputSourceCloud(dc)
        g.align(prev)
        want.append(g.centroidFitnessScore())
        if g.hasConverged():
            prev = g.getFinalTransformation().astype(F)
            g.targetAccumulateCloud(dc, prev)
    got = [float(ln.split(":")[1]) for ln in fit]
    print("map fitness: app", got, "python", want)
    assert got == pytest.approx(want, rel=1e-5)


def app_settings(g):
    """apps/map_sequence.cpp configure(): the mapping node's parameters"""
    g.setResolution(1.0)
    g.setStepSize(0.1)
    g.setTransformationEpsilon(0.01)
    g.setMaximumIterations(64)
