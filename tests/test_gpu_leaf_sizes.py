"""GPU: every voxel search at leaf sizes that are no power of two (0.3, 0.7, 1.5, 3.0), where search_ijk takes its division
branch floorf(__fdiv_rn(x, leaf)) and the grid build bins by the product -- with points ON the cell faces, the only ones that
tell whether a kernel searches by the quotient as the reference does.  The fixtures and what they can tell are pinned on the
CPU by tests/test_leaf_cases.py; the expected values come from tests/nvtl_cases.Grid, tests/fitness_cases.nearest_d2 and
the oracle.  No tolerance is new: per-point NVTL at rel 1e-11 (test_gpu_nvtl.py), calculateScore at 1e-11 and eval within
close_sums (test_gpu_parity.py), icov within 1e-9 of its scale (test_grid_other_resolutions), the final transform within
the README's parity line; found flags, neighbour counts, voxel indices, counts, means and nearest distances are exact.

Lines starting with "DEV" print the largest deviation of each leg, "ITER" the iteration counts (NOTES.md)."""
import numpy as np
import pytest

import centroid_fitness_cases as cc
import fitness_cases as fc
import leaf_cases as lc
import nvtl_cases as nc
from conftest import rot_err, trans_err
from test_gpu_parity import ROT_TOL, TRANS_TOL, close_sums, mods  # noqa: F401  (mods: the fixture)
from test_gpu_target_accumulate import POSES
from test_leaf_cases import oracle_counts, oracle_of

pytestmark = pytest.mark.gpu

F = np.float32
I4 = np.eye(4, dtype=F)
ZERO = np.zeros(6)
REL = 1e-11                  # per-point NVTL, calculateScore, hessian_f64
MOVED_POSE = POSES[1]
DBL_MAX = fc.DBL_MAX
MAX_ONE_POINT = 60
SCENES = [(leaf, origin) for leaf in lc.LEAVES for origin in lc.ORIGINS]


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def rel_dev(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.abs(want)).max()) if got.size else 0.0


def sums_dev(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def handle(ndt, leaf, voxel_index, target=None, halves=None):
    """a handle at `leaf` over a cloud target, or over a target accumulated from the two halves in two calls"""
    g = ndt.NormalDistributionsTransform()
    g.setResolution(leaf)
    g.setMinPointPerVoxel(lc.MIN_PTS)
    g.setVoxelIndex(voxel_index)
    if halves is None:
        g.setInputTarget(target)
    else:
        for h in halves:
            g.targetAccumulate(h)
    return g


def halves_of(points):
    return points[:len(points) // 2], points[len(points) // 2:]


def observe(g, po, method, source, singles):
    """what the per-point search of a handle returns for the face points under one method -> dict of arrays and numbers"""
    g.setNeighborhoodSearchMethod(getattr(po, method))
    g.setInputSource(source)
    out, value, found = g.sourcePointNVTL(I4)
    poses, pose_found = g.nvtlPoses([I4], counts=True)
    score, grad, H, nn = g.eval(ZERO, True)
    ob = dict(per_point=out, nvtl=value, found=found, poses=poses[0], pose_found=int(pose_found[0]), calc=g.calculateScore(source),
              score=score, grad=grad, H=H, nn=nn, h64=g.hessian_f64(ZERO))
    counts = []
    for i in singles:
        g.setInputSource(source[i:i + 1])
        counts.append(g.eval(ZERO, False)[3])
    ob["single_nn"] = np.asarray(counts)
    return ob


def same_observation(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), "%s: %s differs" % (what, k)


class FaceScene:
    """face_scene(leaf, origin) with, per search method, the oracle, the numpy reference and their answers, computed once"""

    def __init__(self, po, leaf, origin):
        self.leaf, self.origin = leaf, origin
        self.t, self.s = lc.face_scene(leaf, origin)
        self.oracle, self.ref, self.want = {}, {}, {}
        differ = np.zeros(len(self.s), dtype=bool)
        for method in nc.METHODS:
            o = oracle_of(po, method, self.t, leaf)
            o.set_source(self.s)
            ref = nc.Grid.of_oracle(o, method, self.t, leaf, lc.MIN_PTS)
            q, has = ref.terms(self.s)
            L, value, found = nc.nvtl(q, has, ref.d1, ref.d2)
            value_differs, count_differs = lc.rules_differ(ref, self.s)
            differ |= value_differs | count_differs
            self.oracle[method], self.ref[method] = o, ref
            self.want[method] = dict(L=L, nvtl=value, found=found, counts=has.sum(axis=1), calc=o.calculate_score(self.s), eval=o.eval(ZERO, True),
                                     h64=o.hessian_f64(ZERO), n_differ=int((value_differs | count_differs).sum()))
        # the points at which the product rule would answer differently (all of them, at most 60) and every 40th point
        self.singles = sorted(set(np.nonzero(differ)[0][:MAX_ONE_POINT]) | set(range(0, len(self.s), 40)))
        for method in nc.METHODS:
            self.want[method]["single_nn"] = oracle_counts(self.oracle[method], self.s[self.singles])


def check_against_the_references(sc, method, ob):
    w = sc.want[method]
    ctx = "leaf %g origin %d %s" % (sc.leaf, sc.origin, method)
    hit = w["L"] >= 0
    so, go, Ho, nno = w["eval"]
    dev = (rel_dev(ob["per_point"][hit], w["L"][hit]), rel_dev(ob["calc"], w["calc"]), rel_dev(ob["score"], so), sums_dev(ob["grad"], go),
           sums_dev(ob["H"], Ho), sums_dev(ob["h64"], w["h64"]))
    print("DEV faces %-28s found %3d/%d, %2d points tell the rules apart; per-point %.3g calculateScore %.3g eval score %.3g gradient %.3g "
          "Hessian %.3g hessian_f64 %.3g" % ((ctx, w["found"], len(sc.s), w["n_differ"]) + dev))
    # the found flags: identical; the values: the NVTL test's per-point bound
    assert np.array_equal(ob["per_point"] >= 0, hit) and np.all(ob["per_point"][~hit] == -1.0), ctx
    assert ob["found"] == w["found"] == ob["pose_found"], ctx
    assert np.all(np.abs(ob["per_point"][hit] - w["L"][hit]) <= REL * np.abs(w["L"][hit])), ctx
    assert abs(ob["nvtl"] - w["nvtl"]) <= REL * abs(w["nvtl"]), ctx
    assert np.array_equal(bits([ob["poses"]]), bits([ob["nvtl"]])), ctx              # nvtlPoses([identity]): the reduction's bits
    assert ob["calc"] == pytest.approx(w["calc"], rel=REL), ctx
    assert ob["nn"] == nno == w["counts"].sum() / len(sc.s), ctx                     # the mean-neighbour value: equal
    assert ob["score"] == pytest.approx(so, rel=1e-6) and close_sums(ob["grad"], go) and close_sums(ob["H"], Ho), ctx
    assert close_sums(ob["h64"], w["h64"], rel=REL), ctx
    # one-point sources: the neighbour count is the oracle's (and the reference's)
    assert np.array_equal(w["single_nn"], w["counts"][sc.singles]), ctx
    assert np.array_equal(ob["single_nn"], w["single_nn"]), ctx


# ------------------------------------------------------------------ per-point search on face points
@pytest.mark.parametrize("leaf,origin", SCENES)
def test_face_points_under_every_method_and_target_form(mods, leaf, origin):
    ndt, po, _ = mods
    sc = FaceScene(po, leaf, origin)
    if origin == 40:
        assert all(sc.want[m]["n_differ"] >= 6 for m in ("DIRECT1", "DIRECT7", "DIRECT26"))
    dense = handle(ndt, leaf, 1, sc.t)
    seen = {}
    for method in nc.METHODS:
        seen[method] = observe(dense, po, method, sc.s, sc.singles)
        check_against_the_references(sc, method, seen[method])
    # (after the evaluations: the dump rewrites the handle's voxel records, NOTES.md "What the dump does not see")
    assert dense.grid_counts()["n_valid"] == len(sc.ref["DIRECT7"].idx) > 100
    # the sparse index, the index the library chooses, and the accumulated target: the dense handle's bits
    forms = [("sparse", handle(ndt, leaf, 2, sc.t), ("DIRECT7", "KDTREE")),
             ("chosen", handle(ndt, leaf, 0, sc.t), ("DIRECT7", "KDTREE")),
             ("accumulated dense", handle(ndt, leaf, 1, halves=halves_of(sc.t)), nc.METHODS),
             ("accumulated sparse", handle(ndt, leaf, 2, halves=halves_of(sc.t)), ("DIRECT7", "KDTREE"))]
    for name, g, methods in forms:
        for method in methods:
            same_observation(observe(g, po, method, sc.s, sc.singles), seen[method], "leaf %g origin %d %s %s" % (leaf, origin, name, method))


# ------------------------------------------------------------------ a moved pose
@pytest.mark.parametrize("leaf", lc.LEAVES)
def test_eval_at_a_moved_pose(mods, leaf):
    """The face structure does not survive the move: the division branch on generic points."""
    ndt, po, _ = mods
    t, s = lc.face_scene(leaf, 40)
    src = np.concatenate([s, t[::4]]).astype(F)
    g = handle(ndt, leaf, 0, t)
    g.setInputSource(src)
    for method in nc.METHODS:
        o = oracle_of(po, method, t, leaf)
        o.set_source(src)
        g.setNeighborhoodSearchMethod(getattr(po, method))
        score, grad, H, nn = g.eval(MOVED_POSE, True)
        so, go, Ho, nno = o.eval(MOVED_POSE, True)
        print("DEV moved leaf %g %-8s mean neighbours %.6f; score %.3g gradient %.3g Hessian %.3g"
              % (leaf, method, nn, rel_dev(score, so), sums_dev(grad, go), sums_dev(H, Ho)))
        assert nn == nno and nn > 0.3
        assert score == pytest.approx(so, rel=1e-6) and close_sums(grad, go) and close_sums(H, Ho)
        assert close_sums(g.hessian_f64(MOVED_POSE), o.hessian_f64(MOVED_POSE), rel=REL)


# ------------------------------------------------------------------ the build rule
@pytest.mark.parametrize("leaf", lc.LEAVES)
def test_target_points_on_faces_are_binned_as_the_oracle_bins_them(mods, leaf):
    ndt, po, _ = mods
    ft = lc.face_target(leaf)
    og = oracle_of(po, "DIRECT7", ft, leaf).grid()
    assert (lc.product_cells(ft, leaf) != lc.quotient_cells(ft, leaf)).any(axis=1).sum() >= 50
    scale = np.abs(og["icov"]).max(axis=(1, 2), keepdims=True) + 1e-300
    forms = [("cloud, chosen index", handle(ndt, leaf, 0, ft)), ("cloud, dense", handle(ndt, leaf, 1, ft)), ("cloud, sparse", handle(ndt, leaf, 2, ft)),
             ("accumulated, dense", handle(ndt, leaf, 1, halves=halves_of(ft))), ("accumulated, sparse", handle(ndt, leaf, 2, halves=halves_of(ft)))]
    for name, g in forms:
        gg = g.grid()
        for k in ("idx", "n", "min_b", "div_b", "mean"):
            assert np.array_equal(gg[k], og[k]), "leaf %g %s: %s" % (leaf, name, k)
        dev = float((np.abs(gg["icov"] - og["icov"]) / scale).max())
        print("DEV build leaf %g %-20s %d voxels; icov %.3g of its scale" % (leaf, name, len(og["idx"]), dev))
        assert dev < 1e-9, name


# ------------------------------------------------------------------ the KDTREE radius
@pytest.mark.parametrize("leaf", lc.LEAVES)
def test_kdtree_radius_on_the_sphere(mods, leaf):
    ndt, po, _ = mods
    t, c, q = lc.sphere_queries(leaf)
    o = oracle_of(po, "KDTREE", t, leaf)
    ref = nc.Grid.of_oracle(o, "KDTREE", t, leaf, lc.MIN_PTS)
    want = ref.terms(q)[1].sum(axis=1)
    assert np.array_equal(want, oracle_counts(o, q)) and 30 < want.sum() < 120
    for voxel_index in (1, 2):
        g = handle(ndt, leaf, voxel_index, t)
        g.setNeighborhoodSearchMethod(po.KDTREE)
        assert np.array_equal(g.gridCentroids()[0][:, :3], c[None, :])
        g.setInputSource(q)
        out, value, found = g.sourcePointNVTL(I4)
        assert np.array_equal(out >= 0, want > 0) and found == want.sum(), "leaf %g index %d" % (leaf, voxel_index)
        assert g.eval(ZERO, False)[3] == want.sum() / len(q)
        counts = []
        for i in range(len(q)):
            g.setInputSource(q[i:i + 1])
            counts.append(g.eval(ZERO, False)[3])
        assert np.array_equal(np.asarray(counts), want), "leaf %g index %d" % (leaf, voxel_index)


# ------------------------------------------------------------------ the exact search at a leaf with slack
def one_query_members(call, q):
    return call([q[i:i + 1] for i in range(len(q))], transforms=[I4] * len(q), max_range=DBL_MAX)


def assert_exact(got, d2, what):
    want = fc.one_point_values(d2)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: %d of %d queries differ, first %d: got %r want %r" % (what, len(bad), len(got), bad[0], got[bad[:3]], want[bad[:3]])


@pytest.mark.parametrize("leaf", lc.LEAVES)
def test_exact_and_centroid_search_per_query(mods, leaf):
    ndt, po, _ = mods
    scenes = [lc.face_scene(leaf, origin) for origin in lc.ORIGINS]
    target = np.concatenate([lc.face_target(leaf)] + [t for t, _ in scenes]).astype(F)
    q = np.concatenate([s for _, s in scenes] + [target, fc.around(target, 600, 71, leaf)]).astype(F)
    d2, _ = fc.nearest_d2(target, q)
    assert (d2[936:936 + len(target)] == 0).all() and np.isfinite(d2).all()
    cloud, _ = cc.centroid_cloud(target, leaf, lc.MIN_PTS)
    c2, _ = fc.nearest_d2(cloud, q)
    assert len(cloud) > 300
    for voxel_index in (0, 1, 2):
        g = handle(ndt, leaf, voxel_index, target)
        assert_exact(one_query_members(g.batchFitness, q), d2, "leaf %g index %d: points" % (leaf, voxel_index))
        assert np.array_equal(g.gridCentroids()[0][:, :3], cloud)
        assert_exact(one_query_members(g.batchCentroidFitness, q), c2, "leaf %g index %d: centroids" % (leaf, voxel_index))
    g = handle(ndt, leaf, 1, halves=halves_of(target))       # an accumulated target keeps no points: the centroid search alone
    assert_exact(one_query_members(g.batchCentroidFitness, q), c2, "leaf %g accumulated: centroids" % leaf)


@pytest.mark.parametrize("leaf", lc.LEAVES)
def test_points_and_centroids_outside_the_cell_they_are_binned_into(mods, leaf):
    """kilometres out the point one ulp below a face is binned above it: only the slack of the cell pruning (index_slack, and
    with it ci.give) finds it -- test_gpu_fitness_edges.py's case at these leaves, and its six-fold form for the centroids"""
    ndt, po, _ = mods
    t, q, gap2 = fc.misbinned_case(leaf)
    d2, arg = fc.nearest_d2(t, q)
    assert (arg % 2 == 0).all() and (d2 < fc.nearest_d2(t[1::2], q)[0]).all()
    target, _, _, cloud = lc.misbinned_voxels(leaf)
    c2, carg = fc.nearest_d2(cloud, q)
    assert (carg % 2 == 1).all() and (c2 < fc.nearest_d2(cloud[0::2], q)[0]).all()
    for voxel_index in (0, 1, 2):
        g = handle(ndt, leaf, voxel_index, t)
        assert_exact(one_query_members(g.batchFitness, q), d2, "misbinned leaf %g index %d: points" % (leaf, voxel_index))
        if voxel_index == 0:
            continue
        for name, g in (("cloud", handle(ndt, leaf, voxel_index, target)), ("accumulated", handle(ndt, leaf, voxel_index, halves=halves_of(target)))):
            assert np.array_equal(g.gridCentroids()[0][:, :3], cloud)
            assert_exact(one_query_members(g.batchCentroidFitness, q), c2, "misbinned leaf %g index %d %s: centroids" % (leaf, voxel_index, name))
            assert g.centroidFitnessDiag()["excursion"] > 0


# ------------------------------------------------------------------ registration
@pytest.mark.parametrize("method", ("DIRECT7", "KDTREE"))
@pytest.mark.parametrize("res", (0.7, 1.5, 3.0))
def test_registration_matches_the_oracles(mods, pair, res, method):
    ndt, po, _ = mods
    t, s = pair
    s = s[:2000]
    g = handle(ndt, res, 0, t)
    g.setNeighborhoodSearchMethod(getattr(po, method))
    g.setInputSource(s)
    g.align()
    T, it = g.getFinalTransformation(), g.getFinalNumIteration()
    runs = {}
    for threads in (1, 8):
        o = po.OracleNDT(resolution=res, num_threads=threads, search_method=getattr(po, method), min_points_per_voxel=lc.MIN_PTS)
        o.set_target(t)
        o.set_source(s)
        runs[threads] = o.align()
    r = runs[8]
    print("ITER res %g %-7s gpu %d oracle %d (1 thread) %d (8 threads); converged %s/%s; rot %.3g trans %.3g"
          % (res, method, it, runs[1]["iterations"], r["iterations"], g.hasConverged(), r["converged"], rot_err(T, r["T"]), trans_err(T, r["T"])))
    assert g.hasConverged() == r["converged"] == runs[1]["converged"]
    assert rot_err(T, r["T"]) < ROT_TOL and trans_err(T, r["T"]) < TRANS_TOL
    if runs[1]["iterations"] == r["iterations"]:       # otherwise the count is no property of the reference to hold
        assert it == r["iterations"]
