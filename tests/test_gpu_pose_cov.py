"""GPU: the pose covariance (k_grad_outer, k_grad_outer_multi; ndt_pose_covariance, ndt_pairs_pose_covariances,
ndt_diag_pose_covariance; map_sequence --covariance, pair_sequence --covariance).

B, g and n_found are held to tests/pose_cov_cases.py -- numpy written from the definition, pinned by
tests/test_pose_cov_cases.py -- n_found exactly, every entry within 1e-11 x S, S the sum of the absolute values of the terms
that were added into that entry as the reference computes it (the bound of the NVTL per-point test: a re-ordered f64 sum with
fused multiply-adds moves by a few eps x S).  A is held to ndt_eval_hessian_f64 BIT FOR BIT where that call sees the same
moved cloud (a transform that is pose_to_matrix of its own pose, exactly: the identity, a pure translation) and to the
reference at 1e-12 of its largest entry elsewhere; cov to ndt_host_pose_covariance of the returned info bit for bit; pairs,
target forms and repeated calls to each other bit for bit."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import centroid_fitness_cases as cc
import eval_plan_sizes as eps
import pose_cov_cases as pc
import pose_cov_child as child
import score_poses_cases as spc
from conftest import ROOT
from test_gpu_centroid_fitness import app_settings
from test_gpu_pairs import build_app

pytestmark = pytest.mark.gpu

F = np.float32
BOUND = 1e-11
N_SOURCE = 2000
METHODS_COV = ("sandwich", "laplace")


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_info(a, b):
    return all(same_bits(a[k], b[k]) for k in ("A", "B", "g", "eig_min", "eig_max")) and a["n_found"] == b["n_found"] and a["indefinite"] == b["indefinite"]


def ratio(got, want, S):
    """worst |got - want| / S over the entries (0 where S is 0 and the entries agree exactly)"""
    got, want, S = (np.asarray(x, dtype=np.float64) for x in (got, want, S))
    d = np.abs(got - want)
    with np.errstate(all="ignore"):
        r = np.where(S > 0, d / S, np.where(d == 0, 0.0, np.inf))
    return float(r.max())


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from oracle import pyoracle as po
    from toyslam_amd import _lib, ndt
    return ndt, po, _lib


class Scene:
    """The bundled pair (the 2 000-point source against the 1.0 m grid) under the four neighbour rules: a GPU handle and the
    numpy reference per rule, the reference's answers computed once per (rule, source, transform)."""

    def __init__(self, mods, pair, golden):
        self.ndt, self.po, self._lib = mods
        self.t, s = pair
        self.s, self.s_full = s[:N_SOURCE], s
        self.T = dict(identity=np.eye(4, dtype=F), golden=spc.golden_T(golden))
        shift = np.eye(4, dtype=F)
        shift[:3, 3] = self.T["golden"][:3, 3]
        self.T["shift"] = shift
        self.handles, self.grids, self.refs = {}, {}, {}

    def handle(self, method):
        if method not in self.handles:
            g = self.ndt.NormalDistributionsTransform()
            g.setNeighborhoodSearchMethod(getattr(self.po, method))
            g.setInputTarget(self.t)
            self.handles[method] = g
        return self.handles[method]

    def grid(self, method):
        if method not in self.grids:
            o = self.po.OracleNDT(num_threads=16, search_method=getattr(self.po, method))
            o.set_target(self.t)
            o.set_source(self.s[:10])
            self.grids[method] = pc.Grid.of_oracle(o, method, self.t)
        return self.grids[method]

    def ref(self, method, n, name):
        if (method, n, name) not in self.refs:
            src, T = self.s[:n], self.T[name]
            self.refs[(method, n, name)] = self.grid(method).information(src, spc.moved(self.po, src, T), self.ndt.host_matrix_to_pose(T))
        return self.refs[(method, n, name)]


@pytest.fixture(scope="module")
def scene(mods, pair, golden):
    return Scene(mods, pair, golden)


def check_sums(I, R, ctx):
    """info of the GPU against the reference's: n_found exactly, B and g within BOUND x S; -> the worst ratio"""
    rB, rg = ratio(I["B"], R["B"], R["S_B"]), ratio(I["g"], R["g"], R["S_g"])
    print("%s: found %d (reference %d)  worst |diff| / S: B %.3g  g %.3g" % (ctx, I["n_found"], R["n_found"], rB, rg))
    assert I["n_found"] == R["n_found"], ctx
    assert rB <= BOUND and rg <= BOUND, ctx
    assert np.array_equal(I["B"], I["B"].T), ctx
    return max(rB, rg)


def check_cov(ndt, g, T, I, ctx):
    """cov of both methods is ndt_host_pose_covariance of the returned info, bit for bit; the info does not depend on the method"""
    for method, scale in (("sandwich", 1.0), ("laplace", 2.5)):
        cov, J = g.poseCovariance(T, method=method, scale=scale, info=True)
        assert same_info(I, J), ctx
        want, lo, hi, flag = ndt.host_pose_covariance(J["A"], J["B"], J["g"], J["n_found"], method, scale)
        assert same_bits(cov, want) and same_bits([lo, hi], [J["eig_min"], J["eig_max"]]) and flag == J["indefinite"], ctx + " " + method
        assert np.isnan(cov).all() == J["indefinite"] and (J["indefinite"] or np.isfinite(cov).all()), ctx


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("method", pc.METHODS)
def test_sums_match_the_reference(scene, method):
    g = scene.handle(method)
    g.setInputSource(scene.s)
    worst = 0.0
    for name in ("identity", "golden"):
        ctx = "%s %s" % (method, name)
        cov, I = g.poseCovariance(scene.T[name], info=True)
        R = scene.ref(method, N_SOURCE, name)
        worst = max(worst, check_sums(I, R, ctx))
        assert R["n_found"] > 1000
        if "NDT_K2_MAX_BLOCKS" not in os.environ:
            assert g.poseCovarianceLaunches() == (1, g.evalPlan(N_SOURCE)["launch_blocks"])
        # A: the reference's, at the bound tests/test_pose_cov_cases.py holds the reference itself to
        rA = float(np.abs(I["A"] - R["A"]).max() / np.abs(R["A"]).max())
        want_cov, lo, hi, flags = pc.covariance(R["A"], R["B"], R["g"], R["n_found"], "sandwich")
        print("%s: A worst |diff| / max|A| %.3g  eigenvalues %.6g .. %.6g  indefinite %d" % (ctx, rA, I["eig_min"], I["eig_max"], I["indefinite"]))
        assert rA <= 1e-12 and np.array_equal(I["A"], I["A"].T), ctx
        assert I["indefinite"] == bool(flags), ctx
        if not flags:
            assert np.linalg.norm(cov - want_cov) <= 1e-8 * np.linalg.norm(want_cov), ctx     # (eps x kappa of A, with margin)
            assert np.all(np.diag(cov) > 0), ctx
        check_cov(scene.ndt, g, scene.T[name], I, ctx)
        again = g.poseCovariance(scene.T[name], info=True)
        assert same_bits(again[0], cov) and same_info(again[1], I), ctx + ": run to run"
    print("%s: worst ratio %.3g of the bound %.3g" % (method, worst, BOUND))


@pytest.mark.parametrize("method", pc.METHODS)
def test_A_is_the_f64_hessians(scene, method):
    """... bit for bit, where ndt_eval_hessian_f64 moves the source by the same matrix"""
    ndt = scene.ndt
    g = scene.handle(method)
    g.setInputSource(scene.s)
    for name in ("identity", "shift"):
        T = scene.T[name]
        p = ndt.host_matrix_to_pose(T)
        assert np.array_equal(ndt.host_pose_to_matrix(p), T), "the fixture: T is pose_to_matrix of its own pose"
        cov, I = g.poseCovariance(T, info=True)
        H = g.hessian_f64(p)
        assert same_bits(I["A"], -(H + H.T) / 2), "%s %s" % (method, name)
        assert np.abs(I["A"]).max() > 0


def test_no_transform_is_the_final_transformation(scene):
    ndt = scene.ndt
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(scene.t)
    g.setInputSource(scene.s)
    before = g.poseCovariance(info=True)                           # before any align: the identity
    at_identity = g.poseCovariance(np.eye(4), info=True)
    assert same_bits(before[0], at_identity[0]) and same_info(before[1], at_identity[1])
    g.align()
    T = g.getFinalTransformation()
    cov, I = g.poseCovariance(info=True)
    explicit = g.poseCovariance(T, info=True)
    assert same_bits(cov, explicit[0]) and same_info(I, explicit[1])
    sigma = np.sqrt(np.diag(cov))
    print("after align: sigma %s  found %d/%d  eigenvalues of A %.6g .. %.6g" % (sigma, I["n_found"], N_SOURCE, I["eig_min"], I["eig_max"]))
    assert not I["indefinite"] and np.all(sigma > 0) and np.all(sigma[:3] < 0.1) and np.all(sigma[3:] < 0.01)
    lap = g.poseCovariance(method="laplace", scale=3.0)
    assert np.linalg.norm(lap - 3.0 * np.linalg.inv(I["A"])) <= 1e-9 * np.linalg.norm(lap)


# ------------------------------------------------------------------ block plan
def plan_sizes(g):
    bounds = eps.boundaries(g.evalPlan, N_SOURCE)
    cuts = eps.sizes_around(bounds, ("launch_two_blocks", "launch_max", "launch_cap", "launch_strided"))
    return sorted(set((1, 255, 256, 257)) | set(n for n in cuts if n <= N_SOURCE))


def test_values_at_the_block_plan_sizes(scene):
    """One point, one block less a lane, exactly, plus a lane, and either side of every cut of the launch plan."""
    sizes = plan_sizes(scene.handle("DIRECT7"))
    print("sizes:", sizes)
    assert {1, 255, 256, 257} <= set(sizes)
    for method in pc.METHODS:
        g = scene.handle(method)
        for n in sizes:
            g.setInputSource(scene.s[:n])
            cov, I = g.poseCovariance(scene.T["golden"], info=True)
            blocks = g.evalPlan(n)["launch_blocks"]
            if "NDT_K2_MAX_BLOCKS" not in os.environ:
                assert blocks == (n + 255) // 256
            assert g.poseCovarianceLaunches() == (1, blocks)
            check_sums(I, scene.ref(method, n, "golden"), "%s n=%d" % (method, n))
            if n == 1:
                assert I["indefinite"] and np.isnan(cov).all()


def unhex(v, shape=None):
    a = np.array([float.fromhex(x) for x in v])
    return a.reshape(shape) if shape else a


def test_values_where_the_walk_is_strided(scene, tmp_path):
    """NDT_K2_MAX_BLOCKS=3: from 769 points a thread walks several points.  Against the reference, and against this process's
    walk (one point per thread) within the same bound."""
    out = tmp_path / "capped.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pose_cov_child.py"), "capped", str(out)],
                       env=dict(os.environ, NDT_K2_MAX_BLOCKS="3"), capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    with open(out) as f:
        res = json.load(f)
    for method in pc.METHODS:
        g = scene.handle(method)
        for n in child.CAPPED_SIZES:
            c = res["%s/%d" % (method, n)]
            assert c["plan_blocks"] == 3 and (c["launches"], c["blocks"]) == (1, 3), (method, n)
            I = dict(B=unhex(c["B"], (6, 6)), g=unhex(c["g"]), n_found=c["n_found"])
            R = scene.ref(method, n, "golden")
            check_sums(I, R, "%s n=%d capped" % (method, n))
            g.setInputSource(scene.s[:n])
            cov, J = g.poseCovariance(scene.T["golden"], info=True)
            assert J["n_found"] == I["n_found"]
            assert ratio(I["B"], J["B"], R["S_B"]) <= BOUND and ratio(I["g"], J["g"], R["S_g"]) <= BOUND, (method, n)
            want = scene.ndt.host_pose_covariance(unhex(c["A"], (6, 6)), I["B"], I["g"], I["n_found"])[0]
            assert same_bits(unhex(c["cov"], (6, 6)), want), (method, n)


# ------------------------------------------------------------------ edges
def test_non_finite_rows_and_points_outside(scene):
    ndt = scene.ndt
    c = spc.spoiled(scene.s)                                      # NaN / +inf / -inf rows and an absurdly far one
    for method in pc.METHODS:
        g = scene.handle(method)
        g.setInputSource(c)
        for name in ("identity", "golden"):
            T = scene.T[name]
            R = scene.grid(method).information(c, spc.moved(scene.po, c, T), ndt.host_matrix_to_pose(T))
            cov, I = g.poseCovariance(T, info=True)
            check_sums(I, R, "%s %s spoiled" % (method, name))
            assert np.isfinite(I["A"]).all() and np.isfinite(I["B"]).all() and I["n_found"] < scene.ref(method, N_SOURCE, name)["n_found"] + 1
            check_cov(ndt, g, T, I, "%s %s spoiled" % (method, name))
        # every point outside the grid: nothing found, the flag, a NaN covariance -- never an error
        far = spc.make_T([1000.0, 0, 0], [0, 0, 0])
        for cov_method in METHODS_COV:
            cov, I = g.poseCovariance(far, method=cov_method, info=True)
            assert I["n_found"] == 0 and I["indefinite"] and np.isnan(cov).all() and cov.shape == (6, 6)
            assert not I["A"].any() and not I["B"].any() and not I["g"].any() and I["eig_min"] == 0.0 == I["eig_max"]
        # only non-finite points
        g.setInputSource(np.full((700, 3), np.nan, F))
        cov, I = g.poseCovariance(np.eye(4), info=True)
        assert I["n_found"] == 0 and I["indefinite"] and np.isnan(cov).all() and not I["B"].any()


def test_a_planar_one_voxel_target(scene):
    """A plane pins z, roll and pitch and hardly x and y: whichever the reference gives for the fixture -- the flag, or in-plane
    translation variances more than 1e3 times the out-of-plane one -- is what the GPU gives."""
    ndt, po = scene.ndt, scene.po
    t, s = pc.planar_fixture()
    for method in pc.METHODS:
        o = po.OracleNDT(num_threads=4, search_method=getattr(po, method))
        o.set_target(t)
        o.set_source(s[:10])
        ref = pc.Grid.of_oracle(o, method, t)
        assert len(ref.idx) == 1
        R = ref.information(s, spc.moved(po, s, np.eye(4, dtype=F)), np.zeros(6))
        want, lo, hi, flags = pc.covariance(R["A"], R["B"], R["g"], R["n_found"], "sandwich")
        g = ndt.NormalDistributionsTransform()
        g.setNeighborhoodSearchMethod(getattr(po, method))
        g.setInputTarget(t)
        g.setInputSource(s)
        cov, I = g.poseCovariance(np.eye(4), info=True)
        check_sums(I, R, "planar " + method)
        print("planar %s: reference flag %d, variances %s" % (method, flags, np.diag(cov)))
        assert I["indefinite"] == bool(flags), method
        if flags:
            assert np.isnan(cov).all(), method
        else:
            for c in (want, cov):
                assert min(c[0, 0], c[1, 1]) > 1e3 * c[2, 2] > 0, method
    assert not flags or method != "DIRECT7"


def test_empty_targets_and_sources(scene):
    ndt = scene.ndt

    def nothing(h, launched):
        for cov_method in METHODS_COV:
            cov, I = h.poseCovariance(scene.T["golden"], method=cov_method, info=True)
            assert I["n_found"] == 0 and I["indefinite"] and np.isnan(cov).all()
            assert not I["A"].any() and not I["B"].any() and not I["g"].any()
        assert (h.poseCovarianceLaunches()[0] > 0) == launched

    # a grid without a valid voxel: 3 points at min_points_per_voxel 6 -- gridded like any other, every probe misses
    h = ndt.NormalDistributionsTransform()
    h.setInputTarget(np.array([[0, 0, 0], [10, 0, 0], [5, 5, 5]], F))
    assert h.grid_counts()["n_valid"] == 0
    h.setInputSource(scene.s[:300])
    nothing(h, True)
    h = ndt.NormalDistributionsTransform()                         # a target of no points
    h.setInputTarget(np.zeros((0, 3), F))
    h.setInputSource(scene.s[:300])
    nothing(h, False)
    h = scene.handle("DIRECT7")                                    # a source of no points
    h.setInputSource(np.zeros((0, 3), F))
    nothing(h, False)
    # no target, then no source
    h = ndt.NormalDistributionsTransform()
    for _ in range(2):
        for call in (h.poseCovariance, h.pairsPoseCovariances):
            with pytest.raises(ndt.NdtError) as e:
                call()
            assert e.value.status == scene._lib.NDT_ERR_NO_INPUT
        h.setInputTarget(scene.t)


def test_every_point_twice_halves_the_sandwich(scene):
    g = scene.handle("DIRECT7")
    T = scene.T["golden"]
    g.setInputSource(scene.s[:1000])
    one, I1 = g.poseCovariance(T, info=True)
    g.setInputSource(np.repeat(scene.s[:1000], 2, axis=0))
    two, I2 = g.poseCovariance(T, info=True)
    assert I2["n_found"] == 2 * I1["n_found"] and not I1["indefinite"]
    for k in ("A", "B", "g"):
        assert np.abs(I2[k] - 2 * I1[k]).max() <= 1e-12 * np.abs(I1[k]).max(), k
    rel = float(np.linalg.norm(two - one / 2) / np.linalg.norm(one))
    print("doubled source: sandwich relative difference from half %.3g" % rel)
    assert rel <= 1e-10


# ------------------------------------------------------------------ target forms
def form_values(g, scene, src):
    out = []
    g.setInputSource(src)
    for method in pc.METHODS:
        g.setNeighborhoodSearchMethod(getattr(scene.po, method))
        for name in ("identity", "golden"):
            for cov_method in METHODS_COV:
                cov, I = g.poseCovariance(scene.T[name], method=cov_method, scale=2.0, info=True)
                out.append((bits(cov).tolist(), bits(I["A"]).tolist(), bits(I["B"]).tolist(), bits(I["g"]).tolist(), I["n_found"], I["indefinite"]))
    return out


def test_sparse_index_and_accumulated_targets_give_the_same_bits(scene):
    ndt = scene.ndt
    src = scene.s

    def cloud_target(points, voxel_index):
        g = ndt.NormalDistributionsTransform()
        g.setVoxelIndex(voxel_index)
        g.setInputTarget(points)
        return g

    dense = form_values(cloud_target(scene.t, 1), scene, src)
    assert all(v[4] > 0 for v in dense)
    assert form_values(cloud_target(scene.t, 2), scene, src) == dense, "the sparse voxel index"
    half = len(scene.t) // 2
    for voxel_index in (1, 2):
        g = ndt.NormalDistributionsTransform()
        g.setVoxelIndex(voxel_index)
        g.targetAccumulate(scene.t[:half])
        g.targetAccumulate(scene.t[half:])
        assert form_values(g, scene, src) == dense, "accumulated, voxel index %d" % voxel_index
        centre = scene.t[:, :3].mean(axis=0)
        lo, hi = centre - [12.0, 9.0, 50.0], centre + [10.0, 14.0, 50.0]
        g.targetAccumulateCrop(lo, hi)
        clo, chi = ndt.crop_cell_range(1.0, lo, hi)
        cells = cc.cells_of(scene.t, 1.0)
        kept = scene.t[((cells >= clo) & (cells <= chi)).all(axis=1)]
        assert 1000 < len(kept) < len(scene.t) - 1000
        cropped = form_values(g, scene, src)
        assert cropped != dense
        assert cropped == form_values(cloud_target(kept, voxel_index), scene, src), "cropped, voxel index %d" % voxel_index


# ------------------------------------------------------------------ pairs
def test_pairs_are_fresh_handles(scene):
    """three pairs, one shared target, sources of 1, 257 and 2 000 points: every member is the handle that holds that pair"""
    ndt = scene.ndt
    clouds = [scene.t, scene.s[:1], scene.s[:257], scene.s]
    pairs = [(0, 1), (0, 2), (0, 3)]
    for method in ("DIRECT7", "KDTREE"):
        g = ndt.NormalDistributionsTransform()
        g.setNeighborhoodSearchMethod(getattr(scene.po, method))
        r = g.alignPairs(clouds, pairs)
        tables = (None, [scene.T["golden"], scene.T["identity"], scene.T["golden"]])
        for transforms in tables:
            for cov_method, scale in (("sandwich", 1.0), ("laplace", 0.5)):
                cov, infos = g.pairsPoseCovariances(transforms, method=cov_method, scale=scale, info=True)
                assert cov.shape == (3, 6, 6) and len(infos) == 3
                if "NDT_K2_MAX_BLOCKS" not in os.environ:
                    assert g.poseCovarianceLaunches() == (1, 1 + 2 + 8)
                for k, (_, c) in enumerate(pairs):
                    ctx = "%s pair %d %s %s" % (method, k, cov_method, "given" if transforms else "final")
                    T = r["T"][k] if transforms is None else transforms[k]
                    h = ndt.NormalDistributionsTransform()
                    h.setNeighborhoodSearchMethod(getattr(scene.po, method))
                    h.setInputTarget(scene.t)
                    h.setInputSource(clouds[c])
                    want, J = h.poseCovariance(T, method=cov_method, scale=scale, info=True)
                    assert same_info(infos[k], J), ctx
                    assert same_bits(cov[k], want), ctx
                    if transforms is not None and k == 2 and method == "DIRECT7":
                        check_sums(infos[k], scene.ref(method, N_SOURCE, "golden"), ctx)
                        assert not J["indefinite"]
                assert infos[0]["indefinite"] and np.isnan(cov[0]).all()          # one point
        assert same_bits(g.pairsPoseCovariances(), g.pairsPoseCovariances([r["T"][k] for k in range(3)]))
        # ... and when every pair has a target of its own
        own = [scene.t, scene.s, scene.t[::2], scene.s_full]
        own_pairs = [(2, 1), (3, 1), (0, 1)]
        g.alignPairs(own, own_pairs)
        given = [scene.T["golden"], scene.T["identity"], scene.T["shift"]]
        cov, infos = g.pairsPoseCovariances(given, info=True)
        for k, (tc, sc) in enumerate(own_pairs):
            h = ndt.NormalDistributionsTransform()
            h.setNeighborhoodSearchMethod(getattr(scene.po, method))
            h.setInputTarget(own[tc])
            h.setInputSource(own[sc])
            want, J = h.poseCovariance(given[k], info=True)
            assert same_info(infos[k], J) and same_bits(cov[k], want), "%s own target, pair %d" % (method, k)
            assert J["n_found"] > 1000
        assert not same_bits(infos[0]["A"], infos[2]["A"])
        with pytest.raises(ValueError):
            g.pairsPoseCovariances([np.eye(4)])
        # after a failed pairs call there are no pairs
        with pytest.raises(ndt.NdtError):
            g.alignPairs(clouds, [(0, 9)])
        with pytest.raises(ndt.NdtError) as e:
            g.pairsPoseCovariances()
        assert e.value.status == scene._lib.NDT_ERR_NO_INPUT
        g.alignPairs(clouds, [])
        with pytest.raises(ndt.NdtError) as e:
            g.pairsPoseCovariances()
        assert e.value.status == scene._lib.NDT_ERR_NO_INPUT


def test_a_pair_with_an_empty_target_or_source(scene):
    ndt = scene.ndt
    g = ndt.NormalDistributionsTransform()
    few = np.array([[0, 0, 0], [10, 0, 0], [5, 5, 5]], F)
    g.alignPairs([scene.t, scene.s[:300], few, np.zeros((0, 3), F)], [(2, 1), (0, 3), (0, 1)])
    cov, infos = g.pairsPoseCovariances([np.eye(4)] * 3, info=True)
    for k in (0, 1):
        assert infos[k]["n_found"] == 0 and infos[k]["indefinite"] and np.isnan(cov[k]).all() and not infos[k]["B"].any()
    h = ndt.NormalDistributionsTransform()
    h.setInputTarget(scene.t)
    h.setInputSource(scene.s[:300])
    want, J = h.poseCovariance(np.eye(4), info=True)
    assert same_info(infos[2], J) and same_bits(cov[2], want) and J["n_found"] > 100


# ------------------------------------------------------------------ state
def result_bits(g):
    T, conv, it, tp = g._result()
    return T.tobytes(), conv, it, float(tp).hex(), tuple(sorted(g.stats().items())), g.scorePosesLaunches(), g.nvtlLaunches()


def test_the_handles_state_is_untouched(scene):
    ndt = scene.ndt
    P = [scene.T["golden"], scene.T["identity"]]

    def prepared():
        g = ndt.NormalDistributionsTransform()
        g.setInputTarget(scene.t)
        g.setInputSource(scene.s)
        g.align()
        g.scorePoses(P)
        g.nvtlPoses(P)
        g.alignPairs([scene.t, scene.s[:500]], [(0, 1)])
        return g

    g, never = prepared(), prepared()
    state = result_bits(g)
    assert state[1] and state[2] > 0 and state[5][0] == 1 and state[6][0] == 1
    assert result_bits(never)[:4] == state[:4]
    grid_before = g.grid_counts()
    for call in (g.poseCovariance, lambda: g.poseCovariance(P[0], method="laplace", scale=2.0, info=True), g.pairsPoseCovariances,
                 lambda: g.pairsPoseCovariances([P[0]], info=True), g.poseCovarianceLaunches):
        call()
        assert result_bits(g) == state and g.grid_counts() == grid_before
    assert same_bits(g.pairsFitness(), never.pairsFitness())
    # a following align is the one of a handle that never made the call
    g.align()
    never.align()
    assert result_bits(g)[:4] == result_bits(never)[:4]
    assert same_bits(g.getNVTL()[0:1], never.getNVTL()[0:1])


# ------------------------------------------------------------------ the apps
def four_scans(ndt, reference_pcd, tmp_path):
    """four scans cut from the bundled pair: the even and the odd points of the target, then of the source"""
    d = tmp_path / "pcd"
    d.mkdir()
    scans = []
    for path in reference_pcd:
        xyz, _ = ndt.pcd_read_xyz(path)
        scans += [xyz[0::2], xyz[1::2]]
    for k, sc in enumerate(scans, 1):
        ndt.pcd_write_xyz(str(d / ("cloud_%d.pcd" % k)), np.ascontiguousarray(sc))
    return scans, d


def sigmas(out, pattern):
    rows = []
    for ln in out.splitlines():
        m = re.fullmatch(pattern, ln)
        if m:
            rows.append([float(x) for x in m.group(1).split()])
    return np.array(rows)


def test_map_sequence_prints_the_pose_sigmas(scene, reference_pcd, tmp_path):
    ndt = scene.ndt
    scans, d = four_scans(ndt, reference_pcd, tmp_path)
    exe = build_app(tmp_path, "map_sequence")
    plain = subprocess.check_output([exe, "--scan-to-map", str(d)], text=True)
    flagged = subprocess.check_output([exe, "--scan-to-map", "--covariance", str(d)], text=True)
    got = sigmas(flagged, r"pose sigma: (.+)")
    assert got.shape == (3, 6) and "registrations 3" in flagged and "pose sigma" not in plain
    timed = lambda ln: ln.startswith("time:") or ln.startswith("start-up") or " ms" in ln
    assert [ln for ln in plain.splitlines() if not timed(ln)] == [ln for ln in flagged.splitlines() if not timed(ln) and not ln.startswith("pose sigma: ")]
    assert subprocess.run([exe, "--covariance", str(d)], capture_output=True).returncode == 2      # goes with --scan-to-map
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
        want.append(np.sqrt(np.diag(g.poseCovariance())))
        if g.hasConverged():
            prev = g.getFinalTransformation().astype(F)
            g.targetAccumulateCloud(dc, prev)
    want = np.array(want)
    print("map_sequence sigmas:\n%s\npython:\n%s" % (got, want))
    assert np.isfinite(want).all() and np.all(want > 0)
    assert np.allclose(got, want, rtol=1e-5, atol=0)


def test_pair_sequence_prints_the_pair_sigmas(scene, reference_pcd, tmp_path):
    ndt = scene.ndt
    scans, d = four_scans(ndt, reference_pcd, tmp_path)
    exe = build_app(tmp_path, "pair_sequence")
    plain = subprocess.check_output([exe, str(d)], text=True)
    flagged = subprocess.check_output([exe, str(d), "--covariance"], text=True)
    got = sigmas(flagged, r"pair \d+ sigma: (.+)")
    assert got.shape == (3, 6) and "pairs 3" in flagged and "sigma" not in plain
    assert [ln for ln in flagged.splitlines() if ln.startswith("pair ")] == ["pair %d sigma: %s" % (k, " ".join("%.9g" % x for x in got[k])) for k in range(3)]
    assert subprocess.run([exe, str(d), "--covariance", "--gicp"], capture_output=True).returncode == 2
    g = ndt.NormalDistributionsTransform()
    app_settings(g)
    clouds = [g.voxelGridFilterCloud(sc, 0.5)[0] for sc in scans]
    g.alignPairs(clouds)
    cov, infos = g.pairsPoseCovariances(info=True)
    want = np.sqrt(np.array([np.diag(c) for c in cov]))
    print("pair_sequence sigmas:\n%s\npython:\n%s" % (got, want))
    for k, I in enumerate(infos):   # (a scan filtered at 0.5 m leaves few voxels of 6 points: a pair may well be flagged)
        print("pair %d: found %d  eigenvalues of A %.6g .. %.6g  indefinite %d" % (k, I["n_found"], I["eig_min"], I["eig_max"], I["indefinite"]))
        assert np.isnan(want[k]).all() == I["indefinite"] and (I["indefinite"] or np.all(want[k] > 0))
    assert not infos[0]["indefinite"]
    assert np.allclose(got, want, rtol=1e-5, atol=0, equal_nan=True)
