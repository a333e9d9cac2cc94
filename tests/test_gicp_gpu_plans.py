"""GPU: the four GICP kernels (k_knn_covariances, k_correspond, k_functor, k_gicp_server) AT THE BOUNDARIES OF THEIR BLOCK
PLANS, against the CPU oracle.

Each kernel cuts its work in its own way (8 query teams per 64-lane block; 32 queries per block with a wave-uniform loop;
256 points per block with a last-block fixed-order sum; 256 points per block dealt to 8 shard counters), and a dropped tail
lane, a query served twice by the strided loop or a shard whose ticket count is off by one shows only where a cloud's size
sits ON such a cut.  The sizes are found by asking the library for its plan (plan = gicp_diag_plan; the chooser is
tests/gicp_plan_sizes.py and has a CPU test of its own) and every boundary case first asserts that it sits where it claims.
What is EXPECTED never comes from the plan or from another GPU path: it is the oracle's answer (oracle.pyoracle), so the
file also holds under the switch that moves the boundaries (NDT_GICP_MAX_BLOCKS) and on either objective path
(NDT_GICP_SERVER=0, NDT_GICP_NO_FUSE=1).

Largest deviations from the oracle are gathered in DEV, the boundaries found in BOUNDS; both are printed when the module is
done (and written as JSON to $GICP_PLAN_REPORT if that is set); NOTES.md quotes them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gicp_plan_sizes as gps
from conftest import ROOT, rot_err, trans_err
from oracle import pyoracle as po
from test_gicp_gpu import ROT_TOL, TRANS_TOL, gmod  # noqa: F401  (gmod: the fixture)
from toyslam_amd import clouds

pytestmark = pytest.mark.gpu

HI = 600000                   # largest size the plan is asked about (both objective grids are capped well below)
# Objective / gradient against the oracle: the figures of test_gicp_gpu.test_functor_sums (f relative, g of the largest
# component), asserted unchanged at every size, the caps included -- what was measured there lies a factor of 40 and more
# below them (NOTES.md, "GICP kernels at their block-plan boundaries").
F_TOL, G_TOL = 1e-12, 1e-11
DEV, BOUNDS = {}, {}
ON_SERVER = os.environ.get("NDT_GICP_SERVER", "1") != "0"   # which kernel answers step_functor in this process
OBJECTIVE = "k_gicp_server" if ON_SERVER else "k_functor"


def note(kernel, what, value):
    k = kernel + "/" + what
    DEV[k] = max(DEV.get(k, 0.0), float(value))


def found(kernel, what, value):
    BOUNDS[kernel + "/" + what] = value


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    text = json.dumps({"boundaries": BOUNDS, "largest_deviation_from_oracle": DEV}, indent=1, sort_keys=True)
    print("\nGICP kernels at their plan boundaries (objective path: %s):\n%s" % (OBJECTIVE, text))
    if os.environ.get("GICP_PLAN_REPORT"):
        with open(os.environ["GICP_PLAN_REPORT"], "w") as f:
            f.write(text + "\n")


@pytest.fixture(scope="module")
def plan(gmod):
    g = gmod.GeneralizedIterativeClosestPoint()
    cache = {}

    def ask(n):
        if n not in cache:
            cache[n] = g.plan(n)
        return cache[n]
    return ask


def spd(rng, n):
    """Random symmetric positive definite covariances (as test_caller_supplied_covariances)."""
    a = rng.normal(0, 1, (n, 3, 3))
    return (a @ a.transpose(0, 2, 1)) * 0.01 + 1e-3 * np.eye(3)


def cube(n, seed, half=3.0, offset=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-half, half, (n, 3)) + np.asarray(offset)).astype(np.float32)


def largest_boundary(plan, field, hi=20000):
    """(blocks, b): the largest block count of gps.BLOCK_COUNTS whose first size the plan reports below hi, asserted to be a
    boundary.  (Under NDT_GICP_MAX_BLOCKS=3 that is the second block.)"""
    bs = gps.block_boundaries(plan, field, hi)
    blocks = max(bs)
    b = bs[blocks]
    assert blocks > 1 and plan(b - 1)[field] != plan(b)[field] and plan(b)[field] == blocks
    return blocks, b


# ------------------------------------------------------------------ k_knn_covariances
def check_neighbours(g, cloud, k, cov_tol, ctx, which=0):
    """g.covariances(which, neighbors=True) of `cloud` against the oracle: indices and f32 distances identical; covariances
    within cov_tol, or not compared at all where cov_tol is None (degenerate shapes, k < 5: the eigenvectors of a
    rank-deficient covariance are not a function of the input)."""
    g.setCorrespondenceRandomness(k)
    (g.setInputTarget if which == 0 else g.setInputSource)(cloud)
    cov, idx, d2 = g.covariances(which, neighbors=True)
    oi, od = po.gicp_knn(cloud, cloud, k)
    assert np.array_equal(idx, oi), ctx
    assert np.array_equal(d2, od), ctx
    if cov_tol is not None:
        dev = float(np.abs(cov - po.gicp_covariances(cloud, k, 1e-3)).max())
        print("%s: covariances max abs deviation %.3g" % (ctx, dev))
        note("k_knn_covariances", "cov_abs" if cov_tol < 1e-10 else "cov_abs_duplicates", dev)
        assert dev < cov_tol, ctx
        assert np.array_equal(cov, cov.transpose(0, 2, 1)), ctx


@pytest.mark.parametrize("k", [1, 2, 5, 20, 63, 64])
def test_neighbours_of_clouds_barely_larger_than_k(gmod, k):
    """n = k (every query's answer is the whole cloud: the shell walk can only end through r >= r_lim or the wave-wide
    two-pass scan), k + 1, and k + 7, k + 8, k + 9 (a partly filled last block of 8 query teams, a full one, one query
    more); k = 1 also on a cloud of a single point.  k in {1, 2}: neighbours and distances only."""
    g = gmod.GeneralizedIterativeClosestPoint()
    sizes = [k, k + 1, k + 7, k + 8, k + 9] + ([1] if k == 1 else [])
    for n in sorted(set(sizes)):
        check_neighbours(g, cube(n, 100 * k + n), k, 1e-12 if k >= 5 else None, "k=%d n=%d" % (k, n))


def test_neighbours_at_a_grid_boundary_and_at_an_odd_size(gmod, plan):
    """k = 5 where the kNN grid takes its next block (b - 1, b, b + 1, b from the plan) and k = 20 on 1003 points."""
    g = gmod.GeneralizedIterativeClosestPoint()
    blocks, b = largest_boundary(plan, "knn_blocks")
    found("k_knn_covariances", "first_size_with_%d_blocks" % blocks, b)
    for n in (b - 1, b, b + 1):
        check_neighbours(g, cube(n, 7 + n), 5, 1e-12, "k=5 n=%d (%d blocks from %d on)" % (n, blocks, b))
    check_neighbours(g, cube(1003, 8), 20, 1e-12, "k=20 n=1003")


@pytest.mark.parametrize("shape", ["plane", "line", "identical", "clusters", "offset", "cube", "duplicates"])
def test_neighbours_on_shapes(gmod, shape):
    """About 2 000 points, k = 20.  Degenerate shapes (a plane z = const, a straight line, 100 identical points -- ties
    decided by index alone): neighbours and distances only.  Generic ones (two clusters 500 m apart plus three isolated
    points, a cloud offset by (1000, -2000, 50) m -- the slack of the shell bound --, a uniform cube): covariances too, at
    1e-12.  Duplicated points: the 1e-9 of test_duplicate_points_and_sparse_outliers."""
    rng = np.random.default_rng(21)
    n, tol = 2000, 1e-12
    if shape == "plane":
        c, tol = np.c_[rng.uniform(-20, 20, (n, 2)), np.full(n, 1.5)], None
    elif shape == "line":
        t = rng.uniform(-30, 30, n)
        c, tol = np.c_[0.6 * t + 1.0, -0.3 * t, 0.74 * t + 2.0], None
    elif shape == "identical":
        c, tol = np.tile(np.array([[1.25, -3.5, 0.75]]), (100, 1)), None
    elif shape == "clusters":
        c = np.concatenate([rng.uniform(-3, 3, (1000, 3)), rng.uniform(-3, 3, (997, 3)) + [500.0, 0, 0],
                            [[250.0, 40.0, 0.0], [0.0, -350.0, 20.0], [700.0, 90.0, 90.0]]])
    elif shape == "offset":
        c = rng.uniform(-10, 10, (n, 3)) + [1000.0, -2000.0, 50.0]
    elif shape == "cube":
        c = rng.uniform(-5, 5, (n, 3))
    else:
        base = rng.uniform(-3, 3, (1500, 3))
        c, tol = np.concatenate([base, base[:300], base[:100], base[:100]]), 1e-9
    check_neighbours(gmod.GeneralizedIterativeClosestPoint(), c.astype(np.float32), 20, tol, shape)


def test_neighbours_over_an_index_built_by_the_bucket_chain(gmod):
    """60 000 generic points, k = 20: above the 49 152 points up to which the index is built by the one-launch form, so the
    search runs over an index from the bucket chain.  (The handle has no way to say which form built its index: the size
    alone selects it.)"""
    rng = np.random.default_rng(22)
    c = rng.uniform(-20, 20, (60000, 3)).astype(np.float32)
    check_neighbours(gmod.GeneralizedIterativeClosestPoint(), c, 20, 1e-12, "chain n=60000")


def test_neighbours_after_the_leaf_hint_of_another_density(gmod):
    """gicp_build_index starts from the leaf the previous cloud of about this size ended up with: one handle, a target of
    n points, then the same n over an extent 50 times larger, then over one 50 times smaller than the first -- each with
    the oracle's neighbours exactly (the leaf only costs time, never results).  Target and source slot alike."""
    n = 3000
    base = cube(n, 23).astype(np.float64)
    for which in (0, 1):
        g = gmod.GeneralizedIterativeClosestPoint()
        for scale in (1.0, 50.0, 1.0 / 50.0):
            check_neighbours(g, (base * scale).astype(np.float32), 20, 1e-12, "leaf hint which=%d scale=%g" % (which, scale), which)


# ------------------------------------------------------------------ k_correspond
GUESS = clouds.make_T([0.2, -0.1, 0.05], np.radians([0.3, -0.2, 0.6])).astype(np.float32)
CUR = clouds.make_T([0.05, -0.05, 0.02], np.radians([0.1, 0.0, 0.2])).astype(np.float32)
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def scene():
    """The suite's 20 000-point target, a pool of source points near it, and fixed-seed covariances for both (supplied by
    the caller on both sides: the kNN pass is not what is under test in the correspondence and functor checks)."""
    tgt = clouds.target_surfaces(20000)[:, :3].astype(np.float32)
    src = clouds.source_from_target(tgt, 8000)[:, :3].astype(np.float32)
    rng = np.random.default_rng(5)
    return tgt, src, spd(rng, len(tgt)), spd(rng, len(src))


class Pairing:
    """A GPU handle and an oracle on the same target with the same supplied covariances and gate."""

    def __init__(self, gmod, tgt, ct, gate, **kw):
        self.g = gmod.GeneralizedIterativeClosestPoint()
        self.o = po.OracleGICP(corr_dist_threshold=gate, **kw)
        self.g.setMaxCorrespondenceDistance(gate)
        if "max_iterations" in kw:
            self.g.setMaximumIterations(kw["max_iterations"])
        if "max_inner_iterations" in kw:
            self.g.setMaximumOptimizerIterations(kw["max_inner_iterations"])
        if "rotation_epsilon" in kw:
            self.g.setRotationEpsilon(kw["rotation_epsilon"])
        if "transformation_epsilon" in kw:
            self.g.setTransformationEpsilon(kw["transformation_epsilon"])
        for x in (self.g, self.o):
            x.setInputTarget(tgt)
            x.setTargetCovariances(ct)

    def source(self, src, cs):
        for x in (self.g, self.o):
            x.setInputSource(src)
            x.setSourceCovariances(cs)

    def correspond(self, guess, cur, ctx):
        """One correspondence step on both sides: count and indices identical, Mahalanobis matrices of the matched points
        within 1e-6 of the largest entry.  -> (count, indices, the oracle's matrices)"""
        self.o.prepare(guess)
        m_o, idx_o, maha_o = self.o.correspond(cur)
        m_g, idx_g, maha_g = self.g.step_correspond(guess, cur)
        assert m_g == m_o, ctx
        assert np.array_equal(idx_g, idx_o), ctx
        assert m_o == int((idx_o >= 0).sum())
        v = idx_o >= 0
        if v.any():
            dev = float(np.abs(maha_o[v] - maha_g[v]).max() / np.abs(maha_o[v]).max())
            note("k_correspond", "maha_rel", dev)
            assert dev <= 1e-6, ctx
        return m_o, idx_o, maha_o


CORRESPOND_SIZES = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257)
GATES = (5.0, 0.15, 1e6, 1e-6)


@pytest.mark.parametrize("n_target", [1, 2, 20000])
def test_correspond_at_team_wave_and_block_edges(gmod, plan, scene, n_target):
    """Sources of 1 ... 257 points (the 8-lane team, the 8-team wave, the 32-query block and their neighbours) and one grid
    boundary +- 1 from the plan, against targets of 1, 2 and 20 000 points, under four gates: 5 m, 0.15 m, 1e6 m (the early
    gate exit never fires) and 1e-6 m (nothing corresponds: the count is 0 and every index is -1).  (The one-point target is
    the slow case, on the CPU side: the oracle's cell grid over a single point has cells of a millimetre, and every query walks
    its 24 shells of them before it looks at the point.)"""
    tgt, src, ct, cs = scene
    blocks, b = largest_boundary(plan, "correspond_blocks")
    found("k_correspond", "first_size_with_%d_blocks" % blocks, b)
    sizes = sorted(set(CORRESPOND_SIZES) | {b - 1, b, b + 1})
    for gate in GATES:
        p = Pairing(gmod, tgt[:n_target], ct[:n_target], gate)
        some = 0
        for n in sizes:
            p.source(src[:n], cs[:n])
            m, idx, _ = p.correspond(GUESS, CUR, "n=%d target=%d gate=%g" % (n, n_target, gate))
            some += m
            if gate == 1e-6:
                assert m == 0 and np.all(idx == -1)
            if gate == 1e6:
                assert m == n
        if n_target == 20000 and gate == 0.15:
            assert 0 < some < sum(sizes)    # the gate really decides


def test_correspond_with_every_query_outside_the_targets_box(gmod):
    """The source shifted wholly outside the target's bounding box (the margin = 0, clamped-cell branch of query_cell): by
    3 m it still corresponds under the 5 m gate; by 30 m nothing does under 5 m and everything does under 1e6 m, through the
    fallback scan."""
    rng = np.random.default_rng(31)
    tgt = rng.uniform(-10, 10, (20000, 3)).astype(np.float32)
    ct, n = spd(rng, len(tgt)), 300
    cs = spd(rng, n)
    for shift, gate, want in ((3.0, 5.0, n), (30.0, 5.0, 0), (30.0, 1e6, n)):
        src = rng.uniform(-7, 7, (n, 3))
        src[:, 0] = tgt[:, 0].max() + shift + rng.uniform(0.01, 0.5, n)
        src = src.astype(np.float32)
        assert np.all(src[:, 0] >= tgt[:, 0].max() + np.float32(shift))
        p = Pairing(gmod, tgt, ct, gate)
        p.source(src, cs)
        m, _, _ = p.correspond(EYE, EYE, "outside by %g m, gate %g" % (shift, gate))
        assert m == want, (shift, gate, m)


@pytest.mark.parametrize("far", [64, 59])
def test_correspond_one_far_point_in_the_last_wave(gmod, scene, far):
    """65 source points of which exactly one is 400 m away: with the 1e6 m gate its team takes wave_nearest while its
    neighbours idle (point 64: alone in the last wave) or are done (point 59); with the 5 m gate it has no correspondence
    and the others keep theirs."""
    tgt, src, ct, cs = scene
    s = src[:65].copy()
    s[far] += np.float32(400.0)
    for gate in (1e6, 5.0):
        p = Pairing(gmod, tgt, ct, gate)
        p.source(s, cs[:65])
        m, idx, _ = p.correspond(EYE, EYE, "far point %d gate %g" % (far, gate))
        assert m == (65 if gate == 1e6 else 64) and (idx[far] >= 0) == (gate == 1e6)


def test_correspond_target_with_every_point_twice(gmod, scene):
    """Equal distances everywhere: the lower index wins each tie, on the shell walk and on the fallback scan."""
    tgt, src, ct, cs = scene
    half = tgt[::4]
    t2, c2 = np.concatenate([half, half]), np.concatenate([ct[:5000], ct[5000:10000]])   # (the twins differ in covariance)
    s = src[:257].copy()
    s[100] += np.float32(400.0)
    for gate in (5.0, 1e6):
        p = Pairing(gmod, t2, c2, gate)
        p.source(s, cs[:257])
        m, idx, _ = p.correspond(GUESS, CUR, "doubled target gate %g" % gate)
        assert m > 200 and np.all(idx < 5000)


# ------------------------------------------------------------------ k_functor / k_gicp_server
STATES = (np.zeros(6), np.array([0.05, -0.02, 0.01, 0.003, -0.002, 0.01]), np.array([-0.21, 0.13, 0.08, -0.02, 0.015, -0.027]))


class FunctorRig:
    """Target of 3 000 points; a pool of source points, point i about 1 cm from target point i mod 3 000; covariances
    supplied for both clouds -- the oracle's share of a size is one exact 1-NN pass and a sum."""

    def __init__(self, gmod, plan):
        self.gmod, self.plan = gmod, plan
        rng = np.random.default_rng(41)
        self.tgt = clouds.target_surfaces(3000)[:, :3].astype(np.float32)
        self.ct = spd(rng, len(self.tgt))
        self.pool = (self.tgt[np.arange(HI) % len(self.tgt)] + rng.normal(0, 0.006, (HI, 3))).astype(np.float32)
        self.cs = spd(rng, HI)
        self.pairings = {}

    def pairing(self, gate):
        if gate not in self.pairings:
            self.pairings[gate] = Pairing(self.gmod, self.tgt, self.ct, gate)
        return self.pairings[gate]

    def per_block(self, field):
        """Points one block of the grid covers in one pass: the size before the second block appears (from the plan)."""
        b2 = gps.first_reaching(self.plan, field, 2, HI)
        assert b2 is not None and self.plan(b2 - 1)[field] == 1
        return b2 - 1

    def heavy_tailed(self, n):
        """pool[:n] with the first and the last point of the objective kernel's last block, and the very last point,
        displaced by 1 m (they still correspond under the 5 m gate).  -> (cloud, indices of the displaced points)"""
        field = "server_blocks" if ON_SERVER else "functor_blocks"
        pb, blocks = self.per_block(field), self.plan(n)[field]
        first = min((blocks - 1) * pb, n - 1)
        tails = sorted({first, min(blocks * pb, n) - 1, n - 1})
        c = self.pool[:n].copy()
        c[tails] += np.array([0.6, -0.64, 0.48], np.float32)   # 1 m
        return c, tails

    def check(self, cloud, tails, gate, size_class, ctx):
        """Correspondences, then the objective in modes 0, 1, 2 at three states against the oracle; every displaced point
        must carry a share of f that the tolerance cannot hide (ten times F_TOL at least)."""
        n = len(cloud)
        p = self.pairing(gate)
        p.source(cloud, self.cs[:n])
        m, idx, maha = p.correspond(EYE, EYE, ctx)
        worst_f = worst_g = 0.0
        for x in STATES:
            for mode in (0, 1, 2):
                fo, go = p.o.functor(mode, x)
                fg, gg = p.g.step_functor(mode, x)
                if mode != 1:
                    worst_f = max(worst_f, abs(fo - fg) / abs(fo))
                    assert abs(fo - fg) <= F_TOL * abs(fo), (ctx, mode, fo, fg)
                if mode != 0:
                    worst_g = max(worst_g, float(np.abs(go - gg).max() / np.abs(go).max()))
                    assert np.abs(go - gg).max() <= G_TOL * np.abs(go).max(), (ctx, mode)
        print("%s (%s, %d correspondences): f rel %.3g  g rel %.3g" % (ctx, OBJECTIVE, m, worst_f, worst_g))
        note(OBJECTIVE, size_class + "/f_rel", worst_f)
        note(OBJECTIVE, size_class + "/g_rel", worst_g)
        if tails:   # the share of each displaced point in f at x = 0, from the oracle's correspondences and matrices
            f0, _ = p.o.functor(2, STATES[0])
            for i in tails:
                assert idx[i] >= 0, (ctx, i)
                r = cloud[i].astype(np.float64) - self.tgt[idx[i]].astype(np.float64)
                share = float(r @ maha[i].reshape(3, 3).astype(np.float64) @ r) / (f0 * m)
                assert 10 * F_TOL < share, (ctx, i, share)
                DEV["heavy_tail/smallest_share_of_f"] = min(DEV.get("heavy_tail/smallest_share_of_f", 1.0), share)
        return m, idx


@pytest.fixture(scope="module")
def rig(gmod, plan):
    return FunctorRig(gmod, plan)


def sweep_sizes(plan):
    """Source sizes of the functor sweep and, for the report, the boundaries they come from."""
    for field, kernel in (("functor_blocks", "k_functor"), ("server_blocks", "k_gicp_server")):
        for blocks, b in gps.block_boundaries(plan, field, HI).items():
            assert gps.is_boundary(plan, field, b) and plan(b)[field] == blocks
            found(kernel, "first_size_with_%d_blocks" % blocks, b)
    return gps.functor_sweep_sizes(plan, HI)


def test_functor_sums_where_the_grids_take_their_next_block(rig, plan):
    """Source sizes at which the functor kernel's and the server's grid first have 1, 2, 7, 8, 9, 16 and 17 blocks, and the
    sizes either side: the grids of 1 ... 9 blocks are where the server's in_shard and the host's n_parts must agree."""
    sizes = sweep_sizes(plan)
    if "NDT_GICP_MAX_BLOCKS" not in os.environ:
        for kernel in ("k_functor", "k_gicp_server"):
            assert all(kernel + "/first_size_with_%d_blocks" % c in BOUNDS for c in gps.BLOCK_COUNTS), BOUNDS
    for n in sizes:
        cloud, tails = rig.heavy_tailed(n)
        rig.check(cloud, tails, 5.0, "block_counts", "n=%d" % n)


@pytest.mark.parametrize("field", ["server_blocks", "functor_blocks"])
def test_functor_sums_at_the_grid_caps(rig, plan, field):
    """Where the server's and the functor kernel's grid stop growing (about 131 k and 262 k source points): the boundary
    +- 1, then one period beyond it, where the capped grid's threads first walk a second point.  The target stays at 3 000
    points: the oracle's share of a size is a fraction of a second."""
    cap = gps.cap_boundary(plan, field, HI)
    assert cap is not None, "the plan has no cap below %d" % HI
    b, period = cap
    assert plan(b - 1)[field] != plan(b)[field] == plan(HI)[field] == plan(b + period + 1)[field]
    found("k_gicp_server" if field == "server_blocks" else "k_functor", "cap", {"first_size": b, "blocks": plan(b)[field], "period": period})
    for n in gps.cap_sizes(plan, field, HI):
        cloud, tails = rig.heavy_tailed(n)
        rig.check(cloud, tails, 5.0, field.split("_")[0] + "_cap", "n=%d (%s cap at %d)" % (n, field, b))


def test_functor_sums_with_sparse_correspondences(rig, plan):
    """A 9-block source of which one whole block (the fourth) lies 500 m away and has no correspondence under the 5 m gate:
    its row of partial sums is all zeros and still has to be counted by its shard; then a source with exactly one
    correspondence in total.  (Where NDT_GICP_MAX_BLOCKS leaves fewer than 9 blocks: the largest grid there is.)"""
    field = "server_blocks" if ON_SERVER else "functor_blocks"
    blocks = min(9, plan(HI)[field])
    assert blocks >= 3 and (blocks == 9 or "NDT_GICP_MAX_BLOCKS" in os.environ)
    n = gps.first_reaching(plan, field, blocks, HI)
    assert plan(n)[field] == blocks and plan(n - 1)[field] == blocks - 1
    pb, victim = rig.per_block(field), min(3, blocks - 2)
    cloud, tails = rig.heavy_tailed(n)
    cloud[victim * pb:(victim + 1) * pb] += np.float32(500.0)
    m, idx = rig.check(cloud, tails, 5.0, "sparse", "n=%d, block %d without correspondences" % (n, victim))
    assert np.all(idx[victim * pb:(victim + 1) * pb] == -1) and m == n - pb
    cloud = rig.pool[:n] + np.float32(500.0)
    cloud[n - 2] = rig.pool[n - 2]
    m, idx = rig.check(cloud, [], 5.0, "sparse", "n=%d, one correspondence" % n)
    assert m == 1 and idx[n - 2] >= 0


# ------------------------------------------------------------------ iteration-limited registrations
def check_limited_registrations(rig, sizes, label):
    """align with max_iterations 1 and 2 and max_inner_iterations 3 (the epsilons at 1e-9, so that the iteration limit is
    what ends the run) from a guess 20 cm off: the only way to reach the fused mode (operator() plus df in one launch) and
    the server's restart between two correspondence steps.  Transform within ROT_TOL / TRANS_TOL of the oracle's; functor
    call counts, correspondences, iterations and the convergence flag identical."""
    for max_it in (1, 2):
        p = Pairing(rig.gmod, rig.tgt, rig.ct, 5.0, max_iterations=max_it, max_inner_iterations=3, rotation_epsilon=1e-9,
                    transformation_epsilon=1e-9)
        for n in sizes:
            cloud, _ = rig.heavy_tailed(n)
            p.source(cloud, rig.cs[:n])
            ro = p.o.align(GUESS)
            p.g.align(GUESS)
            T, st = p.g.getFinalTransformation(), p.g.stats()
            ctx = "%s n=%d max_iterations=%d" % (label, n, max_it)
            r, t = rot_err(T, ro["T"]), trans_err(T, ro["T"])
            print("%s: rot %.3g trans %.3g iterations %d calls %s" % (ctx, r, t, ro["iterations"], (st["n_f"], st["n_df"], st["n_fdf"])))
            note(OBJECTIVE, "align/rot", r)
            note(OBJECTIVE, "align/trans", t)
            assert r < ROT_TOL and t < TRANS_TOL, ctx
            assert (st["n_f"], st["n_df"], st["n_fdf"]) == (ro["n_f"], ro["n_df"], ro["n_fdf"]), ctx
            assert st["correspondences"] == ro["correspondences"], ctx
            assert p.g.hasConverged() == ro["converged"] and p.g.getFinalNumIteration() == ro["iterations"], ctx
            if n >= 4:
                assert ro["iterations"] == max_it and ro["n_f"] > 0, ctx   # the case is what it claims: it iterates


def test_limited_registrations_at_the_first_block_boundaries(rig, plan):
    """The first four source sizes of the functor sweep (one and two points, the last one-block size, the first of two
    blocks)."""
    check_limited_registrations(rig, sweep_sizes(plan)[:4], "first sizes")


def test_limited_registrations_above_the_server_cap(rig, plan):
    b, period = gps.cap_boundary(plan, "server_blocks", HI)
    check_limited_registrations(rig, [b + period + 1], "above the server cap")


# ------------------------------------------------------------------ the same checks under the switches
def rerun(select, env, timeout):
    """This file's tests that match `select`, in a process of their own under `env` (the switches are read once per
    process): all passed, none skipped."""
    child_env = dict(os.environ, **env)
    if os.environ.get("GICP_PLAN_REPORT"):
        child_env["GICP_PLAN_REPORT"] = os.environ["GICP_PLAN_REPORT"] + "." + "_".join("%s=%s" % kv for kv in sorted(env.items()))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gicp_gpu_plans.py"), "-q", "-s", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", select], env=child_env, capture_output=True, text=True, timeout=timeout,
                       cwd=ROOT)
    tail = r.stdout[-4000:] + r.stderr[-1500:]
    assert r.returncode == 0, tail
    last = r.stdout.strip().splitlines()[-1]
    assert " passed" in last and "skipped" not in last and "xfailed" not in last and "failed" not in last, tail
    at = r.stdout.rfind("GICP kernels at their plan boundaries")
    print("\n[%s] %s" % (" ".join("%s=%s" % kv for kv in sorted(env.items())), r.stdout[at:].strip() if at >= 0 else last))


def test_functor_sums_through_the_functor_kernel():
    """NDT_GICP_SERVER=0: every objective evaluation is a launch of k_functor (the last block's fixed-order sum) instead of
    a command to the persistent server -- the functor checks of this file once more, in a process of their own."""
    if not ON_SERVER:
        return  # (this process already runs without the server: the checks above are k_functor's)
    rerun("functor_sums and not through_the_functor_kernel", {"NDT_GICP_SERVER": "0"}, 280)


def test_limited_registration_without_the_fused_mode():
    """NDT_GICP_NO_FUSE=1: operator() and df as separate evaluations -- the registrations at the first block boundaries once
    more."""
    if os.environ.get("NDT_GICP_NO_FUSE"):
        return
    rerun("limited_registrations_at_the_first_block_boundaries", {"NDT_GICP_NO_FUSE": "1"}, 200)


def test_neighbours_and_correspondences_with_every_grid_capped_at_three_blocks():
    """NDT_GICP_MAX_BLOCKS=3 puts every cloud of more than 24 / 96 points into the grid-strided regime of the two search
    kernels, whose real caps (0.5 M and 1 M queries) lie where the oracle's exact search is what would take the time: this
    file's neighbour and correspondence tests once more, in a process of their own."""
    if os.environ.get("NDT_GICP_MAX_BLOCKS"):
        return  # (this process already runs under the switch: the checks above are the strided ones)
    code = ("import sys, json; sys.path.insert(0, %r); from toyslam_amd import gicp; "
            "print(json.dumps(gicp.GeneralizedIterativeClosestPoint().plan(2000)))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, NDT_GICP_MAX_BLOCKS="3"),
                         timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == dict(knn_blocks=3, correspond_blocks=3, functor_blocks=3, server_blocks=3)
    rerun("test_neighbours and not every_grid_capped or test_correspond", {"NDT_GICP_MAX_BLOCKS": "3"}, 280)
