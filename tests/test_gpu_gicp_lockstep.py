"""GPU: gicp_align_pairs_lockstep and gicp_align_guesses -- the registrations of a GICP pairs call advanced together, one
k_correspond_multi and one k_functor_multi launch per step.

What is EXPECTED never comes from the new calls: it is gicp_align_pairs_clouds' answer, what a fresh single-cloud handle fed
the host arrays gives (fresh / same_as_fresh of tests/test_gpu_gicp_pairs.py), or the CPU oracle's -- and against the first
two every comparison is bit for bit (np.array_equal, ==)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gicp_lockstep_cases as lc
from conftest import ROOT, rot_err, trans_err
from oracle import pyoracle as po
from test_gicp_gpu import ROT_TOL, TRANS_TOL, gmod  # noqa: F401  (gmod: the fixture)
from test_gpu_gicp_pairs import GUESS, fresh, same_as_fresh
from toyslam_amd import clouds

pytestmark = pytest.mark.gpu

CAP = int(os.environ.get("NDT_GICP_MAX_BLOCKS", "0") or 0)
WINDOW = min(256, max(1, int(os.environ.get("NDT_GICP_LOCKSTEP_MEMBERS", "32") or 32)))
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def up(gmod):
    from toyslam_amd import ndt
    return ndt.NormalDistributionsTransform()


@pytest.fixture(scope="module")
def edge():
    """(sources, targets) at the edges of the block plans"""
    return lc.noisy_subsets(lc.SOURCE_SIZES, seed=13), lc.noisy_subsets(lc.TARGET_SIZES, seed=17)


def handle(gmod, params=()):
    g = gmod.GeneralizedIterativeClosestPoint()
    for name, v in params:
        getattr(g, name)(v)
    return g


def same_as_sequential(lock, seq, ctx):
    for f in lc.FIELDS:
        assert np.array_equal(lock[f], seq[f]), (ctx, f)


# ------------------------------------------------------------------ 1. block edges in one call
def test_block_edges_in_one_call(gmod, up, edge):
    """Sources of 20 ... 2 500 points against targets of 2 500, 300 and 20: 24 members of 1 to 10 functor blocks and 1 to 79
    correspondence blocks in one lock-step, shuffled (every position of the bisection is used) and reversed."""
    src, tgt = edge
    g = handle(gmod)
    if not CAP:
        assert [g.plan(len(s))["server_blocks"] for s in src] == [1, 1, 1, 1, 2, 8, 9, 10]
        assert [g.plan(len(s))["correspond_blocks"] for s in src] == [1, 1, 2, 8, 9, 64, 65, 79]
    cl = list(tgt) + list(src)
    dcs = [up.uploadCloud(c) for c in cl]
    pairs = [(t, len(tgt) + s) for t in range(len(tgt)) for s in range(len(src))]
    order = [int(x) for x in np.random.default_rng(5).permutation(len(pairs))]
    want = {}
    for direction in (order, order[::-1]):
        P = [pairs[k] for k in direction]
        seq = g.alignPairsClouds(dcs, P, None, 1.0)
        lock = g.alignPairsLockstep(dcs, P, None, 1.0)
        d = g.diagLockstep()
        assert d["max_members_in_step"] == min(WINDOW, len(P)) and d["functor_launches"] == d["steps"] > 0
        same_as_sequential(lock, seq, "edges")
        for pos, k in enumerate(direction):
            t, s = pairs[k]
            if k not in want:
                want[k] = fresh(gmod, cl[t], cl[s], None, 1.0)
            same_as_fresh(lock, pos, want[k], "pair %s (%d onto %d points) at %d" % (pairs[k], len(cl[s]), len(cl[t]), pos))
    assert any(w[2] > 1 for w in want.values()) and all(np.all(np.isfinite(w[0])) for w in want.values())


# ------------------------------------------------------------------ 2. clouds in both roles
def test_clouds_in_both_roles(gmod, up, edge):
    src, tgt = edge
    a, b, c = src[7], tgt[0], src[5]
    cl = [a, b, c]
    dcs = [up.uploadCloud(x) for x in cl]
    g1 = clouds.make_T([0.05, -0.03, 0.02], [0.004, -0.003, 0.01]).astype(np.float32)
    g2 = clouds.make_T([-0.04, 0.06, 0.0], [0.0, 0.005, -0.008]).astype(np.float32)
    pairs = [(0, 1), (1, 0), (2, 2), (1, 2), (1, 2), (1, 2)]
    guesses = [EYE, EYE, g1, EYE, g1, g2]
    g = handle(gmod)
    seq = g.alignPairsClouds(dcs, pairs, guesses, 1.0)
    dseq = g.diagPairs()
    lock = g.alignPairsLockstep(dcs, pairs, guesses, 1.0)
    assert g.diagPairs() == dseq and dseq["index_builds"] == 3 and dseq["knn_launches"] == 1
    same_as_sequential(lock, seq, "roles")
    for k, ((t, s), gu) in enumerate(zip(pairs, guesses)):
        same_as_fresh(lock, k, fresh(gmod, cl[t], cl[s], gu, 1.0), "pair %d %s" % (k, (t, s)))
    for i in range(3):   # the covariances the lock-step call keeps are the sequential call's
        cov = g.pairsCovariances(i)
        g.alignPairsClouds(dcs, pairs[:1] + pairs[2:4])
        assert np.array_equal(g.pairsCovariances(i), cov)
        g.alignPairsLockstep(dcs, pairs, guesses, 1.0)


# ------------------------------------------------------------------ 3. members that leave at different steps
def test_members_leave_at_different_steps(gmod, up, edge):
    src, tgt = edge
    t, s = tgt[0], src[6]
    dcs = [up.uploadCloud(t), up.uploadCloud(s), up.uploadCloud(src[4])]
    answer = fresh(gmod, t, s, None, 1.0)
    assert answer[1] and answer[2] > 1
    off = (clouds.make_T([0.3, 0.0, 0.0], np.radians([0.0, 0.0, 1.0])) @ answer[0].astype(np.float64)).astype(np.float32)
    pairs = [(0, 1), (0, 1), (0, 1), (0, 2)]
    guesses = [answer[0], off, EYE, EYE]
    for params in ((), (("setMaximumIterations", 1),), (("setMaximumIterations", 2),)):
        g = handle(gmod, params)
        lock = g.alignPairsLockstep(dcs, pairs, guesses, 1.0)
        same_as_sequential(lock, g.alignPairsClouds(dcs, pairs, guesses, 1.0), params)
        cl = [t, s, src[4]]
        for k, ((a, b), gu) in enumerate(zip(pairs, guesses)):
            same_as_fresh(lock, k, fresh(gmod, cl[a], cl[b], gu, 1.0, params), "%s pair %d" % (params, k))
        if not params:
            assert lock["iterations"][0] == 1 and lock["converged"][0]   # from the previous answer: one outer iteration
            assert len(set(int(x) for x in lock["iterations"])) > 1
    # a gate nothing passes: fewer than 4 correspondences, the member ends in its first step
    gate = (("setMaxCorrespondenceDistance", 1e-6),)
    g = handle(gmod, gate)
    lock = g.alignPairsLockstep(dcs, pairs[2:], guesses[2:], 1.0)
    assert not lock["converged"].any() and np.all(lock["iterations"] == 0) and np.all(lock["correspondences"] < 4)
    same_as_fresh(lock, 0, fresh(gmod, t, s, EYE, 1.0, gate), "gated pair")
    assert g.diagLockstep() == dict(steps=1, correspond_launches=1, functor_launches=1, max_members_in_step=2)


# ------------------------------------------------------------------ 4. advanced together
def test_copies_advance_together(gmod, up, edge):
    src, tgt = edge
    dcs = [up.uploadCloud(tgt[0]), up.uploadCloud(src[5])]
    gu = clouds.make_T([0.05, -0.03, 0.02], [0.004, -0.003, 0.01]).astype(np.float32)
    want = fresh(gmod, tgt[0], src[5], gu, 1.0)
    one = None
    for params in ((), (("setMaxCorrespondenceDistance", 1e-6),)):
        for M in (1, 2, 9):
            if M > WINDOW:
                continue
            g = handle(gmod, params)
            r = g.alignPairsLockstep(dcs, [(0, 1)] * M, [gu] * M, 1.0)
            d = g.diagLockstep()
            if M == 1:
                one = d
            outer = int(r["iterations"][0])
            # the loop leaves through convergence after `outer` correspondence steps, or through the exception of an
            # estimate that fails: one more correspondence step than counted iterations
            by_exception = not bool(r["converged"][0])
            assert d["steps"] == one["steps"] and d["functor_launches"] == d["steps"], (M, d, one)
            assert d["correspond_launches"] == outer + (1 if by_exception else 0), (M, d, outer)
            assert d["max_members_in_step"] == M
            if not params:
                for k in range(M):
                    same_as_fresh(r, k, want, "copy %d of %d" % (k, M))
                assert d["steps"] > outer > 1
            else:
                assert by_exception and outer == 0


# ------------------------------------------------------------------ 5. against the oracle
@pytest.fixture(scope="module")
def scene():
    tgt = clouds.target_surfaces(20000)[:, :3].astype(np.float32)
    src = clouds.source_from_target(tgt, 8000)[:, :3].astype(np.float32)
    return tgt, src


@pytest.fixture(scope="module")
def oracle(scene):
    o = po.OracleGICP()
    o.setInputTarget(scene[0])
    o.setInputSource(scene[1])
    return o


@pytest.mark.parametrize("case", ["identity", "guess"])
def test_lockstep_call_matches_the_oracle(gmod, up, scene, oracle, case):
    guess = GUESS if case == "guess" else None
    ro = oracle.align(guess)
    g = handle(gmod)
    r = g.alignPairsLockstep([up.uploadCloud(scene[0]), up.uploadCloud(scene[1])], [(0, 1)], None if guess is None else [guess])
    rot, tr = rot_err(r["T"][0], ro["T"]), trans_err(r["T"][0], ro["T"])
    print("%s: rot %.3g trans %.3g iterations %d" % (case, rot, tr, ro["iterations"]))
    assert rot < ROT_TOL and tr < TRANS_TOL
    assert bool(r["converged"][0]) == ro["converged"] and int(r["iterations"][0]) == ro["iterations"]
    assert int(r["correspondences"][0]) == ro["correspondences"]


# ------------------------------------------------------------------ 6. the switches, each in a process of its own
STOP = []   # a child that ended by a signal or at its time limit: nothing further is started


def run_child(tmp_path, **env):
    if STOP:
        pytest.fail("not started: an earlier child process " + STOP[0])
    out = tmp_path / "child.json"
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gicp_lockstep_child.py"), str(out)], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=120, cwd=ROOT)
    except subprocess.TimeoutExpired:
        STOP.append("ran into its time limit")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        STOP.append("ended by a signal (%d)" % r.returncode)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    with open(out) as f:
        j = json.load(f)
    return lc.from_json(j["lockstep"]), lc.from_json(j["sequential"]), j["diag"], j["plan"]


@pytest.fixture(scope="module")
def child_sequential(gmod, up):
    """the child's five pairs through the sequential call, in this process"""
    g = handle(gmod)
    r = g.alignPairsClouds([up.uploadCloud(c) for c in lc.noisy_subsets(lc.CHILD_SIZES, seed=29)], None, lc.child_guesses(), 1.0)
    for v in r.values():
        v.setflags(write=False)
    return r


def test_window_of_two_slides(tmp_path, child_sequential):
    """NDT_GICP_LOCKSTEP_MEMBERS=2 with 5 pairs: two in flight, the next starts when one ends; same bits."""
    lock, seq, diag, _ = run_child(tmp_path, NDT_GICP_LOCKSTEP_MEMBERS="2")
    same_as_sequential(lock, seq, "window 2 (child's sequential call)")
    assert diag["max_members_in_step"] == 2 and diag["functor_launches"] == diag["steps"]
    if not CAP and "NDT_GICP_NO_FUSE" not in os.environ:
        same_as_sequential(lock, child_sequential, "window 2")


def test_every_member_strided_by_three_blocks(tmp_path):
    """NDT_GICP_MAX_BLOCKS=3: every member of more than 768 points strides by three blocks in both kernels (the sequential
    call sums over the same three)."""
    lock, seq, diag, plan = run_child(tmp_path, NDT_GICP_MAX_BLOCKS="3")
    assert [p["server_blocks"] for p in plan] == [3, 3, 3, 3, 2, 1] and [p["correspond_blocks"] for p in plan] == [3, 3, 3, 3, 3, 2]
    same_as_sequential(lock, seq, "three blocks")
    assert diag["max_members_in_step"] == min(WINDOW, 5)


def test_without_the_fused_mode(tmp_path, child_sequential):
    """NDT_GICP_NO_FUSE=1: operator() is asked as mode 0 and every df goes to the device."""
    lock, seq, diag, _ = run_child(tmp_path, NDT_GICP_NO_FUSE="1")
    same_as_sequential(lock, seq, "not fused (child's sequential call)")
    assert diag["functor_launches"] == diag["steps"] > 0


# ------------------------------------------------------------------ 7. alignGuesses
def guesses_of(n, seed=41):
    rng = np.random.default_rng(seed)
    return [clouds.make_T(rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.01, 0.01, 3)).astype(np.float32) for _ in range(n)]


def expected_from_align(g, guesses, max_range):
    out = []
    for gu in guesses:
        g.align(gu)
        out.append((g.getFinalTransformation(), g.hasConverged(), g.getFinalNumIteration(), g.stats()["correspondences"],
                    g.getFitnessScore(max_range)))
    return out


def check_guesses(g, guesses, max_range, ctx):
    want = expected_from_align(g, guesses, max_range)
    before = (g.getFinalTransformation(), g.hasConverged(), g.getFinalNumIteration(), g.stats(), g.covariances(0), g.covariances(1))
    r = g.alignGuesses(guesses, max_range)
    after = (g.getFinalTransformation(), g.hasConverged(), g.getFinalNumIteration(), g.stats(), g.covariances(0), g.covariances(1))
    for x, y in zip(before, after):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, ctx
    for k in range(len(guesses)):
        same_as_fresh(r, k, want[k], "%s guess %d of %d" % (ctx, k, len(guesses)))
    assert g.diagLockstep()["max_members_in_step"] == min(WINDOW, len(guesses))
    return r


def test_align_guesses_equals_align_per_guess(gmod, edge):
    src, tgt = edge
    g = handle(gmod)
    g.setInputTarget(tgt[0])
    g.setInputSource(src[6])
    all_g = guesses_of(9)
    first = handle(gmod)      # a handle that has never aligned: the covariances are computed by the call itself
    first.setInputTarget(tgt[0])
    first.setInputSource(src[6])
    r0 = first.alignGuesses(all_g[:2], 1.0)
    for n in (1, 2, 9):
        r = check_guesses(g, all_g[:n], 1.0, "own covariances")
    for k in range(2):
        assert np.array_equal(r0["T"][k], r["T"][k]) and r0["fitness"][k] == r["fitness"][k]
    assert len(set(int(x) for x in r["iterations"])) > 1 or len(set(r["fitness"])) > 1
    # a new source is followed
    g.setInputSource(src[5])
    check_guesses(g, all_g[:2], 1.0, "new source")
    # caller-set covariances are the ones used
    rng = np.random.default_rng(5)

    def spd(n):
        a = rng.normal(0, 1, (n, 3, 3))
        return (a @ a.transpose(0, 2, 1)) * 0.01 + 1e-3 * np.eye(3)

    g.setTargetCovariances(spd(len(tgt[0])))
    g.setSourceCovariances(spd(len(src[5])))
    rc = check_guesses(g, all_g[:2], 1.0, "caller-set covariances")
    g.setTargetCovariances(None)
    g.setSourceCovariances(None)
    rk = check_guesses(g, all_g[:2], 1.0, "k-NN covariances again")
    assert not np.array_equal(rc["T"], rk["T"])


# ------------------------------------------------------------------ 8. the handle afterwards
def test_lockstep_call_leaves_the_handle_as_it_was(gmod, up, scene, edge):
    src, tgt = edge
    big_t, big_s = scene[0][:6000], scene[1][:2500]
    rng = np.random.default_rng(5)

    def spd(n):
        a = rng.normal(0, 1, (n, 3, 3))
        return (a @ a.transpose(0, 2, 1)) * 0.01 + 1e-3 * np.eye(3)

    g = handle(gmod)
    g.setInputTarget(big_t)
    g.setInputSource(big_s)
    g.setTargetCovariances(spd(len(big_t)))
    g.setSourceCovariances(spd(len(big_s)))
    g.align(GUESS)

    def state():
        return (g.getFinalTransformation(), g.hasConverged(), g.getFinalNumIteration(), g.stats(), g.covariances(0), g.covariances(1),
                g.getFitnessScore(1.0))

    before = state()
    cl = [tgt[0], src[7], src[6], src[5]]
    dcs = [up.uploadCloud(c) for c in cl]
    pairs = [(0, 1), (1, 2), (2, 3)]
    r = g.alignPairsLockstep(dcs, pairs, max_range=1.0)
    assert r["T"].shape == (3, 4, 4) and not np.array_equal(r["T"][0], before[0])
    after = state()
    assert np.isfinite(before[6]) and before[6] > 0
    for x, y in zip(before, after):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    g.align(GUESS)
    assert np.array_equal(g.getFinalTransformation(), before[0]) and g.stats() == before[3]
    # ... and the call did not use the handle's supplied covariances: pair 0 is a fresh handle's
    same_as_fresh(r, 0, fresh(gmod, cl[0], cl[1], None, 1.0), "pair 0 after a used handle")
    # the step scratch is the handle's own: a lock-step call does not touch it
    x = np.array([0.1, -0.2, 0.05, 0.01, -0.02, 0.03])
    g.step_correspond(GUESS)
    f0, g0 = g.step_functor(2, x)
    g.alignPairsLockstep(dcs, pairs, max_range=1.0)
    f1, g1 = g.step_functor(2, x)
    assert np.isfinite(f0) and f1 == f0 and np.array_equal(g1, g0)
    # a handle whose covariances are its own k-NN ones: the source's, with their neighbour lists, around a lock-step call
    h = handle(gmod)
    h.setInputTarget(big_t)
    h.setInputSource(big_s)
    nb_before = h.covariances(1, neighbors=True)
    h.alignPairsLockstep(dcs, pairs, max_range=1.0)
    nb_after = h.covariances(1, neighbors=True)
    for a, b in zip(nb_before, nb_after):
        assert np.array_equal(a, b)
    # pool and scratch reuse: a sequential call right after a lock-step call, and the reverse
    s1 = h.alignPairsClouds(dcs, pairs, max_range=1.0)
    l1 = h.alignPairsLockstep(dcs, pairs, max_range=1.0)
    s2 = h.alignPairsClouds(dcs, pairs, max_range=1.0)
    l2 = h.alignPairsLockstep(dcs[::-1], [(3 - a, 3 - b) for a, b in pairs], max_range=1.0)
    for other in (l1, s2, l2, r):
        same_as_sequential(other, s1, "calls in turn")


# ------------------------------------------------------------------ 9. apps/pair_sequence --gicp --lockstep
def test_pair_sequence_app_lockstep_prints_what_gicp_prints(gmod, tmp_path):
    from test_gpu_pairs import build_app
    from toyslam_amd import ndt
    d = tmp_path / "pcd"
    d.mkdir()
    for k, sc in enumerate(lc.noisy_subsets([2500, 2400, 2300, 2200], seed=31), 1):
        ndt.pcd_write_xyz(str(d / ("cloud_%d.pcd" % k)), sc)
    exe = build_app(tmp_path, "pair_sequence")
    outs = []
    for extra in ([], ["--lockstep"]):
        out = subprocess.run([exe, str(d), "--gicp", "--fitness"] + extra, capture_output=True, text=True, timeout=120)
        if out.returncode < 0:
            pytest.fail("pair_sequence ended by a signal (%d): %s" % (out.returncode, out.stderr[-1500:]))
        assert out.returncode == 0, out.stderr[-2000:]
        outs.append([ln for ln in out.stdout.splitlines() if not ln.startswith("time")])
    assert outs[0] == outs[1] and sum(ln.startswith("fitness ") for ln in outs[0]) == 3
    assert any(ln.startswith("Transform ") for ln in outs[0])
