"""GPU: ndt_score_poses (k_score_poses), ndt_align_guesses and ndt_align_multistart.

scorePoses is held to two references: the CPU oracle's calculate_score of the oracle-transformed cloud (rel 1e-11, the figure
tests/test_gpu_parity.py holds calculateScore to) and the library's own calculateScore of that cloud, BIT FOR BIT -- same f32
transform, same walk of the points, same reduction.  alignGuesses is held to alignBatch over the source repeated (bit for
bit) and to the oracle's align from every guess (the suite's batch tolerances, identical iteration counts).

The two switches that are read once per process (NDT_K2_MAX_BLOCKS, NDT_SCORE_POSES_CHUNK) are exercised in a child
process each (tests/score_poses_child.py computes, this file compares)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import score_poses_cases as spc
import score_poses_child as child
from conftest import ROOT, rot_err, trans_err
from test_gpu_parity import ROT_TOL, TRANS_TOL, mods  # noqa: F401  (mods: the fixture)

pytestmark = pytest.mark.gpu

PLAN_SIZES = (1, 255, 256, 257, 1025)
PLAN_POSES = (spc.I_IDENTITY, spc.I_GOLDEN, 2, 3, 4, spc.I_YAW90, spc.I_FAR)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Scene:
    """The bundled pair under the four neighbour rules: a GPU handle and an oracle per rule, and the oracle's answers per
    (rule, source size), computed once."""

    def __init__(self, mods, pair, golden):
        self.ndt, self.po, _ = mods
        self.t, self.s = pair
        self.P = spc.poses(golden)
        self.handles, self.oracles, self.refs, self.clouds = {}, {}, {}, {}

    def handle(self, method):
        if method not in self.handles:
            g = self.ndt.NormalDistributionsTransform()
            g.setNeighborhoodSearchMethod(getattr(self.po, method))
            g.setInputTarget(self.t)
            self.handles[method] = g
        return self.handles[method]

    def oracle(self, method):
        if method not in self.oracles:
            o = self.po.OracleNDT(num_threads=16, search_method=getattr(self.po, method))
            o.set_target(self.t)
            o.set_source(self.s[:10])
            self.oracles[method] = o
        return self.oracles[method]

    def moved(self, n, k):
        """pcl::transformPointCloud(source[:n], pose k), by the oracle"""
        if (n, k) not in self.clouds:
            self.clouds[(n, k)] = spc.moved(self.po, self.s[:n], self.P[k])
        return self.clouds[(n, k)]

    def ref(self, method, n, which):
        key = (method, n, tuple(which))
        if key not in self.refs:
            o = self.oracle(method)
            self.refs[key] = np.array([o.calculate_score(self.moved(n, k)) for k in which])
        return self.refs[key]


@pytest.fixture(scope="module")
def scene(mods, pair, golden):
    return Scene(mods, pair, golden)


def check_both(scene, method, n, which, got, single=None):
    """got[j] = scorePoses of pose which[j] over source[:n]: against the oracle (rel 1e-11, the far pose exactly 0.0) and
    against calculateScore of the moved cloud (the same bits)."""
    want = scene.ref(method, n, which)
    g = scene.handle(method)
    for j, k in enumerate(which):
        ctx = "%s n=%d pose %d" % (method, n, k)
        print("%s: scorePoses %.17g oracle %.17g" % (ctx, got[j], want[j]))
        assert got[j] == pytest.approx(want[j], rel=1e-11), ctx
        one = g.calculateScore(scene.moved(n, k)) if single is None else single[j]
        assert same_bits([got[j]], [one]), ctx + ": %r != calculateScore's %r" % (float(got[j]).hex(), float(one).hex())
        if k == spc.I_FAR:
            assert got[j] == 0.0 and want[j] == 0.0, ctx


# ------------------------------------------------------------------ scorePoses
@pytest.mark.parametrize("method", spc.METHODS)
def test_scores_match_the_oracle_and_calculate_score(scene, method):
    g = scene.handle(method)
    n = len(scene.s)
    g.setInputSource(scene.s)
    got = g.scorePoses(scene.P)
    assert got.shape == (spc.N_POSES,) and np.isfinite(got).all()
    assert g.scorePosesLaunches() == (1, spc.N_POSES * g.evalPlan(n)["launch_blocks"])
    check_both(scene, method, n, range(spc.N_POSES), got)
    assert all(got[k] != 0.0 for k in spc.near_indices())
    # the order of the poses is the order of the scores
    perm = np.random.default_rng(11).permutation(spc.N_POSES)
    assert same_bits(g.scorePoses([scene.P[k] for k in perm]), got[perm])
    assert same_bits(g.scorePoses([scene.P[spc.I_GOLDEN]]), got[spc.I_GOLDEN:spc.I_GOLDEN + 1])


@pytest.mark.parametrize("n", PLAN_SIZES)
def test_scores_at_the_block_plan_sizes(scene, n):
    """One point, one block less a lane, exactly, plus a lane, and a fifth block of one point."""
    for method in spc.METHODS:
        g = scene.handle(method)
        g.setInputSource(scene.s[:n])
        got = g.scorePoses([scene.P[k] for k in PLAN_POSES])
        blocks = g.evalPlan(n)["launch_blocks"]
        if "NDT_K2_MAX_BLOCKS" not in os.environ:
            assert blocks == (n + 255) // 256
        assert g.scorePosesLaunches() == (1, len(PLAN_POSES) * blocks)
        check_both(scene, method, n, PLAN_POSES, got)


def run_child(mode, tmp_path, **env):
    out = tmp_path / (mode + ".json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "score_poses_child.py"), mode, str(out)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    with open(out) as f:
        return json.load(f)


def unhex(v):
    return np.array([float.fromhex(x) for x in v])


def test_scores_where_the_walk_is_strided(scene, tmp_path):
    """NDT_K2_MAX_BLOCKS=3: 768 points fill the three blocks, from 769 a thread walks several points."""
    res = run_child("capped", tmp_path, NDT_K2_MAX_BLOCKS="3")
    which = range(spc.N_POSES)
    for method in spc.METHODS:
        for n in child.CAPPED_SIZES:
            r = res["%s/%d" % (method, n)]
            assert r["plan_blocks"] == 3 and (r["launches"], r["blocks"]) == (1, 3 * spc.N_POSES), (method, n)
            check_both(scene, method, n, which, unhex(r["poses"]), single=unhex(r["single"]))


def test_chunked_scores_are_the_unchunked_ones(scene, golden, tmp_path):
    """NDT_SCORE_POSES_CHUNK=7: 1, 7, 8 and 50 poses take 1, 1, 2 and 8 launches and give the bits of the one-launch call."""
    P = child.chunk_poses(golden)
    g = scene.handle("DIRECT7")
    g.setInputSource(scene.s)
    whole = g.scorePoses(P)
    if "NDT_SCORE_POSES_CHUNK" not in os.environ:
        assert g.scorePosesLaunches()[0] == 1
    res = run_child("chunked", tmp_path, NDT_SCORE_POSES_CHUNK="7")
    for count, launches in zip(child.CHUNKED_COUNTS, (1, 1, 2, 8)):
        r = res[str(count)]
        assert r["launches"] == launches, count
        assert same_bits(unhex(r["poses"]), whole[:count]), count
    assert sorted(res["perm"]) == list(range(50)) and res["perm"] != list(range(50))
    assert same_bits(unhex(res["permuted"]), whole[res["perm"]])


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("method", spc.METHODS)
def test_source_with_non_finite_points(scene, method):
    """NaN / inf points (the last point among them) and an absurdly far one: counted in the divisor, adding nothing."""
    po = scene.po
    g = scene.handle(method)
    o = scene.oracle(method)
    c = spc.spoiled(scene.s[:2000])
    g.setInputSource(c)
    which = PLAN_POSES
    got = g.scorePoses([scene.P[k] for k in which])
    for j, k in enumerate(which):
        m = spc.moved(po, c, scene.P[k])
        assert got[j] == pytest.approx(o.calculate_score(m), rel=1e-11), (method, k)
        assert same_bits([got[j]], [g.calculateScore(m)]), (method, k)
    assert got[which.index(spc.I_FAR)] == 0.0
    # the divisor is the source's size, bad points included: the clean points alone score higher by exactly that ratio
    clean = c[np.isfinite(c).all(axis=1) & (np.abs(c) < 1e20).all(axis=1)]
    assert len(clean) == len(c) - 4
    g.setInputSource(clean)
    alone = g.scorePoses([scene.P[spc.I_GOLDEN]])[0]
    assert alone * len(clean) == pytest.approx(got[which.index(spc.I_GOLDEN)] * len(c), rel=1e-12)


def test_empty_grid_empty_source_and_missing_inputs(scene):
    ndt, po = scene.ndt, scene.po
    P = [scene.P[k] for k in PLAN_POSES]
    # an empty target -> an empty grid: 0.0 for every pose, nothing launched
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(np.zeros((0, 3), np.float32))
    g.setInputSource(scene.s[:300])
    got = g.scorePoses(P)
    assert same_bits(got, np.zeros(len(P))) and g.scorePosesLaunches() == (0, 0)
    assert g.calculateScore(scene.moved(300, spc.I_GOLDEN)) == 0.0
    r = g.alignGuesses(P[:2])
    assert list(r["iterations"]) == [0, 0] and r["converged"].all()   # (zero rows: the Newton step is 0, as a single align)
    same_registrations(r, g.alignBatch([scene.s[:300]] * 2, P[:2]), "an empty target")
    # a target without a voxel of six points: gridded like any other (its counts are not waited for), every probe misses
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [5, 5, 5]], np.float32))
    assert g.grid_counts()["n_valid"] == 0
    g.setInputSource(scene.s[:300])
    got = g.scorePoses(P)
    assert same_bits(got, np.zeros(len(P))) and g.scorePosesLaunches() == (1, len(P) * g.evalPlan(300)["launch_blocks"])
    assert g.calculateScore(scene.moved(300, spc.I_GOLDEN)) == 0.0
    r = g.alignGuesses(P[:2])
    same_registrations(r, g.alignBatch([scene.s[:300]] * 2, P[:2]), "a target without a valid voxel")
    # a source of no points: 0 / 0, as calculateScore of an empty cloud
    g = scene.handle("DIRECT7")
    g.setInputSource(np.zeros((0, 3), np.float32))
    assert np.isnan(g.calculateScore(np.zeros((0, 3), np.float32)))
    got = g.scorePoses(P)
    assert got.shape == (len(P),) and np.isnan(got).all()
    # no source, no target
    g = ndt.NormalDistributionsTransform()
    for call in (lambda: g.scorePoses(P), lambda: g.alignGuesses(P), lambda: g.alignMultistart(P, 2)):
        with pytest.raises(ndt.NdtError) as e:
            call()
        assert e.value.status == ndt._lib.NDT_ERR_NO_INPUT
    g.setInputTarget(scene.t)
    for call in (lambda: g.scorePoses(P), lambda: g.alignGuesses(P), lambda: g.alignMultistart(P, 2)):
        with pytest.raises(ndt.NdtError) as e:
            call()
        assert e.value.status == ndt._lib.NDT_ERR_NO_INPUT


def result_bits(g):
    T, conv, it, tp = g._result()
    return T.tobytes(), conv, it, float(tp).hex()


def test_the_handles_own_result_is_left_alone(scene):
    ndt = scene.ndt
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(scene.t)
    g.setInputSource(scene.s)
    g.align()
    before = result_bits(g)
    assert before[1] and before[2] > 0
    g.scorePoses(scene.P)
    assert result_bits(g) == before
    g.alignGuesses([scene.P[2], scene.P[3]])
    assert result_bits(g) == before
    g.alignMultistart(scene.P, 2)
    assert result_bits(g) == before
    assert np.isfinite(g.getFitnessScore())   # (still the fitness of the handle's own last align)


# ------------------------------------------------------------------ alignGuesses
def same_registrations(a, b, ctx):
    assert a["T"].shape == b["T"].shape, ctx
    assert a["T"].tobytes() == b["T"].tobytes(), ctx
    assert list(a["converged"]) == list(b["converged"]) and list(a["iterations"]) == list(b["iterations"]), ctx
    assert same_bits(a["trans_probability"], b["trans_probability"]), ctx


@pytest.fixture(scope="module")
def oracle_aligns(scene, golden):
    """The oracle's align of the bundled pair from each of the nine guesses, once."""
    G = spc.guesses(golden, 9)
    o = scene.po.OracleNDT(num_threads=16)
    o.set_target(scene.t)
    o.set_source(scene.s)
    return G, [o.align(T) for T in G]


@pytest.mark.parametrize("n_guesses", [1, 2, 9])
def test_align_guesses_is_align_batch_of_the_source_repeated(scene, oracle_aligns, n_guesses):
    ndt = scene.ndt
    G, want = oracle_aligns
    G = G[:n_guesses]
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(scene.t)
    g.setInputSource(scene.s)
    twin = g.copy()
    got = g.alignGuesses(G)
    same_registrations(got, twin.alignBatch([scene.s] * n_guesses, G), "%d guesses" % n_guesses)
    for k in range(n_guesses):
        ctx = "guess %d of %d" % (k, n_guesses)
        r, t = rot_err(got["T"][k], want[k]["T"]), trans_err(got["T"][k], want[k]["T"])
        print("%s: rot %.3g trans %.3g iterations %d/%d" % (ctx, r, t, got["iterations"][k], want[k]["iterations"]))
        assert r < ROT_TOL and t < TRANS_TOL, ctx
        assert got["iterations"][k] == want[k]["iterations"] and bool(got["converged"][k]) == want[k]["converged"], ctx
        assert got["trans_probability"][k] == pytest.approx(want[k]["trans_probability"], rel=1e-5), ctx
    assert got["best"] == int(np.nanargmax(got["trans_probability"]))
    assert g.stats()["n_evals"] >= int(got["iterations"].sum())   # (statistics as a batch: all members' evaluations)


def test_align_guesses_follows_the_input_source(scene, golden):
    """A second call after setInputSource of another cloud registers the new cloud; a source with non-finite points is the
    member alignBatch makes of it."""
    ndt = scene.ndt
    G = spc.guesses(golden, 2)
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(scene.t)
    g.setInputSource(scene.s)
    first = g.alignGuesses(G)
    other = spc.spoiled(scene.s[1::2], far=False)
    g.setInputSource(other)
    second = g.alignGuesses(G)
    twin = ndt.NormalDistributionsTransform()
    twin.setInputTarget(scene.t)
    same_registrations(second, twin.alignBatch([other, other], G), "the new source")
    same_registrations(first, twin.alignBatch([scene.s, scene.s], G), "the first source")
    assert first["T"].tobytes() != second["T"].tobytes()


# ------------------------------------------------------------------ alignMultistart
def test_multistart_scores_picks_and_registers(scene):
    ndt = scene.ndt
    cand = scene.P + spc.far_poses(7)
    assert len(cand) == 40
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(scene.t)
    g.setInputSource(scene.s)
    scores = g.scorePoses(cand)
    want_picked = ndt.host_pick_top(scores, 4)
    assert list(want_picked) == list(spc.argsort_top(scores, 4)) and want_picked[0] == spc.I_GOLDEN
    got = g.alignMultistart(cand, 4)
    assert list(got["picked"]) == list(want_picked)
    same_registrations(got, g.alignGuesses([cand[k] for k in want_picked]), "multistart members")
    assert got["best"] == int(want_picked[int(np.nanargmax(got["trans_probability"]))])
    assert got["converged"][list(got["picked"]).index(got["best"])]
    # keep larger than the candidates: every candidate, best first
    few = g.alignMultistart(cand[:3], 10)
    assert list(few["picked"]) == list(spc.argsort_top(scores[:3], 10)) and few["T"].shape == (3, 4, 4)


def test_multistart_with_every_candidate_far_away(scene):
    """All scores are 0.0: ties, which are still finite scores, so the lowest indices are picked and the call succeeds."""
    ndt = scene.ndt
    cand = spc.far_poses(40)
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(scene.t)
    g.setInputSource(scene.s[:4000])
    assert same_bits(g.scorePoses(cand), np.zeros(40))
    got = g.alignMultistart(cand, 4)
    assert list(got["picked"]) == [0, 1, 2, 3]
    assert got["T"].shape == (4, 4, 4) and got["best"] in (-1, 0, 1, 2, 3)
    same_registrations(got, g.alignGuesses(cand[:4]), "far members")
