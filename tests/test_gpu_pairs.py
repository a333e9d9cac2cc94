"""GPU: ndt_align_pairs* -- (target, source) pairs of clouds registered in lock-step, every pair against the grid of its own
target.  Each pair must get what a single registration of that pair gets, the same bits in any call (grouping, order,
company), and the grids must be those a handle with that target builds."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, rot_err, trans_err

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-4, 1e-3


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from oracle import pyoracle as po
    from toyslam_amd import clouds, ndt
    return ndt, po, clouds


def handle(ndt, method=None, eps=0.01, iters=40):
    g = ndt.NormalDistributionsTransform()
    if method is not None:
        g.setNeighborhoodSearchMethod(method)
    g.setTransformationEpsilon(eps)
    g.setMaximumIterations(iters)
    return g


def ragged_clouds(clouds, t, s):
    """clouds of every awkward kind, and pairs over them"""
    rng = np.random.default_rng(31)
    big = clouds.target_surfaces(60000, seed=5, extent=40.0)[:, :3].astype(np.float32)  # above the small-form limit
    sparse = np.c_[rng.uniform(-3000, 3000, (4000, 2)), rng.uniform(-2, 2, 4000)].astype(np.float32)  # box too big for a dense LUT
    sparse = np.concatenate([sparse, s[:3000] + sparse[0]]).astype(np.float32)
    lonely = rng.uniform(-40, 40, (30, 3)).astype(np.float32)  # every voxel below min_points_per_voxel
    cl = [t,                                                                              # 0
          clouds.apply_T(np.linalg.inv(clouds.random_T(rng, 0.3, 1.0)), s[::2].copy()),  # 1
          clouds.apply_T(np.linalg.inv(clouds.random_T(rng, 0.3, 1.0)), s[1::3].copy()),  # 2
          (t + 700.0).astype(np.float32),                                                 # 3 far from the origin
          (s[::2] + 700.0).astype(np.float32),                                            # 4
          big,                                                                            # 5
          clouds.apply_T(np.linalg.inv(clouds.random_T(rng, 0.2, 0.5)), big[::3].copy()), # 6
          sparse,                                                                         # 7
          (s[:3000] + sparse[0] + np.float32(0.05)).astype(np.float32),                   # 8
          lonely,                                                                         # 9
          np.zeros((0, 3), np.float32),                                                   # 10
          s[2000:2007].copy()]                                                            # 11
    pairs = [(0, 1), (0, 2), (1, 2), (3, 4), (5, 6), (7, 8), (9, 1), (10, 1), (0, 10), (2, 2), (0, 11), (6, 5)]
    return cl, pairs


def single(g, tgt, src, guess=None, is_dense=True):
    g.setInputTarget(tgt, is_dense=is_dense)
    g.setInputSource(src)
    g.align(guess)
    return g.getFinalTransformation(), g.getFinalNumIteration(), g.hasConverged(), g.getTransformationProbability()


def same(a, b):
    return (np.array_equal(a["T"], b["T"], equal_nan=True) and np.array_equal(a["iterations"], b["iterations"])
            and np.array_equal(a["converged"], b["converged"]) and np.array_equal(a["trans_probability"], b["trans_probability"], equal_nan=True))


def grids_equal(a, b):
    for k in ("idx", "n", "mean", "cov", "icov", "evals", "min_b", "max_b", "div_b"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n_valid"] == b["n_valid"]


def test_pairs_grids_equal_single_handle_grids(mods, pair):
    ndt, po, clouds = mods
    t, s = pair
    cl, pairs = ragged_clouds(clouds, t, s)
    g = handle(ndt)
    g.alignPairs(cl, pairs)
    ref = handle(ndt)
    targets = sorted({p[0] for p in pairs})
    for c in targets:
        ref.setInputTarget(cl[c])
        grids_equal(g.pairsGrid(c), ref.grid())
    assert g.pairsGrid(9)["n_valid"] == 0 and len(g.pairsGrid(7)["idx"]) > 0
    # a cloud that was no target has no pairs grid
    from toyslam_amd._lib import NdtError, NDT_ERR_NO_INPUT
    with pytest.raises(NdtError) as e:
        g.pairsGrid(8)
    assert e.value.status == NDT_ERR_NO_INPUT
    # NaN targets under is_dense = 0
    nan_t = t.copy()
    nan_t[::9] = np.nan
    nan_t[5::17] = np.inf
    g.alignPairs([nan_t, cl[1]], [(0, 1)], is_dense=False)
    ref.setInputTarget(nan_t, is_dense=False)
    grids_equal(g.pairsGrid(0), ref.grid())


@pytest.mark.parametrize("env", [{}, {"NDT_K1_SMALL_LIST": "8"}, {"NDT_K1_LDS_CAP": "512"}, {"NDT_K1_SMALL_FINISH": "0"}],
                         ids=["default", "lists_overflow_second_scan", "small_passes", "general_finish_only"])
def test_pairs_grids_equal_single_handle_grids_in_every_small_form_regime(mods, env, tmp_path):
    """The one-launch build of many small targets and the one-launch build of a single one, forced through each path of the
    small form (wave lists that overflow, LDS passes of 512 points, the general finish only): the same grids, bit for bit,
    for clouds of 6 to 49 152 points, crowded ones included, dense and with NaN / inf (tools/probes/pairs_grids_check.py:
    the switches are read once per process)."""
    import sys
    out = str(tmp_path / "grids.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "probes", "pairs_grids_check.py"), out], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-1500:]
    z = np.load(out)
    for form in ("dense", "nonfinite"):
        for c in range(int(z["n_clouds"])):
            a, b = ({k: z["%s%d_%s_%s" % (form, c, who, k)] for k in ("idx", "n", "mean", "cov", "icov", "evals", "min_b", "max_b", "div_b", "n_valid")}
                    for who in ("pairs", "single"))
            grids_equal(a, b)


@pytest.mark.parametrize("method", ["DIRECT1", "DIRECT7", "DIRECT26", "KDTREE"])
def test_each_pair_matches_a_single_registration(mods, pair, method):
    ndt, po, clouds = mods
    t, s = pair
    m = getattr(po, method)
    cl, pairs = ragged_clouds(clouds, t, s)
    guesses = [np.eye(4, dtype=np.float32) if k % 3 else clouds.make_T([0.05, 0, 0], [0, 0, 0.002]).astype(np.float32)
               for k in range(len(pairs))]
    g = handle(ndt, m)
    res = g.alignPairs(cl, pairs, guesses)
    ref = handle(ndt, m)
    regular = {0, 1, 2, 3, 4, 5}  # the well-posed pairs: batch tolerances; the rest: the ragged batch's
    for k, (a, b) in enumerate(pairs):
        T, it, conv, tp = single(ref, cl[a], cl[b], guesses[k])
        tol = 1e-6 if k in regular else 1e-5
        assert rot_err(res["T"][k], T) < tol and trans_err(res["T"][k], T) < tol, "pair %d" % k
        assert res["iterations"][k] == it and bool(res["converged"][k]) == conv, "pair %d" % k
        p = res["trans_probability"][k]
        assert (np.isnan(p) and np.isnan(tp)) or abs(p - tp) <= 1e-6 * max(abs(tp), 1e-300), "pair %d" % k  # (no source point: 0 / 0)
    for k in (0, 3, 4):  # against the live oracle (the bundled pair, the same far from the origin, the 60 k-point target)
        a, b = pairs[k]
        o = po.OracleNDT(trans_eps=0.01, max_iter=40, num_threads=8, search_method=m)
        o.set_target(cl[a])
        o.set_source(cl[b])
        ro = o.align(guesses[k])
        assert rot_err(res["T"][k], ro["T"]) < ROT_TOL and trans_err(res["T"][k], ro["T"]) < TRANS_TOL, "pair %d" % k


def test_pairs_are_independent_bit_for_bit(mods, pair):
    ndt, po, clouds = mods
    t, s = pair
    cl, pairs = ragged_clouds(clouds, t, s)
    g = handle(ndt)
    g.setBatchGroups(1)
    one = g.alignPairs(cl, pairs)
    g.setBatchGroups(3)
    three = g.alignPairs(cl, pairs)
    assert same(one, three)
    g.setBatchGroups(0)
    rev = g.alignPairs(cl, pairs[::-1])
    assert same(one, {k: v[::-1] for k, v in rev.items()})
    sub = [1, 4, 5]
    part = g.alignPairs(cl, [pairs[k] for k in sub])
    assert same(part, {k: v[sub] for k, v in one.items()})
    # the same data as resident clouds (every one of them, the empty one included)
    dcs = [g.uploadCloud(c if len(c) else np.zeros((0, 3), np.float32)) for c in cl]
    res_c = g.alignPairs(dcs, pairs)
    assert same(one, res_c)
    for d in dcs:
        d.release()


def test_pairs_on_one_target_equal_the_batch(mods, pair):
    ndt, po, clouds = mods
    t, s = pair
    rng = np.random.default_rng(4)
    scans = [clouds.apply_T(np.linalg.inv(clouds.random_T(rng, 0.2, 0.5)), s[k::5].copy()) for k in range(5)]
    g = handle(ndt)
    g.setInputTarget(t)
    batch = g.alignBatch(scans)
    res = g.alignPairs([t] + scans, [(0, k + 1) for k in range(5)])
    for k in range(5):
        assert rot_err(res["T"][k], batch["T"][k]) < 1e-6 and trans_err(res["T"][k], batch["T"][k]) < 1e-6
    assert np.array_equal(res["iterations"], batch["iterations"]) and np.array_equal(res["converged"], batch["converged"])


def test_pairs_leave_the_handle_state_alone(mods, pair):
    ndt, po, clouds = mods
    t, s = pair
    cl, pairs = ragged_clouds(clouds, t, s)
    g = handle(ndt)
    g.setInputTarget(t)
    g.setInputSource(cl[1])
    g.align()
    before = (g.getFinalTransformation(), g.getFinalNumIteration(), g.hasConverged(), g.getTransformationProbability())
    grid_before = g.grid()
    g.alignPairs(cl, pairs)
    assert np.array_equal(g.getFinalTransformation(), before[0]) and g.getFinalNumIteration() == before[1]
    grids_equal(g.grid(), grid_before)
    g.align()
    after = (g.getFinalTransformation(), g.getFinalNumIteration(), g.hasConverged(), g.getTransformationProbability())
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]


def small_scene(clouds):
    """four clouds of ~2 000 points (surfaces over 20 m, four boxes each so that a hundred voxels hold six points: the
    one-launch form's range, so k1_small_multi carries the pairs grids) that share no point, and a source for the first"""
    A, B, C, D = (clouds.target_surfaces(2000 + 37 * k, seed=400 + k, extent=20.0, n_boxes=4)[:, :3].astype(np.float32) for k in range(4))
    S = clouds.source_from_target(A, 700, T_gt=clouds.make_T([0.2, -0.1, 0.02], np.deg2rad([0.2, -0.3, 0.8])), seed=411)[:, :3].astype(np.float32)
    return A, B, C, D, S


def own_registration(g):
    g.align()
    return (g.getFinalTransformation(), g.getFinalNumIteration(), g.hasConverged(), g.getTransformationProbability(),
            g.getFitnessScore())


def same_registration(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


GRID_FIELDS = ("idx", "n", "mean", "cov", "icov", "evals", "min_b", "max_b", "div_b", "n_valid")


def test_pairs_call_and_its_inspection_leave_the_handles_own_target_alone(mods):
    """The pairs call grids other clouds and ndt_pairs_grid_* look at those grids, all with the handle's stream and scratch:
    the handle's own target, its grid and what it registers against it stay what they were, bit for bit."""
    ndt, po, clouds = mods
    A, B, C, D, S = small_scene(clouds)
    g = handle(ndt)
    g.setInputTarget(A)
    g.setInputSource(S)
    grid_before = g.grid()
    before = own_registration(g)
    assert before[2] and len(grid_before["idx"]) > 50 and grid_before["n_valid"] > 20
    cl, pairs = [B, C, D], [(0, 1), (1, 2), (2, 0), (0, 2)]
    g.alignPairs(cl, pairs)
    ref = handle(ndt)
    for c in range(3):  # every cloud is a target: the three inspection entries for each
        got = g.pairsGrid(c)
        ref.setInputTarget(cl[c])
        grids_equal(got, ref.grid())
        assert len(got["idx"]) > 50
        now = g.grid()  # ... and the handle's own grid after each of them
        for k in GRID_FIELDS:
            assert np.array_equal(now[k], grid_before[k]), (c, k)
    assert same_registration(own_registration(g), before)


def test_pairs_call_that_fails_in_its_grid_builds_leaves_nothing_behind(mods):
    """Three targets, the second one two points 3 km apart on every axis: 3001^3 = 2.7e10 cells at resolution 1.0, beyond the
    reference's int indices (voxel_grid_covariance_omp_impl.hpp:75-84) -- an ordinary error return from the middle of the
    grid builds.  The handle's own target and registration are untouched, and no pairs grid is left: the call clears
    them before it builds, so every ndt_pairs_grid_size answers NDT_ERR_NO_INPUT (as before this call took the clouds'
    grids out of the handle's fields)."""
    from toyslam_amd._lib import NdtError, NDT_ERR_GRID_OVERFLOW, NDT_ERR_NO_INPUT
    ndt, po, clouds = mods
    A, B, C, D, S = small_scene(clouds)
    assert 3001 ** 3 > 2 ** 31 - 1
    wide = np.array([[-1500.0, -1500.0, -1500.0], [1500.0, 1500.0, 1500.0]], dtype=np.float32)
    g = handle(ndt)
    g.setInputTarget(A)
    g.setInputSource(S)
    grid_before = g.grid()
    before = own_registration(g)
    g.alignPairs([B, C], [(0, 1)])  # (pairs grids of an earlier call: gone after the failed one)
    assert len(g.pairsGrid(0)["idx"]) > 50
    cl = [B, wide, D, C]
    with pytest.raises(NdtError) as e:
        g.alignPairs(cl, [(0, 3), (1, 3), (2, 3)])
    assert e.value.status == NDT_ERR_GRID_OVERFLOW and "overflow" in str(e.value)
    for c in range(len(cl)):
        nl, nv = ndt.C.c_size_t(0), ndt.C.c_size_t(0)
        assert g._L.ndt_pairs_grid_size(g._h, c, ndt.C.byref(nl), ndt.C.byref(nv)) == NDT_ERR_NO_INPUT, c
    now = g.grid()
    for k in GRID_FIELDS:
        assert np.array_equal(now[k], grid_before[k]), k
    assert same_registration(own_registration(g), before)
    # and the handle goes on: the same call without the wide cloud
    res = g.alignPairs([B, D, C], [(0, 2), (1, 2)])
    assert res["T"].shape == (2, 4, 4) and len(g.pairsGrid(1)["idx"]) > 50


def sequence(clouds, ndt, tmp_path, n=6):
    rng = np.random.default_rng(19)
    world = clouds.target_surfaces(60000, seed=77, extent=60.0)[:, :3].astype(np.float32)
    pose = np.eye(4)
    scans = []
    for k in range(n):
        if k:
            pose = pose @ clouds.make_T(rng.uniform(-0.4, 0.4, 3) * [1, 1, 0.05], np.deg2rad(rng.uniform(-1.5, 1.5, 3) * [0.2, 0.2, 1]))
        pick = world[rng.choice(len(world), 30000, replace=False)]
        scans.append((clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32))
    d = tmp_path / "pcd"
    d.mkdir()
    for k, sc in enumerate(scans, 1):
        ndt.pcd_write_xyz(str(d / ("cloud_%d.pcd" % k)), sc)
    return scans, d


def build_app(tmp_path, name):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "toyslam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "apps", name + ".cpp"),
                           "-o", exe, "-L" + libdir, "-lndt_mi355", "-Wl,-rpath," + libdir])
    return exe


def matrices(out, tag):
    lines = out.splitlines()
    return [np.array([[float(x) for x in lines[i + 1 + r].split()] for r in range(4)]) for i, ln in enumerate(lines) if ln.startswith(tag)]


def test_pair_sequence_app_follows_the_node(mods, tmp_path):
    """apps/pair_sequence.cpp -- ndt_omp_node's loop as one ndt_align_pairs_clouds call -- against the chain built from the
    oracle's pieces and against apps/map_sequence's registrations of the same consecutive pairs."""
    ndt, po, clouds = mods
    scans, d = sequence(clouds, ndt, tmp_path)
    out = subprocess.check_output([build_app(tmp_path, "pair_sequence"), str(d)], text=True)
    step = matrices(out, "Transform ")
    chain = matrices(out, "TransformSum")
    assert len(step) == 5 and len(chain) == 5 and "pairs 5 (not converged 0)" in out
    filt = [po.voxel_grid_filter(sc, 0.5)[0] for sc in scans]
    glob = None
    for k in range(1, 6):
        o = po.OracleNDT(resolution=1.0, step_size=0.1, trans_eps=0.01, max_iter=64, num_threads=8)
        o.set_target(filt[k - 1])
        o.set_source(filt[k])
        r = o.align()
        assert r["converged"]
        glob = r["T"] if glob is None else ndt.host_chain_pose(glob, r["T"])
        assert rot_err(step[k - 1], r["T"]) < 2e-4 and trans_err(step[k - 1], r["T"]) < 2e-3, k
        assert rot_err(chain[k - 1], glob) < 2e-4 and trans_err(chain[k - 1], glob) < 2e-3, k
    # map_sequence, node mode: the same registrations one pair at a time (its trajectory is the chain of them)
    out_m = subprocess.check_output([build_app(tmp_path, "map_sequence"), str(d), "0.5", "-", "node"], text=True)
    traj = matrices(out_m, "trajectory[")
    assert len(traj) == 5
    for k in range(5):
        assert rot_err(chain[k], traj[k]) < 1e-5 and trans_err(chain[k], traj[k]) < 1e-5, k
