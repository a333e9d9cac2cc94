"""GPU: ndt_pairs_fitness_scores / ndt_batch_fitness_scores* -- getFitnessScore of every member of a pairs call or of a
batch, all in one launch.  Each value must be the bits ndt_get_fitness_score gives on a handle holding that target and
source after an align ending at that transform, whatever the company, order, grouping or launch split."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_pairs import build_app, handle, ragged_clouds, sequence, single
from test_gpu_parity import brute_force_fitness

pytestmark = pytest.mark.gpu

DBL_MAX = np.finfo(np.float64).max
RANGES = (DBL_MAX, 0.05, 1e-12)


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import clouds, ndt
    return ndt, clouds


def with_nans(cl):
    """every non-empty cloud gets a few NaN / inf points (is_dense = False)"""
    out = []
    for k, c in enumerate(cl):
        c = c.copy()
        if len(c) > 20:
            c[3::97] = np.nan
            c[5::193, 1] = np.inf
        out.append(c)
    return out


def singles(ndt, cl, pairs, ranges=RANGES):
    """each pair registered on a handle of its own: its final transformation T_k and f[r][k] = ndt_get_fitness_score(r)"""
    f = {r: np.zeros(len(pairs)) for r in ranges}
    Ts = []
    for k, (a, b) in enumerate(pairs):
        g = handle(ndt)
        Ts.append(single(g, cl[a], cl[b], is_dense=False)[0])
        for r in ranges:
            f[r][k] = g.getFitnessScore(r)
    return Ts, f


def se3_f32(T, xyz):
    """[PCL] Transformer<float>::se3 in numpy f32, every product and sum rounded on its own: x*r0 + (y*r1 + (z*r2 + t))"""
    f = np.float32
    T = np.asarray(T, dtype=f)
    x, y, z = (xyz[:, i].astype(f) for i in range(3))
    return np.stack([x * T[i, 0] + (y * T[i, 1] + (z * T[i, 2] + T[i, 3])) for i in range(3)], axis=1).astype(f)


def test_pairs_fitness_equals_single_handles_bit_for_bit(mods, pair):
    ndt, clouds = mods
    t, s = pair
    cl, pairs = ragged_clouds(clouds, t, s)
    cl = with_nans(cl)
    Ts, ref = singles(ndt, cl, pairs)
    g = handle(ndt)
    g.alignPairs(cl, pairs, is_dense=False)
    for r in RANGES:
        got = g.pairsFitness(Ts, max_range=r)
        assert got.shape == (len(pairs),)
        assert np.array_equal(got, ref[r]), (r, got, ref[r])
    # the empty source, the target without a valid voxel: nothing qualifies
    assert ref[DBL_MAX][pairs.index((10, 1))] == DBL_MAX and ref[DBL_MAX][pairs.index((0, 10))] == DBL_MAX
    # NULL transforms = the call's own results (a pair registered in the call ends where it does alone)
    res = g.alignPairs(cl, pairs, is_dense=False)
    assert np.array_equal(g.pairsFitness(None), g.pairsFitness(list(res["T"])))
    assert np.array_equal(g.pairsFitness(None), ref[DBL_MAX])
    # a NaN transform: no moved point is finite
    bad = [T.copy() for T in Ts]
    bad[2][0, 3] = np.nan
    got = g.pairsFitness(bad)
    assert got[2] == DBL_MAX and np.array_equal(np.delete(got, 2), np.delete(ref[DBL_MAX], 2))


def test_pairs_fitness_agrees_with_brute_force(mods, pair):
    ndt, clouds = mods
    t, s = pair
    rng = np.random.default_rng(8)
    tg = t[rng.choice(len(t), 5000, replace=False)]
    srcs = [clouds.apply_T(np.linalg.inv(clouds.random_T(rng, 0.3, 1.0)), s[rng.choice(len(s), 3000, replace=False)])
            for _ in range(3)]
    cl = [tg] + srcs
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2)]
    g = handle(ndt)
    res = g.alignPairs(cl, pairs)
    for r in (DBL_MAX, 0.05):
        got = g.pairsFitness(max_range=r)
        for k, (a, b) in enumerate(pairs):
            want = brute_force_fitness(cl[a], se3_f32(res["T"][k], cl[b]), r)
            assert got[k] == pytest.approx(want, rel=1e-12), (r, k)


def test_pairs_fitness_is_independent_bit_for_bit(mods, pair, tmp_path):
    ndt, clouds = mods
    t, s = pair
    cl, pairs = ragged_clouds(clouds, t, s)
    g = handle(ndt)
    res = g.alignPairs(cl, pairs)
    Ts = list(res["T"])
    one = g.pairsFitness(Ts)
    # reordered and duplicated
    order = [5, 5, 0, 11, 3, 2, 2, 7, 1, 4, 6, 8, 9, 10]
    g.alignPairs(cl, [pairs[k] for k in order])
    assert np.array_equal(g.pairsFitness([Ts[k] for k in order]), one[order])
    # alone
    for k in (0, 4, 5, 11):
        g.alignPairs(cl, [pairs[k]])
        assert np.array_equal(g.pairsFitness([Ts[k]]), one[[k]])
    # grouping of the pairs call
    for groups in (1, 4):
        g2 = handle(ndt)
        g2.setBatchGroups(groups)
        g2.alignPairs(cl, pairs)
        assert np.array_equal(g2.pairsFitness(Ts), one), groups
    # resident clouds (ndt_cloud), the empty one included
    dcs = [g.uploadCloud(c if len(c) else np.zeros((0, 3), np.float32)) for c in cl]
    g.alignPairs(dcs, pairs)
    assert np.array_equal(g.pairsFitness(Ts), one)
    for d in dcs:
        d.release()
    # launches split into chunks of a few blocks: a child process with NDT_FITNESS_CHUNK_BLOCKS=1000 (a member is never
    # split, so a launch holds one member of more blocks -- at most 2048 -- on its own)
    tmp = str(tmp_path / "chunks.npz")
    np.savez(tmp, *cl, pairs=np.array(pairs), Ts=np.array(Ts))
    code = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from toyslam_amd import ndt
d = np.load(sys.argv[2])
cl = [d["arr_%d" % k] for k in range(len(d.files) - 2)]
g = ndt.NormalDistributionsTransform()
g.setTransformationEpsilon(0.01); g.setMaximumIterations(40)
g.alignPairs(cl, [tuple(p) for p in d["pairs"]])
np.save(sys.argv[2] + ".out.npy", g.pairsFitness(list(d["Ts"])))
np.save(sys.argv[2] + ".launches.npy", np.array(g.fitnessLaunches()))
"""
    env = dict(os.environ, NDT_FITNESS_CHUNK_BLOCKS="1000")
    subprocess.check_call([sys.executable, "-c", code, ROOT, tmp], env=env, timeout=300)
    assert np.array_equal(np.load(tmp + ".out.npy"), one)
    launches, blocks = np.load(tmp + ".launches.npy")
    assert launches >= 3 and blocks <= 2048, (launches, blocks)


def test_pairs_fitness_outlives_the_handle_that_made_the_clouds(mods, pair):
    """resident clouds of another handle, kept by the pairs call: scored after that handle (and its stream) is gone"""
    import gc
    ndt, clouds = mods
    t, s = pair
    cl, pairs = ragged_clouds(clouds, t, s)
    maker = handle(ndt)
    dcs = [maker.uploadCloud(c if len(c) else np.zeros((0, 3), np.float32)) for c in cl]
    g = handle(ndt)
    g.alignPairs(dcs, pairs)
    before = g.pairsFitness()
    for d in dcs:
        d.release()
    del dcs, d, maker
    gc.collect()
    assert np.array_equal(g.pairsFitness(), before)


def test_batch_fitness_equals_single_handles_bit_for_bit(mods, pair):
    ndt, clouds = mods
    t, s = pair
    rng = np.random.default_rng(12)
    scans = [clouds.apply_T(np.linalg.inv(clouds.random_T(rng, 0.2, 0.5)), s[k % 7::7].copy()) for k in range(64)]
    Ts = [clouds.random_T(rng, 0.05, 0.2).astype(np.float32) for _ in range(64)]
    ref = {}
    for k in range(0, 64, 9):  # (an align from Ts[k]: the transform it ends at is the one to compare at)
        h = handle(ndt, iters=2)
        Ts[k] = single(h, t, scans[k], guess=Ts[k])[0]
        ref[k] = h.getFitnessScore()
    g = handle(ndt)
    g.setInputTarget(t)
    f = g.batchFitness(scans, transforms=Ts)
    for k in ref:
        assert f[k] == ref[k], k
    # the device form over the same records (a resident cloud of the library: float4 records in HBM)
    dc = g.uploadCloud(np.concatenate(scans))
    offsets = np.r_[0, np.cumsum([len(sc) for sc in scans])]
    fd = g.batchFitness(device_ptr=dc.data_ptr(), offsets=offsets, stride_bytes=16, transforms=Ts)
    assert np.array_equal(f, fd)
    dc.release()
    # a member's value does not depend on its company
    assert np.array_equal(g.batchFitness(scans[:5], transforms=Ts[:5], max_range=0.05),
                          g.batchFitness(scans, transforms=Ts, max_range=0.05)[:5])


def test_batch_fitness_many_large_scans(mods):
    ndt, clouds = mods
    rng = np.random.default_rng(3)
    t = clouds.target_surfaces(100000, seed=9, extent=40.0)[:, :3].astype(np.float32)
    base = clouds.target_surfaces(100000, seed=10, extent=40.0)[:, :3].astype(np.float32)
    Ts = [clouds.random_T(rng, 0.05, 0.2).astype(np.float32) for _ in range(512)]
    h = handle(ndt, iters=2)
    Ts[77] = single(h, t, base, guess=Ts[77])[0]
    g = handle(ndt)
    g.setInputTarget(t)
    # 512 x 100 k points: 512 x 2048 blocks, several launches of the default chunk
    f = g.batchFitness([base] * 512, transforms=Ts)
    assert f.shape == (512,) and np.isfinite(f).all() and (f > 0).all()
    # 1 048 576 blocks in launches of at most 262 144: the partial rows held at once stay within the bound (64 MB)
    launches, blocks = g.fitnessLaunches()
    assert launches == 4 and blocks <= 262144, (launches, blocks)
    assert f[77] == h.getFitnessScore()


def test_fitness_calls_leave_the_handle_state_alone(mods, pair):
    ndt, clouds = mods
    t, s = pair
    cl, pairs = ragged_clouds(clouds, t, s)
    g = handle(ndt)
    g.setInputTarget(t)
    g.setInputSource(cl[1])
    g.align()
    before = (g.getFinalTransformation(), g.getFinalNumIteration(), g.hasConverged(), g.getFitnessScore())
    grid_before = g.grid()
    res = g.alignPairs(cl, pairs)
    g.pairsFitness()
    g.batchFitness([cl[1], cl[2]], transforms=[np.eye(4, dtype=np.float32)] * 2)
    after = (g.getFinalTransformation(), g.getFinalNumIteration(), g.hasConverged(), g.getFitnessScore())
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    grid_after = g.grid()
    for k in grid_before:
        assert np.array_equal(grid_before[k], grid_after[k]), k
    # a second pairs call replaces the retained pairs; a call with no pair clears them
    first = g.pairsFitness(list(res["T"]))
    g.alignPairs(cl, pairs[:3])
    assert np.array_equal(g.pairsFitness(list(res["T"][:3])), first[:3])
    with pytest.raises(ValueError):
        g.pairsFitness(list(res["T"]))
    from toyslam_amd import _lib
    g.alignPairs(cl, [])
    with pytest.raises(_lib.NdtError) as e:
        g.pairsFitness()
    assert e.value.status == _lib.NDT_ERR_NO_INPUT


def test_pair_sequence_app_prints_the_pairs_fitness(mods, tmp_path):
    ndt, clouds = mods
    scans, d = sequence(clouds, ndt, tmp_path)
    exe = build_app(tmp_path, "pair_sequence")
    plain = subprocess.check_output([exe, str(d)], text=True)
    out = subprocess.check_output([exe, str(d), "--fitness"], text=True)
    vals = [float(ln.split(":")[1]) for ln in out.splitlines() if ln.startswith("fitness ")]
    assert len(vals) == 5 and all(np.isfinite(vals))
    assert "fitness" not in plain
    strip = lambda o: [ln for ln in o.splitlines() if not ln.startswith(("fitness ", "time:"))]
    assert strip(plain) == strip(out)
    # the same pairs through Python: the app's filter and settings, one pairs call
    g = ndt.NormalDistributionsTransform()
    g.setResolution(1.0)
    g.setStepSize(0.1)
    g.setTransformationEpsilon(0.01)
    g.setMaximumIterations(64)
    g.setNeighborhoodSearchMethod(ndt.DIRECT7)
    filt = [g.voxelGridFilterCloud(sc, 0.5)[0] for sc in scans]
    g.alignPairs(filt)
    want = g.pairsFitness()
    assert np.allclose(want, vals, rtol=1e-12, atol=0)  # (the app reads the scans back from PCD files: 16-byte records)
    for c in filt:
        c.release()
