"""GPU: ndt_target_accumulate_clear_rays* / _ray_counts against the restatement of the definition (tests/ray_cases.py).

Counts: cells, miss counts and hit flags of every voxel, and the diagnostic's cast / skipped / visited totals, are EXACT:
integer counts of rays whose clearance (ray_cases) is at least 1e-6 m, six orders above the rounding differences a device
could have in one f64 division.  The posed points come from the oracle's transform (what the accumulate tests pose with),
the voxels' cells from numpy f32 floor(p * inv_leaf), never from the library.
Removal: the removed set is the reference's; afterwards the handle is compared, as a crop is (test_gpu_target_crop), with
test_gpu_target_accumulate's Ref of the filtered concatenation -- a second GPU handle bit for bit and the live oracle.
Sizes: 1 ray, either side of a wave and of a block, one point either side of every step of ndt_host_ray_plan up to and
including its block cap (prefixes of one cloud of short rays, the reference walked once), the strided regime with
NDT_RAYS_MAX_BLOCKS=3 in a child (tests/rays_child.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ray_cases as rc
from conftest import rot_err, trans_err
from test_gpu_map_batch import moved_keeping_non_finite
from test_gpu_pairs import build_app, matrices, sequence
from test_gpu_target_accumulate import Ref, handle, observe, same_observation
from test_gpu_target_crop import History, cells_of, check_empty, crop_both, slab

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from oracle import pyoracle as po
    from toyslam_amd import _lib, clouds, ndt
    return ndt, po, clouds, _lib


def spec_of(res, min_rays=2, margin=None, min_range=0.0, max_range=None):
    """the wrapper's defaults as numbers"""
    return dict(min_rays=min_rays, margin=float(np.float32(res)) if margin is None else margin, min_range=min_range,
                max_range=float(np.float32(65536.0) * np.float32(res)) if max_range is None else max_range)


def posed_and_origins(po, scans, poses, origins):
    poses = [EYE] * len(scans) if poses is None else poses
    posed = [moved_keeping_non_finite(po, np.asarray(s, np.float32), np.asarray(T, np.float32)) for s, T in zip(scans, poses)]
    org = [np.asarray(T, np.float32)[:3, 3] for T in poses] if origins is None else origins
    return posed, org


def clear_scan(po, scan, pose, origin, res, sp):
    """the scan without the rows whose rays come too close to a tie (at most 1 %)"""
    posed, org = posed_and_origins(po, [scan], None if pose is None else [pose], None if origin is None else [origin])
    return scan[rc.clear_mask(posed[0], org[0], res, sp["margin"], sp["min_range"], sp["max_range"])]


def reference(po, hist, scans, poses, origins, res, sp):
    posed, org = posed_and_origins(po, scans, poses, origins)
    return rc.call_counts(cells_of(hist.cat(), res), list(zip(posed, org)), res, sp["margin"], sp["min_range"], sp["max_range"], min_clearance=rc.CLEAR)


def check_counts(mods, g, hist, scans, poses=None, origins=None, **kw):
    """targetRayCounts of one call against the reference; the target is not written"""
    ndt, po, clouds, _ = mods
    res = hist.res
    sp = spec_of(res, **kw)
    ref = reference(po, hist, scans, poses, origins, res, sp)
    ups = [g.uploadCloud(s) for s in scans]
    before = g.targetAccumulateExport()
    got = g.targetRayCounts(ups, poses, origins, **kw)
    d = g.targetClearRaysDiag()
    for u in ups:
        u.release()
    assert np.array_equal(got["cells"], ref["cells"])
    assert np.array_equal(got["miss"], ref["miss"]), (np.nonzero(got["miss"] != ref["miss"])[0][:8], got["miss"].sum(), ref["miss"].sum())
    assert np.array_equal(got["hit"], ref["hit"])
    assert (d["rays_cast"], d["rays_skipped"], d["cells_visited"]) == (ref["cast"], ref["skipped"], ref["visited"])
    gone = (ref["miss"] >= sp["min_rays"]) & ~ref["hit"]
    assert d["touched_voxels"] == (ref["miss"] >= 1).sum() and d["removed_voxels"] == gone.sum() and d["kept_voxels"] == (~gone).sum()
    assert d["launches"] == (1 if sum(len(s) for s in scans) else 0) and not d["relinked"]
    assert g.targetAccumulateExport() == before
    return ref, d


def clear_both(mods, g, hist, scans, poses=None, origins=None, **kw):
    """one clearing on the handle and on the history; statistics, diagnostics and launches"""
    ndt, po, clouds, _ = mods
    res = hist.res
    sp = spec_of(res, **kw)
    ref = reference(po, hist, scans, poses, origins, res, sp)
    gone = rc.removed_cells(ref, sp["min_rays"])
    before = g.targetAccumulated()
    n_before = hist.voxels()
    gone_keys = rc.pack(gone)
    hist.parts = [p[~np.isin(rc.pack(cells_of(p, res)), gone_keys)] for p in hist.parts]
    ups = [g.uploadCloud(s) for s in scans]
    st = g.targetClearRays(ups[0] if len(ups) == 1 else ups, None if poses is None else (poses[0] if len(ups) == 1 else poses),
                           None if origins is None else (origins[0] if len(ups) == 1 else origins), **kw)
    d = g.targetClearRaysDiag()
    for u in ups:
        u.release()
    kept = n_before - len(gone)
    assert hist.voxels() == kept
    if len(gone):
        assert st == dict(points=len(hist.cat()), voxels=kept, updates=before["updates"])
    assert (d["rays_cast"], d["rays_skipped"], d["cells_visited"]) == (ref["cast"], ref["skipped"], ref["visited"])
    assert d["touched_voxels"] == (ref["miss"] >= 1).sum()
    assert d["removed_voxels"] == len(gone) and d["kept_voxels"] == kept and d["kept_points"] == len(hist.cat())
    assert d["relinked"] == (0 < kept < n_before)
    assert d["launches"] == (6 if d["relinked"] else 3 if n_before else 1)      # what include/ndt_mi355.h states
    return ref, gone, d


def block_map(rng, res, lo, hi, n, offset=(0, 0, 0)):
    """n points scattered over [lo, hi) (+ offset): a map of a few hundred to a few thousand voxels"""
    return (slab(rng, lo, hi, n) + np.asarray(offset, np.float32)).astype(np.float32)


def scan_into(rng, res, lo, hi, n, offset=(0, 0, 0)):
    return rc.off_faces(rng, slab(rng, lo, hi, n).astype(np.float64) + np.asarray(offset, np.float64), float(np.float32(res)))


# ---- 1: counts at the wave and block sizes, two leaves, the three table forms
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2000])
@pytest.mark.parametrize("res", [1.0, 0.7])
def test_counts(mods, n, res):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(n)
    voxel_index = n % 3
    g = handle(ndt, res=res, voxel_index=voxel_index)
    hist = History(ndt, res)
    cloud = block_map(rng, res, [-14, -14, -3], [14, 14, 3], 2500)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    assert 300 < hist.voxels() < 5000
    origin = rc.off_faces(rng, [0.3, -0.4, 0.2], float(np.float32(res)))
    sp = spec_of(res)
    scan = clear_scan(po, scan_into(rng, res, [-13, -13, -2.5], [13, 13, 2.5], n), None, origin, res, sp)
    ref, d = check_counts(mods, g, hist, [scan], None, [origin])
    if n >= 63:
        assert ref["miss"].max() >= 2 and ref["hit"].any() and d["cells_visited"] > 5 * n
    Ref(mods, cloud, res=res, voxel_index=voxel_index).check(g)        # ... and the target is what it was


# ---- 2: one point either side of every step of the plan, up to and including the block cap
STEP_CASES = 16


@pytest.fixture(scope="module")
def short_rays(mods):
    """256 * 1024 + 1 short rays around one origin into a block of 9^3 voxels, their walks computed once: per ray its cells'
    rows in the voxel list, so that the counts of a prefix are sums over a prefix"""
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(2024)
    blocks, _ = ndt.host_ray_plan(2 ** 30)
    n = 256 * blocks + 1
    origin = np.array([0.37, 0.52, 0.44], np.float32)
    pts = rc.off_faces(rng, rng.uniform(-3.4, 3.4, (n + n // 20, 3)), 1.0)
    pts = pts[np.linalg.norm(pts.astype(np.float64) - origin, axis=1) > 0.6]       # (margin 0.5: every ray is cast)
    pts = rc.clear_points(pts, origin, 1.0, margin=0.5)[:n]
    assert len(pts) == n
    grid = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    cloud = (grid + 0.5).astype(np.float32)
    keys = rc.pack(grid)
    order = np.argsort(keys)
    vox, keys = grid[order], keys[order]
    w = rc.walk_many(origin, pts, 1.0, 0.5)
    assert w["cast"].all() and (w["clearance"] >= rc.CLEAR).all()
    by_ray = np.argsort(w["ray"], kind="stable")
    rows = np.searchsorted(keys, rc.pack(w["cells"][by_ray]))           # (every visited cell lies in the block)
    assert (keys[rows] == rc.pack(w["cells"][by_ray])).all()
    first = np.concatenate([[0], np.cumsum(w["n"])])
    hit_rows = np.searchsorted(keys, rc.pack(rc.build_cells(pts, 1.0)[0]))
    return dict(origin=origin, pts=pts, cloud=cloud, vox=vox, rows=rows, first=first, hit_rows=hit_rows, blocks=blocks)


@pytest.mark.parametrize("part", range(STEP_CASES))
def test_every_step_of_the_plan(mods, short_rays, part):
    ndt, po, clouds, _ = mods
    s = short_rays
    g = handle(ndt)
    g.targetAccumulate(s["cloud"])
    V = len(s["vox"])
    per = s["blocks"] // STEP_CASES
    sizes = [256 * k + e for k in range(part * per + 1, (part + 1) * per + 1) for e in (0, 1)]
    miss, hits, done = np.zeros(V, np.int64), np.zeros(V, np.int64), 0
    for n in sizes:
        miss += np.bincount(s["rows"][s["first"][done]:s["first"][n]], minlength=V)
        hits += np.bincount(s["hit_rows"][done:n], minlength=V)
        done = n
        up = g.uploadCloud(s["pts"][:n])
        got = g.targetRayCounts(up, None, s["origin"], margin=0.5)
        d = g.targetClearRaysDiag()
        up.release()
        blocks, passes = ndt.host_ray_plan(n)
        assert blocks == min(-(-n // 256), s["blocks"]) and passes == (2 if n > 256 * s["blocks"] else 1)
        assert np.array_equal(got["cells"], s["vox"]) and np.array_equal(got["miss"], miss) and np.array_equal(got["hit"], hits > 0), n
        assert (d["rays_cast"], d["rays_skipped"], d["cells_visited"], d["launches"]) == (n, 0, s["first"][n], 1), n


def test_the_strided_regime_in_a_child(mods):
    """NDT_RAYS_MAX_BLOCKS=3: three blocks walk a few thousand rays in several passes (tests/rays_child.py)"""
    env = dict(os.environ, NDT_RAYS_MAX_BLOCKS="3")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rays_child.py")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["cases"] >= 4 and res["max_blocks_seen"] == 3 and res["max_passes"] >= 5, res


# ---- 3: far from the origin; through the box; every kind of skipped ray; non-finite rows; axis-parallel rays
@pytest.mark.parametrize("res", [1.0, 0.7])
def test_a_map_100_km_from_the_origin(mods, res):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(100)
    off = (1e5, -1e5, 30.0)
    g = handle(ndt, res=res)
    hist = History(ndt, res)
    cloud = block_map(rng, res, [-12, -12, -2], [12, 12, 2], 2500, off)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    origin = rc.off_faces(rng, np.array(off) + [0.3, 0.2, 0.1], float(np.float32(res)))
    sp = spec_of(res)
    scan = clear_scan(po, scan_into(rng, res, [-11, -11, -1.8], [11, 11, 1.8], 1500, off), None, origin, res, sp)
    ref, d = check_counts(mods, g, hist, [scan], None, [origin])
    assert ref["miss"].max() >= 2 and d["rays_cast"] > 0.98 * len(scan)    # (a point within the margin of the origin casts no ray)
    clear_both(mods, g, hist, [scan], None, [origin])
    Ref(mods, hist.cat(), scan[::3], res=res).check(g)


def test_rays_that_leave_the_box_on_both_sides(mods):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(8)
    g = handle(ndt)
    hist = History(ndt)
    cloud = block_map(rng, 1.0, [0, 0, 0], [10, 10, 4], 2000)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    origin = np.array([-20.3, 4.4, 1.7], np.float32)                    # outside the box on one side, the points on the other
    sp = spec_of(1.0, margin=0.0)
    scan = clear_scan(po, scan_into(rng, 1.0, [25, -6, -3], [40, 16, 7], 900), None, origin, 1.0, sp)
    ref, d = check_counts(mods, g, hist, [scan], None, [origin], margin=0.0)
    assert not ref["hit"].any() and (ref["miss"] > 0).sum() > 100 and d["cells_visited"] > 40 * len(scan)
    ref, gone, d = clear_both(mods, g, hist, [scan], None, [origin], margin=0.0)
    assert 100 < len(gone) < len(ref["cells"])
    Ref(mods, hist.cat(), cloud[::5]).check(g)


def test_rays_skipped_by_each_rule_and_non_finite_rows(mods):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(12)
    g = handle(ndt)
    hist = History(ndt)
    cloud = block_map(rng, 1.0, [-15, -15, -2], [15, 15, 2], 3000)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    origin = np.array([0.31, 0.22, 0.13], np.float32)
    kw = dict(min_range=4.0, max_range=9.0, margin=5.0)
    sp = spec_of(1.0, **kw)
    pts = scan_into(rng, 1.0, [-14, -14, -1.9], [14, 14, 1.9], 1500)
    pts = np.concatenate([pts, origin[None]])                           # a ray of length 0
    pts[5::37] = np.nan
    pts[11::41, 1] = np.inf
    pts[13::43, 2] = -np.inf
    scan = clear_scan(po, pts, None, origin, 1.0, sp)
    ln = np.linalg.norm(scan.astype(np.float64) - origin, axis=1)
    fin = np.isfinite(scan).all(axis=1)
    assert (ln[fin] < 4).sum() > 20 and (ln[fin] > 9).sum() > 100 and ((ln[fin] >= 4) & (ln[fin] <= 5)).sum() > 10 and (~fin).sum() > 80
    ref, d = check_counts(mods, g, hist, [scan], None, [origin], **kw)
    assert d["rays_cast"] + d["rays_skipped"] == fin.sum()              # non-finite rows are counted nowhere
    assert d["rays_cast"] == ((ln[fin] > 5) & (ln[fin] <= 9)).sum()     # min_range 4 <= margin 5: t_end > 0 decides below
    assert ref["hit"].sum() > 500                                       # the hit set takes every finite point, whatever its range
    kw2 = dict(min_range=6.0, max_range=9.0, margin=5.0)                # ... and min_range above the margin
    scan2 = clear_scan(po, scan, None, origin, 1.0, spec_of(1.0, **kw2))
    ref2, d2 = check_counts(mods, g, hist, [scan2], None, [origin], **kw2)
    ln2 = np.linalg.norm(scan2[np.isfinite(scan2).all(axis=1)].astype(np.float64) - origin, axis=1)
    assert d2["rays_cast"] == ((ln2 >= 6) & (ln2 <= 9)).sum()
    clear_both(mods, g, hist, [scan], None, [origin], **kw)
    Ref(mods, hist.cat(), cloud[::4], is_dense=True).check(g)


def test_axis_parallel_rays(mods):
    """d_k exactly 0 on one or two axes: t_k = +inf there"""
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(21)
    g = handle(ndt, res=0.7)
    hist = History(ndt, 0.7)
    cloud = block_map(rng, 0.7, [-8, -8, -2], [8, 8, 2], 2500)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    origin = np.array([0.2, -0.3, 0.1], np.float32)
    ends = rc.off_faces(rng, rng.uniform(-7.5, 7.5, (600, 3)) * [1, 1, 0.25], float(np.float32(0.7)))
    for k in range(600):
        if k % 3 == 0:
            ends[k, 1:] = origin[1:]                                    # along x
        elif k % 3 == 1:
            ends[k, 2] = origin[2]                                      # in the plane z = const
        else:
            ends[k, 0] = origin[0]
            ends[k, 1] = origin[1]                                      # along z
    scan = clear_scan(po, ends, None, origin, 0.7, spec_of(0.7, margin=0.0))
    ref, d = check_counts(mods, g, hist, [scan], None, [origin], margin=0.0)
    assert d["rays_cast"] == len(scan) and ref["miss"].max() >= 3


# ---- 4: a wall behind a parked car, seen from two poses
def car_scene(clouds, res):
    rng = np.random.default_rng(55)
    ground = np.c_[rng.uniform(0, 30, 9000), rng.uniform(-10, 10, 9000), rng.uniform(0.02, 0.18, 9000)]
    wall = np.c_[rng.uniform(25.05, 25.45, 4000), rng.uniform(-10, 10, 4000), rng.uniform(0.2, 4.0, 4000)]
    car = np.c_[rng.uniform(12.1, 14.9, 1500), rng.uniform(-0.9, 0.9, 1500), rng.uniform(1.05, 1.95, 1500)]
    world = [w.astype(np.float32) for w in (ground, wall, car)]
    poses = [clouds.make_T([0.3, 0.2, 1.5], [0.0, 0.0, 0.02]).astype(np.float32), clouds.make_T([0.4, 3.1, 1.6], [0.0, 0.01, -0.1]).astype(np.float32)]
    leaf = float(np.float32(res))
    later = []
    for k, T in enumerate(poses):   # the later scans: the car has left; the wall and the ground sampled anew, off the cell faces
        again = np.concatenate([np.c_[rng.uniform(0, 30, 5000), rng.uniform(-10, 10, 5000), rng.uniform(0.02, 0.18, 5000)],
                                np.c_[rng.uniform(25.05, 25.45, 5000), rng.uniform(-10, 10, 5000), rng.uniform(0.2, 4.0, 5000)]])
        later.append(clouds.apply_T(np.linalg.inv(T.astype(np.float64)), rc.off_faces(rng, again, leaf).astype(np.float64)).astype(np.float32))
    return world, poses, later


@pytest.mark.parametrize("min_rays,voxel_index", [(1, 0), (2, 1), (2, 2), (None, 0)])
def test_the_parked_car_goes_the_wall_and_the_ground_stay(mods, min_rays, voxel_index):
    ndt, po, clouds, _ = mods
    res = 1.0
    (ground, wall, car), poses, later = car_scene(clouds, res)
    g = handle(ndt, voxel_index=voxel_index)
    hist = History(ndt, res)
    for part in (ground, wall, car):
        g.targetAccumulate(part)
        hist.add(part)
    sp = spec_of(res)
    scans = [clear_scan(po, s, T, None, res, sp) for s, T in zip(later, poses)]
    ref, _ = check_counts(mods, g, hist, scans, poses)
    top = int(ref["miss"][~ref["hit"]].max())
    if min_rays is None:
        min_rays = top + 1                                              # one more than the largest miss count of a voxel that could go
    ref, gone, d = clear_both(mods, g, hist, scans, poses, min_rays=min_rays)
    gone_keys = set(rc.pack(gone).tolist())
    car_keys = set(rc.pack(cells_of(car, res)).tolist())
    wall_keys = set(rc.pack(cells_of(wall, res)).tolist())
    if min_rays > top:
        assert len(gone) == 0 and d["launches"] == 3 and not d["relinked"]
    else:
        assert car_keys <= gone_keys                                    # the car's voxels go
        assert not (wall_keys & gone_keys)                              # the wall, which is hit, stays
        ground_hit = set(rc.pack(ref["cells"][ref["hit"] & (ref["cells"][:, 2] == 0)]).tolist())
        assert len(ground_hit) > 400 and not (ground_hit & gone_keys)   # the ground under grazing rays stays: its cells are in H
        assert (ref["miss"][ref["hit"] & (ref["cells"][:, 2] == 0)] >= min_rays).sum() > 100
    src = np.concatenate([ground[::9], wall[::7]]) + np.float32(0.03)
    got = Ref(mods, hist.cat(), src, voxel_index=voxel_index).check(g)
    if voxel_index == 0 and min_rays == 1:
        g.warmUp(3000)                                                  # leaves a cleared target as it was
        same_observation(ndt, observe(ndt, g, src), got)
    b = handle(ndt, voxel_index=voxel_index)
    b.setInputTarget(hist.cat())
    guess = clouds.make_T([0.1, -0.05, 0.02], [0.0, 0.0, 0.01]).astype(np.float32)
    results = []
    for h in (g, b):
        h.setInputSource(src)
        h.align(guess)
        results.append((h.getFinalTransformation(), h.getFinalNumIteration(), h.stats()["n_evals"], h.hasConverged()))
    assert np.array_equal(results[0][0], results[1][0]) and results[0][1:] == results[1][1:]
    poses_tab = [EYE, guess, results[0][0]]
    assert np.array_equal(g.scorePoses(poses_tab), b.scorePoses(poses_tab))
    # the cleared target's export is, byte for byte, that of a target accumulated from the filtered concatenation
    c = handle(ndt, voxel_index=voxel_index)
    c.targetAccumulate(hist.cat())
    assert g.targetAccumulateExport() == c.targetAccumulateExport()


# ---- 5: many clouds in one call: the misses are summed over the call
def test_many_clouds_sum_their_misses(mods):
    ndt, po, clouds, _ = mods
    res = 1.0
    (ground, wall, car), poses, later = car_scene(clouds, res)
    sp = spec_of(res)
    scans = [clear_scan(po, s[::2], T, None, res, sp) for s, T in zip(later, poses)]
    a, b = handle(ndt), handle(ndt)
    ha, hb = History(ndt, res), History(ndt, res)
    for h, hist in ((a, ha), (b, hb)):
        for part in (ground, wall, car):
            h.targetAccumulate(part)
            hist.add(part)
    both = reference(po, ha, scans, poses, None, res, sp)
    each = [reference(po, ha, [s], [T], None, res, sp) for s, T in zip(scans, poses)]
    assert np.array_equal(both["miss"], each[0]["miss"] + each[1]["miss"]) and np.array_equal(both["hit"], each[0]["hit"] | each[1]["hit"])
    m = int(max(e["miss"][~both["hit"]].max() for e in each)) + 1       # no single scan reaches it ...
    assert ((both["miss"] >= m) & ~both["hit"]).sum() >= 1              # ... the two together do: where the forms differ
    _, gone_a, _ = clear_both(mods, a, ha, scans, poses, min_rays=m)
    assert len(gone_a) >= 1
    n_gone_b = 0
    for s, T in zip(scans, poses):
        _, gone, _ = clear_both(mods, b, hb, [s], [T], min_rays=m)
        n_gone_b += len(gone)
    assert n_gone_b == 0                                                # exactly as the reference says: nothing for the single calls
    src = ground[::9] + np.float32(0.03)
    Ref(mods, ha.cat(), src).check(a)
    Ref(mods, hb.cat(), src).check(b)


# ---- 6: nothing removed; everything removed; after a crop and an import; voxel states
def test_nothing_removed_writes_nothing(mods):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(3)
    g = handle(ndt)
    hist = History(ndt)
    cloud = block_map(rng, 1.0, [-10, -10, -2], [10, 10, 2], 2500)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    src = cloud[::5] + np.float32(0.02)
    before = observe(ndt, g, src)
    blob, stats = g.targetAccumulateExport(), g.targetAccumulated()
    origin = np.array([0.3, 0.3, 0.3], np.float32)
    scan = clear_scan(po, scan_into(rng, 1.0, [-9, -9, -1.8], [9, 9, 1.8], 800), None, origin, 1.0, spec_of(1.0))
    _, gone, d = clear_both(mods, g, hist, [scan], None, [origin], min_rays=10 ** 6)
    assert len(gone) == 0 and d["launches"] == 3 and not d["relinked"] and d["kept_voxels"] == stats["voxels"]
    assert g.targetAccumulateExport() == blob and g.targetAccumulated() == stats
    same_observation(ndt, observe(ndt, g, src), before)
    up = g.uploadCloud(np.zeros((0, 3), np.float32))                    # only empty clouds: nothing happens
    assert g.targetClearRays([up, up]) == stats and g.targetClearRaysDiag() == d
    assert g.targetClearRays([]) == stats
    up.release()


def test_everything_removed_and_a_later_accumulate(mods):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(4)
    g = handle(ndt)
    hist = History(ndt)
    cloud = block_map(rng, 1.0, [2, -3, -1], [8, 3, 1], 1500)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    origin = np.array([-5.2, 0.1, 0.05], np.float32)
    # a fan of rays through the inner part of every voxel's cell, eight per cell, ending far behind the block
    through = np.repeat(np.unique(cells_of(cloud, 1.0), axis=0), 8, axis=0) + rng.uniform(0.2, 0.8, (8 * hist.voxels(), 3))
    far = (origin + (through - origin) * 3.0).astype(np.float32)
    scan = clear_scan(po, far, None, origin, 1.0, spec_of(1.0, margin=0.0))
    ref, gone, d = clear_both(mods, g, hist, [scan], None, [origin], min_rays=1, margin=0.0)
    assert not ref["hit"].any() and hist.voxels() == 0
    d = g.targetClearRaysDiag()
    assert d["kept_voxels"] == 0 and not d["relinked"] and d["launches"] == 3
    check_empty(mods, g)
    _, _, d = clear_both(mods, g, hist, [scan], None, [origin], min_rays=1, margin=0.0)   # a clearing of the empty target
    assert d["launches"] == 1 and d["rays_cast"] == len(scan)
    check_empty(mods, g)
    assert g.targetAccumulate(cloud)["updates"] == 2                   # the removed cells start from empty sums
    hist.add(cloud)
    Ref(mods, cloud, cloud[::4]).check(g)


def test_after_a_crop_and_after_an_import(mods):
    ndt, po, clouds, _ = mods
    res = 1.0
    (ground, wall, car), poses, later = car_scene(clouds, res)
    sp = spec_of(res)
    scans = [clear_scan(po, s, T, None, res, sp) for s, T in zip(later, poses)]
    g = handle(ndt)
    hist = History(ndt, res)
    for part in (ground, wall, car):
        g.targetAccumulate(part)
        hist.add(part)
    # the crop's diagnostics are what they were before its tail was shared
    d = crop_both(g, hist, [-5, -8, -1], [28, 8, 6])
    assert d["launches"] == 5 and d["relinked"] and d["removed_voxels"] > 50 and d["kept_voxels"] == hist.voxels() and d["kept_points"] == len(hist.cat())
    d = crop_both(g, hist, [-5, -8, -1], [28, 8, 6])
    assert d["launches"] == 2 and not d["relinked"] and d["removed_voxels"] == 0
    _, gone, _ = clear_both(mods, g, hist, scans[:1], poses[:1])
    assert len(gone) >= 6                                               # the car at the least
    src = ground[::9] + np.float32(0.03)
    Ref(mods, hist.cat(), src).check(g)
    # a second handle imports the cleared map and is cleared from the other pose; the first continues with points
    b = handle(ndt)
    b.targetAccumulateImport(g.targetAccumulateExport())
    hb = History(ndt, res)
    hb.parts = [p.copy() for p in hist.parts]
    clear_both(mods, b, hb, scans[1:], poses[1:], min_rays=1)
    Ref(mods, hb.cat(), src).check(b)
    g.targetAccumulate(car)                                             # the removed cells receive points again
    hist.add(car)
    Ref(mods, hist.cat(), src).check(g)
    d = crop_both(g, hist, [-100, -100, -100], [100, 100, 100])
    assert d["launches"] == 2


def test_voxel_states_survive(mods):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(7)
    ox, oy = 500000, -500000     # out here a voxel of 3000 collinear points cancels into a negative eigenvalue: rejected

    def in_cell(cell, n, spread=0.8):
        return (np.asarray(cell, np.float32) + 0.1 + spread * rng.random((n, 3))).astype(np.float32)

    def line(cell):
        at = np.array([cell[0] + 0.5, cell[1] + 0.5, 0.5], np.float32)
        return (at + np.c_[np.linspace(-0.3, 0.3, 3000), np.zeros(3000), np.zeros(3000)]).astype(np.float32)

    parts = []
    for dx in (0, 20):           # the same block twice: rays cross the one at dx = 20, and end behind it
        bx = ox - 2 + dx
        parts += [in_cell((bx + i, oy - 2 + j, 0), 30) for i in range(4) for j in range(4) if (i, j) not in ((1, 1), (2, 2))]
        parts += [in_cell((bx + 1, oy - 1, 0), 4), line((bx + 2, oy))]
    cloud = np.concatenate(parts)
    src = np.concatenate([in_cell((ox - 2 + dx + i, oy - 2 + j, 0), 20, 0.7) for dx in (0, 20) for i in range(4) for j in range(4)])
    g = handle(ndt)
    hist = History(ndt)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    full = Ref(mods, cloud, src).check(g)["grid"]
    assert (full["n"] == -1).sum() >= 1 and ((full["n"] > 0) & (full["n"] < 6)).sum() == 2 and len(full["n"]) == 32
    origin = np.array([ox + 40.5, oy + 0.25, 0.5], np.float32)
    ends = np.c_[np.full(400, ox + 10.5), oy - 4 + 8 * rng.random(400), rng.random(400)]
    scan = clear_scan(po, rc.off_faces(rng, ends, 1.0), None, origin, 1.0, spec_of(1.0))
    ref, gone, d = clear_both(mods, g, hist, [scan], None, [origin], min_rays=1)
    assert len(gone) == 16                                              # the block at dx = 20 goes whatever its voxels' states
    got = Ref(mods, hist.cat(), src).check(g)
    n = got["grid"]["n"]
    assert len(n) == 16 and (n == -1).sum() == 1 and ((n > 0) & (n < 6)).sum() == 1
    more = np.concatenate([in_cell((ox - 1, oy - 1, 0), 3), in_cell((ox + 19, oy - 1, 0), 3)])
    g.targetAccumulate(more)                                            # the kept voxel under min_pts continues and crosses it;
    hist.add(more)                                                      # its removed twin starts again from nothing
    n = Ref(mods, hist.cat(), src).check(g)["grid"]["n"]
    assert len(n) == 17 and sorted(n[(n > 0) & (n < 6)].tolist()) == [3]


# ---- 7: the app
def test_map_sequence_clear_rays(mods, tmp_path):
    ndt, po, clouds, _ = mods
    scans, d = sequence(clouds, ndt, tmp_path, n=5)
    exe = build_app(tmp_path, "map_sequence")
    out = subprocess.check_output([exe, "--scan-to-map", "--clear-rays", "2", "1.5", str(d)], text=True)
    step = matrices(out, "Transform ")
    lines = [ln for ln in out.splitlines() if ln.startswith("cleared: ")]
    assert len(step) == 4 and len(lines) == 4 and "registrations 4" in out
    g = handle(ndt)
    g.setStepSize(0.1)
    g.setTransformationEpsilon(0.01)
    g.setMaximumIterations(64)
    g.setNeighborhoodSearchMethod(ndt.DIRECT7)
    filt = [g.voxelGridFilter(sc, 0.5) for sc in scans]
    pose = EYE.copy()
    g.targetAccumulate(filt[0], pose)
    want = []
    for k in range(1, 5):
        g.setInputSource(filt[k])
        g.align(pose)
        pose = g.getFinalTransformation().astype(np.float32)
        assert rot_err(step[k - 1], pose) < 1e-5 and trans_err(step[k - 1], pose) < 1e-5, k
        before = g.targetAccumulated()["voxels"]
        up = g.uploadCloud(filt[k])
        g.targetClearRays(up, pose, None, min_rays=2, margin=1.5)
        up.release()
        want.append("cleared: %d/%d" % (g.targetClearRaysDiag()["removed_voxels"], before))
        g.targetAccumulate(filt[k], pose)
    assert lines == want
    assert any(int(ln.split()[1].split("/")[0]) > 0 for ln in lines)
    plain = subprocess.check_output([exe, "--scan-to-map", str(d)], text=True)
    assert "cleared" not in plain
    assert subprocess.run([exe, "--clear-rays", "2", "1.5", str(d)], capture_output=True).returncode == 2
    assert subprocess.run([exe, "--scan-to-map", "--clear-rays", "0", "1.5", str(d)], capture_output=True).returncode == 2
