"""ndt_nvtl_poses beside ndt_score_poses -- existing code, the yardstick -- on the same handle, the same source and the same pose
tables, alternating in one process; and one ndt_get_nvtl beside one ndt_get_fitness_score after an align.
    python tools/time_nvtl.py [runs (>= 5)]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_nvtl.py trace     (a run of its own: two calls per shape, no timing)
Sources: the bundled pair's source (15 950 points against its 15 772-point target) and a synthetic pair of 100 k source points
against a 39 k-point target (60 k raw points filtered at 0.5 m), resolution 1.0, DIRECT7.  Pose tables: 64 / 1 024 / 16 384
poses of an x / y / yaw lattice around the registering pose.  Every figure is a host clock around a call that ends in a
stream synchronise, the median of the runs after a warm-up of both calls at that shape.  Prints one JSON line and writes it
to profiles/nvtl_time.json; the expectation it reports on (NVTL no slower than 1.10 x scorePoses per pose at each shape) is
checked here, not tuned for."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import _lib, clouds, ndt  # noqa: E402

trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
runs = 2 if trace else max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
POSE_COUNTS = (64, 1024, 16384)


def handle():
    g = ndt.NormalDistributionsTransform()
    g.setResolution(1.0)
    g.setStepSize(0.1)
    g.setTransformationEpsilon(0.01)
    g.setMaximumIterations(64)
    g.setNeighborhoodSearchMethod(_lib.DIRECT7)
    return g


def lattice(n, T_true):
    """n poses of an x / y / yaw lattice around the true pose (+-2 m, +-10 degrees)"""
    side = int(round(n ** (1.0 / 3.0)))
    while side ** 3 < n:
        side += 1
    xs = np.linspace(-2.0, 2.0, side)
    yaws = np.deg2rad(np.linspace(-10.0, 10.0, side))
    out = [clouds.make_T([x, y, 0.0], [0.0, 0.0, a]) @ T_true for x in xs for y in xs for a in yaws]
    return np.stack(out[:n]).astype(np.float32)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def pair_scene():
    d = np.load(os.path.join(ROOT, "tests", "golden", "pair_0p1.npz"))
    with open(os.path.join(ROOT, "tests", "golden", "oracle_golden.json")) as f:
        T_true = np.asarray(json.load(f)["aligns"]["DIRECT7/default"]["T"], dtype=np.float64)
    return d["target"], d["source"], T_true


def synthetic_scene():
    rng = np.random.default_rng(5)
    world = clouds.target_surfaces(400000, seed=77, extent=60.0)[:, :3].astype(np.float32)
    g = handle()
    target = g.voxelGridFilter(world[rng.choice(len(world), 60000, replace=False)], 0.5)
    T_true = clouds.make_T([0.6, -0.4, 0.05], np.deg2rad([0.2, -0.1, 3.0]))
    raw = clouds.apply_T(np.linalg.inv(T_true), world[rng.choice(len(world), 100000, replace=False)]) + rng.normal(0, 0.01, (100000, 3))
    return target, np.ascontiguousarray(raw, dtype=np.float32), T_true


out = dict(metric="median of %d runs after a warm-up, host clock around synchronising calls" % runs, search="DIRECT7", shapes={}, single={})
worst = 0.0
for name, (target, source, T_true) in (("pair", pair_scene()), ("synthetic_100k", synthetic_scene())):
    g = handle()
    g.warmUp(max(65536, len(source)))
    g.setInputTarget(target)
    g.setInputSource(source)
    for n in POSE_COUNTS:
        P = lattice(n, T_true)
        g.scorePoses(P)
        g.nvtlPoses(P)  # warm-up of both at this shape
        ts, tn = [], []
        for _ in range(runs):  # alternating
            ts.append(timed(lambda: g.scorePoses(P))[0])
            tn.append(timed(lambda: g.nvtlPoses(P))[0])
        values, found = g.nvtlPoses(P, counts=True)
        scores = g.scorePoses(P)
        ms, mn = float(np.median(ts)), float(np.median(tn))
        worst = max(worst, mn / ms)
        out["shapes"]["%s/%d" % (name, n)] = dict(
            source_points=len(source), target_points=len(target), poses=n,
            score_poses_ms=round(1e3 * ms, 3), nvtl_poses_ms=round(1e3 * mn, 3), ratio=round(mn / ms, 4),
            score_poses_us_per_pose=round(1e6 * ms / n, 3), nvtl_poses_us_per_pose=round(1e6 * mn / n, 3),
            score_poses_spread=round((max(ts) - min(ts)) / ms, 4), nvtl_poses_spread=round((max(tn) - min(tn)) / mn, 4),
            launches=g.nvtlLaunches()[0], blocks=g.nvtlLaunches()[1],
            best_by_nvtl_error_m=round(float(np.linalg.norm(P[int(np.argmax(values))][:3, 3] - T_true[:3, 3])), 3),
            best_by_score_error_m=round(float(np.linalg.norm(P[int(np.argmax(scores))][:3, 3] - T_true[:3, 3])), 3),
            found_fraction_at_best=round(float(found[int(np.argmax(values))]) / len(source), 4))
    g.align(T_true.astype(np.float32))
    g.getNVTL()
    g.getFitnessScore()
    ta, tb = [], []
    for _ in range(runs):
        ta.append(timed(g.getNVTL)[0])
        tb.append(timed(g.getFitnessScore)[0])
    value, n_found = g.getNVTL()
    out["single"][name] = dict(get_nvtl_us=round(1e6 * float(np.median(ta)), 2), get_fitness_score_us=round(1e6 * float(np.median(tb)), 2),
                               nvtl=round(value, 6), n_found=n_found, source_points=len(source), converged=bool(g.hasConverged()))
out["worst_ratio"] = round(worst, 4)
out["expectation_nvtl_within_1p10_of_score_poses"] = bool(worst <= 1.10)
text = json.dumps(out)
print(text)
if not trace:
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "nvtl_time.json"), "w") as f:
        f.write(text + "\n")
