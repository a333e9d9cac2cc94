"""ndt_score_poses against the loop of ndt_calculate_score over host-transformed clouds (the only way to score a candidate
pose without it), and ndt_align_guesses against ndt_align_batch with the source replicated, alternating in one process: the
node shape -- a 16 k-point scan (16 000 of the points of a filtered 60 k-point scan) against a 39 k-point target (60 k raw
points filtered at 0.5 m), resolution 1.0, DIRECT7.
    python tools/time_score_poses.py [runs (>= 5)]
scorePoses is timed at 64 / 1 024 / 16 384 poses (an x / y / yaw search around the true pose); the loop is SAMPLED on 64
poses and scaled (16 384 transforms and uploads would take the better part of a minute).  alignGuesses is timed at 8 / 64 /
256 guesses.  Every figure is a host clock around calls that end in a stream synchronise or a polled result.  Prints one
JSON line and writes it to profiles/score_poses_time.json; no ratio is fixed in advance."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import _lib, clouds, ndt  # noqa: E402

runs = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
LOOP_SAMPLE = 64

rng = np.random.default_rng(5)
world = clouds.target_surfaces(400000, seed=77, extent=60.0)[:, :3].astype(np.float32)
g = ndt.NormalDistributionsTransform()
g.setResolution(1.0)
g.setStepSize(0.1)
g.setTransformationEpsilon(0.01)
g.setMaximumIterations(64)
g.setNeighborhoodSearchMethod(_lib.DIRECT7)
g.warmUp(65536)
target = g.voxelGridFilter(world[rng.choice(len(world), 60000, replace=False)], 0.5)   # ~39 k points
T_true = clouds.make_T([0.6, -0.4, 0.05], np.deg2rad([0.2, -0.1, 3.0]))
raw = clouds.apply_T(np.linalg.inv(T_true), world[rng.choice(len(world), 60000, replace=False)]) + rng.normal(0, 0.01, (60000, 3))
source = g.voxelGridFilter(raw.astype(np.float32), 0.5)
source = np.ascontiguousarray(source[np.sort(rng.choice(len(source), min(16000, len(source)), replace=False))])
g.setInputTarget(target)
g.setInputSource(source)


def search_poses(n):
    """n poses of an x / y / yaw lattice around the true pose (+-2 m, +-10 degrees)"""
    side = int(round(n ** (1.0 / 3.0)))
    while side ** 3 < n:
        side += 1
    xs = np.linspace(-2.0, 2.0, side)
    yaws = np.deg2rad(np.linspace(-10.0, 10.0, side))
    out = [clouds.make_T([x, y, 0.0], [0.0, 0.0, a]) @ T_true for x in xs for y in xs for a in yaws]
    return np.stack(out[:n]).astype(np.float32)


def moved(T):
    """pcl::transformPointCloud on the host, in f32"""
    return (source @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def loop(P):
    t0 = time.perf_counter()
    out = [g.calculateScore(moved(T)) for T in P]
    return time.perf_counter() - t0, out


def one_call(P):
    t0 = time.perf_counter()
    out = g.scorePoses(P)
    return time.perf_counter() - t0, out


out = dict(metric="median of %d runs after a warm-up" % runs, target_points=len(target), source_points=len(source), score_poses={},
           align_guesses={})
sample = search_poses(LOOP_SAMPLE)
loop(sample)
for n in (64, 1024, 16384):
    P = search_poses(n)
    one_call(P)  # warm-up
    tl, tc = [], []
    for _ in range(runs):  # alternating
        tl.append(loop(sample)[0])
        tc.append(one_call(P)[0])
    per_pose_loop = float(np.median(tl)) / LOOP_SAMPLE
    launches, blocks = g.scorePosesLaunches()
    scores = one_call(P)[1]
    out["score_poses"][str(n)] = dict(call_ms=round(1e3 * float(np.median(tc)), 3), poses_per_s=round(n / float(np.median(tc)), 1),
                                      loop_ms_scaled=round(1e3 * per_pose_loop * n, 3), loop_us_per_pose=round(1e6 * per_pose_loop, 2),
                                      speedup=round(per_pose_loop * n / float(np.median(tc)), 2), launches=launches, blocks=blocks,
                                      best_pose_error_m=round(float(np.linalg.norm(P[int(np.argmax(scores))][:3, 3] - T_true[:3, 3])), 3))

# alignBatch splits 16 scans and more over independent lock-step groups (host work of one behind the kernels of another);
# alignGuesses is one loop, so the replicated batch is timed both ways: as it runs by default and as one loop
twin, twin1 = g.copy(), g.copy()
twin1.setBatchGroups(1)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


for n in (8, 64, 256):
    G = np.stack([clouds.random_T(np.random.default_rng(100 + k), 0.3, 1.0) @ T_true for k in range(n)]).astype(np.float32)
    rep = [source] * n
    g.alignGuesses(G)
    twin.alignBatch(rep, G)
    twin1.alignBatch(rep, G)  # warm-up
    ta, tb, t1 = [], [], []
    for _ in range(runs):
        ta.append(timed(lambda: g.alignGuesses(G))[0])
        tb.append(timed(lambda: twin.alignBatch(rep, G))[0])
        t1.append(timed(lambda: twin1.alignBatch(rep, G))[0])
    r, rb = g.alignGuesses(G), twin.alignBatch(rep, G)
    out["align_guesses"][str(n)] = dict(call_ms=round(1e3 * float(np.median(ta)), 3), batch_ms=round(1e3 * float(np.median(tb)), 3),
                                        batch_one_loop_ms=round(1e3 * float(np.median(t1)), 3),
                                        speedup=round(float(np.median(tb)) / float(np.median(ta)), 3),
                                        speedup_over_one_loop=round(float(np.median(t1)) / float(np.median(ta)), 3),
                                        same_results=bool(r["T"].tobytes() == rb["T"].tobytes()),
                                        not_converged=int((~r["converged"]).sum()))
text = json.dumps(out)
print(text)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "score_poses_time.json"), "w") as f:
    f.write(text + "\n")
