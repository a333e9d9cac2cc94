"""ndt_align_pairs_clouds against the sequential loop (ndt_set_input_target_cloud + ndt_set_input_source_cloud + ndt_align per
pair) on the same resident clouds, alternating in one process: the node shape -- a static world seen from a moving pose, 40
scans of 60 k raw points filtered at 0.5 m (~39 k points), resolution 1.0, step 0.1, epsilon 0.01, 64 iterations, DIRECT7.
Prints one JSON line: median pairs/s of both forms at 8 / 16 / 39 / 128 pairs, and the pairs call's target build on its own
(every target paired with an empty source).
    python tools/time_pairs.py [runs (>= 5)] [scans] [raw points per scan]
--profile-one: the same clouds, then ONE call over the consecutive pairs and nothing else (the kernel table in profiles/:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o pairs39 -- python tools/time_pairs.py --profile-one)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import _lib, clouds, ndt  # noqa: E402

profile_one = "--profile-one" in sys.argv
args = [a for a in sys.argv[1:] if a != "--profile-one"]
runs = max(5, int(args[0]) if len(args) > 0 else 7)
n_scans = int(args[1]) if len(args) > 1 else 40
n_raw = int(args[2]) if len(args) > 2 else 60000

rng = np.random.default_rng(3)
world = clouds.target_surfaces(4 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
g = ndt.NormalDistributionsTransform()
g.setResolution(1.0)
g.setStepSize(0.1)
g.setTransformationEpsilon(0.01)
g.setMaximumIterations(64)
g.setNeighborhoodSearchMethod(_lib.DIRECT7)
g.warmUp(65536)
pose = np.eye(4)
dcs = []
for k in range(n_scans):
    if k:
        pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
    pick = world[rng.choice(len(world), n_raw, replace=False)]
    raw = (clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32)
    dcs.append(g.voxelGridFilterCloud(raw, 0.5)[0])
pts_per_scan = float(np.mean([len(d) for d in dcs]))
if profile_one:
    r = g.alignPairs(dcs)
    print(json.dumps(dict(pairs=len(r["iterations"]), converged=int(r["converged"].sum()), iterations=r["iterations"].tolist())))
    sys.exit(0)
empty = g.uploadCloud(np.zeros((0, 3), np.float32))

# consecutive pairs first, then (k-2, k), (k-3, k) ... until there are enough
all_pairs = [(i - d, i) for d in range(1, n_scans) for i in range(d, n_scans)]


def sequential(pairs):
    t0 = time.perf_counter()
    for a, b in pairs:
        g.setInputTargetCloud(dcs[a])
        g.setInputSourceCloud(dcs[b])
        g.align()
    return time.perf_counter() - t0


def batched(pairs):
    t0 = time.perf_counter()
    g.alignPairs(dcs, pairs)
    return time.perf_counter() - t0


def build_only(targets):
    cl = [dcs[t] for t in targets] + [empty]
    pairs = [(k, len(targets)) for k in range(len(targets))]
    t0 = time.perf_counter()
    g.alignPairs(cl, pairs)
    return time.perf_counter() - t0


out = dict(metric="pairs/s (median of %d runs after a warm-up)" % runs, scans=n_scans, raw_points=n_raw,
           points_per_scan=round(pts_per_scan, 1), sizes={})
for n in (8, 16, 39, 128):
    pairs = all_pairs[:n]
    sequential(pairs)
    batched(pairs)  # warm-up
    ts, tb = [], []
    for _ in range(runs):  # alternating
        ts.append(sequential(pairs))
        tb.append(batched(pairs))
    res = g.alignPairs(dcs, pairs)
    out["sizes"][str(len(pairs))] = dict(pairs_per_s=round(len(pairs) / float(np.median(tb)), 1),
                                         sequential_per_s=round(len(pairs) / float(np.median(ts)), 1),
                                         speedup=round(float(np.median(ts)) / float(np.median(tb)), 3),
                                         lock_steps=g.commStats()["lock_steps"],
                                         not_converged=int((~res["converged"]).sum()))
targets = sorted({a for a, _ in all_pairs[:39]})
build_only(targets)
tbuild = [build_only(targets) for _ in range(runs)]
out["target_build_ms_%d" % len(targets)] = round(1e3 * float(np.median(tbuild)), 3)
print(json.dumps(out))
