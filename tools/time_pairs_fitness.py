"""ndt_pairs_fitness_scores (every pair of the last pairs call scored in one launch) against the loop a caller has today:
ndt_get_fitness_score on per-pair handles, each holding that pair's target, source and an align result.  The clouds are
tools/time_pairs.py's (40 scans of 60 k raw points filtered at 0.5 m, ~39 k points each, the node's settings).  At 8 / 16 /
39 / 128 pairs, every run: one pairs call (its time reported for scale), then the two forms alternately, each on fresh
grids (so both include the search-index builds).  Prints one JSON line of medians in ms.
    python tools/time_pairs_fitness.py [runs (>= 5)] [scans] [raw points per scan]
--profile-one: the same clouds, then ONE pairs call over the consecutive pairs, ONE ndt_pairs_fitness_scores call and the
    per-pair loop once (the kernel table in profiles/: rocprofv3 --kernel-trace --stats --output-format csv -d DIR
    -o pairs_fitness39 -- python tools/time_pairs_fitness.py --profile-one)"""
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


def make_handle():
    h = ndt.NormalDistributionsTransform()
    h.setResolution(1.0)
    h.setStepSize(0.1)
    h.setTransformationEpsilon(0.01)
    h.setMaximumIterations(64)
    h.setNeighborhoodSearchMethod(_lib.DIRECT7)
    return h


rng = np.random.default_rng(3)
world = clouds.target_surfaces(4 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
g = make_handle()
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
    f = g.pairsFitness()
    # ... and the per-pair loop once, so that the table holds its 39 k_fitness launches beside the one k_fitness_multi
    hs = []
    for k in range(len(f)):
        h = make_handle()
        h.setInputTargetCloud(dcs[k])
        h.setInputSourceCloud(dcs[k + 1])
        h.align()
        hs.append(h)
    fl = np.array([h.getFitnessScore() for h in hs])
    print(json.dumps(dict(pairs=len(f), converged=int(r["converged"].sum()), fitness_median=float(np.median(f)),
                          values_equal=bool(np.array_equal(f, fl)))))
    sys.exit(0)

# consecutive pairs first, then (k-2, k), (k-3, k) ... until there are enough (time_pairs.py's order)
all_pairs = [(i - d, i) for d in range(1, n_scans) for i in range(d, n_scans)]
singles = [make_handle() for _ in range(128)]


def pairs_call(pairs):
    t0 = time.perf_counter()
    r = g.alignPairs(dcs, pairs)
    return time.perf_counter() - t0, r


def fitness_call():
    t0 = time.perf_counter()
    f = g.pairsFitness()
    return time.perf_counter() - t0, f


def loop_setup(pairs):  # (not timed) every pair on a handle of its own, target set anew: its search index is not built yet
    for h, (a, b) in zip(singles, pairs):
        h.setInputTargetCloud(dcs[a])
        h.setInputSourceCloud(dcs[b])
        h.align()


def loop_call(pairs):
    t0 = time.perf_counter()
    f = [h.getFitnessScore() for h in singles[:len(pairs)]]
    return time.perf_counter() - t0, np.array(f)


out = dict(metric="ms per call (median of %d runs after a warm-up)" % runs, scans=n_scans, raw_points=n_raw,
           points_per_scan=round(pts_per_scan, 1), sizes={})
for n in (8, 16, 39, 128):
    pairs = all_pairs[:n]
    tp, tf, tl = [], [], []
    for rep in range(runs + 1):  # (run 0: warm-up)
        a, _ = pairs_call(pairs)
        b, f = fitness_call()
        loop_setup(pairs)
        c, fl = loop_call(pairs)
        if rep:
            tp.append(a)
            tf.append(b)
            tl.append(c)
    med = lambda v: round(1e3 * float(np.median(v)), 3)  # noqa: E731
    out["sizes"][str(n)] = dict(fitness_ms=med(tf), sequential_ms=med(tl), pairs_call_ms=med(tp),
                                speedup=round(float(np.median(tl)) / float(np.median(tf)), 2),
                                fitness_over_pairs_call=round(float(np.median(tf)) / float(np.median(tp)), 3),
                                values_equal=bool(np.array_equal(f, fl)))
print(json.dumps(out))
