"""Scan-to-map GICP against the accumulated target (gicp_set_input_target_grid) beside the route a caller had before it, on
accumulated maps of 8 / 40 / 128 synthetic scans (tools/time_target_accumulate.py's generator: 60 k raw points, 0.5 m prefilter,
1 m voxels, the poses of a walk).  Per map size, the scan that follows the map's last one is registered from the previous pose:
  grid       the NEW route: the map gets one more scan (not timed), then align on the bound handle -- the refresh pass after the map
             update included
  reference  the route before: ndt_grid_centroids_cloud, the covariances through the host (gicp_target_grid_voxels stands in for
             the dump's, in the reference route's favour), gicp_set_input_target_cloud (an index build over every centroid of the
             map), gicp_set_target_covariances, align
  ndt        ndt_align of the same scan on the map handle, for scale
  refresh    the mark / scan / gather pass alone: gicp_target_grid_voxels' count query after a map update
Protocol: one MI355X, median of 7 after a warm-up, the host clock around calls that return after their own work, the alternatives
alternated in one process.  Before each repetition the map is touched by an update of the same scan at the same pose, so that
every repetition of `grid` and `refresh` pays its refresh.  The structural claim is read from the counters: refreshes per align
(gicp_diag_target_grid), and the index builds the reference route queues (one per scan, over the whole map).
Writes profiles/gicp_grid_time.json and prints it.
    python tools/time_gicp_grid.py [runs (>= 7)] [raw points per scan]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import clouds, gicp, ndt  # noqa: E402

runs = max(7, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
n_raw = int(sys.argv[2]) if len(sys.argv) > 2 else 60000
sizes = (8, 40, 128)
LEAF, GATE = 0.5, 3.0

rng = np.random.default_rng(3)
world = clouds.target_surfaces(4 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
pose = np.eye(4)
f = ndt.NormalDistributionsTransform()
f.warmUp(65536)
filt, poses = [], []
for k in range(max(sizes) + 1):
    if k:
        pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
    pick = world[rng.choice(len(world), n_raw, replace=False)]
    scan = (clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32)
    dc = f.voxelGridFilterCloud(scan, LEAF)[0]
    filt.append(dc.numpy())
    dc.release()
    poses.append(pose.astype(np.float32))
del f


def med(v):
    return float(np.median(v) * 1e3)


m = ndt.NormalDistributionsTransform()
m.setResolution(1.0)
m.warmUp(65536)
dev = [m.uploadCloud(c) for c in filt]
out = dict(runs=runs, raw_points=n_raw, gate=GATE, cov_mode="plane", sizes={})
done = 0
for S in sizes:
    while done < S:
        m.targetAccumulateCloud(dev[done], poses[done])
        done += 1
    scan, guess = dev[S], poses[S - 1]
    m.setInputSourceCloud(scan)
    new = gicp.GeneralizedIterativeClosestPoint()
    new.setMaxCorrespondenceDistance(GATE)
    new.setInputTargetGrid(m, "plane")
    new.setInputSourceCloud(scan)
    ref = gicp.GeneralizedIterativeClosestPoint()
    ref.setMaxCorrespondenceDistance(GATE)
    ref.setInputSourceCloud(scan)
    t = dict(grid=[], reference=[], ndt=[], refresh=[])
    results = {}
    touch = lambda: m.targetAccumulateCloud(dev[S - 1], poses[S - 1])   # the map changes: the same scan at the same pose again
    r0 = new.diagTargetGrid()["refreshes"]
    aligns = 0
    for rep in range(runs + 1):                                          # (the first repetition is the warm-up)
        touch()
        t0 = time.perf_counter()
        new.align(guess)
        t["grid"].append(time.perf_counter() - t0)
        aligns += 1
        results["grid"] = new.getFinalTransformation()
        t0 = time.perf_counter()
        cen = m.gridCentroidsCloud()
        _, cov, _ = new.targetGridVoxels()                               # (no refresh: the align above made it)
        ref.setInputTargetCloud(cen)
        ref.setTargetCovariances(cov)
        ref.align(guess)
        t["reference"].append(time.perf_counter() - t0)
        results["reference"] = ref.getFinalTransformation()
        cen.release()
        t0 = time.perf_counter()
        m.align(guess)
        t["ndt"].append(time.perf_counter() - t0)
        results["ndt"] = m.getFinalTransformation()
        touch()
        t0 = time.perf_counter()
        new.targetGridVoxels()
        t["refresh"].append(time.perf_counter() - t0)
    d = new.diagTargetGrid()
    truth = poses[S]
    out["sizes"][str(S)] = dict(
        voxels=d["voxels"], scan_points=len(filt[S]), excursion=d["excursion"], correspond_blocks=d["correspond_blocks"],
        grid_ms=med(t["grid"][1:]), reference_ms=med(t["reference"][1:]), ndt_ms=med(t["ndt"][1:]), refresh_ms=med(t["refresh"][1:]),
        refreshes=d["refreshes"] - r0, aligns=aligns, map_updates=2 * (runs + 1),
        reference_index_builds=runs + 1, reference_index_points=d["voxels"],
        same_bits=bool(np.array_equal(results["grid"], results["reference"])),
        trans_err={k: float(np.abs(v[:3, 3] - truth[:3, 3]).max()) for k, v in results.items()},
        iterations=dict(grid=new.getFinalNumIteration(), reference=ref.getFinalNumIteration()))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "gicp_grid_time.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
