"""Cost of the centroid fitness (ndt_get_centroid_fitness_score) of one scan against an accumulated map of S = 8 / 40 / 128 /
512 scans -- the scans of tools/time_target_crop.py (60 k raw points, ~39 k after the 0.5 m prefilter, at the poses of their
walk, 1 m voxels) -- beside, in the same sitting and on the same map:
 (i)  one ndt_align of that scan against the map (from its true pose);
 (ii) the route that needs no new kernel: ndt_grid_centroids_cloud -> ndt_set_input_target_cloud on a second handle ->
      ndt_batch_fitness_scores of the scan there.  Its grid and point index are rebuilt per scan, as a changing map forces.
The scan is scan S at its pose (the next scan of the walk).  Every timed call is followed by hipDeviceSynchronize inside the
timed region; the first repetition of each is the warm-up and is dropped.  `direct_first` is a call right after an update
(the excursion is stale: one more launch and read-back), `direct` the calls after it.  Prints one JSON line.
    python tools/time_centroid_fitness.py [runs (>= 7)] [raw points per scan] [only this map size]"""
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import _lib, clouds, ndt  # noqa: E402

runs = max(7, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
n_raw = int(sys.argv[2]) if len(sys.argv) > 2 else 60000
sizes = (int(sys.argv[3]),) if len(sys.argv) > 3 else (8, 40, 128, 512)
LEAF = 0.5

up = ndt.NormalDistributionsTransform()   # makes and holds every resident cloud
up.warmUp(65536)
linked = [m.group(1) for m in re.finditer(r"(/\S*libamdhip64\.so[.\d]*)", open("/proc/self/maps").read()) if "/torch/" not in m.group(1)]
hip = C.CDLL(linked[0] if linked else "libamdhip64.so")


def timed(call):
    t0 = time.perf_counter()
    out = call()
    hip.hipDeviceSynchronize()
    return time.perf_counter() - t0, out


def stats(t):
    return dict(median_ms=round(1e3 * float(np.median(t)), 3), min_ms=round(1e3 * float(np.min(t)), 3), max_ms=round(1e3 * float(np.max(t)), 3))


rng = np.random.default_rng(3)
world = clouds.target_surfaces(4 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
pose = np.eye(4)
dev, host, poses = [], {}, []
for k in range(max(sizes) + 1):
    if k:
        pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
    pick = world[rng.choice(len(world), n_raw, replace=False)]
    dev.append(up.voxelGridFilterCloud((clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32), LEAF)[0])
    poses.append(pose.astype(np.float32))
    if k in sizes:
        host[k] = np.ascontiguousarray(np.c_[dev[k].numpy(), np.ones(len(dev[k]), np.float32)])
res = dict(metric="ms per call, hipDeviceSynchronize included", raw_points=n_raw, prefilter_leaf=LEAF, resolution=1.0, runs=runs,
           library=os.path.relpath(_lib.LIB_PATH, ROOT), maps={})
a = ndt.NormalDistributionsTransform()
a.warmUp(65536)
b = ndt.NormalDistributionsTransform()    # route (ii)'s second handle
b.warmUp(65536)
for S in sizes:
    a.targetAccumulateReset()
    for k in range(S):
        a.targetAccumulateCloud(dev[k], poses[k])
    scan, T = host[S], poses[S]
    a.setInputSourceCloud(dev[S])
    t_align, t_direct, t_first, t_route, t_parts = [], [], [], [], []
    for r in range(runs + 1):
        ta, _ = timed(lambda: a.align(T))
        # the excursion made stale as every update makes it: one point at the scan's position (inside the map's box)
        a.targetAccumulate(np.array([[T[0, 3], T[1, 3], T[2, 3], 1.0]], np.float32))
        hip.hipDeviceSynchronize()
        tf, first = timed(lambda: a.batchCentroidFitness([scan], [T]))
        d_first = a.centroidFitnessDiag()
        td, direct = timed(lambda: a.batchCentroidFitness([scan], [T]))
        diag = a.centroidFitnessDiag()

        def route():
            t0 = time.perf_counter()
            dc = a.gridCentroidsCloud()
            hip.hipDeviceSynchronize()
            t1 = time.perf_counter()
            b.setInputTargetCloud(dc, is_dense=True)
            hip.hipDeviceSynchronize()
            t2 = time.perf_counter()
            v = b.batchFitness([scan], [T])
            hip.hipDeviceSynchronize()
            t3 = time.perf_counter()
            dc.release()
            return v, (t1 - t0, t2 - t1, t3 - t2)
        tr, (via, parts) = timed(route)
        assert first[0] == direct[0] == via[0], (first, direct, via)    # the same bits by both routes
        assert d_first["excursion_passes"] == 1 and diag["excursion_passes"] == 0
        if r:
            t_align.append(ta)
            t_first.append(tf)
            t_direct.append(td)
            t_route.append(tr)
            t_parts.append(parts)
    parts = np.asarray(t_parts)
    acc = a.targetAccumulated()
    row = dict(voxels=acc["voxels"], centroids=len(a.gridCentroids()[1]), scan_points=len(scan), fitness=float(direct[0]),
               box_cells=[int(v) for v in a.grid()["div_b"]], search_blocks=diag["max_blocks"], excursion=diag["excursion"],
               align=stats(t_align), align_iterations=a.getFinalNumIteration(), direct=stats(t_direct), direct_first=stats(t_first),
               route_cloud_target_fitness=stats(t_route), route_centroids_cloud=stats(parts[:, 0]), route_set_target=stats(parts[:, 1]),
               route_batch_fitness=stats(parts[:, 2]))
    row["route_over_direct"] = round(row["route_cloud_target_fitness"]["median_ms"] / row["direct"]["median_ms"], 2)
    row["route_over_direct_first"] = round(row["route_cloud_target_fitness"]["median_ms"] / row["direct_first"]["median_ms"], 2)
    row["direct_over_align"] = round(row["direct"]["median_ms"] / row["align"]["median_ms"], 3)
    res["maps"][str(S)] = row
print(json.dumps(res))
