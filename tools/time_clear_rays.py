"""Cost of clearing the accumulating target by rays (ndt_target_accumulate_clear_rays) beside the update it precedes.
One clearing by a scan of 16 k points and by one of 100 k points (min_rays 2, margin = the resolution, every range) of a target
of S = 8 / 40 / 128 accumulated scans -- the scans of tools/time_target_crop.py (60 k raw points, ~39 k after the 0.5 m prefilter,
at the poses of their walk, 1 m voxels) -- beside the ndt_align of that scan from the previous pose and the
ndt_target_accumulate_cloud update of it, in the same sitting.  The scans are random picks of the world's points, seen from
the pose of scan S: their beams cross whatever lies between.  Per case the target is built `runs + 1` times per form of the
miss count (NDT_RAYS_MERGE=0: an atomic per lane; 1: equal slots of a wave merged), the forms alternating; the first build is
the warm-up; every timed call is followed by hipDeviceSynchronize inside the timed region.  Beside each time: the mean ray
length, the cells a ray visits and the occupied fraction of the visited cells.
Writes profiles/clear_rays_time.json and prints it.
    python tools/time_clear_rays.py [runs (>= 7)] [raw points per map scan]"""
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
sizes = (8, 40, 128)
scan_points = (16000, 100000)
LEAF = 0.5

up = ndt.NormalDistributionsTransform()   # makes and holds every resident cloud
up.warmUp(65536)
linked = [m.group(1) for m in re.finditer(r"(/\S*libamdhip64\.so[.\d]*)", open("/proc/self/maps").read()) if "/torch/" not in m.group(1)]
hip = C.CDLL(linked[0] if linked else "libamdhip64.so")


def timed(call):
    t0 = time.perf_counter()
    call()
    hip.hipDeviceSynchronize()
    return time.perf_counter() - t0


def stats(t):
    return dict(median_ms=round(1e3 * float(np.median(t)), 3), min_ms=round(1e3 * float(np.min(t)), 3), max_ms=round(1e3 * float(np.max(t)), 3))


rng = np.random.default_rng(3)
world = clouds.target_surfaces(4 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
pose = np.eye(4)
dev, poses = [], []
for k in range(max(sizes) + 1):
    if k:
        pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
    pick = world[rng.choice(len(world), n_raw, replace=False)]
    dev.append(up.voxelGridFilterCloud((clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32), LEAF)[0])
    poses.append(pose.astype(np.float32))

res = dict(metric="ms per call, hipDeviceSynchronize included", raw_points_per_map_scan=n_raw, prefilter_leaf=LEAF, resolution=1.0, runs=runs,
           min_rays=2, margin=1.0, library=os.path.relpath(_lib.LIB_PATH, ROOT), cases={})
a = ndt.NormalDistributionsTransform()
a.warmUp(131072)
a.setNeighborhoodSearchMethod(ndt.DIRECT7)
for S in sizes:
    T = poses[S]
    for n_scan in scan_points:
        pick = world[rng.choice(len(world), n_scan, replace=False)]
        host = (clouds.apply_T(np.linalg.inv(T.astype(np.float64)), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32)
        scan = up.uploadCloud(host)
        lens = np.linalg.norm(clouds.apply_T(T.astype(np.float64), host) - T[:3, 3], axis=1)
        t = dict(clear_per_lane=[], clear_merged=[], update=[], align=[])
        row = {}
        for r in range(runs + 1):
            for form in ("clear_per_lane", "clear_merged"):
                os.environ["NDT_RAYS_MERGE"] = "1" if form == "clear_merged" else "0"
                a.targetAccumulateReset()
                for k in range(S):
                    a.targetAccumulateCloud(dev[k], poses[k])
                hip.hipDeviceSynchronize()
                before = a.targetAccumulated()
                if form == "clear_per_lane":
                    a.setInputSourceCloud(scan)
                    ta = timed(lambda: a.align(poses[S - 1]))
                    row["align_iterations"] = a.getFinalNumIteration()
                    misses = int(a.targetRayCounts(scan, T)["miss"].sum())
                    counts = a.targetClearRaysDiag()
                tc = timed(lambda: a.targetClearRays(scan, T))
                d = a.targetClearRaysDiag()
                if form == "clear_per_lane":
                    tu = timed(lambda: a.targetAccumulateCloud(scan, T))
                if r:   # (the first build is the warm-up: the pool finds its blocks)
                    t[form].append(tc)
                    if form == "clear_per_lane":
                        t["update"].append(tu)
                        t["align"].append(ta)
                row[form + "_diag"] = d
        row.update(voxels_before=before["voxels"], points_before=before["points"], scan_points=n_scan, mean_ray_length_m=round(float(lens.mean()), 2),
                   cells_per_ray=round(counts["cells_visited"] / max(counts["rays_cast"], 1), 1),
                   occupied_fraction_of_visited_cells=round(misses / max(counts["cells_visited"], 1), 4),
                   **{k: stats(v) for k, v in t.items()})
        row["clear_over_update"] = round(min(row["clear_per_lane"]["median_ms"], row["clear_merged"]["median_ms"]) / row["update"]["median_ms"], 2)
        res["cases"]["%d scans, %d points" % (S, n_scan)] = row
        scan.release()
os.environ.pop("NDT_RAYS_MERGE", None)
out = os.path.join(ROOT, "profiles", "clear_rays_time.json")
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
