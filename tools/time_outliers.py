"""ndt_cloud_remove_outliers (radius 0.5 m / 2 neighbours; mean_k 20, 1.0 sigma) beside three calls on the same resident cloud --
selectCloud(finite=True), its voxel filter, and GICP's index + covariance pass at k = 20 (with its read-back) -- and
ndt_cloud_remove_outliers_clouds beside a loop of single calls.
    python tools/time_outliers.py [runs (>= 5)]
Clouds: a wavy sheet of 60 m x 60 m with 1 cm noise and 1 % stray points in the 3 m above it (16 k, 100 k, 2 M points).  Many
clouds: 8 / 40 / 128 clouds of 16 k points.  Every figure is a host clock around a call that returns after its own work is
done, the median of the runs after a warm-up of every call at that shape; the calls of a shape alternate.  Prints one JSON
line and writes it to profiles/outlier_time.json.  Times only: no threshold is checked, nobody had measured any of this."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import gicp, ndt  # noqa: E402

runs = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
SIDE = 60.0
RADIUS = dict(radius=0.5, min_neighbors=2)
STAT = dict(mean_k=20, stddev_mul=1.0)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def med_us(ts):
    return round(1e6 * float(np.median(ts)), 2)


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.random((n, 2)) * SIDE
    z = 0.3 * np.sin(0.2 * u[:, 0]) * np.cos(0.15 * u[:, 1]) + 0.01 * rng.standard_normal(n)
    stray = rng.random(n) < 0.01
    z[stray] += 3.0 * rng.random(int(stray.sum()))
    return np.column_stack([u, z]).astype(np.float32)


def filter_resident(g, dc):
    g.voxelGridFilterBegin(dc, 0.5)
    return g.voxelGridFilterEnd()[0]


g = ndt.NormalDistributionsTransform()
g.warmUp(65536)
gi = gicp.GeneralizedIterativeClosestPoint()
gi.setCorrespondenceRandomness(20)


def gicp_pass(dc):
    gi.setInputTargetCloud(dc)
    return gi.covariances(0)


out = dict(metric="median of %d runs after a warm-up, host clock around calls that return after their own work" % runs,
           filters="radius 0.5 m / 2 neighbours; mean_k 20, 1.0 sigma", single={}, many={})
for n in (16384, 100000, 2000000):
    dc = g.uploadCloud(cloud(n, n))
    calls = dict(remove_radius=lambda: g.removeOutliers(dc, **RADIUS), remove_stat=lambda: g.removeOutliers(dc, **STAT),
                 select_finite=lambda: g.selectCloud(dc, finite=True), voxel_filter_0p5=lambda: filter_resident(g, dc),
                 gicp_index_covariances_k20_to_host=lambda: gicp_pass(dc))
    for fn in calls.values():
        fn()
        fn()
    ts = {k: [] for k in calls}
    for _ in range(runs):  # alternating
        for k, fn in calls.items():
            ts[k].append(timed(fn)[0])
    row = dict(points=n)
    for name, kw in (("radius", RADIUS), ("stat", STAT)):
        kept, st = g.removeOutliers(dc, **kw)
        row[name] = dict(kept=len(kept), threshold=st["threshold"], **g.outlierDiag())
    for k in ts:
        row[k + "_us"] = med_us(ts[k])
        row[k + "_spread"] = round((max(ts[k]) - min(ts[k])) / float(np.median(ts[k])), 3)
    out["single"][str(n)] = row
for m in (8, 40, 128):
    dcs = [g.uploadCloud(cloud(16384, 1000 + k)) for k in range(m)]
    row = dict(clouds=m, points_each=16384)
    for name, kw in (("radius", RADIUS), ("stat", STAT)):
        calls = dict(clouds=lambda: g.removeOutliersClouds(dcs, **kw), loop=lambda: [g.removeOutliers(dc, **kw) for dc in dcs])
        for fn in calls.values():
            fn()
            fn()
        ts = {k: [] for k in calls}
        for _ in range(runs):
            for k, fn in calls.items():
                ts[k].append(timed(fn)[0])
        g.removeOutliersClouds(dcs, **kw)
        row[name] = dict(clouds_us=med_us(ts["clouds"]), loop_us=med_us(ts["loop"]), us_per_cloud=round(med_us(ts["clouds"]) / m, 2),
                         loop_us_per_cloud=round(med_us(ts["loop"]) / m, 2), **g.outlierDiag())
    out["many"][str(m)] = row
text = json.dumps(out)
print(text)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "outlier_time.json"), "w") as f:
    f.write(text + "\n")
