"""ndt_cloud_extract_clusters and ndt_cloud_cluster (min_size 10) beside ndt_cloud_remove_outliers(radius = tolerance, 1 neighbour) of
the same resident cloud -- the RADIUS value launch does the walk of the link kernel with no unions, so it is the yardstick -- and
ndt_cloud_extract_clusters_clouds beside a loop of single calls.
    python tools/time_clusters.py [runs (>= 5)]
Clouds: the golden source scan without its ground (segmentPlane: 0.2 m, 128 hypotheses, within 15 degrees of z), and a street
of 100 m x 100 m without its ground -- 300 boxes of car to van size with points on their faces, 40 poles, 2 % stray points -- at
16 k, 100 k and 2 M points; tolerances 0.2 and 0.5 m.  Many clouds: 8 / 40 / 128 streets of 16 k points at 0.5 m.  Every figure is
a host clock around a call that returns after its own work is done, the median of the runs after a warm-up of every call at
that shape; the calls of a shape alternate.  cas_retries is what the timed calls' last run reported (it varies from run to
run).  Prints one JSON line and writes it to profiles/cluster_time.json.  Times only: no threshold is checked, nobody had
measured any of this."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import ndt  # noqa: E402

runs = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
SIDE = 100.0
MIN_SIZE = 10


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def med_us(ts):
    return round(1e6 * float(np.median(ts)), 2)


def street(n, seed):
    """what stands on the ground: points on the faces of boxes, on poles, and a few stray ones"""
    rng = np.random.default_rng(seed)
    n_pole, n_stray = n // 20, n // 50
    n_box = n - n_pole - n_stray
    centre = np.column_stack([rng.random((300, 2)) * SIDE, np.zeros(300)])
    half = np.column_stack([1.0 + 1.5 * rng.random(300), 0.8 + 0.4 * rng.random(300), 0.7 + 0.6 * rng.random(300)])
    which = rng.integers(0, 300, n_box)
    p = (2.0 * rng.random((n_box, 3)) - 1.0) * half[which]
    face = rng.integers(0, 3, n_box)
    p[np.arange(n_box), face] = np.where(rng.random(n_box) < 0.5, -1.0, 1.0) * half[which, face]  # onto a face of the box
    boxes = p + centre[which] + np.array([0.0, 0.0, 1.3])
    foot = rng.random((40, 2)) * SIDE
    k = rng.integers(0, 40, n_pole)
    poles = np.column_stack([foot[k] + 0.05 * rng.standard_normal((n_pole, 2)), 6.0 * rng.random(n_pole)])
    stray = np.column_stack([rng.random((n_stray, 2)) * SIDE, 8.0 * rng.random(n_stray)])
    out = np.concatenate([boxes, poles, stray]).astype(np.float32)
    return out[rng.permutation(len(out))]


g = ndt.NormalDistributionsTransform()
g.warmUp(65536)
out = dict(metric="median of %d runs after a warm-up, host clock around calls that return after their own work" % runs,
           spec="min_size %d, no max_size; removeOutliers: radius = tolerance, 1 neighbour" % MIN_SIZE, single={}, many={})

golden = np.load(os.path.join(ROOT, "tests", "golden", "pair_0p1.npz"))["source"]
ground = ndt.plane_spec(0.2, 128, seed=0, axis=(0, 0, 1), eps_angle=float(np.float32(np.pi / 12)))
clouds = [("golden scan without its ground", g.segmentPlane(g.uploadCloud(golden), ground, inliers=False, others=True)[2])]
clouds += [("street %d" % n, g.uploadCloud(street(n, n))) for n in (16384, 100000, 2000000)]
for name, dc in clouds:
    for tol in (0.2, 0.5):
        calls = dict(extract_clusters=lambda: g.extractClusters(dc, tol, MIN_SIZE), cluster_cloud=lambda: g.clusterCloud(dc, tol, MIN_SIZE),
                     cluster_cloud_32_rows_no_indices=lambda: g.clusterCloud(dc, tol, MIN_SIZE, capacity=32, indices=False),
                     remove_outliers_radius=lambda: g.removeOutliers(dc, radius=tol, min_neighbors=1))
        for fn in calls.values():
            fn()
            fn()
        ts = {k: [] for k in calls}
        retries = {}
        for _ in range(runs):  # alternating
            for k, fn in calls.items():
                ts[k].append(timed(fn)[0])
                if k != "remove_outliers_radius":
                    retries[k] = g.diagClusters()["cas_retries"]
        kept, sm = g.extractClusters(dc, tol, MIN_SIZE)
        row = dict(points=len(dc), tolerance=tol, kept=len(kept), summary=sm, diag=g.diagClusters(), cas_retries=retries)
        g.removeOutliers(dc, radius=tol, min_neighbors=1)
        row["outlier_diag"] = g.outlierDiag()
        for k in ts:
            row[k + "_us"] = med_us(ts[k])
            row[k + "_spread"] = round((max(ts[k]) - min(ts[k])) / float(np.median(ts[k])), 3)
        row["extract_over_remove_outliers"] = round(row["extract_clusters_us"] / row["remove_outliers_radius_us"], 3)
        row["cluster_over_remove_outliers"] = round(row["cluster_cloud_us"] / row["remove_outliers_radius_us"], 3)
        out["single"]["%s, %.1f m" % (name, tol)] = row
for m in (8, 40, 128):
    dcs = [g.uploadCloud(street(16384, 1000 + k)) for k in range(m)]
    calls = dict(clouds=lambda: g.extractClustersClouds(dcs, 0.5, MIN_SIZE), loop=lambda: [g.extractClusters(dc, 0.5, MIN_SIZE) for dc in dcs],
                 outliers_clouds=lambda: g.removeOutliersClouds(dcs, radius=0.5, min_neighbors=1))
    for fn in calls.values():
        fn()
        fn()
    ts = {k: [] for k in calls}
    for _ in range(runs):
        for k, fn in calls.items():
            ts[k].append(timed(fn)[0])
    g.extractClustersClouds(dcs, 0.5, MIN_SIZE)
    out["many"][str(m)] = dict(clouds=m, points_each=16384, clouds_us=med_us(ts["clouds"]), loop_us=med_us(ts["loop"]),
                               outliers_clouds_us=med_us(ts["outliers_clouds"]), us_per_cloud=round(med_us(ts["clouds"]) / m, 2),
                               loop_us_per_cloud=round(med_us(ts["loop"]) / m, 2),
                               clouds_over_outliers_clouds=round(med_us(ts["clouds"]) / med_us(ts["outliers_clouds"]), 3), **g.diagClusters())
text = json.dumps(out)
print(text)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "cluster_time.json"), "w") as f:
    f.write(text + "\n")
