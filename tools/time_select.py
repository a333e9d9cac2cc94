"""ndt_cloud_select beside the two things a caller had before it -- the host round trip (download, numpy mask,
ndt_cloud_upload) and, as a yardstick that does strictly more work on the same bytes, the voxel filter of the same resident
cloud -- ndt_cloud_select_clouds beside a loop of single calls, and ndt_source_select_by_nvtl beside ndt_source_point_nvtl.
    python tools/time_select.py [runs (>= 5)]
Clouds: uniform points in a 60 m cube about the sensor (16 k, 100 k, 2 M points); the predicate is RANGE | FINITE with the
radius that keeps half the cube's volume.  Many clouds: 8 / 40 / 128 clouds of 16 k points.  NVTL form: the bundled pair at its
registering pose, threshold = the median per-point value.  Every figure is a host clock around a call that returns after its
own work is done, the median of the runs after a warm-up of every call at that shape; the three calls of a shape alternate,
and select and the filter are then also timed back to back with themselves.  Prints one JSON line and writes it to
profiles/select_time.json.  No threshold is checked: nobody had measured any of this."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import _lib, ndt  # noqa: E402

runs = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 9)
SIDE = 60.0
R_HALF = float(SIDE * (3.0 / (8.0 * np.pi)) ** (1.0 / 3.0))  # the ball of half the cube's volume (it fits inside the cube)
SPEC = dict(finite=True, range=(0.0, R_HALF))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def med_us(ts):
    return round(1e6 * float(np.median(ts)), 2)


def cloud(n, seed):
    return np.random.default_rng(seed).uniform(-SIDE / 2, SIDE / 2, (n, 3)).astype(np.float32)


def host_round_trip(g, dc):
    xyz = dc.numpy()
    d = xyz.astype(np.float32)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    keep = np.isfinite(xyz).all(1) & (d2 <= np.float32(R_HALF) * np.float32(R_HALF))
    return g.uploadCloud(xyz[keep])


def filter_resident(g, dc):
    g.voxelGridFilterBegin(dc, 0.5)
    return g.voxelGridFilterEnd()[0]


g = ndt.NormalDistributionsTransform()
g.warmUp(65536)
out = dict(metric="median of %d runs after a warm-up, host clock around calls that return after their own work" % runs,
           predicate="RANGE | FINITE, r_max = %.4f m in a %g m cube: about half the points" % (R_HALF, SIDE), single={}, many={}, nvtl={})
for n in (16384, 100000, 2000000):
    dc = g.uploadCloud(cloud(n, n))
    calls = dict(select=lambda: g.selectCloud(dc, **SPEC), host_round_trip=lambda: host_round_trip(g, dc),
                 voxel_filter_0p5=lambda: filter_resident(g, dc))
    for fn in calls.values():
        fn()
        fn()
    ts = {k: [] for k in calls}
    for _ in range(runs):  # alternating
        for k, fn in calls.items():
            ts[k].append(timed(fn)[0])
    # ... and each call back to back with itself: the alternation above leaves the GPU idle for the round trip's host work
    # (50 ms at 2 M points) in front of every select, the loop of a node does not
    for k in ("select", "voxel_filter_0p5"):
        ts[k + "_back_to_back"] = [timed(calls[k])[0] for _ in range(runs)]
    kept = len(g.selectCloud(dc, **SPEC))
    row = dict(points=n, kept=kept, blocks=g.selectDiag()["blocks"], filtered_points=len(filter_resident(g, dc)))
    for k in ts:
        row[k + "_us"] = med_us(ts[k])
        row[k + "_spread"] = round((max(ts[k]) - min(ts[k])) / float(np.median(ts[k])), 3)
    # bytes the two launches move: the points and a ballot bit each, the kept records in and out
    moved = 16.0 * n + n / 8.0 + n / 8.0 + 32.0 * kept
    row["select_gb_per_s"] = round(moved / float(np.median(ts["select"])) / 1e9, 1)
    row["select_back_to_back_gb_per_s"] = round(moved / float(np.median(ts["select_back_to_back"])) / 1e9, 1)
    row["select_over_filter"] = round(float(np.median(ts["select"])) / float(np.median(ts["voxel_filter_0p5"])), 3)
    out["single"][str(n)] = row
for m in (8, 40, 128):
    dcs = [g.uploadCloud(cloud(16384, 1000 + k)) for k in range(m)]
    calls = dict(clouds=lambda: g.selectClouds(dcs, **SPEC), loop=lambda: [g.selectCloud(dc, **SPEC) for dc in dcs])
    for fn in calls.values():
        fn()
        fn()
    ts = {k: [] for k in calls}
    for _ in range(runs):
        for k, fn in calls.items():
            ts[k].append(timed(fn)[0])
    g.selectClouds(dcs, **SPEC)
    d = g.selectDiag()
    out["many"][str(m)] = dict(clouds=m, points_each=16384, clouds_us=med_us(ts["clouds"]), loop_us=med_us(ts["loop"]),
                               us_per_cloud=round(med_us(ts["clouds"]) / m, 2), loop_us_per_cloud=round(med_us(ts["loop"]) / m, 2),
                               launches=d["launches"], blocks=d["blocks"])
d = np.load(os.path.join(ROOT, "tests", "golden", "pair_0p1.npz"))
with open(os.path.join(ROOT, "tests", "golden", "oracle_golden.json")) as f:
    T = np.asarray(json.load(f)["aligns"]["DIRECT7/default"]["T"], dtype=np.float32)
g.setResolution(1.0)
g.setNeighborhoodSearchMethod(_lib.DIRECT7)
g.setInputTarget(d["target"])
g.setInputSource(d["source"])
L = g.sourcePointNVTL(T)[0]
thr = float(np.median(L[L >= 0]))
calls = dict(source_point_nvtl_to_host=lambda: g.sourcePointNVTL(T), source_point_nvtl_device=lambda: g.sourcePointNVTL(T, device=True),
             source_select_by_nvtl=lambda: g.sourceSelectByNVTL(thr, T))
for fn in calls.values():
    fn()
    fn()
ts = {k: [] for k in calls}
for _ in range(runs):
    for k, fn in calls.items():
        ts[k].append(timed(fn)[0])
kept, n_found = g.sourceSelectByNVTL(thr, T)
out["nvtl"] = dict(source_points=len(d["source"]), n_found=n_found, kept=len(kept), threshold=round(thr, 6), **{k + "_us": med_us(v) for k, v in ts.items()})
text = json.dumps(out)
print(text)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "select_time.json"), "w") as f:
    f.write(text + "\n")
