"""ndt_cloud_segment_plane (threshold 0.1 m, the z axis within 10 degrees, no refinement) at 256 / 1 024 / 4 096 hypotheses
beside two calls on the same resident cloud -- selectCloud(finite=True) and its voxel filter -- ndt_cloud_segment_plane_clouds
beside a loop of single calls, and the two forms of the count merge (one integer atomic per lane / partial rows summed by the
choice launch) alternating in one process.
    python tools/time_plane.py [runs (>= 5)]
Clouds: a tilted ground of 60 m x 60 m with +-3 cm noise and 30 % clutter in the 6 m above it (16 k, 100 k, 2 M points).  Many
clouds: 8 / 40 / 128 clouds of 16 k points, 256 hypotheses.  Every figure is a host clock around a call that returns after its
own work is done (the calls wait for their stream), the median of the runs after a warm-up of every call at that shape; the
calls of a shape alternate.  Prints one JSON line and writes it to profiles/plane_time.json.  Times only: no threshold is
checked, nobody had measured any of this."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import ndt  # noqa: E402

runs = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
SIDE = 60.0
HYPOTHESES = (256, 1024, 4096)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def med_us(ts):
    return round(1e6 * float(np.median(ts)), 2)


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.random((n, 2)) * SIDE - SIDE / 2
    z = 0.02 * u[:, 0] - 0.015 * u[:, 1] - 1.7 + rng.uniform(-0.03, 0.03, n)
    up = rng.random(n) < 0.3
    z[up] += 0.4 + 6.0 * rng.random(int(up.sum()))
    return np.column_stack([u, z]).astype(np.float32)


def spec(H, refine=False):
    return ndt.plane_spec(0.1, H, seed=1, axis=(0, 0, 1), eps_angle=math.radians(10.0), refine=refine)


def filter_resident(g, dc):
    g.voxelGridFilterBegin(dc, 0.5)
    return g.voxelGridFilterEnd()[0]


def alternate(calls):
    for fn in calls.values():
        fn()
        fn()
    ts = {k: [] for k in calls}
    for _ in range(runs):
        for k, fn in calls.items():
            ts[k].append(timed(fn)[0])
    return ts


def with_merge(form, fn):
    def call():
        os.environ["NDT_PLANE_MERGE"] = form      # (read at every call)
        try:
            return fn()
        finally:
            os.environ.pop("NDT_PLANE_MERGE", None)
    return call


g = ndt.NormalDistributionsTransform()
g.warmUp(65536)
out = dict(metric="median of %d runs after a warm-up, host clock around calls that return after their own work" % runs,
           spec="threshold 0.1 m, axis z within 10 degrees, seed 1", single={}, merge={}, many={})
for n in (16384, 100000, 2000000):
    dc = g.uploadCloud(cloud(n, n))
    calls = {"segment_%d" % H: (lambda H=H: g.segmentPlane(dc, spec(H))) for H in HYPOTHESES}
    calls["segment_256_result_only"] = lambda: g.segmentPlane(dc, spec(256), inliers=False, others=False)
    calls["segment_256_refined"] = lambda: g.segmentPlane(dc, spec(256, True))
    calls["select_finite"] = lambda: g.selectCloud(dc, finite=True)
    calls["voxel_filter_0p5"] = lambda: filter_resident(g, dc)
    ts = alternate(calls)
    row = dict(points=n)
    for H in HYPOTHESES:
        res = g.segmentPlane(dc, spec(H))[0]
        row["result_%d" % H] = dict(best_count=res["best_count"], n_rejected=res["n_rejected"], **g.planeDiag())
    for k in ts:
        row[k + "_us"] = med_us(ts[k])
        row[k + "_spread"] = round((max(ts[k]) - min(ts[k])) / float(np.median(ts[k])), 3)
    out["single"][str(n)] = row
    # the two count-merge forms, alternating: the counts call (models, counts, choice and the read-back of the rows)
    mrow = dict(points=n)
    for H in HYPOTHESES:
        forms = alternate({"atomic": with_merge("atomic", lambda H=H: g.planeCounts(dc, spec(H))),
                           "rows": with_merge("rows", lambda H=H: g.planeCounts(dc, spec(H)))})
        a, b = (with_merge(f, lambda H=H: g.planeCounts(dc, spec(H)))()[2] for f in ("atomic", "rows"))
        assert np.array_equal(a, b)
        mrow[str(H)] = dict(atomic_us=med_us(forms["atomic"]), rows_us=med_us(forms["rows"]))
    out["merge"][str(n)] = mrow
for m in (8, 40, 128):
    dcs = [g.uploadCloud(cloud(16384, 1000 + k)) for k in range(m)]
    ts = alternate(dict(clouds=lambda: g.segmentPlaneClouds(dcs, spec(256)), loop=lambda: [g.segmentPlane(dc, spec(256)) for dc in dcs]))
    g.segmentPlaneClouds(dcs, spec(256))
    out["many"][str(m)] = dict(n_clouds=m, points_each=16384, hypotheses=256, clouds_us=med_us(ts["clouds"]), loop_us=med_us(ts["loop"]),
                               us_per_cloud=round(med_us(ts["clouds"]) / m, 2), loop_us_per_cloud=round(med_us(ts["loop"]) / m, 2), **g.planeDiag())
text = json.dumps(out)
print(text)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "plane_time.json"), "w") as f:
    f.write(text + "\n")
