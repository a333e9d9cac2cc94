"""ndt_cloud_deskew beside two yardsticks on the same resident cloud -- ndt_cloud_select with no test enabled (a copy of the
records through two launches) and the voxel filter (strictly more work on the same bytes) -- and ndt_cloud_deskew_clouds beside a
loop of single calls.
    python tools/time_deskew.py [runs (>= 5)]
Clouds: uniform points in a 60 m cube about the sensor (16 k, 100 k, 2 M points), times uniform over a 0.1 s sweep at an
epoch-sized offset, already in device memory (the upload of host times is timed as a call of its own); the motion is 1 m and
0.3 rad over the sweep.  Many clouds: 8 / 40 / 128 clouds of 16 k points, times on the host as the many-clouds call takes them.
Every figure is a host clock around a call that returns after its own work is done, the median of the runs after a warm-up of
every call at that shape; the calls of a shape alternate, and deskew, the copy and the filter are then also timed back to back
with themselves.  Prints one JSON line and writes it to profiles/deskew_time.json.  No threshold is checked: nobody had
measured any of this."""
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import _lib, ndt  # noqa: E402

runs = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 9)
SIDE = 60.0
T_BEGIN, T_END = 1.7e9, 1.7e9 + 0.1


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def med_us(ts):
    return round(1e6 * float(np.median(ts)), 2)


def cloud(n, seed):
    return np.random.default_rng(seed).uniform(-SIDE / 2, SIDE / 2, (n, 3)).astype(np.float32)


def times_of(n, seed):
    return np.random.default_rng(seed + 5).uniform(T_BEGIN, T_END, n)


def filter_resident(g, dc):
    g.voxelGridFilterBegin(dc, 0.5)
    return g.voxelGridFilterEnd()[0]


class DeviceDoubles:
    """float64 arrays in HBM, through the HIP runtime the library is linked to"""

    def __init__(self):
        assert _lib.lib() is not None
        linked = [m.group(1) for m in re.finditer(r"(/\S*libamdhip64\.so[.\d]*)", open("/proc/self/maps").read()) if "/torch/" not in m.group(1)]
        self.hip = C.CDLL(linked[0] if linked else "libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
        assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p.value


T = np.eye(4)
T[:3, :3] = [[np.cos(0.3), -np.sin(0.3), 0], [np.sin(0.3), np.cos(0.3), 0], [0, 0, 1]]
T[:3, 3] = [1.0, 0.05, 0.0]
motion = ndt.host_deskew_motion(T, T_BEGIN, T_END)
g = ndt.NormalDistributionsTransform()
g.warmUp(65536)
dev = DeviceDoubles()
out = dict(metric="median of %d runs after a warm-up, host clock around calls that return after their own work" % runs,
           motion="1 m and 0.3 rad about z over a 0.1 s sweep at t = 1.7e9 s; uniform points in a %g m cube" % SIDE, single={}, many={})
for n in (16384, 100000, 2000000):
    dc = g.uploadCloud(cloud(n, n))
    ts_host = times_of(n, n)
    ts_dev = dev.put(ts_host)
    calls = dict(deskew=lambda: g.deskewCloud(dc, motion, ts_dev, device=True), deskew_host_times=lambda: g.deskewCloud(dc, motion, ts_host),
                 select_copy=lambda: g.selectCloud(dc), voxel_filter_0p5=lambda: filter_resident(g, dc))
    for fn in calls.values():
        fn()
        fn()
    ts = {k: [] for k in calls}
    for _ in range(runs):  # alternating
        for k, fn in calls.items():
            ts[k].append(timed(fn)[0])
    for k in ("deskew", "select_copy", "voxel_filter_0p5"):
        ts[k + "_back_to_back"] = [timed(calls[k])[0] for _ in range(runs)]
    g.deskewCloud(dc, motion, ts_dev, device=True)
    row = dict(points=n, blocks=g.deskewDiag()["blocks"], launches=g.deskewDiag()["launches"], filtered_points=len(filter_resident(g, dc)))
    for k in ts:
        row[k + "_us"] = med_us(ts[k])
        row[k + "_spread"] = round((max(ts[k]) - min(ts[k])) / float(np.median(ts[k])), 3)
    moved = 40.0 * n  # bytes the launch moves: a record in, a time in, a record out
    row["deskew_gb_per_s"] = round(moved / float(np.median(ts["deskew"])) / 1e9, 1)
    row["deskew_back_to_back_gb_per_s"] = round(moved / float(np.median(ts["deskew_back_to_back"])) / 1e9, 1)
    row["deskew_over_select_copy"] = round(float(np.median(ts["deskew_back_to_back"])) / float(np.median(ts["select_copy_back_to_back"])), 3)
    row["deskew_over_filter"] = round(float(np.median(ts["deskew_back_to_back"])) / float(np.median(ts["voxel_filter_0p5_back_to_back"])), 3)
    out["single"][str(n)] = row
for m in (8, 40, 128):
    dcs = [g.uploadCloud(cloud(16384, 1000 + k)) for k in range(m)]
    tss = [times_of(16384, 1000 + k) for k in range(m)]
    packed = np.concatenate(tss)
    ms = [motion] * m
    calls = dict(clouds=lambda: g.deskewClouds(dcs, ms, packed), loop=lambda: [g.deskewCloud(dc, motion, t) for dc, t in zip(dcs, tss)])
    for fn in calls.values():
        fn()
        fn()
    ts = {k: [] for k in calls}
    for _ in range(runs):
        for k, fn in calls.items():
            ts[k].append(timed(fn)[0])
    g.deskewClouds(dcs, ms, packed)
    d = g.deskewDiag()
    out["many"][str(m)] = dict(clouds=m, points_each=16384, clouds_us=med_us(ts["clouds"]), loop_us=med_us(ts["loop"]),
                               us_per_cloud=round(med_us(ts["clouds"]) / m, 2), loop_us_per_cloud=round(med_us(ts["loop"]) / m, 2),
                               launches=d["launches"], blocks=d["blocks"])
text = json.dumps(out)
print(text)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "deskew_time.json"), "w") as f:
    f.write(text + "\n")
