"""Per-update time and device memory of the accumulating target (ndt_target_accumulate_cloud) against the route a caller
had before it for the same target: keep every posed point in HBM, concatenate, ndt_set_input_target_device of the whole
buffer before each scan.  The map-sequence shape: tools/time_map_batch.py's scans (60 k raw points, ~39 k after the 0.5 m
prefilter) at the poses of their walk, 1 m voxels; targets of 8 / 40 / 128 / 512 accumulated scans.
  accumulate   the REAL updates of one run: the time of the call that adds scan k to a target of k scans, median over the
               seven updates k = S - 3 .. S + 3 around each size S
  rebuild      ndt_set_input_target_device over the first S + 1 posed scans of one device buffer, median of >= 7 calls
               (the append of the new scan to the buffer -- its transform and copy -- is NOT counted: in the rebuild's favour)
Every timed call is followed by hipDeviceSynchronize (inside the timed region, both routes).  Device memory: what
hipMemGetInfo reports as used beyond the state before the route started (the library's pool keeps its scratch blocks:
they count), and for the rebuild route the buffer's 16 B per point besides.  The two routes run one after the other in one
process; the grids are compared leaf count for leaf count.  Prints one JSON line.
    python tools/time_target_accumulate.py [runs (>= 7)] [raw points per scan]"""
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
sizes = (8, 40, 128, 512)
n_scans = max(sizes) + 4
LEAF = 0.5

rng = np.random.default_rng(3)
world = clouds.target_surfaces(4 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
pose = np.eye(4)
g = ndt.NormalDistributionsTransform()
g.warmUp(65536)
# the HIP runtime the library itself is linked to (a second instance of the runtime would see another context)
linked = [m.group(1) for m in re.finditer(r"(/\S*libamdhip64\.so[.\d]*)", open("/proc/self/maps").read()) if "/torch/" not in m.group(1)]
hip = C.CDLL(linked[0] if linked else "libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]


def used_bytes():
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


filt, poses = [], []
for k in range(n_scans):
    if k:
        pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
    pick = world[rng.choice(len(world), n_raw, replace=False)]
    scan = (clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32)
    dc = g.voxelGridFilterCloud(scan, LEAF)[0]
    filt.append(dc.numpy())
    dc.release()
    poses.append(pose.astype(np.float32))
del g

# ---- the accumulating target: one run, every update timed
base = used_bytes()
a = ndt.NormalDistributionsTransform()
a.warmUp(65536)
dev = [a.uploadCloud(c) for c in filt]
resident = used_bytes() - base       # the scans themselves, resident for both the timing and the upload: not the target's
t_acc, acc_mem, acc_state = [], {}, {}
for k in range(n_scans):
    t0 = time.perf_counter()
    a.targetAccumulateCloud(dev[k], poses[k])
    hip.hipDeviceSynchronize()
    t_acc.append(time.perf_counter() - t0)
    if k in sizes:  # (the target now holds S + 1 scans: what the rebuild of the same step builds)
        acc_mem[k] = used_bytes() - base - resident
        acc_state[k] = dict(a.targetAccumulated(), **a.targetAccumulateDiag())
final_counts = a.grid_counts()
for d in dev:
    d.release()
del a, dev

# ---- the rebuild route: every posed point kept in HBM, the grid rebuilt from the growing buffer
posed = []
for c, T in zip(filt, poses):
    p = (c[:, :3].astype(np.float32) @ T[:3, :3].T.astype(np.float32) + T[:3, 3].astype(np.float32)).astype(np.float32)
    posed.append(np.ascontiguousarray(np.c_[p, np.ones(len(p), np.float32)], dtype=np.float32))
offsets = np.concatenate([[0], np.cumsum([len(p) for p in posed])])
base = used_bytes()
buf = C.c_void_p()
assert hip.hipMalloc(C.byref(buf), int(offsets[-1]) * 16) == 0
for p, o in zip(posed, offsets):
    assert hip.hipMemcpy(C.c_void_p(buf.value + int(o) * 16), p.ctypes.data, p.nbytes, 1) == 0
buffer_bytes = used_bytes() - base
b = ndt.NormalDistributionsTransform()
b.warmUp(65536)
res = dict(metric="ms per update of a target of S accumulated scans, hipDeviceSynchronize included", raw_points=n_raw, prefilter_leaf=LEAF,
           resolution=1.0, runs=runs, compared_route="ndt_set_input_target_device of the concatenation of all posed scans kept in HBM "
           "(the append of the new scan not counted)", library=os.path.relpath(_lib.LIB_PATH, ROOT), sizes={})
for S in sizes:
    n_pts = int(offsets[S + 1])
    t = []
    for _ in range(runs + 1):  # (the first call is the warm-up: the pool finds its blocks)
        t0 = time.perf_counter()
        b.setInputTargetDevice(buf.value, n_pts, 16)
        hip.hipDeviceSynchronize()
        t.append(time.perf_counter() - t0)
    around = t_acc[S - 3:S + 4]
    row = dict(points_in_target=int(offsets[S]), points_per_update=int(np.mean([len(c) for c in filt[S - 3:S + 4]])),
               accumulate_ms=round(1e3 * float(np.median(around)), 3), accumulate_min_ms=round(1e3 * float(np.min(around)), 3),
               accumulate_max_ms=round(1e3 * float(np.max(around)), 3),
               rebuild_ms=round(1e3 * float(np.median(t[1:])), 3), rebuild_min_ms=round(1e3 * float(np.min(t[1:])), 3),
               rebuild_max_ms=round(1e3 * float(np.max(t[1:])), 3),
               accumulate_device_bytes=int(acc_mem[S]), rebuild_points_bytes=n_pts * 16, rebuild_handle_bytes=int(used_bytes() - base - buffer_bytes),
               accumulate_state=acc_state[S], rebuild_leaves=b.grid_counts()["n_leaves"])
    row["speedup"] = round(row["rebuild_ms"] / row["accumulate_ms"], 2)
    res["sizes"][str(S)] = row
res["first_update_ms"] = round(1e3 * t_acc[0], 3)
res["rebuild_buffer_bytes_all_scans"] = int(buffer_bytes)
res["accumulated_leaves_all_scans"] = final_counts["n_leaves"]
hip.hipFree(buf)
print(json.dumps(res))
