"""Cost of cropping the accumulating target (ndt_target_accumulate_crop), and what a window does to a long run.
 A  one crop that removes about a tenth of the voxels, of a target of S = 8 / 40 / 128 / 512 accumulated scans -- the scans of
    tools/time_target_accumulate.py (60 k raw points, ~39 k after the 0.5 m prefilter, at the poses of their walk, 1 m
    voxels) -- beside one ndt_target_accumulate_cloud update of the same target (scan S into the target of S scans) in the
    same sitting.  Per size the target is built `runs + 1` times in one handle (reset in between, so the pool holds the
    blocks; the first build is the warm-up); every timed call is followed by hipDeviceSynchronize inside the timed region.
 B  a marching trajectory of 512 scans (0.5 m per scan along x through a world tiled every 60 m), one handle with a window of
    half-side 30 m cropped after every update, one without: the time of an update (and of the crop), the time of ndt_align
    of the next scan from the previous pose, voxels and the device memory the handle's route added (hipMemGetInfo: the
    library's pool keeps freed blocks, they count).  The unwindowed handle is the behaviour before the crop existed.
Prints one JSON line.
    python tools/time_target_crop.py [runs (>= 7)] [raw points per scan] [scans of part B]"""
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
n_march = int(sys.argv[3]) if len(sys.argv) > 3 else 512
sizes = (8, 40, 128, 512)
LEAF, HALF = 0.5, 30.0

up = ndt.NormalDistributionsTransform()   # makes and holds every resident cloud
up.warmUp(65536)
linked = [m.group(1) for m in re.finditer(r"(/\S*libamdhip64\.so[.\d]*)", open("/proc/self/maps").read()) if "/torch/" not in m.group(1)]
hip = C.CDLL(linked[0] if linked else "libamdhip64.so")
hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]


def used_bytes():
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


def timed(call):
    t0 = time.perf_counter()
    call()
    hip.hipDeviceSynchronize()
    return time.perf_counter() - t0


def stats(t):
    return dict(median_ms=round(1e3 * float(np.median(t)), 3), min_ms=round(1e3 * float(np.min(t)), 3), max_ms=round(1e3 * float(np.max(t)), 3))


def prefiltered(scan):
    dc = up.voxelGridFilterCloud(scan, LEAF)[0]
    return dc


# ---- A: the cost of one crop beside one update
rng = np.random.default_rng(3)
world = clouds.target_surfaces(4 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
pose = np.eye(4)
dev, poses = [], []
for k in range(max(sizes) + 1):
    if k:
        pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
    pick = world[rng.choice(len(world), n_raw, replace=False)]
    dev.append(prefiltered((clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32)))
    poses.append(pose.astype(np.float32))
res = dict(metric="ms per call, hipDeviceSynchronize included", raw_points=n_raw, prefilter_leaf=LEAF, resolution=1.0, runs=runs,
           library=os.path.relpath(_lib.LIB_PATH, ROOT), crop={}, march={})
a = ndt.NormalDistributionsTransform()
a.warmUp(65536)
for S in sizes:
    t_update, t_crop, t_keep, bound, row = [], [], [], None, {}
    for r in range(runs + 1):
        a.targetAccumulateReset()
        for k in range(S):
            a.targetAccumulateCloud(dev[k], poses[k])
        hip.hipDeviceSynchronize()
        tu = timed(lambda: a.targetAccumulateCloud(dev[S], poses[S]))
        if bound is None:   # the x below which a tenth of the voxels lie
            gr = a.grid()
            x = gr["idx"] % int(gr["div_b"][0]) + int(gr["min_b"][0])
            bound = float(np.quantile(x, 0.1)) + 0.5
        inf = np.inf
        tk = timed(lambda: a.targetAccumulateCrop([-inf, -inf, -inf], [inf, inf, inf]))   # removes nothing: mark, scan, read-back
        before = a.targetAccumulated()
        tc = timed(lambda: a.targetAccumulateCrop([bound, -inf, -inf], [inf, inf, inf]))
        if r:   # (the first build is the warm-up: the pool finds its blocks)
            t_update.append(tu)
            t_crop.append(tc)
            t_keep.append(tk)
        row = dict(voxels_before=before["voxels"], points_before=before["points"], **a.targetCropDiag())
    row.update(points_per_update=int(dev[S].numpy().shape[0]), update=stats(t_update), crop=stats(t_crop),
               crop_that_removes_nothing=stats(t_keep))
    row["crop_over_update"] = round(row["crop"]["median_ms"] / row["update"]["median_ms"], 2)
    res["crop"][str(S)] = row
del a
for d in dev:
    d.release()

# ---- B: a marching trajectory, windowed against unwindowed
rng = np.random.default_rng(5)
dev, poses = [], []
for k in range(n_march + 1):
    x = 0.5 * k
    T = clouds.make_T([x, 0.05 * np.sin(0.1 * k), 0.0], np.deg2rad([0.0, 0.0, 2.0 * np.sin(0.05 * k)]))
    tile = 60.0 * np.round(x / 60.0)
    near = np.concatenate([world + np.float32([tile + s, 0, 0]) for s in (-60.0, 0.0, 60.0)])
    near = near[np.abs(near[:, 0] - x) < 30.0]
    pick = near[rng.choice(len(near), n_raw, replace=False)]
    dev.append(prefiltered((clouds.apply_T(np.linalg.inv(T), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32)))
    poses.append(T.astype(np.float32))
for name, window in (("unwindowed", 0.0), ("windowed", HALF)):
    base = used_bytes()
    h = ndt.NormalDistributionsTransform()
    h.warmUp(65536)
    h.setNeighborhoodSearchMethod(ndt.DIRECT7)
    warm = used_bytes() - base
    t_up, t_crop, t_align, iters, voxels = [], [], [], [], []
    for k in range(n_march):
        t_up.append(timed(lambda: h.targetAccumulateCloud(dev[k], poses[k])))
        if window:
            t = poses[k][:3, 3]
            t_crop.append(timed(lambda: h.targetAccumulateCrop(t - window, t + window)))
        voxels.append(h.targetAccumulated()["voxels"])
        h.setInputSourceCloud(dev[k + 1])
        t_align.append(timed(lambda: h.align(poses[k])))
        iters.append(h.getFinalNumIteration())
    tail = slice(n_march - 64, n_march)
    gi = h.grid_counts()
    lat = h.grid()
    row = dict(window_half_side=window, update_last64=stats(t_up[tail]), update_all=stats(t_up), align_last64=stats(t_align[tail]),
               align_first64=stats(t_align[8:72]), iterations_last64=float(np.mean(iters[tail])), voxels_end=voxels[-1], voxels_max=max(voxels),
               box_cells_end=[int(v) for v in lat["div_b"]], leaves=gi["n_leaves"], device_bytes_beyond_warm_up=int(used_bytes() - base - warm))
    if window:
        row.update(crop_last64=stats(t_crop[tail]), crop_all=stats(t_crop), last_crop=h.targetCropDiag())
    res["march"][name] = row
    del h
res["march"]["scans"] = n_march
res["march"]["step_m"] = 0.5
print(json.dumps(res))
