"""Cost of moving an accumulated target out of a handle and into another one (ndt_target_accumulate_export / _import /
_save / _load), beside the only route there was before: accumulating every posed scan again (ndt_target_accumulate_clouds).
Targets of S = 8 / 40 / 128 / 512 accumulated scans -- the scans of tools/time_target_accumulate.py (60 k raw points, ~39 k
after the 0.5 m prefilter, at the poses of their walk, 1 m voxels).  Per size the target is built once in one handle; export
and save are timed on it, import, load and the re-accumulation on a second handle that is reset before every call.  Host clock
around calls that end in a device synchronise (hipDeviceSynchronize inside the timed region), median of `runs` after one
warm-up call each.  Prints one JSON line (profiles/target_persist_time.json).
    python tools/time_target_persist.py [runs (>= 7)] [raw points per scan]"""
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import _lib, clouds, ndt  # noqa: E402

runs = max(7, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
n_raw = int(sys.argv[2]) if len(sys.argv) > 2 else 60000
sizes = (8, 40, 128, 512)
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
for k in range(max(sizes)):
    if k:
        pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
    pick = world[rng.choice(len(world), n_raw, replace=False)]
    dev.append(up.voxelGridFilterCloud((clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32), LEAF)[0])
    poses.append(pose.astype(np.float32))
res = dict(metric="ms per call, hipDeviceSynchronize included", raw_points=n_raw, prefilter_leaf=LEAF, resolution=1.0, runs=runs,
           library=os.path.relpath(_lib.LIB_PATH, ROOT), sizes={})
a, b = ndt.NormalDistributionsTransform(), ndt.NormalDistributionsTransform()
a.warmUp(65536)
b.warmUp(65536)
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "map.ndtacc")
    for S in sizes:
        a.targetAccumulateReset()
        for k in range(S):
            a.targetAccumulateCloud(dev[k], poses[k])
        hip.hipDeviceSynchronize()
        blobs = []
        t_export = [timed(lambda: blobs.append(a.targetAccumulateExport())) for _ in range(runs + 1)][1:]
        t_save = [timed(lambda: a.targetAccumulateSave(path)) for _ in range(runs + 1)][1:]
        blob = blobs[-1]
        t_import, t_load, t_again = [], [], []
        for r in range(runs + 1):
            for t, call in ((t_import, lambda: b.targetAccumulateImport(blob)), (t_load, lambda: b.targetAccumulateLoad(path)),
                            (t_again, lambda: b.targetAccumulateClouds(dev[:S], poses[:S]))):
                b.targetAccumulateReset()
                hip.hipDeviceSynchronize()
                dt = timed(call)
                if r:
                    t.append(dt)
                assert b.targetAccumulateExport() == blob   # every route gives the same target
        st = a.targetAccumulated()
        row = dict(voxels=st["voxels"], points=st["points"], blob_bytes=len(blob), export=stats(t_export), save=stats(t_save),
                   **{"import": stats(t_import)}, load=stats(t_load), accumulate_all_scans_again=stats(t_again),
                   export_launches=a.targetExportDiag()["launches"])
        row["again_over_import"] = round(row["accumulate_all_scans_again"]["median_ms"] / row["import"]["median_ms"], 2)
        res["sizes"][str(S)] = row
print(json.dumps(res))
