"""ndt_map_update_clouds / ndt_map_update_batch against the loops they replace, alternating in one process:
tools/time_filter_batch.py's scans (60 k raw points, prefiltered at the 0.5 m of ndt_omp_node) at the poses of their walk,
8 / 16 / 40 / 128 scans into an empty map.  Two comparisons, every run ending with ndt_map_size so both sides are complete:
  clouds form  (the resident filtered clouds, one call)  vs  the loop of ndt_map_update_cloud over the same clouds
  buffer form  (the host arrays, one buffer, one call)   vs  the loop of ndt_map_update over the host arrays
Medians of >= 5 runs after an untimed warm-up.  The one call's map is NOT the loop's (one filter of everything against
centroids of centroids); the two forms of the one call are checked array_equal, and so are the two loops.  Prints one JSON line.
    python tools/time_map_batch.py [runs (>= 5)] [raw points per scan]
--loop-only: only the two loops; --lib PATH: another build of the library (the yardstick: the parent commit's build, kept
side by side as tools/ab_libs.sh keeps its builds; with --loop-only it needs none of the new entry points).
--profile-one: the 40 scans, then ONE clouds-form call and nothing else (the kernel table in profiles/:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o map_batch40 -- python tools/time_map_batch.py --profile-one)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import _lib, clouds, ndt  # noqa: E402

flags = ("--profile-one", "--loop-only")
profile_one, loop_only = (f in sys.argv for f in flags)
args = [a for a in sys.argv[1:] if a not in flags]
if "--lib" in args:
    import ctypes
    i = args.index("--lib")
    _lib.LIB_PATH = os.path.abspath(args[i + 1])
    del args[i:i + 2]
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ndt_map_update_clouds", "ndt_map_update_batch", "ndt_diag_map_batch"):
        if loop_only and not hasattr(have, name):  # a build from before these entry points
            del _lib.SIGNATURES[name]
runs = max(5, int(args[0]) if len(args) > 0 else 7)
n_raw = int(args[1]) if len(args) > 1 else 60000
sizes = (8, 16, 40, 128)
n_scans = 40 if profile_one else max(sizes)
LEAF = 0.5

rng = np.random.default_rng(3)
world = clouds.target_surfaces(4 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
pose = np.eye(4)
scans, poses = [], []
for k in range(n_scans):
    if k:
        pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
    pick = world[rng.choice(len(world), n_raw, replace=False)]
    scans.append((clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32))
    poses.append(pose.astype(np.float32))
g = ndt.NormalDistributionsTransform()
g.warmUp(65536)
dev_all = [g.voxelGridFilterCloud(s, LEAF)[0] for s in scans]  # the prefiltered scans, resident ...
host_all = [d.numpy() for d in dev_all]                        # ... and on the host
if profile_one:
    n_map, ov = g.mapUpdateClouds(dev_all, poses, LEAF)
    print(json.dumps(dict(scans=len(dev_all), points_in=int(sum(len(c) for c in host_all)), map_points=n_map, **g.mapBatchDiag())))
    sys.exit(0)


def timed(fn):
    """an empty map (untimed), then fn and the map's size: the update is complete"""
    g.mapClear()
    t0 = time.perf_counter()
    fn()
    n = g.mapSize()
    return time.perf_counter() - t0, n


def cloud_loop(dev, P):
    for c, T in zip(dev, P):
        g.mapUpdateCloud(c, T, LEAF)


def host_loop(host, P):
    for c, T in zip(host, P):
        g.mapUpdate(c, T, LEAF)


res = dict(metric="ms per map of n scans, ndt_map_size included (median of %d runs after a warm-up)" % runs, raw_points=n_raw, leaf=LEAF,
           library=os.path.relpath(_lib.LIB_PATH, ROOT), sizes={})
for n in sizes:
    dev, host, P = dev_all[:n], host_all[:n], poses[:n]
    sides = [("cloud_loop", lambda: cloud_loop(dev, P)), ("host_loop", lambda: host_loop(host, P))]
    if not loop_only:
        sides += [("clouds_form", lambda: g.mapUpdateClouds(dev, P, LEAF)), ("buffer_form", lambda: g.mapUpdateBatch(host, P, LEAF))]
    for _, fn in sides:
        timed(fn)  # warm-up
    t = {k: [] for k, _ in sides}
    maps, diag = {}, {}
    for _ in range(runs):  # alternating
        for key, fn in sides:
            dt, n_map = timed(fn)
            t[key].append(dt)
            maps[key] = g.mapGet()
            if key.endswith("_form"):
                diag[key] = g.mapBatchDiag()
        assert np.array_equal(maps["cloud_loop"], maps["host_loop"]), "the two loops differ"
        if not loop_only:
            assert np.array_equal(maps["clouds_form"], maps["buffer_form"]), "the two forms of the one call differ"
            assert len(maps["clouds_form"]) == len(maps["cloud_loop"]), "the one call and the loop occupy different voxels"
    med = {k: 1e3 * float(np.median(v)) for k, v in t.items()}
    row = dict(points_in=int(sum(len(c) for c in host)), map_points=int(len(maps["cloud_loop"])),
               cloud_loop_ms=round(med["cloud_loop"], 3), host_loop_ms=round(med["host_loop"], 3))
    if not loop_only:
        row.update(clouds_form_ms=round(med["clouds_form"], 3), clouds_speedup=round(med["cloud_loop"] / med["clouds_form"], 2),
                   buffer_form_ms=round(med["buffer_form"], 3), buffer_speedup=round(med["host_loop"] / med["buffer_form"], 2),
                   clouds_diag=diag["clouds_form"], buffer_diag=diag["buffer_form"])
    res["sizes"][str(n)] = row
print(json.dumps(res))
