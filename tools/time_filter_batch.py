"""ndt_cloud_voxel_filter_batch / _clouds against the loops they replace, alternating in one process: tools/time_pairs.py's
scans (60 k raw points, the 0.5 m prefilter of ndt_omp_node), 8 / 16 / 40 / 128 clouds.  Two comparisons:
  buffer form  (one host buffer, one call)      vs  the loop of ndt_cloud_voxel_filter over the host arrays
  clouds form  (the resident raw clouds)        vs  the loop of ndt_cloud_voxel_filter_begin / _end over the same clouds
Medians of >= 5 runs after an untimed warm-up call (the batch asks the pool for sizes of its own).  Every run's outputs are
checked array_equal between the two forms of its comparison.  Prints one JSON line.
    python tools/time_filter_batch.py [runs (>= 5)] [raw points per scan]
--profile-one: the 40 scans, then ONE buffer-form call and nothing else (the kernel table in profiles/:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o filter_batch40 -- python tools/time_filter_batch.py --profile-one)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import clouds, ndt  # noqa: E402

profile_one = "--profile-one" in sys.argv
args = [a for a in sys.argv[1:] if a != "--profile-one"]
runs = max(5, int(args[0]) if len(args) > 0 else 7)
n_raw = int(args[1]) if len(args) > 1 else 60000
sizes = (8, 16, 40, 128)
n_scans = 40 if profile_one else max(sizes)
LEAF = 0.5

rng = np.random.default_rng(3)
world = clouds.target_surfaces(4 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
pose = np.eye(4)
scans = []
for k in range(n_scans):
    if k:
        pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
    pick = world[rng.choice(len(world), n_raw, replace=False)]
    scans.append((clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32))
g = ndt.NormalDistributionsTransform()
g.warmUp(65536)
if profile_one:
    outs, _ = g.voxelGridFilterClouds(scans, LEAF)
    print(json.dumps(dict(clouds=len(outs), points=int(sum(len(o) for o in outs)), **g.filterBatchDiag())))
    sys.exit(0)
raw_all = [g.uploadCloud(s) for s in scans]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(a, b))


def host_loop(cl):
    t0 = time.perf_counter()
    out = [g.voxelGridFilterCloud(c, LEAF)[0] for c in cl]
    return time.perf_counter() - t0, out


def host_batch(cl):
    t0 = time.perf_counter()
    out = g.voxelGridFilterClouds(cl, LEAF)[0]
    return time.perf_counter() - t0, out


def begin_end_loop(raw):
    t0 = time.perf_counter()
    out = []
    for c in raw:
        g.voxelGridFilterBegin(c, LEAF)
        out.append(g.voxelGridFilterEnd()[0])
    return time.perf_counter() - t0, out


def clouds_batch(raw):
    t0 = time.perf_counter()
    out = g.voxelGridFilterClouds(raw, LEAF)[0]
    return time.perf_counter() - t0, out


res = dict(metric="ms per call (median of %d runs after a warm-up)" % runs, raw_points=n_raw, leaf=LEAF, sizes={})
for n in sizes:
    cl, raw = scans[:n], raw_all[:n]
    for f, x in ((host_loop, cl), (host_batch, cl), (begin_end_loop, raw), (clouds_batch, raw)):
        f(x)  # warm-up
    t = {"loop": [], "buffer": [], "begin_end": [], "clouds": []}
    for _ in range(runs):  # alternating
        ta, a = host_loop(cl)
        tb, b = host_batch(cl)
        assert same(a, b), "buffer form differs from the loop"
        d_buf = g.filterBatchDiag()
        tc, c = begin_end_loop(raw)
        td, d = clouds_batch(raw)
        assert same(c, d), "clouds form differs from the loop"
        d_cl = g.filterBatchDiag()
        for key, v in (("loop", ta), ("buffer", tb), ("begin_end", tc), ("clouds", td)):
            t[key].append(v)
    med = {k: 1e3 * float(np.median(v)) for k, v in t.items()}
    res["sizes"][str(n)] = dict(host_loop_ms=round(med["loop"], 3), buffer_form_ms=round(med["buffer"], 3),
                                buffer_speedup=round(med["loop"] / med["buffer"], 2),
                                begin_end_loop_ms=round(med["begin_end"], 3), clouds_form_ms=round(med["clouds"], 3),
                                clouds_speedup=round(med["begin_end"] / med["clouds"], 2),
                                buffer_diag=d_buf, clouds_diag=d_cl, points_out=int(sum(len(x) for x in d)))
print(json.dumps(res))
