"""ndt_cloud_estimate_normals beside the parent's kernels that do the same search on the same resident cloud, and
ndt_cloud_estimate_normals_clouds beside a loop of single calls.
    python tools/time_normals.py [runs (>= 5)]          the timings -> profiles/normals_time.json
    python tools/time_normals.py trace <kind>           five calls of one kind (knn, radius_0.3, radius_1) and of its yardsticks at
        100 k points, no timing: for rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_normals.py trace <kind>
    python tools/time_normals.py merge <kind> <kernel_stats.csv>   that trace's kernel rows into profiles/normals_kernel_stats.csv
        and into the JSON (the kernels alone: k_normals beside k_knn_covariances and k_outlier_values)
KNN k = 20 beside GICP's covariance pass at k = 20 (gicp_covariances of a target set by reference: the pass alone, its index was
built by the setter, and 72 bytes per point come back to the host) and beside neighborValues STATISTICAL mean_k = 20; RADIUS at
0.3 m and 1.0 m beside neighborValues RADIUS with the same radius.  The normals and the neighbour values are written to device
memory (no download); a second normals figure includes the download of the 16-byte records and the counts.  Every normals and
neighbour-values call builds its own point index.  Clouds: a street scene -- 60 % ground with 1 cm noise, boxes of car to van size
with points on their faces, 5 % stray points -- of 16 k, 100 k and 2 M points at about 20 ground points per square metre.  Many
clouds: 8 / 40 / 128 scenes of 16 k points, KNN k = 20.  Every figure is a host clock around a call that returns after its own work
is done, the median of the runs after a warm-up of every call at that shape; the calls of a shape alternate; the spread is (max -
min) / median of the same runs.  Times only: no threshold is checked, nobody had measured any of this."""
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyslam_amd import gicp, ndt  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "normals_time.json")
K = 20
RADII = (0.3, 1.0)


def scene(n, seed):
    rng = np.random.default_rng(seed)
    n_stray = n // 20
    n_ground = (n * 3) // 5
    n_box = n - n_ground - n_stray
    side = float(np.sqrt(n_ground / 20.0))
    ground = np.column_stack([rng.random((n_ground, 2)) * side, 0.01 * rng.standard_normal(n_ground)])
    boxes = max(4, n_box // 600)
    centre = np.column_stack([rng.random((boxes, 2)) * side, np.zeros(boxes)])
    half = np.column_stack([1.0 + 1.5 * rng.random(boxes), 0.8 + 0.4 * rng.random(boxes), 0.7 + 0.6 * rng.random(boxes)])
    which = rng.integers(0, boxes, n_box)
    p = (2.0 * rng.random((n_box, 3)) - 1.0) * half[which]
    face = rng.integers(0, 3, n_box)
    p[np.arange(n_box), face] = np.where(rng.random(n_box) < 0.5, -1.0, 1.0) * half[which, face]  # onto a face of the box
    stray = np.column_stack([rng.random((n_stray, 2)) * side, 8.0 * rng.random(n_stray)])
    out = np.concatenate([ground, p + centre[which] + np.array([0.0, 0.0, 1.3]), stray]).astype(np.float32)
    out -= np.array([side / 2, side / 2, 1.8], np.float32)  # the sensor at the origin, 1.8 m above the ground
    return out[rng.permutation(len(out))]


class DeviceBuffer:
    """bytes of HBM through the HIP runtime the library is linked to"""

    def __init__(self, nbytes):
        linked = [m.group(1) for m in re.finditer(r"(/\S*libamdhip64\.so[.\d]*)", open("/proc/self/maps").read()) if "/torch/" not in m.group(1)]
        self.hip = C.CDLL(linked[0] if linked else "libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipFree.argtypes = [C.c_void_p]
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), nbytes) == 0
        self.p = p.value

    def free(self):
        self.hip.hipFree(self.p)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def med_us(ts):
    return round(1e6 * float(np.median(ts)), 2)


def spread(ts):
    return round((max(ts) - min(ts)) / float(np.median(ts)), 3)


def calls_of(g, gi, dc, buf):
    """name -> (call, which diag to read scanned_queries from)"""
    calls = {"normals_knn": (lambda: g.estimateNormals(dc, k=K, device=buf.p), g.normalDiag),
             "normals_knn_to_host": (lambda: g.estimateNormals(dc, k=K), g.normalDiag),
             "gicp_covariances": (lambda: gi.covariances(0), None),
             "neighbor_values_stat": (lambda: g.neighborValues(dc, mean_k=K, stddev_mul=1.0, device=buf.p), g.outlierDiag)}
    for r in RADII:
        calls["normals_radius_%g" % r] = (lambda r=r: g.estimateNormals(dc, radius=r, device=buf.p), g.normalDiag)
        calls["neighbor_values_radius_%g" % r] = (lambda r=r: g.neighborValues(dc, radius=r, min_neighbors=3, device=buf.p), g.outlierDiag)
    return calls


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "merge":
        return merge(sys.argv[2], sys.argv[3])
    g = ndt.NormalDistributionsTransform()
    gi = gicp.GeneralizedIterativeClosestPoint()
    gi.setCorrespondenceRandomness(K)
    g.warmUp(65536)
    if mode == "trace":
        dc = g.uploadCloud(scene(100000, 100000))
        gi.setInputTargetCloud(dc)
        buf = DeviceBuffer(20 * len(dc))
        kind = sys.argv[2]
        pick = ("normals_knn", "gicp_covariances", "neighbor_values_stat") if kind == "knn" else tuple(
            k for k in calls_of(g, gi, dc, buf) if k.endswith(kind) and "radius" in k)
        assert len(pick) >= 2, kind
        for name in pick:
            for _ in range(5):
                calls_of(g, gi, dc, buf)[name][0]()
        buf.free()
        return
    runs = max(5, int(mode) if mode else 7)
    out = dict(metric="median of %d runs after a warm-up, host clock around calls that return after their own work; spread = (max - min) / median" % runs,
               spec="KNN k = %d (the point included), RADIUS %s m, min_neighbors 3, viewpoint the origin; neighborValues: mean_k %d / the same radius; "
                    "gicp_covariances: k = %d, the pass alone (index built by the setter), 72 bytes per point downloaded" % (K, list(RADII), K, K),
               single={}, many={})
    for n in (16384, 100000, 2000000):
        dc = g.uploadCloud(scene(n, n))
        t_index = timed(lambda: gi.setInputTargetCloud(dc))
        buf = DeviceBuffer(20 * n)
        calls = calls_of(g, gi, dc, buf)
        for fn, _ in calls.values():
            fn()
            fn()
        ts = {k: [] for k in calls}
        scanned = {}
        for _ in range(runs):  # alternating
            for k, (fn, diag) in calls.items():
                ts[k].append(timed(fn))
                if diag is not None:
                    scanned[k] = diag()["scanned_queries"]
        row = dict(points=n, gicp_set_input_target_cloud_us=round(1e6 * t_index, 2), scanned_queries=scanned)
        for k in ts:
            row[k + "_us"] = med_us(ts[k])
            row[k + "_spread"] = spread(ts[k])
        row["normals_knn_over_gicp_covariances"] = round(row["normals_knn_us"] / row["gicp_covariances_us"], 3)
        row["normals_knn_over_neighbor_values_stat"] = round(row["normals_knn_us"] / row["neighbor_values_stat_us"], 3)
        for r in RADII:
            row["normals_radius_%g_over_neighbor_values" % r] = round(row["normals_radius_%g_us" % r] / row["neighbor_values_radius_%g_us" % r], 3)
        st = g.estimateNormals(dc, k=K)[2]
        row["stats_knn"] = st
        for r in RADII:
            row["stats_radius_%g" % r] = g.estimateNormals(dc, radius=r)[2]
        out["single"][str(n)] = row
        print("single", n, "done", file=sys.stderr, flush=True)
        buf.free()
    for m in (8, 40, 128):
        dcs = [g.uploadCloud(scene(16384, 1000 + k)) for k in range(m)]
        calls = dict(clouds=lambda: g.estimateNormalsClouds(dcs, k=K), loop=lambda: [g.estimateNormals(dc, k=K) for dc in dcs])
        for fn in calls.values():
            fn()
            fn()
        ts = {k: [] for k in calls}
        for _ in range(runs):
            for k, fn in calls.items():
                ts[k].append(timed(fn))
        g.estimateNormalsClouds(dcs, k=K)
        out["many"][str(m)] = dict(clouds=m, points_each=16384, clouds_us=med_us(ts["clouds"]), clouds_spread=spread(ts["clouds"]), loop_us=med_us(ts["loop"]),
                                   loop_spread=spread(ts["loop"]), us_per_cloud=round(med_us(ts["clouds"]) / m, 2),
                                   loop_us_per_cloud=round(med_us(ts["loop"]) / m, 2), **g.normalDiag())
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text + "\n")


def merge(kind, stats_csv):
    """the rows of the kernels of interest of a rocprofv3 kernel_stats.csv (a trace mode's run) into profiles/"""
    import csv
    keep = ("k_normals", "k_normal_order_keys", "k_knn_covariances", "k_outlier_values")
    rows = []
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            short = next((k for k in keep if k in name), None)
            if short is None:
                continue
            rows.append((short, int(r["Calls"]), int(r["TotalDurationNs"]), float(r["AverageNs"]), int(r["MinNs"]), int(r["MaxNs"])))
    path = os.path.join(ROOT, "profiles", "normals_kernel_stats.csv")
    fresh = not os.path.exists(path)
    with open(path, "a") as f:
        if fresh:
            f.write("shape (five calls of the normals and of each yardstick),kernel,Calls,TotalDurationNs,AverageNs,MinNs,MaxNs\n")
        for r in rows:
            f.write("100000 points %s,%s,%d,%d,%.1f,%d,%d\n" % ((kind,) + r))
    with open(OUT) as f:
        out = json.loads(f.read())
    out.setdefault("kernel_trace_100000_points", {})[kind] = {r[0]: dict(calls=r[1], average_us=round(r[3] / 1e3, 2)) for r in rows}
    with open(OUT, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
