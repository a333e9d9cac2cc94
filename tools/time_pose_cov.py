"""One ndt_pose_covariance beside one ndt_eval_hessian_f64 and one ndt_align -- existing code, the yardsticks -- on the same
handle, alternating in one process.
    python tools/time_pose_cov.py [runs (>= 5)]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_pose_cov.py trace     (a run of its own: two calls per shape, no timing)
Shapes: the bundled pair (15 950 source points against its 15 772-point target) and a synthetic pair of 100 k source points
against a 39 k-point target (60 k raw points filtered at 0.5 m), resolution 1.0, DIRECT7, at the registering pose.  Every
figure is a host clock around a call that ends with its result on the host, the median of the runs after a warm-up of the
three calls at that shape.  ndt_pose_covariance launches k_hessian64 AND k_grad_outer, so (covariance - hessian) is what the new
kernel, its reduction and the host algebra add.  Prints one JSON line and writes it to profiles/pose_cov_time.json; the
expectation it reports on (that difference no longer than the Hessian call, k_grad_outer doing strictly less f64 work per
neighbour than k_hessian64) is checked here, not tuned for."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from toyslam_amd import _lib, clouds, ndt  # noqa: E402

trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
runs = 2 if trace else max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 9)


def handle():
    g = ndt.NormalDistributionsTransform()
    g.setResolution(1.0)
    g.setStepSize(0.1)
    g.setTransformationEpsilon(0.01)
    g.setMaximumIterations(64)
    g.setNeighborhoodSearchMethod(_lib.DIRECT7)
    return g


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def pair_scene():
    d = np.load(os.path.join(ROOT, "tests", "golden", "pair_0p1.npz"))
    with open(os.path.join(ROOT, "tests", "golden", "oracle_golden.json")) as f:
        T_true = np.asarray(json.load(f)["aligns"]["DIRECT7/default"]["T"], dtype=np.float64)
    return d["target"], d["source"], T_true


def synthetic_scene():
    rng = np.random.default_rng(5)
    world = clouds.target_surfaces(400000, seed=77, extent=60.0)[:, :3].astype(np.float32)
    g = handle()
    target = g.voxelGridFilter(world[rng.choice(len(world), 60000, replace=False)], 0.5)
    T_true = clouds.make_T([0.6, -0.4, 0.05], np.deg2rad([0.2, -0.1, 3.0]))
    raw = clouds.apply_T(np.linalg.inv(T_true), world[rng.choice(len(world), 100000, replace=False)]) + rng.normal(0, 0.01, (100000, 3))
    return target, np.ascontiguousarray(raw, dtype=np.float32), T_true


out = dict(metric="median of %d runs after a warm-up, host clock around calls that end with the result on the host" % runs,
           search="DIRECT7", shapes={})
holds = True
for name, (target, source, T_true) in (("pair", pair_scene()), ("synthetic_100k", synthetic_scene())):
    g = handle()
    g.warmUp(max(65536, len(source)))
    g.setInputTarget(target)
    g.setInputSource(source)
    guess = T_true.astype(np.float32)
    g.align(guess)
    T = g.getFinalTransformation()
    p = ndt.host_matrix_to_pose(T)
    g.poseCovariance(T)
    g.hessian_f64(p)  # warm-up of the three at this shape
    tc, th, ta = [], [], []
    for _ in range(runs):  # alternating
        tc.append(timed(lambda: g.poseCovariance(T))[0])
        th.append(timed(lambda: g.hessian_f64(p))[0])
        ta.append(timed(lambda: g.align(guess))[0])
    cov, info = g.poseCovariance(T, info=True)
    mc, mh, ma = (float(np.median(x)) for x in (tc, th, ta))
    holds = holds and (mc - mh) <= mh
    out["shapes"][name] = dict(
        source_points=len(source), target_points=len(target),
        pose_covariance_us=round(1e6 * mc, 2), eval_hessian_f64_us=round(1e6 * mh, 2), align_us=round(1e6 * ma, 2),
        covariance_minus_hessian_us=round(1e6 * (mc - mh), 2), covariance_over_align=round(mc / ma, 4),
        pose_covariance_spread=round((max(tc) - min(tc)) / mc, 4), eval_hessian_f64_spread=round((max(th) - min(th)) / mh, 4),
        align_spread=round((max(ta) - min(ta)) / ma, 4), iterations=int(g.getFinalNumIteration()), converged=bool(g.hasConverged()),
        launches=g.poseCovarianceLaunches()[0], blocks=g.poseCovarianceLaunches()[1], n_found=info["n_found"],
        indefinite=info["indefinite"], sigma=[float("%.6g" % x) for x in np.sqrt(np.diag(cov))],
        eig_min=float("%.6g" % info["eig_min"]), eig_max=float("%.6g" % info["eig_max"]))
out["expectation_grad_outer_no_longer_than_hessian64"] = bool(holds)
text = json.dumps(out)
print(text)
if not trace:
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pose_cov_time.json"), "w") as f:
        f.write(text + "\n")
