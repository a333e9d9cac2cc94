"""gicp_align_pairs_clouds against the only way there was before it, on consecutive pairs of a scan sequence: clouds of the
reference pair's size (about 16 k points after the 0.1 m prefilter of apps/align.cpp), a static world seen from a moving pose
as in tools/time_pairs.py, pclomp::GeneralizedIterativeClosestPoint's constructor settings.
  pairs call : every filtered scan resident in HBM, one gicp_align_pairs_clouds over the pairs (k-1, k) with fitness
  loop       : one handle and, per pair, gicp_set_input_target + gicp_set_input_source from host arrays + gicp_align +
               gicp_get_fitness_score -- every scan set twice, once in each role
Both in the same process, alternating, median of the runs after a warm-up pass of each; the pairs call also split into its
preparation (finite check, index builds, covariance launch) and its registrations (gicp_diag_pairs_time).  One child process
per pair count, each under a time limit of its own; the parent only gathers.  Writes profiles/gicp_pairs_time.json and
prints it.
    python tools/time_gicp_pairs.py [runs (>= 5)] [raw points per scan]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COUNTS = (8, 16, 39, 128)
LEAF = 0.1


def one(n_pairs, runs, n_raw):
    from toyslam_amd import clouds, gicp, ndt
    rng = np.random.default_rng(3)
    world = clouds.target_surfaces(12 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
    nd = ndt.NormalDistributionsTransform()
    nd.warmUp(65536)
    pose = np.eye(4)
    dcs, host = [], []
    for k in range(n_pairs + 1):
        if k:
            pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
        pick = world[rng.choice(len(world), n_raw, replace=False)]
        raw = (clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32)
        dcs.append(nd.voxelGridFilterCloud(raw, LEAF)[0])
        host.append(dcs[-1].numpy())
    gp, gl = gicp.GeneralizedIterativeClosestPoint(), gicp.GeneralizedIterativeClosestPoint()

    def pairs_call():
        t0 = time.perf_counter()
        r = gp.alignPairsClouds(dcs)
        return time.perf_counter() - t0, r

    def loop():
        T, fit = [], []
        t0 = time.perf_counter()
        for k in range(n_pairs):
            gl.setInputTarget(host[k])
            gl.setInputSource(host[k + 1])
            gl.align()
            fit.append(gl.getFitnessScore())
            T.append(gl.getFinalTransformation())
        return time.perf_counter() - t0, np.stack(T), np.array(fit)

    _, r = pairs_call()
    _, T, fit = loop()  # warm-up of both, and the check that they do the same work
    same = bool(np.array_equal(r["T"], T) and np.array_equal(r["fitness"], fit))
    tp, tl, prep, reg = [], [], [], []
    for _ in range(runs):  # alternating
        tl.append(loop()[0])
        tp.append(pairs_call()[0])
        t = gp.pairsTime()
        prep.append(t["prepare_ms"])
        reg.append(t["register_ms"])
    ms = lambda v: round(1e3 * float(np.median(v)), 3)  # noqa: E731
    d = gp.diagPairs()
    return dict(pairs=n_pairs, points_per_scan=round(float(np.mean([len(h) for h in host])), 1), pairs_call_ms=ms(tp), loop_ms=ms(tl),
                speedup=round(float(np.median(tl)) / float(np.median(tp)), 3), prepare_ms=round(float(np.median(prep)), 3),
                register_ms=round(float(np.median(reg)), 3), per_pair_ms=dict(pairs_call=round(ms(tp) / n_pairs, 4), loop=round(ms(tl) / n_pairs, 4)),
                index_builds=d["index_builds"], knn_launches=d["knn_launches"], mean_iterations=round(float(r["iterations"].mean()), 2),
                not_converged=int((~r["converged"]).sum()), same_results_as_loop=same)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        print(json.dumps(one(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))))
        sys.exit(0)
    runs = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
    n_raw = int(sys.argv[2]) if len(sys.argv) > 2 else 17500
    out = dict(metric="ms per call, median of %d alternating runs after a warm-up pass" % runs, leaf=LEAF, raw_points=n_raw, sizes={})
    for n in COUNTS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), str(runs), str(n_raw)], capture_output=True,
                           text=True, timeout=60 + 3 * n)
        if r.returncode != 0:  # whatever went wrong on the device: nothing more is started on it
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("time_gicp_pairs: the run of %d pairs ended with status %d" % (n, r.returncode))
        out["sizes"][str(n)] = json.loads(r.stdout.strip().splitlines()[-1])
        sys.stderr.write("time_gicp_pairs: %d pairs done\n" % n)
    text = json.dumps(out)
    with open(os.path.join(ROOT, "profiles", "gicp_pairs_time.json"), "w") as f:
        f.write(text + "\n")
    print(text)
