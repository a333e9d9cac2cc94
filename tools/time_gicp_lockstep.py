"""gicp_align_pairs_lockstep against gicp_align_pairs_clouds (the registrations one after the other, each with its own
objective server) on the clouds and settings of tools/time_gicp_pairs.py: consecutive pairs of a scan sequence, clouds of the
reference pair's size (about 16 k points after the 0.1 m prefilter), pclomp::GeneralizedIterativeClosestPoint's constructor
settings.  Both calls in the same process, alternating, median of the runs after a warm-up pass of each; compared on
register_ms of gicp_diag_pairs_time (the preparation is the same code in both).  And a multi-start shape: one pair from 8
and 64 guesses, alignGuesses against the align + getFitnessScore loop.  One child process per size, each under a time limit
of its own; the parent only gathers.  Writes profiles/gicp_lockstep_time.json and prints it.
    python tools/time_gicp_lockstep.py [runs (>= 5)] [raw points per scan]
    python tools/time_gicp_lockstep.py --profile-one      one 39-pair lock-step call (for rocprofv3 --kernel-trace --stats)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COUNTS = (8, 16, 39, 128)
GUESS_COUNTS = (8, 64)
LEAF = 0.1


def sequence(n_clouds, n_raw):
    """tools/time_gicp_pairs.py's clouds: a static world seen from a moving pose, prefiltered at 0.1 m, resident in HBM"""
    from toyslam_amd import clouds, ndt
    rng = np.random.default_rng(3)
    world = clouds.target_surfaces(12 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
    nd = ndt.NormalDistributionsTransform()
    nd.warmUp(65536)
    pose = np.eye(4)
    dcs = []
    for k in range(n_clouds):
        if k:
            pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
        pick = world[rng.choice(len(world), n_raw, replace=False)]
        raw = (clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32)
        dcs.append(nd.voxelGridFilterCloud(raw, LEAF)[0])
    return nd, dcs


def same(a, b):
    return bool(all(np.array_equal(a[f], b[f]) for f in ("T", "converged", "iterations", "correspondences", "fitness")))


def one(n_pairs, runs, n_raw):
    from toyslam_amd import gicp
    nd, dcs = sequence(n_pairs + 1, n_raw)
    gs, gl = gicp.GeneralizedIterativeClosestPoint(), gicp.GeneralizedIterativeClosestPoint()

    def call(g, fn):
        t0 = time.perf_counter()
        r = fn(dcs)
        return time.perf_counter() - t0, r, g.pairsTime()

    _, rs, _ = call(gs, gs.alignPairsClouds)
    _, rl, _ = call(gl, gl.alignPairsLockstep)   # warm-up of both, and the check that they give the same
    d = gl.diagLockstep()
    ts, tl, regs, regl, prep = [], [], [], [], []
    for _ in range(runs):   # alternating
        t, _, pt = call(gs, gs.alignPairsClouds)
        ts.append(t)
        regs.append(pt["register_ms"])
        t, _, pt = call(gl, gl.alignPairsLockstep)
        tl.append(t)
        regl.append(pt["register_ms"])
        prep.append(pt["prepare_ms"])
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    return dict(pairs=n_pairs, points_per_scan=round(float(np.mean([len(c) for c in dcs])), 1),
                sequential=dict(call_ms=med(1e3 * np.array(ts)), register_ms=med(regs)),
                lockstep=dict(call_ms=med(1e3 * np.array(tl)), register_ms=med(regl)), prepare_ms=med(prep),
                register_speedup=round(float(np.median(regs)) / float(np.median(regl)), 3), steps=d["steps"],
                correspond_launches=d["correspond_launches"], max_members_in_step=d["max_members_in_step"],
                mean_iterations=round(float(rs["iterations"].mean()), 2), same_results=same(rs, rl))


def one_guesses(n_guesses, runs, n_raw):
    from toyslam_amd import clouds, gicp
    nd, dcs = sequence(2, n_raw)
    rng = np.random.default_rng(9)
    guesses = [clouds.make_T(rng.uniform(-0.3, 0.3, 3) * [1, 1, 0.1], np.deg2rad(rng.uniform(-1.0, 1.0, 3) * [0.2, 0.2, 1])).astype(np.float32)
               for _ in range(n_guesses)]
    g = gicp.GeneralizedIterativeClosestPoint()
    g.setInputTargetCloud(dcs[0])
    g.setInputSourceCloud(dcs[1])

    def loop():
        T, fit = [], []
        t0 = time.perf_counter()
        for gu in guesses:
            g.align(gu)
            fit.append(g.getFitnessScore())
            T.append(g.getFinalTransformation())
        return time.perf_counter() - t0, np.stack(T), np.array(fit)

    def together():
        t0 = time.perf_counter()
        r = g.alignGuesses(guesses)
        return time.perf_counter() - t0, r

    _, T, fit = loop()
    _, r = together()
    ok = bool(np.array_equal(r["T"], T) and np.array_equal(r["fitness"], fit))
    tl, tg = [], []
    for _ in range(runs):
        tl.append(loop()[0])
        tg.append(together()[0])
    d = g.diagLockstep()
    ms = lambda v: round(1e3 * float(np.median(v)), 3)  # noqa: E731
    return dict(guesses=n_guesses, points=[len(dcs[0]), len(dcs[1])], align_loop_ms=ms(tl), align_guesses_ms=ms(tg),
                speedup=round(float(np.median(tl)) / float(np.median(tg)), 3), steps=d["steps"], max_members_in_step=d["max_members_in_step"],
                mean_iterations=round(float(r["iterations"].mean()), 2), same_results=ok)


def profile_one(n_raw):
    from toyslam_amd import gicp
    nd, dcs = sequence(40, n_raw)
    g = gicp.GeneralizedIterativeClosestPoint()
    r = g.alignPairsLockstep(dcs)
    print(json.dumps(dict(pairs=39, steps=g.diagLockstep()["steps"], not_converged=int((~r["converged"]).sum()))))


def child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:  # whatever went wrong on the device: nothing more is started on it
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit("time_gicp_lockstep: %s ended with status %d" % (args, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        print(json.dumps(one(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--one-guesses":
        print(json.dumps(one_guesses(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--profile-one":
        profile_one(int(sys.argv[2]) if len(sys.argv) > 2 else 17500)
        sys.exit(0)
    runs = max(5, int(sys.argv[1]) if len(sys.argv) > 1 else 5)
    n_raw = int(sys.argv[2]) if len(sys.argv) > 2 else 17500
    out = dict(metric="ms, median of %d alternating runs after a warm-up pass of each" % runs, leaf=LEAF, raw_points=n_raw, pairs={}, guesses={})
    for n in COUNTS:
        out["pairs"][str(n)] = child(["--one", n, runs, n_raw], 60 + 3 * n)
        sys.stderr.write("time_gicp_lockstep: %d pairs done\n" % n)
    for n in GUESS_COUNTS:
        out["guesses"][str(n)] = child(["--one-guesses", n, runs, n_raw], 60 + 3 * n)
        sys.stderr.write("time_gicp_lockstep: %d guesses done\n" % n)
    text = json.dumps(out)
    with open(os.path.join(ROOT, "profiles", "gicp_lockstep_time.json"), "w") as f:
        f.write(text + "\n")
    print(text)
