"""Child process of tests/test_gpu_gicp_grid.py, and the runs the parent shares with it: the development switches that are read
once per process (NDT_GICP_MAX_BLOCKS, NDT_GICP_SERVER, NDT_GICP_NO_FUSE) need a process of their own.  It only COMPUTES -- the
correspondence steps of every source size against the voxel target, and the registrations of the bundled pair's first 2 000 source
points against the grid of its target, as hex floats in a JSON file -- and the parent does the comparing.

    python tests/gicp_grid_child.py out.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import centroid_fitness_cases as cc  # noqa: E402
import gicp_grid_cases as gc  # noqa: E402

F = np.float32
N_SOURCE = 2000
FIT_RANGE = 1.0


def make_map(ndt, updates, form, res=1.0, min_pts=6, poses=None):
    """an NDT handle whose target is built from the updates: form = (kind "cloud" | "acc", voxel index 0 auto / 1 dense / 2 sparse)"""
    kind, index = form
    m = ndt.NormalDistributionsTransform()
    m.setResolution(res)
    m.setMinPointPerVoxel(min_pts)
    m.setVoxelIndex(index)
    if kind == "acc":
        for k, u in enumerate(updates):
            m.targetAccumulate(u, None if poses is None else poses[k])
    else:
        m.setInputTarget(np.concatenate(updates), is_dense=True)
    return m


def new_route(gicp, m, mode, src, src_cov=None, gate=None):
    g = gicp.GeneralizedIterativeClosestPoint()
    g.setInputTargetGrid(m, mode)
    g.setInputSource(src)
    if src_cov is not None:
        g.setSourceCovariances(src_cov)
    if gate is not None:
        g.setMaxCorrespondenceDistance(gate)
    return g


def ref_route(gicp, voxels, src, src_cov=None, gate=None):
    """the existing, oracle-pinned path: a fresh handle whose target CLOUD is D's centroids with D's covariances"""
    xyz1, cov, _ = voxels
    g = gicp.GeneralizedIterativeClosestPoint()
    g.setInputTarget(xyz1[:, :3])
    g.setTargetCovariances(cov)
    g.setInputSource(src)
    if src_cov is not None:
        g.setSourceCovariances(src_cov)
    if gate is not None:
        g.setMaxCorrespondenceDistance(gate)
    return g


def registration(g, guess):
    """align + everything the issue compares afterwards"""
    g.align(guess)
    st = g.stats()
    return dict(T=g.getFinalTransformation(), converged=g.hasConverged(), iterations=g.getFinalNumIteration(),
                stats=[st["n_f"], st["n_df"], st["n_fdf"], st["correspondences"]], fitness=g.getFitnessScore(FIT_RANGE))


def same_registration(a, b):
    return (np.array_equal(a["T"], b["T"]) and a["converged"] == b["converged"] and a["iterations"] == b["iterations"] and
            list(a["stats"]) == list(b["stats"]) and a["fitness"] == b["fitness"])


def guesses():
    a = np.deg2rad(3.0)
    G = np.eye(4, dtype=F)
    G[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=F)
    G[:3, 3] = np.asarray([0.2, -0.2, 0.1], F)     # |t| = 0.3 m
    return [None, G]


def pieces_and_poses(target):
    """the target in three posed pieces: piece k is stored moved by the inverse of pose k, and accumulated under pose k"""
    out, poses = [], []
    for k in range(3):
        a = 0.1 * (k + 1)
        P = np.eye(4)
        P[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        P[:3, 3] = [1.0 * k, -0.5 * k, 0.25 * k]
        Pi = np.linalg.inv(P)
        piece = target[k::3].astype(np.float64)
        out.append((piece @ Pi[:3, :3].T + Pi[:3, 3]).astype(F))
        poses.append(P.astype(F))
    return out, poses


def step_run(ndt, gicp):
    """the correspondence step of every source size against the mixed target's accumulated map, identity pose and a rotation"""
    u = cc.mixed_target()
    m = make_map(ndt, u, ("acc", 1))
    D, _, _ = gc.d_of(np.concatenate(u))
    pool = gc.query_pool(D, np.concatenate(u), 1.0, 31)
    rng = np.random.default_rng(32)
    out = {}
    for n in gc.SIZES:
        src = pool[rng.permutation(len(pool))[:n]]
        g = new_route(gicp, m, "plane", src, gc.spd(n, 100 + n))
        for name, T in (("I", None), ("R", gc.rotation())):
            cnt, corr, maha = g.step_correspond(None, T)
            f, grad = g.step_functor(2, np.array([0.01, -0.02, 0.03, 0.001, 0.002, -0.001])) if cnt else (0.0, np.zeros(6))
            out["%d%s" % (n, name)] = dict(src=src, corr=corr, maha=maha, f=f, g=grad, blocks=g.diagTargetGrid()["correspond_blocks"],
                                           plan=g.plan(n)["correspond_blocks"])
    return out


def registration_run(ndt, gicp, target, source):
    m = make_map(ndt, [target.astype(F)], ("cloud", 0))
    src = np.ascontiguousarray(source[:N_SOURCE], dtype=F)
    out = {}
    for mode in ("plane", "raw"):
        for k, guess in enumerate(guesses()):
            out["%s%d" % (mode, k)] = registration(new_route(gicp, m, mode, src), guess)
    return out


def hexed(x):
    if isinstance(x, dict):
        return {k: hexed(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [hexed(v) for v in x]
    if isinstance(x, np.ndarray):
        return dict(shape=list(x.shape), dtype=str(x.dtype), hex=x.tobytes().hex())
    if isinstance(x, (float, np.floating)):
        return dict(f64=float(x).hex())
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    return x


def unhexed(x):
    if isinstance(x, dict):
        if "hex" in x and "dtype" in x:
            return np.frombuffer(bytes.fromhex(x["hex"]), dtype=x["dtype"]).reshape(x["shape"])
        if set(x) == {"f64"}:
            return float.fromhex(x["f64"])
        return {k: unhexed(v) for k, v in x.items()}
    if isinstance(x, list):
        return [unhexed(v) for v in x]
    return x


def main(out_path):
    from toyslam_amd import gicp, ndt
    d = np.load(os.path.join(ROOT, "tests", "golden", "pair_0p1.npz"))
    res = dict(steps=step_run(ndt, gicp), registrations=registration_run(ndt, gicp, d["target"], d["source"]))
    with open(out_path, "w") as f:
        json.dump(hexed(res), f)


if __name__ == "__main__":
    main(sys.argv[1])
