"""Clouds, pairs and guesses shared by tests/test_gpu_gicp_lockstep.py and its child process tests/gicp_lockstep_child.py."""
import numpy as np

from toyslam_amd import clouds

# sources at the edges of the two plans (32 queries per k_correspond block, 256 points per functor block, 8 parts in the
# fixed-order sum: 2 048 points are 8 blocks, 2 049 a ninth), targets large, small and of k points
SOURCE_SIZES = (20, 32, 33, 256, 257, 2048, 2049, 2500)
TARGET_SIZES = (2500, 300, 20)
CHILD_SIZES = (2500, 1025, 900, 2049, 257, 33)   # five consecutive pairs: members of 10, 5, 4, 9, 2, 1 functor blocks


def noisy_subsets(sizes, seed=7):
    """Random subsets of a 3 000-point scene of 20 m, each under a small pose of its own (+-0.1 m, +-0.01 rad) plus 1 cm noise
    (the recipe of tests/test_gpu_gicp_pairs.py)."""
    base = clouds.target_surfaces(3000, extent=20.0, n_boxes=12)[:, :3]
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        sub = base[rng.choice(len(base), n, replace=False)]
        T = clouds.make_T(rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.01, 0.01, 3))
        out.append((clouds.apply_T(T, sub) + rng.normal(0, 0.01, (n, 3))).astype(np.float32))
    return out


def child_guesses():
    rng = np.random.default_rng(23)
    return [clouds.make_T(rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.005, 0.005, 3)).astype(np.float32) for _ in range(len(CHILD_SIZES) - 1)]


FIELDS = ("T", "converged", "iterations", "correspondences", "fitness")


def to_json(r):
    """A result dict with every float as a hex string."""
    return dict(T=[[float(x).hex() for x in T.reshape(-1)] for T in r["T"]], converged=[bool(x) for x in r["converged"]],
                iterations=[int(x) for x in r["iterations"]], correspondences=[int(x) for x in r["correspondences"]],
                fitness=[float(x).hex() for x in r["fitness"]])


def from_json(j):
    return dict(T=np.array([[float.fromhex(x) for x in T] for T in j["T"]], np.float32).reshape(-1, 4, 4),
                converged=np.array(j["converged"], bool), iterations=np.array(j["iterations"], np.int32),
                correspondences=np.array(j["correspondences"], np.int32), fitness=np.array([float.fromhex(x) for x in j["fitness"]]))


def same_results(a, b):
    return all(np.array_equal(np.asarray(a[f]), np.asarray(b[f])) for f in FIELDS)
