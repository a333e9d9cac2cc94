"""Poses and clouds shared by tests/test_score_poses_host.py (CPU: the oracle side) and tests/test_gpu_score_poses.py (GPU).

The candidate poses of a re-localisation are poses of the SOURCE in the target's frame, so the set is built around what
registers the bundled pair (the oracle's golden result) and around what does not (a quarter turn, a kilometre away)."""
import numpy as np

METHODS = ("DIRECT7", "DIRECT1", "DIRECT26", "KDTREE")
N_POSES = 33
I_IDENTITY, I_GOLDEN, I_YAW90, I_FAR = 0, 1, 31, 32


def make_T(t, rpy):
    from toyslam_amd import clouds
    return clouds.make_T(t, rpy).astype(np.float32)


def golden_T(golden):
    return np.asarray(golden["aligns"]["DIRECT7/default"]["T"], dtype=np.float32)


def poses(golden):
    """The 33 poses: the identity, the golden registration result, 29 small perturbations of it (up to 0.5 m / 2 degrees,
    the batch workload's range), a 90 degree yaw and a pose 1 km away."""
    from toyslam_amd import clouds
    Tg = golden_T(golden)
    rng = np.random.default_rng(3301)
    out = [np.eye(4, dtype=np.float32), Tg]
    for _ in range(N_POSES - 4):
        out.append((clouds.random_T(rng, 0.5, 2.0) @ Tg.astype(np.float64)).astype(np.float32))
    out.append(make_T([0, 0, 0], [0, 0, np.pi / 2]))
    out.append(make_T([1000.0, 0, 0], [0, 0, 0]))
    assert len(out) == N_POSES
    return out


def near_indices():
    return list(range(0, I_YAW90))   # the identity, the golden result and its perturbations: the scans overlap


def far_poses(n, seed=3302):
    """n poses that put the scan 1 - 3 km from the target, with small rotations: every point outside the grid."""
    from toyslam_amd import clouds
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        T = clouds.random_T(rng, 0.5, 2.0)
        T[:3, 3] += [1000.0 + 50.0 * k, -1200.0, 0.0]
        out.append(T.astype(np.float32))
    return out


def guesses(golden, n):
    """n starting guesses of a registration of the bundled pair: the identity, then perturbations of it (up to 0.3 m /
    1 degree: inside the basin the reference's own nodes start from)."""
    from toyslam_amd import clouds
    rng = np.random.default_rng(3303)
    out = [np.eye(4, dtype=np.float32)]
    while len(out) < n:
        out.append(clouds.random_T(rng, 0.3, 1.0).astype(np.float32))
    return out


def xyz1(cloud):
    c = np.asarray(cloud, dtype=np.float32)
    return np.ascontiguousarray(np.c_[c[:, :3], np.ones(len(c), np.float32)], dtype=np.float32)


def moved(po, cloud, T):
    """pcl::transformPointCloud(cloud, T) as the oracle restates it: (N, 4) float32."""
    return po.transform_cloud(xyz1(cloud), T)


def spoiled(cloud, far=True):
    """A copy with NaN / +inf / -inf points (one of them the last point) and, with `far`, one absurdly far finite point."""
    c = np.array(cloud, dtype=np.float32, copy=True)
    n = len(c)
    c[n // 3] = np.nan
    c[n // 2, 1] = np.inf
    c[n - 1, 2] = -np.inf
    if far:
        c[n // 5] = 1e30
    return c


def argsort_top(scores, keep):
    """numpy's statement of ndt_host_pick_top: the finite scores, largest first, ties to the lower index."""
    s = np.asarray(scores, dtype=np.float64)
    idx = np.flatnonzero(np.isfinite(s))
    order = idx[np.argsort(-s[idx], kind="stable")]
    return order[:keep].astype(np.int32)
