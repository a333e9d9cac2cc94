"""numpy reference of the pose covariance (Laplace / sandwich), written from the definition in include/ndt_mi355.h.  Used by
tests/test_pose_cov_cases.py (CPU: pins this file against the oracle's gradient and f64 Hessian and against hand cases),
tests/test_pose_cov_host.py (the host algebra) and tests/test_gpu_pose_cov.py (GPU).  No GPU, no library call.

  angle_tables      the f64 angle-derivative tables at a pose (j_ang_d 8x3, h_ang_d 15x3), with the reference's snap
  Grid              nvtl_cases.Grid plus records(): per point and neighbour slot, the voxel row and whether it is a neighbour
  Grid.information  source, moved source, pose -> A, B, g, n_found and, per entry of B and g, the sum S of the absolute values
                    of the terms that were added into it (what a bound on a re-ordered f64 sum is stated in)
  covariance        steps 7 and 8 of the definition with numpy.linalg.eigh

The moved cloud is an INPUT (pcl::transformPointCloud of the source in f32: score_poses_cases.moved); so is the pose p =
matrix_to_pose(transform)."""
import numpy as np

import nvtl_cases as nc

F = np.float32
METHODS = nc.METHODS
INDEFINITE = 1


def angle_tables(p):
    """(j_ang_d (8, 3), h_ang_d (15, 3)) at p = x y z roll pitch yaw; |angle| < 10e-5 snaps to cos 1, sin 0"""
    c, s = [], []
    for a in np.asarray(p, dtype=np.float64)[3:6]:
        snap = abs(a) < 10e-5
        c.append(1.0 if snap else np.cos(a))
        s.append(0.0 if snap else np.sin(a))
    (cx, cy, cz), (sx, sy, sz) = c, s
    J = [[-sx * sz + cx * sy * cz, -sx * cz - cx * sy * sz, -cx * cy],
         [cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy],
         [-sy * cz, sy * sz, cy],
         [sx * cy * cz, -sx * cy * sz, sx * sy],
         [-cx * cy * cz, cx * cy * sz, -cx * sy],
         [-cy * sz, -cy * cz, 0],
         [cx * cz - sx * sy * sz, -cx * sz - sx * sy * cz, 0],
         [sx * cz + cx * sy * sz, cx * sy * cz - sx * sz, 0]]
    H = [[-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, sx * cy],
         [-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, -cx * cy],
         [cx * cy * cz, -cx * cy * sz, cx * sy],
         [sx * cy * cz, -sx * cy * sz, sx * sy],
         [-sx * cz - cx * sy * sz, sx * sz - cx * sy * cz, 0],
         [cx * cz - sx * sy * sz, -sx * sy * cz - cx * sz, 0],
         [-cy * cz, cy * sz, -sy],
         [-sx * sy * cz, sx * sy * sz, sx * cy],
         [cx * sy * cz, -cx * sy * sz, -cx * cy],
         [sy * sz, sy * cz, 0],
         [-sx * cy * sz, -sx * cy * cz, 0],
         [cx * cy * sz, cx * cy * cz, 0],
         [-cy * cz, cy * sz, 0],
         [-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, 0],
         [-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, 0]]
    return np.array(J, dtype=np.float64), np.array(H, dtype=np.float64)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def point_jacobians(src, j_ang):
    """(N, 3, 6): identity | the angle columns, from the UNMOVED points"""
    x = np.ascontiguousarray(np.asarray(src)[:, :3], dtype=F).astype(np.float64)
    with np.errstate(all="ignore"):                                               # (a non-finite point: NaN entries, never used)
        t = np.stack([dot3(x, j_ang[r][None, :]) for r in range(8)], axis=1)      # (N, 8)
    J = np.zeros((len(x), 3, 6))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1.0
    J[:, 1, 3], J[:, 2, 3] = t[:, 0], t[:, 1]
    J[:, 0, 4], J[:, 1, 4], J[:, 2, 4] = t[:, 2], t[:, 3], t[:, 4]
    J[:, 0, 5], J[:, 1, 5], J[:, 2, 5] = t[:, 5], t[:, 6], t[:, 7]
    return J


def point_hessian_vectors(src, h_ang):
    """(N, 3, 3, 3): [i - 3][j - 3][r] = the second derivative of the moved point by angles i and j, component r"""
    x = np.ascontiguousarray(np.asarray(src)[:, :3], dtype=F).astype(np.float64)
    with np.errstate(all="ignore"):
        xh = np.stack([dot3(x, h_ang[r][None, :]) for r in range(15)], axis=1)    # (N, 15)
    z = np.zeros(len(x))
    a, b, c = (np.stack([z, xh[:, k], xh[:, k + 1]], axis=1) for k in (0, 2, 4))
    d, e, f = (xh[:, k:k + 3] for k in (6, 9, 12))
    rows = [[a, b, c], [b, d, e], [c, e, f]]
    return np.stack([np.stack(r, axis=1) for r in rows], axis=1)


class Grid(nc.Grid):
    def records(self, points):
        """points (N, >= 3) f32, used as given -> row (N, K) voxel row, hit (N, K) bool: nvtl_cases.Grid.terms' probe (the
        neighbour set of calculateScore and of computeHessian alike), in the kernels' slot order"""
        p = np.ascontiguousarray(np.asarray(points)[:, :3], dtype=F)
        N, offs = len(p), nc.offsets(self.method)
        rows = np.zeros((N, len(offs)), dtype=np.int64)
        hits = np.zeros((N, len(offs)), dtype=bool)
        if len(self.idx) == 0 or N == 0:
            return rows, hits
        with np.errstate(all="ignore"):
            c = np.floor(p / self.leaf)
        ok = np.isfinite(p).all(axis=1) & (np.abs(c) < 2.0 ** 30).all(axis=1)
        cell = np.where(ok[:, None], c, 0).astype(np.int64)
        for k, off in enumerate(offs):
            rel = cell + np.asarray(off) - self.min_b
            inside = ok & ((rel >= 0) & (rel < self.div_b)).all(axis=1)
            lin = rel[:, 0] + rel[:, 1] * self.div_b[0] + rel[:, 2] * self.div_b[0] * self.div_b[1]
            row = np.minimum(np.searchsorted(self.idx, np.where(inside, lin, 0)), len(self.idx) - 1)
            hit = inside & (self.idx[row] == lin)
            if self.method == "KDTREE":
                ci = self.c_of_row[row]
                hit &= ci >= 0
                cen = self.c_xyz[np.maximum(ci, 0)]
                with np.errstate(all="ignore"):
                    e = np.where(hit[:, None], p - cen, F(0)).astype(F)
                    d = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                hit &= d < self.r2
            else:
                hit &= self.n[row] >= self.min_pts
            rows[:, k], hits[:, k] = row, hit
        return rows, hits

    def information(self, src, moved, p, hessian=True):
        """src (N, >= 3): the source as given; moved (N, >= 3): the same points moved by the transform in f32; p: the pose.
        -> dict A (6, 6; None without `hessian`), H (the unsymmetrised f64 Hessian), B (6, 6, uncentred), g (6,), n_found,
        S_B (6, 6), S_g (6,), g_i (N, 6), found (N,)"""
        j_ang, h_ang = angle_tables(p)
        J = point_jacobians(src, j_ang)
        N = len(J)
        rows, hits = self.records(moved)
        pd = np.ascontiguousarray(np.asarray(moved)[:, :3], dtype=F).astype(np.float64)
        g_i, S_i = np.zeros((N, 6)), np.zeros((N, 6))
        found = np.zeros(N, dtype=bool)
        H = np.zeros((6, 6))
        HV = point_hessian_vectors(src, h_ang) if hessian else None
        for k in range(rows.shape[1]):
            hit = hits[:, k]
            with np.errstate(all="ignore"):
                xt = np.where(hit[:, None], pd - self.mean[rows[:, k]], 0.0)
                Cm = self.icov[rows[:, k]]
                Cx = (Cm[:, :, 0] * xt[:, [0]] + Cm[:, :, 1] * xt[:, [1]]) + Cm[:, :, 2] * xt[:, [2]]
                w = self.d2 * np.exp(-self.d2 * dot3(xt, Cx) / 2)
                use = hit & ~((w > 1) | (w < 0) | np.isnan(w))
                w = np.where(use, w * self.d1, 0.0)
                Cx = np.where(use[:, None], Cx, 0.0)
            with np.errstate(all="ignore"):                        # (0 x NaN of a non-finite point: masked by `found` below)
                t = (Cx[:, 0, None] * J[:, 0, :] + Cx[:, 1, None] * J[:, 1, :]) + Cx[:, 2, None] * J[:, 2, :]      # (N, 6)
                g_i += w[:, None] * t
                S_i += np.abs(w)[:, None] * ((np.abs(Cx[:, 0, None] * J[:, 0, :]) + np.abs(Cx[:, 1, None] * J[:, 1, :]))
                                            + np.abs(Cx[:, 2, None] * J[:, 2, :]))
            found |= use
            if hessian:
                Cu = np.where(use[:, None, None], Cm, 0.0)
                CJ = np.einsum("nab,nbk->nak", Cu, J)
                term = -self.d2 * t[:, :, None] * t[:, None, :] + np.einsum("nai,naj->nij", CJ, J)
                term[:, 3:, 3:] += np.einsum("nr,nijr->nij", Cx, HV)
                H += np.einsum("n,nij->ij", w, np.where(use[:, None, None], term, 0.0))   # (a NaN point: 0 x NaN otherwise)
        g_i = np.where(found[:, None], g_i, 0.0)
        B = np.einsum("na,nb->ab", g_i, g_i)
        out = dict(H=H if hessian else None, A=-(H + H.T) / 2 if hessian else None, B=B, g=g_i.sum(axis=0),
                   n_found=int(found.sum()), S_B=np.einsum("na,nb->ab", np.abs(g_i), np.abs(g_i)),
                   S_g=np.where(found[:, None], S_i, 0.0).sum(axis=0), g_i=g_i, found=found)
        return out


def centred(B, g, n_found):
    B, g = np.asarray(B, dtype=np.float64).reshape(6, 6), np.asarray(g, dtype=np.float64)
    return B - np.outer(g, g) / n_found if n_found else B


def covariance(A, B, g, n_found, method, scale=1.0):
    """steps 7 and 8 with numpy.linalg.eigh -> (cov (6, 6), eig_min, eig_max, flags)"""
    A = np.asarray(A, dtype=np.float64).reshape(6, 6)
    if not np.isfinite(A).all():
        return np.full((6, 6), np.nan), np.nan, np.nan, INDEFINITE
    lam, V = np.linalg.eigh(A)
    lo, hi = float(lam.min()), float(lam.max())
    if n_found < 6 or not lo > 1e-12 * hi:
        return np.full((6, 6), np.nan), lo, hi, INDEFINITE
    Ai = (V / lam) @ V.T
    M = scale * Ai if method == "laplace" else Ai @ centred(B, g, n_found) @ Ai
    return (M + M.T) / 2, lo, hi, 0


def planar_fixture(seed=7):
    """(target, source): 400 target points of ONE voxel ([0, 1)^3 at resolution 1) scattered over the plane z = 0.5 with
    a millimetre of noise, and 300 source points of the same patch.  In the plane the voxel's Gaussian is a cell wide, across
    it the inflated smallest eigenvalue (1 % of the largest) wide: the plane pins z, roll and pitch, hardly x and y."""
    rng = np.random.default_rng(seed)
    t = np.c_[rng.uniform(0.05, 0.95, (400, 2)), 0.5 + 1e-3 * rng.standard_normal(400)].astype(F)
    s = np.c_[rng.uniform(0.15, 0.85, (300, 2)), 0.5 + 2e-3 * rng.standard_normal(300)].astype(F)
    return t, s
