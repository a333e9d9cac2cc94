"""Reference and generators for the tests of GICP against a voxel target (tests/test_gpu_gicp_grid.py; the helpers' own tests:
tests/test_gicp_grid_cases.py).  numpy only, no GPU.

  target_set        D from a grid dump: the voxels the DIRECT searches see (n >= min_pts; a rejected voxel has n == -1)
  cov_raw           RAW covariances: the inverse of icov (cofactors times 1 / det, as the library's inv3_cofactor)
  cov_plane         PLANE covariances: I - (1 - eps) n n^T, n the eigenvector of icov's largest eigenvalue
  plane_defects     the three properties a PLANE covariance is checked by (normals are not unique in degenerate voxels)
  correspond        brute-force correspondences over D: f32 d2 as fitness_cases.nearest_d2, lower index on ties, the strict gate
  queries of all kinds, the source sizes, random SPD covariances, the non-identity rotation
"""
import numpy as np

import centroid_fitness_cases as cc
import fitness_cases as fc

F = np.float32
GICP_EPSILON = 0.001
PLANE, RAW = 0, 1
# a block of k_correspond_voxel takes 32 queries a pass: one block up to 32, two up to 64, three beyond
SIZES = (1, 7, 8, 9, 31, 32, 33, 64, 65, 255, 256, 257)
MAX_BLOCKS_CHILD = 3


def correspond_blocks(n, cap=0):
    """gicp::correspond_blocks: 32 query teams per block, at most 32768 blocks, NDT_GICP_MAX_BLOCKS caps it"""
    limit = min(32768, cap) if cap > 0 else 32768
    return max(1, min(limit, -(-n // 32)))


# ------------------------------------------------------------------------------------------------ the reference
def target_set(dump_n, min_pts):
    """mask over the rows of a grid dump (ascending linear index): the voxels of D"""
    return np.asarray(dump_n) >= min_pts


def cov_raw(icov):
    """(V, 3, 3): Matrix3d::inverse() as Eigen evaluates it for 3x3 -- cofactors, times 1 / det"""
    a = np.asarray(icov, dtype=np.float64).reshape(-1, 3, 3)
    out = np.empty_like(a)
    cof = lambda i, j: a[:, (i + 1) % 3, (j + 1) % 3] * a[:, (i + 2) % 3, (j + 2) % 3] - a[:, (i + 1) % 3, (j + 2) % 3] * a[:, (i + 2) % 3, (j + 1) % 3]
    c00, c10, c20 = cof(0, 0), cof(1, 0), cof(2, 0)
    invdet = 1.0 / ((c00 * a[:, 0, 0] + c10 * a[:, 1, 0]) + c20 * a[:, 2, 0])
    for i in range(3):
        for j in range(3):
            out[:, i, j] = cof(j, i) * invdet
    return out


def cov_plane(icov, eps=GICP_EPSILON):
    a = np.asarray(icov, dtype=np.float64).reshape(-1, 3, 3)
    a = (a + a.transpose(0, 2, 1)) / 2
    _, v = np.linalg.eigh(a)
    n = v[:, :, 2]
    return np.eye(3)[None] - (1.0 - eps) * n[:, :, None] * n[:, None, :]


def plane_defects(C, icov, eps=GICP_EPSILON):
    """-> (asymmetry, eigenvalue error against {eps, 1, 1}, ||icov n - lmax n|| / lmax with n recovered from (I - C) / (1 - eps)),
    the largest of each over the voxels"""
    C = np.asarray(C, dtype=np.float64).reshape(-1, 3, 3)
    a = np.asarray(icov, dtype=np.float64).reshape(-1, 3, 3)
    asym = np.abs(C - C.transpose(0, 2, 1)).max() if len(C) else 0.0
    w = np.linalg.eigvalsh((C + C.transpose(0, 2, 1)) / 2)
    eig = np.abs(w - np.array([eps, 1.0, 1.0])).max() if len(C) else 0.0
    P = (np.eye(3)[None] - C) / (1.0 - eps)        # n n^T
    res = 0.0
    for p, m in zip(P, a):
        k = int(np.argmax(np.diag(p)))
        n = p[:, k] / np.sqrt(p[k, k])
        lmax = np.linalg.eigvalsh((m + m.T) / 2)[2]
        res = max(res, float(np.linalg.norm(m @ n - lmax * n) / lmax))
    return float(asym), float(eig), res


def correspond(d_xyz, queries, gate):
    """-> (corr, d2): corr[i] = the index in D of the point nearest to query i (f32 d2, the lower index on ties) if d2 < gate^2
    (in f64, strict), else -1"""
    d2, arg = fc.nearest_d2(d_xyz, queries)
    ok = (arg >= 0) & (d2.astype(np.float64) < float(gate) * float(gate))
    return np.where(ok, arg, -1).astype(np.int32), d2


# ------------------------------------------------------------------------------------------------ generators
def finite(q):
    q = np.asarray(q, dtype=F)
    return q[np.isfinite(q).all(axis=1)]


def spd(n, seed):
    """n random symmetric positive definite 3x3 f64 matrices, condition number below 100"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, 3, 3))
    q, _ = np.linalg.qr(a)
    w = 0.05 + rng.random((n, 3)) * 2.0
    return np.einsum("nij,nj,nkj->nik", q, w, q)


def rotation():
    """a general rotation with a small translation, f32 (gicp_step_correspond's `transformation`)"""
    T = cc.transforms()[2].astype(F).copy()
    T[:3, 3] = np.asarray([0.25, -0.125, 0.5], F)
    return T


def matvec_eigen(T, xyz):
    """the query of source point (x, y, z) under T as the kernels compute it: ((T0 x + T1 y) + T2 z) + T3 * 1, f32"""
    T = np.asarray(T, dtype=F)
    x, y, z = (np.asarray(xyz)[:, i].astype(F) for i in range(3))
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] * F(1) for i in range(3)], axis=1).astype(F)


def d2_f32(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    d = a - b
    return F((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def gate_steps(v):
    """Gates around a query whose f32 squared nearest distance is v.  The library compares float64(d2) < gate * gate, strictly.
    -> (g_at, g_up, g_lo32, g_hi32): g_at the largest f64 with g * g <= v (for a v that is a perfect square: g * g == v, the gate AT
    d2) -- no correspondence; g_up the next f64 up, g * g > v -- a correspondence; and gates whose squares lie one f32 ulp of v
    below and above (strictly inside that ulp's far side), the "+-1 ulp" pair."""
    v = float(F(v))
    g = float(np.sqrt(v))
    while g * g > v:
        g = float(np.nextafter(g, 0.0))
    while float(np.nextafter(g, np.inf)) ** 2 <= v:
        g = float(np.nextafter(g, np.inf))
    lo32, hi32 = float(np.nextafter(F(v), F(0))), float(np.nextafter(F(v), F(np.inf)))
    g_lo = float(np.sqrt(lo32))
    while g_lo * g_lo > lo32:
        g_lo = float(np.nextafter(g_lo, 0.0))
    g_hi = float(np.sqrt(hi32))
    while g_hi * g_hi < hi32:
        g_hi = float(np.nextafter(g_hi, np.inf))
    return g, float(np.nextafter(g, np.inf)), g_lo, g_hi


def face_queries(d_xyz, res):
    """on the faces of the voxels' cells and one ulp either side"""
    out = []
    for c in np.asarray(d_xyz, F)[:: max(1, len(d_xyz) // 8)]:
        base = np.floor(c / F(res)) * F(res)
        for ax in range(3):
            for face in (base[ax], base[ax] + F(res)):
                for k in (-1, 0, 1):
                    p = c.copy()
                    p[ax] = cc.ulp_steps(face, k)
                    out.append(p)
    return np.asarray(out, dtype=F)


def far_queries(d_xyz):
    """100 km off the target in every axis direction"""
    c = np.asarray(d_xyz, F).mean(axis=0)
    return np.asarray([c + F(100000.0) * np.asarray(d, F) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))], dtype=F)


def query_pool(d_xyz, points, res, seed, n_random=120):
    """every kind of query around a target whose D is d_xyz: cc.edge_queries (finite rows), cell faces +-1 ulp, 100 km offsets"""
    rng = np.random.default_rng(seed)
    return finite(np.concatenate([cc.edge_queries(d_xyz, points, res, rng, n_random), face_queries(d_xyz, res), far_queries(d_xyz)]))


GATES = (1e-6, 1e-3, 0.5, 2.0, 5.0, 40.0, 1e3, 1e6)


# ------------------------------------------------------------------------------------------------ fixtures shared with the GPU file
def d_of(points, res=1.0, min_pts=6, rejected_cells=()):
    """-> (xyz (n, 3) f32, linear idx (n,), absolute cells (n, 3)): D expected from the points in arrival order -- the centroid
    cloud (cc.centroid_cloud) less the voxels in the given (rejected) cells"""
    xyz, idx = cc.centroid_cloud(points, res, min_pts)
    if len(xyz) == 0:
        return xyz, idx, np.zeros((0, 3), np.int64)
    cells = cc.cloud_cells(points, res, min_pts)
    keep = np.ones(len(xyz), bool)
    for c in rejected_cells:
        keep &= ~(cells == np.asarray(c)).all(axis=1)
    return xyz[keep], idx[keep], cells[keep]


REJECTED_GATE = 40.0


def rejected_case():
    """cc.rejected_target with queries beside the rejected voxel's centroid: in the centroid cloud C that voxel is their nearest,
    in D it is passed over.  -> (points, rejected cell, queries)"""
    pts, cell = cc.rejected_target()
    xyz, _ = cc.centroid_cloud(pts, 1.0, 6)
    cells = cc.cloud_cells(pts, 1.0, 6)
    c = xyz[(cells == np.asarray(cell)).all(axis=1)][0]
    off = np.asarray([[0.01, 0, 0], [0, -0.02, 0.01], [0.2, 0.2, 0.1], [-0.3, 0.1, 0.0]], F)
    return pts, cell, (c[None, :] + off).astype(F)


def under_case():
    """cc.mixed_target's two updates and queries in the two cells that matter: (5, 1, 1) never reaches min_pts, (1, 3, 1) only with
    the second update.  -> (updates, queries)"""
    u = cc.mixed_target()
    q = np.asarray([[5.5, 1.5, 1.5], [5.4, 1.6, 1.45], [1.5, 3.5, 1.5], [1.45, 3.55, 1.6]], F)
    return u, q


def excursion_case():
    """cc.excursion_target: the big voxel's centroid lies outside its own cell.  -> (points, its cell, queries)"""
    pts, cell = cc.excursion_target()
    return pts, cell, finite(cc.excursion_queries(pts, cell))
