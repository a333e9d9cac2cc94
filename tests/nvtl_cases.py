"""numpy reference of the nearest-voxel transformation likelihood (NVTL), written from the definition in include/ndt_mi355.h.
Used by tests/test_nvtl_cases.py (CPU: pins this file against the oracle's calculateScore and against hand cases) and
tests/test_gpu_nvtl.py (GPU).  No GPU, no library call.

  Grid            the oracle's voxels (OracleNDT.grid(): idx, n, mean, icov, min_b, div_b) behind one search method
  Grid.terms      per point and neighbour slot: q = x^T C^-1 x (f64) and whether the slot holds a neighbour
  nvtl            q -> (L per point, -1.0 where not found; NVTL; n_found): exp of the smallest q, mean over the found points
  score           the same terms reduced as calculateScore reduces them -- the check that the terms are the reference's

The cell of a point is floor(f32(p) / f32(leaf)).  DIRECT1 / DIRECT7 / DIRECT26 neighbours are the cells of the method's
offsets that lie inside the box and whose voxel has n >= min_points_per_voxel (DIRECT26: the 26 cells AROUND the point's
cell, not the cell itself -- the reference's getAllNeighborCellIndices).  KDTREE neighbours are the voxels of the centroid
cloud in the 3x3x3 block whose f32 centroid (tests/centroid_fitness_cases.centroid_cloud) lies closer than the radius, the
distance (dx*dx + dy*dy) + dz*dz in f32, strictly below f32(resolution^2)."""
import numpy as np

import centroid_fitness_cases as cc

F = np.float32
METHODS = ("DIRECT7", "DIRECT1", "DIRECT26", "KDTREE")
OFF7 = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
OFF27 = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]


def offsets(method):
    return {"DIRECT1": OFF7[:1], "DIRECT7": OFF7, "DIRECT26": [o for o in OFF27 if o != (0, 0, 0)], "KDTREE": OFF27}[method]


class Grid:
    """grid: dict with idx (ascending linear indices over the box), n, mean, icov, min_b, div_b.  centroids: (xyz f32, linear
    idx) of the centroid cloud, needed for KDTREE only."""

    def __init__(self, grid, gauss, method, resolution=1.0, min_pts=6, centroids=None):
        self.idx = np.asarray(grid["idx"], dtype=np.int64)
        assert np.all(np.diff(self.idx) > 0)
        self.n = np.asarray(grid["n"])
        self.mean = np.asarray(grid["mean"], dtype=np.float64).reshape(-1, 3)
        self.icov = np.asarray(grid["icov"], dtype=np.float64).reshape(-1, 3, 3)
        self.min_b = np.asarray(grid["min_b"], dtype=np.int64)
        self.div_b = np.asarray(grid["div_b"], dtype=np.int64)
        self.d1, self.d2, self.d3 = (float(x) for x in gauss)
        self.method, self.leaf, self.min_pts = method, F(resolution), int(min_pts)
        # the f32 resolution squared in f64, then rounded to f32: kd_radius2 (ndt_eval.hip) and ndt_oracle.cpp:433
        self.r2 = F(float(F(resolution)) ** 2)
        if method == "KDTREE":
            xyz, lin = centroids
            self.c_row = np.searchsorted(self.idx, lin)          # centroid -> voxel row
            assert np.array_equal(self.idx[self.c_row], lin)
            self.c_of_row = np.full(len(self.idx), -1, dtype=np.int64)
            self.c_of_row[self.c_row] = np.arange(len(lin))
            self.c_xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)

    @classmethod
    def of_oracle(cls, oracle, method, target_points, resolution=1.0, min_pts=6):
        cen = cc.centroid_cloud(target_points, resolution, min_pts) if method == "KDTREE" else None
        return cls(oracle.grid(), oracle.gauss(), method, resolution, min_pts, cen)

    def terms(self, points):
        """points: (N, >= 3), used as given (f32).  -> q (N, K) float64, has (N, K) bool; K = the method's neighbour slots in
        the kernels' order.  q is meaningless where has is False."""
        p = np.ascontiguousarray(np.asarray(points)[:, :3], dtype=F)
        N, offs = len(p), offsets(self.method)
        q = np.zeros((N, len(offs)))
        has = np.zeros((N, len(offs)), dtype=bool)
        if len(self.idx) == 0 or N == 0:
            return q, has
        with np.errstate(all="ignore"):
            c = np.floor(p / self.leaf)
        ok = np.isfinite(p).all(axis=1) & (np.abs(c) < 2.0 ** 30).all(axis=1)
        cell = np.where(ok[:, None], c, 0).astype(np.int64)
        pd = p.astype(np.float64)
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
                assert d.dtype == F
                hit &= d < self.r2
            else:
                hit &= self.n[row] >= self.min_pts
            x = np.where(hit[:, None], pd - self.mean[row], 0.0)
            C = self.icov[row]
            cx = (C[:, :, 0] * x[:, [0]] + C[:, :, 1] * x[:, [1]]) + C[:, :, 2] * x[:, [2]]
            q[:, k] = (x[:, 0] * cx[:, 0] + x[:, 1] * cx[:, 1]) + x[:, 2] * cx[:, 2]
            has[:, k] = hit
        return q, has

    def q_lists(self, points):
        q, has = self.terms(points)
        return [list(q[i, has[i]]) for i in range(len(q))]

    def nvtl(self, points):
        return nvtl(*self.terms(points), self.d1, self.d2)

    def score(self, points):
        return score(*self.terms(points), self.d1, self.d2, self.d3)


def q_min(q, has):
    """the smallest q per point, in slot order: starts at +inf, replaced whenever q < q_min -- a NaN never wins"""
    m = np.full(len(q), np.inf)
    for k in range(q.shape[1]):
        with np.errstate(invalid="ignore"):
            better = has[:, k] & (q[:, k] < m)
        m = np.where(better, q[:, k], m)
    return m


def nvtl(q, has, d1, d2):
    """-> (L (N,) with -1.0 where the point has no neighbour, NVTL, n_found)"""
    found = has.any(axis=1)
    L = np.where(found, -d1 * np.exp(-d2 * q_min(q, has) / 2), -1.0)
    n_found = int(found.sum())
    return L, (float(L[found].sum()) / n_found if n_found else 0.0), n_found


def nvtl_max_form(q, has, d1, d2):
    """the usual wording, for d2 > 0: the largest -d1 exp(-d2 q / 2) over the neighbours"""
    with np.errstate(invalid="ignore"):
        terms = np.where(has & ~np.isnan(q), -d1 * np.exp(-d2 * q / 2), -np.inf)
    found = has.any(axis=1)
    best = terms.max(axis=1) if q.shape[1] else np.full(len(q), -np.inf)
    return np.where(found, np.where(np.isinf(best), -d1 * 0.0, best), -1.0)


def score(q, has, d1, d2, d3):
    """calculateScore from the same terms: sum over points and neighbours of (-d1 e - d3) / cnt, over all points"""
    if len(q) == 0:
        return float("nan")
    cnt = has.sum(axis=1)
    with np.errstate(invalid="ignore"):
        inc = np.where(has, (-d1 * np.exp(-d2 * q / 2) - d3) / np.maximum(cnt, 1)[:, None], 0.0)
    return float(inc.sum()) / len(q)
