"""Reference and generators for the tests of the centroid cloud and the centroid fitness (tests/test_gpu_centroid_fitness.py;
the helpers' own tests: tests/test_centroid_fitness_cases.py).  numpy only, no GPU.

  centroid_cloud       the expected cloud from the points in arrival order, in the reference's f32 arithmetic
  centroids_from_blob  the same cloud from the rows of ndt_target_accumulate_export
  shell_limit          the cost rule of the search as implemented (ndt_centroid_fitness.hip centroid_shell_limit)
  *_target / *_queries the generators

Expected distances are tests/fitness_cases.nearest_d2 over the expected cloud: a fitness value of a scan of ONE query is that
query's squared nearest distance as f32, widened to f64 -- exact."""
import numpy as np

import fitness_cases as fc

F = np.float32
DBL_MAX = fc.DBL_MAX
K_TEAM_SHELLS = 2    # k_centroid_fitness_multi: shells 0..2 by the query's team of 8 lanes, shells 3.. by the whole wave
K_KNN_MIN_RING = 3   # shells every query may try before the one scan of the table
LUT_BORDER = 2       # the padded dense table: the box plus two empty cells on every side

ACC_ROW_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("k", "<i4"), ("count", "<i4"), ("d", "<f8", (9,)), ("f", "<f4", (3,)), ("pad", "<f4")])
ACC_BLOB_HEADER_BYTES = 64


# ------------------------------------------------------------------------------------------------ the reference
def cells_of(points, resolution):
    """the reference's cell of every point: floor(x * inv_leaf), the product rounded to f32 before the floor"""
    inv = F(1.0) / F(resolution)
    return np.floor(np.asarray(points)[:, :3].astype(F) * inv).astype(np.int64)


def centroid_cloud(points_in_arrival_order, resolution, min_pts):
    """-> ((V, 3) float32, (V,) int64): the centroid of every voxel with at least min_pts points -- the f32 coordinate sums in
    arrival order divided by float32(count) -- and its linear index over the box of the finite points, ascending.  Rows with
    a non-finite coordinate land in no voxel."""
    p = np.ascontiguousarray(np.asarray(points_in_arrival_order)[:, :3], dtype=F)
    p = p[np.isfinite(p).all(axis=1)]
    if len(p) == 0:
        return np.zeros((0, 3), F), np.zeros(0, np.int64)
    ijk = cells_of(p, resolution)
    lo = ijk.min(axis=0)
    div = ijk.max(axis=0) - lo + 1
    lin = (ijk[:, 0] - lo[0]) + (ijk[:, 1] - lo[1]) * div[0] + (ijk[:, 2] - lo[2]) * div[0] * div[1]
    order = np.argsort(lin, kind="stable")  # arrival order kept inside a voxel
    lin_s, p_s = lin[order], p[order]
    starts = np.nonzero(np.r_[True, lin_s[1:] != lin_s[:-1]])[0]
    ends = np.r_[starts[1:], len(lin_s)]
    xyz, idx = [], []
    for a, b in zip(starts, ends):
        if b - a < min_pts:
            continue
        s = np.cumsum(p_s[a:b], axis=0, dtype=F)[-1]  # sequential f32 sums (equal to the scalar loop)
        xyz.append(s / F(b - a))
        idx.append(lin_s[a])
    if not xyz:
        return np.zeros((0, 3), F), np.zeros(0, np.int64)
    return np.stack(xyz).astype(F), np.asarray(idx, dtype=np.int64)


def centroids_from_blob(export_bytes, min_pts):
    """-> ((V, 3) float32, (V, 3) int64 cells): the same cloud from an exported target's rows: f[3] / float32(count) of every
    row with at least min_pts points, in ascending (k, j, i) -- the order of the linear index over any box."""
    rows = np.frombuffer(bytes(export_bytes), dtype=ACC_ROW_DTYPE, offset=ACC_BLOB_HEADER_BYTES)
    rows = rows[rows["count"] >= min_pts]
    order = np.lexsort((rows["i"], rows["j"], rows["k"]))
    rows = rows[order]
    xyz = (rows["f"].astype(F) / rows["count"].astype(F)[:, None]).astype(F)
    return xyz.reshape(-1, 3), np.stack([rows["i"], rows["j"], rows["k"]], axis=1).astype(np.int64).reshape(-1, 3)


def rows_blob(rows):
    """a header-less stand-in for an export: 64 zero bytes and the given (i, j, k, count, f) rows"""
    a = np.zeros(len(rows), dtype=ACC_ROW_DTYPE)
    for n, (i, j, k, count, f) in enumerate(rows):
        a[n]["i"], a[n]["j"], a[n]["k"], a[n]["count"] = i, j, k, count
        a[n]["f"] = np.asarray(f, dtype=F)
    return bytes(ACC_BLOB_HEADER_BYTES) + a.tobytes()


def shell_limit(div_b, entries=None):
    """Shells the search walks before the one pass over the table (the cost rule): while (2r+1)^3 <= entries / 4, at least
    K_KNN_MIN_RING, at most the grid's largest extent.  entries: the padded dense table of the box by default."""
    div_b = [int(d) for d in div_b]
    if entries is None:
        entries = int(np.prod([d + 2 * LUT_BORDER for d in div_b]))
    r_lim = max(div_b)
    r = 0
    while r < r_lim and (2 * r + 3) ** 3 <= entries // 4:
        r += 1
    return min(r_lim, max(K_KNN_MIN_RING, r))


# ------------------------------------------------------------------------------------------------ targets
def voxel_points(cells, rng, res=1.0, pts=8, lo=0.15, hi=0.85):
    """`pts` points inside each of the given cells (well inside: the centroid stays in its cell), cell after cell"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3)
    out = (cells[:, None, :] + lo + (hi - lo) * rng.random((len(cells), pts, 3))) * res
    return out.reshape(-1, 3).astype(F)


def mixed_target(seed=3, res=1.0, min_pts=6):
    """Ordinary voxels, a voxel of six collinear points, a voxel of six identical points, a voxel of min_pts - 1 points and a
    voxel that reaches min_pts only with the second update -> [update 0, update 1].  (The covariance sums start from the
    identity, voxel_grid_covariance_omp.h:107, so six collinear or identical points are NOT rejected: rejected_target is the
    fixture with a voxel of nr_points == -1.)"""
    rng = np.random.default_rng(seed)
    cells = [(i, j, k) for i in range(0, 7, 2) for j in range(0, 5, 2) for k in (0, 1)]
    a = voxel_points(cells, rng, res, 9)
    t = np.linspace(0.2, 0.8, 6)
    collinear = np.stack([1.0 + t, 0.5 + 0 * t, 0.5 + 0 * t], axis=1) * res
    identical = np.tile([[3.5, 1.5, 0.5]], (6, 1)) * res
    under = voxel_points([(5, 1, 1)], rng, res, min_pts - 1)
    late0 = voxel_points([(1, 3, 1)], rng, res, min_pts - 2)
    late1 = voxel_points([(1, 3, 1)], rng, res, 3)
    more = voxel_points(cells[::3] + [(9, 6, 2)], rng, res, 7)
    u0 = np.concatenate([a, collinear, identical, under, late0]).astype(F)
    u1 = np.concatenate([late1, more]).astype(F)
    return [u0, u1]


def rejected_target(seed=7):
    """The recipe of the accumulate tests for a REJECTED voxel: 500 km out a voxel of 3000 collinear points cancels into a
    negative eigenvalue (nr_points == -1 in the dump; still in the centroid cloud, trap 7).  Around it ordinary voxels of 30
    points and one of 4 (under min_pts).  -> (points, cell of the collinear voxel)"""
    rng = np.random.default_rng(seed)
    ox, oy = 500000, -500000
    in_cell = lambda cell, n: (np.asarray(cell, F) + 0.1 + 0.8 * rng.random((n, 3))).astype(F)
    parts = [in_cell((ox - 2 + i, oy - 2 + j, 0), 30) for i in range(4) for j in range(4) if (i, j) not in ((1, 1), (2, 2))]
    at = np.array([ox + 0.5, oy + 0.5, 0.5], F)
    line = (at + np.c_[np.linspace(-0.3, 0.3, 3000), np.zeros(3000), np.zeros(3000)]).astype(F)
    parts += [in_cell((ox - 1, oy - 1, 0), 4), line]
    return np.concatenate(parts).astype(F), (ox, oy, 0)


def under_target(seed=4, res=1.0, min_pts=6):
    """every voxel under min_pts: an empty centroid cloud"""
    rng = np.random.default_rng(seed)
    return [voxel_points([(i, j, 0) for i in range(4) for j in range(3)], rng, res, min_pts - 1)]


def shape_targets(seed=5):
    """name -> cells: 1, 2, 3 voxels, a line with a gap, a plane, a block with a far outlier (a long, mostly empty box)"""
    return {
        "one": [(0, 0, 0)],
        "two": [(0, 0, 0), (3, 1, 0)],
        "three": [(0, 0, 0), (1, 0, 0), (0, 4, 2)],
        "line": [(i, 0, 0) for i in range(5)] + [(i, 0, 0) for i in range(17, 24)],
        "plane": [(i, j, 0) for i in range(12) for j in range(12)],
        "block": [(i, j, k) for i in range(3) for j in range(3) for k in range(3)] + [(20, 1, 1)],
    }


def tie_target():
    """two voxels of eight identical points each: exact centroids (1.5, 0.5, 0.5) and (3.5, 0.5, 0.5); a query at x = 2.5 ties"""
    a = np.tile([[1.5, 0.5, 0.5]], (8, 1))
    b = np.tile([[3.5, 0.5, 0.5]], (8, 1))
    return np.concatenate([a, b]).astype(F), np.array([[2.5, 0.5, 0.5], [2.5, 0.25, 0.75], [2.5, -3.0, 9.0]], dtype=F)


def ulp_steps(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def edge_queries(cloud_xyz, points, res, rng, n_random=160):
    """Queries around a target whose expected centroid cloud is cloud_xyz (built from `points`):
    in occupied cells; on cell faces and one ulp either side; in empty cells 1..8 shells off the box in every direction class
    (axis, edge, corner), which crosses the team-to-wave hand-off (2 | 3) and the shell bound of every small table; uniformly
    over the box grown by 6 cells; outside the box from one ulp to 1e20 m; NaN / inf rows."""
    res = float(res)
    ijk = cells_of(points, res)
    lo, hi = ijk.min(axis=0), ijk.max(axis=0)
    box_lo, box_hi = lo * res, (hi + 1) * res
    q = []
    q.append(cloud_xyz + F(0.05 * res))                                             # in occupied cells
    q.append(cloud_xyz - F(0.3 * res) * rng.random(cloud_xyz.shape).astype(F))
    faces = []
    for c in cloud_xyz[:: max(1, len(cloud_xyz) // 12)]:                            # cell faces, one ulp either side
        base = np.floor(c / F(res)) * F(res)
        for ax in range(3):
            for face in (base[ax], base[ax] + F(res)):
                for k in (-1, 0, 1):
                    p = c.copy()
                    p[ax] = ulp_steps(face, k)
                    faces.append(p)
    q.append(np.asarray(faces, dtype=F))
    far = []
    for k in range(1, 9):                                                           # k shells off the box
        for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 1, 1), (-1, 0, 0), (-1, -1, -1), (1, -1, 0)):
            d = np.asarray(d, dtype=np.float64)
            corner = np.where(d > 0, box_hi, np.where(d < 0, box_lo, (box_lo + box_hi) / 2))
            far.append(corner + d * (k - 0.5) * res)
    q.append(np.asarray(far, dtype=F))
    span = (box_hi - box_lo) + 12 * res
    q.append((box_lo - 6 * res + span * rng.random((n_random, 3))).astype(F))        # anywhere around
    out = []
    for ax in range(3):                                                             # outside: 1 ulp .. 1e20 m
        for side, edge in ((1, box_hi[ax]), (-1, box_lo[ax])):
            for step in (None, 1.0, 1e3, 1e6, 1e12, 1e20):
                p = ((box_lo + box_hi) / 2).astype(F)
                p[ax] = ulp_steps(edge, side) if step is None else F(edge + side * step)
                out.append(p)
    out.append(np.array([1e20, -1e20, 1e20]))
    q.append(np.asarray(out, dtype=F))
    q.append(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]], dtype=F))
    return np.concatenate(q).astype(F)


def transforms():
    """non-identity transforms: a translation, a rotation about z with a translation, a general rotation"""
    c, s = np.cos(0.3), np.sin(0.3)
    Rz = np.array([[c, -s, 0, 1.5], [s, c, 0, -0.75], [0, 0, 1, 0.25], [0, 0, 0, 1]])
    a, b = np.cos(-1.1), np.sin(-1.1)
    Rx = np.array([[1, 0, 0, 0], [0, a, -b, 0], [0, b, a, 0], [0, 0, 0, 1]])
    return [fc.translation([0.5, -2.0, 0.125]), Rz.astype(F), (Rz @ Rx).astype(F)]


# ------------------------------------------------------------------------------------------------ the excursion
EXC_BASE = 100000.0


def excursion_target(base=EXC_BASE, seed=7, n=6000, res=1.0):
    """A voxel of n points drawn in [base, base + 1) on x (y, z in the cell 0): far from the origin its sequential f32 sum
    drifts, and the centroid leaves the voxel by cells.  Around it ordinary voxels of 8 points, beside the owning cell and
    beside where the centroid lands.  -> (points, cell of the big voxel)"""
    rng = np.random.default_rng(seed)
    top = np.nextafter(F(base + 1.0), F(0))
    x = np.minimum((base + rng.random(n)).astype(F), top)
    big = np.stack([x, (0.25 + 0.5 * rng.random(n)).astype(F), (0.25 + 0.5 * rng.random(n)).astype(F)], axis=1).astype(F)
    b = int(base)
    cells = [(b - 2, 0, 0), (b + 1, 1, 0), (b + 2, 0, 1), (b + 4, 1, 0), (b + 5, 0, 0), (b + 7, 1, 1), (b + 3, 3, 0)]
    small = voxel_points(cells, rng, res, 8, 0.4, 0.6)
    return np.concatenate([big, small]).astype(F), (b, 0, 0)


def excursion_of(cloud_xyz, cloud_cells, res=1.0):
    """the largest per-axis distance by which a centroid lies outside the box of its own cell, in the search's f32 arithmetic
    (box: float32(cell) * leaf, + leaf); 0 when all are inside"""
    lo = cloud_cells.astype(F) * F(res)
    hi = lo + F(res)
    gap = np.maximum(np.maximum(lo - cloud_xyz, cloud_xyz - hi), F(0))
    return float(gap.max()) if gap.size else 0.0


def cloud_cells(points, resolution, min_pts):
    """the absolute cells of centroid_cloud's voxels, in its order"""
    p = np.asarray(points)[:, :3].astype(F)
    p = p[np.isfinite(p).all(axis=1)]
    ijk = cells_of(p, resolution)
    lo = ijk.min(axis=0)
    div = ijk.max(axis=0) - lo + 1
    _, idx = centroid_cloud(p, resolution, min_pts)
    k = idx // (div[0] * div[1])
    j = (idx - k * div[0] * div[1]) // div[0]
    i = idx - k * div[0] * div[1] - j * div[0]
    return np.stack([i + lo[0], j + lo[1], k + lo[2]], axis=1)


def excursion_queries(points, big_cell, res=1.0, min_pts=6, seed=8):
    """beside the drifted centroid, beside the owning cell, halfway between, and a lattice over the neighbourhood"""
    xyz, _ = centroid_cloud(points, res, min_pts)
    cells = cloud_cells(points, res, min_pts)
    me = np.nonzero((cells == np.asarray(big_cell)).all(axis=1))[0][0]
    c = xyz[me].astype(np.float64)
    own = (np.asarray(big_cell, dtype=np.float64) + 0.5) * res
    rng = np.random.default_rng(seed)
    q = [c + 0.2 * (rng.random((24, 3)) - 0.5), own + 0.9 * (rng.random((24, 3)) - 0.5), (c + own) / 2 + 0.5 * (rng.random((24, 3)) - 0.5)]
    gx, gy, gz = np.meshgrid(np.arange(big_cell[0] - 4.3, big_cell[0] + 10, 0.61), np.arange(-2.2, 5.5, 0.87), [-1.4, 0.5, 1.6], indexing="ij")
    q.append(np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1))
    return np.concatenate(q).astype(F)
