"""Fixtures for the tests at leaf sizes that are no power of two (tests/test_leaf_cases.py pins them on the CPU against the
oracle, tests/test_gpu_leaf_sizes.py runs them on the GPU).  numpy only, no GPU, no library call.

At such a leaf floor(x / leaf) -- the cell a point is SEARCHED from -- and floor(x * (1 / leaf)) -- the cell a target point is
BINNED into -- are different f32 numbers for some x next to a cell face ("trap 2" of SURVEY.md), and random points do not
find those x: the fixtures put points on the faces, f32(k * leaf) and its two f32 neighbours.

  face_scene        a target block with every point mid-cell, a source with every point on (or one ulp off) a face
  face_target       target points on faces themselves: which cell the BUILD puts them into
  sphere_queries    one voxel and queries within 12 ulps of the KDTREE radius around its centroid
  misbinned_voxels  voxels whose centroid lies outside the cell it is binned into (fitness_cases.misbinned_case, six-fold)
  product_rule_terms   nvtl_cases.Grid.terms with the search cell taken by the product rule -- the WRONG kernel, there to show
                    that the fixtures tell the two rules apart

The references: neighbours, NVTL and score are tests/nvtl_cases.Grid (search: the quotient); distances are
tests/fitness_cases.nearest_d2; the centroid cloud is tests/centroid_fitness_cases.centroid_cloud (build: the product)."""
import numpy as np

import centroid_fitness_cases as cc
import fitness_cases as fc
import nvtl_cases as nc

F = np.float32
LEAVES = (0.3, 0.7, 1.5, 3.0)
ORIGINS = (40, -5)
MIN_PTS = 6
BLOCK = (8, 8, 3)         # cells of face_scene's target: from `origin` in x and y, from 0 in z
FACE_K = range(-2, 11)    # faces from two cells below the block's origin to two cells above its far side in x and y
SPHERE_ULPS = 12


def quotient_cells(points, leaf):
    """the cell a point is searched from: floor(x / leaf), the quotient rounded to f32 before the floor"""
    with np.errstate(all="ignore"):
        return np.floor(np.asarray(points)[:, :3].astype(F) / F(leaf)).astype(np.int64)


def product_cells(points, leaf):
    """the cell a target point is binned into: floor(x * (1 / leaf)), reciprocal and product rounded to f32"""
    return cc.cells_of(points, leaf)


def with_neighbours(v):
    """every value of v, followed by the next f32 above and the next f32 below it -> (3 * len(v),) f32, value-major"""
    v = np.asarray(v, dtype=F)
    return np.stack([v, np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf))], axis=1).reshape(-1)


def face_values(leaf, ks):
    """f32(k * f32(leaf)) and its two f32 neighbours for every k"""
    return with_neighbours(np.asarray(list(ks), dtype=F) * F(leaf))


def face_scene(leaf, origin, seed=61):
    """-> (target (N, 3) f32, source (468, 3) f32).

    target: the block of BLOCK cells without the cells whose (i + j + k) % 5 == 0 (i, j, k counted inside the block); eight
    points within +-0.2 leaf of the centre of every other cell, so that both rules bin every target point alike.
    source: for every face value (13 faces x 3), along each of the three axes, four points whose other two coordinates are
    mid-cell: along x (and y) the face values are those of cells origin - 2 .. origin + 10, the other in-plane coordinate
    (origin + 1.5 | origin + 3.5) leaf and z (0.5 | 1.5) leaf; along z they are those of cells -2 .. 10 at x, y from
    (origin + 1.5 | origin + 3.5) leaf."""
    rng = np.random.default_rng([seed, int(round(leaf * 1000)), origin + 1000])
    cells = [(i, j, k) for i in range(BLOCK[0]) for j in range(BLOCK[1]) for k in range(BLOCK[2]) if (i + j + k) % 5 != 0]
    centre = np.asarray(cells, dtype=np.float64) + [origin + 0.5, origin + 0.5, 0.5]
    jitter = rng.uniform(-0.2, 0.2, (len(cells), 8, 3))
    target = ((centre[:, None, :] + jitter) * leaf).reshape(-1, 3).astype(F)
    in_plane = [F((origin + 1.5) * leaf), F((origin + 3.5) * leaf)]
    height = [F(0.5 * leaf), F(1.5 * leaf)]
    src = []
    for axis in range(3):
        for v in face_values(leaf, [(0 if axis == 2 else origin) + k for k in FACE_K]):
            for a in in_plane:
                for b in (in_plane if axis == 2 else height):
                    src.append({0: (v, a, b), 1: (a, v, b), 2: (a, b, v)}[axis])
    return target, np.asarray(src, dtype=F)


def face_target(leaf, seed=62):
    """-> (1440, 3) f32: six points at each of the 240 x values f32(k * f32(leaf)), + 1 ulp, - 1 ulp, k = -20 .. 59; y and z
    within +-0.1 leaf of the middle of cell 0.  Arrival order: x value after x value."""
    rng = np.random.default_rng([seed, int(round(leaf * 1000))])
    x = np.repeat(face_values(leaf, range(-20, 60)), 6)
    yz = ((0.5 + rng.uniform(-0.1, 0.1, (len(x), 2))) * leaf).astype(F)
    return np.stack([x, yz[:, 0], yz[:, 1]], axis=1).astype(F)


def sphere_queries(leaf, seed=63):
    """-> (target (9, 3) f32: one voxel, its f32 centroid (3,), queries (150, 3) f32: the centroid moved along +-x, +-y, +-z by
    r, for r = f32(leaf) and its SPHERE_ULPS f32 neighbours on either side).  The KDTREE radius is f32(leaf); whether a query
    sees the voxel is decided in the last bits of f32(leaf)^2."""
    rng = np.random.default_rng([seed, int(round(leaf * 1000))])
    target = ((np.array([3.0, -2.0, 1.0]) + rng.uniform(0.3, 0.7, (9, 3))) * leaf).astype(F)
    xyz, _ = cc.centroid_cloud(target, leaf, MIN_PTS)
    assert xyz.shape == (1, 3)
    c = xyz[0]
    radii = [cc.ulp_steps(F(leaf), k) for k in range(-SPHERE_ULPS, SPHERE_ULPS + 1)]
    q = []
    for axis in range(3):
        for sign in (1, -1):
            for r in radii:
                p = c.copy()
                p[axis] = c[axis] + F(sign) * r
                q.append(p)
    return target, c, np.asarray(q, dtype=F)


def misbinned_voxels(leaf):
    """fitness_cases.misbinned_case with every target point six times: voxels whose CENTROID (the point itself) lies outside
    the cell it is binned into, and queries only the give of the centroid search's cell pruning saves.
    -> (target (576, 3), queries (48, 3), gap2 (48,), the expected centroid cloud (96, 3): R0, P0, R1, P1, ..)"""
    t, q, gap2 = fc.misbinned_case(leaf)
    target = np.repeat(t, MIN_PTS, axis=0)
    cloud, _ = cc.centroid_cloud(target, leaf, MIN_PTS)
    return target, q, gap2, cloud


def kd_radius2(leaf):
    """the KDTREE radius squared as the oracle (ndt_oracle.cpp:433) and the library (kd_radius2) form it: the f32 resolution
    squared in f64, rounded to f32"""
    return F(float(F(leaf)) ** 2)


def terms_from_cells(grid, points, cell, ok):
    """nvtl_cases.Grid.terms with the search cell of every point given, not computed: -> q (N, K) f64, has (N, K) bool.
    (With quotient_cells this is Grid.terms itself, which tests/test_leaf_cases.py asserts bit for bit.)"""
    p = np.ascontiguousarray(np.asarray(points)[:, :3], dtype=F)
    N, offs = len(p), nc.offsets(grid.method)
    q = np.zeros((N, len(offs)))
    has = np.zeros((N, len(offs)), dtype=bool)
    if len(grid.idx) == 0 or N == 0:
        return q, has
    pd = p.astype(np.float64)
    for k, off in enumerate(offs):
        rel = cell + np.asarray(off) - grid.min_b
        inside = ok & ((rel >= 0) & (rel < grid.div_b)).all(axis=1)
        lin = rel[:, 0] + rel[:, 1] * grid.div_b[0] + rel[:, 2] * grid.div_b[0] * grid.div_b[1]
        row = np.minimum(np.searchsorted(grid.idx, np.where(inside, lin, 0)), len(grid.idx) - 1)
        hit = inside & (grid.idx[row] == lin)
        if grid.method == "KDTREE":
            ci = grid.c_of_row[row]
            hit &= ci >= 0
            cen = grid.c_xyz[np.maximum(ci, 0)]
            with np.errstate(all="ignore"):
                e = np.where(hit[:, None], p - cen, F(0)).astype(F)
                d = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            hit &= d < grid.r2
        else:
            hit &= grid.n[row] >= grid.min_pts
        x = np.where(hit[:, None], pd - grid.mean[row], 0.0)
        C = grid.icov[row]
        cx = (C[:, :, 0] * x[:, [0]] + C[:, :, 1] * x[:, [1]]) + C[:, :, 2] * x[:, [2]]
        q[:, k] = (x[:, 0] * cx[:, 0] + x[:, 1] * cx[:, 1]) + x[:, 2] * cx[:, 2]
        has[:, k] = hit
    return q, has


def quotient_rule_terms(grid, points):
    p = np.asarray(points)[:, :3].astype(F)
    return terms_from_cells(grid, p, quotient_cells(p, grid.leaf), np.isfinite(p).all(axis=1))


def product_rule_terms(grid, points):
    """Grid.terms of a kernel that searched from the cell the BUILD would put the point into.  Wrong; used only to count the
    points at which a fixture tells the two rules apart."""
    p = np.asarray(points)[:, :3].astype(F)
    return terms_from_cells(grid, p, product_cells(p, grid.leaf), np.isfinite(p).all(axis=1))


def rules_differ(grid, points):
    """-> (value differs (N,) bool, neighbour count differs (N,) bool) between Grid.terms and product_rule_terms: the per-point
    NVTL value (-1.0 where nothing is found) and the number of neighbours"""
    q, has = grid.terms(points)
    qp, hasp = product_rule_terms(grid, points)
    L = nc.nvtl(q, has, grid.d1, grid.d2)[0]
    Lp = nc.nvtl(qp, hasp, grid.d1, grid.d2)[0]
    return L != Lp, has.sum(axis=1) != hasp.sum(axis=1)
