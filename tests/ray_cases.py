"""The ray of ndt_target_accumulate_clear_rays restated (include/ndt_mi355.h, "Clearing by rays"): one ray in pure Python
(walk_one), many rays at once in numpy (walk_many: the same operations in the same order on f64 arrays), the counts of a whole
call (call_counts), the fixtures, and a clearance measure per ray.

Clearance (metres): the smallest difference between the two lowest t_k at any step, and between the chosen t_a and t_end at any
step (the stopping one included), times len.  A ray whose clearance is tiny could take another branch under another
rounding of one division; fixtures for exact comparison keep only rays with clearance >= CLEAR (1e-6 m; rounding differences
are about 1e-11 m even 100 km from the origin) and may drop at most 1 % of their rays this way."""
import math

import numpy as np

LATTICE = 1 << 20
CLEAR = 1e-6
INF = float("inf")


def f32(x):
    return np.asarray(x, np.float32)


def start_cell(o, L):
    """m with m L <= o < (m + 1) L (exact products), or None outside the lattice"""
    q = math.floor(o / L)
    if not (-LATTICE - 1 <= q <= LATTICE):
        return None
    c = int(q)
    while c * L > o:
        c -= 1
    while (c + 1) * L <= o:
        c += 1
    return c if -LATTICE <= c < LATTICE else None


def walk_one(origin, point, leaf, margin=0.0, min_range=0.0, max_range=INF):
    """-> (cells, clearance, len) of a cast ray (cells: list of (i, j, k)), or None when the ray is not cast"""
    o = [float(v) for v in f32(origin)]
    p = [float(v) for v in f32(point)]
    L, margin = float(np.float32(leaf)), float(np.float32(margin))
    d = [p[k] - o[k] for k in range(3)]
    ln = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    if not (ln > 0.0 and float(np.float32(min_range)) <= ln <= float(np.float32(max_range))):
        return None
    t_end = 1.0 - margin / ln
    if not t_end > 0.0:
        return None
    m = [start_cell(o[k], L) for k in range(3)]
    if any(c is None for c in m):
        return [], INF, ln
    s = [1 if d[k] > 0 else -1 if d[k] < 0 else 0 for k in range(3)]
    f = [m[k] + (1 if s[k] > 0 else 0) for k in range(3)]
    t = [(f[k] * L - o[k]) / d[k] if s[k] else INF for k in range(3)]
    cells, clearance = [tuple(m)], INF
    while True:
        a = 0
        if t[1] < t[a]:
            a = 1
        if t[2] < t[a]:
            a = 2
        two = sorted(t)
        if two[1] != INF:
            clearance = min(clearance, (two[1] - two[0]) * ln)
        clearance = min(clearance, abs(t[a] - t_end) * ln)
        if not t[a] <= t_end:
            break
        m[a] += s[a]
        f[a] += s[a]
        if not -LATTICE <= m[a] < LATTICE:
            break
        t[a] = (f[a] * L - o[a]) / d[a]
        cells.append(tuple(m))
    return cells, clearance, ln


def walk_many(origins, points, leaf, margin=0.0, min_range=0.0, max_range=INF):
    """walk_one over N rays at once.  origins: (N, 3) or (3,).  -> dict(cast (N,) bool, n (N,) cells visited, clearance (N,),
    len (N,), ray (M,) and cells (M, 3): every visited cell with the index of its ray, grouped by step)"""
    p = f32(points).reshape(-1, 3).astype(np.float64)
    o = np.broadcast_to(f32(origins).reshape(-1, 3), p.shape).astype(np.float64)
    N = len(p)
    L, margin = float(np.float32(leaf)), float(np.float32(margin))
    d = p - o
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        t_end = 1.0 - margin / ln
        cast = (ln > 0.0) & (ln >= float(np.float32(min_range))) & (ln <= float(np.float32(max_range))) & (t_end > 0.0)
        q = np.floor(o / L)
    inside = ((q >= -LATTICE - 1) & (q <= LATTICE)).all(axis=1)
    m = np.where(inside[:, None], q, 0.0).astype(np.int64)
    for _ in range(4):
        m -= (m * L > o)
        m += ((m + 1) * L <= o)
    assert ((m * L <= o) & (o < (m + 1) * L))[inside].all()
    inside &= ((m >= -LATTICE) & (m < LATTICE)).all(axis=1)
    s = np.sign(d).astype(np.int64)
    f = m + (s > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(s != 0, (f * L - o) / d, INF)
    n = np.zeros(N, np.int64)
    clearance = np.full(N, INF)
    idx = np.nonzero(cast & inside)[0]
    n[idx] = 1
    rays, cells = [idx], [m[idx].copy()]
    while len(idx):
        tt = t[idx]
        a = np.argmin(tt, axis=1)                                 # the first of equal minima: the lowest axis wins a tie
        ta = tt[np.arange(len(idx)), a]
        two = np.sort(tt, axis=1)
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isinf(two[:, 1]), INF, two[:, 1] - two[:, 0])
        clearance[idx] = np.minimum(clearance[idx], np.minimum(gap, np.abs(ta - t_end[idx])) * ln[idx])
        go = ta <= t_end[idx]
        idx, a = idx[go], a[go]
        m[idx, a] += s[idx, a]
        f[idx, a] += s[idx, a]
        ok = (m[idx, a] >= -LATTICE) & (m[idx, a] < LATTICE)
        idx, a = idx[ok], a[ok]
        t[idx, a] = (f[idx, a] * L - o[idx, a]) / d[idx, a]
        n[idx] += 1
        rays.append(idx)
        cells.append(m[idx].copy())
    return dict(cast=cast, n=n, clearance=clearance, len=ln, ray=np.concatenate(rays), cells=np.concatenate(cells))


def pack(cells):
    """the key of the accumulated target's table: k high, i low (ndt_host_acc_pack_cell)"""
    c = np.asarray(cells, np.int64).reshape(-1, 3) + LATTICE
    return (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]


def build_cells(posed, res):
    """floor(p * inv_leaf) in f32, the arithmetic that bins a point -> (cells (N, 3) int64, inside the lattice (N,))"""
    fl = np.floor(f32(posed)[:, :3] * (np.float32(1.0) / np.float32(res)))
    ok = ((fl >= -LATTICE) & (fl < LATTICE)).all(axis=1)
    return np.where(ok[:, None], fl, 0).astype(np.int64), ok


def call_counts(voxel_cells, clouds, res, margin, min_range=0.0, max_range=1e30, min_clearance=None):
    """One call: clouds = [(posed points (N, 3) f32, non-finite rows allowed; origin (3,))], voxel_cells = the target's cells.
    -> dict(cells: the voxels in ascending key, miss, hit per voxel; cast, skipped, visited totals; clearance: the smallest of
    the call's cast rays; mean_len).  min_clearance: assert that no cast ray is closer to a tie than that."""
    vox = np.unique(np.asarray(voxel_cells, np.int64).reshape(-1, 3), axis=0)
    keys = pack(vox)
    order = np.argsort(keys)
    vox, keys = vox[order], keys[order]
    miss = np.zeros(len(vox), np.int64)
    hit = np.zeros(len(vox), bool)
    cast = skipped = visited = 0
    clearance, lens = INF, []

    def slots(k):
        at = np.clip(np.searchsorted(keys, k), 0, max(len(keys) - 1, 0))
        found = (keys[at] == k) if len(keys) else np.zeros(len(k), bool)
        return at[found]

    for posed, origin in clouds:
        posed = f32(posed)[:, :3]
        posed = posed[np.isfinite(posed).all(axis=1)]
        bc, ok = build_cells(posed, res)
        skipped += int((~ok).sum())
        posed, bc = posed[ok], bc[ok]
        hit[slots(pack(bc))] = True
        w = walk_many(origin, posed, res, margin, min_range, max_range)
        cast += int(w["cast"].sum())
        skipped += int((~w["cast"]).sum())
        visited += int(w["n"].sum())
        np.add.at(miss, slots(pack(w["cells"])), 1)
        if w["cast"].any():
            clearance = min(clearance, float(w["clearance"][w["cast"]].min()))
            lens.append(w["len"][w["cast"]])
    if min_clearance is not None:
        assert clearance >= min_clearance, clearance
    return dict(cells=vox, miss=miss, hit=hit, cast=cast, skipped=skipped, visited=visited, clearance=clearance,
                mean_len=float(np.concatenate(lens).mean()) if lens else 0.0)


def removed_cells(counts, min_rays):
    """the cells a clearing removes"""
    return counts["cells"][(counts["miss"] >= min_rays) & ~counts["hit"]]


def clear_mask(points, origin, res, margin=0.0, min_range=0.0, max_range=INF, max_drop=0.01):
    """which points keep a clearance >= CLEAR on their rays from `origin` (non-finite rows and rays that are not cast stay);
    at most max_drop of them may go"""
    points = f32(points)[:, :3]
    fin = np.isfinite(points).all(axis=1)
    w = walk_many(origin, np.where(fin[:, None], points, 1.0), res, margin, min_range, max_range)
    keep = ~fin | ~w["cast"] | (w["clearance"] >= CLEAR)
    assert (~keep).sum() <= max_drop * max(len(points), 1), ((~keep).sum(), len(points))
    return keep


def clear_points(points, origin, res, margin=0.0, min_range=0.0, max_range=INF, max_drop=0.01):
    points = f32(points)
    return points[clear_mask(points, origin, res, margin, min_range, max_range, max_drop)]


def off_faces(rng, xyz, leaf):
    """every coordinate moved into the middle nine tenths of its cell: far from the origin f32 coordinates are multiples of
    2^-7 m and one in a hundred would lie exactly on a face of a dyadic leaf (a ray ending there has t = t_end)"""
    cell = np.floor(np.asarray(xyz, np.float64) / leaf)
    return ((cell + rng.uniform(0.05, 0.95, cell.shape)) * leaf).astype(np.float32)


def random_rays(seed, n, leaf, reach=60.0, centre=(0.0, 0.0, 0.0)):
    """n rays from one origin near `centre` to points up to `reach` away, the unclear ones dropped -> (origin, points)"""
    rng = np.random.default_rng(seed)
    origin = off_faces(rng, np.asarray(centre) + rng.uniform(-2, 2, 3), leaf)
    pts = off_faces(rng, np.asarray(centre) + rng.uniform(-reach, reach, (n, 3)) * np.array([1.0, 1.0, 0.3]), leaf)
    return origin, clear_points(pts, origin, leaf)


# the hand cases of the definition at leaf 1: (origin, point, margin, cells or None when nothing is cast)
HAND = [
    ((0.5, 0.5, 0.5), (3.5, 0.5, 0.5), 0.0, [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)]),
    ((0.5, 0.5, 0.5), (3.5, 0.5, 0.5), 1.0, [(0, 0, 0), (1, 0, 0), (2, 0, 0)]),
    ((0.5, 0.5, 0.5), (-2.5, 0.5, 0.5), 0.25, [(0, 0, 0), (-1, 0, 0), (-2, 0, 0), (-3, 0, 0)]),
    ((0.25, 0.25, 0.5), (2.25, 2.25, 0.5), 0.0, [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 2, 0)]),
    ((1.0, 0.5, 0.5), (-0.5, 0.5, 0.5), 0.0, [(1, 0, 0), (0, 0, 0), (-1, 0, 0)]),     # a start on a face, d < 0: a step at t = 0
    ((1.0, 0.5, 0.5), (2.5, 0.5, 0.5), 0.0, [(1, 0, 0), (2, 0, 0)]),                  # the same start, d > 0
    ((0.5, 0.5, 0.5), (1.5, 0.5, 0.5), 1.0, None),                                     # margin == len
    ((0.5, 0.5, 0.5), (1.5, 0.5, 0.5), 2.5, None),                                     # margin > len
    ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 0.0, None),                                     # len == 0
]
