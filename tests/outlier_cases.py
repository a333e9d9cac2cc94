"""The outlier filters of include/ndt_mi355.h restated in numpy FROM THE DEFINITIONS (not from the kernel), and the clouds
the tests run them on.

F = the rows whose three coordinates are finite.  d2(i, j) = (dx*dx + dy*dy) + dz*dz in f32, every operation rounded on its
own (numpy never fuses).  The other points of i are the j in F with j != i by index.
  RADIUS       value_i = the number of other points with d2 <= radius*radius (f32 product)
  STATISTICAL  value_i = (sum, f64, ascending d2, of sqrt((double)d2) over the mean_k smallest d2) / mean_k if |F| > mean_k,
               else 0; mean / stddev (n - 1) over F; threshold = mean + stddev_mul * stddev
A row outside F has value NaN and is never kept."""
import math

import numpy as np

F32 = np.float32
RADIUS, STATISTICAL = 1, 2


def finite_rows(xyz):
    return np.isfinite(np.asarray(xyz, dtype=F32)[:, :3]).all(axis=1)


def _d2_rows(pts, rows):
    """(len(rows), len(pts)) f32 squared distances from pts[rows] to every point of pts, the rows' own entries set to inf"""
    q = pts[rows]
    with np.errstate(over="ignore"):
        dx = q[:, None, 0] - pts[None, :, 0]
        dy = q[:, None, 1] - pts[None, :, 1]
        dz = q[:, None, 2] - pts[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == F32
    d2[np.arange(len(rows)), rows] = np.inf  # j != i by index: a duplicate elsewhere stays a neighbour at distance 0
    return d2


def radius_counts(xyz, radius, step=256):
    """(n,) float64: the count of every row of F, NaN elsewhere"""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=F32)[:, :3])
    fin = finite_rows(xyz)
    pts = xyz[fin]
    r2 = F32(radius) * F32(radius)
    out = np.full(len(xyz), np.nan)
    counts = np.zeros(len(pts))
    for a in range(0, len(pts), step):
        rows = np.arange(a, min(a + step, len(pts)))
        counts[rows] = (_d2_rows(pts, rows) <= r2).sum(axis=1)
    out[fin] = counts
    return out


def knn_mean_distances(xyz, mean_k, step=256):
    """(n,) float64: the STATISTICAL value of every row of F, NaN elsewhere"""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=F32)[:, :3])
    fin = finite_rows(xyz)
    pts = xyz[fin]
    out = np.full(len(xyz), np.nan)
    vals = np.zeros(len(pts))
    if len(pts) > mean_k:
        for a in range(0, len(pts), step):
            rows = np.arange(a, min(a + step, len(pts)))
            d2 = _d2_rows(pts, rows)
            near = np.sort(np.partition(d2, mean_k - 1, axis=1)[:, :mean_k], axis=1)  # the mean_k smallest, ascending
            terms = np.sqrt(near.astype(np.float64))
            vals[rows] = np.cumsum(terms, axis=1)[:, -1] / mean_k  # (cumsum adds in order)
    out[fin] = vals
    return out


def reference(xyz, method, radius=None, min_neighbors=None, mean_k=None, stddev_mul=None, negate=False):
    """dict(values, keep, n_finite, n_valid, mean, stddev, threshold) from the definitions"""
    fin = finite_rows(xyz)
    nf = int(fin.sum())
    if method == RADIUS:
        values = radius_counts(xyz, radius)
        thr = float(min_neighbors)
        with np.errstate(invalid="ignore"):
            inside = values >= thr
        stats = dict(n_finite=nf, n_valid=nf, mean=0.0, stddev=0.0, threshold=thr)
    else:
        values = knn_mean_distances(xyz, mean_k)
        if nf > mean_k:
            v = values[fin]
            mean = math.fsum(v) / nf
            sd = math.sqrt(math.fsum((v - mean) ** 2) / (nf - 1)) if nf >= 2 else 0.0
            stats = dict(n_finite=nf, n_valid=nf, mean=mean, stddev=sd, threshold=mean + stddev_mul * sd)
        else:
            stats = dict(n_finite=nf, n_valid=0, mean=0.0, stddev=0.0, threshold=0.0)
        with np.errstate(invalid="ignore"):
            inside = values <= stats["threshold"]
    keep = fin & (~inside if negate else inside)
    return dict(values=values, keep=keep, **stats)


def threshold_margin(ref):
    """the smallest |value - threshold| over F, relative to the threshold's size (inf for an empty F)"""
    v = ref["values"][np.isfinite(ref["values"])]
    if len(v) == 0:
        return math.inf
    return float(np.abs(v - ref["threshold"]).min() / max(abs(ref["threshold"]), 1e-300))


def keep_by(values, threshold, method, negate=False):
    """the kept set a call must return given ITS OWN values and threshold"""
    values = np.asarray(values)
    with np.errstate(invalid="ignore"):
        inside = values >= threshold if method == RADIUS else values <= threshold
    return ~np.isnan(values) & (~inside if negate else inside)


# ---------------------------------------------------------------------------------------------------- clouds
def surface(n, seed, outliers=0, scale=10.0, offset=(0.0, 0.0, 0.0)):
    """n points on a wavy sheet of `scale` metres with a little noise; the first `outliers` of them lifted far off it"""
    rng = np.random.default_rng(seed)
    u = rng.random((n, 2)) * scale
    z = 0.3 * np.sin(u[:, 0]) * np.cos(0.7 * u[:, 1]) + 0.01 * rng.standard_normal(n)
    p = np.column_stack([u, z])
    p[:outliers, 2] += 3.0 + 5.0 * rng.random(outliers)
    return (p + np.asarray(offset)).astype(F32)


def lattice(m=3, pitch=1.0):
    a = np.arange(m, dtype=F32) * F32(pitch)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)


def lattice_class(m=3):
    """per lattice point the number of its coordinates that are interior: 0 corner, 1 edge, 2 face, 3 centre (m = 3)"""
    p = lattice(m)
    return ((p > 0) & (p < m - 1)).sum(axis=1)


def with_nonfinite(xyz, every=5):
    """a copy with NaN / +inf / -inf rows interleaved (every `every`-th row, one bad coordinate in turn)"""
    out = np.array(xyz, dtype=F32, copy=True)
    bad = [np.nan, np.inf, -np.inf]
    for c, r in enumerate(range(1, len(out), every)):
        out[r, c % 3] = bad[c % 3]
    return out


def line(n, seed=0):
    t = np.sort(np.random.default_rng(seed).random(n)) * 20
    return np.column_stack([t, 0.5 * t, np.full(n, 2.0)]).astype(F32)


def plane(n, seed=0):
    u = np.random.default_rng(seed).random((n, 2)) * 8
    return np.column_stack([u, np.full(n, -1.0)]).astype(F32)


def duplicate_pairs(n_pairs, seed=0):
    p = surface(n_pairs, seed)
    return np.repeat(p, 2, axis=0)


def identical(n):
    return np.tile(np.array([[1.5, -2.25, 0.75]], F32), (n, 1))


def clustered(sizes, seed=0, gap=50.0, spread=0.4):
    """clusters of the given sizes, `gap` metres apart on a line: cells of 1 ... len(sizes) points, and isolated ones"""
    rng = np.random.default_rng(seed)
    parts = [np.array([gap * k, 0, 0]) + spread * rng.random((s, 3)) for k, s in enumerate(sizes)]
    return np.concatenate(parts).astype(F32)


def with_far_points(xyz, far=((4000.0, 0, 0), (-3000.0, 2500.0, 0), (0, 0, 5000.0))):
    """the cloud plus a few points so far away that no shell walk can reach their neighbours within its limit"""
    return np.concatenate([np.asarray(xyz, F32), np.asarray(far, F32)])


def sphere_rows():
    """exactly representable rows about the origin point (row 0): d2 = 25 (three ways), 24, 26, 0 (a duplicate of row 0)"""
    return np.array([[0, 0, 0], [3, 4, 0], [0, -3, 4], [-5, 0, 0], [4, 2, 2], [5, 1, 0], [0, 0, 0], [40, 40, 40]], F32)


# ---------------------------------------------------------------------------------------------------- the cases of the GPU tests
def stat(k, mul=1.0, negate=False):
    return dict(method=STATISTICAL, mean_k=k, stddev_mul=mul, negate=negate)


def rad(r, m, negate=False):
    return dict(method=RADIUS, radius=float(F32(r)), min_neighbors=m, negate=negate)


MEAN_K_EDGES = (1, 2, 8, 9, 64, 65, 256)
UP5, DOWN5 = float(np.nextafter(F32(5), F32(6))), float(np.nextafter(F32(5), F32(4)))


def gpu_cases():
    """name -> (xyz, [spec, ...]): every cloud the GPU tests compare kept sets on, with the specs it is filtered under
    (tests/test_outlier_cases.py holds the reference's own values clear of its thresholds on exactly these)"""
    c = {}
    for n in (1, 2, 7, 8, 9, 16, 17):  # teams of a wave, either side of one block
        c["plan n=%d" % n] = (surface(n, 100 + n, scale=2.0), [stat(1), stat(2), rad(0.7, 1), rad(0.7, 0)])
    base = surface(3000, 7, outliers=12)
    c["surface"] = (base, [stat(k) for k in MEAN_K_EDGES] + [stat(8, 1.0, True), stat(20, 2.5), stat(8, -0.5), rad(0.3, 3), rad(0.3, 3, True),
                           rad(1e-5, 1), rad(100.0, 2999), rad(100.0, 3000), rad(0.3, 0), rad(2.5, 40)])
    c["surface, no stray point"] = (surface(3000, 7), [stat(8), rad(0.3, 3)])
    for k in MEAN_K_EDGES:
        for d in (0, 1, 2):  # |F| = mean_k, mean_k + 1, mean_k + 2 (two NaN rows besides)
            p = surface(k + d + 2, 1000 + 3 * k + d, scale=3.0)
            p[[0, k + d + 1]] = np.nan
            c["|F| = %d + %d" % (k, d)] = (p, [stat(k), stat(k, 0.0, True)])
    c["non-finite rows"] = (with_nonfinite(base[:1500]), [stat(8), rad(0.3, 3), rad(0.3, 3, True)])
    bad = np.full((20, 3), np.nan, F32)
    bad[::3, 1] = np.inf
    bad[1::3] = (1, -np.inf, 2)
    c["every row non-finite"] = (bad, [stat(2), rad(1.0, 0), rad(1.0, 0, True)])
    one = bad.copy()
    one[11] = (3, 4, 5)
    c["a single finite row"] = (one, [stat(1), rad(1.0, 0), rad(1.0, 1)])
    c["every point identical"] = (identical(300), [stat(8), stat(256), stat(8, 0.0, True), rad(0.5, 299), rad(0.5, 300)])
    c["duplicate pairs"] = (duplicate_pairs(400, 5), [stat(1), stat(2), rad(1e-6, 1), rad(1e-6, 2)])
    c["a line"] = (line(500), [stat(8), rad(0.5, 2)])
    c["a plane"] = (plane(1500), [stat(8), rad(0.5, 2)])
    c["one occupied cell"] = (surface(200, 9, scale=0.05, offset=(0.3, 0.3, 0.3)), [rad(1.0, 5), rad(1.0, 200), stat(8)])
    c["cells of 1 ... 129 points"] = (clustered(range(1, 130), 4, gap=20.0), [rad(0.8, 10), stat(1), stat(9)])
    c["100 km from the origin"] = (surface(2000, 3, offset=(1e5, -1e5, 50.0)), [stat(8), rad(0.05, 1), rad(0.5, 3)])
    c["far points"] = (with_far_points(surface(3000, 7), far=((60.0, 0, 0), (-40.0, 45.0, 0), (0, 0, 70.0))), [stat(8), stat(65)])
    c["on the sphere"] = (sphere_rows(), [rad(5.0, m) for m in (0, 1, 5, 6)] + [rad(UP5, 5), rad(DOWN5, 2), rad(DOWN5, 3), rad(5.0, 5, True)])
    return c


RAGGED_SPECS = (stat(8, 1.0), stat(8, 0.5, True), rad(0.4, 4), rad(0.4, 4, True))


def ragged():
    """the clouds of the many-clouds tests: empty ones, |F| <= mean_k = 8, no finite row, NaN rows, unequal sizes"""
    c = gpu_cases()
    base = c["surface"][0]
    return [base[:1500], base[:0], base[:7].copy(), with_nonfinite(base[1500:2600]), c["every row non-finite"][0], base[2600:], base[:0],
            c["a line"][0]]


_refs = {}


def reference_of(name, xyz, spec):
    """reference(xyz, **spec), computed once per (case, spec)"""
    key = (name, tuple(sorted(spec.items())))
    if key not in _refs:
        _refs[key] = reference(xyz, **spec)
    return _refs[key]
