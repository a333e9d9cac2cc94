"""The Euclidean cluster extraction of include/ndt_mi355.h restated in numpy FROM THE DEFINITIONS (not from the kernels), and
the clouds the tests run it on.

F = the rows whose three coordinates are finite.  d2(i, j) = (dx*dx + dy*dy) + dz*dz in f32, every operation rounded on its
own (numpy never fuses); tol2 = tolerance*tolerance in f32.  i ~ j iff both in F, i != j by index and d2(i, j) <= tol2.
  component  a connected component of (F, ~): its root is its smallest index, its size its number of points
  cluster    a component with min_size <= size <= max_size; numbered by descending size, equal sizes by ascending root
  label_i    the number of i's cluster, -1 in no cluster or outside F;  root_i: the root of i's component, -1 outside F
The device computes the same f32 d2, so labels, roots, sizes, tables, indices and boxes compare EXACTLY on every cloud -- no
clearance from tol2 is needed.  Centroids: the f64 sum of the widened coordinates / size, here by math.fsum; a sum of `size`
terms in any order is within size * 2^-53 * sum|x| of it (centroid_bound)."""
import math

import numpy as np

import outlier_cases as oc

F32 = np.float32
BIG = 2 ** 31 - 1
CLUSTER_DTYPE = np.dtype([("root", np.int32), ("size", np.int32), ("first", np.uint32), ("box_min", np.float32, 3),
                          ("box_max", np.float32, 3), ("centroid", np.float64, 3)], align=True)


def finite_rows(xyz):
    return np.isfinite(np.asarray(xyz, dtype=F32)[:, :3]).all(axis=1)


def edge_list(xyz, tolerance, step=256):
    """(m, 2) int64: every pair (i, j), j < i, both in F, with d2(i, j) <= tol2 -- brute force over all pairs, in chunks of rows"""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=F32)[:, :3])
    fin = finite_rows(xyz)
    ids = np.flatnonzero(fin)
    pts = xyz[fin]
    tol2 = F32(tolerance) * F32(tolerance)
    out = []
    for a in range(0, len(pts), step):
        rows = np.arange(a, min(a + step, len(pts)))
        q = pts[rows]
        with np.errstate(over="ignore"):
            dx = q[:, None, 0] - pts[None, :, 0]
            dy = q[:, None, 1] - pts[None, :, 1]
            dz = q[:, None, 2] - pts[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == F32
        hit = (d2 <= tol2) & (np.arange(len(pts))[None, :] < rows[:, None])  # j < i: by index, and each pair once
        r, c = np.nonzero(hit)
        out.append(np.column_stack([ids[rows[r]], ids[c]]))
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 2), np.int64)


def component_roots(n, fin, edges):
    """(n,) int32: per row the smallest index of its component (a plain union-find over the edge list), -1 outside F"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, j in edges.tolist():
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    roots = np.array([find(i) for i in range(n)], dtype=np.int32) if n else np.zeros(0, np.int32)
    roots[~fin] = -1
    return roots


def reference(xyz, tolerance, min_size=1, max_size=BIG, roots=None):
    """dict(roots, labels, table (CLUSTER_DTYPE), indices, keep, others, summary) from the definitions (roots: those of an
    earlier call with this cloud and tolerance, which depend on nothing else)"""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=F32)[:, :3])
    n = len(xyz)
    fin = finite_rows(xyz)
    if roots is None:
        roots = component_roots(n, fin, edge_list(xyz, tolerance))
    comp_roots, comp_sizes = np.unique(roots[fin], return_counts=True)
    ok = (comp_sizes >= min_size) & (comp_sizes <= max_size)
    cr, cs = comp_roots[ok], comp_sizes[ok]
    order = np.lexsort((cr, -cs))  # descending size, then ascending root
    cr, cs = cr[order], cs[order]
    number = {int(r): c for c, r in enumerate(cr)}
    labels = np.array([number.get(int(r), -1) for r in roots], dtype=np.int32) if n else np.zeros(0, np.int32)
    table = np.zeros(len(cr), dtype=CLUSTER_DTYPE)
    indices = []
    for c, (r, s) in enumerate(zip(cr, cs)):
        idx = np.flatnonzero(labels == c)  # ascending
        assert len(idx) == s and idx[0] == r
        p = xyz[idx]
        table[c] = (r, s, len(indices), np.minimum.reduce(p), np.maximum.reduce(p),
                    [math.fsum(p[:, a].astype(np.float64)) / s for a in range(3)])
        indices.extend(idx.tolist())
    summary = dict(n_finite=int(fin.sum()), n_components=len(comp_roots), n_clusters=len(cr), n_clustered=int(cs.sum()),
                   largest=int(comp_sizes.max()) if len(comp_sizes) else 0)
    return dict(roots=roots, labels=labels, table=table, indices=np.array(indices, dtype=np.int32), keep=labels >= 0,
                others=fin & (labels < 0), summary=summary)


def centroid_bound(xyz, idx):
    """per axis: size * 2^-53 * sum|x| over the cluster's points"""
    p = np.abs(np.asarray(xyz, dtype=np.float64)[idx, :3])
    return len(idx) * 2.0 ** -53 * p.sum(axis=0)


# ---------------------------------------------------------------------------------------------------- clouds
def chain(n, tolerance, order="shuffled", seed=0):
    """n points on a line at spacing 0.9 * tolerance, stored in shuffled / ascending / descending order: one component"""
    x = (np.arange(n, dtype=np.float64) * 0.9 * tolerance).astype(F32)
    p = np.column_stack([x, np.full(n, 1.0, F32), np.full(n, -2.0, F32)]).astype(F32)
    if order == "descending":
        return p[::-1].copy()
    if order == "shuffled":
        return p[np.random.default_rng(seed).permutation(n)]
    return p


def two_blobs(beyond=False):
    """two lattices of pitch 1 whose closest pair is (0, 0, 0) -- (3, 4, 0): d2 == 25 exactly; every other pair across is
    further.  beyond: the second blob's nearest face one f32 ulp further in x, so that pair's d2 rounds above 25"""
    a = -oc.lattice(4)
    b = oc.lattice(4) + np.array([3, 4, 0], F32)
    if beyond:
        b[b[:, 0] == 3, 0] = np.nextafter(F32(3), F32(4))
    return np.concatenate([a, b]).astype(F32)


def collinear(tolerance, last_ulp=False):
    """three points on the x axis at spacing exactly `tolerance` (a power of two: every product is exact)"""
    t = F32(tolerance)
    x2 = np.nextafter(F32(2) * t, F32(np.inf)) if last_ulp else F32(2) * t
    return np.array([[0, 0, 0], [t, 0, 0], [x2, 0, 0]], F32)


def blobs(sizes, seed=0, gap=20.0, spread=0.4, shuffle=True):
    """blobs of the given sizes, each inside a cube of `spread`, `gap` apart; the rows shuffled so that roots are not in blob order"""
    p = oc.clustered(sizes, seed, gap=gap, spread=spread)
    return p[np.random.default_rng(seed + 1).permutation(len(p))] if shuffle else p


def spec(tolerance, min_size=1, max_size=BIG):
    return dict(tolerance=float(F32(tolerance)), min_size=min_size, max_size=max_size)


UP5, DOWN5 = float(np.nextafter(F32(5), F32(6))), float(np.nextafter(F32(5), F32(4)))
TIE_SIZES = (5, 3, 5, 1, 3, 5, 2, 1, 9, 9, 4)


def gpu_cases():
    """name -> (xyz, [spec, ...]): every cloud the GPU tests compare with the reference, with the specs it is clustered under"""
    c = {}
    for n in (1, 2, 7, 8, 9, 16, 17, 63, 64, 65):  # a pass of eight teams, either side of every step of the plan small clouds reach
        c["plan n=%d" % n] = (oc.surface(n, 100 + n, scale=2.0), [spec(0.7), spec(0.7, 2), spec(0.3, 1, 3)])
    for order in ("shuffled", "ascending", "descending"):
        c["chain, %s" % order] = (chain(4096, 0.5, order), [spec(0.5), spec(0.5, 4096, 4096), spec(0.5, 1, 4095), spec(0.4)])
    c["two blobs at tol2"] = (two_blobs(), [spec(5.0), spec(DOWN5), spec(UP5), spec(5.0, 65, 128)])
    c["two blobs, one ulp beyond"] = (two_blobs(True), [spec(5.0), spec(UP5)])
    c["every point identical"] = (oc.identical(300), [spec(0.5), spec(0.5, 300, 300), spec(0.5, 301), spec(0.5, 1, 299), spec(1e-30)])
    c["duplicate pairs"] = (oc.duplicate_pairs(400, 5), [spec(1e-6), spec(1e-6, 2, 2), spec(1e-6, 1, 1), spec(1e-6, 3)])
    c["one occupied cell"] = (oc.surface(129, 9, scale=0.05, offset=(0.3, 0.3, 0.3)), [spec(1.0), spec(0.004), spec(0.004, 2)])
    base = oc.surface(3000, 7, outliers=12)
    c["components over many cells"] = (base, [spec(0.5), spec(0.5, 10), spec(0.5, 2, 100), spec(0.25, 3)])
    c["every point its own component"] = (oc.surface(1000, 13), [spec(1e-3), spec(1e-3, 2)])
    c["blobs of 1 ... 59 points"] = (blobs(range(1, 60), 4), [spec(0.8), spec(0.8, 10, 50), spec(0.8, 59, 59), spec(0.8, 60), spec(0.8, 1, 1)])
    c["equal sizes"] = (blobs(TIE_SIZES, 6), [spec(0.8), spec(0.8, 3, 5), spec(0.8, 4, 5), spec(0.8, 6, 8)])
    c["far points"] = (oc.with_far_points(oc.surface(3000, 7)), [spec(0.5), spec(0.5, 1, 1)])
    c["non-finite rows"] = (oc.with_nonfinite(base[:1500]), [spec(0.5), spec(0.5, 5)])
    bad = np.full((20, 3), np.nan, F32)
    bad[::3, 1] = np.inf
    bad[1::3] = (1, -np.inf, 2)
    c["every row non-finite"] = (bad, [spec(1.0)])
    one = bad.copy()
    one[11] = (3, 4, 5)
    c["a single finite row"] = (one, [spec(1.0), spec(1.0, 2)])
    c["100 km from the origin"] = (oc.surface(2000, 3, offset=(1e5, -1e5, 50.0)), [spec(0.05), spec(0.5), spec(0.5, 5, 500)])
    c["on the sphere"] = (oc.sphere_rows(), [spec(5.0), spec(DOWN5), spec(5.0, 2)])
    return c


RAGGED_SPECS = (spec(0.5, 5), spec(0.3, 1, 4))


def ragged():
    """the clouds of the many-clouds tests: empty ones, a degenerate one (no finite row), NaN rows, unequal sizes"""
    c = gpu_cases()
    base = c["components over many cells"][0]
    return [base[:1500], base[:0], base[:7].copy(), oc.with_nonfinite(base[1500:2600]), c["every row non-finite"][0], base[2600:], base[:0],
            c["equal sizes"][0], c["chain, shuffled"][0][:700]]


_refs = {}


def reference_of(name, xyz, sp):
    """reference(xyz, **sp), computed once per (case, spec); the components once per (case, tolerance)"""
    key = (name, sp["tolerance"], sp["min_size"], sp["max_size"])
    if key not in _refs:
        shared = _refs.get(key[:2])
        _refs[key] = reference(xyz, roots=None if shared is None else shared["roots"], **sp)
        _refs.setdefault(key[:2], _refs[key])
    return _refs[key]
