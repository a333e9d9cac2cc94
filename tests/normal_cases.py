"""A numpy restatement of the normals contract (include/ndt_mi355.h, "surface normals and curvature of resident clouds"), written
from the contract alone, and the clouds the tests use.  Shared by tests/test_normal_cases.py (CPU: this file against
ndt_host_normal_from_sums, the conditioning of every case), tests/test_gpu_normals.py and its child tests/normals_child.py.

The reference: d2 by brute force in f32 with the contract's parenthesisation, the stable (d2, index) order, sums about the query in
f64 (numpy's order of summation, not the device's: the comparison rules below allow for it), numpy.linalg.eigh, the orientation, the
curvature, the NaN rules and the filter's predicate.

Comparison rules (derived, not measured; u = 2^-53): counts, n_finite, n_valid, max_neighbors and which records are NaN are exact.
Every term of S2 is at most R^2 (R: the largest neighbour distance of the point), so an entry of C carries at most about
(m + 8) u R^2 < 1e-13 R^2 at m <= 256 and Jacobi adds a few tens of u |C|.  The eigenvector's angle error is at most |E| / (l1 - l0):
on WELL-CONDITIONED points -- (l1 - l0) >= 1e-4 R^2 by the reference's values -- below 1e-9, far under the f32 rounding of the output,
and each component is compared to 2^-24 absolute (up to a common sign where the reference's |s| <= 1e-9 |v - p|).  On every valid
point: | |n| - 1 | <= 2^-22, |C_ref n - l0_ref n| <= 4 * 2^-24 t_ref, n . (v - p) >= -2^-22 |v - p|, and |c - c_ref| <= 2^-24 c_ref
+ 1e-9 (t >= R^2 / (2 m): the query and the farthest member are both in the set, so the f64 error stays under 1e-10).  A case that
compares directions may have at most 10 % of its valid points ill-conditioned (tests/test_normal_cases.py asserts it per case)."""
import lzma
import os

import numpy as np

F = np.float32
KNN, RADIUS = 1, 2
KEEP_CURVATURE, KEEP_ANGLE, KEEP_NEGATE = 1, 2, 4
COLLINEAR = 1e-12
WELL = 1e-4
ILL_CAP = 0.10
QNAN_BITS = 0x7FC00000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def spec(k=None, radius=None, min_neighbors=3, viewpoint=(0.0, 0.0, 0.0)):
    assert (k is None) != (radius is None)
    return dict(method=KNN if k is not None else RADIUS, k=int(k or 0), radius=float(F(radius or 0.0)), min_neighbors=int(min_neighbors),
                viewpoint=tuple(float(v) for v in viewpoint))


def kw_of(sp):
    """the wrapper's keywords of a spec"""
    kw = dict(min_neighbors=sp["min_neighbors"], viewpoint=sp["viewpoint"])
    kw["k" if sp["method"] == KNN else "radius"] = sp["k"] if sp["method"] == KNN else sp["radius"]
    return kw


def tag_of(sp):
    return ("k=%d" % sp["k"] if sp["method"] == KNN else "r=%g" % sp["radius"]) + (" min=%d" % sp["min_neighbors"] if sp["min_neighbors"] != 3 else "") + (
        " vp=%g,%g,%g" % sp["viewpoint"] if any(sp["viewpoint"]) else "")


def finite_mask(xyz):
    return np.isfinite(xyz[:, :3]).all(axis=1) if len(xyz) else np.zeros(0, bool)


def d2_rows(xyz, rows, cols=None):
    """d2(i, j) = (dx*dx + dy*dy) + dz*dz in f32, every operation rounded on its own: (len(rows), len(cols))"""
    a = np.asarray(xyz, F)[:, :3]
    q = a[rows]
    p = a if cols is None else a[cols]
    with np.errstate(all="ignore"):
        dx, dy, dz = (q[:, None, c] - p[None, :, c] for c in range(3))
        return ((dx * dx + dy * dy) + dz * dz).astype(F)


def neighbourhoods(xyz, sp, rows=None):
    """per row of `rows` (default: every point): the indices of its neighbourhood in the contract's order, None outside F"""
    xyz = np.asarray(xyz, F)
    fin = finite_mask(xyz)
    idx_f = np.flatnonzero(fin)
    rows = np.arange(len(xyz)) if rows is None else np.asarray(rows)
    out = [None] * len(rows)
    r2 = F(sp["radius"]) * F(sp["radius"])
    todo = [j for j, i in enumerate(rows) if fin[i]]
    for lo in range(0, len(todo), 256):
        part = todo[lo:lo + 256]
        d2 = d2_rows(xyz, rows[part], idx_f)
        for row, j in zip(d2, part):
            if sp["method"] == KNN:
                order = np.lexsort((idx_f, row))  # ascending (d2, index), stable
                out[j] = idx_f[order[:min(sp["k"], len(idx_f))]]
            else:
                out[j] = idx_f[row <= r2]
    return out


def sums_about(xyz, i, nb):
    """S1 (3) and S2 (6: xx xy xz yy yz zz) of the neighbours about the query, f64"""
    e = np.asarray(xyz, F)[nb, :3].astype(np.float64) - np.asarray(xyz, F)[i, :3].astype(np.float64)
    S2 = np.array([(e[:, a] * e[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
    return e.sum(axis=0), S2


def nan_record():
    return np.full(4, QNAN_BITS, np.uint32).view(F)


def record_from_sums(sp, p, m, S1, S2):
    """-> dict(record (4,) f32, valid, collinear, C (3, 3), l (3,), t, s): the contract's steps 1 ... 9 with numpy.linalg.eigh"""
    out = dict(record=nan_record(), valid=False, collinear=False, C=None, l=None, t=0.0, s=0.0)
    if m < sp["min_neighbors"] or m < 1:
        return out
    with np.errstate(all="ignore"):
        mu = np.asarray(S1, np.float64) / m
        s2 = np.asarray(S2, np.float64) / m
        C = np.array([[s2[0], s2[1], s2[2]], [s2[1], s2[3], s2[4]], [s2[2], s2[4], s2[5]]]) - np.outer(mu, mu)
    out["C"] = C
    if not np.isfinite(C).all():
        return out
    l, V = np.linalg.eigh(C)
    t = float(l.sum())
    out.update(l=l, t=t)
    if not t > 0.0:
        return out
    n = V[:, 0] / np.linalg.norm(V[:, 0])
    v = np.asarray(sp["viewpoint"], np.float64) - np.asarray(p, F).astype(np.float64)
    s = float(n @ v)
    if s < 0.0 or (s == 0.0 and n[int(np.argmax(np.abs(n)))] < 0.0):
        n = -n
    rec = np.array([n[0], n[1], n[2], max(l[0], 0.0) / t]).astype(F)
    out.update(record=rec, valid=True, collinear=bool(l[1] <= COLLINEAR * l[2]), s=s)
    return out


def reference(xyz, sp, rows=None):
    """The contract on the rows `rows` (default: all) of the cloud: records (r, 4) f32, counts (r,) int32, valid, collinear, well
    (bool: valid and well-conditioned), near_line (valid, l1 within a factor 10 of the collinear cut), C (r, 3, 3), l (r, 3), t, s,
    R2 (the largest neighbour d2) -- and, over all rows, stats."""
    xyz = np.asarray(xyz, F)
    rows = np.arange(len(xyz)) if rows is None else np.asarray(rows)
    r = len(rows)
    nbs = neighbourhoods(xyz, sp, rows)
    ref = dict(records=np.tile(nan_record(), (r, 1)), counts=np.zeros(r, np.int32), valid=np.zeros(r, bool), collinear=np.zeros(r, bool),
               well=np.zeros(r, bool), near_line=np.zeros(r, bool), C=np.zeros((r, 3, 3)), l=np.zeros((r, 3)), t=np.zeros(r), s=np.zeros(r),
               R2=np.zeros(r), rows=rows)
    for j, (i, nb) in enumerate(zip(rows, nbs)):
        if nb is None:
            continue
        S1, S2 = sums_about(xyz, i, nb)
        one = record_from_sums(sp, xyz[i, :3], len(nb), S1, S2)
        ref["counts"][j] = len(nb)
        ref["records"][j] = one["record"]
        ref["valid"][j] = one["valid"]
        ref["collinear"][j] = one["collinear"]
        if one["valid"]:
            e = xyz[nb, :3].astype(np.float64) - xyz[i, :3].astype(np.float64)
            R2 = float((e * e).sum(axis=1).max())
            ref["C"][j], ref["l"][j], ref["t"][j], ref["s"][j], ref["R2"][j] = one["C"], one["l"], one["t"], one["s"], R2
            ref["well"][j] = (one["l"][1] - one["l"][0]) >= WELL * R2
            ref["near_line"][j] = COLLINEAR / 10 * one["l"][2] <= one["l"][1] <= COLLINEAR * 10 * one["l"][2]
    ref["stats"] = dict(n_finite=int(finite_mask(xyz).sum()), n_valid=int(ref["valid"].sum()), n_collinear=int(ref["collinear"].sum()),
                        max_neighbors=int(ref["counts"].max()) if r else 0)
    return ref


def ill_fraction(ref):
    """the share of the valid points that are not well-conditioned"""
    v = int(ref["valid"].sum())
    return 0.0 if v == 0 else float((ref["valid"] & ~ref["well"]).sum()) / v


def keep_filter(flags=0, curvature=(0.0, 0.0), axis=(0.0, 0.0, 1.0), cos=(0.0, 1.0)):
    return dict(flags=int(flags), curvature_lo=float(F(curvature[0])), curvature_hi=float(F(curvature[1])), axis=tuple(float(a) for a in axis),
                cos_lo=float(cos[0]), cos_hi=float(cos[1]))


def keep_by(flt, records):
    """the filter's predicate on stored records (n, 4) f32 -> (n,) bool"""
    rec = np.asarray(records, F).reshape(-1, 4)
    valid = ~np.isnan(rec).any(axis=1)
    keep = np.ones(len(rec), bool)
    with np.errstate(invalid="ignore"):
        if flt["flags"] & KEEP_CURVATURE:
            keep &= (F(flt["curvature_lo"]) <= rec[:, 3]) & (rec[:, 3] <= F(flt["curvature_hi"]))
        if flt["flags"] & KEEP_ANGLE:
            n = rec[:, :3].astype(np.float64)
            a = np.abs((n[:, 0] * flt["axis"][0] + n[:, 1] * flt["axis"][1]) + n[:, 2] * flt["axis"][2])
            keep &= (flt["cos_lo"] <= a) & (a <= flt["cos_hi"])
    if flt["flags"] & KEEP_NEGATE:
        keep = ~keep
    return keep & valid


def filter_margin(flt, records):
    """how far the valid records' curvatures / cosines keep from the enabled bounds (inf without an enabled test)"""
    rec = np.asarray(records, F).reshape(-1, 4)
    rec = rec[~np.isnan(rec).any(axis=1)].astype(np.float64)
    gaps = [np.inf]
    if flt["flags"] & KEEP_CURVATURE and len(rec):
        gaps += [np.abs(rec[:, 3] - flt["curvature_hi"]).min()]
        if flt["curvature_lo"] > 0.0:  # (a curvature is never negative: a lower bound of 0 decides nothing)
            gaps += [np.abs(rec[:, 3] - flt["curvature_lo"]).min()]
    if flt["flags"] & KEEP_ANGLE and len(rec):
        a = np.abs(rec[:, :3] @ np.asarray(flt["axis"]))
        if flt["cos_hi"] < 1.0 or np.count_nonzero(flt["axis"]) != 1:  # (along a coordinate axis a is one stored component: at most 1)
            gaps += [np.abs(a - flt["cos_hi"]).min()]
        if flt["cos_lo"] > 0.0:
            gaps += [np.abs(a - flt["cos_lo"]).min()]
    return float(min(gaps))


# ---------------------------------------------------------------------------------------------------- comparison
def compare(got_records, got_counts, ref, sp, xyz, directions=True):
    """The comparison rules of the module's docstring on the rows of `ref`; returns the list of what is violated (empty: fine).
    directions=False: the property checks of rule 5 alone (cases whose conditioning is out of the cap)."""
    bad = []
    rows = ref["rows"]
    got = np.asarray(got_records, F).reshape(-1, 4)[rows]
    if got_counts is not None and not np.array_equal(np.asarray(got_counts)[rows], ref["counts"]):
        bad.append("counts differ at rows %s" % rows[np.flatnonzero(np.asarray(got_counts)[rows] != ref["counts"])[:5]])
    nan_got = np.isnan(got).any(axis=1)
    if not np.array_equal(nan_got, ~ref["valid"]):
        bad.append("NaN records differ at rows %s" % rows[np.flatnonzero(nan_got != ~ref["valid"])[:5]])
        return bad
    if not (got.view(np.uint32)[nan_got] == QNAN_BITS).all():
        bad.append("an invalid record is not four quiet NaNs")
    v = np.flatnonzero(ref["valid"])
    if not len(v):
        return bad
    n = got[v, :3].astype(np.float64)
    p = np.asarray(xyz, F)[rows[v], :3].astype(np.float64)
    view = np.asarray(sp["viewpoint"], np.float64)[None, :] - p
    vlen = np.linalg.norm(view, axis=1)
    if (np.abs(np.linalg.norm(n, axis=1) - 1.0) > 2.0 ** -22).any():
        bad.append("a normal is not a unit vector to 2^-22")
    res = np.linalg.norm(np.einsum("rab,rb->ra", ref["C"][v], n) - ref["l"][v, 0:1] * n, axis=1)
    if (res > 4 * 2.0 ** -24 * ref["t"][v]).any():
        w = int(np.argmax(res / ref["t"][v]))
        bad.append("residual |C n - l0 n| = %.3g t at row %d" % (res[w] / ref["t"][v][w], rows[v][w]))
    if ((n * view).sum(axis=1) < -2.0 ** -22 * vlen).any():
        bad.append("a normal points away from the viewpoint")
    c, c_ref = got[v, 3].astype(np.float64), ref["records"][v, 3].astype(np.float64)
    if (np.abs(c - c_ref) > 2.0 ** -24 * c_ref + 1e-9).any():
        w = int(np.argmax(np.abs(c - c_ref)))
        bad.append("curvature %.9g vs %.9g at row %d" % (c[w], c_ref[w], rows[v][w]))
    if directions:
        w = np.flatnonzero(ref["well"][v])
        nw, rw = n[w], ref["records"][v[w], :3].astype(np.float64)
        either = np.abs(ref["s"][v[w]]) <= 1e-9 * vlen[w]
        err = np.abs(nw - rw).max(axis=1)
        err = np.where(either, np.minimum(err, np.abs(nw + rw).max(axis=1)), err)
        if (err > 2.0 ** -24).any():
            k = int(np.argmax(err))
            bad.append("direction off by %.3g at row %d" % (err[k], rows[v[w]][k]))
    return bad


# ---------------------------------------------------------------------------------------------------- clouds
def surface(n, seed, scale=6.0, noise=0.01, offset=(0.0, 0.0, 0.0)):
    """n points of a gently curved, slightly noisy surface in front of the origin's sensor"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-scale, scale, n), rng.uniform(-scale, scale, n)
    z = 0.08 * np.sin(0.9 * x) * scale + 0.05 * np.cos(0.7 * y) * scale - 2.0 + rng.normal(0.0, noise, n)
    return (np.stack([x, y, z], axis=1) + np.asarray(offset)).astype(F)


def blob(n, seed, sigma=(1.0, 0.6, 0.15), centre=(0.0, 0.0, 3.0)):
    rng = np.random.default_rng(seed)
    return (rng.normal(0.0, 1.0, (n, 3)) * np.asarray(sigma) + np.asarray(centre)).astype(F)


def with_rows(xyz, rows, value=np.nan):
    out = np.array(xyz, F)
    for j, r in enumerate(rows):
        out[r, j % 3] = value
    return out


def lattice(side):
    g = np.arange(side)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(F) + F(1.0)


def radius_edge():
    """the query (row 0, at the origin: with the default viewpoint also the s == 0 rule) with points exactly on, one ulp inside and one ulp outside the radius 0.5 on each
    axis, and a few near points that make it a neighbourhood"""
    r = F(0.5)
    q = np.zeros(3, F)  # (offsets of one ulp of 0.5 survive the addition only here)
    steps = [r, np.nextafter(r, F(0)), np.nextafter(r, F(1))]
    pts = [q]
    for a in range(3):
        for sgn in (1, -1):
            for s in steps:
                e = np.zeros(3, F)
                e[a] = F(sgn) * s
                pts.append(q + e)
    rng = np.random.default_rng(5)
    pts += list((q + rng.uniform(-0.2, 0.2, (9, 3))).astype(F))
    return np.array(pts, F)


def golden_scan():
    """the golden scan tests/golden/251370668.pcd.xz thinned to the first point of every 0.5 m cell: 2 683 points"""
    raw = lzma.open(os.path.join(GOLDEN, "251370668.pcd.xz")).read()
    body = raw[raw.index(b"\n", raw.index(b"DATA binary")) + 1:]
    pts = np.frombuffer(body, F).reshape(-1, 4)[:, :3]
    cell = np.floor(pts.astype(np.float64) / 0.5).astype(np.int64)
    _, first = np.unique(cell, axis=0, return_index=True)
    return np.ascontiguousarray(pts[np.sort(first)])


ABOVE = (0.0, 0.0, 30.0)
SIZES = (7, 8, 9, 63, 64, 65, 511, 512, 513)
NEAR_K = (3, 5, 8, 9, 16, 17, 64, 256)


def gpu_cases():
    """name -> (xyz, [(spec, directions)]): the clouds of tests/test_gpu_normals.py.  directions False: rule 5's property checks
    alone (the case's conditioning is out of the cap, or every record is degenerate by construction)."""
    c = {}
    both = [(spec(k=8), True), (spec(radius=1.2), True)]
    for n in (0, 1, 2, 3):
        c["tiny n=%d" % n] = (surface(n, 40 + n), [(spec(k=3), False), (spec(k=5), False), (spec(radius=100.0), False)])
    c["|F| < k"] = (surface(6, 46), [(spec(k=10), True), (spec(k=256), True)])
    c["|F| < min_neighbors"] = (with_rows(surface(9, 47), (1, 4, 5, 8)), [(spec(k=10, min_neighbors=8), False), (spec(radius=50.0, min_neighbors=6), False)])
    for n in SIZES:
        c["size n=%d" % n] = (surface(n, n, scale=1.0 + n ** 0.5 / 4), both)
    c["non-finite rows"] = (with_rows(with_rows(surface(300, 50), [0, 299, 17, 101], np.nan), list(range(8, 16)) + [200, 250], np.inf), both)
    dup = surface(200, 51)
    dup[100:150] = dup[0:50]
    c["duplicates"] = (dup, both)
    c["every point equal"] = (np.tile(np.array([[1.5, -2.0, 0.25]], F), (70, 1)), [(spec(k=8), False), (spec(radius=1.0), False)])
    g = np.arange(12)
    plane = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2).astype(F)
    c["an exact plane"] = (np.concatenate([plane, np.full((len(plane), 1), 3.0, F)], axis=1), [(spec(k=9), True), (spec(radius=1.5), True)])
    c["an exact line"] = (np.stack([np.arange(40), 2 * np.arange(40), np.full(40, 5)], axis=1).astype(F), [(spec(k=5), False), (spec(radius=7.0), False)])
    c["an integer lattice"] = (lattice(6), [(spec(k=5), False), (spec(k=7), False), (spec(k=27), False)])
    c["on the radius"] = (radius_edge(), [(spec(radius=0.5), True)])
    c["1000+ neighbours in one cell"] = (blob(1300, 52, sigma=(0.1, 0.08, 0.02)), [(spec(radius=1.0), True)])
    c["1000+ neighbours over many cells"] = (surface(3600, 53, scale=1.5, noise=0.004), [(spec(radius=1.0), True)])
    c["100 km from the origin"] = (surface(1500, 54, scale=2.0, offset=(1.0e5, -1.0e5, 50.0)), [(spec(k=10), True), (spec(radius=0.1), True), (spec(radius=0.6), True)])
    far = np.concatenate([blob(600, 55, sigma=(0.5, 0.4, 0.1)), np.array([[400, 0, 3], [0, -500, 2], [380, 420, -6], [-450, 30, 9]], F)])
    c["a blob and far points"] = (far, [(spec(k=8), True), (spec(radius=0.4), True)])
    scan = golden_scan()
    c["golden scan"] = (scan, [(spec(k=5), True), (spec(k=10), True), (spec(k=20), True), (spec(radius=0.8), True), (spec(radius=1.5), True),
                               (spec(k=10, viewpoint=ABOVE), True), (spec(radius=1.5, viewpoint=ABOVE), True), (spec(k=3), False)])
    return c


def near_k_clouds(k):
    """the clouds of k ... k + 9 points"""
    return [surface(k + d, 1000 + 10 * k + d, scale=1.0 + k ** 0.5 / 3) for d in range(10)]


# which route the search of a case takes (ndt_diag_normals' scanned_queries > 0)
ROUTES = {("a blob and far points", "k=8"): "scan", ("100 km from the origin", "r=0.1"): "scan",
          ("1000+ neighbours over many cells", "r=1"): "shells"}

RAGGED = ("size n=65", "tiny n=0", "non-finite rows", "tiny n=2", "size n=7", "every point equal", "duplicates", "tiny n=0", "size n=513")
