"""The plane of a cloud (ndt_cloud_segment_plane, include/ndt_mi355.h) restated in numpy f64, and the fixtures the CPU and the
GPU tests share.  Every operation is an IEEE f64 operation rounded on its own, in the order the header gives, so the models,
distances and counts are the header's to the bit; the refinement's sums are taken exactly (math.fsum), which is what the
device's per-block sums are compared with at a derived bound (refine_bound)."""
import functools
import math

import numpy as np

F = np.float32
D = np.float64
U = 2.0 ** -53
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
VALID, DEGENERATE, REJECTED = 0, 1, 2
# the first outputs of splitmix64 seeded with 0 (Vigna, splitmix64.c)
SPLITMIX64_SEED0 = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC)


def finalise(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def splitmix64(x):
    """the header's splitmix64(x): the finaliser of x + golden"""
    return finalise((x + GOLDEN) & M64)


def sample(seed, h, n):
    return [splitmix64((seed + 3 * h + j) & M64) % n for j in range(3)]


def triples_of(seed, H, n):
    return np.array([sample(seed, h, n) for h in range(H)], dtype=np.int32).reshape(H, 3)


def spec(T, H, seed=0, axis=None, eps=0.0, refine=False):
    return dict(T=float(F(T)), H=int(H), seed=int(seed), axis=None if axis is None else tuple(float(F(v)) for v in axis),
                eps=float(F(eps)), refine=bool(refine))


def params(sp):
    """(T, unit axis or None, cos_eps) as the host computes them once"""
    if sp["axis"] is None:
        return D(sp["T"]), None, D(0.0)
    x, y, z = (D(v) for v in sp["axis"])
    ln = np.sqrt((x * x + y * y) + z * z)
    return D(sp["T"]), np.array([x / ln, y / ln, z / ln]), D(math.cos(sp["eps"]))


def models(xyz, sp, triples):
    """-> (coeffs (H, 4), states (H,), aux): the model of every triple; aux holds len2, uu*vv and the axis dot product"""
    xyz = np.asarray(xyz, dtype=F)
    H = len(triples)
    T, axis, cos_eps = params(sp)
    coeffs, states = np.zeros((H, 4)), np.full(H, DEGENERATE, dtype=np.int32)
    aux = dict(len2=np.full(H, np.nan), uuvv=np.full(H, np.nan), dot=np.full(H, np.nan))
    if len(xyz) < 3 or H == 0:
        return coeffs, states, aux
    t = np.asarray(triples, dtype=np.int64)
    a, b, c = (xyz[t[:, j]].astype(D) for j in range(3))
    same = (t[:, 0] == t[:, 1]) | (t[:, 0] == t[:, 2]) | (t[:, 1] == t[:, 2])
    fin = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
    with np.errstate(all="ignore"):
        u, v = b - a, c - a
        m = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        len2 = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
        uu = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
        vv = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        good = ~same & fin & (len2 > 1e-8 * (uu * vv))
        n = m / np.sqrt(len2)[:, None]
        if axis is not None:
            dot = (n[:, 0] * axis[0] + n[:, 1] * axis[1]) + n[:, 2] * axis[2]
            flip = dot < 0.0
            dot = np.where(flip, -dot, dot)
            ok = dot >= cos_eps
            aux["dot"] = np.where(good, dot, np.nan)
        else:
            last = np.where(n[:, 2] != 0.0, n[:, 2], np.where(n[:, 1] != 0.0, n[:, 1], n[:, 0]))
            flip = last < 0.0
            ok = np.ones(H, dtype=bool)
        n = np.where(flip[:, None], -n, n)
        d = -((n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2])
    coeffs[good, :3] = n[good]
    coeffs[good, 3] = d[good]
    states[good & ok] = VALID
    states[good & ~ok] = REJECTED
    aux["len2"], aux["uuvv"] = np.where(~same & fin, len2, np.nan), np.where(~same & fin, uu * vv, np.nan)
    return coeffs, states, aux


def model(sp, a, b, c, same=False):
    """the model of one triple of f32 points -> ((4,), state)"""
    pts = np.array([a, b, c], dtype=F)
    co, st, _ = models(pts, sp, np.array([[0, 0 if same else 1, 2]]))
    return co[0], int(st[0])


def distances(coeff, xyz):
    """s of every row of the f32 cloud (the raw formula: rows that are not finite give NaN or an infinity)"""
    p = np.asarray(xyz, dtype=F).astype(D).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return ((coeff[0] * p[:, 0] + coeff[1] * p[:, 1]) + coeff[2] * p[:, 2]) + coeff[3]


def inlier(s, T):
    with np.errstate(all="ignore"):
        return (-T <= s) & (s <= T)


def counts(xyz, sp, triples=None):
    """-> (coeffs, states, counts (H,) uint32, triples, aux)"""
    xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
    if triples is None:
        triples = triples_of(sp["seed"], sp["H"], len(xyz)) if len(xyz) else np.zeros((sp["H"], 3), dtype=np.int32)
    triples = np.asarray(triples, dtype=np.int32).reshape(-1, 3)
    co, st, aux = models(xyz, sp, triples)
    T = D(sp["T"])
    cn = np.zeros(len(triples), dtype=np.uint32)
    for h in np.flatnonzero(st == VALID):
        cn[h] = inlier(distances(co[h], xyz), T).sum()
    return co, st, cn, triples, aux


def fit(sp, pts64, a):
    """the refinement's fit of the inliers pts64 (k, 3) f64 about a: exact sums, numpy's symmetric solver
    -> (taken, coeff, lambda ascending, sums dict)"""
    k = len(pts64)
    q = pts64 - a
    S1 = np.array([math.fsum(q[:, i]) for i in range(3)])
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    S2 = np.array([math.fsum(q[:, i] * q[:, j]) for i, j in pairs])
    sums = dict(count=k, S1=S1, S2=S2, M2=float(math.fsum((q * q).sum(1)) / max(k, 1)))
    if k < 3:
        return False, None, None, sums
    mu = S1 / k
    Cm = np.zeros((3, 3))
    for (i, j), v in zip(pairs, S2):
        Cm[i, j] = Cm[j, i] = v / k - mu[i] * mu[j]
    lam, vec = np.linalg.eigh(Cm)
    if not (np.isfinite(lam).all() and lam[1] > 1e-12 * lam[2]):
        return False, None, lam, sums
    n = vec[:, 0] / np.linalg.norm(vec[:, 0])
    _, axis, _ = params(sp)
    if axis is not None:
        if n @ axis < 0:
            n = -n
    else:
        last = n[2] if n[2] != 0 else n[1] if n[1] != 0 else n[0]
        if last < 0:
            n = -n
    c = a + mu
    d = -((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2])
    return True, np.array([n[0], n[1], n[2], d]), lam, sums


def refine_bound(sums, lam, centre_norm):
    """How far the device's refined (normal, d) may lie from fit()'s: the device sums k terms per entry in f64 (each sum within
    k u sum|terms|), so every covariance entry is within 3 (k + 4) u M2 (M2 = mean |q|^2 bounds the entries and |mu|^2), the
    matrix within 9 (k + 4) u M2 in norm; the two solvers (Jacobi, eigh) add 32 u M2 each.  An eigenvector moves by at most
    2 |dC| / gap (Davis-Kahan), gap = lambda_mid - lambda_min; d = -n . c moves by that times |c| plus the roundings of c and
    of the dot product."""
    k, M2 = sums["count"], sums["M2"]
    dC = (9.0 * (k + 4) + 64.0) * U * M2
    gap = lam[1] - lam[0]
    dn = 2.0 * dC / gap + 8 * U
    dd = dn * centre_norm + (k + 8) * U * (centre_norm + math.sqrt(M2))
    return dn, dd


def segment(xyz, sp, triples=None):
    """the whole call -> dict(found, refined, coeff, best, best_count, n_inliers, n_finite, n_degenerate, n_rejected, inliers
    (mask), others (mask), keys, plus what the bounds need)"""
    xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
    co, st, cn, triples, aux = counts(xyz, sp, triples)
    T = D(sp["T"])
    fin = np.isfinite(xyz).all(1) if len(xyz) else np.zeros(0, dtype=bool)
    r = dict(found=False, refined=False, coeff=np.zeros(4), best=-1, best_count=0, n_inliers=0, n_finite=int(fin.sum()),
             n_degenerate=int((st == DEGENERATE).sum()), n_rejected=int((st == REJECTED).sum()), counts=cn, states=st, coeffs=co)
    valid = np.flatnonzero(st == VALID)
    if len(valid) == 0:
        r["inliers"], r["others"] = np.zeros(len(xyz), dtype=bool), fin.copy()
        r["keys"] = np.where(fin, np.inf, np.nan)
        return r
    best = int(valid[np.argmax(cn[valid])])      # (argmax: the first of equals)
    r.update(found=True, best=best, best_count=int(cn[best]), coeff=co[best].copy())
    s = distances(co[best], xyz)
    mask = inlier(s, T) & fin
    if sp["refine"]:
        a = xyz[triples[best, 0]].astype(D)
        taken, coeff, lam, sums = fit(sp, xyz[mask].astype(D), a)
        r.update(unrefined=co[best].copy(), sums=sums, lam=lam, a=a)
        if taken:
            r.update(refined=True, coeff=coeff)
            s = distances(coeff, xyz)
            mask = inlier(s, T) & fin
    r["keys"] = np.where(fin, s, np.nan)
    r["inliers"], r["others"], r["n_inliers"] = mask, fin & ~mask, int(mask.sum())
    return r


def clearances(xyz, sp, triples=None):
    """what the exact comparisons rely on -> dict(distance: the smallest | |s| - T | over every finite point and every valid
    hypothesis, angle: the smallest |n . a^ - cos_eps| over the valid and rejected ones, degeneracy: the smallest factor
    between len2 and its bound (either way))"""
    xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
    co, st, cn, triples, aux = counts(xyz, sp, triples)
    T, axis, cos_eps = params(sp)
    out = dict(distance=np.inf, angle=np.inf, degeneracy=np.inf)
    fin = np.isfinite(xyz).all(1)
    for h in np.flatnonzero(st == VALID):
        s = distances(co[h], xyz[fin])
        if len(s):
            out["distance"] = min(out["distance"], float(np.abs(np.abs(s) - T).min()))
    if axis is not None and np.isfinite(aux["dot"]).any():
        out["angle"] = float(np.nanmin(np.abs(aux["dot"] - cos_eps)))
    with np.errstate(all="ignore"):
        ratio = aux["len2"] / (1e-8 * aux["uuvv"])
    ratio = ratio[np.isfinite(ratio) & (ratio > 0)]
    if len(ratio):
        out["degeneracy"] = float(np.minimum(ratio, 1.0 / ratio).max())   # 1 = on the bound; the tests want <= 1/2
    else:
        out["degeneracy"] = 0.0
    return out


# ---------------------------------------------------------------------------------------------------- fixtures
def ground(n, seed, offset=(0.0, 0.0, 0.0), noise=0.03, clutter=0.3, tilt=(0.02, -0.015), lift=0.4):
    """n points: a ground plane z = tilt . (x, y) - 1.7 with +-noise, and a fraction `clutter` of points at least `lift` above
    it, inside 40 m x 40 m, moved by offset and rounded to f32"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-20.0, 20.0, (n, 2))
    z = xy @ np.array(tilt) - 1.7 + rng.uniform(-noise, noise, n)
    up = rng.random(n) < clutter
    z = np.where(up, z + lift + rng.uniform(0.0, 6.0, n), z)
    return np.ascontiguousarray((np.column_stack([xy, z]) + np.array(offset)).astype(F))


AXIS_Z = dict(axis=(0.0, 0.0, 1.0), eps=math.radians(10.0))
FAR = (100000.0, -100000.0, 50.0)


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> (xyz, spec): the fixtures of the GPU tests; tests/test_plane_cases.py holds their clearances"""
    c = {}
    c["ground 1000"] = (ground(1000, 1), spec(0.1, 256, seed=7, **AXIS_Z))
    c["ground 4099"] = (ground(4099, 2), spec(0.1, 256, seed=11, **AXIS_Z))
    c["ground 4099, any plane"] = (ground(4099, 2), spec(0.1, 256, seed=11))
    c["ground 1000 at 100 km"] = (ground(1000, 3, FAR), spec(0.1, 256, seed=5, **AXIS_Z))
    c["ground 4099 at 100 km, any plane"] = (ground(4099, 4, FAR), spec(0.1, 256, seed=9))
    x = ground(1500, 5)
    x[::97] = np.nan
    x[5::131, 1] = np.inf
    x[7::151, 2] = -np.inf
    c["non-finite rows"] = (x, spec(0.1, 300, seed=3, **AXIS_Z))
    return c


@functools.lru_cache(maxsize=None)
def refine_cases():
    """noise <= T / 2 and clutter >= 2 T from the plane"""
    c = {}
    c["refine 4099"] = (ground(4099, 21, noise=0.05, lift=0.25), spec(0.1, 256, seed=2, refine=True, **AXIS_Z))
    c["refine 1000, any plane"] = (ground(1000, 22, noise=0.05, lift=0.25), spec(0.1, 256, seed=4, refine=True))
    c["refine 5000 at 100 km"] = (ground(5000, 23, FAR, noise=0.05, lift=0.25), spec(0.1, 256, seed=6, refine=True, **AXIS_Z))
    return c


def shape_cloud(n, seed=0):
    """the cloud of the plan-boundary shapes: the first n points of one ground cloud"""
    return _shape_base()[:n] if n <= len(_shape_base()) else ground(n, 40 + seed)


SHAPE_N = (3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)    # a tile is 1024 points
SHAPE_H = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)                             # a hypothesis block is 256 hypotheses


def shape_cases():
    """[(n, spec)]: every point count about the tile steps under 257 hypotheses, every hypothesis count about the block steps
    over two tiles + 1 and over 65 points (with and without an axis in turn)"""
    out = [(n, spec(0.1, 257, seed=n, **(AXIS_Z if k % 2 == 0 else {}))) for k, n in enumerate(SHAPE_N)]
    out += [(1025 if k % 2 else 2049, spec(0.1, H, seed=100 + H, **(AXIS_Z if k % 3 else {}))) for k, H in enumerate(SHAPE_H)]
    out += [(65, spec(0.1, H, seed=200 + H, **AXIS_Z)) for H in SHAPE_H]
    return out


@functools.lru_cache(maxsize=None)
def _shape_base():
    return ground(2 * 1024 + 1, 40)


@functools.lru_cache(maxsize=None)
def reference_of(name):
    cases = dict(gpu_cases())
    cases.update(refine_cases())
    xyz, sp = cases[name]
    return segment(xyz, sp)
