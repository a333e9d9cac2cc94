"""The selection predicate of ndt_cloud_select (include/ndt_mi355.h, "selection"), restated in numpy from its definition,
with f32 arithmetic done step by step in np.float32; the cloud builders and sizes the selection tests share.  No library
code is used here: tests/test_select_cases.py pins this module to hand cases, the other tests compare the library with it."""
import numpy as np

F32 = np.float32
FINITE, BOX, BOX_NEGATE, RANGE, RANGE_NEGATE, KEY, KEY_NEGATE = 1, 2, 4, 8, 16, 32, 64
KNOWN = 127
INF = float("inf")
NAN = float("nan")


def spec(flags=0, box_min=(0, 0, 0), box_max=(0, 0, 0), centre=(0, 0, 0), r_min=0.0, r_max=0.0, key_lo=0.0, key_hi=0.0):
    return dict(flags=int(flags), box_min=np.asarray(box_min, F32), box_max=np.asarray(box_max, F32), centre=np.asarray(centre, F32),
                r_min=F32(r_min), r_max=F32(r_max), key_lo=float(key_lo), key_hi=float(key_hi))


def spec_is_valid(s):
    f = s["flags"]
    if f & ~KNOWN:
        return False
    if (f & BOX_NEGATE and not f & BOX) or (f & RANGE_NEGATE and not f & RANGE) or (f & KEY_NEGATE and not f & KEY):
        return False
    if f & BOX and not bool((s["box_min"] <= s["box_max"]).all()):   # (a NaN bound compares false)
        return False
    if f & RANGE and (np.isnan(s["centre"]).any() or not s["r_min"] >= 0 or not s["r_min"] <= s["r_max"]):
        return False
    if f & KEY and not s["key_lo"] <= s["key_hi"]:
        return False
    return True


def dist2(xyz, centre):
    """(dx*dx + dy*dy) + dz*dz, every operation an f32 operation of its own"""
    with np.errstate(all="ignore"):
        d = xyz[:, :3].astype(F32) - np.asarray(centre, F32)[None, :]
        sq = d * d
        return (sq[:, 0] + sq[:, 1]) + sq[:, 2]


def keep_mask(s, xyz, keys=None):
    """(n,) bool: which rows of the (n, >= 3) float32 cloud are kept under spec `s` (keys: (n,) float64 where KEY is set)"""
    xyz = np.asarray(xyz, F32)
    xyz = xyz[None, :] if xyz.ndim == 1 else xyz
    n, f = xyz.shape[0], s["flags"]
    keep = np.ones(n, bool)
    with np.errstate(all="ignore"):
        if f & FINITE:
            keep &= np.isfinite(xyz[:, :3]).all(1)
        if f & BOX:
            inside = ((s["box_min"][None, :] <= xyz[:, :3]) & (xyz[:, :3] <= s["box_max"][None, :])).all(1)
            keep &= ~inside if f & BOX_NEGATE else inside
        if f & RANGE:
            d2 = dist2(xyz, s["centre"])
            inside = (F32(s["r_min"]) * F32(s["r_min"]) <= d2) & (d2 <= F32(s["r_max"]) * F32(s["r_max"]))
            keep &= ~inside if f & RANGE_NEGATE else inside
        if f & KEY:
            k = np.asarray(keys, np.float64).reshape(n)
            inside = (s["key_lo"] <= k) & (k <= s["key_hi"])
            keep &= (~inside if f & KEY_NEGATE else inside) & ~np.isnan(k)
    return keep


def to_ctypes(s, SelectSpec):
    c = SelectSpec()
    c.flags = s["flags"]
    c.box_min[:], c.box_max[:], c.centre[:] = s["box_min"].tolist(), s["box_max"].tolist(), s["centre"].tolist()
    c.r_min, c.r_max, c.key_lo, c.key_hi = float(s["r_min"]), float(s["r_max"]), s["key_lo"], s["key_hi"]
    return c


def up(v):
    return np.nextafter(F32(v), F32(INF))


def down(v):
    return np.nextafter(F32(v), F32(-INF))


# rows no test may mishandle: NaN in each coordinate, all NaN, +-inf, a finite point inside and one outside the unit tests
ODD_ROWS = np.array([[NAN, 1, 1], [1, NAN, 1], [1, 1, NAN], [NAN, NAN, NAN], [INF, 1, 1], [1, -INF, 1], [1, 1, INF], [-INF, INF, -INF],
                     [1, 1, 1], [50, 50, 50], [0, 0, 0], [-0.0, 0.0, -0.0]], F32)
ODD_KEYS = np.array([NAN, -1.0, INF, -INF, 0.0, -0.0, 0.25, 0.5, 0.75, 1.0, 1e300, -1e300])
BOX_UNIT = ((-2, -3, -4), (2, 3, 4))


def box_face_rows(box=BOX_UNIT):
    """(rows, inside): a point on each of the six faces (inside) and the f32 neighbour one ulp beyond it (outside)"""
    mn, mx = np.asarray(box[0], F32), np.asarray(box[1], F32)
    mid = (mn + mx) / F32(2)
    rows, inside = [], []
    for a in range(3):
        for bound, beyond in ((mn[a], down(mn[a])), (mx[a], up(mx[a]))):
            for v, ins in ((bound, True), (beyond, False)):
                p = mid.copy()
                p[a] = v
                rows.append(p)
                inside.append(ins)
    return np.array(rows, F32), np.array(inside)


# a = 1 + 2^-12, b = 2^-12: a*a rounds to 1 + 2^-11 (= r^2 for r = a), and adding b*b = 2^-24 rounds back to it -- inside
# r_max = a.  A fused multiply-add keeps a*a exact, and the sum becomes 1 + 2^-11 + 2^-23: outside.  Every placement of
# (a, b) over the axes, so that whichever product a compiler fuses is caught.
A_FUSED, B_FUSED = F32(1) + F32(2.0 ** -12), F32(2.0 ** -12)
FUSED_ROWS = np.array([[A_FUSED, B_FUSED, 0], [B_FUSED, A_FUSED, 0], [A_FUSED, 0, B_FUSED], [B_FUSED, 0, A_FUSED], [0, A_FUSED, B_FUSED],
                       [0, B_FUSED, A_FUSED], [A_FUSED, B_FUSED, B_FUSED]], F32)


def edge_cloud():
    """the rows of the hand cases in one cloud (with keys), for the device tests"""
    faces, _ = box_face_rows()
    radius = np.array([[3, 4, 0], [up(3), 4, 0], [0, 0, 5], [0, 0, up(5)], [0, 1, 0], [0, down(1), 0]], F32)
    xyz = np.concatenate([ODD_ROWS, faces, radius, FUSED_ROWS]).astype(F32)
    keys = np.resize(ODD_KEYS, xyz.shape[0]).astype(np.float64)
    return xyz, keys


def edge_specs():
    """every combination of FINITE and the NEGATE bits over BOX / RANGE / KEY on the edge cloud, and flags == 0"""
    out = [spec(0)]
    for fin in (0, FINITE):
        for neg in (0, 1):
            out.append(spec(fin | BOX | (BOX_NEGATE * neg), box_min=BOX_UNIT[0], box_max=BOX_UNIT[1]))
            out.append(spec(fin | RANGE | (RANGE_NEGATE * neg), r_min=1.0, r_max=5.0))
            out.append(spec(fin | RANGE | (RANGE_NEGATE * neg), r_min=0.0, r_max=INF))
            out.append(spec(fin | RANGE | (RANGE_NEGATE * neg), r_min=0.0, r_max=A_FUSED))
            out.append(spec(fin | KEY | (KEY_NEGATE * neg), key_lo=0.25, key_hi=0.75))
            out.append(spec(fin | KEY | (KEY_NEGATE * neg), key_lo=0.5, key_hi=0.5))
            out.append(spec(fin | KEY | (KEY_NEGATE * neg), key_lo=-INF, key_hi=INF))
    out.append(spec(FINITE))
    out.append(spec(BOX | RANGE | KEY, box_min=(-2, -3, -4), box_max=(60, 60, 60), r_min=1.0, r_max=100.0, key_lo=0.0, key_hi=1.0))
    out.append(spec(FINITE | BOX | BOX_NEGATE | RANGE | KEY | KEY_NEGATE, box_min=(-1, -1, -1), box_max=(1.5, 1.5, 1.5), r_min=0.5, r_max=INF,
                    key_lo=0.5, key_hi=1.0))
    return out


def random_spec(rng):
    f = int(rng.integers(0, 128))
    if not f & BOX:
        f &= ~BOX_NEGATE
    if not f & RANGE:
        f &= ~RANGE_NEGATE
    if not f & KEY:
        f &= ~KEY_NEGATE
    a, b = rng.uniform(-8, 8, 3).astype(F32), rng.uniform(-8, 8, 3).astype(F32)
    r = np.sort(rng.uniform(0, 12, 2)).astype(F32)
    k = np.sort(rng.uniform(-1, 1, 2))
    return spec(f, box_min=np.minimum(a, b), box_max=np.maximum(a, b), centre=rng.uniform(-2, 2, 3), r_min=r[0],
                r_max=INF if rng.random() < 0.2 else r[1], key_lo=k[0], key_hi=k[1])


def random_cloud(n, seed, odd_every=0):
    """(n, 3) float32 in a 20 m cube and (n,) float64 keys in [-1, 1]; odd_every > 0: every odd_every-th row is one of ODD_ROWS"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-10, 10, (n, 3)).astype(F32)
    keys = rng.uniform(-1, 1, n)
    if odd_every and n:
        at = np.arange(odd_every // 2, n, odd_every)
        xyz[at] = ODD_ROWS[np.arange(at.shape[0]) % ODD_ROWS.shape[0]]
        keys[at] = ODD_KEYS[np.arange(at.shape[0]) % ODD_KEYS.shape[0]]
    return xyz, keys


def invalid_specs():
    """one spec per rule of the definition's "a spec is invalid if" """
    box = dict(box_min=(0, 0, 0), box_max=(1, 1, 1))
    out = [spec(128), spec(1 << 31), spec(BOX_NEGATE), spec(RANGE_NEGATE), spec(KEY_NEGATE), spec(FINITE | BOX_NEGATE),
           spec(BOX | RANGE_NEGATE, **box)]
    for a in range(3):
        for which in ("box_min", "box_max"):
            s = spec(BOX, **box)
            s[which][a] = NAN
            out.append(s)
        s = spec(BOX, **box)
        s["box_min"][a] = F32(2)
        out.append(s)
        s = spec(RANGE, r_min=0, r_max=1)
        s["centre"][a] = NAN
        out.append(s)
    out += [spec(RANGE, r_min=NAN, r_max=1), spec(RANGE, r_min=0, r_max=NAN), spec(RANGE, r_min=-1, r_max=1), spec(RANGE, r_min=2, r_max=1),
            spec(KEY, key_lo=NAN, key_hi=1), spec(KEY, key_lo=0, key_hi=NAN), spec(KEY, key_lo=1, key_hi=0)]
    return out
