"""Shared by the bounding-box tests (no GPU): the numpy reference of a cloud's two boxes, written from the definition, and a
builder of clouds in which every box value is owned by exactly one row.

Box [0] is over the coordinates that are not NaN (what getMinMax3D sees for an is_dense cloud: fmin / fmax drop a NaN
operand, an infinity stays); box [1] is over the rows whose three coordinates are finite (the !is_dense rule).  An empty
box is (FLT_MAX, -FLT_MAX).  min and max do not round, so boxes are compared with == on the f32 values: no tolerance, and
-0.0 agrees with +0.0.

A box layout everywhere in these files: (2, 2, 3) float32, [box][min | max][xyz]."""
import os

import numpy as np

FLT_MAX = np.finfo(np.float32).max
F32 = np.float32

# the cuts of the producers as they stand in the code (toyslam_amd/csrc; NOTES.md "Who writes a cloud's boxes")
HOST_STAGE_MAX = min(65536, max(0, int(os.environ.get("NDT_HOST_STAGE_MAX", "20480"))))  # upload_cloud: host route up to here
BLOCK = 256                       # kBlock
REPACK_MAX_BLOCKS = 1024          # k_repack_bbox: min(1024, ceil(n / 256)) blocks
REC16_MAX_BLOCKS = 256            # k_bbox16 (uploads): min(256, ceil(n / 256)) blocks, eight loads per thread and trip
REC16_LOADS = 8
OUT_BOX_BLOCKS = 64               # kOutBoxBlocks: k_bbox16 over a filter's output; the grid of k_repack_bbox_multi
TRANSFORM_MAX_BLOCKS = 2048       # k_transform / k_transform_multi: grid_for(n, 2048)
FILTER_BUCKETS_FROM = 131072      # filter_takes_buckets: n >= this and n_cells <= 4 n


def reference_boxes(xyz):
    """(n, >= 3) float32 -> (2, 2, 3) float32 boxes, from the definition"""
    xyz = np.asarray(xyz, dtype=F32)
    assert xyz.ndim == 2 and xyz.shape[1] >= 3
    xyz = xyz[:, :3]
    out = np.empty((2, 2, 3), F32)
    for v, rows in ((0, xyz), (1, xyz[np.isfinite(xyz).all(1)])):
        out[v, 0] = np.fmin.reduce(rows, axis=0, initial=F32(FLT_MAX))
        out[v, 1] = np.fmax.reduce(rows, axis=0, initial=F32(-FLT_MAX))
    return out


EMPTY_BOXES = reference_boxes(np.zeros((0, 3), F32))


def same_boxes(got, ref):
    """== on the f32 values (exact: min / max do not round; -0.0 == +0.0); boxes never hold a NaN"""
    got, ref = np.asarray(got), np.asarray(ref)
    return got.dtype == F32 and got.shape == (2, 2, 3) and not np.isnan(got).any() and bool((got == ref).all())


def boxes_text(got, ref):
    bad = np.argwhere(~(np.asarray(got) == np.asarray(ref)))
    return "; ".join("box[%d].%s.%s got %r want %r" % (v, "min max".split()[m], "xyz"[k], got[v, m, k], ref[v, m, k]) for v, m, k in bad)


# the 12 values in the order hot rows are handed out: both boxes, both ends and all axes come early, so that a cloud of
# three or four rows still has owners in either box
SLOTS = [(1, 1, 0), (0, 0, 1), (1, 0, 2), (0, 1, 2), (1, 0, 0), (0, 1, 1), (0, 0, 0), (1, 1, 2), (1, 1, 1), (0, 0, 2), (1, 0, 1), (0, 1, 0)]
VARIANTS = ("plain", "denormal", "fltmax", "inf", "far")


def build_cloud(n, hot, floats=3, variant="plain", seed=0, nan_rows=()):
    """(n, floats) float32 records.  Row hot[j] is the only owner of value SLOTS[j] of the reference boxes (len(hot) <= 12,
    distinct rows); every other row lies strictly inside both boxes; rows `nan_rows` are all NaN.  Floats behind z are
    garbage (huge, NaN, inf).  -> (records, {slot: row})

    An owner of box [1] is a finite row.  An owner of box [0] carries a NaN in another coordinate, so it gives its value to
    box [0] and nothing to box [1] -- and it lies beyond the owner of the same value of box [1], which box [0] sees too.

    variant: "denormal": every z is negative but the two max-z owners, which are denormal (1e-40, 3e-40);
    "fltmax": the x owners of box [0] are -FLT_MAX / +FLT_MAX;  "inf": box [0]'s max y is +inf and its min z -inf;
    "far": the cloud sits 100 km from the origin on every axis."""
    assert variant in VARIANTS and len(hot) <= 12 and len(set(hot)) == len(hot) and all(0 <= r < n for r in hot)
    rng = np.random.default_rng(seed + 7 * n)
    off = np.array([1e5, -1e5, 1e5], F32) if variant == "far" else np.zeros(3, F32)
    rec = rng.uniform(-1e30, 1e30, (n, floats)).astype(F32)
    if floats > 3 and n:
        rec[rng.integers(0, n, max(1, n // 5)), 3] = np.nan
        rec[rng.integers(0, n, max(1, n // 7)), floats - 1] = np.inf
    inner = rng.uniform(-10, 10, (n, 3)).astype(F32)
    if variant == "denormal":
        inner[:, 2] = rng.uniform(-10, -1, n).astype(F32)
    rec[:, :3] = inner + off
    owners = {}
    for j, row in enumerate(hot):
        v, m, k = SLOTS[j]
        sign = F32(1 if m else -1)
        val = off[k] + sign * F32(20 if v else 40)
        if variant == "denormal" and k == 2 and m == 1:
            val = F32(1e-40) if v else F32(3e-40)
        if variant == "fltmax" and v == 0 and k == 0:
            val = sign * F32(FLT_MAX)
        if variant == "inf" and v == 0 and (m, k) in ((1, 1), (0, 2)):
            val = sign * F32(np.inf)
        rec[row, k] = val
        if v == 0:
            rec[row, (k + 1) % 3] = np.nan
        owners[SLOTS[j]] = row
    for r in nan_rows:
        assert r not in hot
        rec[r, :3] = np.nan
    check_owners(rec, owners)
    return rec, owners


def check_owners(rec, owners):
    """from the reference alone: the owners are distinct rows, each holds its value, and without it the value changes"""
    ref = reference_boxes(rec)
    assert len(set(owners.values())) == len(owners)
    for (v, m, k), row in owners.items():
        assert rec[row, k] == ref[v, m, k], ((v, m, k), row)
        less = reference_boxes(np.delete(rec, row, axis=0))
        assert less[v, m, k] != ref[v, m, k], ((v, m, k), row)
        others = np.ones((2, 2, 3), bool)
        others[v, m, k] = False
        if len(owners) == 12:  # ... and it owns nothing else (a cloud too small for 12 owners: a row may hold several values)
            assert (less[others] == ref[others]).all(), ((v, m, k), row)
    return ref


def spread_hot(n, must=()):
    """up to 12 distinct rows of a cloud of n: `must` first (the indices a case is about, those outside [0, n) dropped), then
    the first and the last row, then rows spread over the cloud"""
    rows = []
    for r in list(must) + [0, n - 1] + [(n * j) // 11 for j in range(1, 11)] + list(range(n)):
        if 0 <= r < n and r not in rows:
            rows.append(r)
        if len(rows) == 12:
            break
    return rows


def host_route():
    """the route of a host upload of at most HOST_STAGE_MAX points on this machine"""
    from toyslam_amd import _lib, ndt
    off = os.environ.get("NDT_HOST_AVX2")
    if off is not None and int(off) == 0:
        return "host_scalar"
    try:
        ndt.host_repack_bbox(np.zeros(3, F32), 1, 12, avx2=True)
    except _lib.NdtError:
        return "host_scalar"
    return "host_avx2"


def upload_route(n, stride, on_device=False, aligned=True, by_reference=False):
    """the producer upload_cloud takes (ndt_clouds.hip), as a route name"""
    if n == 0:
        return "none"
    if not on_device and n <= HOST_STAGE_MAX:
        return host_route()
    if stride != 16 or not aligned:
        return "repack"
    return "rec16_polled" if by_reference else "rec16_copy"


# ---- moved points: the f64 transform and its f32 allowance ------------------------------------------------------------
GAMMA4 = 4 * 2.0 ** -24 / (1 - 4 * 2.0 ** -24)  # three f32 multiply-adds and one add: (1 + u)^4 - 1 <= gamma_4, u = 2^-24


def moved_f64(xyz, T):
    """-> (moved (n, 3) f64, allowance (n, 3) f64 = gamma_4 (|R| |p| + |t|)) for finite rows of xyz under the 4x4 T as the
    kernel holds it (f32 entries)"""
    T = np.asarray(T, dtype=F32).astype(np.float64)
    p = np.asarray(xyz, dtype=F32)[:, :3].astype(np.float64)
    return p @ T[:3, :3].T + T[:3, 3], GAMMA4 * (np.abs(p) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3]))
