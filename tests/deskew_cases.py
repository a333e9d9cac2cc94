"""Shared by the deskew tests (no GPU, no library): the numpy restatement of the motion compensation defined in
include/ndt_mi355.h ("deskew"), in f64 and unrounded, the error bound the tests hold the library to, and cloud builders.

A sweep covers [t_begin, t_end]; over it the sensor moves by the rotation vector w = angle * axis and the translation tau (in
the sensor frame at t_begin).  Its pose at time t relative to t_begin is (Exp(u w), u tau), u = (t - t_begin) / (t_end - t_begin).
The output is the scan seen from the sensor frame at t_ref:
    s = (t_i - t_ref) / (t_end - t_begin),  theta = s * angle,
    q = p cos(theta) + (k x p) sin(theta) + k (k . p)(1 - cos(theta)) + s tau_ref,   tau_ref = Exp(-u_ref w) tau."""
from types import SimpleNamespace

import numpy as np

F32 = np.float32
QNAN_BITS = 0x7fc00000     # what an untimed record's coordinates become


def exp_rot(axis, angle):
    """Rodrigues: the rotation matrix Exp(angle * axis), f64"""
    k = np.asarray(axis, dtype=np.float64)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def make_motion(w, tau, t_begin=0.0, t_end=1.0, t_ref=None):
    """the motion of a sweep from its rotation vector w and translation tau (frame at t_begin); t_ref None = t_begin"""
    w, tau = np.asarray(w, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    t_ref = t_begin if t_ref is None else t_ref
    angle = float(np.linalg.norm(w))
    axis = w / angle if angle > 0 else np.array([1.0, 0.0, 0.0])
    axis = axis / np.linalg.norm(axis)
    u_ref = (t_ref - t_begin) / (t_end - t_begin)
    return SimpleNamespace(t_begin=float(t_begin), t_end=float(t_end), t_ref=float(t_ref), axis=axis, angle=angle,
                           tau_ref=exp_rot(axis, -u_ref * angle) @ tau)


def fields(m):
    """(t_begin, t_end, t_ref, axis (3,), angle, tau_ref (3,)) of a make_motion namespace or a ctypes ndt_deskew_motion"""
    return (float(m.t_begin), float(m.t_end), float(m.t_ref), np.array(list(m.axis), dtype=np.float64), float(m.angle),
            np.array(list(m.tau_ref), dtype=np.float64))


def to_ctypes(m, cls):
    """the motion as the ctypes structure cls (toyslam_amd._lib.DeskewMotion)"""
    t_begin, t_end, t_ref, axis, angle, tau_ref = fields(m)
    c = cls()
    c.t_begin, c.t_end, c.t_ref, c.angle = t_begin, t_end, t_ref, angle
    c.axis[:], c.tau_ref[:] = axis.tolist(), tau_ref.tolist()
    return c


def s_of(times, motion):
    t_begin, t_end, t_ref, _, _, _ = fields(motion)
    return (np.asarray(times, dtype=np.float64) - t_ref) / (t_end - t_begin)


def kinds(records, times):
    """(n,) int: 0 a finite record with a finite time (moved), 1 a non-finite coordinate (copied), 2 finite but untimed (NaN)"""
    xyz = np.asarray(records)[:, :3]
    bad = ~np.isfinite(xyz).all(1)
    return np.where(bad, 1, np.where(np.isfinite(np.asarray(times, dtype=np.float64)), 0, 2))


def reference_deskew(records, times, motion):
    """(n, >= 3) records (f32 as stored; f64 is taken as it is), (n,) times -> (n, 3) f64, unrounded: the definition.  Rows with
    a non-finite coordinate come back as they are, finite rows without a finite time as NaN."""
    p = np.asarray(records)[:, :3].astype(np.float64)
    _, _, _, k, angle, tau_ref = fields(motion)
    kind = kinds(p, times)
    with np.errstate(invalid="ignore", over="ignore"):
        s = s_of(times, motion)
        theta = s * angle
        c, sn = np.cos(theta)[:, None], np.sin(theta)[:, None]
        q = p * c + np.cross(k[None, :], p) * sn + k[None, :] * (p @ k)[:, None] * (1 - c) + s[:, None] * tau_ref[None, :]
    q[kind == 1] = p[kind == 1]
    q[kind == 2] = np.nan
    return q


def bound(q_got, records, times, motion):
    """per coordinate: 1/2 ulp32(q_got) -- the one final rounding -- + 64 * 2^-53 * (|p|_1 + |s| |tau_ref|_1): at most 12
    rounded f64 operations per path and sin / cos at 2 ulp, on both sides, doubled"""
    p = np.asarray(records)[:, :3].astype(np.float64)
    tau_ref = fields(motion)[5]
    with np.errstate(invalid="ignore", over="ignore"):
        half_ulp = 0.5 * np.spacing(np.abs(np.asarray(q_got, dtype=F32))).astype(np.float64)
        mag = np.abs(p).sum(1) + np.abs(s_of(times, motion)) * np.abs(tau_ref).sum()
    return half_ulp + 64 * 2.0 ** -53 * mag[:, None]


def check_moved(q_got, records, times, motion, what=None):
    """every finite, timed row of q_got (n, 3) f32 within the bound of the restatement"""
    kind = kinds(records, times)
    ref = reference_deskew(records, times, motion)
    ok = kind == 0
    err = np.abs(np.asarray(q_got, dtype=F32).astype(np.float64)[ok] - ref[ok])
    lim = bound(q_got, records, times, motion)[ok]
    bad = np.argwhere(~(err <= lim))
    assert len(bad) == 0, (what, "row %d axis %d: error %.3g over the bound %.3g" % (
        np.flatnonzero(ok)[bad[0][0]], bad[0][1], err[tuple(bad[0])], lim[tuple(bad[0])]))
    return float((err / lim).max()) if ok.any() else 0.0


def expected_records(rec_u32, times, motion, got_u32):
    """What must hold bit for bit of the output records got_u32 (n, 4) uint32 of the input rec_u32: fourth words, copied rows,
    the NaN-ing; -> number of untimed rows"""
    kind = kinds(rec_u32.view(F32), times)
    assert got_u32.shape == rec_u32.shape
    assert np.array_equal(got_u32[:, 3], rec_u32[:, 3]), "fourth words"
    assert np.array_equal(got_u32[kind == 1], rec_u32[kind == 1]), "records with a non-finite coordinate"
    assert (got_u32[kind == 2][:, :3] == QNAN_BITS).all(), "untimed records"
    at_ref = (kind == 0) & (s_of(times, motion) == 0)
    assert (got_u32.view(F32)[at_ref][:, :3] == rec_u32.view(F32)[at_ref][:, :3]).all(), "s == 0 rows"
    return int((kind == 2).sum())


# ---- clouds -------------------------------------------------------------------------------------------------------------
def azimuth_times(xyz, t_begin, t_end):
    """times by azimuth, as a spinning lidar stamps its points: t_begin at -pi, t_end at +pi"""
    az = np.arctan2(xyz[:, 1].astype(np.float64), xyz[:, 0].astype(np.float64))
    return t_begin + (az + np.pi) / (2 * np.pi) * (t_end - t_begin)


def build_records(n, seed=0, offset=(0.0, 0.0, 0.0), odd_every=0):
    """(n, 4) float32 records around `offset` with garbage fourth words; with odd_every > 0 every odd_every-th row has a NaN or
    an infinite coordinate (and odd bits elsewhere)"""
    rng = np.random.default_rng(1000 + seed + 7 * n)
    rec = np.empty((n, 4), F32)
    rec[:, :3] = (rng.uniform(-60, 60, (n, 3)) * [1, 1, 0.1] + np.asarray(offset)).astype(F32)
    rec[:, 3] = rng.uniform(-1e30, 1e30, n).astype(F32)
    if n:
        rec[rng.integers(0, n, max(1, n // 9)), 3] = np.nan
    if odd_every:
        rows = np.arange(odd_every // 2, n, odd_every)
        for j, r in enumerate(rows):
            rec[r, j % 3] = (np.nan, np.inf, -np.inf)[(j // 3) % 3]
    return rec


def build_times(n, motion, seed=0, untimed_every=0, outside=True, at_ref_every=0):
    """(n,) float64 times over the sweep of `motion`; with `outside` a tenth before t_begin and a tenth after t_end; every
    untimed_every-th is NaN or infinite; every at_ref_every-th is t_ref itself (s == 0)"""
    rng = np.random.default_rng(2000 + seed + 3 * n)
    t_begin, t_end, t_ref = fields(motion)[:3]
    lo, hi = (-0.3, 1.3) if outside else (0.0, 1.0)
    t = t_begin + rng.uniform(lo, hi, n) * (t_end - t_begin)
    if at_ref_every:
        t[at_ref_every // 3::at_ref_every] = t_ref
    if untimed_every:
        rows = np.arange(untimed_every // 2, n, untimed_every)
        t[rows] = np.array([np.nan, np.inf, -np.inf])[np.arange(len(rows)) % 3]
    return t


def skew_scan(world, times, w, tau, t_begin, t_end):
    """static world points (n, 3), each measured at its own time from the moving sensor: p_i = T(u_i)^-1 W_i, f64"""
    world = np.asarray(world, dtype=np.float64)
    angle = float(np.linalg.norm(w))
    axis = np.asarray(w, dtype=np.float64) / angle if angle > 0 else np.array([1.0, 0, 0])
    u = (np.asarray(times, dtype=np.float64) - t_begin) / (t_end - t_begin)
    v = world - u[:, None] * np.asarray(tau, dtype=np.float64)[None, :]
    c, sn = np.cos(-u * angle)[:, None], np.sin(-u * angle)[:, None]
    return v * c + np.cross(axis[None, :], v) * sn + axis[None, :] * (v @ axis)[:, None] * (1 - c)
