"""CPU: the deskew entries (ndt_cloud_deskew, ndt_cloud_deskew_clouds, ndt_diag_deskew, ndt_host_deskew_motion / _point / _plan,
ndt_host_extract_field, ndt_pcd_read_field) -- declared, exported and wrapped; the host definition against the numpy
restatement (tests/deskew_cases.py) within the derived bound; the logarithm of ndt_host_deskew_motion; the launch plan; every
refusal done before any device work, with its outputs untouched; the two entries that fetch the times; the PCD field reader
under sanitizers (tests/pcd_field_fuzz.cpp, a stand-alone program)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import deskew_cases as dc
from conftest import ROOT

NEW = ("ndt_cloud_deskew", "ndt_cloud_deskew_clouds", "ndt_diag_deskew", "ndt_host_deskew_motion", "ndt_host_deskew_point",
       "ndt_host_deskew_plan", "ndt_host_extract_field", "ndt_pcd_read_field")
SENTINEL = 0x5A5A5A5A
F = np.float32


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def to_ctypes(m, _lib):
    return dc.to_ctypes(m, _lib.DeskewMotion)


def test_entries_are_declared_exported_and_wrapped(mods):
    L, _lib, ndt = mods
    with open(os.path.join(ROOT, "include", "ndt_mi355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\(" % name, header), name + " is not declared in include/ndt_mi355.h"
    for method in ("deskewCloud", "deskewClouds", "deskewDiag"):
        assert callable(getattr(ndt.NormalDistributionsTransform, method))
    for fn in ("host_deskew_motion", "host_deskew_point", "host_deskew_plan", "extract_field", "pcd_read_field"):
        assert callable(getattr(ndt, fn))
    assert re.search(r"NDT_BOX_ROUTE_DESKEW = 10\b", header) and _lib.BOX_ROUTES[10] == "deskew"
    assert C.sizeof(_lib.DeskewMotion) == 80 and _lib.DeskewMotion.tau_ref.offset == 56


def motions():
    out = [dc.make_motion([0, 0, np.pi / 2], [0.8, -0.4, 0.2], 10.0, 12.0),
           dc.make_motion([0, 0, 0], [2, 4, -6], 0.0, 0.1),
           dc.make_motion([0.3, -0.2, 0.9], [1, 2, 3], 3.0, 4.0, 3.5),
           dc.make_motion([1e-9, 0, 0], [1, 0, 0], 1.7e9, 1.7e9 + 0.1),
           dc.make_motion(np.array([1, 2, -2]) / 3 * (np.pi - 1e-3), [0.5, 0.5, 0.5], 1.7e9, 1.7e9 + 0.1, 1.7e9 + 0.1),
           dc.make_motion([0, 0, np.pi], [0, 0, 0], -1.0, 1.0, 0.25)]
    return out


def test_host_point_is_the_restatement_within_the_bound(mods):
    L, _lib, ndt = mods
    worst, n_checked = 0.0, 0
    for j, m in enumerate(motions()):
        cm = to_ctypes(m, _lib)
        for offset in ((0, 0, 0), (1e5, -1e5, 1e5)):
            rec = dc.build_records(300, seed=j, offset=offset, odd_every=17)
            t = dc.build_times(300, m, seed=j, untimed_every=23, at_ref_every=29)
            got = np.empty((300, 3), F)
            untimed = np.zeros(300, bool)
            for i in range(300):
                got[i], untimed[i] = ndt.host_deskew_point(cm, rec[i, :3], t[i])
            kind = dc.kinds(rec, t)
            assert np.array_equal(untimed, kind == 2)
            out = rec.copy()
            out[:, :3] = got
            assert dc.expected_records(rec.view(np.uint32), t, m, out.view(np.uint32)) == int((kind == 2).sum()) > 0
            worst = max(worst, dc.check_moved(got, rec, t, m, (j, offset)))
            n_checked += int((kind == 0).sum())
    assert n_checked > 2500
    print("host point: worst error / bound = %.3f" % worst)


def test_host_point_refusals(mods):
    L, _lib, ndt = mods
    ok = to_ctypes(motions()[0], _lib)
    p = np.zeros(3, F).ctypes.data_as(C.POINTER(C.c_float))
    q = np.full(3, -7, F)
    qp = q.ctypes.data_as(C.POINTER(C.c_float))
    u = C.c_int(-7)
    assert L.ndt_host_deskew_point(None, p, 0.0, qp, C.byref(u)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_deskew_point(C.byref(ok), None, 0.0, qp, C.byref(u)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_deskew_point(C.byref(ok), p, 0.0, None, C.byref(u)) == _lib.NDT_ERR_INVALID
    for bad in invalid_motions(_lib):
        assert L.ndt_host_deskew_point(C.byref(bad), p, 0.0, qp, C.byref(u)) == _lib.NDT_ERR_INVALID
    assert (q == -7).all() and u.value == -7
    assert L.ndt_host_deskew_point(C.byref(ok), p, 0.0, qp, None) == _lib.NDT_OK


def invalid_motions(_lib):
    out = []

    def vary(**kw):
        m = to_ctypes(dc.make_motion([0, 0, 1], [1, 2, 3], 0.0, 1.0), _lib)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(m, k)[:] = list(v)
            else:
                setattr(m, k, v)
        out.append(m)
    for name in ("t_begin", "t_end", "t_ref", "angle"):
        vary(**{name: float("nan")})
        vary(**{name: float("inf")})
    vary(axis=(float("nan"), 0.0, 1.0))
    vary(tau_ref=(0.0, float("inf"), 0.0))
    vary(t_end=0.0)
    vary(t_end=-1.0)
    vary(angle=-1e-9)
    vary(angle=float(np.nextafter(np.pi, 4.0)) + 1e-15)
    vary(angle=4.0)
    vary(axis=(0.0, 0.0, 1.0 + 1e-11))
    vary(axis=(0.0, 0.0, 0.0))
    vary(axis=(0.6, 0.0, 0.8 - 1e-11))
    return out


def rot_of(m):
    return dc.exp_rot(np.array(list(m.axis)), m.angle)


@pytest.mark.parametrize("angle", (0.0, 1e-9, 1e-4, 1.0, np.pi - 1e-3))
def test_host_motion_takes_the_logarithm(mods, angle):
    L, _lib, ndt = mods
    rng = np.random.default_rng(5)
    axes = [np.array([1.0, 0, 0]), np.array([0, 0, -1.0]), np.array([1, 2, -2]) / 3.0, np.array([-0.6, 0.8, 0.0]), np.array([1e-3, 1, 1e-3])]
    axes += [rng.standard_normal(3) for _ in range(8)]
    for axis in axes:
        axis = axis / np.linalg.norm(axis)
        T = np.eye(4)
        T[:3, :3] = dc.exp_rot(axis, angle)
        T[:3, 3] = rng.uniform(-3, 3, 3)
        T32 = T.astype(F)
        for t_ref in (20.0, 20.05, 20.1, 19.0):
            m = ndt.host_deskew_motion(T32, 20.0, 20.1, t_ref)
            k = np.array(list(m.axis))
            assert 0 <= m.angle <= np.pi and abs(np.linalg.norm(k) - 1) <= 1e-12
            assert (m.t_begin, m.t_end, m.t_ref) == (20.0, 20.1, t_ref)
            if angle == 0:
                assert m.angle == 0 and list(k) == [1, 0, 0]
            assert np.abs(rot_of(m) - T32[:3, :3].astype(np.float64)).max() <= 1e-6, (angle, axis)
            u_ref = (t_ref - 20.0) / (20.1 - 20.0)
            want = dc.exp_rot(k, -u_ref * m.angle) @ T32[:3, 3].astype(np.float64)
            assert np.abs(np.array(list(m.tau_ref)) - want).max() <= 1e-12
    assert ndt.host_deskew_motion(np.eye(4), 1.0, 2.0).t_ref == 1.0


def test_host_motion_at_half_a_turn_and_refusals(mods):
    L, _lib, ndt = mods
    for axis in ([0, 0, 1.0], [0.6, 0, -0.8], [1 / 3, 2 / 3, -2 / 3]):
        T = np.eye(4)
        T[:3, :3] = dc.exp_rot(np.array(axis), np.pi)
        m = ndt.host_deskew_motion(T, 0.0, 1.0)
        assert abs(m.angle - np.pi) < 1e-6 and np.abs(rot_of(m) - T[:3, :3].astype(F)).max() <= 1e-6
    out = _lib.DeskewMotion()
    out.angle = -7.0
    eye = np.eye(4, dtype=F).reshape(16)
    fp = eye.ctypes.data_as(C.POINTER(C.c_float))
    assert L.ndt_host_deskew_motion(None, 0.0, 1.0, 0.0, C.byref(out)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_deskew_motion(fp, 0.0, 1.0, 0.0, None) == _lib.NDT_ERR_INVALID
    for times in ((1.0, 1.0, 1.0), (2.0, 1.0, 1.0), (float("nan"), 1.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 1.0, float("nan"))):
        assert L.ndt_host_deskew_motion(fp, *times, C.byref(out)) == _lib.NDT_ERR_INVALID
    bad = eye.copy()
    bad[13] = np.nan
    assert L.ndt_host_deskew_motion(bad.ctypes.data_as(C.POINTER(C.c_float)), 0.0, 1.0, 0.0, C.byref(out)) == _lib.NDT_ERR_INVALID
    assert out.angle == -7.0


def test_plan_tiles_the_points(mods):
    L, _lib, ndt = mods
    plan = ndt.host_deskew_plan
    cap, block = 1024, 256
    assert os.environ.get("NDT_DESKEW_MAX_BLOCKS") is None
    assert plan(0) == (0, block) and plan(1) == (1, block) and plan(block) == (1, block) and plan(block + 1) == (2, block)
    assert plan(cap * block) == (cap, block) and plan(cap * block + 1) == (1021, block + 1)
    ns = {0, 1, 63, 64, 65, block - 1, block, block + 1, 2 * block, 2 * block + 1, cap * block - 1, cap * block, cap * block + 1}
    for ppb in range(block, 300000 // cap + 2):
        ns |= {cap * ppb, cap * ppb + 1}
    last = 0
    for n in sorted(ns) + [2 ** 31 - 1]:
        blocks, ppb = plan(n)
        assert 0 <= blocks <= cap and ppb >= block and ppb >= last
        last = ppb
        assert (blocks - 1) * ppb < n <= blocks * ppb or (n == 0 and blocks == 0)
    b, p = C.c_int(-3), C.c_int(-3)
    assert L.ndt_host_deskew_plan(2 ** 31, C.byref(b), C.byref(p)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_deskew_plan(5, None, C.byref(p)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_deskew_plan(5, C.byref(b), None) == _lib.NDT_ERR_INVALID
    assert (b.value, p.value) == (-3, -3)


def test_refusals_leave_the_outputs_untouched(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    ok = to_ctypes(motions()[0], _lib)
    times = np.zeros(4)
    tp = C.c_void_p(times.ctypes.data)

    class Args:
        def __init__(self):
            self.out = C.c_void_p(SENTINEL)
            self.outs = (C.c_void_p * 4)(*([SENTINEL] * 4))
            self.nu = C.c_size_t(SENTINEL)
            self.nus = (C.c_size_t * 4)(*([SENTINEL] * 4))

        def untouched(self, out_null=False, outs_null=0):
            return ((self.out.value is None if out_null else self.out.value == SENTINEL)
                    and all(self.outs[k] is None for k in range(outs_null)) and all(self.outs[k] == SENTINEL for k in range(outs_null, 4))
                    and self.nu.value == SENTINEL and all(v == SENTINEL for v in self.nus))
    # ndt_cloud_deskew: NULL handle / out / in (no cloud can exist without a device: the refusals that need one are GPU tests)
    a = Args()
    assert L.ndt_cloud_deskew(None, None, C.byref(ok), tp, 0, C.byref(a.out), C.byref(a.nu)) == _lib.NDT_ERR_INVALID
    assert a.untouched(out_null=True)
    a = Args()
    assert L.ndt_cloud_deskew(g._h, None, C.byref(ok), tp, 0, None, C.byref(a.nu)) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    a = Args()
    assert L.ndt_cloud_deskew(g._h, None, C.byref(ok), tp, 0, C.byref(a.out), C.byref(a.nu)) == _lib.NDT_ERR_INVALID
    assert a.untouched(out_null=True)
    # ndt_cloud_deskew_clouds: NULL handle / out, too many clouds, NULL in / motions / entries
    null_entries = (C.c_void_p * 4)()
    ms = (_lib.DeskewMotion * 4)(*([ok] * 4))
    a = Args()
    assert L.ndt_cloud_deskew_clouds(None, null_entries, 4, ms, tp, 0, a.outs, a.nus) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    assert L.ndt_cloud_deskew_clouds(g._h, null_entries, 4, ms, tp, 0, None, a.nus) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    assert L.ndt_cloud_deskew_clouds(g._h, null_entries, 65536, ms, tp, 0, a.outs, a.nus) == _lib.NDT_ERR_INVALID
    assert a.untouched()                        # (refused before the 65 536 outputs it does not have are written)
    for in_p, m_p in ((None, ms), (null_entries, None), (null_entries, ms)):
        a = Args()
        assert L.ndt_cloud_deskew_clouds(g._h, in_p, 4, m_p, tp, 0, a.outs, a.nus) == _lib.NDT_ERR_INVALID
        assert a.untouched(outs_null=4)
    n = C.c_size_t(SENTINEL)
    assert L.ndt_diag_deskew(None, C.byref(n), C.byref(n), C.byref(n)) == _lib.NDT_ERR_INVALID
    assert L.ndt_diag_deskew(g._h, None, C.byref(n), C.byref(n)) == _lib.NDT_ERR_INVALID and n.value == SENTINEL
    # no clouds: NDT_OK without a device, nothing touched
    a = Args()
    assert L.ndt_cloud_deskew_clouds(g._h, None, 0, None, None, 0, a.outs, a.nus) == _lib.NDT_OK
    assert a.untouched()
    assert g.deskewClouds([], [], []) == ([], [])
    assert g.deskewDiag() == dict(launches=0, blocks=0, clouds=0)
    if L.ndt_device_count() == 0:
        with pytest.raises(ndt.NdtError) as e:
            g.uploadCloud(np.zeros((3, 3), F))
        assert e.value.status == _lib.NDT_ERR_NO_DEVICE


# ---- where the times come from ----------------------------------------------------------------------------------------------
NP_OF = {"int8": "i1", "uint8": "u1", "int16": "<i2", "uint16": "<u2", "int32": "<i4", "uint32": "<u4", "float32": "<f4", "float64": "<f8"}


def test_extract_field_for_the_eight_datatypes_at_odd_offsets(mods):
    L, _lib, ndt = mods
    rng = np.random.default_rng(9)
    n = 257
    for name, code in ndt.POINTFIELD_TYPES.items():
        dt = np.dtype(NP_OF[name])
        if dt.kind == "f":
            vals = rng.standard_normal(n).astype(dt) * 1e3
            vals[::31] = np.nan
            vals[5] = np.inf
        else:
            info = np.iinfo(dt)
            vals = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
            vals[0], vals[1] = info.min, info.max
        for step, off in ((22, 18 if dt.itemsize <= 4 else 13), (dt.itemsize, 0), (37, 37 - dt.itemsize), (23, 1)):
            buf = rng.integers(0, 256, n * step, dtype=np.uint8)
            rows = buf.reshape(n, step)
            rows[:, off:off + dt.itemsize] = vals.view(np.uint8).reshape(n, dt.itemsize)
            for dtype in (name, code):
                got = ndt.extract_field(buf.tobytes(), n, step, off, dtype)
                assert got.dtype == np.float64 and np.array_equal(got, vals.astype(np.float64), equal_nan=True), (name, step, off)
    # the Velodyne record of ndt_host_repack_fields' comment: x y z f32, intensity f32, ring u16, time f32 at 18
    rec = np.zeros(n, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("i", "<f4"), ("ring", "<u2"), ("t", "<f4")]))
    assert rec.dtype.itemsize == 22
    rec["t"] = np.linspace(0, 0.1, n).astype(F)
    assert np.array_equal(ndt.extract_field(rec.tobytes(), n, 22, 18, "float32"), rec["t"].astype(np.float64))
    out = np.full(4, -7.0)
    op = out.ctypes.data_as(C.POINTER(C.c_double))
    data = np.zeros(64, np.uint8)
    for args in ((data.ctypes.data, 4, 16, 0, 0), (data.ctypes.data, 4, 16, 0, 9), (data.ctypes.data, 4, 16, 13, 7), (data.ctypes.data, 4, 16, 9, 8),
                 (data.ctypes.data, 4, 16, 17, 2), (data.ctypes.data, 4, 0, 0, 2), (None, 4, 16, 0, 7)):
        assert L.ndt_host_extract_field(*args, op) == _lib.NDT_ERR_INVALID, args
    assert L.ndt_host_extract_field(data.ctypes.data, 4, 16, 0, 7, None) == _lib.NDT_ERR_INVALID
    assert (out == -7).all()
    assert L.ndt_host_extract_field(None, 0, 16, 0, 7, None) == _lib.NDT_OK


def lzf_literal(raw):
    out = b""
    for i in range(0, len(raw), 32):
        part = raw[i:i + 32]
        out += bytes([len(part) - 1]) + part
    return out


def write_pcd(path, columns, kind):
    """columns: [(name, numpy dtype string, TYPE letter, COUNT, (n, COUNT) array)]"""
    n = len(columns[0][4])
    hdr = "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\nCOUNT %s\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA %s\n" % (
        " ".join(c[0] for c in columns), " ".join(str(np.dtype(c[1]).itemsize) for c in columns), " ".join(c[2] for c in columns),
        " ".join(str(c[3]) for c in columns), n, n, kind)
    cols = [np.asarray(c[4]).reshape(n, c[3]).astype(c[1]) for c in columns]
    with open(path, "wb") as f:
        f.write(hdr.encode())
        if kind == "ascii":
            for i in range(n):
                toks = []
                for c, a in zip(columns, cols):
                    for v in a[i]:
                        toks.append(("nan" if np.isnan(v) else repr(float(v))) if c[2] == "F" else str(int(v)))
                f.write((" ".join(toks) + "\n").encode())
        elif kind == "binary":
            f.write(b"".join(b"".join(a[i].tobytes() for a in cols) for i in range(n)))
        else:
            raw = b"".join(a.tobytes() for a in cols)
            comp = lzf_literal(raw)
            f.write(struct.pack("<II", len(comp), len(raw)) + comp)


@pytest.mark.parametrize("kind", ("ascii", "binary", "binary_compressed"))
def test_pcd_read_field(mods, tmp_path, kind):
    L, _lib, ndt = mods
    rng = np.random.default_rng(11)
    n = 333
    xyz = rng.standard_normal((n, 3)).astype(F)
    t64 = 1.7e9 + np.sort(rng.uniform(0, 0.1, n))
    t32 = np.linspace(0, 0.1, n).astype(F)
    t32[7] = np.nan
    ints = {"i1": ("I", "i1"), "u1": ("U", "u1"), "i2": ("I", "<i2"), "u2": ("U", "<u2"), "i4": ("I", "<i4"), "u4": ("U", "<u4"),
            "i8": ("I", "<i8"), "u8": ("U", "<u8")}
    columns = [("x", "<f4", "F", 1, xyz[:, 0]), ("normal", "<f4", "F", 3, rng.standard_normal((n, 3))), ("y", "<f4", "F", 1, xyz[:, 1]),
               ("t", "<f8", "F", 1, t64), ("z", "<f4", "F", 1, xyz[:, 2]), ("time", "<f4", "F", 1, t32)]
    want = {"t": t64, "time": t32.astype(np.float64), "x": xyz[:, 0].astype(np.float64)}
    for name, (letter, dt) in ints.items():
        info = np.iinfo(np.dtype(dt))
        v = rng.integers(max(info.min, -2 ** 52), min(info.max, 2 ** 52), n, dtype=np.dtype(dt), endpoint=True)
        columns.append((name, dt, letter, 1, v))
        want[name] = v.astype(np.float64)
    p = str(tmp_path / ("fields_%s.pcd" % kind))
    write_pcd(p, columns, kind)
    for name, w in want.items():
        got = ndt.pcd_read_field(p, name)
        assert got.dtype == np.float64 and np.array_equal(got, w, equal_nan=True), (kind, name)
    got_xyz, _ = ndt.pcd_read_xyz(p)
    assert np.array_equal(got_xyz, xyz)
    # refused: an absent field, a field with COUNT > 1, a small buffer (the count still comes back), NULLs, a missing file
    out = np.full(n, -7.0)
    op = out.ctypes.data_as(C.POINTER(C.c_double))
    cnt = C.c_size_t(SENTINEL)
    for name in (b"absent", b"normal", b"T", b""):
        assert L.ndt_pcd_read_field(p.encode(), name, op, n, C.byref(cnt)) == _lib.NDT_ERR_INVALID, name
    assert cnt.value == SENTINEL
    assert L.ndt_pcd_read_field(p.encode(), b"t", op, n - 1, C.byref(cnt)) == _lib.NDT_ERR_INVALID and cnt.value == n
    assert L.ndt_pcd_read_field(None, b"t", op, n, None) == _lib.NDT_ERR_INVALID
    assert L.ndt_pcd_read_field(p.encode(), None, op, n, None) == _lib.NDT_ERR_INVALID
    assert L.ndt_pcd_read_field(p.encode(), b"t", None, n, None) == _lib.NDT_ERR_INVALID
    assert L.ndt_pcd_read_field(str(tmp_path / "missing.pcd").encode(), b"t", op, n, None) == _lib.NDT_ERR_INVALID
    assert (out == -7).all()
    with pytest.raises(ndt.NdtError):
        ndt.pcd_read_field(p, "normal")


def test_pcd_read_field_refuses_odd_types(mods, tmp_path):
    L, _lib, ndt = mods
    n = 4
    for size, letter in ((2, "F"), (3, "U"), (5, "I"), (4, "X")):
        p = str(tmp_path / ("odd_%d%s.pcd" % (size, letter)))
        hdr = "VERSION 0.7\nFIELDS x y z t\nSIZE 4 4 4 %d\nTYPE F F F %s\nCOUNT 1 1 1 1\nWIDTH %d\nHEIGHT 1\nPOINTS %d\nDATA binary\n" % (size, letter, n, n)
        with open(p, "wb") as f:
            f.write(hdr.encode() + bytes(n * (12 + size)))
        with pytest.raises(ndt.NdtError):
            ndt.pcd_read_field(p, "t")
        assert len(ndt.pcd_read_field(p, "x")) == n


def test_field_reader_survives_mutated_files_under_sanitizers(tmp_path):
    """tests/pcd_field_fuzz.cpp: mutated ascii / binary / compressed files through ndt::pcd_read_field, built with ASan + UBSan
    (host code, a program of its own): parsed or rejected, never a crash or an out-of-bounds access, and it ends."""
    exe = str(tmp_path / "pcd_field_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "toyslam_amd", "csrc"), os.path.join(ROOT, "tests", "pcd_field_fuzz.cpp"),
                           os.path.join(ROOT, "toyslam_amd", "csrc", "ndt_pcd.cpp"), "-o", exe])
    out = subprocess.run([exe, "4000", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "no crash" in out.stdout
    m = re.search(r"(\d+) parsed, (\d+) rejected", out.stdout)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) > 100, out.stdout
