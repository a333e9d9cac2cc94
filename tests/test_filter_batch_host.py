"""CPU: ndt_cloud_voxel_filter_batch / _clouds and ndt_diag_filter_batch -- exported, their argument checks done before any
device work (so they hold with or without a GPU, and leave every out[k] NULL), and the Python side of voxelGridFilterClouds /
voxelGridFilterBatchDevice."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def test_filter_batch_entries_are_exported(mods):
    L, _lib, ndt = mods
    for name in ("ndt_cloud_voxel_filter_batch", "ndt_cloud_voxel_filter_clouds", "ndt_diag_filter_batch"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None


def poisoned(n):
    out = (C.c_void_p * max(n, 1))()
    for k in range(max(n, 1)):
        out[k] = 0x1234  # whatever the caller's array held: must come back NULL
    return out


def call_buffer(L, h, pts, offsets, n, stride=16, leaf=0.5, out="new", ov="new", device=False):
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
    o = poisoned(n) if out == "new" else out
    f = np.full(max(n, 1), 7, np.int32) if ov == "new" else ov
    st = L.ndt_cloud_voxel_filter_batch(h, None if pts is None else pts.ctypes.data,
                                        None if off is None else off.ctypes.data_as(C.POINTER(C.c_size_t)), n, stride, None, leaf,
                                        int(device), o, None if f is None else f.ctypes.data_as(C.POINTER(C.c_int)))
    return st, o, f


def test_buffer_argument_errors_are_refused_before_any_device_work(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    pts = np.zeros((30, 4), np.float32)
    ok = [0, 10, 20, 30]
    bad = [
        dict(h=None),                                   # NULL handle
        dict(out=None),                                 # NULL out
        dict(leaf=0.0),                                 # leaf size not > 0
        dict(leaf=float("nan")),
        dict(offsets=None),                             # NULL offsets with clouds
        dict(offsets=[0, 10, 5, 30]),                   # decreasing offsets
        dict(stride=10),                                # stride not a multiple of 4
        dict(stride=8),                                 # ... or below 12 bytes
        dict(pts=None),                                 # NULL points with points
        dict(n=65536, offsets=np.zeros(65537)),         # more than 65535 clouds
    ]
    for device in (False, True):
        for b in bad:
            a = dict(h=g._h, pts=pts, offsets=ok, n=3, stride=16, leaf=0.5, out="new")
            a.update(b)
            st, o, f = call_buffer(L, a["h"], a["pts"], a["offsets"], a["n"], a["stride"], a["leaf"], a["out"], device=device)
            assert st == _lib.NDT_ERR_INVALID, (device, b)
            if o is not None and a["h"] is not None:
                assert all(o[k] is None for k in range(a["n"])), (device, b)
                assert not f[:a["n"]].any(), (device, b)
    # no clouds at all: nothing to do, no device needed
    st, _, _ = call_buffer(L, g._h, None, [0], 0)
    assert st == _lib.NDT_OK
    st, _, _ = call_buffer(L, g._h, None, None, 0)
    assert st == _lib.NDT_OK


def test_clouds_argument_errors_are_refused_before_any_device_work(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    fn = L.ndt_cloud_voxel_filter_clouds
    one = (C.c_void_p * 2)(None, None)  # a NULL entry
    for h, arr, n, leaf, out in [(None, one, 2, 0.5, poisoned(2)),     # NULL handle
                                 (g._h, one, 2, 0.5, None),             # NULL out
                                 (g._h, None, 2, 0.5, poisoned(2)),     # NULL in with clouds
                                 (g._h, one, 2, 0.5, poisoned(2)),      # a NULL entry of in
                                 (g._h, one, 2, -1.0, poisoned(2)),     # leaf size
                                 (g._h, one, 70000, 0.5, poisoned(70000))]:  # more than 65535 clouds
        f = np.full(max(n, 1), 7, np.int32)
        assert fn(h, arr, n, None, leaf, out, f.ctypes.data_as(C.POINTER(C.c_int))) == _lib.NDT_ERR_INVALID
        if out is not None and h is not None:
            assert all(out[k] is None for k in range(n)) and not f[:n].any()
    assert fn(g._h, None, 0, None, 0.5, poisoned(0), None) == _lib.NDT_OK


def test_diag_on_a_fresh_handle(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    assert g.filterBatchDiag() == dict(passes=0, single_route=0, launches=0)
    n = C.c_size_t(0)
    assert L.ndt_diag_filter_batch(None, C.byref(n), C.byref(n), C.byref(n)) == _lib.NDT_ERR_INVALID
    assert L.ndt_diag_filter_batch(g._h, None, C.byref(n), C.byref(n)) == _lib.NDT_ERR_INVALID


class _Recorder:
    """stands in for the library: records what the wrappers pass"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_wrappers_refuse_mixes_and_pass_shapes(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    rec = _Recorder()
    keep = g._L
    g._L = rec
    try:
        fake = ndt.DeviceCloud(g, None)  # (an ndt_cloud stand-in: nothing to release)
        host = np.ones((5, 3), np.float32)
        with pytest.raises(ValueError):
            g.voxelGridFilterClouds([host, fake], 0.5)
        with pytest.raises(ValueError):
            g.voxelGridFilterClouds([fake, host], 0.5)
        with pytest.raises(ValueError):
            g.voxelGridFilterClouds([host, host], 0.5, is_dense=[True])  # one flag per cloud
        with pytest.raises(ValueError):
            g.voxelGridFilterClouds([fake, fake], 0.5, is_dense=[True, False, True])
        with pytest.raises(ValueError):
            g.voxelGridFilterBatchDevice(0x1000, [0, 4, 9], 16, 0.5, is_dense=[1, 0, 1])
        with pytest.raises(ValueError):
            g.voxelGridFilterClouds([np.ones((5, 3), np.float32), np.ones((5, 4), np.float32)], 0.5)  # column counts differ
        assert not rec.calls  # every refusal before the library
        # host clouds: concatenated, offsets, the records' own stride, one flag per cloud
        cl = [np.ones((5, 3), np.float32), np.ones((0, 3), np.float32), np.ones((2, 3), np.float32)]
        outs, ov = g.voxelGridFilterClouds(cl, 0.25, is_dense=[True, False, True])
        name, args = rec.calls[-1]
        assert name == "ndt_cloud_voxel_filter_batch" and args[3] == 3 and args[4] == 12 and args[7] == 0
        assert abs(args[6] - 0.25) < 1e-7
        assert list(np.ctypeslib.as_array(args[2], shape=(4,))) == [0, 5, 5, 7]
        assert list(np.ctypeslib.as_array(args[5], shape=(3,))) == [1, 0, 1]
        assert len(outs) == 3 and ov.shape == (3,) and ov.dtype == bool
        # one bool for every cloud
        g.voxelGridFilterClouds(cl, 0.5, is_dense=False)
        assert list(np.ctypeslib.as_array(rec.calls[-1][1][5], shape=(3,))) == [0, 0, 0]
        # resident clouds: the clouds form
        g.voxelGridFilterClouds([fake, fake], 0.5)
        name, args = rec.calls[-1]
        assert name == "ndt_cloud_voxel_filter_clouds" and args[2] == 2
        # the device buffer form: the pointer, the caller's offsets and stride as given
        outs, ov = g.voxelGridFilterBatchDevice(0x1000, [0, 4, 9], 32, 0.5)
        name, args = rec.calls[-1]
        assert name == "ndt_cloud_voxel_filter_batch" and args[1].value == 0x1000 and args[3] == 2 and args[4] == 32 and args[7] == 1
        assert len(outs) == 2
        # no clouds
        outs, ov = g.voxelGridFilterClouds([], 0.5)
        assert outs == [] and ov.shape == (0,)
        for o in outs:
            o._c = None
    finally:
        g._L = keep
