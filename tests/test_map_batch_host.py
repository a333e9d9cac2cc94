"""CPU: ndt_map_update_clouds / ndt_map_update_batch / ndt_diag_map_batch -- exported, their argument checks done before any
device work (so they hold with or without a GPU and leave the map as it was), and the Python side of mapUpdateClouds /
mapUpdateBatch / mapUpdateBatchDevice."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def test_map_batch_entries_are_exported(mods):
    L, _lib, ndt = mods
    for name in ("ndt_map_update_clouds", "ndt_map_update_batch", "ndt_diag_map_batch"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None


def map_size(L, _lib, h):
    n = C.c_size_t(99)
    assert L.ndt_map_size(h, C.byref(n)) == _lib.NDT_OK
    return n.value


def call_buffer(L, h, pts, offsets, n, stride=16, leaf=0.5, device=False, poses=None):
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
    ov = C.c_int(7)
    st = L.ndt_map_update_batch(h, None if pts is None else pts.ctypes.data,
                                None if off is None else off.ctypes.data_as(C.POINTER(C.c_size_t)), n, stride, None, poses, leaf,
                                int(device), C.byref(ov))
    return st, ov.value


def test_buffer_argument_errors_are_refused_before_any_device_work(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    pts = np.zeros((30, 4), np.float32)
    ok = [0, 10, 20, 30]
    bad = [
        dict(h=None),                                   # NULL handle
        dict(leaf=0.0),                                 # leaf size not > 0
        dict(leaf=-1.0),
        dict(leaf=float("nan")),
        dict(offsets=None),                             # NULL offsets with scans
        dict(offsets=[0, 10, 5, 30]),                   # decreasing offsets
        dict(stride=10),                                # stride not a multiple of 4
        dict(stride=8),                                 # ... or below 12 bytes
        dict(pts=None),                                 # NULL points with points
        dict(n=65536, offsets=np.zeros(65537)),         # more than 65535 scans
        dict(n=2, offsets=[0, 2 ** 30, 2 ** 31]),       # a total above INT_MAX points (refused before the buffer is read)
    ]
    for device in (False, True):
        for b in bad:
            a = dict(h=g._h, pts=pts, offsets=ok, n=3, stride=16, leaf=0.5)
            a.update(b)
            st, ov = call_buffer(L, a["h"], a["pts"], a["offsets"], a["n"], a["stride"], a["leaf"], device=device)
            assert st == _lib.NDT_ERR_INVALID, (device, b)
            if a["h"] is not None:
                assert ov == 0, (device, b)
            assert map_size(L, _lib, g._h) == 0  # the map is what it was, and asking needs no device
    # no scans at all: nothing to do, no device needed
    for device in (False, True):
        assert call_buffer(L, g._h, None, [0], 0, device=device) == (_lib.NDT_OK, 0)
        assert call_buffer(L, g._h, None, None, 0, device=device) == (_lib.NDT_OK, 0)
        assert call_buffer(L, g._h, pts, ok, 0, device=device) == (_lib.NDT_OK, 0)
    assert map_size(L, _lib, g._h) == 0


def test_clouds_argument_errors_are_refused_before_any_device_work(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    fn = L.ndt_map_update_clouds
    two = (C.c_void_p * 2)(None, None)  # NULL entries
    for h, arr, n, leaf in [(None, two, 2, 0.5),       # NULL handle
                            (g._h, None, 2, 0.5),      # NULL scans with scans
                            (g._h, two, 2, 0.5),       # a NULL entry of scans
                            (g._h, two, 2, 0.0),       # leaf size
                            (g._h, two, 2, float("nan")),
                            (g._h, two, 70000, 0.5)]:  # more than 65535 scans
        ov = C.c_int(7)
        assert fn(h, arr, n, None, None, leaf, C.byref(ov)) == _lib.NDT_ERR_INVALID
        if h is not None:
            assert ov.value == 0
        assert map_size(L, _lib, g._h) == 0
    ov = C.c_int(7)
    assert fn(g._h, None, 0, None, None, 0.5, C.byref(ov)) == _lib.NDT_OK and ov.value == 0
    assert fn(g._h, two, 0, None, None, 0.5, None) == _lib.NDT_OK
    assert fn(g._h, None, 0, None, None, -0.5, None) == _lib.NDT_ERR_INVALID  # (the leaf size is checked whatever n_scans is)
    assert map_size(L, _lib, g._h) == 0


def test_diag_on_a_fresh_handle(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    assert g.mapBatchDiag() == dict(transform_launches=0, filters=0, box_passes=0)
    n = C.c_size_t(0)
    assert L.ndt_diag_map_batch(None, C.byref(n), C.byref(n), C.byref(n)) == _lib.NDT_ERR_INVALID
    assert L.ndt_diag_map_batch(g._h, None, C.byref(n), C.byref(n)) == _lib.NDT_ERR_INVALID
    assert L.ndt_diag_map_batch(g._h, C.byref(n), None, C.byref(n)) == _lib.NDT_ERR_INVALID
    assert L.ndt_diag_map_batch(g._h, C.byref(n), C.byref(n), None) == _lib.NDT_ERR_INVALID


class _Recorder:
    """stands in for the library: records what the wrappers pass"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_wrappers_check_and_pass_shapes(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    rec = _Recorder()
    keep = g._L
    g._L = rec
    try:
        fake = ndt.DeviceCloud(g, None)  # (an ndt_cloud stand-in: nothing to release)
        host = np.ones((5, 3), np.float32)
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = (1, 2, 3)
        with pytest.raises(ValueError):
            g.mapUpdateClouds([fake, host])                         # host arrays belong to mapUpdateBatch
        with pytest.raises(ValueError):
            g.mapUpdateClouds([fake, fake], poses=[T])              # one pose per scan
        with pytest.raises(ValueError):
            g.mapUpdateClouds([fake], poses=[T, T])
        with pytest.raises(ValueError):
            g.mapUpdateBatch([host, host], poses=[T, T, T])
        with pytest.raises(ValueError):
            g.mapUpdateBatchDevice(0x1000, [0, 4, 9], 16, poses=[T])
        with pytest.raises(ValueError):
            g.mapUpdateClouds([fake, fake], is_dense=[True])        # one flag per scan
        with pytest.raises(ValueError):
            g.mapUpdateBatch([host, host], is_dense=[True, False, True])
        with pytest.raises(ValueError):
            g.mapUpdateBatchDevice(0x1000, [0, 4, 9], 16, is_dense=[1, 0, 1])
        with pytest.raises(ValueError):
            g.mapUpdateBatch([np.ones((5, 3), np.float32), np.ones((5, 4), np.float32)])  # column counts differ
        assert not rec.calls  # every refusal before the library
        # the clouds form: the handles, one flag and one column-major pose per scan
        size, ov = g.mapUpdateClouds([fake, fake], poses=[T, np.eye(4)], leaf_size=0.25, is_dense=[True, False])
        name, args = rec.calls[-2]  # (the last call is the wrapper's ndt_map_size)
        assert rec.calls[-1][0] == "ndt_map_size" and size == 0 and ov is False
        assert name == "ndt_map_update_clouds" and args[2] == 2 and abs(args[5] - 0.25) < 1e-7
        assert list(np.ctypeslib.as_array(args[3], shape=(2,))) == [1, 0]
        P = np.ctypeslib.as_array(args[4], shape=(32,))
        assert list(P[12:15]) == [1, 2, 3] and P[0] == P[5] == P[10] == P[15] == 1 and P[16] == 1 and not P[28:31].any()
        # one bool for every scan, no poses: NULL = the identity for all
        g.mapUpdateClouds([fake, fake, fake], is_dense=False)
        name, args = rec.calls[-2]
        assert args[2] == 3 and list(np.ctypeslib.as_array(args[3], shape=(3,))) == [0, 0, 0] and args[4] is None
        # host scans: concatenated once, offsets, the records' own stride
        cl = [np.ones((5, 3), np.float32), np.ones((0, 3), np.float32), np.ones((2, 3), np.float32)]
        g.mapUpdateBatch(cl, poses=[T, T, T], leaf_size=0.2, is_dense=[True, False, True])
        name, args = rec.calls[-2]
        assert name == "ndt_map_update_batch" and args[3] == 3 and args[4] == 12 and args[8] == 0
        assert abs(args[7] - 0.2) < 1e-7
        assert list(np.ctypeslib.as_array(args[2], shape=(4,))) == [0, 5, 5, 7]
        assert list(np.ctypeslib.as_array(args[5], shape=(3,))) == [1, 0, 1]
        assert np.ctypeslib.as_array(args[6], shape=(48,))[12 + 32] == 1
        # the device buffer form: the pointer, the caller's offsets and stride as given
        g.mapUpdateBatchDevice(0x1000, [0, 4, 9], 32, poses=[T, T], leaf_size=0.5)
        name, args = rec.calls[-2]
        assert name == "ndt_map_update_batch" and args[1].value == 0x1000 and args[3] == 2 and args[4] == 32 and args[8] == 1
        assert list(np.ctypeslib.as_array(args[2], shape=(3,))) == [0, 4, 9]
        # no scans
        g.mapUpdateClouds([])
        assert rec.calls[-2][0] == "ndt_map_update_clouds" and rec.calls[-2][1][2] == 0 and rec.calls[-2][1][4] is None
        g.mapUpdateBatch([], poses=[])
        assert rec.calls[-2][0] == "ndt_map_update_batch" and rec.calls[-2][1][3] == 0
    finally:
        g._L = keep
