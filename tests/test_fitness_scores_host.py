"""CPU: ndt_pairs_fitness_scores / ndt_batch_fitness_scores* -- exported, their argument checks done before any device work
(so they hold with or without a GPU), and the Python side of pairsFitness / batchFitness."""
import ctypes as C

import numpy as np
import pytest

DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def test_fitness_entries_are_exported(mods):
    L, _lib, ndt = mods
    for name in ("ndt_pairs_fitness_scores", "ndt_batch_fitness_scores", "ndt_batch_fitness_scores_device"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None


def call_batch(L, h, pts, offsets, n_scans, T, fit, stride=16, device=False):
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
    fn = L.ndt_batch_fitness_scores_device if device else L.ndt_batch_fitness_scores
    return fn(h, None if pts is None else pts.ctypes.data, None if off is None else off.ctypes.data_as(C.POINTER(C.c_size_t)),
              n_scans, stride, None if T is None else T.ctypes.data_as(C.POINTER(C.c_float)), DBL_MAX,
              None if fit is None else fit.ctypes.data_as(C.POINTER(C.c_double)))


def test_batch_argument_errors_are_refused_before_any_device_work(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()  # (no target: an INVALID argument wins over the missing target)
    pts = np.zeros((30, 4), np.float32)
    T = np.tile(np.eye(4, dtype=np.float32).reshape(16), (3, 1))
    fit = np.zeros(3)
    ok = [0, 10, 20, 30]
    bad = [
        dict(h=None),                                   # NULL handle
        dict(offsets=None),                             # NULL offsets
        dict(T=None),                                   # NULL transforms with scans
        dict(fit=None),                                 # NULL fitness with scans
        dict(offsets=[0, 10, 5, 30]),                   # decreasing offsets
        dict(stride=10),                                # stride not a multiple of 4
        dict(stride=8),                                 # ... or below 12 bytes
        dict(pts=None),                                 # NULL points with points
        dict(n_scans=65536, offsets=np.zeros(65537)),   # more than 65535 scans
    ]
    for device in (False, True):
        for b in bad:
            a = dict(h=g._h, pts=pts, offsets=ok, n_scans=3, T=T, fit=fit, stride=16)
            a.update(b)
            st = call_batch(L, a["h"], a["pts"], a["offsets"], a["n_scans"], a["T"], a["fit"], a["stride"], device)
            assert st == _lib.NDT_ERR_INVALID, (device, b)
        # valid arguments, but no target
        assert call_batch(L, g._h, pts, ok, 3, T, fit, device=device) == _lib.NDT_ERR_NO_INPUT
        assert call_batch(L, g._h, pts, [0], 0, None, None, device=device) == _lib.NDT_ERR_NO_INPUT


def test_pairs_fitness_needs_a_pairs_call(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    fit = np.zeros(4)
    d = fit.ctypes.data_as(C.POINTER(C.c_double))
    assert L.ndt_pairs_fitness_scores(None, None, DBL_MAX, d) == _lib.NDT_ERR_INVALID
    assert L.ndt_pairs_fitness_scores(g._h, None, DBL_MAX, d) == _lib.NDT_ERR_NO_INPUT
    assert L.ndt_pairs_fitness_scores(g._h, None, DBL_MAX, None) == _lib.NDT_ERR_NO_INPUT  # (no pairs: nothing to write)
    with pytest.raises(_lib.NdtError) as e:
        g.pairsFitness()
    assert e.value.status == _lib.NDT_ERR_NO_INPUT
    # a pairs call refused on its arguments leaves nothing to score either
    pts = np.zeros((30, 4), np.float32)
    off = np.array([0, 10, 20, 30], np.uintp)
    pr = np.array([0, 5], np.int32)
    T = np.zeros(16, np.float32)
    assert L.ndt_align_pairs(g._h, pts.ctypes.data, off.ctypes.data_as(C.POINTER(C.c_size_t)), 3, 16, 1,
                             pr.ctypes.data_as(C.POINTER(C.c_int)), 1, None, T.ctypes.data_as(C.POINTER(C.c_float)), None, None,
                             None) == _lib.NDT_ERR_INVALID
    assert L.ndt_pairs_fitness_scores(g._h, None, DBL_MAX, d) == _lib.NDT_ERR_NO_INPUT


class _Recorder:
    """stands in for the library: records what the wrappers pass"""

    def __init__(self, status=0, n_pairs=0):
        self.calls = []
        self.status = status
        self.n_pairs = n_pairs  # what ndt_pairs_count reports

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "ndt_pairs_count":
                args[1]._obj.value = self.n_pairs
            return self.status
        return fn


def test_wrappers_pass_shapes_and_nulls(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    rec = _Recorder(n_pairs=3)
    keep = g._L
    g._L = rec
    try:
        # pairsFitness: None -> NULL transforms; P = the pairs the library holds (ndt_pairs_count)
        out = g.pairsFitness()
        assert out.shape == (3,) and out.dtype == np.float64
        name, args = rec.calls[-1]
        assert name == "ndt_pairs_fitness_scores" and args[1] is None and args[2] == DBL_MAX
        Ts = [np.eye(4, dtype=np.float32) * (k + 1) for k in range(3)]
        g.pairsFitness(Ts, max_range=0.25)
        name, args = rec.calls[-1]
        assert args[1] is not None and args[2] == 0.25
        col = np.ctypeslib.as_array(args[1], shape=(3 * 16,)).reshape(3, 4, 4)
        assert np.array_equal(col[2].T, Ts[2])  # column-major, one after the other
        with pytest.raises(ValueError):
            g.pairsFitness(Ts[:2])
        # batchFitness, host clouds: concatenated, offsets, the records' own stride (as alignBatch)
        cl = [np.ones((5, 3), np.float32), np.ones((0, 3), np.float32), np.ones((2, 3), np.float32)]
        out = g.batchFitness(cl, transforms=Ts)
        assert out.shape == (3,)
        name, args = rec.calls[-1]
        assert name == "ndt_batch_fitness_scores" and args[3] == 3 and args[4] == 12
        assert list(np.ctypeslib.as_array(args[2], shape=(4,))) == [0, 5, 5, 7]
        # device form: the pointer, the caller's offsets and stride as given
        out = g.batchFitness(device_ptr=0x1000, offsets=[0, 4, 9], stride_bytes=32, transforms=Ts[:2])
        name, args = rec.calls[-1]
        assert name == "ndt_batch_fitness_scores_device" and args[1].value == 0x1000 and args[3] == 2 and args[4] == 32
        assert out.shape == (2,)
        with pytest.raises(ValueError):
            g.batchFitness(cl)  # transforms are required
        with pytest.raises(ValueError):
            g.batchFitness(cl, transforms=Ts[:2])
    finally:
        g._L = keep


def test_pairs_fitness_buffer_is_the_library_count(mods):
    """the output buffer holds as many values as the library writes, whatever the Python side saw: a pairs call refused
    in Python (before the library is reached) leaves the library's pairs -- and their count -- in place"""
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    rec = _Recorder(n_pairs=12)
    keep = g._L
    g._L = rec
    try:
        with pytest.raises(ValueError):
            g.alignPairs([np.zeros((5, 2), np.float32)] * 3)  # (N, 2): refused by the wrapper, the library never called
        with pytest.raises(ValueError):
            g.alignPairs([np.zeros((5, 3), np.float32), np.zeros((5, 4), np.float32)])  # column counts differ
        assert not [c for c in rec.calls if c[0].startswith("ndt_align_pairs")]
        out = g.pairsFitness()
        name, args = rec.calls[-1]
        assert name == "ndt_pairs_fitness_scores" and out.shape == (12,)
        np.ctypeslib.as_array(args[3], shape=(12,))[:] = 7.0  # the buffer passed holds 12 values
        rec.n_pairs = 0
        assert g.pairsFitness().shape == (0,)
    finally:
        g._L = keep


def test_pairs_count_and_launch_diagnostics_on_a_fresh_handle(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    n = C.c_size_t(99)
    assert L.ndt_pairs_count(g._h, C.byref(n)) == _lib.NDT_OK and n.value == 0
    assert L.ndt_pairs_count(None, C.byref(n)) == _lib.NDT_ERR_INVALID
    assert L.ndt_pairs_count(g._h, None) == _lib.NDT_ERR_INVALID
    assert g.fitnessLaunches() == (0, 0)
    assert L.ndt_diag_fitness_launches(None, C.byref(n), C.byref(n)) == _lib.NDT_ERR_INVALID
