"""CPU: ndt_score_poses / ndt_diag_score_poses / ndt_align_guesses / ndt_host_pick_top / ndt_align_multistart -- declared and
exported, their argument checks done before any device work (so they hold with or without a GPU), the host-only pick
against numpy, the Python wrappers' shapes, and the ORACLE side of tests/test_gpu_score_poses.py: what the GPU tests compare
against is finite and non-zero where the scans overlap and exactly 0.0 for the far poses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import score_poses_cases as spc
from conftest import ROOT

NEW = ("ndt_score_poses", "ndt_diag_score_poses", "ndt_align_guesses", "ndt_host_pick_top", "ndt_align_multistart")


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def test_entries_are_declared_and_exported(mods):
    L, _lib, ndt = mods
    with open(os.path.join(ROOT, "include", "ndt_mi355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\(" % name, header), name + " is not declared in include/ndt_mi355.h"
    for method in ("scorePoses", "alignGuesses", "alignMultistart", "scorePosesLaunches"):
        assert callable(getattr(ndt.NormalDistributionsTransform, method))


def eye_table(n):
    return np.ascontiguousarray(np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1)))


def test_no_poses_is_ok_and_writes_nothing(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()   # no target, no source, no device: none is needed
    T = eye_table(2)
    scores = np.full(2, 7.5)
    assert L.ndt_score_poses(g._h, fp(T), 0, dp(scores)) == _lib.NDT_OK
    assert L.ndt_score_poses(g._h, None, 0, None) == _lib.NDT_OK
    assert list(scores) == [7.5, 7.5]
    out_T, conv, it, tp = np.full((2, 16), 3.0, np.float32), np.full(2, 9, np.int32), np.full(2, 9, np.int32), np.full(2, 7.5)
    best = C.c_int(5)
    assert L.ndt_align_guesses(g._h, fp(T), 0, fp(out_T), ip(conv), ip(it), dp(tp), C.byref(best)) == _lib.NDT_OK
    assert (out_T == 3.0).all() and list(conv) == [9, 9] and list(it) == [9, 9] and list(tp) == [7.5, 7.5]
    assert best.value == -1                  # "-1 if none": the one thing a call without guesses has to say
    assert L.ndt_align_guesses(g._h, None, 0, None, None, None, None, None) == _lib.NDT_OK
    picked, n_picked = np.full(2, 9, np.int32), C.c_size_t(5)
    best = C.c_int(5)
    for n, keep in ((0, 2), (2, 0), (0, 0)):
        assert L.ndt_align_multistart(g._h, fp(T), n, keep, ip(picked), C.byref(n_picked), fp(out_T), ip(conv), ip(it), dp(tp),
                                      C.byref(best)) == _lib.NDT_OK
        assert n_picked.value == 0 and best.value == -1
        assert list(picked) == [9, 9] and (out_T == 3.0).all() and list(tp) == [7.5, 7.5]
    assert g.scorePoses([]).shape == (0,)
    r = g.alignGuesses([])
    assert r["T"].shape == (0, 4, 4) and r["best"] == -1 and r["iterations"].shape == (0,)
    r = g.alignMultistart([], 3)
    assert r["picked"].shape == (0,) and r["best"] == -1


def test_null_arguments_are_refused_without_a_device(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    T, scores = eye_table(2), np.zeros(2)
    assert L.ndt_score_poses(None, fp(T), 2, dp(scores)) == _lib.NDT_ERR_INVALID
    assert L.ndt_score_poses(None, fp(T), 0, dp(scores)) == _lib.NDT_ERR_INVALID   # (the handle is checked whatever n_poses is)
    assert L.ndt_score_poses(g._h, None, 2, dp(scores)) == _lib.NDT_ERR_INVALID
    assert L.ndt_score_poses(g._h, fp(T), 2, None) == _lib.NDT_ERR_INVALID
    n = C.c_size_t(0)
    assert L.ndt_diag_score_poses(None, C.byref(n), C.byref(n)) == _lib.NDT_ERR_INVALID
    assert L.ndt_diag_score_poses(g._h, None, C.byref(n)) == _lib.NDT_ERR_INVALID
    assert L.ndt_diag_score_poses(g._h, C.byref(n), None) == _lib.NDT_ERR_INVALID
    assert g.scorePosesLaunches() == (0, 0)
    assert L.ndt_align_guesses(None, fp(T), 2, None, None, None, None, None) == _lib.NDT_ERR_INVALID
    assert L.ndt_align_guesses(g._h, None, 2, None, None, None, None, None) == _lib.NDT_ERR_INVALID
    assert L.ndt_align_guesses(g._h, fp(T), 65536, None, None, None, None, None) == _lib.NDT_ERR_INVALID   # (refused before the table is read)
    assert L.ndt_align_multistart(None, fp(T), 2, 1, None, None, None, None, None, None, None) == _lib.NDT_ERR_INVALID
    assert L.ndt_align_multistart(g._h, None, 2, 1, None, None, None, None, None, None, None) == _lib.NDT_ERR_INVALID
    # a handle with an all-reduce hook: one source under many poses is not sharded
    g.setAllreduce(lambda buf, n, on_device: 0)
    assert L.ndt_score_poses(g._h, fp(T), 2, dp(scores)) == _lib.NDT_ERR_INVALID
    assert L.ndt_align_guesses(g._h, fp(T), 2, None, None, None, None, None) == _lib.NDT_ERR_INVALID
    assert L.ndt_align_multistart(g._h, fp(T), 2, 1, None, None, None, None, None, None, None) == _lib.NDT_ERR_INVALID
    assert list(scores) == [0.0, 0.0]


def test_a_valid_call_needs_a_device(mods):
    L, _lib, ndt = mods
    if L.ndt_device_count() >= 1:
        return  # (with a GPU the same calls are tests/test_gpu_score_poses.py's business)
    g = ndt.NormalDistributionsTransform()
    T, scores = eye_table(2), np.full(2, 7.5)
    assert L.ndt_score_poses(g._h, fp(T), 2, dp(scores)) == _lib.NDT_ERR_NO_DEVICE
    assert L.ndt_align_guesses(g._h, fp(T), 2, None, None, None, None, None) == _lib.NDT_ERR_NO_DEVICE
    n_picked, best = C.c_size_t(5), C.c_int(5)
    assert L.ndt_align_multistart(g._h, fp(T), 2, 1, None, C.byref(n_picked), None, None, None, None, C.byref(best)) == _lib.NDT_ERR_NO_DEVICE
    assert list(scores) == [7.5, 7.5] and n_picked.value == 0 and best.value == -1
    with pytest.raises(ndt.NdtError) as e:
        g.scorePoses([np.eye(4)])
    assert e.value.status == _lib.NDT_ERR_NO_DEVICE


def test_pick_top_against_argsort(mods):
    L, _lib, ndt = mods
    inf, nan = np.inf, np.nan
    vectors = [
        [0.3, 0.1, 0.3, 0.2, 0.3],                      # ties: the lower index first
        [nan, 0.5, inf, -inf, 0.5, -1.0, nan, 0.25],    # NaN and the infinities are no scores
        [nan, nan, inf],                                # nothing finite
        [0.0] * 6,                                      # all tied (every candidate far away)
        [-0.0, 0.0, -0.0],                              # the two zeros tie
        [1.5],
        [],
    ]
    rng = np.random.default_rng(5)
    big = np.round(rng.normal(0, 1, 500), 1)            # many ties
    big[rng.choice(500, 40, replace=False)] = nan
    big[rng.choice(500, 10, replace=False)] = -inf
    vectors.append(list(big))
    for v in vectors:
        for keep in (0, 1, 2, 4, len(v), len(v) + 3, 1000):
            got = ndt.host_pick_top(v, keep)
            want = spc.argsort_top(v, keep)
            assert got.dtype == np.int32 and list(got) == list(want), (v[:8], keep)
    # the raw entry: nothing is written past *n_out, NULL outputs are tolerated
    s = np.array([0.2, nan, 0.9, 0.2])
    idx, n = np.full(4, -7, np.int32), C.c_size_t(99)
    L.ndt_host_pick_top(dp(s), 4, 2, ip(idx), C.byref(n))
    assert n.value == 2 and list(idx) == [2, 0, -7, -7]
    L.ndt_host_pick_top(dp(s), 4, 4, ip(idx), C.byref(n))
    assert n.value == 3 and list(idx) == [2, 0, 3, -7]
    L.ndt_host_pick_top(dp(s), 4, 0, ip(idx), C.byref(n))
    assert n.value == 0
    L.ndt_host_pick_top(dp(s), 4, 2, None, C.byref(n))
    L.ndt_host_pick_top(dp(s), 4, 2, ip(idx), None)
    L.ndt_host_pick_top(None, 0, 2, ip(idx), C.byref(n))
    assert n.value == 0


class _Recorder:
    """stands in for the library: records what the wrappers pass"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_wrappers_pass_column_major_tables(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    rec, keep = _Recorder(), g._L
    g._L = rec
    try:
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = (1, 2, 3)
        T[0, 1] = 0.5
        out = g.scorePoses([np.eye(4), T])
        name, args = rec.calls[-1]
        assert name == "ndt_score_poses" and args[2] == 2 and out.shape == (2,)
        tab = np.ctypeslib.as_array(args[1], shape=(32,))
        assert list(tab[28:31]) == [1, 2, 3] and tab[16 + 4] == 0.5 and tab[0] == tab[5] == tab[15] == 1
        r = g.alignGuesses([T, T, T])
        name, args = rec.calls[-1]
        assert name == "ndt_align_guesses" and args[2] == 3 and r["T"].shape == (3, 4, 4) and r["converged"].shape == (3,)
        r = g.alignMultistart([T] * 5, 2)
        name, args = rec.calls[-1]
        assert name == "ndt_align_multistart" and args[2] == 5 and args[3] == 2
        with pytest.raises(ValueError):
            g.alignMultistart([T], -1)
    finally:
        g._L = keep


# ------------------------------------------------------------------ the oracle side of the GPU tests
@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


def test_oracle_scores_of_the_test_poses(po, pair, golden):
    t, s = pair
    P = spc.poses(golden)
    far = spc.far_poses(40)
    for method in spc.METHODS:
        o = po.OracleNDT(num_threads=8, search_method=getattr(po, method))
        o.set_target(t)
        o.set_source(s)
        sc = [o.calculate_score(spc.moved(po, s, T)) for T in P]
        assert np.isfinite(sc).all(), method
        assert all(sc[k] != 0.0 for k in spc.near_indices()), method
        assert sc[spc.I_FAR] == 0.0, method
        # the registered pose scores highest of the poses that overlap.  (A term is -d1 e - d3 with d3 > 0: a neighbour voxel
        # the point fits badly counts NEGATIVE, so under the widest neighbour rule, DIRECT26, even the registered pose
        # scores below the 0.0 of no overlap at all: calculateScore's own semantics, which a caller ranking candidates
        # must know.)
        assert int(np.argmax(sc[:spc.I_FAR])) == spc.I_GOLDEN and sc[spc.I_GOLDEN] > sc[spc.I_YAW90], method
        assert all(o.calculate_score(spc.moved(po, s[:400], T)) == 0.0 for T in far), method


def test_oracle_transform_is_the_f32_chain_the_kernel_uses(po, pair):
    """x T00 + (y T01 + (z T02 + T03)), every product and sum rounded to f32: what xform_point computes on the device."""
    _, s = pair
    T = spc.make_T([0.4, -7.25, 1000.0], [0.01, -0.02, 1.2])
    c = s[:257]
    got = spc.moved(po, c, T)
    x, y, z = (c[:, k].astype(np.float32) for k in range(3))
    for r in range(3):
        want = x * T[r, 0] + (y * T[r, 1] + (z * T[r, 2] + T[r, 3]))
        assert want.dtype == np.float32 and np.array_equal(got[:, r], want)
    assert np.array_equal(got[:, 3], np.ones(len(c), np.float32))
    bad = spc.moved(po, spc.spoiled(c), T)
    assert not np.isfinite(bad[len(c) // 3, :3]).any() and not np.isfinite(bad[len(c) - 1, :3]).all()
