"""CPU: the pose covariance's host side.  ndt_host_pose_covariance (steps 7 and 8 of the definition: a 6x6 Jacobi
eigen-decomposition, A^-1, Laplace / sandwich, the indefinite flag) against the same formula through numpy.linalg.eigh
(tests/pose_cov_cases.covariance) on random symmetric positive definite A with condition number up to 1e6: relative Frobenius
error <= 1e-9, i.e. eps x kappa ~ 1e-10 with a tenfold margin.  The entries are declared, exported and bound; every refusal
that precedes device work leaves sentinel-filled outputs untouched, so it holds with or without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_cov_cases as pc
from conftest import ROOT

NEW = ("ndt_pose_covariance", "ndt_pairs_pose_covariances", "ndt_host_pose_covariance", "ndt_diag_pose_covariance")
SENTINEL = 7.5
BOUND = 1e-9


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def random_case(rng, kappa):
    """A = Q diag(lambda) Q^T with lambda log-spaced over [1, kappa] times a random scale, B = sum of n outer products"""
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    lam = np.exp(rng.uniform(0.0, np.log(kappa), 6))
    lam[0], lam[-1] = 1.0, kappa
    A = (Q * (lam * 10.0 ** rng.uniform(-3, 6))) @ Q.T
    A = (A + A.T) / 2
    n = int(rng.integers(6, 400))
    G = rng.standard_normal((n, 6)) * 10.0 ** rng.uniform(-2, 3, 6)
    return A, G.T @ G, G.sum(axis=0), n


def rel_fro(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def test_entries_are_declared_exported_and_wrapped(mods):
    L, _lib, ndt = mods
    with open(os.path.join(ROOT, "include", "ndt_mi355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\(" % name, header), name + " is not declared in include/ndt_mi355.h"
    for name in ("ndt_pose_information", "NDT_COV_LAPLACE", "NDT_COV_SANDWICH", "NDT_COV_INDEFINITE"):
        assert name in header
    for method in ("poseCovariance", "pairsPoseCovariances", "poseCovarianceLaunches"):
        assert callable(getattr(ndt.NormalDistributionsTransform, method))
    assert callable(ndt.host_pose_covariance)
    # the structure the bindings fill is the header's: 36 + 36 + 6 doubles, a size_t, two doubles, an int (padded to 8)
    assert C.sizeof(_lib.PoseInformation) == 8 * (36 + 36 + 6) + 8 + 16 + 8
    assert (_lib.COV_LAPLACE, _lib.COV_SANDWICH, _lib.COV_INDEFINITE, pc.INDEFINITE) == (0, 1, 1, 1)


@pytest.mark.parametrize("kappa", (1.0 + 1e-9, 10.0, 1e3, 1e6))
def test_host_algebra_is_numpys(mods, kappa):
    _, _, ndt = mods
    rng = np.random.default_rng(int(kappa) + 41)
    worst = dict(laplace=0.0, sandwich=0.0, invariance=0.0, eig=0.0)
    for _ in range(40):
        A, B, g, n = random_case(rng, kappa)
        for method, scale in (("laplace", 2.5), ("sandwich", 1.0)):
            cov, lo, hi, flag = ndt.host_pose_covariance(A, B, g, n, method, scale)
            want, wlo, whi, wflag = pc.covariance(A, B, g, n, method, scale)
            assert not flag and wflag == 0
            assert np.array_equal(cov, cov.T)
            worst[method] = max(worst[method], rel_fro(cov, want))
            worst["eig"] = max(worst["eig"], abs(lo - wlo) / wlo, abs(hi - whi) / whi)
        # the sandwich does not move when the objective is scaled: A -> cA, B -> c^2 B, g -> c g
        base = ndt.host_pose_covariance(A, B, g, n, "sandwich")[0]
        for c in (1e-3, 7.0, 1e4):
            worst["invariance"] = max(worst["invariance"], rel_fro(ndt.host_pose_covariance(c * A, c * c * B, c * g, n, "sandwich")[0], base))
        # ... and Laplace is linear in its scale, and ignores B and g
        assert rel_fro(ndt.host_pose_covariance(A, 0 * B, 0 * g, n, "laplace", 5.0)[0],
                       2 * ndt.host_pose_covariance(A, B, g, n, "laplace", 2.5)[0]) <= 1e-15
        assert np.array_equal(ndt.host_pose_covariance(A, B, g, n, "sandwich", 1.0)[0], ndt.host_pose_covariance(A, B, g, n, "sandwich", -3.0)[0])
    print("kappa %.3g: worst relative Frobenius error %r" % (kappa, worst))
    assert worst["laplace"] <= BOUND and worst["sandwich"] <= BOUND and worst["invariance"] <= BOUND
    assert worst["eig"] <= BOUND


def test_the_indefinite_flag(mods):
    _, _, ndt = mods
    rng = np.random.default_rng(5)
    A, B, g, _ = random_case(rng, 100.0)

    def flagged(A, n):
        out = []
        for method in ("laplace", "sandwich"):
            cov, lo, hi, flag = ndt.host_pose_covariance(A, B, g, n, method)
            assert np.isnan(cov).all() == flag and (flag or np.isfinite(cov).all()), (method, n)
            assert pc.covariance(A, B, g, n, method)[3] == int(flag)
            out.append(flag)
        assert out[0] == out[1]
        return out[0], lo, hi

    assert flagged(A, 5)[0] and not flagged(A, 6)[0]               # n_found 5 | 6
    assert flagged(A, 0)[0]
    lam, V = np.linalg.eigh(A)
    zero = (V * np.r_[0.0, lam[1:]]) @ V.T                          # a zero eigenvalue (to rounding: far below 1e-12 max)
    f, lo, hi = flagged((zero + zero.T) / 2, 50)
    assert f and abs(lo) <= 1e-12 * hi
    neg = (V * np.r_[-lam[0], lam[1:]]) @ V.T                       # a negative one
    f, lo, hi = flagged((neg + neg.T) / 2, 50)
    assert f and lo < 0 < hi
    f, lo, hi = flagged(np.zeros((6, 6)), 50)                       # A = 0: max eigenvalue <= 0
    assert f and lo == 0.0 and hi == 0.0
    assert flagged(-A, 50)[0]                                       # negative definite
    just = (V * np.r_[2e-12 * lam[-1], lam[1:]]) @ V.T              # just above the 1e-12 threshold: not flagged
    assert not flagged((just + just.T) / 2, 50)[0]
    bad = A.copy()
    bad[2, 3] = bad[3, 2] = np.nan
    assert flagged(bad, 50)[0]


def test_refusals_before_device_work_write_nothing(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    INV = _lib.NDT_ERR_INVALID
    T = np.ascontiguousarray(np.eye(4, dtype=np.float32).reshape(16))
    cov = np.full(72, SENTINEL)
    info = (_lib.PoseInformation * 2)()
    info[0].n_found = 99
    for call in (L.ndt_pose_covariance, L.ndt_pairs_pose_covariances):
        assert call(None, fp(T), 1, 1.0, dp(cov), None) == INV                         # NULL handle
        assert call(g._h, fp(T), 1, 1.0, None, None) == INV                            # NULL cov
        for method in (-1, 2, 7):
            assert call(g._h, fp(T), method, 1.0, dp(cov), C.cast(info, C.c_void_p)) == INV, method
        for scale in (0.0, -1.0, float("nan"), float("inf")):
            assert call(g._h, fp(T), 0, scale, dp(cov), C.cast(info, C.c_void_p)) == INV, scale   # Laplace needs a scale
    a = C.c_size_t(99)
    assert L.ndt_diag_pose_covariance(None, C.byref(a), C.byref(a)) == INV
    assert L.ndt_diag_pose_covariance(g._h, None, C.byref(a)) == INV
    assert L.ndt_diag_pose_covariance(g._h, C.byref(a), None) == INV
    # the host function: NULL arguments, an unknown method, a bad Laplace scale
    A = np.eye(6).reshape(36)
    v = np.zeros(6)
    assert L.ndt_host_pose_covariance(None, dp(A), dp(v), 9, 1, 1.0, dp(cov), None, None, None) == INV
    assert L.ndt_host_pose_covariance(dp(A), None, dp(v), 9, 1, 1.0, dp(cov), None, None, None) == INV
    assert L.ndt_host_pose_covariance(dp(A), dp(A), None, 9, 1, 1.0, dp(cov), None, None, None) == INV
    assert L.ndt_host_pose_covariance(dp(A), dp(A), dp(v), 9, 1, 1.0, None, None, None, None) == INV
    assert L.ndt_host_pose_covariance(dp(A), dp(A), dp(v), 9, 2, 1.0, dp(cov), None, None, None) == INV
    assert L.ndt_host_pose_covariance(dp(A), dp(A), dp(v), 9, 0, 0.0, dp(cov), None, None, None) == INV
    with pytest.raises(ValueError):
        g.poseCovariance(method="fisher")
    # a handle with an all-reduce hook
    g.setAllreduce(lambda buf, n, on_device: 0)
    assert L.ndt_pose_covariance(g._h, fp(T), 1, 1.0, dp(cov), None) == INV
    assert L.ndt_pairs_pose_covariances(g._h, fp(T), 1, 1.0, dp(cov), None) == INV
    assert list(cov) == [SENTINEL] * 72 and info[0].n_found == 99 and a.value == 99
    # (the sandwich ignores its scale: with valid arguments the host function works, NULL outputs allowed)
    assert L.ndt_host_pose_covariance(dp(A), dp(A), dp(v), 9, 1, float("nan"), dp(cov), None, None, None) == _lib.NDT_OK
    assert np.array_equal(cov[:36].reshape(6, 6), np.eye(6))


def test_a_valid_call_needs_a_device_then_inputs(mods):
    L, _lib, ndt = mods
    if L.ndt_device_count() >= 1:
        return  # (with a GPU the same calls are tests/test_gpu_pose_cov.py's business)
    g = ndt.NormalDistributionsTransform()
    cov = np.full(36, SENTINEL)
    assert L.ndt_pose_covariance(g._h, None, 1, 1.0, dp(cov), None) == _lib.NDT_ERR_NO_DEVICE
    assert L.ndt_pairs_pose_covariances(g._h, None, 0, 2.0, dp(cov), None) == _lib.NDT_ERR_NO_DEVICE
    assert list(cov) == [SENTINEL] * 36 and g.poseCovarianceLaunches() == (0, 0)
    with pytest.raises(ndt.NdtError) as e:
        g.poseCovariance()
    assert e.value.status == _lib.NDT_ERR_NO_DEVICE
