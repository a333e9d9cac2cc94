"""CPU: the new GICP entry points over resident clouds (gicp_set_input_*_cloud, gicp_align_pairs_clouds,
gicp_pairs_covariances, gicp_diag_pairs, gicp_diag_pairs_time) are exported, and the argument checks of
gicp_align_pairs_clouds that come before any device work hold with or without a GPU."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gicp_set_input_target_cloud", "gicp_set_input_source_cloud", "gicp_align_pairs_clouds", "gicp_pairs_covariances",
       "gicp_diag_pairs", "gicp_diag_pairs_time")
SENTINEL = 7.5


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, gicp
    return built_lib, _lib, gicp


def test_new_symbols_are_exported_and_listed(mods):
    L, _lib, _ = mods
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None


class Outputs:
    """n_pairs-sized outputs filled with sentinel values."""

    def __init__(self, n):
        n = max(n, 1)
        self.T = np.full((n, 16), SENTINEL, np.float32)
        self.conv, self.it, self.corr = (np.full(n, -77, np.int32) for _ in range(3))
        self.fit = np.full(n, SENTINEL, np.float64)

    def args(self):
        return (self.T.ctypes.data_as(C.POINTER(C.c_float)), self.conv.ctypes.data_as(C.POINTER(C.c_int)),
                self.it.ctypes.data_as(C.POINTER(C.c_int)), self.corr.ctypes.data_as(C.POINTER(C.c_int)),
                self.fit.ctypes.data_as(C.POINTER(C.c_double)))

    def untouched(self):
        return bool(np.all(self.T == SENTINEL) and np.all(self.conv == -77) and np.all(self.it == -77) and
                    np.all(self.corr == -77) and np.all(self.fit == SENTINEL))


def call(L, h, clouds, n_clouds, pairs, n_pairs, out):
    pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
    return L.gicp_align_pairs_clouds(h, clouds, n_clouds, None if pr is None else pr.ctypes.data_as(C.POINTER(C.c_int)), n_pairs,
                                     None, 1.0, *out.args())


def test_invalid_arguments_are_refused_before_any_device_work(mods):
    L, _lib, gicp = mods
    g = gicp.GeneralizedIterativeClosestPoint()
    fake = (C.c_void_p * 2)(None, None)   # (never dereferenced: each call below is refused for another reason first)
    cases = {
        "null handle": (None, fake, 2, [0, 1], 1),
        "null clouds": (g._h, None, 2, [0, 1], 1),
        "null pairs": (g._h, fake, 2, None, 1),
        "65535": (g._h, fake, 2, np.zeros(2 * 65536, np.int32), 65536),
    }
    for what, (h, cl, nc, pr, npairs) in cases.items():
        out = Outputs(npairs)
        assert call(L, h, cl, nc, pr, npairs, out) == _lib.NDT_ERR_INVALID, what
        assert what in L.ndt_last_error().decode(), (what, L.ndt_last_error())
        assert out.untouched(), what
    # a NULL entry and an index beyond the clouds are refused here too (the device tests repeat them with real clouds)
    out = Outputs(1)
    assert call(L, g._h, fake, 2, [0, 1], 1, out) == _lib.NDT_ERR_INVALID and out.untouched()


def test_no_pairs_is_ok_without_a_device(mods):
    L, _lib, gicp = mods
    g = gicp.GeneralizedIterativeClosestPoint()
    out = Outputs(0)
    assert call(L, g._h, None, 0, None, 0, out) == _lib.NDT_OK and out.untouched()
    r = g.alignPairsClouds([])
    assert r["T"].shape == (0, 4, 4) and len(r["converged"]) == len(r["fitness"]) == 0
    assert g.diagPairs() == dict(index_builds=0, knn_launches=0, knn_blocks=0)


def test_pairs_covariances_before_any_pairs_call(mods):
    L, _lib, gicp = mods
    g = gicp.GeneralizedIterativeClosestPoint()
    cov = np.zeros(9)
    assert L.gicp_pairs_covariances(g._h, 0, cov.ctypes.data_as(C.POINTER(C.c_double))) == _lib.NDT_ERR_NO_INPUT
    n = C.c_size_t(0)
    assert L.gicp_diag_pairs(g._h, C.byref(n), C.byref(n), C.byref(n)) == _lib.NDT_ERR_NO_INPUT
    with pytest.raises(_lib.NdtError) as e:
        g.pairsCovariances(0)
    assert e.value.status == _lib.NDT_ERR_NO_INPUT
