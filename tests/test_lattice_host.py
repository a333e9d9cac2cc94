"""CPU: the lattice of a bounding box (lattice_geometry, ndt_kernels.hpp: every cell index in the project comes from it) and
the dense-or-sparse rule of the voxel index (wants_sparse_index), through ndt_host_lattice -- against the live oracle's
VoxelGridCovariance and the reference's own overflow rule (voxel_grid_covariance_omp_impl.hpp:75-103).  No GPU is used."""
import itertools

import numpy as np
import pytest

from oracle import pyoracle as po

f32 = np.float32
INT32_MAX = 2 ** 31 - 1
LEAVES = [f32(0.1), f32(0.3), f32(1.0) / f32(3.0), f32(1.0), f32(2.0)]


@pytest.fixture(scope="module")
def ndt(built_lib):
    from toyslam_amd import ndt as m
    return m


def near(v, ulps):
    """v moved by that many f32 ulps (0: v itself)"""
    v = f32(v)
    for _ in range(abs(ulps)):
        v = np.nextafter(v, f32(np.inf if ulps > 0 else -np.inf))
    return v


def oracle_lattice(o, mn, mx):
    """the lattice the oracle's VoxelGridCovariance lays over the two corners (one point is enough for a voxel)"""
    assert o.set_target(np.array([mn, mx], dtype=f32)) == 0
    g = o.grid()
    return g["min_b"], g["max_b"], g["div_b"]


def check_against_oracle(ndt, o, leaf, mn, mx):
    mn, mx = np.asarray(mn, dtype=f32), np.asarray(mx, dtype=f32)
    got = ndt.host_lattice(leaf, mn, mx)
    ref = oracle_lattice(o, mn, mx)
    where = (float(leaf), mn.tolist(), mx.tolist())
    assert got["status"] == 0, where
    for k, r in zip(("min_b", "max_b", "div_b"), ref):
        assert np.array_equal(got[k], r), (k, where)
    assert got["n_cells"] == int(np.prod(ref[2].astype(np.int64))), where


@pytest.mark.parametrize("leaf", LEAVES, ids=lambda v: "%.3g" % v)
def test_lattice_at_cell_borders_equals_the_oracle(ndt, leaf):
    """corners at k * leaf and one f32 ulp either side, k negative, zero and positive, a different pair of cells on every
    axis (the third axis: both corners around the same border)"""
    o = po.OracleNDT(resolution=float(leaf), min_points_per_voxel=1)
    ks = (-37, -1, 0, 1, 52)
    n = 0
    for (k_lo, k_hi), (u_lo, u_hi) in itertools.product(itertools.combinations_with_replacement(ks, 2),
                                                        itertools.product((-1, 0, 1), repeat=2)):
        if k_lo == k_hi and u_lo > u_hi:
            continue
        mn = [near(f32(k_lo) * leaf, u_lo), near(f32(k_lo - 1) * leaf, u_lo), near(f32(k_lo) * leaf, min(u_lo, u_hi))]
        mx = [near(f32(k_hi) * leaf, u_hi), near(f32(k_hi + 2) * leaf, u_hi), near(f32(k_lo) * leaf, max(u_lo, u_hi))]
        check_against_oracle(ndt, o, leaf, mn, mx)
        n += 1
    assert n == 15 * 9 - 5 * 3


def test_lattice_of_plain_boxes_equals_the_oracle(ndt):
    boxes = {
        "one cell": ([0.2, 0.2, 0.2], [0.7, 0.7, 0.7]),
        "a kilometre out": ([1000.3, -1020.9, 998.2], [1031.6, -1000.1, 1003.4]),
        "100 km out": ([100000.25, -100000.5, 99990.1], [100020.7, -99980.2, 100001.9]),
        "negative only": ([-50.3, -20.1, -5.5], [-10.2, -0.4, -0.01]),
        "degenerate": ([1.5, -2.5, 0.0], [1.5, -2.5, 0.0]),
    }
    for leaf in LEAVES:
        o = po.OracleNDT(resolution=float(leaf), min_points_per_voxel=1)
        for mn, mx in boxes.values():
            check_against_oracle(ndt, o, leaf, mn, mx)
    one = ndt.host_lattice(1.0, *boxes["one cell"])
    assert one["div_b"].tolist() == [1, 1, 1] and one["n_cells"] == 1
    flat = ndt.host_lattice(0.1, *boxes["degenerate"])
    assert flat["div_b"].tolist() == [1, 1, 1] and np.array_equal(flat["min_b"], flat["max_b"])


def reference_overflows(leaf, mn, mx):
    """voxel_grid_covariance_omp_impl.hpp:75-84, restated: dx * dy * dz > INT32_MAX in int64, d = int64((max - min) * inv) + 1 in f32"""
    inv = f32(1.0) / f32(leaf)
    d = [int(f32(f32(b) - f32(a)) * inv) + 1 for a, b in zip(mn, mx)]
    return d[0] * d[1] * d[2] > INT32_MAX


def test_lattice_refuses_what_the_reference_refuses(ndt):
    """1290^3 = 2 146 689 000 cells are the last the reference's int indices hold, 1291^3 = 2 151 685 171 are too many.  The
    oracle is asked about the first box only -- the one it accepts; what is expected of the second comes from the
    reference's rule, restated above and by plain arithmetic."""
    from toyslam_amd import _lib
    assert 1290 ** 3 <= INT32_MAX < 1291 ** 3
    mn = [0.5, 0.5, 0.5]
    under, over = [1289.5] * 3, [1290.5] * 3
    assert not reference_overflows(1.0, mn, under) and reference_overflows(1.0, mn, over)
    got = ndt.host_lattice(1.0, mn, under)
    assert got["status"] == _lib.NDT_OK and got["div_b"].tolist() == [1290] * 3 and got["n_cells"] == 1290 ** 3
    check_against_oracle(ndt, po.OracleNDT(resolution=1.0, min_points_per_voxel=1), f32(1.0), mn, under)
    assert ndt.host_lattice(1.0, mn, over)["status"] == _lib.NDT_ERR_GRID_OVERFLOW
    # one long axis: the same rule
    assert ndt.host_lattice(1.0, [0.5, 0.5, 0.5], [2 ** 24, 100.5, 1.5])["status"] == _lib.NDT_ERR_GRID_OVERFLOW
    assert reference_overflows(1.0, [0.5, 0.5, 0.5], [2 ** 24, 100.5, 1.5])


def box_of_cells(n_cells):
    """a box at leaf 1.0 with exactly that many cells: corners in the middle of the first and the last cell of every axis"""
    for a in range(1, 5000):
        if n_cells % a:
            continue
        for b in range(a, 5000):
            c, r = divmod(n_cells // a, b)
            if r == 0 and c <= 2 ** 22:
                return [0.5, 0.5, 0.5], [a - 0.5, b - 0.5, c - 0.5]
    raise AssertionError("no box of %d cells" % n_cells)


def test_dense_or_sparse_voxel_index_rule(ndt):
    """automatic (mode 0): sparse above 2^25 cells, or above 64 cells per point + 2^22; modes 1 (dense) and 2 (sparse) override"""
    def sparse(n_cells, n_points, mode=0):
        got = ndt.host_lattice(1.0, *box_of_cells(n_cells), voxel_index=mode, n_points=n_points)
        assert got["status"] == 0 and got["n_cells"] == n_cells
        return got["sparse"]
    many = 10 ** 6  # points enough for the second term to stay out of the first one's way: 64e6 + 2^22 > 2^25 + 1
    assert not sparse(2 ** 25, many) and sparse(2 ** 25 + 1, many)
    for n in (0, 1000, 12345):
        edge = 64 * n + 2 ** 22
        assert edge < 2 ** 25
        assert not sparse(edge, n) and sparse(edge + 1, n)
        assert not sparse(edge + 1, n, mode=1) and sparse(edge, n, mode=2)
    assert not sparse(2 ** 25 + 1, many, mode=1) and sparse(1, many, mode=2)
