"""CPU: tests/nvtl_cases.py, the numpy reference of the nearest-voxel transformation likelihood, pinned before anything trusts
it.  Its neighbour terms, reduced the way calculateScore reduces them, must be the oracle's calculate_score (rel 1e-11, the
figure the suite holds calculateScore to) under all four search methods; then hand cases of the NVTL reduction itself."""
import numpy as np
import pytest

import nvtl_cases as nc
import score_poses_cases as spc

F = np.float32


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


@pytest.mark.parametrize("method", nc.METHODS)
def test_terms_reduce_to_the_oracles_calculate_score(po, pair, golden, method):
    t, s = pair
    o = po.OracleNDT(num_threads=8, search_method=getattr(po, method))
    o.set_target(t)
    o.set_source(s[:10])
    ref = nc.Grid.of_oracle(o, method, t)
    sub = s[::7]
    for name, T in (("identity", np.eye(4, dtype=F)), ("golden", spc.golden_T(golden))):
        m = spc.moved(po, sub, T)
        q, has = ref.terms(m)
        got, want = nc.score(q, has, ref.d1, ref.d2, ref.d3), o.calculate_score(m)
        L, value, n_found = nc.nvtl(q, has, ref.d1, ref.d2)
        several = int((has.sum(axis=1) > 1).sum())
        print("%s %s: score %.17g oracle %.17g rel %.3g; nvtl %.6f found %d/%d, %d with several neighbours"
              % (method, name, got, want, abs(got - want) / abs(want), value, n_found, len(sub), several))
        assert got == pytest.approx(want, rel=1e-11)
        assert 0 < n_found <= len(sub) and 0.0 < value <= -ref.d1
        if method != "DIRECT1":
            assert several > 0                                       # max and mean differ somewhere
        if method in ("DIRECT1", "DIRECT7"):
            assert n_found < len(sub)                                # the divisor is not the scan's size
        # for d2 > 0 the max-of-exp wording and the exp-of-min definition are the same number
        assert ref.d2 > 0 and np.array_equal(nc.nvtl_max_form(q, has, ref.d1, ref.d2), L)
        assert np.array_equal(L >= 0, has.any(axis=1)) and np.all(L[~has.any(axis=1)] == -1.0)
        lists = ref.q_lists(m[:50])
        assert [len(x) for x in lists] == list(has[:50].sum(axis=1))
    # a pose a kilometre away: nothing found, 0.0, no NaN
    L, value, n_found = ref.nvtl(spc.moved(po, sub, spc.make_T([1000.0, 0, 0], [0, 0, 0])))
    assert (value, n_found) == (0.0, 0) and np.all(L == -1.0)


GAUSS = (-2.0, 0.5, 0.25)   # d1 < 0 as the reference's constants are; d2 > 0


def hand_grid(voxels, div=(3, 1, 1)):
    """voxels: {i along x: (n, mean, icov)} in a box of `div` cells from the origin, resolution 1"""
    keys = sorted(voxels)
    return dict(idx=np.array(keys, dtype=np.int64), n=np.array([voxels[k][0] for k in keys]),
                mean=np.array([voxels[k][1] for k in keys], dtype=np.float64),
                icov=np.array([voxels[k][2] for k in keys], dtype=np.float64), min_b=np.zeros(3, np.int64), div_b=np.array(div))


def test_a_point_at_the_mean_of_its_only_voxel():
    g = nc.Grid(hand_grid({0: (6, [0.5, 0.5, 0.5], np.eye(3))}), GAUSS, "DIRECT7")
    L, value, n_found = g.nvtl(np.array([[0.5, 0.5, 0.5]], F))
    assert L[0] == -GAUSS[0] == value and n_found == 1


def test_the_smaller_q_of_two_neighbours_wins():
    vox = {0: (6, [0.5, 0.5, 0.5], np.eye(3)), 1: (9, [1.5, 0.5, 0.5], 4 * np.eye(3))}
    for method in ("DIRECT7", "DIRECT26"):
        g = nc.Grid(hand_grid(vox), GAUSS, method)
        p = np.array([[0.75, 0.5, 0.5], [1.25, 0.5, 0.5]], F)       # q against voxel 0 | voxel 1: 0.0625 | 2.25 and 0.5625 | 0.25
        q, has = g.terms(p)
        L, value, n_found = nc.nvtl(q, has, g.d1, g.d2)
        if method == "DIRECT7":
            assert sorted(q[0, has[0]]) == [0.0625, 2.25] and sorted(q[1, has[1]]) == [0.25, 0.5625]
            want = [2.0 * np.exp(-0.5 * 0.0625 / 2), 2.0 * np.exp(-0.5 * 0.25 / 2)]
        else:   # the 26 cells around the point's own: only the other voxel
            assert list(q[0, has[0]]) == [2.25] and list(q[1, has[1]]) == [0.5625]
            want = [2.0 * np.exp(-0.5 * 2.25 / 2), 2.0 * np.exp(-0.5 * 0.5625 / 2)]
        assert list(L) == want and n_found == 2 and value == (want[0] + want[1]) / 2
    g = nc.Grid(hand_grid(vox), GAUSS, "DIRECT1")
    assert list(g.q_lists(np.array([[0.75, 0.5, 0.5]], F))[0]) == [0.0625]


def test_a_nan_q_never_wins():
    nan = np.full((3, 3), np.nan)
    g = nc.Grid(hand_grid({0: (6, [0.5, 0.5, 0.5], nan), 1: (6, [1.5, 0.5, 0.5], np.eye(3))}), GAUSS, "DIRECT7")
    L, value, n_found = g.nvtl(np.array([[0.75, 0.5, 0.5]], F))      # its own voxel gives NaN (first in order), the next 0.5625
    assert L[0] == 2.0 * np.exp(-0.5 * 0.5625 / 2) and n_found == 1
    g = nc.Grid(hand_grid({0: (6, [0.5, 0.5, 0.5], nan)}), GAUSS, "DIRECT7")
    L, value, n_found = g.nvtl(np.array([[0.75, 0.5, 0.5]], F))      # only NaN: found, q_min stays +inf, L = -d1 exp(-inf) = 0
    assert L[0] == 0.0 and n_found == 1 and value == 0.0


def test_no_neighbour_is_minus_one_and_not_counted():
    vox = {0: (6, [0.5, 0.5, 0.5], np.eye(3)), 2: (5, [2.5, 0.5, 0.5], np.eye(3))}   # the second is under min_points_per_voxel
    g = nc.Grid(hand_grid(vox), GAUSS, "DIRECT1")
    p = np.array([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [1.5, 0.5, 0.5], [7.0, 0.5, 0.5], [np.nan, 0, 0], [0.5, np.inf, 0.5], [1e30, 0, 0]], F)
    L, value, n_found = g.nvtl(p)
    assert list(L) == [2.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0] and n_found == 1 and value == 2.0
    assert nc.nvtl(*g.terms(p[1:]), g.d1, g.d2)[1:] == (0.0, 0)       # nobody found: 0.0, never NaN
    assert nc.nvtl(*g.terms(p[:0]), g.d1, g.d2)[1:] == (0.0, 0)       # an empty cloud
    empty = nc.Grid(hand_grid({}), GAUSS, "DIRECT7")
    assert empty.nvtl(p)[1:] == (0.0, 0)                              # an empty grid


def test_kdtree_takes_the_centroids_within_the_radius():
    vox = {0: (6, [0.5, 0.5, 0.5], np.eye(3)), 2: (6, [2.5, 0.5, 0.5], np.eye(3))}
    cen = (np.array([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5]], F), np.array([0, 2], np.int64))
    g = nc.Grid(hand_grid(vox), GAUSS, "KDTREE", centroids=cen)
    # 1.25: 0.75 from the first centroid (inside the radius of 1), 1.25 from the second; 1.5: exactly 1 from both -- strict <
    q = g.q_lists(np.array([[1.25, 0.5, 0.5], [1.5, 0.5, 0.5], [2.0, 0.5, 0.5]], F))
    assert q[0] == [0.5625] and q[1] == [] and q[2] == [0.25]
