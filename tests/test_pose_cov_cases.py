"""CPU: tests/pose_cov_cases.py, the numpy reference of the pose covariance, pinned before anything trusts it.

  sum of g_i   against the oracle's computeDerivatives gradient on every 7th source point of the bundled pair, at the identity
               and at the golden pose, under all four search methods.  The oracle's gradient is rounded to f32 per neighbour
               (updateDerivatives), so the two differ by f32 rounding of each term: the difference of entry k is measured
               against S_g[k], the sum of the absolute values of the terms of that entry.  Worst measured: 7.7e-9 (an f32 half
               ulp is 6e-8; the roundings of thousands of terms partly cancel).  The test asserts ten times that, GRAD_BOUND.
  A            against -sym(oracle.hessian_f64), each entry within 1e-12 of the largest entry of A: the entries are sums of
               ~1e4 terms of both signs, and the reference adds them per neighbour slot, the oracle per point, so an entry
               moves by eps x (its terms' absolute sum), which the largest entry stands for.  Measured: 5.3e-14 at worst
               (entry by entry against itself the worst is 2.9e-11, in an entry that cancels to 1e-4 of the largest).
  hand cases   one point in one voxel against the closed form (B = g g^T exactly); a source with every point twice."""
import numpy as np
import pytest

import pose_cov_cases as pc
import score_poses_cases as spc

F = np.float32
GRAD_BOUND = 7.7e-8
GAUSS = (-2.0, 0.5, 0.25)


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


@pytest.mark.parametrize("method", pc.METHODS)
def test_gradient_and_hessian_are_the_oracles(po, built_lib, pair, golden, method):
    from toyslam_amd import ndt
    t, s = pair
    sub = s[::7]
    o = po.OracleNDT(num_threads=8, search_method=getattr(po, method))
    o.set_target(t)
    o.set_source(sub)
    ref = pc.Grid.of_oracle(o, method, t)
    for name, p in (("identity", np.zeros(6)), ("golden", ndt.host_matrix_to_pose(spc.golden_T(golden)))):
        T = po.pose_to_matrix(p)                                   # the oracle moves the source by T(p)
        I = ref.information(sub, spc.moved(po, sub, T), p)
        _, g, _, _ = o.eval(p)
        H = o.hessian_f64(p)
        A = -(H + H.T) / 2
        worst_g = float((np.abs(I["g"] - g) / I["S_g"]).max())
        worst_A = float(np.abs(I["A"] - A).max() / np.abs(A).max())
        print("%s %s: found %d/%d  gradient worst |diff| / S %.3g  A worst |diff| / max|A| %.3g  min eig %.6g"
              % (method, name, I["n_found"], len(sub), worst_g, worst_A, np.linalg.eigvalsh(A).min()))
        assert 0 < I["n_found"] <= len(sub)
        assert worst_g <= GRAD_BOUND
        assert worst_A <= 1e-12
        assert np.array_equal(I["B"], I["B"].T) and np.all(np.diag(I["B"]) > 0)
        assert np.all(np.abs(I["B"]) <= I["S_B"] * (1 + 1e-15)) and np.all(np.abs(I["g"]) <= I["S_g"])


def test_minus_the_hessian_is_positive_definite_at_the_golden_pose(po, built_lib, pair, golden):
    """the sign of A: all six eigenvalues of -H are positive where the pair registers"""
    from toyslam_amd import ndt
    t, s = pair
    o = po.OracleNDT(num_threads=8)
    o.set_target(t)
    o.set_source(s)
    H = o.hessian_f64(ndt.host_matrix_to_pose(spc.golden_T(golden)))
    lam = np.linalg.eigvalsh(-(H + H.T) / 2)
    print("eigenvalues of -H at the golden pose:", " ".join("%.6g" % x for x in lam))
    assert np.all(lam > 0)


def hand_grid(voxels, div=(3, 1, 1)):
    keys = sorted(voxels)
    return dict(idx=np.array(keys, dtype=np.int64), n=np.array([voxels[k][0] for k in keys]),
                mean=np.array([voxels[k][1] for k in keys], dtype=np.float64),
                icov=np.array([voxels[k][2] for k in keys], dtype=np.float64), min_b=np.zeros(3, np.int64), div_b=np.array(div))


def test_one_point_in_one_voxel_is_the_closed_form():
    Cm = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.25], [0.5, 0.25, 2.0]])
    mean = np.array([0.5, 0.5, 0.5])
    g = pc.Grid(hand_grid({0: (6, mean, Cm)}), GAUSS, "DIRECT7")
    x = np.array([[0.75, 0.25, 0.625]], F)
    I = g.information(x, x, np.zeros(6))                          # the identity: the moved point is the point
    xt = x[0].astype(np.float64) - mean
    Cx = Cm @ xt
    w = GAUSS[0] * GAUSS[1] * np.exp(-GAUSS[1] * (xt @ Cx) / 2)
    px, py, pz = x[0].astype(np.float64)
    # at zero angles the angle columns of J are the cross products e_k x x: d(Rx)/d(roll, pitch, yaw)
    want = w * np.array([Cx[0], Cx[1], Cx[2], -pz * Cx[1] + py * Cx[2], pz * Cx[0] - px * Cx[2], -py * Cx[0] + px * Cx[1]])
    assert I["n_found"] == 1 and np.allclose(I["g"], want, rtol=1e-15, atol=0)
    assert np.array_equal(I["B"], np.outer(I["g"], I["g"]))        # one term: exactly g g^T
    assert np.array_equal(pc.centred(I["B"], I["g"], 1), np.zeros((6, 6)))
    # A of one point: -w (-d2 t t^T + J^T C J) with t = J^T Cx (the second-derivative vectors vanish against Cx only in sum)
    assert np.allclose(I["A"], I["A"].T, rtol=0, atol=0)
    cov, lo, hi, flags = pc.covariance(I["A"], I["B"], I["g"], I["n_found"], "sandwich")
    assert flags == pc.INDEFINITE and np.isnan(cov).all()          # one point: n_found < 6
    # a point outside the box, a non-finite one, a voxel below min_points_per_voxel: nothing found, everything zero
    for bad, vox in ((np.array([[7.0, 0.5, 0.5]], F), {0: (6, mean, Cm)}), (np.array([[np.nan, 0.5, 0.5]], F), {0: (6, mean, Cm)}),
                     (x, {0: (5, mean, Cm)})):
        J = pc.Grid(hand_grid(vox), GAUSS, "DIRECT7").information(bad, bad, np.zeros(6))
        assert J["n_found"] == 0 and not J["B"].any() and not J["g"].any() and not J["A"].any()
    # a neighbour whose weight is out of range is skipped: d2 = 3 gives w = 3 exp(..) > 1 near the mean
    K = pc.Grid(hand_grid({0: (6, mean, Cm)}), (-2.0, 3.0, 0.25), "DIRECT7").information(x, x, np.zeros(6))
    assert K["n_found"] == 0 and not K["B"].any()


def test_every_point_twice_doubles_the_sums(po, built_lib, pair, golden):
    from toyslam_amd import ndt
    t, s = pair
    sub = s[::16]
    o = po.OracleNDT(num_threads=8)
    o.set_target(t)
    o.set_source(s[:10])
    ref = pc.Grid.of_oracle(o, "DIRECT7", t)
    T = spc.golden_T(golden)
    p = ndt.host_matrix_to_pose(T)
    twice = np.repeat(sub, 2, axis=0)
    one = ref.information(sub, spc.moved(po, sub, T), p)
    two = ref.information(twice, spc.moved(po, twice, T), p)
    assert two["n_found"] == 2 * one["n_found"] > 12
    for k in ("A", "B", "g"):
        assert np.abs(two[k] - 2 * one[k]).max() <= 1e-12 * np.abs(one[k]).max(), k
    # ... and halves the sandwich covariance, while the Laplace one follows 1 / A
    c1 = pc.covariance(one["A"], one["B"], one["g"], one["n_found"], "sandwich")[0]
    c2 = pc.covariance(two["A"], two["B"], two["g"], two["n_found"], "sandwich")[0]
    assert np.linalg.norm(c2 - c1 / 2) <= 1e-10 * np.linalg.norm(c1)
    l1 = pc.covariance(one["A"], one["B"], one["g"], one["n_found"], "laplace", 3.0)[0]
    l2 = pc.covariance(two["A"], two["B"], two["g"], two["n_found"], "laplace", 3.0)[0]
    assert np.linalg.norm(l2 - l1 / 2) <= 1e-10 * np.linalg.norm(l1)
