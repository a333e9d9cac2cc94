"""CPU: the numpy restatement of the outlier filters (tests/outlier_cases.py) pinned to cases worked out by hand, and the
margin every kept-set comparison of the GPU tests relies on: on each of their clouds the reference's own values keep clear of
the reference's threshold by more than 1e-9 (relative), or every value IS the threshold (all values equal: stddev 0)."""
import math

import numpy as np

import outlier_cases as oc

F = np.float32
NAN = float("nan")


def test_three_collinear_points():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]], F)
    assert np.array_equal(oc.knn_mean_distances(xyz, 1), [1, 1, 2])
    assert np.array_equal(oc.knn_mean_distances(xyz, 2), [2, 1.5, 2.5])
    assert np.array_equal(oc.knn_mean_distances(xyz, 3), [0, 0, 0])  # |F| <= mean_k
    assert np.array_equal(oc.radius_counts(xyz, 1.0), [1, 1, 0])
    assert np.array_equal(oc.radius_counts(xyz, 2.0), [1, 2, 1])
    r = oc.reference(xyz, **oc.stat(1, 1.0))
    mean, sd = 4 / 3, math.sqrt(((1 / 3) ** 2 * 2 + (2 / 3) ** 2) / 2)
    assert r["n_finite"] == 3 and r["n_valid"] == 3
    assert abs(r["mean"] - mean) < 1e-15 and abs(r["stddev"] - sd) < 1e-15 and abs(r["threshold"] - (mean + sd)) < 1e-15
    assert np.array_equal(r["keep"], [True, True, False])
    assert np.array_equal(oc.reference(xyz, **oc.stat(1, 1.0, True))["keep"], [False, False, True])


def test_a_duplicate_pair_and_a_far_point():
    xyz = np.array([[2, 2, 2], [2, 2, 2], [2, 2, 12]], F)
    assert np.array_equal(oc.knn_mean_distances(xyz, 1), [0, 0, 10])  # the duplicate is a neighbour at distance 0, by index
    assert np.array_equal(oc.knn_mean_distances(xyz, 2), [5, 5, 10])
    assert np.array_equal(oc.radius_counts(xyz, 0.5), [1, 1, 0])
    assert np.array_equal(oc.reference(xyz, **oc.rad(0.5, 1))["keep"], [True, True, False])
    assert np.array_equal(oc.reference(xyz, **oc.rad(0.5, 1, True))["keep"], [False, False, True])
    assert np.array_equal(oc.reference(xyz, **oc.rad(0.5, 0))["keep"], [True, True, True])


def test_lattice_in_closed_form():
    xyz, cls = oc.lattice(3), oc.lattice_class(3)
    assert np.array_equal(np.bincount(cls), [8, 12, 6, 1])
    assert np.array_equal(oc.radius_counts(xyz, 1.0), 3 + cls)       # neighbours at distance 1: corner 3, edge 4, face 5, centre 6
    assert np.array_equal(oc.knn_mean_distances(xyz, 3), np.ones(27))
    r2 = math.sqrt(2.0)
    want = np.array([(3 + 3 * r2) / 6, (4 + 2 * r2) / 6, (5 + r2) / 6, 1.0])[cls]
    got = oc.knn_mean_distances(xyz, 6)
    assert np.abs(got - want).max() < 4e-16 and got[13] == 1.0
    r = oc.reference(xyz, **oc.stat(3, 1.0))
    assert r["mean"] == 1.0 and r["stddev"] == 0.0 and r["threshold"] == 1.0 and r["keep"].all()
    assert not oc.reference(xyz, **oc.stat(3, 1.0, True))["keep"].any()


def test_rows_that_are_not_finite():
    xyz = np.array([[0, 0, 0], [NAN, 0, 0], [1, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [4, 0, 0]], F)
    v = oc.knn_mean_distances(xyz, 1)
    assert np.array_equal(np.isnan(v), [False, True, False, True, True, False]) and np.array_equal(v[[0, 2, 5]], [1, 1, 3])
    c = oc.radius_counts(xyz, 1.0)
    assert np.array_equal(np.isnan(c), np.isnan(v)) and np.array_equal(c[[0, 2, 5]], [1, 1, 0])
    for spec in (oc.stat(1, 5.0), oc.stat(1, 5.0, True), oc.rad(1.0, 0), oc.rad(1.0, 0, True)):
        r = oc.reference(xyz, **spec)
        assert r["n_finite"] == 3 and not r["keep"][[1, 3, 4]].any()      # never kept, in either sense
    assert oc.reference(xyz, **oc.rad(1.0, 0))["keep"].sum() == 3 and oc.reference(xyz, **oc.rad(1.0, 0, True))["keep"].sum() == 0


def test_mean_k_at_the_number_of_finite_points():
    xyz = oc.surface(6, 1)
    xyz[2] = NAN
    r = oc.reference(xyz, **oc.stat(5))                   # |F| = mean_k: nobody has mean_k other points
    assert (r["n_finite"], r["n_valid"], r["mean"], r["stddev"], r["threshold"]) == (5, 0, 0.0, 0.0, 0.0)
    assert np.array_equal(r["values"][[0, 1, 3, 4, 5]], np.zeros(5)) and math.isnan(r["values"][2])
    assert r["keep"].sum() == 5 and not oc.reference(xyz, **oc.stat(5, 1.0, True))["keep"].any()
    r = oc.reference(xyz, **oc.stat(4))                   # |F| = mean_k + 1: every other point is a neighbour
    assert r["n_valid"] == 5 and (r["values"][[0, 1, 3, 4, 5]] > 0).all() and r["stddev"] > 0


def test_sphere_rows_are_exact():
    xyz = oc.sphere_rows()
    assert np.array_equal(oc.radius_counts(xyz, 5.0)[[0, 6]], [5, 5])          # d2 == r2 counts
    assert np.array_equal(oc.radius_counts(xyz, oc.UP5)[[0, 6]], [5, 5])
    assert np.array_equal(oc.radius_counts(xyz, oc.DOWN5)[[0, 6]], [2, 2])     # one ulp below: the three on the sphere are out
    assert F(oc.UP5) * F(oc.UP5) > 25 > F(oc.DOWN5) * F(oc.DOWN5)


def test_values_keep_clear_of_the_threshold_on_every_gpu_cloud():
    n = 0
    for name, (xyz, specs) in oc.gpu_cases().items():
        for spec in specs:
            r = oc.reference_of(name, xyz, spec)
            v = r["values"][~np.isnan(r["values"])]
            if spec["method"] == oc.RADIUS:
                assert np.array_equal(v, np.round(v))      # integers: a count is on one side of an integer threshold or on it
            else:
                tie = len(v) > 0 and bool((v == r["threshold"]).all())
                assert tie or oc.threshold_margin(r) > 1e-9, (name, spec, oc.threshold_margin(r))
            assert np.array_equal(r["keep"], oc.keep_by(r["values"], r["threshold"], spec["method"], spec["negate"]))
            n += 1
    assert n > 100
    for j, xyz in enumerate(oc.ragged()):
        for spec in oc.RAGGED_SPECS:
            r = oc.reference(xyz, **spec)
            v = r["values"][~np.isnan(r["values"])]
            assert spec["method"] == oc.RADIUS or oc.threshold_margin(r) > 1e-9 or (len(v) > 0 and bool((v == r["threshold"]).all())), (j, spec)
    # what the names promise
    c = oc.gpu_cases()
    assert (oc.reference_of("surface", c["surface"][0], oc.rad(1e-5, 1))["values"] == 0).all()
    assert (oc.reference_of("surface", c["surface"][0], oc.rad(100.0, 2999))["values"] == 2999).all()
    assert oc.reference_of("every point identical", c["every point identical"][0], oc.stat(8))["stddev"] == 0.0
