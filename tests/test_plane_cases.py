"""CPU: tests/plane_cases.py, the numpy restatement of the plane definitions (include/ndt_mi355.h), pinned to hand cases; and
for every fixture of the GPU tests the clearances the exact comparisons there rely on: under every hypothesis no point's
| |s| - T | is below 1e-9 m (at 100 km an ulp of a coordinate's f64 product is 1.5e-11 m: about 70 ulps), no valid or rejected
hypothesis lies within 1e-9 of cos_eps, none within a factor 2 of the degeneracy bound.  A fixture that does not keep them is
changed, not the rule."""
import math

import numpy as np
import pytest

import plane_cases as pc

F = np.float32


def test_splitmix64_first_outputs_for_seed_0():
    state, got = 0, []
    for _ in range(4):
        state = (state + pc.GOLDEN) & pc.M64
        got.append(pc.finalise(state))
    assert tuple(got) == pc.SPLITMIX64_SEED0
    # the header's splitmix64(x) finalises x + golden: x = 0, golden, 2 golden are the generator's first three states
    assert [pc.splitmix64((k * pc.GOLDEN) & pc.M64) for k in range(3)] == list(pc.SPLITMIX64_SEED0[:3])
    assert pc.sample(0, 0, 1000) == [pc.SPLITMIX64_SEED0[0] % 1000, pc.splitmix64(1) % 1000, pc.splitmix64(2) % 1000]
    assert pc.sample(5, 2, 77) == [pc.splitmix64(11 + j) % 77 for j in range(3)]
    assert pc.sample(pc.M64, 1, 10) == [pc.splitmix64(2 + j) % 10 for j in range(3)]      # u64 wrap-around


def test_three_points_on_z_1():
    for sp in (pc.spec(0.1, 1), pc.spec(0.1, 1, axis=(0, 0, 2), eps=0.1)):
        for tri in (((0, 0, 1), (1, 0, 1), (0, 1, 1)), ((0, 0, 1), (0, 1, 1), (1, 0, 1))):   # either winding
            co, st = pc.model(sp, *tri)
            assert st == pc.VALID and co.tolist() == [0.0, 0.0, 1.0, -1.0]
    assert pc.distances(np.array([0.0, 0.0, 1.0, -1.0]), [[5, 5, 1.25]]).tolist() == [0.25]


def test_degenerate_triples():
    sp = pc.spec(0.1, 1)
    for tri in (((0, 0, 0), (1, 1, 1), (2, 2, 2)), ((0, 0, 0), (1, 0, 0), (1 + 1e-5, 1e-5, 0))):   # collinear, nearly collinear
        co, st = pc.model(sp, *tri)
        assert st == pc.DEGENERATE and not co.any()
    co, st = pc.model(sp, (0, 0, 0), (1, 0, 0), (0, 1, 0), same=True)                            # a repeated index
    assert st == pc.DEGENERATE and not co.any()
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            tri = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
            tri[k][k] = bad
            co, st = pc.model(sp, *tri)
            assert st == pc.DEGENERATE and not co.any()
    # just inside the bound: |u x v|^2 = sin^2 |u|^2 |v|^2 with sin^2 = 4e-8
    co, st = pc.model(sp, (0, 0, 0), (1, 0, 0), (1, 2e-4, 0))
    assert st == pc.VALID


def test_the_angle_test_rejects_11_degrees_under_10():
    for deg, want in ((11.0, pc.REJECTED), (9.0, pc.VALID)):
        t = math.tan(math.radians(deg))
        sp = pc.spec(0.1, 1, axis=(0, 0, 1), eps=math.radians(10.0))
        co, st = pc.model(sp, (0, 0, 0), (1, 0, t), (0, 1, 0))
        assert st == want and co[2] > 0 and abs(math.degrees(math.acos(co[2])) - deg) < 1e-5
        co2, st2 = pc.model(sp, (0, 0, 0), (0, 1, 0), (1, 0, t))          # the other winding: flipped towards the axis
        assert st2 == want and np.array_equal(co2, co)
    co, st = pc.model(pc.spec(0.1, 1, axis=(0, 0, -3), eps=0.2), (0, 0, 1), (1, 0, 1), (0, 1, 1))
    assert st == pc.VALID and co.tolist() == [0.0, 0.0, -1.0, 1.0]


def test_the_orientation_rule_on_each_axis():
    sp = pc.spec(0.1, 1)
    for tri, want in ((((0, 0, 0), (1, 0, 0), (0, 1, 0)), [0, 0, 1]), (((0, 0, 0), (0, 1, 0), (1, 0, 0)), [0, 0, 1]),       # z decides
                      (((0, 0, 0), (1, 0, 0), (0, 0, 1)), [0, 1, 0]), (((0, 0, 0), (0, 0, 1), (1, 0, 0)), [0, 1, 0]),       # z == 0: y
                      (((0, 0, 0), (0, 1, 0), (0, 0, 1)), [1, 0, 0]), (((0, 0, 0), (0, 0, 1), (0, 1, 0)), [1, 0, 0])):      # z == y == 0: x
        co, st = pc.model(sp, *tri)
        assert st == pc.VALID and co[:3].tolist() == want
    co, st = pc.model(sp, (0, 0, 0), (1, 0, 1), (0, 1, 0))       # n = (-1, 0, 1) / sqrt 2 or its negative: z positive
    assert co[2] > 0 and co[0] < 0


def test_inliers_counts_and_the_choice():
    T = float(F(0.1))
    s = np.array([-T, T, np.nextafter(T, 1), np.nextafter(-T, -1), np.nan, np.inf, -np.inf, 0.0])
    assert pc.inlier(s, T).tolist() == [True, True, False, False, False, False, False, True]
    # two parallel planes with four points each: equal counts, the lowest h wins
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]], F)
    r = pc.segment(xyz, pc.spec(0.1, 3), triples=[[4, 5, 6], [0, 1, 2], [0, 0, 1]])
    assert r["counts"].tolist() == [4, 4, 0] and r["states"].tolist() == [0, 0, 1] and r["best"] == 0 and r["best_count"] == 4
    assert r["inliers"].tolist() == [False] * 4 + [True] * 4 and r["others"].tolist() == [True] * 4 + [False] * 4
    # no valid hypothesis; fewer than three points
    r = pc.segment(xyz, pc.spec(0.1, 1), triples=[[0, 0, 1]])
    assert not r["found"] and r["best"] == -1 and not r["coeff"].any() and not r["inliers"].any() and r["others"].all()
    assert np.isinf(r["keys"]).all()
    for n in (0, 1, 2):
        r = pc.segment(xyz[:n], pc.spec(0.1, 5, seed=1))
        assert not r["found"] and r["n_degenerate"] == 5 and r["others"].sum() == n


def test_refinement_restated():
    xyz, sp = pc.refine_cases()["refine 4099"]
    r = pc.reference_of("refine 4099")
    assert r["found"] and r["refined"] and r["n_inliers"] >= r["best_count"]
    truth = np.array([-0.02, 0.015, 1.0])
    truth /= np.linalg.norm(truth)
    assert np.abs(r["coeff"][:3] - truth).max() < 2e-3 < np.abs(r["unrefined"][:3] - truth).max() * 10
    # rank 1: refused, the unrefined plane stays
    line = np.array([[k, 2 * k, 3 * k] for k in range(10)], np.float64)
    taken, coeff, lam, sums = pc.fit(sp, line, line[0])
    assert not taken
    taken, coeff, lam, sums = pc.fit(sp, line[:2], line[0])
    assert not taken


ALL = dict(pc.gpu_cases())
ALL.update(pc.refine_cases())


@pytest.mark.parametrize("name", sorted(ALL))
def test_fixture_clearances(name):
    xyz, sp = ALL[name]
    c = pc.clearances(xyz, sp)
    r = pc.reference_of(name)
    print(name, "clearances", c, "best", r["best"], r["best_count"], "of", len(xyz), "degenerate", r["n_degenerate"], "rejected", r["n_rejected"])
    assert c["distance"] >= 1e-9, "a point within 1e-9 m of a threshold: change the fixture"
    assert c["angle"] >= 1e-9, "a hypothesis within 1e-9 of cos_eps: change the fixture"
    assert c["degeneracy"] <= 0.5, "a hypothesis within a factor 2 of the degeneracy bound: change the fixture"
    assert r["found"] and r["best_count"] > len(xyz) // 3
    if sp["axis"] is not None:
        assert r["n_rejected"] > 0
    if sp["refine"]:
        # noise <= T / 2, clutter >= 2 T: the refined plane's inliers keep clear of the threshold by far more than the bound
        dn, dd = pc.refine_bound(r["sums"], r["lam"], float(np.linalg.norm(r["a"] + r["sums"]["S1"] / r["sums"]["count"])))
        s = r["keys"][np.isfinite(r["keys"])]
        reach = float(np.abs(xyz[np.isfinite(xyz).all(1)].astype(np.float64)).sum(1).max())
        margin = float(np.abs(np.abs(s) - sp["T"]).min())
        print(name, "refine bound dn %.3g dd %.3g, margin %.3g" % (dn, dd, margin))
        assert r["refined"] and margin > 2 * (dn * reach + dd)


def test_shape_cloud_clearances():
    """the plan-boundary shapes of tests/test_gpu_plane.py: prefixes of one cloud"""
    assert len(pc.shape_cases()) == len(pc.SHAPE_N) + 2 * len(pc.SHAPE_H)
    for n, sp in pc.shape_cases():
        c = pc.clearances(pc.shape_cloud(n), sp)
        assert c["distance"] >= 1e-9 and c["angle"] >= 1e-9 and c["degeneracy"] <= 0.5, (n, sp, c)
