"""CPU: tests/leaf_cases.py, the fixtures at leaf sizes that are no power of two, pinned before the GPU tests stand on them.

(a) The reference (tests/nvtl_cases.Grid, the search cell by the QUOTIENT floor(x / leaf)) against the oracle on these
    fixtures: the score at rel 1e-13 (test_nvtl_cases.py's route; the terms are the same f64 numbers, only their order of
    summation differs), the neighbour count of every source point exactly, the KDTREE radius on every sphere query exactly.
(b) The fixtures tell the quotient from the PRODUCT floor(x * (1 / leaf)): a CONDITION of the GPU tests' worth, asserted
    here.  Per leaf and DIRECT method at origin 40, the source points whose NVTL value | neighbour count changes when the
    search cell is taken by the product rule (leaf_cases.product_rule_terms) are counted, at least 6 are demanded, and the
    counts are held to the table below (they depend on the face values and on which cells are occupied, not on the seed).
    KDTREE is exempt by construction: the two cells differ by one along an axis, a centroid that the shifted 3x3x3 block
    loses (or gains) lies at least one leaf from the point on that axis, and the radius test is strict -- the count is 0
    everywhere, which is asserted too.  face_target: the two rules bin at least 50 of its points differently, and the
    oracle's points per voxel are the product rule's."""
import numpy as np
import pytest

import centroid_fitness_cases as cc
import fitness_cases as fc
import leaf_cases as lc
import nvtl_cases as nc
import test_fitness_cases as tfc

F = np.float32
DIRECT = ("DIRECT1", "DIRECT7", "DIRECT26")
# origin 40: points whose value differs / whose neighbour count differs
DIFFER_AT_40 = {
    0.3: {"DIRECT1": (8, 4), "DIRECT7": (14, 20), "DIRECT26": (24, 20)},
    0.7: {"DIRECT1": (16, 10), "DIRECT7": (0, 14), "DIRECT26": (16, 16)},
    1.5: {"DIRECT1": (24, 14), "DIRECT7": (8, 30), "DIRECT26": (32, 30)},
    3.0: {"DIRECT1": (24, 14), "DIRECT7": (8, 30), "DIRECT26": (32, 30)},
}
BINNED_DIFFERENTLY = {0.3: 102, 0.7: 54, 1.5: 108, 3.0: 108}


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


def oracle_of(po, method, target, leaf):
    o = po.OracleNDT(resolution=leaf, num_threads=1, search_method=getattr(po, method), min_points_per_voxel=lc.MIN_PTS)
    o.set_target(target)
    return o


def oracle_counts(o, points):
    """the oracle's neighbour count of every point: the mean-neighbour value of a one-point source fed as trans_cloud"""
    out = np.zeros(len(points), dtype=np.int64)
    for i, p in enumerate(np.asarray(points, dtype=F)):
        o.set_source(p[None, :3])
        nn = o.eval(np.zeros(6), False, trans_cloud=np.r_[p[:3], F(1)][None, :])[3]
        assert nn == int(nn)
        out[i] = int(nn)
    return out


def test_the_fixtures_are_what_they_say():
    for leaf in lc.LEAVES:
        for origin in lc.ORIGINS:
            t, s = lc.face_scene(leaf, origin)
            assert s.shape == (468, 3) and t.dtype == s.dtype == F
            cells = lc.product_cells(t, leaf)
            assert np.array_equal(cells, lc.quotient_cells(t, leaf))               # no target point near a face
            lo = np.array([origin, origin, 0])
            assert np.array_equal(cells.min(axis=0), lo) and np.array_equal(cells.max(axis=0), lo + lc.BLOCK - np.ones(3, int))
            occupied, counts = np.unique(cells, axis=0, return_counts=True)
            assert (counts == 8).all() and ((occupied - lo).sum(axis=1) % 5 != 0).all()
            assert len(occupied) == sum((i + j + k) % 5 != 0 for i in range(8) for j in range(8) for k in range(3))
            # every source point: one coordinate within an ulp of a face f32(k * f32(leaf)), the other two mid-cell
            frac = s.astype(np.float64) / float(F(leaf))
            off = np.abs(frac - np.round(frac))
            assert ((off < 1e-5).sum(axis=1) == 1).all() and ((np.abs(off - 0.5) < 1e-5).sum(axis=1) == 2).all()
            assert len(np.unique(s, axis=0)) == 468
        ft = lc.face_target(leaf)
        assert ft.shape == (1440, 3) and len(np.unique(ft[:, 0])) == 240
        t, c, q = lc.sphere_queries(leaf)
        assert t.shape == (9, 3) and q.shape == (150, 3) and len(np.unique(lc.product_cells(t, leaf), axis=0)) == 1
        assert ((q != c).sum(axis=1) == 1).all()


@pytest.mark.parametrize("origin", lc.ORIGINS)
@pytest.mark.parametrize("leaf", lc.LEAVES)
def test_the_reference_is_the_oracle_on_face_points(po, leaf, origin):
    t, s = lc.face_scene(leaf, origin)
    for method in nc.METHODS:
        o = oracle_of(po, method, t, leaf)
        ref = nc.Grid.of_oracle(o, method, t, leaf, lc.MIN_PTS)
        q, has = ref.terms(s)
        q2, has2 = lc.quotient_rule_terms(ref, s)                                 # the copy product_rule_terms is made from
        assert np.array_equal(q, q2) and np.array_equal(has, has2)
        o.set_source(s)
        got, want = ref.score(s), o.calculate_score(s)
        counts = oracle_counts(o, s)
        wrong = int((has.sum(axis=1) != counts).sum())
        print("leaf %g origin %d %s: score rel %.3g; neighbour counts wrong at %d of %d points, %d points with a neighbour"
              % (leaf, origin, method, abs(got - want) / abs(want), wrong, len(s), int(has.any(axis=1).sum())))
        assert got == pytest.approx(want, rel=1e-13)
        assert wrong == 0 and has.any(axis=1).sum() > 100


@pytest.mark.parametrize("leaf", lc.LEAVES)
def test_the_radius_is_the_oracles_on_the_sphere(po, leaf):
    t, c, q = lc.sphere_queries(leaf)
    o = oracle_of(po, "KDTREE", t, leaf)
    ref = nc.Grid.of_oracle(o, "KDTREE", t, leaf, lc.MIN_PTS)
    assert ref.r2 == lc.kd_radius2(leaf) and ref.r2.dtype == F
    assert np.array_equal(ref.c_xyz, c[None, :])
    found = ref.terms(q)[1].sum(axis=1)
    counts = oracle_counts(o, q)
    print("leaf %g: %d of 150 queries inside the radius, %d disagree with the oracle" % (leaf, int(found.sum()), int((found != counts).sum())))
    assert np.array_equal(found, counts)
    assert 30 < found.sum() < 120 and found.max() == 1                            # the queries straddle the sphere


def test_the_radius_is_squared_from_the_f32_resolution():
    """at 0.7 the square of the Python double rounds to another f32 than the square of the f32 resolution"""
    assert F(0.7 * 0.7) != lc.kd_radius2(0.7)
    assert nc.Grid(dict(idx=[], n=[], mean=[], icov=[], min_b=[0, 0, 0], div_b=[0, 0, 0]), (1, 1, 1), "DIRECT7", 0.7).r2 == lc.kd_radius2(0.7)
    for leaf in (1.0, 0.5, 2.0):
        assert F(leaf * leaf) == lc.kd_radius2(leaf)                              # nothing changes where the file was pinned


@pytest.mark.parametrize("leaf", lc.LEAVES)
def test_the_fixture_tells_the_two_rules_apart(po, leaf):
    t, s = lc.face_scene(leaf, 40)
    for method in nc.METHODS:
        o = oracle_of(po, method, t, leaf)
        ref = nc.Grid.of_oracle(o, method, t, leaf, lc.MIN_PTS)
        value, count = lc.rules_differ(ref, s)
        either = int((value | count).sum())
        print("leaf %g %s: value differs at %d points, neighbour count at %d, either at %d" % (leaf, method, value.sum(), count.sum(), either))
        if method == "KDTREE":
            assert either == 0
            continue
        assert either >= 6
        assert (int(value.sum()), int(count.sum())) == DIFFER_AT_40[leaf][method]
        # ... and the score, which the GPU tests compare, moves with them
        qp, hasp = lc.product_rule_terms(ref, s)
        assert nc.score(qp, hasp, ref.d1, ref.d2, ref.d3) != ref.score(s)
    assert DIFFER_AT_40[0.7]["DIRECT7"][0] == 0                                   # there only the neighbour count tells


@pytest.mark.parametrize("leaf", lc.LEAVES)
def test_misbinned_points_and_centroids_need_the_slack(leaf):
    """fitness_cases.misbinned_case at these leaves: every claim test_fitness_cases.py makes of it at 0.1, 0.3 and 1/3, and the
    same of the six-fold form, whose centroids are the points"""
    tfc.test_misbinned_points_are_outside_their_cells(leaf)
    t, q, gap2 = fc.misbinned_case(leaf)
    target, q6, gap6, cloud = lc.misbinned_voxels(leaf)
    assert np.array_equal(q6, q) and np.array_equal(gap6, gap2) and target.shape == (576, 3)
    # (R, P) per site, in index order: a centroid is its point but for the rounding of the f32 sums -- and P's x is P's x
    assert np.array_equal(cloud[1::2, 0], t[0::2, 0]) and np.allclose(cloud, np.stack([t[1::2], t[0::2]], axis=1).reshape(-1, 3), rtol=1e-6, atol=0)
    cells = cc.cloud_cells(target, leaf, lc.MIN_PTS)
    assert np.array_equal(cells, lc.product_cells(cloud, leaf)) and (cells[1::2, 0] == cells[0::2, 0] + 1).all()
    assert cc.excursion_of(cloud[1::2], cells[1::2], leaf) > 0                                # P: below its cell's lower face
    d2, arg = fc.nearest_d2(cloud, q)
    d_r = fc.nearest_d2(cloud[0::2], q)[0]
    assert (arg % 2 == 1).all() and (d2 < d_r).all() and (d_r < gap2).all()                   # the bound after R's cell prunes P's


@pytest.mark.parametrize("leaf", lc.LEAVES)
def test_the_oracle_bins_target_points_by_the_product(po, leaf):
    ft = lc.face_target(leaf)
    prod, quot = lc.product_cells(ft, leaf), lc.quotient_cells(ft, leaf)
    differ = int((prod != quot).any(axis=1).sum())
    print("leaf %g: %d of %d target points binned differently by the two rules" % (leaf, differ, len(ft)))
    assert differ >= 50 and differ == BINNED_DIFFERENTLY[leaf]
    g = oracle_of(po, "DIRECT7", ft, leaf).grid()

    def per_voxel(cells):
        rel = cells - g["min_b"]
        assert (rel >= 0).all() and (rel < g["div_b"]).all()
        lin, n = np.unique(rel[:, 0] + rel[:, 1] * int(g["div_b"][0]) + rel[:, 2] * int(g["div_b"][0]) * int(g["div_b"][1]), return_counts=True)
        return lin, n

    lin, n = per_voxel(prod)
    assert np.array_equal(g["min_b"], prod.min(axis=0)) and np.array_equal(g["idx"], lin)
    # (the dump reports a voxel under min_points_per_voxel with its count too)
    assert np.array_equal(np.abs(g["n"]), n)
    qlin, qn = per_voxel(np.clip(quot, g["min_b"], g["min_b"] + g["div_b"] - 1))
    assert not (np.array_equal(qlin, lin) and np.array_equal(qn, n))
