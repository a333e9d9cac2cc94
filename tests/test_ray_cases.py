"""CPU: the reference of the clearing rays (tests/ray_cases.py) pinned to hand cases with exact cells, its two forms (one ray
in pure Python, many in numpy) against each other, and the properties every walk has."""
import numpy as np
import pytest

import ray_cases as rc

LEAVES = (1.0, 0.3, 0.7, 1.5)


@pytest.mark.parametrize("case", range(len(rc.HAND)))
def test_hand_cases(case):
    o, p, margin, want = rc.HAND[case]
    got = rc.walk_one(o, p, 1.0, margin)
    many = rc.walk_many(o, [p], 1.0, margin)
    if want is None:
        assert got is None and not many["cast"][0] and many["n"][0] == 0 and len(many["cells"]) == 0
        return
    assert got[0] == want
    assert many["cast"][0] and many["n"][0] == len(want) and [tuple(c) for c in many["cells"]] == want


def test_the_lowest_axis_wins_a_tie():
    cells, clearance, _ = rc.walk_one((0.25, 0.25, 0.5), (2.25, 2.25, 0.5), 1.0)
    assert cells[1] == (1, 0, 0) and clearance == 0.0
    cells, _, _ = rc.walk_one((0.5, 0.5, 0.5), (2.5, 2.5, 2.5), 1.0)
    assert cells == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)]


def test_range_tests_and_the_lattice():
    o, p = (0.5, 0.5, 0.5), (3.5, 0.5, 0.5)                          # len 3
    assert rc.walk_one(o, p, 1.0, 0.0, 3.0, 3.0) is not None
    assert rc.walk_one(o, p, 1.0, 0.0, 3.5, 10.0) is None and rc.walk_one(o, p, 1.0, 0.0, 0.0, 2.5) is None
    lim = float(rc.LATTICE)
    cells, _, _ = rc.walk_one((lim - 1.5, 0.5, 0.5), (lim + 2.5, 0.5, 0.5), 1.0)   # leaves the lattice: the walk ends there
    assert cells == [(rc.LATTICE - 2, 0, 0), (rc.LATTICE - 1, 0, 0)]
    cells, _, _ = rc.walk_one((lim + 0.5, 0.5, 0.5), (lim - 2.5, 0.5, 0.5), 1.0)   # a start outside it visits nothing
    assert cells == []
    w = rc.walk_many([(lim - 1.5, 0.5, 0.5), (lim + 0.5, 0.5, 0.5)], [(lim + 2.5, 0.5, 0.5), (lim - 2.5, 0.5, 0.5)], 1.0)
    assert w["cast"].all() and w["n"].tolist() == [2, 0]


@pytest.mark.parametrize("leaf", LEAVES)
def test_properties_and_the_two_forms(leaf):
    origin, pts = rc.random_rays(int(leaf * 10), 1500, leaf, reach=40.0)
    assert len(pts) >= 0.99 * 1500
    w = rc.walk_many(origin, pts, leaf)
    assert w["cast"].all() and (w["clearance"] >= rc.CLEAR).all()
    L = float(np.float32(leaf))
    total = 0
    for i in range(len(pts)):
        cells, clearance, ln = rc.walk_one(origin, pts[i], leaf)
        mine = w["cells"][w["ray"] == i]
        assert np.array_equal(np.array(cells), mine) and clearance == w["clearance"][i] and ln == w["len"][i]
        assert len(set(cells)) == len(cells)                              # unique
        steps = np.abs(np.diff(np.array(cells), axis=0))
        assert (steps.sum(axis=1) == 1).all()                             # one axis, one cell at a time
        start = [rc.start_cell(float(v), L) for v in origin]
        end = [rc.start_cell(float(v), L) for v in pts[i]]
        assert list(cells[0]) == start
        assert len(cells) == 1 + sum(abs(a - b) for a, b in zip(start, end))   # margin 0, a clear ray: it ends in the point's cell
        assert list(cells[-1]) == end
        total += len(cells)
    assert total == w["n"].sum() == len(w["cells"])


@pytest.mark.parametrize("leaf", (1.0, 0.7))
def test_margin_shortens_a_walk_and_counts_sum_over_clouds(leaf):
    origin, pts = rc.random_rays(77, 800, leaf, reach=30.0)
    pts = rc.clear_points(pts, origin, leaf, margin=2.5 * leaf)
    full = rc.walk_many(origin, pts, leaf)
    short = rc.walk_many(origin, pts, leaf, margin=2.5 * leaf)
    assert (short["n"] <= full["n"]).all() and (short["n"][short["cast"]] >= 1).all() and short["n"].sum() < full["n"].sum()
    for i in np.nonzero(short["cast"])[0][:200]:
        a, b = full["cells"][full["ray"] == i], short["cells"][short["ray"] == i]
        assert np.array_equal(a[:len(b)], b)                              # a prefix of the unshortened walk
    # a call's counts: two clouds summed, the hit cells flagged, every voxel in ascending key
    vox = np.unique(np.concatenate([full["cells"][::5], rc.build_cells(pts, leaf)[0][::3]]), axis=0)
    one = rc.call_counts(vox, [(pts, origin)], leaf, 0.0)
    two = rc.call_counts(vox, [(pts[:300], origin), (pts[300:], origin)], leaf, 0.0)
    for k in ("cast", "skipped", "visited"):
        assert one[k] == two[k]
    assert np.array_equal(one["miss"], two["miss"]) and np.array_equal(one["hit"], two["hit"])
    assert (np.diff(rc.pack(one["cells"])) > 0).all() and one["visited"] == full["n"].sum() and one["cast"] == len(pts)
    assert one["hit"].any() and (one["miss"] > 0).any() and one["clearance"] >= rc.CLEAR
    gone = rc.removed_cells(one, 1)
    assert len(gone) == ((one["miss"] >= 1) & ~one["hit"]).sum() > 0
