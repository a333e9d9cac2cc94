"""CPU: the helpers of tests/fitness_cases.py -- the brute-force reference of the per-query getFitnessScore tests and the
generators of their inputs.  The reference is checked against an f64 k-d tree; every generator is checked to produce the
classes of queries it claims, for the seeds the GPU tests (tests/test_gpu_fitness_edges.py) use, from the reference and the
geometry model alone."""
import numpy as np
import pytest

import fitness_cases as fc

F = np.float32


# ---------------------------------------------------------------------------------------------------- nearest_d2
def test_nearest_d2_equals_a_kdtree_to_f32_rounding():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(1)
    t = rng.uniform(-20, 20, (5000, 3)).astype(F)
    q = rng.uniform(-25, 25, (3000, 3)).astype(F)
    d2, arg = fc.nearest_d2(t, q)
    dist, idx = cKDTree(t.astype(np.float64)).query(q.astype(np.float64))
    # three squares and two sums of f32 (each within 2^-24 relative), differences of f32 coordinates up to 45 m taken in f32
    # (exact here only when the exponents agree: allow an ulp of the coordinates)
    assert d2.dtype == F and np.allclose(d2, dist ** 2, rtol=4 * 2.0 ** -24, atol=45 * 2.0 ** -20)
    # the neighbour is the tree's, or one that ties with it within that rounding
    other = arg != idx
    assert other.mean() < 0.01
    alt = ((t[arg[other]].astype(np.float64) - q[other].astype(np.float64)) ** 2).sum(axis=1)
    assert np.allclose(alt, dist[other] ** 2, rtol=1e-5)
    # any chunking gives the same bits
    d2b, argb = fc.nearest_d2(t, q, pairs_per_step=5000)
    assert np.array_equal(d2, d2b) and np.array_equal(arg, argb)


def test_nearest_d2_is_brute_force_fitness_per_query():
    """the standing reference of the mean checks (test_gpu_parity.brute_force_fitness), per query"""
    rng = np.random.default_rng(2)
    t = rng.uniform(-5, 5, (9000, 3)).astype(F)  # more than one chunk of either
    q = rng.uniform(-6, 6, (700, 3)).astype(F)
    d2, _ = fc.nearest_d2(t, q)
    best = np.full(len(q), np.inf, dtype=F)
    for a in range(0, len(t), 4096):
        tt = t[a:a + 4096]
        dx, dy, dz = (q[:, None, i] - tt[None, :, i] for i in range(3))
        best = np.minimum(best, ((dx * dx + dy * dy).astype(F) + (dz * dz).astype(F)).min(axis=1))
    assert np.array_equal(d2, best)
    for r in (np.inf, 0.05):
        ok = best.astype(np.float64) <= r
        assert fc.member_value(d2, r) == float(best[ok].astype(np.float64).sum() / ok.sum())


def test_nearest_d2_ties_non_finite_points_and_overflow():
    t = np.array([[0, 0, 0], [2, 0, 0], [np.nan, 0, 0], [0, 2, 0], [0, np.inf, 0], [2, 0, 0]], dtype=F)
    q = np.array([[1, 0, 0],        # ties between points 0, 1 and 5: the value is 1, the first index wins
                  [2, 0, 0],        # on points 1 and 5
                  [np.nan, 0, 0],   # no neighbour
                  [0, np.inf, 0],
                  [1e20, 0, 0],     # 1e40 overflows f32
                  [1, 1, 0]], dtype=F)
    d2, arg = fc.nearest_d2(t, q)
    assert np.array_equal(d2, np.array([1, 0, np.inf, np.inf, np.inf, 2], dtype=F))
    assert arg.tolist() == [0, 1, -1, -1, -1, 0]
    assert np.array_equal(fc.one_point_values(d2), [1, 0, fc.DBL_MAX, fc.DBL_MAX, fc.DBL_MAX, 2])
    assert fc.member_value(d2) == 1.0 and fc.member_value(d2[2:5]) == fc.DBL_MAX
    assert fc.member_value(d2, 1.0) == 0.5 and fc.member_value(d2, np.nextafter(1.0, 0)) == 0.0
    # a doubled target: the same values
    assert np.array_equal(fc.nearest_d2(np.concatenate([t, t]), q)[0], d2)
    # no finite target point, no query
    assert np.array_equal(fc.nearest_d2(t[[2, 4]], q)[0], np.full(6, np.inf, dtype=F))
    assert fc.nearest_d2(t, np.zeros((0, 3), F))[0].shape == (0,)


def test_grid_model_cells_and_margins():
    m = fc.GridModel([-2, 0, 1], [3, 0, 4], 0.5)
    assert m.div_b.tolist() == [6, 1, 4] and m.r_lim == 6
    lo, hi = m.box()
    assert lo.tolist() == [-1.0, 0.0, 0.5] and hi.tolist() == [2.0, 0.5, 2.5]
    q = np.array([[0.1, 0.2, 0.6], [-1.0, 0.25, 1.0], [2.0, 0.1, 0.7], [-9.0, 9.0, 0.75]], dtype=F)
    cell, inside, margin = m.query_cell(q)
    assert cell.tolist() == [[2, 0, 0], [0, 0, 1], [5, 0, 0], [0, 0, 0]]
    assert inside.tolist() == [True, True, False, False]
    assert margin[1] == 0 and margin[2] == 0 and margin[3] == 0 and margin[0] == pytest.approx(0.1, abs=1e-6)
    assert m.point_cell(np.array([[1.9, 0.4, 2.4]], dtype=F)).tolist() == [[5, 0, 3]]
    t = np.array([[1.9, 0.4, 2.4], [-0.9, 0.1, 0.6]], dtype=F)
    c = m.classify(t, q)
    assert c["shell"].tolist() == [2, 1, 3, 0]
    # max_shells: the cost term of the code, and where it steps
    steps = fc.by_cost_steps()
    for n in steps:
        assert (int(np.sqrt(np.sqrt(F(2 * n)))) - 1) // 2 == (int(np.sqrt(np.sqrt(F(2 * (n - 1))))) - 1) // 2 + 1


# ---------------------------------------------------------------------------------------------------- the generators
def test_plan_sizes_sit_on_the_plan_boundaries():
    sizes = fc.PLAN_SIZES + fc.CAP_SIZES
    blocks = [fc.fitness_blocks(n) for n in sizes]
    assert blocks[sizes.index(32)] == 1 and blocks[sizes.index(33)] == 2          # a block's 32 teams
    assert blocks[sizes.index(65535)] == 2048 and fc.fitness_blocks(65505) == 2048 and fc.fitness_blocks(65504) == 2047
    assert 65536 == 2048 * 32 and blocks[sizes.index(65537)] == 2048                # the teams stride from here on
    assert {1, 2, 3, 4} <= set(sizes)                                               # fewer slots than a wave has teams
    assert sum(fc.plan_spoiled(n) for n in sizes) >= len(sizes) // 3
    q = fc.plan_queries(131073)
    assert np.array_equal(fc.plan_queries(4097), q[:4097]) and q.dtype == F
    model = fc.GridModel.from_points(fc.plan_target(), fc.PLAN_RES)
    inside = model.query_cell(q[:8193])[1]
    assert 0.2 < inside.mean() < 0.9  # queries in and around the box


def test_reduce_members_have_the_block_counts_named():
    scans, blocks = fc.reduce_members()
    assert [fc.fitness_blocks(len(s)) if len(s) else 0 for s in scans] == blocks
    kinds = [("empty" if len(s) == 0 else "bad" if not np.isfinite(s).any() else "ok") for s in scans]
    assert sorted(b for b, k in zip(blocks, kinds) if k == "ok") == sorted(fc.REDUCE_BLOCKS)
    assert kinds.count("empty") == 2 and kinds.count("bad") == 2
    first, last = kinds.index("ok"), len(kinds) - 1 - kinds[::-1].index("ok")
    assert any(k != "ok" for k in kinds[first:last])  # ... between them
    assert blocks != sorted(blocks)  # shuffled
    assert sum(len(s) for s in scans) * 2000 < 1e9  # brute force stays quick


def test_handoff_members_have_exactly_their_masks():
    t = fc.slab_target()
    model = fc.GridModel.from_points(t, fc.SLAB_RES)
    assert model.div_b.tolist() == [20, 20, 20]
    mem = fc.handoff_members()
    assert len(mem) == 256 and all(m.shape == (8, 3) for m in mem)
    cls = model.classify(t, np.concatenate(mem))
    far, near = fc.is_far(model, cls).reshape(256, 8), fc.is_near(model, cls).reshape(256, 8)
    assert (far ^ near).all()  # every query is one or the other
    assert cls["inside"].all()
    got = (far * (1 << np.arange(8))).sum(axis=1)
    assert np.array_equal(got, np.arange(256))  # member m's far bits are exactly m
    for k, mask in enumerate(fc.handoff_masks64()):
        q = fc.handoff_queries(mask, seed=2000 + k)
        c = model.classify(t, q)
        assert np.array_equal(fc.is_far(model, c), np.asarray(mask, dtype=bool))
        assert np.array_equal(fc.is_near(model, c), ~np.asarray(mask, dtype=bool))
    masks = fc.handoff_masks64()
    assert any(1 < np.sum(m) < 63 for m in masks) and any(np.sum(m) == 1 for m in masks)


@pytest.mark.parametrize("n", fc.SHELL_SIZES)
def test_shell_queries_cover_every_ending(n):
    # the sizes sit either side of a step of max_shells' cost term -- recomputed from the model of the code
    steps = fc.by_cost_steps()
    lo, hi = fc.SHELL_SIZES[fc.SHELL_SIZES.index(n) & ~1], fc.SHELL_SIZES[fc.SHELL_SIZES.index(n) | 1]
    assert hi == lo + 1 and hi in steps
    t = fc.shell_target(n)
    assert len(t) == n and np.isfinite(t).all()
    model = fc.GridModel.from_points(t, fc.SHELL_RES)
    assert model.div_b.tolist() == [16, 12, 12]
    r_max = model.r_max(n)
    assert r_max == model.r_max(lo) + (n == hi) and r_max + 1 < 8
    q, kind = fc.shell_queries(t, n)
    cls = model.classify(t, q)
    assert cls["inside"].all()
    d = np.sqrt(cls["d2"].astype(np.float64))
    own = kind == "own"
    # stops at r = 0: the neighbour is in the query's own cell and nearer than the margin less the slack
    assert own.sum() >= 8 and (cls["shell"][own] == 0).all() and (d[own] < cls["margin"][own] - model.slack).all()
    for name, k in (("shell1", 1), ("shell2", 2), ("shell3", 3), ("rmax", r_max), ("rmax+1", r_max + 1)):
        sel = kind == name
        assert sel.sum() >= 8 and (cls["shell"][sel] == k).all(), name
        # ... and no nearer shell can end the search: the neighbour is farther than shell k - 1's largest bound
        assert (d[sel] > (k - 1) + cls["margin"][sel]).all(), name
    assert (cls["d2"][kind == "exact"] == 0).all() and (kind == "exact").sum() >= 8
    for name in ("face", "edge", "corner"):
        sel = kind == name
        assert sel.sum() >= 8 and (cls["margin"][sel] == 0).all(), name
        on = (q[sel] == np.floor(q[sel])).sum(axis=1)
        assert (on == {"face": 1, "edge": 2, "corner": 3}[name]).all()
    assert set(cls["shell"][kind == "face"]) >= {0, 1, 2, 4, 7}  # (7: beyond r_max + 1 as well)


@pytest.mark.parametrize("L", (1, 2, 3, 4))
def test_rlim_targets_have_the_box_named(L):
    t = fc.rlim_target(L)
    model = fc.GridModel.from_points(t, 1.0)
    assert model.div_b.tolist() == [L, L, L] and model.r_lim == L
    assert model.r_max(len(t)) == min(L, 3)  # r >= r_lim ends the walk before (L < 3) or with (L = 3) the shells allowed
    q = fc.rlim_queries(L)
    cls = model.classify(t, q)
    assert cls["inside"].any() and (~cls["inside"]).any()
    assert set(cls["shell"]) == set(range(L))  # every shell the box has


def test_awkward_cases_are_what_they_are_called():
    cases = {name: (t, res, dense, q) for name, t, res, dense, q in fc.awkward_cases()}
    assert len(cases) == 22
    for name, (t, res, dense, q) in cases.items():
        assert 200 <= len(q) <= 500 and q.dtype == F and t.dtype == F, name
        assert dense == bool(np.isfinite(t).all()), name
        model = fc.GridModel.from_points(t, res)
        cls = model.classify(t, q)
        assert cls["inside"].any() and (~cls["inside"]).any(), name
        assert (cls["d2"] == 0).any(), name
    div = lambda name: fc.GridModel.from_points(cases[name][0], cases[name][1]).div_b.tolist()
    assert div("one_point") == [1, 1, 1] and div("three_coincident") == [1, 1, 1] and div("one_cell_res50") == [1, 1, 1]
    assert div("line_x")[1:] == [1, 1] and div("line_x")[0] >= 39 and div("line_z")[:2] == [1, 1] and div("line_z")[2] >= 39
    assert div("plane")[2] == 1 and min(div("plane")[:2]) >= 29
    for c in (1, 15, 16, 17, 127, 128, 129):
        t = cases["cell_of_%d" % c][0]
        model = fc.GridModel.from_points(t, 1.0)
        cells = model.point_cell(t)
        assert (cells == 0).all(axis=1).sum() == c and len(t) == c + 1
        assert (fc.nearest_d2(cases["cell_of_%d" % c][3], t)[0] == 0).all()  # every point of the cell is a query
    for n in (255, 256, 257):
        t, res, _, q = cases["scan_all_%d" % n]
        model = fc.GridModel.from_points(t, res)
        cls = model.classify(t, q)
        assert len(t) == n and (cls["shell"] > model.r_max(n)).sum() >= 100  # reached only by the scan over all points
    for name in ("nan_front", "nan_back", "nan_scattered"):
        t = cases[name][0]
        bad = ~np.isfinite(t).all(axis=1)
        assert 30 <= bad.sum() < len(t) // 4
    assert not np.isfinite(cases["nan_front"][0][0]).all() and not np.isfinite(cases["nan_back"][0][-1]).all()
    t = cases["doubled"][0]
    assert np.array_equal(t[:len(t) // 2], t[len(t) // 2:])
    assert np.abs(cases["100km"][0]).min() > 9e4


@pytest.mark.parametrize("res", fc.FACE_RESOLUTIONS)
def test_face_case_sits_on_and_next_to_cell_faces(res):
    t, q, on_face = fc.face_case(res)
    assert t.shape == (3375, 3) and len(q) == 1500
    r = F(res)
    base = (np.arange(-2, 3).astype(F) * r).astype(F)
    for k in range(5):  # the target: k * res and its two f32 neighbours, on every axis
        for v in (base[k], np.nextafter(base[k], F(np.inf)), np.nextafter(base[k], F(-np.inf))):
            assert (t == v).any(axis=0).all()
    model = fc.GridModel.from_points(t, res)
    cls = model.classify(t, q)
    assert on_face.sum() > 300 and (cls["margin"][on_face & cls["inside"]] <= 2e-7).all()
    # queries an ulp off a face on either side, 0.4 and 0.6 of a leaf off, on target points
    _, vals, table = fc.face_tables(res)
    assert len(fc.FACE_OFFSETS) == len(table) == 7
    for o, name in enumerate(fc.FACE_OFFSETS):
        assert np.isin(q, table[o]).any(axis=1).sum() > 200, name
    assert np.array_equal(table[1], np.nextafter(vals, F(np.inf))) and np.array_equal(table[2], np.nextafter(vals, F(-np.inf)))
    for o, f in ((3, 0.4), (4, -0.4), (5, 0.6), (6, -0.6)):
        assert np.allclose((table[o] - vals) / r, f, atol=1e-5)
    assert cls["inside"].all() and (cls["d2"] == 0).sum() > 50  # (the ulp-off points open a layer of cells: all inside)
    # the point of the case: target points that sit OUTSIDE the cell they are binned into by the search's own arithmetic
    # cannot be ruled out -- queries whose neighbour is in another cell although it is (almost) no distance away
    assert ((cls["shell"] >= 1) & (cls["d2"] <= F(1e-10))).sum() > 100


@pytest.mark.parametrize("res", fc.MISBINNED_RESOLUTIONS)
def test_misbinned_points_are_outside_their_cells(res):
    t, q, gap2 = fc.misbinned_case(res)
    assert len(q) == 48 and len(t) == 96
    model = fc.GridModel.from_points(t, res)
    cls = model.classify(t, q)
    cell_q = cls["cell"]
    cell_p = model.point_cell(t[0::2])
    assert cls["inside"].all() and (cls["arg"] % 2 == 0).all() and (cls["shell"] == 1).all()  # the neighbour is P, next door
    assert (cell_p[:, 0] == cell_q[:, 0] + 1).all() and np.array_equal(model.point_cell(t[1::2]), cell_q)  # R: Q's own cell
    # P is binned into cell k although it lies below that cell's lower face
    lo = ((cell_p[:, 0] + model.min_b[0]).astype(F) * model.leaf).astype(F)
    assert (t[0::2, 0] < lo).all() and (t[0::2, 0] == np.nextafter(lo, F(-np.inf))).all()
    # after shell 0 the bound is |QR|^2: cell k's box is farther than that, P is nearer -- and the slack bridges it
    d_r = fc.nearest_d2(t[1::2], q)[0]
    assert (cls["d2"] < d_r).all() and (d_r < gap2).all()
    assert np.array_equal(gap2, ((lo - q[:, 0]) * (lo - q[:, 0])).astype(F))
    assert ((np.sqrt(gap2.astype(np.float64)) - model.slack) ** 2 < 0.99 * d_r).all()
    # shell 0 cannot end the search: |QR| is beyond the margin less the slack, the bound of shell 0
    assert (np.sqrt(d_r.astype(np.float64)) > 1.01 * (cls["margin"] - model.slack)).all()
    # the rounding of d^2 (2^-23 relative) is far below the gaps between the three distances
    assert ((d_r - cls["d2"]) > 1e-4 * d_r).all() and ((gap2 - d_r) > 1e-4 * d_r).all()


def test_outside_queries_cover_every_direction_and_distance():
    t = fc.plan_target()
    model = fc.GridModel.from_points(t, fc.PLAN_RES)
    q, di, ki = fc.outside_queries(model)
    assert len(q) == 26 * 6 + 1
    cls = model.classify(t, q)
    assert not cls["inside"].any()
    assert {(d, k) for d, k in zip(di[:-1], ki[:-1])} == {(d, k) for d in range(26) for k in range(6)}
    lo, hi = model.box()
    for i in range(len(q) - 1):
        d = fc.DIRECTIONS[di[i]]
        for ax in range(3):
            side = 1 if q[i, ax] >= hi[ax] else -1 if q[i, ax] < lo[ax] else 0
            assert side == d[ax], (i, ax)
    octants = {tuple(fc.DIRECTIONS[d]) for d in di[:-1] if 0 not in fc.DIRECTIONS[d]}
    assert len(octants) == 8
    # 1 ulp: the nearest f32 beyond the face
    ulp = ki == 0
    for i in np.nonzero(ulp)[0]:
        d = fc.DIRECTIONS[di[i]]
        for ax in range(3):
            if d[ax] > 0:
                assert q[i, ax] == np.nextafter(hi[ax], F(np.inf))
            if d[ax] < 0:
                assert q[i, ax] == np.nextafter(lo[ax], F(-np.inf))
    # the distances are what they are called, and finite in f32 up to 1e9 m; the last query overflows
    d = np.sqrt(cls["d2"][:-1].astype(np.float64))
    for k, want in enumerate(fc.OUTSIDE_DISTANCES):
        if want != "ulp":
            assert (d[ki[:-1] == k] >= 0.99 * want).all() and (d[ki[:-1] == k] <= 2 * want + 30).all()
    assert np.isfinite(cls["d2"][:-1]).all() and cls["d2"][-1] == np.inf
    assert fc.one_point_values(cls["d2"])[-1] == fc.DBL_MAX


def test_forms_queries_hold_the_classes_of_the_other_groups():
    for t in fc.forms_targets():
        model = fc.GridModel.from_points(t, fc.FORMS_RES)
        q = fc.forms_queries(t)
        assert 1400 <= len(q) <= 1600 and q.dtype == F
        cls = model.classify(t, q)
        r_max = model.r_max(len(t))
        assert cls["inside"].sum() > 500 and (~cls["inside"]).sum() > 300
        assert (cls["d2"] == 0).sum() >= 100
        assert (cls["margin"][cls["inside"]] == 0).sum() > 100      # on faces, edges, corners
        for k in range(0, 4):
            assert (cls["shell"] == k).sum() >= 5, k
        assert cls["d2"][-1] == np.inf
    # the small target is the one-launch build's, the large one is above it
    small, large = fc.forms_targets()
    assert len(small) == 3000 and len(large) == 60000
