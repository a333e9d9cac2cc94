"""CPU: the helpers of the centroid-fitness tests (tests/centroid_fitness_cases.py) checked on their own, so that the GPU cases
cannot silently stop covering their ground."""
import numpy as np

import centroid_fitness_cases as cc

F = np.float32


def scalar_centroid(p):
    s = np.zeros(3, dtype=F)
    for row in np.asarray(p, dtype=F):
        s = (s + row).astype(F)
    return s / F(len(p))


def test_centroid_cloud_is_the_scalar_loop_in_arrival_order():
    rng = np.random.default_rng(0)
    a = (1000.0 + rng.random((40, 3))).astype(F)            # one voxel of 40 points, a kilometre out: the order matters
    b = (np.array([1002.0, 1000.0, 1000.0]) + rng.random((5, 3))).astype(F)    # under min_pts
    pts = np.concatenate([a[:20], b, a[20:]])               # arrival order: the voxel's points are not contiguous
    xyz, idx = cc.centroid_cloud(pts, 1.0, 6)
    assert xyz.shape == (1, 3) and np.array_equal(idx, [0])
    assert np.array_equal(xyz[0], scalar_centroid(a))
    assert not np.array_equal(xyz[0], scalar_centroid(a[::-1]))   # (an order-free mean would pass both)
    xyz5, idx5 = cc.centroid_cloud(pts, 1.0, 5)             # min_pts 5: the second voxel is in, at linear index 2
    assert np.array_equal(idx5, [0, 2]) and np.array_equal(xyz5[1], scalar_centroid(b))


def test_the_two_derivations_agree_on_hand_built_rows():
    # three voxels: (0,0,0) of 6 points, (2,0,0) of 7, (1,1,0) of 5 (under min_pts 6)
    v0 = np.array([[0.25, 0.5, 0.75]] * 6, dtype=F) + np.arange(6, dtype=F)[:, None] * np.array([0.0625, 0.03125, 0.0], dtype=F)
    v1 = np.array([[2.5, 0.125, 0.5]] * 7, dtype=F) + np.arange(7, dtype=F)[:, None] * np.array([0.03125, 0.0625, 0.015625], dtype=F)
    v2 = np.array([[1.5, 1.5, 0.5]] * 5, dtype=F)
    pts = np.concatenate([v1, v2, v0])
    xyz, idx = cc.centroid_cloud(pts, 1.0, 6)
    blob = cc.rows_blob([(2, 0, 0, 7, np.cumsum(v1, axis=0, dtype=F)[-1]), (1, 1, 0, 5, np.cumsum(v2, axis=0, dtype=F)[-1]),
                         (0, 0, 0, 6, np.cumsum(v0, axis=0, dtype=F)[-1])])
    bx, cells = cc.centroids_from_blob(blob, 6)
    assert np.array_equal(cells, [[0, 0, 0], [2, 0, 0]])    # ascending (k, j, i), the voxel under min_pts left out
    assert np.array_equal(idx, [0, 2])
    assert np.array_equal(xyz, bx)
    assert np.array_equal(cc.cloud_cells(pts, 1.0, 6), cells)
    ex, ei = cc.centroid_cloud(v2, 1.0, 6)
    assert ex.shape == (0, 3) and ei.shape == (0,)
    assert cc.centroids_from_blob(cc.rows_blob([]), 6)[0].shape == (0, 3)


def test_mixed_target_holds_what_it_claims():
    u = cc.mixed_target()
    cat = np.concatenate(u)
    cells0 = {tuple(c) for c in cc.cloud_cells(u[0], 1.0, 6)}
    cells = {tuple(c) for c in cc.cloud_cells(cat, 1.0, 6)}
    assert (1, 0, 0) in cells and (3, 1, 0) in cells        # the collinear voxel and the voxel of identical points
    assert (5, 1, 1) not in cells                           # min_pts - 1 points
    assert (1, 3, 1) not in cells0 and (1, 3, 1) in cells   # crosses min_pts on the second update
    assert (9, 6, 2) in cells and cc.cells_of(u[0], 1.0).max(axis=0).tolist() != cc.cells_of(cat, 1.0).max(axis=0).tolist()  # the box grows
    assert cc.centroid_cloud(np.concatenate(cc.under_target()), 1.0, 6)[0].shape == (0, 3)
    pts, cell = cc.rejected_target()
    cells = cc.cloud_cells(pts, 1.0, 6)
    assert len(cells) == 15 and (cells == np.asarray(cell)).all(axis=1).sum() == 1   # 14 ordinary voxels and the collinear one
    assert (cc.cells_of(pts[-3000:], 1.0) == np.asarray(cell)).all()


def test_excursion_fixture_leaves_its_voxel_by_two_cells():
    pts, big = cc.excursion_target()
    xyz, _ = cc.centroid_cloud(pts, 1.0, 6)
    cells = cc.cloud_cells(pts, 1.0, 6)
    me = np.nonzero((cells == np.asarray(big)).all(axis=1))[0]
    assert len(me) == 1
    c = xyz[me[0]]
    assert (cc.cells_of(pts[:6000], 1.0) == np.asarray(big)).all()      # every point of the voxel IS in the owning cell
    assert c[0] - F(big[0] + 1) >= 2.0, c                               # its centroid: at least two cells outside
    assert cc.excursion_of(xyz, cells) == float(c[0] - F(big[0] + 1)) >= 2.0
    others = np.delete(np.arange(len(xyz)), me[0])
    assert cc.excursion_of(xyz[others], cells[others]) == 0.0           # the ordinary voxels stay inside
    # the same target a kilometre from the origin: every centroid inside its cell
    near, _ = cc.excursion_target(base=1000.0)
    nx, _ = cc.centroid_cloud(near, 1.0, 6)
    assert cc.excursion_of(nx, cc.cloud_cells(near, 1.0, 6)) == 0.0
    q = cc.excursion_queries(pts, big)
    assert len(q) > 500 and np.isfinite(q).all()


def test_shell_limit_is_the_cost_rule():
    assert cc.shell_limit((1, 1, 1)) == 1                   # the grid's extent bounds it
    assert cc.shell_limit((24, 1, 1)) == 3                  # 28 * 5 * 5 = 700 entries: (2r+1)^3 <= 175 gives 2, the floor 3
    assert cc.shell_limit((12, 12, 1)) == 3                 # 16 * 16 * 5 = 1280: 320 -> 2, the floor 3
    assert cc.shell_limit((40, 40, 1)) == 6                 # 44 * 44 * 5 = 9680: 2420 -> 13^3 = 2197 <= 2420 < 15^3
    assert cc.shell_limit((40, 40, 1), entries=1024) == 3   # a hash of 1024 slots
    assert cc.shell_limit((100, 100, 100), entries=1 << 20) == 31   # 262144 = 64^3: 63^3 <= it < 65^3


def test_edge_queries_cover_their_classes():
    rng = np.random.default_rng(1)
    for name, cells in cc.shape_targets().items():
        pts = cc.voxel_points(cells, rng)
        xyz, _ = cc.centroid_cloud(pts, 1.0, 6)
        assert len(xyz) == len(cells), name
        assert cc.excursion_of(xyz, cc.cloud_cells(pts, 1.0, 6)) == 0.0
        q = cc.edge_queries(xyz, pts, 1.0, np.random.default_rng(2))
        fin = q[np.isfinite(q).all(axis=1)]
        assert len(fin) == len(q) - 4
        d2, _ = cc.fc.nearest_d2(xyz, fin)
        shells = np.sqrt(d2.astype(np.float64))
        for lo, hi in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 6), (6, 9)):    # near, either side of the hand-off, beyond the floor
            assert ((shells >= lo) & (shells < hi)).any(), (name, lo, hi)
        assert np.isinf(d2).any() and (np.abs(fin) >= 1e20).any()          # the 1e20 m queries overflow f32
    t, q = cc.tie_target()
    xyz, _ = cc.centroid_cloud(t, 1.0, 6)
    assert np.array_equal(xyz, [[1.5, 0.5, 0.5], [3.5, 0.5, 0.5]])
    dx = [cc.fc.nearest_d2(xyz[k:k + 1], q)[0] for k in (0, 1)]
    assert np.array_equal(dx[0], dx[1])                                     # an exact tie for every query
