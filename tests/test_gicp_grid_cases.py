"""CPU: the numpy reference of GICP's voxel target (tests/gicp_grid_cases.py) pinned to hand cases, and every fixture of
tests/test_gpu_gicp_grid.py shown to test what it claims: ties really tie in f32, the gate steps lie where they say, the rejected /
under-min_pts / drifted voxels are the nearest ones for their queries."""
import numpy as np

import centroid_fitness_cases as cc
import fitness_cases as fc
import gicp_grid_cases as gc

F = np.float32


def ndt_icov(points, eig_ratio=0.01):
    """the inverse covariance of one voxel as the reference makes it: sample covariance, the small eigenvalues raised to
    eig_ratio times the largest, inverted"""
    p = np.asarray(points, np.float64)
    c = np.cov(p.T, bias=False)
    w, v = np.linalg.eigh(c)
    w = np.maximum(w, eig_ratio * w[2])
    c = v @ np.diag(w) @ v.T
    return np.linalg.inv(c), c


def test_a_coplanar_voxel_has_its_plane_normal():
    n0 = np.array([1.0, 2.0, 2.0]) / 3.0
    a, b = np.array([2.0, -1.0, 0.0]) / np.sqrt(5.0), np.cross(n0, np.array([2.0, -1.0, 0.0]) / np.sqrt(5.0))
    uv = np.array([[0.1, 0.2], [0.4, -0.3], [-0.35, 0.3], [0.25, 0.4], [-0.2, -0.4], [0.0, 0.05], [0.3, 0.1], [-0.4, -0.1]])
    pts = np.array([0.5, 0.5, 0.5]) + uv[:, :1] * a + uv[:, 1:] * b      # 8 coplanar points
    icov, cov = ndt_icov(pts)
    C = gc.cov_plane(icov[None])[0]
    assert np.allclose(C @ n0, gc.GICP_EPSILON * n0, atol=1e-12)         # epsilon along the normal ...
    assert np.allclose(C @ a, a, atol=1e-12) and np.allclose(C @ b, b, atol=1e-12)   # ... one in the plane
    asym, eig, res = gc.plane_defects(C[None], icov[None])
    assert asym == 0.0 and eig < 1e-12 and res < 1e-9
    assert np.abs(gc.cov_raw(icov[None])[0] - cov).max() <= 1e-11 * np.abs(cov).max()
    wrong = np.eye(3) - (1 - gc.GICP_EPSILON) * np.outer(a, a)            # a covariance flattened along an in-plane direction fails
    assert gc.plane_defects(wrong[None], icov[None])[2] > 0.5


def test_cov_raw_is_the_cofactor_inverse():
    m = gc.spd(50, 3)
    assert np.abs(gc.cov_raw(m) @ m - np.eye(3)).max() < 1e-12
    assert np.linalg.cond(m).max() < 100


def test_a_tie_goes_to_the_lower_index_and_really_ties():
    pts, q = cc.tie_target()
    xyz, idx, _ = gc.d_of(pts)
    assert len(xyz) == 2 and idx[0] < idx[1]
    for row in q:
        assert gc.d2_f32(row, xyz[0]) == gc.d2_f32(row, xyz[1])            # equal in f32, bit for bit
    corr, _ = gc.correspond(xyz, q, 1e3)
    assert (corr == 0).all()
    corr, _ = gc.correspond(xyz[::-1], q, 1e3)                             # whichever comes first
    assert (corr == 0).all()


def test_a_query_on_the_gate_sphere_has_no_correspondence():
    pts, _ = cc.tie_target()
    xyz, _, _ = gc.d_of(pts)
    q = np.array([[-0.5, 0.5, 0.5]], F)                                    # 2 m from (1.5, 0.5, 0.5): d2 = 4 exactly
    v = float(gc.d2_f32(q[0], xyz[0]))
    assert v == 4.0
    g_at, g_up, g_lo, g_hi = gc.gate_steps(v)
    assert g_at * g_at == v and g_up * g_up > v and g_up == np.nextafter(g_at, np.inf)
    assert gc.correspond(xyz, q, g_at)[0][0] == -1                         # strict: d2 == gate^2 is outside
    assert gc.correspond(xyz, q, g_up)[0][0] == 0
    lo32, hi32 = float(np.nextafter(F(v), F(0))), float(np.nextafter(F(v), F(np.inf)))
    assert g_lo * g_lo <= lo32 < v < hi32 <= g_hi * g_hi                   # one f32 ulp of d2 either side
    assert g_lo * g_lo > float(np.nextafter(F(lo32), F(0))) and g_hi * g_hi < float(np.nextafter(F(hi32), F(np.inf)))
    assert gc.correspond(xyz, q, g_lo)[0][0] == -1 and gc.correspond(xyz, q, g_hi)[0][0] == 0


def test_gate_steps_of_general_distances():
    rng = np.random.default_rng(5)
    for v in (rng.random(40) * 30).astype(F):
        g_at, g_up, g_lo, g_hi = gc.gate_steps(v)
        assert g_at * g_at <= float(v) < g_up * g_up and g_lo * g_lo < float(v) < g_hi * g_hi


def test_source_sizes_sit_either_side_of_every_plan_step():
    steps = [n for n in range(1, 258) if gc.correspond_blocks(n + 1) != gc.correspond_blocks(n)]
    for n in steps[:2]:                                                    # up to the third block
        assert n in gc.SIZES and n + 1 in gc.SIZES
    assert [gc.correspond_blocks(n) for n in (32, 33, 64, 65)] == [1, 2, 2, 3]
    assert all(n in gc.SIZES for n in (1, 7, 8, 9, 31, 32, 33, 255, 256, 257))
    assert gc.correspond_blocks(257, gc.MAX_BLOCKS_CHILD) == 3 and gc.correspond_blocks(257) == 9   # the child strides


def test_the_rejected_voxel_is_the_nearest_centroid_of_its_queries():
    pts, cell, q = gc.rejected_case()
    C, _ = cc.centroid_cloud(pts, 1.0, 6)
    cells = cc.cloud_cells(pts, 1.0, 6)
    rej = int(np.nonzero((cells == np.asarray(cell)).all(axis=1))[0][0])
    assert (fc.nearest_d2(C, q)[1] == rej).all()                           # in the centroid cloud it wins ...
    D, _, dcells = gc.d_of(pts, rejected_cells=[cell])
    assert len(D) == len(C) - 1 and not (dcells == np.asarray(cell)).all(axis=1).any()
    corr, d2 = gc.correspond(D, q, gc.REJECTED_GATE)                       # (its f32 centroid has drifted some 20 m off, 500 km out)
    assert (corr >= 0).all() and (d2 > fc.nearest_d2(C, q)[0]).all()       # ... in D the next valid voxel does, farther away
    assert (gc.correspond(D, q, 5.0)[0] == -1).all()                       # and the default gate of 5 m leaves them without one


def test_the_voxels_under_min_pts_are_the_nearest_cells_of_their_queries():
    u, q = gc.under_case()
    d0, _, c0 = gc.d_of(u[0])
    d1, _, c1 = gc.d_of(np.concatenate(u))
    has = lambda cells, c: bool((cells == np.asarray(c)).all(axis=1).any())
    assert not has(c0, (5, 1, 1)) and not has(c1, (5, 1, 1))
    assert not has(c0, (1, 3, 1)) and has(c1, (1, 3, 1))
    for D, cells in ((d0, c0), (d1, c1)):
        corr, _ = gc.correspond(D, q[:2], 5.0)
        assert (corr >= 0).all() and not (cells[corr] == (5, 1, 1)).all(axis=1).any()
    late0, _ = gc.correspond(d0, q[2:], 5.0)
    late1, _ = gc.correspond(d1, q[2:], 5.0)
    assert not (c0[late0] == (1, 3, 1)).all(axis=1).any() and (c1[late1] == (1, 3, 1)).all(axis=1).all()


def test_the_drifted_centroid_lies_outside_its_cell_and_is_found():
    pts, cell, q = gc.excursion_case()
    D, _, cells = gc.d_of(pts)
    assert cc.excursion_of(D, cells) > 1.0                                 # by more than a cell
    me = int(np.nonzero((cells == np.asarray(cell)).all(axis=1))[0][0])
    corr, _ = gc.correspond(D, q, 5.0)
    mine = q[corr == me]
    assert len(mine) >= 20
    qc = cc.cells_of(mine, 1.0)
    assert (np.abs(qc - np.asarray(cell)).max(axis=1) >= 1).any()          # found from cells that are not its own


def test_every_kind_of_query_is_in_the_pool():
    pts = np.concatenate(cc.mixed_target())
    D, _, _ = gc.d_of(pts)
    q = gc.query_pool(D, pts, 1.0, 21)
    assert np.isfinite(q).all() and len(q) > 300
    d2, arg = fc.nearest_d2(D, q)
    assert np.isinf(d2).any() and (arg == -1).any()                        # 1e20 m: the distance overflows f32
    assert (np.abs(q).max(axis=1) > 9e4).any() and (d2[np.isfinite(d2)] > 1e9).any()   # the 100 km offsets
    for gate in gc.GATES:
        corr, _ = gc.correspond(D, q, gate)
        assert (corr == -1).any()
    assert (gc.correspond(D, q, gc.GATES[0])[0] == -1).all() and (gc.correspond(D, q, 5.0)[0] >= 0).any()


def test_matvec_and_rotation():
    T = gc.rotation()
    R = T[:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.abs(R - np.eye(3)).max() > 0.3
    p = np.asarray([[1.0, 2.0, 3.0]], F)
    assert np.allclose(gc.matvec_eigen(T, p)[0], R @ p[0] + T[:3, 3], atol=1e-5)
    assert np.array_equal(gc.matvec_eigen(np.eye(4, dtype=F), p), p)
