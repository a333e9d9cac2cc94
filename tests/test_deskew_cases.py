"""The numpy restatement of the motion compensation (tests/deskew_cases.py) pinned to cases worked by hand and to the physical
property it exists for.  No GPU, no library: this is the yardstick the host and GPU tests hold the library to."""
import numpy as np

import deskew_cases as dc


def one(p, t, m):
    return dc.reference_deskew(np.asarray([p], dtype=np.float64), np.array([t]), m)[0]


def test_a_quarter_turn_at_half_the_sweep():
    tau = np.array([0.8, -0.4, 0.2])
    m = dc.make_motion([0, 0, np.pi / 2], tau, 10.0, 12.0)
    q = one([1, 0, 0], 11.0, m)                          # s = 1/2: an eighth of a turn about z, half the translation
    assert np.abs(q - (np.array([np.sqrt(0.5), np.sqrt(0.5), 0]) + 0.5 * tau)).max() < 1e-15
    q = one([1, 0, 0], 12.0, m)                          # the end of the sweep: the whole motion
    assert np.abs(q - (np.array([0, 1, 0]) + tau)).max() < 1e-15
    q = one([1, 0, 0], 9.0, m)                           # before the sweep: extrapolated, no clamp
    assert np.abs(q - (np.array([np.sqrt(0.5), -np.sqrt(0.5), 0]) - 0.5 * tau)).max() < 1e-15


def test_pure_translation():
    m = dc.make_motion([0, 0, 0], [2, 4, -6], 0.0, 0.1)
    assert m.angle == 0 and list(m.axis) == [1, 0, 0]
    assert np.array_equal(one([1, 2, 3], 0.025, m), [1.5, 3, 1.5])
    assert np.array_equal(one([1, 2, 3], 0.2, m), [5, 10, -9])


def test_s_zero_leaves_the_point():
    for t_ref in (3.0, 3.5, 4.0, 7.0):
        m = dc.make_motion([0.3, -0.2, 0.9], [1, 2, 3], 3.0, 4.0, t_ref)
        p = np.array([12.5, -7.25, 0.125])
        assert np.array_equal(one(p, t_ref, m), p)


def test_edge_rows():
    m = dc.make_motion([0, 0, 1], [1, 0, 0])
    rec = np.array([[1, 2, 3], [np.nan, 2, 3], [1, np.inf, 3], [1, 2, 3], [1, 2, 3]], dtype=np.float32)
    t = np.array([0.5, 0.5, np.nan, np.nan, np.inf])
    assert list(dc.kinds(rec, t)) == [0, 1, 1, 2, 2]
    q = dc.reference_deskew(rec, t, m)
    assert np.isfinite(q[0]).all() and np.array_equal(q[1:3], rec[1:3].astype(np.float64), equal_nan=True) and np.isnan(q[3:]).all()


def test_t_ref_at_the_end_is_the_start_result_moved_by_the_inverse_motion():
    rng = np.random.default_rng(1)
    w, tau = np.array([0.2, -0.5, 0.7]), np.array([3.0, -1.0, 0.5])
    p = rng.uniform(-50, 50, (200, 3))
    t = rng.uniform(4.9, 5.3, 200)
    a = dc.reference_deskew(p, t, dc.make_motion(w, tau, 5.0, 5.1))
    b = dc.reference_deskew(p, t, dc.make_motion(w, tau, 5.0, 5.1, t_ref=5.1))
    R = dc.exp_rot(w / np.linalg.norm(w), np.linalg.norm(w))
    assert np.abs(b - (a - tau) @ R).max() < 1e-12       # rows (a - tau) R = (R^T (a - tau))^T


def test_static_world_points_come_back():
    """the property the step exists for: points of a static world, each measured at its own time from the moving sensor,
    p_i = T(u_i)^-1 W_i, are the world again after the deskew to t_begin"""
    rng = np.random.default_rng(2)
    world = rng.uniform(-80, 80, (500, 3))
    for w, tau in (([0, 0, 0.35], [1.0, 0.1, 0]), ([0.1, -0.2, 3.0], [0, 0, 0]), ([0, 0, 0], [1, 2, 3]), ([1e-9, 0, 0], [0.5, 0, 0])):
        t = rng.uniform(1.7e9, 1.7e9 + 0.1, 500)
        p = dc.skew_scan(world, t, w, tau, 1.7e9, 1.7e9 + 0.1)
        q = dc.reference_deskew(p, t, dc.make_motion(w, tau, 1.7e9, 1.7e9 + 0.1))
        assert np.abs(q - world).max() < 1e-12 * 80 * 10, (w, tau)
        if np.linalg.norm(w) > 0.1:
            assert np.abs(p - world).max() > 0.5             # (and the skew was no small thing)


def test_the_bound_is_the_derived_one():
    m = dc.make_motion([0, 0, 1], [1, -2, 0.5], 0.0, 1.0)
    rec = np.array([[1e5, -2e5, 3.0]], dtype=np.float32)
    b = dc.bound(np.array([[1.0, 3.0, 0.0]], np.float32), rec, np.array([2.0]), m)
    want = 64 * 2.0 ** -53 * (300003.0 + 2 * 3.5)
    assert np.allclose(b[0], [2.0 ** -24 + want, 2.0 ** -23 + want, 0.5 * 2.0 ** -149 + want], rtol=1e-12, atol=0)
