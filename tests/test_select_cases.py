"""CPU: tests/select_cases.py -- the numpy restatement of the selection predicate -- pinned to cases worked out by hand from the
definition in include/ndt_mi355.h ("selection").  No library code runs here."""
import numpy as np

import select_cases as sc
from select_cases import BOX, BOX_NEGATE, FINITE, INF, KEY, KEY_NEGATE, NAN, RANGE, RANGE_NEGATE, F32


def one(s, p, k=0.0):
    return bool(sc.keep_mask(s, np.asarray([p], F32), np.asarray([k]))[0])


def test_the_exact_radius_is_inside_and_the_next_float_is_outside():
    s = sc.spec(RANGE, r_min=0, r_max=5)
    assert one(s, (3, 4, 0)) and one(s, (0, 0, 5)) and one(s, (0, 0, 0))
    assert not one(s, (sc.up(3), 4, 0)) and not one(s, (3, sc.up(4), 0)) and not one(s, (0, 0, sc.up(5)))
    s = sc.spec(RANGE, r_min=1, r_max=5)
    assert one(s, (0, 1, 0)) and not one(s, (0, sc.down(1), 0)) and not one(s, (0, 0, 0))
    s = sc.spec(RANGE | RANGE_NEGATE, r_min=1, r_max=5)
    assert not one(s, (3, 4, 0)) and one(s, (sc.up(3), 4, 0)) and one(s, (0, 0, 0)) and not one(s, (0, 1, 0))
    s = sc.spec(RANGE, centre=(10, -10, 1), r_min=0, r_max=5)
    assert one(s, (13, -6, 1)) and not one(s, (sc.up(13), -6, 1))


def test_the_distance_is_rounded_step_by_step_in_f32():
    # dx*dx = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 in f32; a fused multiply-add, or f64, would keep the 2^-24 and leave the
    # sum above r_max^2 = 1 + 2^-11 (with r_max = sqrt of it not needed: the centre trick below compares the sum directly)
    x = F32(1) + F32(2.0 ** -12)
    d2 = sc.dist2(np.asarray([[x, 0, 0]], F32), (0, 0, 0))[0]
    assert d2.dtype == F32 and d2 == F32(1) + F32(2.0 ** -11)
    assert float(x) * float(x) > float(d2)
    # the rows on which a fused multiply-add would differ are inside r_max = a, the last one (a third term of 2^-24) too
    s = sc.spec(RANGE, r_min=0, r_max=sc.A_FUSED)
    assert sc.keep_mask(s, sc.FUSED_ROWS).all()
    fused = [float(p[0]) ** 2 + float(p[1]) ** 2 + float(p[2]) ** 2 for p in sc.FUSED_ROWS]     # exact in f64
    assert all(F32(v) > sc.A_FUSED * sc.A_FUSED for v in fused)                                  # ... and would be outside
    # (dx*dx + dy*dy) first: 2^24 + 1 is lost, then + 1 is lost again; the other order would keep 2
    d2 = sc.dist2(np.asarray([[4096, 1, 1]], F32), (0, 0, 0))[0]
    assert d2 == F32(2.0 ** 24)


def test_each_box_face_is_inside_and_one_ulp_beyond_is_outside():
    rows, inside = sc.box_face_rows()
    assert rows.shape == (12, 3) and inside.sum() == 6
    s = sc.spec(BOX, box_min=sc.BOX_UNIT[0], box_max=sc.BOX_UNIT[1])
    assert (sc.keep_mask(s, rows) == inside).all()
    s["flags"] |= BOX_NEGATE
    assert (sc.keep_mask(s, rows) == ~inside).all()
    corner = sc.spec(BOX, box_min=(1, 2, 3), box_max=(1, 2, 3))        # a box of one point
    assert one(corner, (1, 2, 3)) and not one(corner, (1, 2, sc.up(3)))


def test_nan_and_inf_rows_under_every_combination_of_finite_and_negate():
    nan_row, inf_row, fin_in, fin_out = (NAN, 1, 1), (1, -INF, 1), (1, 1, 1), (50, 50, 50)
    box = dict(box_min=sc.BOX_UNIT[0], box_max=sc.BOX_UNIT[1])
    rng = dict(r_min=0, r_max=5)
    #            flags                                   NaN    inf    in     out
    table = [(sc.spec(0),                                 True,  True,  True,  True),
             (sc.spec(FINITE),                            False, False, True,  True),
             (sc.spec(BOX, **box),                        False, False, True,  False),
             (sc.spec(BOX | BOX_NEGATE, **box),           True,  True,  False, True),
             (sc.spec(BOX | FINITE, **box),               False, False, True,  False),
             (sc.spec(BOX | BOX_NEGATE | FINITE, **box),  False, False, False, True),
             (sc.spec(RANGE, **rng),                      False, False, True,  False),
             (sc.spec(RANGE | RANGE_NEGATE, **rng),       True,  True,  False, True),
             (sc.spec(RANGE | FINITE, **rng),             False, False, True,  False),
             (sc.spec(RANGE | RANGE_NEGATE | FINITE, **rng), False, False, False, True),
             (sc.spec(RANGE, r_min=0, r_max=INF),         False, True,  True,  True),    # d2 = inf <= inf; NaN never
             (sc.spec(RANGE | FINITE, r_min=0, r_max=INF), False, False, True, True)]
    for s, a, b, c, d in table:
        got = [one(s, nan_row), one(s, inf_row), one(s, fin_in), one(s, fin_out)]
        assert got == [a, b, c, d], (s["flags"], got)


def test_keys():
    s = sc.spec(KEY, key_lo=-1.0, key_hi=0.5)
    neg = sc.spec(KEY | KEY_NEGATE, key_lo=-1.0, key_hi=0.5)
    p = (1, 1, 1)
    for k, want, want_neg in ((NAN, False, False), (-1.0, True, False), (0.5, True, False), (np.nextafter(0.5, 1), False, True),
                              (np.nextafter(-1.0, -2), False, True), (INF, False, True), (-INF, False, True), (0.0, True, False)):
        assert one(s, p, k) == want and one(neg, p, k) == want_neg, k
    s = sc.spec(KEY, key_lo=0.25, key_hi=0.25)                       # key_lo == key_hi: exactly that value
    assert one(s, p, 0.25) and not one(s, p, np.nextafter(0.25, 1)) and not one(s, p, np.nextafter(0.25, 0))
    s = sc.spec(KEY | KEY_NEGATE, key_lo=0.25, key_hi=0.25)
    assert not one(s, p, 0.25) and one(s, p, np.nextafter(0.25, 1)) and not one(s, p, NAN)
    s = sc.spec(KEY, key_lo=-INF, key_hi=INF)                        # everything but NaN
    assert one(s, p, INF) and one(s, p, -INF) and one(s, p, 1e300) and not one(s, p, NAN)
    s = sc.spec(KEY | KEY_NEGATE, key_lo=-INF, key_hi=INF)           # nothing at all
    assert not one(s, p, 0.0) and not one(s, p, NAN) and not one(s, p, INF)
    assert one(sc.spec(KEY, key_lo=0, key_hi=1), (NAN, NAN, NAN), 0.5)   # the key test does not look at the point


def test_no_flags_keeps_everything_and_tests_combine_with_and():
    xyz, keys = sc.edge_cloud()
    assert sc.keep_mask(sc.spec(0), xyz, keys).all()
    assert sc.keep_mask(sc.spec(0), xyz).all()                          # no keys needed without KEY
    a = sc.spec(BOX, box_min=(-2, -3, -4), box_max=(60, 60, 60))
    b = sc.spec(RANGE, r_min=1, r_max=100)
    c = sc.spec(KEY, key_lo=0, key_hi=1)
    abc = sc.spec(BOX | RANGE | KEY, box_min=(-2, -3, -4), box_max=(60, 60, 60), r_min=1, r_max=100, key_lo=0, key_hi=1)
    want = sc.keep_mask(a, xyz) & sc.keep_mask(b, xyz) & sc.keep_mask(c, xyz, keys)
    assert (sc.keep_mask(abc, xyz, keys) == want).all() and 0 < want.sum() < xyz.shape[0]


def test_validity_rules():
    for s in sc.invalid_specs():
        assert not sc.spec_is_valid(s), s
    for s in sc.edge_specs():
        assert sc.spec_is_valid(s), s
    assert sc.spec_is_valid(sc.spec(RANGE, r_min=0, r_max=INF)) and sc.spec_is_valid(sc.spec(RANGE, r_min=-0.0, r_max=0))
    assert sc.spec_is_valid(sc.spec(KEY, key_lo=-INF, key_hi=INF)) and sc.spec_is_valid(sc.spec(BOX, box_min=(1, 1, 1), box_max=(1, 1, 1)))
    # bounds of a test that is not enabled are not looked at
    assert sc.spec_is_valid(sc.spec(FINITE, box_min=(NAN,) * 3, r_min=-1, key_lo=NAN))
    rng = np.random.default_rng(5)
    assert all(sc.spec_is_valid(sc.random_spec(rng)) for _ in range(200))
