"""CPU: tests/normal_cases.py holds -- the numpy restatement of the normals contract against ndt_host_normal_from_sums on its own
sums and ndt_host_normal_keep on its own records, and the properties the GPU tests rely on: the conditioning cap of every case that
compares directions, the cases that are collinear (or clearly not) by construction, the golden scan's size, and the filters whose
kept sets keep 1e-6 clear of their bounds."""
import ctypes as C

import numpy as np
import pytest

import normal_cases as nc

F = np.float32
CASES = nc.gpu_cases()


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


@pytest.fixture(scope="module")
def refs():
    """the reference of every (case, spec), computed once"""
    return {(name, nc.tag_of(sp)): nc.reference(xyz, sp) for name, (xyz, specs) in CASES.items() for sp, _ in specs}


def c_spec(_lib, sp):
    s = _lib.NormalSpec()
    s.method, s.k, s.radius, s.min_neighbors = sp["method"], sp["k"], sp["radius"], sp["min_neighbors"]
    s.viewpoint[:] = sp["viewpoint"]
    return s


def c_filter(_lib, flt):
    f = _lib.NormalFilter()
    f.flags, f.curvature_lo, f.curvature_hi, f.cos_lo, f.cos_hi = flt["flags"], flt["curvature_lo"], flt["curvature_hi"], flt["cos_lo"], flt["cos_hi"]
    f.axis[:] = flt["axis"]
    return f


def host_record(L, _lib, sp, p, m, S1, S2):
    out, line = np.zeros(4, F), C.c_int(-1)
    p, S1, S2 = np.ascontiguousarray(p, F), np.ascontiguousarray(S1, np.float64), np.ascontiguousarray(S2, np.float64)
    st = L.ndt_host_normal_from_sums(C.byref(c_spec(_lib, sp)), p.ctypes.data_as(C.POINTER(C.c_float)), int(m),
                                     S1.ctypes.data_as(C.POINTER(C.c_double)), S2.ctypes.data_as(C.POINTER(C.c_double)),
                                     out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(line))
    assert st == _lib.NDT_OK
    return out, line.value


def test_the_golden_scan_is_the_issues_cloud():
    assert nc.golden_scan().shape == (2683, 3)


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if len(CASES[n][0]) <= 700])
def test_restatement_against_the_host_definition(mods, refs, name):
    """every row's record from the restatement's own sums through ndt_host_normal_from_sums: the comparison rules hold"""
    L, _lib, ndt = mods
    xyz, specs = CASES[name]
    for sp, directions in specs:
        ref = refs[(name, nc.tag_of(sp))]
        got = np.tile(nc.nan_record(), (len(xyz), 1))
        lines = 0
        for i, nb in enumerate(nc.neighbourhoods(xyz, sp)):
            if nb is None:
                continue
            S1, S2 = nc.sums_about(xyz, i, nb)
            got[i], line = host_record(L, _lib, sp, xyz[i], len(nb), S1, S2)
            lines += line
        bad = nc.compare(got, None, ref, sp, xyz, directions)
        assert not bad, (name, nc.tag_of(sp), bad)
        assert abs(lines - ref["stats"]["n_collinear"]) <= int(ref["near_line"].sum()), (name, nc.tag_of(sp))


def test_conditioning_cap_of_every_case_that_compares_directions(refs):
    worst = {}
    for name, (xyz, specs) in CASES.items():
        for sp, directions in specs:
            frac = nc.ill_fraction(refs[(name, nc.tag_of(sp))])
            worst[(name, nc.tag_of(sp))] = frac
            if directions:
                assert frac <= nc.ILL_CAP, (name, nc.tag_of(sp), frac)
    print({k: round(v, 4) for k, v in worst.items() if v > 0})
    # the golden scan (measured with this file: k = 20 0 %, k = 10 0.04 %, k = 5 2.9 %, r = 1.5 1.9 %, r = 0.8 6.0 %, k = 3 18 %):
    # k = 3 is out of the cap and is used for the property checks alone
    assert worst[("golden scan", "k=20")] == 0.0 and worst[("golden scan", "k=10")] < 0.001
    assert worst[("golden scan", "k=3")] > nc.ILL_CAP and not [d for sp, d in CASES["golden scan"][1] if sp["k"] == 3 and d]
    for k in nc.NEAR_K:
        if k == 3:
            continue
        for xyz in nc.near_k_clouds(k):
            assert nc.ill_fraction(nc.reference(xyz, nc.spec(k=k))) <= nc.ILL_CAP, (k, len(xyz))


def test_cases_built_to_be_collinear_or_clearly_not(refs):
    for sp in ("k=5", "r=7"):
        r = refs[("an exact line", sp)]
        assert r["valid"].all() and r["collinear"].all() and not r["near_line"].any()
    for key in (("an exact plane", "k=9"), ("an integer lattice", "k=7"), ("size n=513", "k=8"), ("golden scan", "k=10")):
        r = refs[key]
        assert r["valid"].any() and not r["collinear"].any() and not r["near_line"].any(), key
    r = refs[("an exact plane", "k=9")]
    assert (r["records"][:, 3] == 0).all() and (np.abs(r["records"][:, 2]) == 1).all()
    r = refs[("every point equal", "k=8")]
    assert not r["valid"].any() and (r["counts"] == 8).all() and r["stats"] == dict(n_finite=70, n_valid=0, n_collinear=0, max_neighbors=8)
    r = refs[("|F| < min_neighbors", "k=10 min=8")]
    assert not r["valid"].any() and sorted(set(r["counts"])) == [0, 5]
    r = refs[("|F| < k", "k=10")]
    assert (r["counts"] == 6).all() and r["valid"].all()
    # the k-th place of the lattice cuts a six-fold tie: the (d2, index) rule decides
    xyz = CASES["an integer lattice"][0]
    i = int(np.flatnonzero((xyz == 3).all(axis=1))[0])
    nb = nc.neighbourhoods(xyz, nc.spec(k=5), [i])[0]
    ring = np.flatnonzero(nc.d2_rows(xyz, [i])[0] == 1)
    assert len(ring) == 6 and list(nb) == [i] + list(ring[:4])
    # the radius case: exactly on and one ulp inside are members, one ulp outside is not
    xyz = CASES["on the radius"][0]
    assert refs[("on the radius", "r=0.5")]["counts"][0] == 1 + 12 + 9


SELECTIONS = {"curvature": nc.keep_filter(nc.KEEP_CURVATURE, curvature=(0.0, 0.02)),
              "angle to z": nc.keep_filter(nc.KEEP_ANGLE, axis=(0.0, 0.0, 1.0), cos=(0.9, 1.0)),
              "both, negated": nc.keep_filter(nc.KEEP_CURVATURE | nc.KEEP_ANGLE | nc.KEEP_NEGATE, curvature=(0.0, 0.05), axis=(0.0, 0.6, 0.8), cos=(0.0, 0.7)),
              "every normal": nc.keep_filter(0)}


def test_filter_restatement_against_the_host_predicate(mods, refs):
    L, _lib, ndt = mods
    rec = refs[("golden scan", "k=10")]["records"][:400]
    rec = np.concatenate([rec, np.tile(nc.nan_record(), (3, 1)), np.array([[0, 0, 1, 0.02], [0, 0, -1, 0], [1, 0, 0, 0.05], [0.6, 0, 0.8, np.nan]], F)])
    for name, flt in SELECTIONS.items():
        want = nc.keep_by(flt, rec)
        f = c_filter(_lib, flt)
        for r, w in zip(rec, want):
            k = C.c_int(-1)
            assert L.ndt_host_normal_keep(C.byref(f), np.ascontiguousarray(r).ctypes.data_as(C.POINTER(C.c_float)), C.byref(k)) == _lib.NDT_OK
            assert k.value == int(w), (name, r)
        assert not want[400:403].any() and not want[-1]
    assert nc.keep_by(SELECTIONS["every normal"], rec)[:400].sum() == (~np.isnan(rec[:400]).any(axis=1)).sum()


def test_the_golden_selections_keep_clear_of_their_bounds(refs):
    """so that the kept set of the device equals the reference's (tests/test_gpu_normals.py)"""
    rec = refs[("golden scan", "k=10")]["records"]
    for name in ("curvature", "angle to z"):
        flt = SELECTIONS[name]
        assert nc.filter_margin(flt, rec) > 1e-6, (name, nc.filter_margin(flt, rec))
        kept = int(nc.keep_by(flt, rec).sum())
        assert 0 < kept < len(rec), (name, kept)
