"""CPU: the numpy restatement of the cluster definitions (tests/cluster_cases.py) pinned to cases worked out by hand -- the
comparison d2 <= tol2 at equality and one ulp beyond it, duplicates, the numbering rule, the size limits at size -/+ 1 -- and
its components cross-checked against scipy.sparse.csgraph where scipy is at hand.  No library code runs here."""
import numpy as np

import cluster_cases as cc
import outlier_cases as oc

F = np.float32


def sizes_of(ref):
    return ref["table"]["size"].tolist()


def test_three_collinear_points_at_exactly_the_tolerance():
    # 0, 0.5, 1.0 with tolerance 0.5: d2 = 0.25 == tol2, the comparison is <=
    ref = cc.reference(cc.collinear(0.5), 0.5)
    assert ref["roots"].tolist() == [0, 0, 0] and ref["labels"].tolist() == [0, 0, 0] and ref["indices"].tolist() == [0, 1, 2]
    assert ref["summary"] == dict(n_finite=3, n_components=1, n_clusters=1, n_clustered=3, largest=3)
    t = ref["table"][0]
    assert (t["root"], t["size"], t["first"]) == (0, 3, 0) and t["box_min"].tolist() == [0, 0, 0] and t["box_max"].tolist() == [1, 0, 0]
    assert t["centroid"].tolist() == [0.5, 0, 0]
    # the last point one ulp further: (1.0000001 - 0.5)^2 rounds above 0.25
    ref = cc.reference(cc.collinear(0.5, last_ulp=True), 0.5)
    assert ref["roots"].tolist() == [0, 0, 2] and ref["labels"].tolist() == [0, 0, 1] and sizes_of(ref) == [2, 1]
    assert ref["summary"]["n_components"] == 2 and ref["table"]["first"].tolist() == [0, 2]


def test_a_duplicate_pair_is_joined_at_any_tolerance():
    p = np.array([[1, 2, 3], [7, 7, 7], [1, 2, 3]], F)
    ref = cc.reference(p, 1e-30)  # tol2 underflows to 0: d2 == 0 <= 0
    assert ref["roots"].tolist() == [0, 1, 0] and ref["labels"].tolist() == [0, 1, 0] and ref["indices"].tolist() == [0, 2, 1]
    assert cc.reference(p, 1e-30, 2)["labels"].tolist() == [0, -1, 0]


def test_a_lattice_at_the_tolerance_and_just_beyond():
    ref = cc.reference(oc.lattice(3, 1.0), 1.0)
    assert ref["summary"] == dict(n_finite=27, n_components=1, n_clusters=1, n_clustered=27, largest=27)
    assert ref["table"][0]["centroid"].tolist() == [1, 1, 1] and ref["table"][0]["box_max"].tolist() == [2, 2, 2]
    ref = cc.reference(oc.lattice(3, 1.0 + 2.0 ** -20), 1.0)
    assert ref["summary"] == dict(n_finite=27, n_components=27, n_clusters=27, n_clustered=27, largest=1)
    assert ref["labels"].tolist() == list(range(27)) and ref["roots"].tolist() == list(range(27))


def test_equal_sizes_are_numbered_by_root_and_larger_ones_first():
    # rows: a pair (1, 4), a triple (0, 3, 5), a pair (2, 6), a single (7)
    p = np.array([[50, 0, 0], [0, 0, 0], [90, 0, 0], [50.1, 0, 0], [0.1, 0, 0], [50.2, 0, 0], [90.1, 0, 0], [-40, 0, 0]], F)
    ref = cc.reference(p, 0.15)
    assert ref["roots"].tolist() == [0, 1, 2, 0, 1, 0, 2, 7]
    assert ref["table"]["root"].tolist() == [0, 1, 2, 7] and sizes_of(ref) == [3, 2, 2, 1] and ref["table"]["first"].tolist() == [0, 3, 5, 7]
    assert ref["labels"].tolist() == [0, 1, 2, 0, 1, 0, 2, 3] and ref["indices"].tolist() == [0, 3, 5, 1, 4, 2, 6, 7]
    ref = cc.reference(p, 0.15, 2, 2)  # the triple and the single drop out: the pairs become 0 and 1
    assert ref["labels"].tolist() == [-1, 0, 1, -1, 0, -1, 1, -1] and ref["summary"]["n_clustered"] == 4 and ref["summary"]["largest"] == 3
    assert ref["others"].tolist() == [True, False, False, True, False, True, False, True]


def test_the_size_limits_at_size_minus_and_plus_one():
    p = cc.blobs((4, 6), 3, shuffle=False)  # rows 0 ... 3 and 4 ... 9
    for lo, hi, want in ((1, cc.BIG, [6, 4]), (4, 6, [6, 4]), (5, 6, [6]), (4, 5, [4]), (5, 5, []), (7, cc.BIG, []), (1, 3, []), (6, 6, [6]), (4, 4, [4])):
        ref = cc.reference(p, 0.8, lo, hi)
        assert sizes_of(ref) == want, (lo, hi)
        assert ref["summary"]["n_components"] == 2 and ref["summary"]["largest"] == 6 and ref["summary"]["n_clustered"] == sum(want)


def test_rows_that_are_not_finite_belong_to_nothing():
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [0.1, 0, 0], [0, np.inf, 0], [0.2, 0, 0]], F)
    ref = cc.reference(p, 0.15)
    assert ref["roots"].tolist() == [0, -1, 0, -1, 0] and ref["labels"].tolist() == [0, -1, 0, -1, 0]
    assert not ref["keep"][[1, 3]].any() and not ref["others"][[1, 3]].any() and ref["summary"]["n_finite"] == 3


def test_every_gpu_case_has_consistent_parts():
    for name, (xyz, specs) in cc.gpu_cases().items():
        for sp in specs:
            ref = cc.reference_of(name, xyz, sp)
            t, s = ref["table"], ref["summary"]
            assert len(t) == s["n_clusters"] and int(t["size"].sum()) == s["n_clustered"] == int(ref["keep"].sum()) == len(ref["indices"]), name
            assert (np.diff(t["size"]) <= 0).all() and ((np.diff(t["size"]) < 0) | (np.diff(t["root"]) > 0)).all(), name
            for c in range(len(t)):
                run = ref["indices"][t["first"][c]:t["first"][c] + t["size"][c]]
                assert (np.diff(run) > 0).all() and run[0] == t["root"][c] and (ref["labels"][run] == c).all(), (name, c)


def test_components_against_scipy():
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return  # (the hand cases above pin the components where scipy is not at hand)
    for name, (xyz, specs) in cc.gpu_cases().items():
        for tol in sorted({s["tolerance"] for s in specs}):
            fin = cc.finite_rows(xyz)
            e = cc.edge_list(xyz, tol)
            n = len(xyz)
            graph = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
            _, lab = connected_components(graph, directed=False)
            roots = cc.component_roots(n, fin, e)
            ids = np.flatnonzero(fin)
            # the same partition of F: a root per scipy label, and the root is the smallest index that carries the label
            first_of = {}
            for i in ids:
                first_of.setdefault(lab[i], i)
            assert all(roots[i] == first_of[lab[i]] for i in ids), (name, tol)
