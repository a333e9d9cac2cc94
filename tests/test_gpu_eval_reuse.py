"""GPU: evaluation reuse (ndt_set_evaluation_reuse) changes how often the device is asked, and nothing else.  One handle,
the setter switched off and on, every output compared for equality: the server and the launch path of ndt_align, a lock-step
batch, a pairs call; and the premise itself -- an evaluation asked twice returns the same bits.

Clouds: the bundled pair at 1.0 m, the source whole (15 772 points) and as two 2 000-point draws.  The repeat counts of the
GPU's walks differ from the oracle's (last bits of the sums), so a count is asserted per path over its cases, not per case."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KDTREE, DIRECT26, DIRECT7, DIRECT1 = 0, 1, 2, 3
# (search, eps, max_iter): the four search methods at eps 1e-3, and DIRECT1 at eps 1e-9
CASES = [(KDTREE, 1e-3, 35), (DIRECT26, 1e-3, 35), (DIRECT7, 1e-3, 35), (DIRECT1, 1e-3, 35), (DIRECT1, 1e-9, 28)]


@pytest.fixture(scope="module")
def ndt(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import ndt as m
    return m


@pytest.fixture(scope="module")
def scans(pair):
    t, s = pair
    small = s[np.random.default_rng(5).choice(len(s), 2000, replace=False)]
    small2 = s[np.random.default_rng(6).choice(len(s), 2000, replace=False)]
    return t, s, small, small2


def handle(ndt, t):
    g = ndt.NormalDistributionsTransform()
    g.setResolution(1.0)
    g.setInputTarget(t)
    return g


def configure(g, case):
    search, eps, max_iter = case
    g.setNeighborhoodSearchMethod(search)
    g.setTransformationEpsilon(eps)
    g.setMaximumIterations(max_iter)


def single(g, n):
    cloud = g.align(n_out=n)
    return dict(T=g.getFinalTransformation(), iterations=g.getFinalNumIteration(), converged=g.hasConverged(),
                probability=g.getTransformationProbability(), stats=g.stats(), cloud=cloud)


def check_counters(g, st, reuse_on):
    served, reused = g.evalReuse()
    assert served + reused == st["n_evals"] + st["n_hessian_recomputes"]
    if not reuse_on:
        assert reused == 0
    return reused


@pytest.mark.parametrize("persistent", [True, False], ids=["server", "launch"])
def test_align_is_unchanged_by_reuse(ndt, scans, persistent):
    t, _, small, _ = scans
    g = handle(ndt, t)
    g.setInputSource(small)
    g.setEvaluationPath(persistent)
    total = 0
    for case in CASES:
        configure(g, case)
        g.setEvaluationReuse(False)
        off = single(g, len(small))
        check_counters(g, off["stats"], False)
        g.setEvaluationReuse(True)
        on = single(g, len(small))
        n = check_counters(g, on["stats"], True)
        print("align %s case %s: %d evaluations, %d reused" % ("server" if persistent else "launch", case,
                                                              on["stats"]["n_evals"] + on["stats"]["n_hessian_recomputes"], n))
        total += n
        assert np.array_equal(on["T"], off["T"]), case
        assert on["iterations"] == off["iterations"] and on["converged"] == off["converged"], case
        assert on["probability"] == off["probability"], case
        assert on["stats"] == off["stats"], case
        assert np.array_equal(on["cloud"], off["cloud"]), case
    assert total >= 1, "no case of this path repeated an evaluation"


def compare_many(on, off, case):
    assert np.array_equal(on["T"], off["T"]), case
    assert np.array_equal(on["iterations"], off["iterations"]), case
    assert np.array_equal(on["converged"], off["converged"]), case
    assert np.array_equal(on["trans_probability"], off["trans_probability"]), case


def test_batch_is_unchanged_by_reuse(ndt, scans):
    t, s, small, small2 = scans
    g = handle(ndt, t)
    members = [small, small2, s]
    total = 0
    for case in CASES:
        configure(g, case)
        g.setEvaluationReuse(False)
        off = g.alignBatch(members)
        st_off = g.stats()
        check_counters(g, st_off, False)
        g.setEvaluationReuse(True)
        on = g.alignBatch(members)
        st_on = g.stats()
        n = check_counters(g, st_on, True)
        print("batch case %s: %d evaluations, %d reused" % (case, st_on["n_evals"] + st_on["n_hessian_recomputes"], n))
        total += n
        compare_many(on, off, case)
        assert st_on == st_off, case
    assert total >= 1, "no case of the batch repeated an evaluation"


def test_pairs_are_unchanged_by_reuse(ndt, scans):
    t, _, small, small2 = scans
    g = handle(ndt, t)
    clouds, pairs = [t, small, small2], [(0, 1), (0, 2)]
    total = 0
    for case in CASES:
        configure(g, case)
        g.setEvaluationReuse(False)
        off = g.alignPairs(clouds, pairs)
        st_off = g.stats()
        check_counters(g, st_off, False)
        g.setEvaluationReuse(True)
        on = g.alignPairs(clouds, pairs)
        st_on = g.stats()
        n = check_counters(g, st_on, True)
        print("pairs case %s: %d evaluations, %d reused" % (case, st_on["n_evals"] + st_on["n_hessian_recomputes"], n))
        total += n
        compare_many(on, off, case)
        assert st_on == st_off, case
    assert total >= 1, "no case of the pairs call repeated an evaluation"


def test_profile_mode_counts_every_evaluation(ndt, scans):
    """ndt_profile_enable(h, 1) times one launch per evaluation: reuse stays off under it, whatever the setter says."""
    t, s, _, _ = scans
    g = handle(ndt, t)
    g.setInputSource(s)
    g.setNeighborhoodSearchMethod(DIRECT26)
    g.setTransformationEpsilon(1e-3)
    g.setEvaluationReuse(True)
    g.profile(1)
    for k in range(3):
        g.profile_read(k)
    g.align()
    st = g.stats()
    n0, n1, n2 = (g.profile_read(k)[0] for k in range(3))
    g.profile(0)
    assert n0 + n1 == st["n_evals"] and n2 == st["n_hessian_recomputes"]
    assert g.evalReuse() == (st["n_evals"] + st["n_hessian_recomputes"], 0)


def test_an_evaluation_asked_twice_returns_the_same_bits(ndt, scans):
    """The premise: kinds 0, 1 and the f64 Hessian, through the launch path (eval / hessian_f64) and through one server."""
    t, _, small, _ = scans
    g = handle(ndt, t)
    g.setInputSource(small)
    p = np.array([0.31, -0.12, 0.04, 0.004, -0.007, 0.011])
    for search in (KDTREE, DIRECT26, DIRECT7, DIRECT1):
        g.setNeighborhoodSearchMethod(search)
        for with_h in (True, False):
            a, b = g.eval(p, with_h), g.eval(p, with_h)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[3] == b[3], (search, with_h)
            if with_h:
                assert np.array_equal(a[2], b[2]), search
        assert np.array_equal(g.hessian_f64(p), g.hessian_f64(p)), search
        for kind in (0, 1, 2):
            rows = g.evalServer(p, kind, 3)
            assert np.array_equal(rows[0].view(np.uint64), rows[1].view(np.uint64)), (search, kind)
            assert np.array_equal(rows[0].view(np.uint64), rows[2].view(np.uint64)), (search, kind)
            if kind != 2:
                assert rows[0, 0] != 0.0, (search, kind)  # a real evaluation, not an empty row
