"""CPU: evaluation reuse in the product's Newton / More-Thuente driver (ScanSolver, SolverParams::reuse_evaluations), through
ndt_host_run_driver_reuse.  The plain driver runs against the oracle and every (request bytes -> answer) is recorded; the
reusing driver then runs against an evaluator that replays that record and fails on a request it has not seen, so both runs
see the same function whatever OpenMP does.  Everything is compared for equality, nothing with a tolerance."""
import numpy as np
import pytest

from oracle import pyoracle as po


@pytest.fixture(scope="module")
def ndt(built_lib):
    from toyslam_amd import ndt as m
    return m


def small_source(s):
    rng = np.random.default_rng(5)
    return s[rng.choice(len(s), 2000, replace=False)]


# (source, search, eps, max_iter, expected repeats: the count the issue states for this case, None = whatever the record holds)
CASES = [
    ("full", po.DIRECT26, 1e-3, 35, 7),
    ("small", po.DIRECT7, 1e-3, 35, 9),
    ("small", po.DIRECT1, 1e-3, 35, 9),
    ("small", po.DIRECT1, 1e-9, 28, 8),
    ("full", po.DIRECT7, 0.01, 35, 0),
]


def request_key(kind, T, p):
    return (int(kind), np.ascontiguousarray(T, dtype=np.float32).tobytes(), np.ascontiguousarray(p, dtype=np.float64).tobytes())


def consecutive_same_kind_repeats(keys):
    """Requests equal to the last request of their kind before them."""
    last, n = {}, 0
    for k in keys:
        if last.get(k[0]) == k:
            n += 1
        last[k[0]] = k
    return n


@pytest.mark.parametrize("source,search,eps,max_iter,expected", CASES)
def test_reusing_driver_walks_the_plain_drivers_path(ndt, pair, source, search, eps, max_iter, expected):
    t, s = pair
    if source == "small":
        s = small_source(s)
    o = po.OracleNDT(resolution=1.0, search_method=search, num_threads=4, trans_eps=eps, max_iter=max_iter)
    o.set_target(t)
    o.set_source(s)
    s4 = np.c_[s, np.ones(len(s), np.float32)]
    record, order = {}, []

    def oracle_evaluator(kind, T, p):
        tc = po.transform_cloud(s4, T)
        if kind == 2:
            o.eval(p, False, tc)  # leaves the angle vectors at p, as the last computeDerivatives did
            ans = (0.0, np.zeros(6), np.array(o.hessian_f64(p), dtype=np.float64).copy())
        else:
            sc, g, H, _ = o.eval(p, kind == 0, tc)
            ans = (float(sc), np.array(g, dtype=np.float64).copy(), np.array(H, dtype=np.float64).copy())
        key = request_key(kind, T, p)
        order.append(key)
        record.setdefault(key, ans)  # a repeated request keeps its first answer: the recorded function is single-valued
        return record[key]

    plain = ndt.host_run_driver(oracle_evaluator, len(s), trans_eps=eps, max_iter=max_iter)
    assert len(order) == plain["n_evals"] + plain["n_hessian_recomputes"]  # one callback per evaluation, as ever
    repeats = consecutive_same_kind_repeats(order)
    if expected is not None:
        assert repeats == expected  # (so that no case is vacuous, and one case has none)

    calls = []

    def replay(kind, T, p):
        key = request_key(kind, T, p)
        assert key in record, "the reusing driver asked something the plain driver never asked"
        calls.append(key)
        return record[key]

    # the plain driver against the record: the walk the reusing driver is compared with sees the same function
    again = ndt.host_run_driver(replay, len(s), trans_eps=eps, max_iter=max_iter)
    assert calls == order
    del calls[:]
    got = ndt.host_run_driver(replay, len(s), trans_eps=eps, max_iter=max_iter, reuse=True)

    assert np.array_equal(got["T"].view(np.uint32), again["T"].view(np.uint32))
    for k in ("iterations", "n_evals", "n_hessian_recomputes", "trans_probability", "converged"):
        assert got[k] == again[k], k
    assert got["n_reused"] == repeats
    assert len(calls) == got["n_evals"] + got["n_hessian_recomputes"] - got["n_reused"]
    # and it asked exactly the plain walk's questions, minus the repeats, in order
    last, kept = {}, []
    for k in order:
        if last.get(k[0]) != k:
            kept.append(k)
        last[k[0]] = k
    assert calls == kept


def test_start_clears_the_memory(ndt):
    """Two runs of one evaluator: the second run's first request equals the first run's, and must be asked again."""
    n = [0]

    def flat(kind, T, p):
        n[0] += 1
        return 0.0, np.zeros(6), np.zeros((6, 6))

    for _ in range(2):
        r = ndt.host_run_driver(flat, 10, reuse=True)
        assert r["n_reused"] == 0 and r["n_evals"] == 1
    assert n[0] == 2


def test_only_the_same_kind_counts(ndt):
    """A quadratic bowl whose line search ends at the clamp: kinds 0, 1 and 2 are asked at one pose, and none of them is
    served from another kind's answer -- every reused step repeats a request of its own kind."""
    A = np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    p_star = np.array([0.05, -0.03, 0.02, 0.01, -0.02, 0.015])
    seen = []

    def bowl(kind, T, p):
        seen.append(request_key(kind, T, p))
        d = p - p_star
        return -0.5 * d @ A @ d, -(A @ d), -A

    plain = ndt.host_run_driver(bowl, 1, trans_eps=1e-6, max_iter=50)
    order = list(seen)
    del seen[:]
    got = ndt.host_run_driver(bowl, 1, trans_eps=1e-6, max_iter=50, reuse=True)
    assert np.array_equal(got["T"], plain["T"])
    for k in ("iterations", "n_evals", "n_hessian_recomputes", "trans_probability", "converged"):
        assert got[k] == plain[k], k
    assert got["n_reused"] == consecutive_same_kind_repeats(order)
    assert len(seen) == len(order) - got["n_reused"]
