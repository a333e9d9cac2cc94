"""GPU: every form of the score / gradient / Hessian kernels AT THE BOUNDARIES OF ITS BLOCK PLAN, against the CPU oracle.

The reduction exists in six forms (one-launch kernel, separate derivative + reduce kernels, all-f64 Hessian, persistent
evaluation server, lock-step batch, pairs), each with its own way of cutting a scan into blocks, lanes and per-thread runs.
A tail lane dropped or a point counted twice shows where a scan's size sits ON a boundary of such a plan, so the sizes here
are found by asking the library for its plan (evalPlan = ndt_diag_eval_plan; the chooser is tests/eval_plan_sizes.py and
has a CPU test of its own) and every case first asserts that it sits where it claims.  What is EXPECTED never comes from
the plan: it is the oracle's answer, so the file also holds under the switches that move the boundaries (NDT_K2_PPB,
NDT_K2_MAX_BLOCKS, NDT_PERSISTENT=0, NDT_K2_FUSED=0, NDT_SPIN_WAIT=0).

The forms that only a registration can reach (server, batch, pairs) are probed with iteration-limited registrations:
with the transformation epsilon at 0 and one or two permitted iterations the result is a function of a handful of
evaluations from the guess and nothing else -- a lost point moves it far more than it moves a converged registration.

Largest deviations from the oracle over the sweep are gathered in DEV and printed when the module is done (and written as
JSON to $EVAL_PLAN_REPORT if that is set); NOTES.md quotes them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_plan_sizes as eps
from conftest import ROOT, rot_err, trans_err
from test_gpu_parity import ROT_TOL, TRANS_TOL, close_sums, mods  # noqa: F401  (mods: the fixture)

pytestmark = pytest.mark.gpu

METHODS = ("DIRECT7", "DIRECT1", "DIRECT26", "KDTREE")
POSE = np.array([0.25, -0.15, 0.08, 0.008, -0.004, 0.015])  # 5 cm / a few mrad off the scene's T_gt: nothing cancels
HI = {0: 300000, 2: 40000}    # largest size looked at: whole device (the suite's largest oracle cloud) / side partition
ORDER_FROM = 65536            # a single scan of this many points is registered from an ordered copy WITHOUT its non-finite
#                               points (order_cloud); batch members and pair sources always are.  Smaller single scans keep
#                               them (the kernels skip them), so the plan is taken on the raw count there.
# One- and two-iteration transforms against the oracle: the project's line is ROT_TOL / TRANS_TOL (1e-4 / 1e-3 m); what the
# sweep measured is orders of magnitude below it, so this file asserts TEN TIMES THE LARGEST DEVIATION OBSERVED AGAINST THE
# ORACLE over the sweep (margin for another block order of the f64 sums), per form (NOTES.md, "Evaluation kernels at their
# block-plan boundaries"):
#   single scan (server and launch path alike): rotation 2.3e-9, translation 6.0e-8 m.  The transform is handed back in f32:
#     one ulp of a rotation entry next to 1 is 1.2e-7, so that is the floor of the rotation figure (ten times the observed
#     2.3e-9 would forbid the last bit of a diagonal entry from moving under another block order).
#   batch and pairs (the same figures for both, every group count): members of 512 points and more 1.9e-9 / 1.5e-8 m, held
#     to the single scan's figures; the ONE-POINT member 3.34e-7 / 1.16e-6 m after two iterations (a rank-deficient Hessian
#     through the SVD solve: the worst conditioned probe there is), a line of its own.
PROBE_TOL = {"scan": (1.2e-7, 6.0e-7), "one_point": (3.4e-6, 1.2e-5)}
DEV = {}


def note(form, what, value):
    k = form + "/" + what
    DEV[k] = max(DEV.get(k, 0.0), float(value))


def rel_dev(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    text = json.dumps(DEV, indent=1, sort_keys=True)
    print("\nlargest GPU-vs-oracle deviations, per form:\n" + text)
    if os.environ.get("EVAL_PLAN_REPORT"):
        with open(os.environ["EVAL_PLAN_REPORT"], "w") as f:
            f.write(text + "\n")


def sorts_single_scans(n_raw):
    mode = os.environ.get("NDT_SORT_SOURCE")
    return n_raw >= ORDER_FROM if mode is None else int(mode) != 0


def with_bad_points(pts, size, always_ordered):
    """A cloud whose EVALUATED count (what the plan is taken on) is `size`, with three non-finite points: where the scan is
    ordered they are dropped first, so three more raw points are taken; where it is not, they stay in their lanes (one of
    them the very last point: the tail lane).  -> (cloud, evaluated count)"""
    raw = size + 3 if (always_ordered or sorts_single_scans(size + 3)) else size
    c = pts[:raw].copy()
    c[raw // 3] = np.nan
    c[raw // 2, 1] = np.inf
    c[raw - 1, 2] = -np.inf
    ordered = always_ordered or sorts_single_scans(raw)
    return c, (int(np.isfinite(c).all(axis=1).sum()) if ordered else raw)


def is_bad_case(size):
    return size >= 7 and size % 3 == 1   # a third of the sizes carry NaN / inf points


class Rig:
    """One CU partition: the plan table of its handles, GPU handles per neighbour rule (one on the default evaluation path,
    one with a pass-through all-reduce hook = the separate derivative + reduce kernels), oracles, and caches of both sides'
    answers per size so that boundaries that share a size do not pay twice."""

    def __init__(self, mods, tgt, src, partition):
        self.ndt, self.po, _ = mods
        self.tgt, self.src, self.partition = tgt, src, partition
        self.handles, self.oracles, self.gpu, self.ora = {}, {}, {}, {}
        self.hook_calls = 0
        probe = self.handle("DIRECT7", False)
        self.partition_got, self.cus = probe.getCuPartition()
        self.hi = HI[partition]
        self.table = eps.plan_table(probe.evalPlan, self.hi)
        self.bounds = eps.boundaries(None, self.hi, table=self.table)
        print("\npartition %d: handle reports partition %d with %d CUs%s; boundaries %s" % (
            partition, self.partition_got, self.cus,
            " (no CU mask granted: the whole device's plan)" if partition and self.cus == self.rig_whole_cus() else "",
            json.dumps(self.bounds, sort_keys=True)))

    def rig_whole_cus(self):
        g = self.ndt.NormalDistributionsTransform()
        return g.getCuPartition()[1]

    def plan(self, n):
        return dict(zip(eps.FIELDS, (int(x) for x in self.table[n])))

    def handle(self, method, hook):
        if (method, hook) not in self.handles:
            g = self.ndt.NormalDistributionsTransform()
            if self.partition:
                g.setCuPartition(self.partition)
            g.setNeighborhoodSearchMethod(getattr(self.po, method))
            g.setInputTarget(self.tgt)
            if hook:
                def passthrough(buf, n, on_device):
                    self.hook_calls += 1
                    return 0
                g.setAllreduce(passthrough)
            self.handles[(method, hook)] = g
        return self.handles[(method, hook)]

    def oracle(self, method):
        if method not in self.oracles:
            o = self.po.OracleNDT(num_threads=16, search_method=getattr(self.po, method))
            o.set_target(self.tgt)
            self.oracles[method] = o
        return self.oracles[method]

    def cloud(self, size):
        if is_bad_case(size):
            c, count = with_bad_points(self.src, size, False)
        else:
            c, count = self.src[:size], size
        assert count == size, "the scan is not evaluated at the size the case is named for"
        return c

    def gpu_eval(self, method, hook, size):
        """-> dict(full=(score, grad, H, nn), no_h=(score, grad), h64=H or None), cached"""
        key = (method, hook, size)
        if key not in self.gpu:
            g = self.handle(method, hook)
            g.setInputSource(self.cloud(size))
            calls = self.hook_calls
            full = g.eval(POSE, True)
            no_h = g.eval(POSE, False)
            if hook:  # the separate derivative + reduce kernels ran: each evaluation handed its row to the hook once
                assert self.hook_calls == calls + 2, "the all-reduce hook did not see the two evaluations"
            assert no_h[2] is None
            h64 = g.hessian_f64(POSE) if (not hook and self.wants_h64(method, size)) else None
            self.gpu[key] = dict(full=full, no_h=no_h[:2], h64=h64)
        return self.gpu[key]

    @staticmethod
    def wants_h64(method, size):
        # the oracle's all-f64 Hessian is a serial loop (1 - 2 s per 260 k-point scan and neighbour rule): every rule up to
        # 70 k points, DIRECT7 (the default rule) at every size
        return method == "DIRECT7" or size <= 70000

    def oracle_eval(self, method, size):
        key = (method, size)
        if key not in self.ora:
            o = self.oracle(method)
            o.set_source(self.cloud(size))   # (the oracle skips non-finite points itself, as the reference does)
            self.ora[key] = dict(full=o.eval(POSE, True), h64=o.hessian_f64(POSE) if self.wants_h64(method, size) else None)
        return self.ora[key]


@pytest.fixture(scope="module")
def rigs(mods):
    _, _, clouds = mods
    tgt = clouds.target_surfaces(400000, extent=60.0, n_boxes=30)
    src = clouds.source_from_target(tgt, HI[0] + 8)
    made = {}

    def get(partition):
        if partition not in made:
            made[partition] = Rig(mods, tgt, src, partition)
        return made[partition]
    return get


def switches_move_the_plan():
    return any(k in os.environ for k in ("NDT_K2_PPB", "NDT_K2_MAX_BLOCKS"))


def assert_boundary_is_hit(rig, name, b):
    """The plan really changes at b in the respect `name` claims (a property of the library's answer, not of a formula)."""
    lo, at, end = rig.plan(b - 1), rig.plan(b), rig.plan(rig.hi)
    form = name.split("_")[0]
    f = form + "_blocks"
    if name.startswith("ppb_"):
        assert lo["ppb"] != at["ppb"]
        if name == "ppb_saturates":
            assert at["ppb"] == end["ppb"]
    elif name.endswith("_two_blocks"):
        assert (lo[f], at[f]) == (1, 2)
    elif name.endswith("_max"):
        assert at[f] == int(rig.table[1:, eps.FIELDS.index(f)].max()) and lo[f] < at[f]
    elif name.endswith("_cap"):
        assert lo[f] != at[f] and at[f] == end[f]
    elif name in ("fused_strided", "server_walk"):
        assert at[f] * at["ppb"] < b and lo[f] * lo["ppb"] >= b - 1
    elif name == "launch_strided":
        assert b > rig.bounds["launch_cap"] and lo[f] == at[f] == end[f]
    else:
        raise AssertionError("unknown boundary " + name)


def check_eval_sums(rig, size):
    """One size: the four neighbour rules, with and without the Hessian, on the default evaluation path (the one-launch
    kernel) and through the separate kernels (hook), and the all-f64 Hessian -- against the oracle, with the figures of
    test_eval_matches_oracle_and_golden; the translation blocks are compared on their own as well (close_sums scales by
    the largest entry: the rotational ones)."""
    for method in METHODS:
        want = rig.oracle_eval(method, size)
        so, go, Ho, nno = want["full"]
        for hook in (False, True):
            got = rig.gpu_eval(method, hook, size)
            form = "separate_kernels" if hook else "one_launch_kernel"
            ctx = "%s %s n=%d partition=%d" % (form, method, size, rig.partition)
            score, grad, H, nn = got["full"]
            s2, g2 = got["no_h"]
            print("%s: score rel %.3g  grad %.3g (xyz %.3g)  H %.3g (xyz %.3g)  no-H score %.3g grad %.3g" % (
                ctx, abs(score - so) / max(abs(so), 1e-300), rel_dev(grad, go), rel_dev(grad[:3], go[:3]), rel_dev(H, Ho),
                rel_dev(H[:3, :3], Ho[:3, :3]), abs(s2 - so) / max(abs(so), 1e-300), rel_dev(g2, go)))
            note(form, "sums_rel", max(rel_dev(grad, go), rel_dev(H, Ho), rel_dev(grad[:3], go[:3]), rel_dev(H[:3, :3], Ho[:3, :3]),
                                       rel_dev(g2, go), abs(score - so) / max(abs(so), 1e-300)))
            assert nn == nno, ctx                                   # neighbour search: exact
            assert score == pytest.approx(so, rel=1e-6), ctx
            assert close_sums(grad, go) and close_sums(H, Ho), ctx
            assert close_sums(grad[:3], go[:3]) and close_sums(H[:3, :3], Ho[:3, :3]), ctx
            assert np.array_equal(H, H.T), ctx
            assert s2 == pytest.approx(so, rel=1e-6) and close_sums(g2, go) and close_sums(g2[:3], go[:3]), ctx
            if got["h64"] is not None:
                note("f64_hessian", "sums_rel", rel_dev(got["h64"], want["h64"]))
                assert close_sums(got["h64"], want["h64"], rel=1e-11), ctx


def check_linearity(rig, b):
    """Sums over the first b + 1 points = sums over the first b + the sums of point b alone, and the same one point lower
    (figures of test_eval_linearity_in_points).  GPU against GPU: it would see a doubled or dropped boundary point even if
    kernel and oracle shared a mistake."""
    for hook in (False, True):
        g = rig.handle("DIRECT7", hook)
        for n in (b, b + 1):
            if n < 2:
                continue
            parts = []
            for c in (rig.src[:n], rig.src[:n - 1], rig.src[n - 1:n]):
                g.setInputSource(c)
                parts.append(g.eval(POSE, True))
            full, a, one = parts
            ctx = "n=%d hook=%d partition=%d" % (n, hook, rig.partition)
            assert full[0] == pytest.approx(a[0] + one[0], rel=1e-12), ctx
            assert np.allclose(full[1], a[1] + one[1], rtol=1e-10, atol=1e-9), ctx
            assert np.allclose(full[2], a[2] + one[2], rtol=1e-10, atol=1e-8), ctx
            assert full[3] * n == pytest.approx(a[3] * (n - 1) + one[3], abs=1e-6), ctx


PARTITIONS = pytest.mark.parametrize("partition", [0, 2], ids=["whole_device", "side_partition"])


@PARTITIONS
def test_eval_sums_at_small_sizes(rigs, partition):
    """1, 2, 7 points, the 64-lane edge (63, 64, 65) and a size that is no multiple of 8."""
    rig = rigs(partition)
    assert any(s % 8 for s in eps.SMALL_SIZES)
    for size in eps.SMALL_SIZES:
        check_eval_sums(rig, size)
    check_linearity(rig, 64)


@PARTITIONS
@pytest.mark.parametrize("name", eps.EVAL_BOUNDARIES)
def test_eval_sums_at_plan_boundaries(rigs, partition, name):
    rig = rigs(partition)
    b = rig.bounds.get(name)
    if b is None:
        # The plan has no such boundary below HI: legitimate only where a switch pins the plan (NDT_K2_PPB: ppb never
        # changes; NDT_K2_MAX_BLOCKS: a grid capped from the start), or on the side partition (the separate kernels' cap
        # lies at the same size as on the whole device, beyond this partition's range; without a CU mask the handle has the
        # whole device's plan).  On the whole device with no switch set every boundary must be there.
        assert partition != 0 or switches_move_the_plan(), "the whole device's plan lost its boundary " + name
        return
    assert_boundary_is_hit(rig, name, b)
    for size in (b - 1, b, b + 1):
        check_eval_sums(rig, size)
    check_linearity(rig, b)


def test_side_partition_reaches_the_grid_strided_regime(rigs):
    """With a CU mask granted the one-launch kernel's first two grid-strided sizes lie below the side partition's range
    (and are run by test_eval_sums_at_plan_boundaries[fused_strided]: b and b + 1); without one the handle says so."""
    whole, side = rigs(0), rigs(2)
    if side.cus == whole.cus:
        assert side.bounds.get("fused_strided") in (None, whole.bounds.get("fused_strided"))
        return
    if switches_move_the_plan():
        return
    b = side.bounds["fused_strided"]
    assert b + 1 < HI[2] and b < whole.bounds["fused_strided"]
    for n in (b, b + 1):
        p = side.plan(n)
        assert p["fused_blocks"] * p["ppb"] < n


# ------------------------------------------------------------------ server / launch path: iteration-limited registrations
def compare_registration(form, ctx, T, it, conv, tp, ro, tol="scan"):
    r, t = rot_err(T, ro["T"]), trans_err(T, ro["T"])
    note(form, "rot", r)
    note(form, "trans", t)
    tp_o = ro["trans_probability"]
    if not (np.isnan(tp) and np.isnan(tp_o)):
        note(form, "trans_probability_rel", abs(tp - tp_o) / max(abs(tp_o), 1e-300))
    print("%s: rot %.3g trans %.3g iterations %d/%d tp %.9g/%.9g" % (ctx, r, t, it, ro["iterations"], tp, tp_o))
    assert r < ROT_TOL and t < TRANS_TOL, ctx
    tight = PROBE_TOL[tol]
    assert r <= tight[0] and t <= tight[1], ctx
    assert it == ro["iterations"] and bool(conv) == ro["converged"], ctx
    assert tp == pytest.approx(tp_o, rel=1e-6, nan_ok=True), ctx   # (no source point: 0 / 0 on both sides)


@PARTITIONS
@pytest.mark.parametrize("name", ["server_two_blocks", "server_max", "server_cap", "server_walk"])
def test_limited_registrations_at_server_boundaries(mods, rigs, partition, name):
    """The persistent evaluation server (and, as its twin, the launch-per-evaluation path) where its grid goes to two
    blocks, first fills the CUs, settles, and where its threads start to walk several points."""
    ndt, po, _ = mods
    rig = rigs(partition)
    b = rig.bounds.get(name)
    if b is None:
        assert partition != 0 or switches_move_the_plan(), "the whole device's plan lost its boundary " + name
        return
    assert_boundary_is_hit(rig, name, b)
    g = ndt.NormalDistributionsTransform()
    if partition:
        g.setCuPartition(partition)
    g.setTransformationEpsilon(0.0)
    g.setInputTarget(rig.tgt)
    o = po.OracleNDT(num_threads=16, trans_eps=0.0)
    o.set_target(rig.tgt)
    for size in (b - 1, b, b + 1):
        c = rig.cloud(size)
        g.setInputSource(c)
        o.set_source(c)
        for max_iter in (1, 2):
            o.set(max_iter=max_iter)
            ro = o.align()
            g.setMaximumIterations(max_iter)
            for persistent in (True, False):
                g.setEvaluationPath(persistent)
                g.align()
                T, conv, it, tp = g._result()
                form = "server" if persistent else "launch_path"
                ctx = "%s n=%d max_iter=%d partition=%d" % (form, size, max_iter, partition)
                compare_registration(form + "/%d_iter" % max_iter, ctx, T, it, conv, tp, ro)
                assert g.stats()["n_evals"] == ro["n_evals"], ctx


# ------------------------------------------------------------------ batch and pairs
@pytest.fixture(scope="module")
def members(mods, pair, rigs):
    """The bundled target and a ragged set of sources whose EVALUATED sizes are the batch plan's boundaries: 0, 1, each
    of 1 -> 2, 2 -> 3 and 8 -> 9 blocks +- 1, and one a good deal above (more than 8 blocks for the XCD deal).  A third of
    them carry three non-finite points on top (a batch orders its scans and drops those first).  Every member is a random
    subset of the bundled source moved by its own small transform; odd members start from a guess."""
    _, _, clouds = mods
    t, s = pair
    rig = rigs(0)
    for name in eps.BATCH_BOUNDARIES:
        b = rig.bounds[name]
        assert rig.plan(b)["batch_blocks"] == rig.plan(b - 1)["batch_blocks"] + 1 == int(name.split("_")[1])
    sizes = eps.batch_member_sizes(rig.bounds, above=rig.bounds["batch_9_blocks"] + 903)
    assert len(sizes) == 12 and rig.plan(sizes[-1])["batch_blocks"] > 8
    scans, guesses = [], []
    for k, size in enumerate(sizes):
        rng = np.random.default_rng(7000 + k)
        bad = is_bad_case(size)
        sel = rng.choice(len(s), size + (3 if bad else 0), replace=False)
        c = clouds.apply_T(np.linalg.inv(clouds.random_T(rng, 0.2, 0.5)), s[sel]) if size else np.zeros((0, 3), np.float32)
        if bad:
            c, count = with_bad_points(c, size, True)
            assert count == size
        scans.append(c)
        guesses.append(np.eye(4, dtype=np.float32) if k % 2 == 0 else clouds.make_T([0.05, 0, 0], [0, 0, 0.002]).astype(np.float32))
    return t, s, sizes, scans, guesses


def oracle_aligns(po, target, scans, guesses, **kw):
    o = po.OracleNDT(num_threads=16, **kw)
    o.set_target(target)
    out = []
    for c, G in zip(scans, guesses):
        o.set_source(c)
        out.append(o.align(G))
    return out


@pytest.mark.parametrize("max_iter", [1, 2])
def test_limited_batch_at_batch_boundaries(mods, members, max_iter):
    """ndt_align_batch, member by member against the ORACLE (not the single-scan GPU path, which shares the kernel body),
    as one lock-step loop and as three groups."""
    ndt, po, _ = mods
    t, _, sizes, scans, guesses = members
    want = oracle_aligns(po, t, scans, guesses, trans_eps=0.0, max_iter=max_iter)
    g = ndt.NormalDistributionsTransform()
    g.setTransformationEpsilon(0.0)
    g.setMaximumIterations(max_iter)
    g.setInputTarget(t)
    for groups in (1, 3):
        g.setBatchGroups(groups)
        res = g.alignBatch(scans, guesses)
        for k, size in enumerate(sizes):
            ctx = "batch member %d n=%d max_iter=%d groups=%d" % (k, size, max_iter, groups)
            compare_registration("batch/%d_iter" % max_iter, ctx, res["T"][k], res["iterations"][k], res["converged"][k],
                                 res["trans_probability"][k], want[k], tol="one_point" if size == 1 else "scan")


@pytest.mark.parametrize("max_iter", [1, 2])
def test_limited_pairs_at_batch_boundaries(mods, members, max_iter):
    """ndt_align_pairs with an explicit pair list: every boundary-sized cloud as a source against the full-size target
    cloud, and one pair the other way round (a boundary-sized cloud as the target grid, the full cloud as its source)."""
    ndt, po, _ = mods
    t, _, sizes, scans, guesses = members
    cl = [t] + scans
    back = 1 + next(k for k, size in enumerate(sizes) if size > 1000 and not is_bad_case(size))  # (a target without NaN: is_dense)
    pairs = [(0, k + 1) for k in range(len(scans))] + [(back, 0)]
    G = guesses + [np.eye(4, dtype=np.float32)]
    want = oracle_aligns(po, t, scans, guesses, trans_eps=0.0, max_iter=max_iter)
    want += oracle_aligns(po, cl[back], [t], G[-1:], trans_eps=0.0, max_iter=max_iter)
    g = ndt.NormalDistributionsTransform()
    g.setTransformationEpsilon(0.0)
    g.setMaximumIterations(max_iter)
    for groups in (1, 3):
        g.setBatchGroups(groups)
        res = g.alignPairs(cl, pairs, G)
        for k, (a, b) in enumerate(pairs):
            ctx = "pair %d (target %d points, source %d) max_iter=%d groups=%d" % (k, len(cl[a]), len(cl[b]), max_iter, groups)
            compare_registration("pairs/%d_iter" % max_iter, ctx, res["T"][k], res["iterations"][k], res["converged"][k],
                                 res["trans_probability"][k], want[k], tol="one_point" if len(cl[b]) == 1 else "scan")


def test_long_batch_runs_mixed_steps_and_follows_the_oracle(mods, members):
    """A batch long enough (30 iterations at most, epsilon 1e-9, members of mixed size and difficulty) for k_batch_step to
    serve with-Hessian, without-Hessian and all-f64-Hessian requests in the same lock-step: the members finish after
    different numbers of iterations, all-f64 Hessians were recomputed, and the loop took fewer steps than the members'
    requests add up to.  Converged transforms: the project's own line against the oracle."""
    ndt, po, _ = mods
    t, _, sizes, scans, guesses = members
    keep = [k for k, size in enumerate(sizes) if size > 1000]   # (7 members: 8 to 29 iterations in the oracle)
    sc, G = [scans[k] for k in keep], [guesses[k] for k in keep]
    want = oracle_aligns(po, t, sc, G, trans_eps=1e-9, max_iter=30)
    g = ndt.NormalDistributionsTransform()
    g.setTransformationEpsilon(1e-9)
    g.setMaximumIterations(30)
    g.setInputTarget(t)
    g.setBatchGroups(1)
    g.profile(1)
    g.profile_read(0)
    res = g.alignBatch(sc, G)
    n_steps, ms = g.profile_read(0)
    g.profile(0)
    st = g.stats()
    for k in range(len(sc)):
        ctx = "long batch member n=%d" % sizes[keep[k]]
        r, tr = rot_err(res["T"][k], want[k]["T"]), trans_err(res["T"][k], want[k]["T"])
        note("batch/converged", "rot", r)
        note("batch/converged", "trans", tr)
        assert r < ROT_TOL and tr < TRANS_TOL, ctx
        assert bool(res["converged"][k]) == want[k]["converged"], ctx
        assert res["trans_probability"][k] == pytest.approx(want[k]["trans_probability"], rel=1e-5), ctx  # (the converged figure)
    assert len(set(int(i) for i in res["iterations"])) > 1          # members in different phases of their searches
    assert st["n_hessian_recomputes"] > 0 and st["n_evals"] >= sum(int(i) for i in res["iterations"])
    assert 0 < n_steps < st["n_evals"] + st["n_hessian_recomputes"] and ms > 0


# ------------------------------------------------------------------ every size grid-strided
def test_eval_sums_with_every_grid_capped_at_eight_blocks():
    """NDT_K2_MAX_BLOCKS=8 puts every size above a few thousand points into the grid-strided regime of the one-launch and of
    the separate kernels: the side partition's evaluation checks of this file once more, in a process of their own."""
    if os.environ.get("NDT_K2_MAX_BLOCKS"):
        return  # (this process already runs under the switch: the checks above are the strided ones)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_eval_plans.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", "side_partition and (small_sizes or plan_boundaries)"],
                       env=dict(os.environ, NDT_K2_MAX_BLOCKS="8", EVAL_PLAN_REPORT=""), capture_output=True, text=True,
                       timeout=280, cwd=ROOT)
    tail = r.stdout[-2500:] + r.stderr[-1500:]
    assert r.returncode == 0, tail
    last = r.stdout.strip().splitlines()[-1]
    assert " passed" in last and "skipped" not in last and "xfailed" not in last and "failed" not in last, tail
