"""GPU: GICP against a voxel target (gicp_set_input_target_grid): the target set D and its covariances on every form of grid, the
correspondence step against two references, registrations, a live map, and what must stay untouched.

The anchor is the existing, oracle-pinned GICP path.  For a map M the REFERENCE route is a fresh GICP handle whose target cloud
is D's centroids (gicp_target_grid_voxels) with D's covariances (gicp_set_target_covariances); the NEW route binds M.  Both
searches are exact with the same f32 distance and the same tie rule and the algebra behind them is shared, so the two agree BIT FOR
BIT.  Independently of any library search, the correspondences equal numpy brute force over D (tests/gicp_grid_cases.correspond).

Bounds: RAW covariances within 1e-11 of max|cov| of the dump's cov (the project's standing f64 bound; condition <= 1 / eig_ratio =
100); PLANE by properties -- symmetric, eigenvalues {eps, 1, 1} to 1e-12, and the recovered normal an eigenvector of icov's largest
eigenvalue to 1e-9 relative (the bound the project holds icov to)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import centroid_fitness_cases as cc
import fitness_cases as fc
import gicp_grid_cases as gc
import gicp_grid_child as run
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
RAW_REL, PLANE_EIG, PLANE_RES = 1e-11, 1e-12, 1e-9
STOP = []   # set when a child process was ended by a signal or a time limit: no further child is started


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import gicp, ndt
    return ndt, gicp


def bucket_points():
    rng = np.random.default_rng(13)
    return (rng.random((66000, 3)) * [60, 60, 4]).astype(F)      # ~4.6 points a cell: voxels either side of min_pts


def grid_forms(ndt):
    """name -> (make a map handle, make its twin).  The twin is dumped (the dump rewrites records), the map is bound."""
    u = cc.mixed_target()
    rng = np.random.default_rng(14)
    small = cc.voxel_points([(i, j, 0) for i in range(5) for j in range(4)], rng, pts=7)
    rej = gc.rejected_case()[0]
    box = ([0.0, 0.0, 0.0], [5.0, 4.0, 2.0])

    def cropped(form):
        m = run.make_map(ndt, u, form)
        m.targetAccumulateCrop(*box)
        return m

    def imported(form):
        a = run.make_map(ndt, u, form)
        blob = a.targetAccumulateExport()
        m = ndt.NormalDistributionsTransform()
        m.setResolution(1.0)
        m.setMinPointPerVoxel(6)
        m.setVoxelIndex(form[1])
        m.targetAccumulateImport(blob)
        return m

    return {
        "one-launch": lambda: run.make_map(ndt, [small], ("cloud", 0)),
        "buckets-uncompacted": lambda: run.make_map(ndt, [bucket_points()], ("cloud", 1)),
        "cloud-dense": lambda: run.make_map(ndt, u, ("cloud", 1)),
        "cloud-sparse": lambda: run.make_map(ndt, u, ("cloud", 2)),
        "acc-dense": lambda: run.make_map(ndt, u, ("acc", 1)),
        "acc-sparse": lambda: run.make_map(ndt, u, ("acc", 2)),
        "acc-first-update": lambda: run.make_map(ndt, u[:1], ("acc", 1)),
        "rejected-dense": lambda: run.make_map(ndt, [rej], ("cloud", 1)),
        "rejected-acc-sparse": lambda: run.make_map(ndt, [rej], ("acc", 2)),
        "cropped-dense": lambda: cropped(("acc", 1)),
        "cropped-sparse": lambda: cropped(("acc", 2)),
        "imported-dense": lambda: imported(("acc", 1)),
        "imported-sparse": lambda: imported(("acc", 2)),
    }


FORM_NAMES = ("one-launch", "buckets-uncompacted", "cloud-dense", "cloud-sparse", "acc-dense", "acc-sparse", "acc-first-update",
              "rejected-dense", "rejected-acc-sparse", "cropped-dense", "cropped-sparse", "imported-dense", "imported-sparse")


# ------------------------------------------------------------------------------------------------ 1. D and its covariances
@pytest.mark.parametrize("name", FORM_NAMES)
def test_target_set_and_covariances_of_every_grid_form(mods, name):
    ndt, gicp = mods
    make = grid_forms(ndt)[name]
    m, twin = make(), make()
    if name == "buckets-uncompacted":
        gb = m.gridBuild()
        assert gb["form"] == "buckets" and gb["compact_pending"], gb
    g = gicp.GeneralizedIterativeClosestPoint()
    g.setInputTargetGrid(m, "raw")
    xyz1, raw, idx = g.targetGridVoxels()
    if name == "buckets-uncompacted":
        assert m.gridBuild()["compact_pending"]                              # read as it is: nothing was compacted for us
    dump = twin.grid()
    in_d = gc.target_set(dump["n"], 6)
    assert np.array_equal(idx, dump["idx"][in_d]), name                     # the valid voxels, ascending; rejected and under-min_pts absent
    assert len(idx) and (np.diff(idx) > 0).all()
    if name.startswith("rejected"):
        assert (dump["n"] == -1).sum() == 1 and ((dump["n"] > 0) & (dump["n"] < 6)).any()
    if "acc" in name or name.startswith("cloud"):
        assert ((dump["n"] > 0) & (dump["n"] < 6)).any()                    # the fixture has a voxel under min_pts
    cxyz1, cidx = m.gridCentroids()
    at = np.searchsorted(cidx, idx)
    assert np.array_equal(cidx[at], idx)
    assert xyz1.tobytes() == cxyz1[at].tobytes(), name                      # the same bits as ndt_grid_centroids
    cov, icov = dump["cov"][in_d], dump["icov"][in_d]
    dev = np.abs(raw - cov).reshape(len(cov), -1).max(axis=1) / np.abs(cov).reshape(len(cov), -1).max(axis=1)
    mine = gc.cov_raw(icov)                                                 # the same cofactor inverse of the dump's icov, in numpy
    dev_inv = np.abs(raw - mine).reshape(len(cov), -1).max(axis=1) / np.abs(mine).reshape(len(cov), -1).max(axis=1)
    print("DEV %-22s voxels=%-6d raw rel=%.3g against the inverse of the dump's icov=%.3g" % (name, len(idx), dev.max(), dev_inv.max()))
    far = name.startswith("rejected")
    # (the rejected fixture lies 500 km out, where the f32 sums of a voxel cancel and depend on the order they were taken in: the
    # twin's dump recomputes them and is no reference for the VALUES there -- measured 6e-10 and, in one voxel, 6e-4 between the
    # dump's icov and the records' -- so that fixture checks the index set, the centroid bits and the PLANE structure only)
    if not far:
        assert dev.max() <= RAW_REL and dev_inv.max() <= RAW_REL, name
    assert np.array_equal(raw, raw.transpose(0, 2, 1))
    assert np.array_equal(g.covariances(0), raw)                           # gicp_covariances(which = 0) on a grid target
    g.setInputTargetGrid(m, "plane")
    xyz1p, plane, idxp = g.targetGridVoxels()
    assert np.array_equal(idxp, idx) and xyz1p.tobytes() == xyz1.tobytes()
    asym, eig, res = gc.plane_defects(plane, icov)
    print("DEV %-22s plane asym=%.3g eig=%.3g residual=%.3g" % (name, asym, eig, res))
    assert asym == 0.0 and eig <= PLANE_EIG and (far or res <= PLANE_RES), name
    d = g.diagTargetGrid()
    assert d["voxels"] == len(idx) and d["refreshes"] == 2                 # one pass per binding, none for the repeated reads
    import ctypes as C
    from toyslam_amd import _lib
    small = np.full((max(len(idx) - 1, 1), 4), 7.0, F)
    cnt = C.c_size_t(0)
    st = g._L.gicp_target_grid_voxels(g._h, small.ctypes.data_as(C.POINTER(C.c_float)), None, None, len(idx) - 1, C.byref(cnt))
    assert st == _lib.NDT_ERR_INVALID and cnt.value == len(idx) and (small == 7.0).all()   # capacity < *n: *n written, no array is


def test_an_empty_target_set_and_a_map_without_target(mods):
    ndt, gicp = mods
    from toyslam_amd import _lib
    src = np.zeros((30, 3), F) + np.arange(30, dtype=F)[:, None]
    for form in (("cloud", 1), ("acc", 2)):
        m = run.make_map(ndt, cc.under_target(), form)                      # every voxel under min_pts: D is empty
        g = run.new_route(gicp, m, "plane", src)
        for call in (g.align, g.targetGridVoxels, lambda: g.step_correspond(), g.getFitnessScore, lambda: g.covariances(0)):
            with pytest.raises(_lib.NdtError) as e:
                call()
            assert e.value.status == _lib.NDT_ERR_NO_INPUT
    g = run.new_route(gicp, ndt.NormalDistributionsTransform(), "plane", src)
    with pytest.raises(_lib.NdtError) as e:
        g.align()
    assert e.value.status == _lib.NDT_ERR_NO_INPUT


# ------------------------------------------------------------------------------------------------ 2. the correspondence step
def check_steps(gicp, m, mode, src, src_cov, gate, what, T=None, D=None):
    """new route == reference route bit for bit (corr, maha, f and g in the three modes), and corr == brute force over D"""
    gn = run.new_route(gicp, m, mode, src, src_cov, gate)
    vox = gn.targetGridVoxels()
    gr = run.ref_route(gicp, vox, src, src_cov, gate)
    cn, corr_n, maha_n = gn.step_correspond(None, T)
    cr, corr_r, maha_r = gr.step_correspond(None, T)
    q = src if T is None else gc.matvec_eigen(T, src)
    want, d2 = gc.correspond(vox[0][:, :3], q, gate)
    bad = np.nonzero(corr_n != want)[0]
    assert len(bad) == 0, "%s: %d of %d differ from brute force, first %d: got %d want %d (d2 %r)" % (
        what, len(bad), len(src), bad[0], corr_n[bad[0]], want[bad[0]], d2[bad[0]])
    assert np.array_equal(corr_n, corr_r) and cn == cr == int((want >= 0).sum()), what
    has = want >= 0
    assert maha_n[has].tobytes() == maha_r[has].tobytes(), what
    if D is not None:
        assert np.array_equal(vox[0][:, :3], D), what
    if cn:
        x = np.array([0.02, -0.01, 0.03, 0.002, -0.001, 0.0015])
        for fmode in (0, 1, 2):
            fn, gn_ = gn.step_functor(fmode, x)
            fr, gr_ = gr.step_functor(fmode, x)
            assert fn == fr and gn_.tobytes() == gr_.tobytes(), "%s functor mode %d" % (what, fmode)
    assert gn.diagTargetGrid()["correspond_blocks"] == gn.plan(len(src))["correspond_blocks"]
    return corr_n, d2


def test_every_source_size_against_both_references(mods):
    ndt, gicp = mods
    u = cc.mixed_target()
    pts = np.concatenate(u)
    D, _, _ = gc.d_of(pts)
    m = run.make_map(ndt, u, ("acc", 1))
    pool = gc.query_pool(D, pts, 1.0, 31)
    rng = np.random.default_rng(32)
    for n in gc.SIZES:
        src = pool[rng.permutation(len(pool))[:n]]
        for T in (None, gc.rotation()):
            check_steps(gicp, m, "plane", src, gc.spd(n, 100 + n), 5.0, "n=%d %s" % (n, "I" if T is None else "R"), T, D)


TARGETS = ("mixed-dense", "mixed-sparse", "mixed-acc-sparse", "one", "two", "three", "line", "plane", "block")


@pytest.mark.parametrize("name", TARGETS)
def test_every_kind_of_query_and_gate(mods, name):
    ndt, gicp = mods
    if name.startswith("mixed"):
        u = cc.mixed_target()
        form = {"mixed-dense": ("cloud", 1), "mixed-sparse": ("cloud", 2), "mixed-acc-sparse": ("acc", 2)}[name]
    else:
        u = [cc.voxel_points(cc.shape_targets()[name], np.random.default_rng(5), pts=8)]
        form = ("cloud", 1) if name in ("one", "line", "block") else ("acc", 2)
    pts = np.concatenate(u)
    D, _, _ = gc.d_of(pts)
    assert len(D) == {"one": 1, "two": 2, "three": 3}.get(name, len(D))
    m = run.make_map(ndt, u, form)
    q = gc.query_pool(D, pts, 1.0, 40, 80)
    cov = gc.spd(len(q), 41)
    seen_far = seen_none = False
    for gate in gc.GATES:                                                   # 1e-6 m .. 1e6 m: the early -1, and the pass over the table
        corr, d2 = check_steps(gicp, m, "raw" if gate == 5.0 else "plane", q, cov, gate, "%s gate %g" % (name, gate), None, D)
        seen_none |= bool((corr == -1).all())
        seen_far |= bool((corr[np.isfinite(d2) & (d2 > 1e9)] >= 0).any())
    assert seen_none and seen_far, name                                     # nothing under the smallest gate; 100 km away under the largest
    check_steps(gicp, m, "plane", q, cov, 40.0, name + " rotated", gc.rotation(), D)


def test_ties_and_the_gate_at_one_ulp(mods):
    ndt, gicp = mods
    pts, q = cc.tie_target()
    D, _, _ = gc.d_of(pts)
    for form in (("cloud", 1), ("cloud", 2), ("acc", 1), ("acc", 2)):
        m = run.make_map(ndt, [pts], form)
        corr, _ = check_steps(gicp, m, "plane", q, gc.spd(len(q), 50), 1e3, "tie %s" % (form,), None, D)
        assert (corr == 0).all()                                           # equal d2: the lower linear voxel index
        on_sphere = np.array([[-0.5, 0.5, 0.5]], F)                        # d2 == 4 exactly
        g_at, g_up, g_lo, g_hi = gc.gate_steps(4.0)
        for gate, want in ((g_at, -1), (g_up, 0), (g_lo, -1), (g_hi, 0)):
            corr, d2 = check_steps(gicp, m, "plane", on_sphere, gc.spd(1, 51), gate, "gate %r %s" % (gate, form), None, D)
            assert d2[0] == 4.0 and corr[0] == want
    rng = np.random.default_rng(52)                                        # general distances: the gate just under and just over d2
    u = cc.mixed_target()
    m = run.make_map(ndt, u, ("acc", 1))
    Dm, _, _ = gc.d_of(np.concatenate(u))
    for p in (rng.random((6, 3)) * [8, 6, 3]).astype(F):
        one = np.array([p], dtype=F)
        v = fc.nearest_d2(Dm, one)[0][0]
        g_at, g_up, _, _ = gc.gate_steps(v)
        for gate, ok in ((g_at, False), (g_up, True)):
            corr, _ = check_steps(gicp, m, "plane", one, gc.spd(1, 53), gate, "gate at d2 %r" % v, None, Dm)
            assert (corr[0] >= 0) == ok


def test_rejected_under_and_drifted_voxels(mods):
    ndt, gicp = mods
    pts, cell, q = gc.rejected_case()                                      # the nearest centroid is a REJECTED voxel: passed over
    D, _, dcells = gc.d_of(pts, rejected_cells=[cell])
    for form in (("cloud", 1), ("acc", 2)):
        m = run.make_map(ndt, [pts], form)
        rng = np.random.default_rng(16)
        more = (np.asarray(cell, np.float64) + [-6, -6, -3] + rng.random((120, 3)) * [12, 12, 6]).astype(F)
        allq = np.concatenate([q, more])
        corr, _ = check_steps(gicp, m, "plane", allq, gc.spd(len(allq), 60), gc.REJECTED_GATE, "rejected %s" % (form,), None, D)
        assert (corr[:len(q)] >= 0).all()
    u, q = gc.under_case()                                                 # an accumulated target whose nearest voxel is under min_pts
    for upd in (u[:1], u):
        Du, _, cells = gc.d_of(np.concatenate(upd))
        for index in (1, 2):
            m = run.make_map(ndt, upd, ("acc", index))
            corr, _ = check_steps(gicp, m, "raw", q, gc.spd(len(q), 61), 5.0, "under %d updates" % len(upd), None, Du)
            assert (corr >= 0).all() and not (cells[corr] == (5, 1, 1)).all(axis=1).any()
    pts, cell, q = gc.excursion_case()                                     # a centroid outside its own cell, found from its neighbours
    De, _, cells = gc.d_of(pts)
    me = int(np.nonzero((cells == np.asarray(cell)).all(axis=1))[0][0])
    for form in (("cloud", 1), ("cloud", 2), ("acc", 1)):
        m = run.make_map(ndt, [pts], form)
        corr, _ = check_steps(gicp, m, "plane", q, gc.spd(len(q), 62), 5.0, "excursion %s" % (form,), None, De)
        assert (corr == me).sum() >= 20
        g = run.new_route(gicp, m, "plane", q[:32])
        g.step_correspond()
        assert g.diagTargetGrid()["excursion"] == pytest.approx(cc.excursion_of(De, cells), abs=0.0)


# ------------------------------------------------------------------------------------------------ 3. registration
@pytest.fixture(scope="module")
def registrations(mods, pair):
    ndt, gicp = mods
    return run.registration_run(ndt, gicp, pair[0], pair[1])


def test_registration_equals_the_reference_route(mods, pair, registrations):
    ndt, gicp = mods
    target, source = pair
    src = np.ascontiguousarray(source[:run.N_SOURCE], dtype=F)
    pieces, poses = run.pieces_and_poses(target)
    maps = {"grid": run.make_map(ndt, [target.astype(F)], ("cloud", 0)), "accumulated": run.make_map(ndt, pieces, ("acc", 0), poses=poses)}
    for name, m in maps.items():
        for mode in ("plane", "raw"):
            vox = run.new_route(gicp, m, mode, src).targetGridVoxels()
            for k, guess in enumerate(run.guesses()):
                new = run.registration(run.new_route(gicp, m, mode, src), guess)
                ref = run.registration(run.ref_route(gicp, vox, src), guess)
                print("REG %-11s %-5s guess %d: it=%d conv=%s corr=%d fitness=%.6f" % (name, mode, k, new["iterations"], new["converged"],
                                                                                       new["stats"][3], new["fitness"]))
                assert run.same_registration(new, ref), (name, mode, k, new, ref)
                assert new["stats"][3] > run.N_SOURCE // 2 and new["fitness"] < 1.0
                if name == "grid":
                    assert run.same_registration(new, registrations["%s%d" % (mode, k)])     # and a repeat gives the same bits


def run_child(tmp_path, **env):
    if STOP:
        pytest.fail("not started: an earlier child process " + STOP[0])
    out = tmp_path / "child.json"
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gicp_grid_child.py"), str(out)], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=150, cwd=ROOT)
    except subprocess.TimeoutExpired:
        STOP.append("ran into its time limit")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        STOP.append("ended by a signal (%d)" % r.returncode)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    import json
    with open(out) as f:
        return run.unhexed(json.load(f))


@pytest.mark.parametrize("env", [dict(NDT_GICP_MAX_BLOCKS=str(gc.MAX_BLOCKS_CHILD)), dict(NDT_GICP_SERVER="0"), dict(NDT_GICP_NO_FUSE="1")],
                         ids=["max-blocks-3", "no-server", "no-fuse"])
def test_development_switches_change_no_bit(mods, tmp_path, registrations, env):
    ndt, gicp = mods
    got = run_child(tmp_path, **env)
    for key, want in registrations.items():
        assert run.same_registration(got["registrations"][key], want), (env, key)
    mine = run.step_run(ndt, gicp)
    u = cc.mixed_target()
    D, _, _ = gc.d_of(np.concatenate(u))
    for key, a in mine.items():
        b = got["steps"][key]
        n = len(a["src"])
        assert np.array_equal(a["src"], b["src"]) and np.array_equal(a["corr"], b["corr"]), (env, key)
        has = a["corr"] >= 0
        assert a["maha"][has].tobytes() == b["maha"][has].tobytes() and a["f"] == b["f"] and a["g"].tobytes() == b["g"].tobytes(), (env, key)
        q = a["src"] if key.endswith("I") else gc.matvec_eigen(gc.rotation(), a["src"])
        assert np.array_equal(b["corr"], gc.correspond(D, q, 5.0)[0]), (env, key)          # the child against brute force, too
        if "NDT_GICP_MAX_BLOCKS" in env:
            assert b["blocks"] == b["plan"] == gc.correspond_blocks(n, gc.MAX_BLOCKS_CHILD)
            assert a["blocks"] == gc.correspond_blocks(n)


# ------------------------------------------------------------------------------------------------ 4. a live map
def test_live_map_every_align_reads_the_map_as_it_is(mods, pair):
    ndt, gicp = mods
    target, source = pair
    src = np.ascontiguousarray(source[:run.N_SOURCE], dtype=F)
    pieces, poses = run.pieces_and_poses(target)
    box = ([-30.0, -30.0, -10.0], [20.0, 30.0, 10.0])
    other = target[::2].astype(F)

    def state(k):
        """a map handle taken through the first k changes"""
        m = ndt.NormalDistributionsTransform()
        m.setResolution(1.0)
        m.targetAccumulate(pieces[0], poses[0])
        if k >= 1:
            m.targetAccumulateCloud(m.uploadCloud(pieces[1]), poses[1])
        if k >= 2:
            m.targetAccumulateCrop(*box)
        if k >= 3:
            m.setInputTarget(other, is_dense=True)
        return m

    live = state(0)
    g = run.new_route(gicp, live, "plane", src)
    seen = 0
    for k in range(4):
        if k == 1:
            live.targetAccumulateCloud(live.uploadCloud(pieces[1]), poses[1])
        elif k == 2:
            live.targetAccumulateCrop(*box)
        elif k == 3:
            live.setInputTarget(other, is_dense=True)
        got = run.registration(g, None)
        d = g.diagTargetGrid()
        assert d["refreshes"] == seen + 1, (k, d)                          # one pass per change ...
        again = run.registration(g, None)
        assert g.diagTargetGrid()["refreshes"] == seen + 1                 # ... and none on a repeated align
        seen += 1
        fresh = run.registration(run.new_route(gicp, state(k), "plane", src), None)
        assert run.same_registration(got, fresh) and run.same_registration(again, fresh), k
        print("LIVE state %d: voxels=%d it=%d corr=%d" % (k, d["voxels"], got["iterations"], got["stats"][3]))
    n_before = g.diagTargetGrid()["voxels"]
    g.step_correspond()
    live.targetAccumulate(pieces[2], poses[2])                             # (setInputTarget dropped the accumulated target: a new one)
    from toyslam_amd import _lib
    with pytest.raises(_lib.NdtError) as e:
        g.step_functor(0, np.zeros(6))                                     # the ordinals of the step mean nothing in the new D
    assert e.value.status == _lib.NDT_ERR_NO_INPUT and g.diagTargetGrid()["voxels"] != n_before


# ------------------------------------------------------------------------------------------------ 5. what stays untouched
def test_the_map_handle_and_the_pairs_calls_are_left_as_they_were(mods, pair):
    ndt, gicp = mods
    target, source = pair
    src = np.ascontiguousarray(source[:run.N_SOURCE], dtype=F)
    m = run.make_map(ndt, [target.astype(F)], ("cloud", 0))
    m.setInputSource(src)
    m.align(None)
    p = np.array([0.05, -0.02, 0.01, 0.002, -0.001, 0.003])

    def snapshot():
        s, grad, H, nn = m.eval(p)
        return (s, grad.tobytes(), H.tobytes(), nn, tuple(sorted(m.grid_counts().items())), m.getFinalTransformation().tobytes(),
                repr(m.stats()), m.gridCentroids()[0].tobytes())

    before = snapshot()
    g = run.new_route(gicp, m, "plane", src)
    run.registration(g, run.guesses()[1])
    g.step_correspond()
    g.targetGridVoxels()
    assert snapshot() == before
    up = ndt.NormalDistributionsTransform()
    dcs = [up.uploadCloud(np.ascontiguousarray(c[:1500], dtype=F)) for c in (target, source)]
    with_binding = g.alignPairsClouds(dcs, None, None, 1.0)
    h = gicp.GeneralizedIterativeClosestPoint()
    without = h.alignPairsClouds(dcs, None, None, 1.0)
    for key in with_binding:
        assert np.asarray(with_binding[key]).tobytes() == np.asarray(without[key]).tobytes(), key
    after_pairs = run.registration(g, None)                                # the binding survives a pairs call
    assert run.same_registration(after_pairs, run.registration(run.new_route(gicp, m, "plane", src), None))
    g.setInputTarget(target[:3000])                                        # a cloud target drops the binding
    from toyslam_amd import _lib
    with pytest.raises(_lib.NdtError) as e:
        g.targetGridVoxels()
    assert e.value.status == _lib.NDT_ERR_NO_INPUT
    assert snapshot() == before


# ------------------------------------------------------------------------------------------------ 6. the app
def test_map_sequence_gicp_follows_the_same_loop_in_python(mods, tmp_path):
    """apps/map_sequence --scan-to-map --gicp on synthetic PCD files against the same loop here: prefilter, GICP against the
    accumulated target from the previous pose, accumulate at the result; --map-fitness moves the scan by the GICP result"""
    ndt, gicp = mods
    from test_gpu_pairs import build_app, matrices, sequence
    from toyslam_amd import clouds
    scans, d = sequence(clouds, ndt, tmp_path, n=3)
    m = ndt.NormalDistributionsTransform()
    m.setResolution(1.0)
    filt = [m.voxelGridFilter(sc, 0.5)[:, :3] for sc in scans]
    g = gicp.GeneralizedIterativeClosestPoint()
    g.setInputTargetGrid(m, "plane")
    g.setMaxCorrespondenceDistance(3.0)
    pose = np.eye(4, dtype=F)
    m.targetAccumulate(filt[0], pose)
    result, fitness = [], []
    for k in range(1, 3):
        g.setInputSource(filt[k])
        g.align(pose)
        assert g.hasConverged()
        pose = g.getFinalTransformation().astype(F)
        fitness.append(m.batchCentroidFitness([filt[k]], transforms=[pose])[0])
        m.targetAccumulate(filt[k], pose)
        result.append(pose)
    exe = build_app(tmp_path, "map_sequence")
    r = subprocess.run([exe, "--scan-to-map", "--gicp", "--gicp-gate", "3", "--map-fitness", str(d)], capture_output=True, text=True, timeout=120)
    if r.returncode < 0:
        pytest.fail("map_sequence ended by a signal (%d): %s" % (r.returncode, r.stderr[-1500:]))
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    step, traj = matrices(out, "Transform "), matrices(out, "trajectory[")
    assert len(step) == 2 and len(traj) == 2 and "registrations 2 (not converged 0)" in out
    printed = [float(ln.split(":")[1]) for ln in out.splitlines() if ln.startswith("map fitness:")]
    for k in range(2):
        assert np.abs(step[k] - result[k]).max() < 1e-5, k
        assert np.array_equal(step[k], traj[k])
        assert printed[k] == pytest.approx(fitness[k], rel=1e-5)
    assert np.abs(result[1][:3, 3]).max() > 0.05                           # the scans do move
    for bad in (["--gicp", str(d)], ["--scan-to-map", "--gicp", "--nvtl", str(d)], ["--scan-to-map", "--gicp", "--covariance", str(d)],
                ["--scan-to-map", "--gicp", "--reject-unexplained", "0.1", str(d)], ["--scan-to-map", "--gicp-gate", "3", str(d)],
                ["--scan-to-map", "--gicp", "--gicp-gate", "0", str(d)], ["--scan-to-map", "--gicp", "--gicp-gate"]):
        b = subprocess.run([exe] + bad, capture_output=True, text=True, timeout=60)
        assert b.returncode == 2 and "usage: map_sequence" in b.stderr and "--gicp" in b.stderr, bad
