"""GPU: the target-grid build AT THE BOUNDARIES OF ITS PLAN, against the CPU oracle.

The bucket form of the build (k1_hist / k1_colscan / k1_scatter / k1_finalize), the one-launch form, the dense chain with
k_finalize, the sparse index, the record compaction and the voxel filter on the same front end each cut a cloud by a plan:
buckets and cells per bucket, points per block, passes of at most lds_cap points over windows of at most wmax cells, tiles of
the look-up table.  A tail point, a pass boundary or a rank bit that is wrong shows where a cloud sits ON a boundary of such a
plan, so the cases (tests/grid_plan_cases.py, with a CPU test of its own) are found by asking the library for its plan
(ndt_host_grid_plan) and every case first asserts, through gridBuild() = ndt_diag_grid_build, that the build took the form
and plan it is named for.  What is EXPECTED never comes from the plan: (b) the grid dump against the oracle's grid at the line
tools/fuzz_grid.py holds, and (c) -- the dump recomputes its sums and never reads the records the build wrote -- one
evaluation with Hessian of a 2000-point source drawn from the cloud: bit-identical to a handle with the other voxel index
form (sparse, or dense for the sparse case), and within close_sums (rel 2e-6) of the oracle's.

Largest deviations from the oracle per group are gathered in DEV and printed when the module is done (and written as JSON to
$GRID_PLAN_REPORT if that is set, with the plan each case reported); NOTES.md quotes them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_plan_cases as gpc
from conftest import ROOT
from test_gpu_parity import close_sums, mods  # noqa: F401  (mods: the fixture)

pytestmark = pytest.mark.gpu

COUNTS = dict(A=12, B=12, C=9, D=8)   # cases per group under the default plan (tests/test_grid_plan_cases.py asserts them)
DEV, PLANS = {}, {}


def note(group, what, value):
    k = group + "/" + what
    DEV[k] = max(DEV.get(k, 0.0), float(value))


def note_report(case, rep):
    PLANS[case.name] = {k: v for k, v in rep["build"].items() if v not in (0, False)}
    note(case.group, "eval", rep.get("eval_dev", 0.0))
    for k, v in rep.get("grid_dev", {}).items():
        note(case.group, k, v)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    text = json.dumps(dict(deviations=DEV, plans=PLANS), indent=1, sort_keys=True)
    print("\nlargest GPU-vs-oracle deviations per group:\n" + json.dumps(DEV, indent=1, sort_keys=True))
    if os.environ.get("GRID_PLAN_REPORT"):
        with open(os.environ["GRID_PLAN_REPORT"], "w") as f:
            f.write(text + "\n")


def ids(group):
    return ["%s%d" % (group, i) for i in range(COUNTS[group])]


def case_of(cid):
    cases = gpc.cases_of(cid[0])
    assert len(cases) == COUNTS[cid[0]], "the chooser found %d cases of group %s, not %d" % (len(cases), cid[0], COUNTS[cid[0]])
    return cases[int(cid[1:])]


@pytest.mark.parametrize("cid", ids("A") + ids("B") + ids("C"))
def test_build_on_a_plan_boundary_against_the_oracle(mods, cid):
    """Groups A (point count), B (cell count) and C (bucket contents, arrival orders, alias clouds): (a), (b), (c)."""
    ndt, po, _ = mods
    case = case_of(cid)
    fails, rep = gpc.check_case(ndt, po, case)
    print(case.name, json.dumps(rep["build"]), "other form:", rep.get("other_form"), "eval dev %.3g" % rep.get("eval_dev", -1),
          "grid dev", rep.get("grid_dev"))
    note_report(case, rep)
    assert not fails, (case.name, fails)
    assert rep["valid"] >= min(50, gpc.RUN if case.dims == (gpc.RUN, 1, 1) else 50)


@pytest.mark.parametrize("cid", ids("D"))
def test_record_compaction_on_a_tile_plan_boundary(mods, cid):
    """Group D: the compaction (k_rc_count / k_rc_scan / k_rc_apply) either side of every step of its tile plan.  Evaluation and f64
    Hessian as built, a first registration (records still as built), a second (compacted first): the same bits after as
    before, compact_pending from 1 to 0, and the compacted grid held to (b) and (c)."""
    ndt, po, _ = mods
    case = case_of(cid)
    g = gpc.handle_for(ndt, case)
    gb = g.gridBuild()
    print(case.name, json.dumps(gb))
    for k, v in case.expect.items():
        assert gb[k] == v, (case.name, k, gb[k], v)
    for what, ok in case.claims:
        assert ok, (case.name, what)
    assert gb["compact_pending"]
    src = gpc.source_of(case.cloud())
    g.setInputSource(src)
    g.setMaximumIterations(2)
    e0, h0 = g.eval(gpc.POSE, True), g.hessian_f64(gpc.POSE)
    g.align()
    assert g.gridBuild()["compact_pending"]
    g.align()
    assert not g.gridBuild()["compact_pending"]
    e1, h1 = g.eval(gpc.POSE, True), g.hessian_f64(gpc.POSE)
    assert gpc.evals_identical(e0, e1) and np.array_equal(h0, h1)
    g2 = gpc.handle_for(ndt, case, 2)
    g2.setInputSource(src)
    assert g2.gridBuild()["form"] == "sparse" and gpc.evals_identical(e1, g2.eval(gpc.POSE, True))
    o = gpc.oracle_for(po, case)
    og, gg = o.grid(), g.grid()
    assert gpc.grid_mismatch(gg, og) is None, gpc.grid_mismatch(gg, og)
    o.set_source(src)
    oe = o.eval(gpc.POSE, True)
    rep = dict(build=gb, eval_dev=gpc.eval_deviation(e1, oe), grid_dev=gpc.grid_deviation(gg, og))
    note_report(case, rep)
    note("D", "hessian_f64", gpc.eval_deviation((0.0, 0.0, h1), (0.0, 0.0, o.hessian_f64(gpc.POSE))))
    assert e1[3] == oe[3] and close_sums(e1[0], oe[0]) and close_sums(e1[1], oe[1]) and close_sums(e1[2], oe[2])
    assert close_sums(h1, o.hessian_f64(gpc.POSE))
    assert int((og["n"] >= gpc.MIN_PTS).sum()) >= 50


@pytest.mark.parametrize("k", range(6))
def test_voxel_filter_on_a_route_boundary(mods, k):
    """Group E: voxelGridFilter bit for bit against the oracle's pcl::VoxelGrid either side of the route choice (points, cells per
    point) and of one | two chunks of the bitmap prefix pass."""
    ndt, po, _ = mods
    name, dims, n, seed, claims = gpc.group_e()[k]
    for what, ok in claims:
        assert ok, (name, what)
    dense = seed % 2 == 0
    cloud = gpc.mixed_cloud(seed, n, dims, dense)
    assert tuple(gpc.lattice_of(cloud)["div_b"]) == dims
    ref, ov = po.voxel_grid_filter(cloud, gpc.LEAF, is_dense=dense)
    got = ndt.NormalDistributionsTransform().voxelGridFilter(cloud, gpc.LEAF, is_dense=dense)
    assert not ov and len(ref) > 1000 and got.shape == ref.shape
    assert np.array_equal(got, ref), (name, float(np.abs(got - ref).max()))


def run_child(env, group, names):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "grid_plan_child.py"), group] + list(names),
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    for row in rows:
        print(row["name"], json.dumps(row["build"]), row["eval_dev"])
        assert not row["fails"], (row["name"], row["fails"])
        note(group + "-switched", "eval", row["eval_dev"])
    return rows


def test_two_ranking_rounds_per_block(mods):
    """NDT_K1_PPB=4096: every block of the two point passes ranks its points in two rounds of 2048 (by default only above 1 M
    points); group A's first bucket-form size and its first size with a ballot bit."""
    names = ["A-one_launch_to_buckets-above", "A-K_step1-above"]
    rows = run_child(dict(NDT_K1_PPB="4096"), "A", names)
    assert [r["name"] for r in rows] == names
    assert all(r["build"]["form"] == "buckets" and r["build"]["pts_per_block"] == 4096 for r in rows)
    assert rows[0]["build"]["n_buckets"] == 256 and rows[1]["build"]["n_buckets"] == 512


def test_bucket_count_that_is_no_power_of_two(mods):
    """NDT_K1_BUCKETS=264: the multiply-high division of the dealing rule takes its correction step; all of group C (its contents
    are dealt by the plan of the child's own process)."""
    rows = run_child(dict(NDT_K1_BUCKETS="264"), "C", [])
    assert len(rows) == COUNTS["C"] and all(r["build"]["form"] == "buckets" for r in rows)
    ks = [r["build"]["n_buckets"] for r in rows]
    assert ks.count(264) == COUNTS["C"] - 1 and max(ks) == 8192   # (the largest lattice needs every bucket there is)
