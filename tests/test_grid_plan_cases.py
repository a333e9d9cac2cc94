"""CPU: the cases of tests/test_gpu_grid_plans.py (tests/grid_plan_cases.py) -- that each sits where its name says under the
library's own plan (ndt_host_grid_plan, ndt_host_lattice: host code, no GPU), that the oracle's grid of its cloud has what
the case is about (the named voxel sizes, and at least 50 voxels with min_pts points and more, so that "the records agree" is
not vacuous), and that the comparator the GPU test uses rejects a grid with one count off by one or one mean off by one ulp."""
import numpy as np
import pytest

import grid_plan_cases as gpc


@pytest.fixture(scope="module")
def po(built_lib):
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


@pytest.fixture(scope="module")
def cases(built_lib):
    return gpc.all_cases()


def test_host_grid_plan_answers_without_a_device(built_lib):
    from toyslam_amd import ndt
    p = ndt.host_grid_plan(64 * 64 * 16, 60000, (64, 64, 16))
    assert p["bucket_form"] and not p["one_launch"] and p["n_buckets"] >= 8 and p["n_buckets"] % 8 == 0
    assert p["n_buckets"] * p["cells_per_bucket"] >= 64 * 64 * 16 and p["n_blocks"] % 8 == 0
    assert p["n_blocks"] * p["pts_per_block"] >= 60000 and 0 < p["wmax"] <= p["cells_per_bucket"] and p["lds_cap"] % 256 == 0
    assert p["lut_cells"] == 68 * 68 * 20 and p["compact_tiles"] * 256 * p["compact_items"] >= p["lut_cells"]
    q = ndt.host_grid_plan(64 * 64 * 16, 60000)
    assert q["lut_cells"] == 0 and q["compact_items"] == 0 and {k: q[k] for k in gpc.PLAN_FIELDS} == {k: p[k] for k in gpc.PLAN_FIELDS}
    assert not ndt.host_grid_plan(1 << 26, 60000)["bucket_form"]          # beyond the bucket form's range
    assert not ndt.host_grid_plan(1000, 0)["bucket_form"]
    with pytest.raises(ndt.NdtError):
        ndt.host_grid_plan(1000, 1 << 40)
    assert gpc.run_bits_hold()


def test_every_group_has_its_cases(cases):
    names = [c.name for g in "ABCD" for c in cases[g]]
    assert len(names) == len(set(names))
    # A: one-launch | buckets, last block full | one point, four steps of the bucket count; B: six steps of the cell count;
    # C: contents and the one-run cloud in three arrival orders, three alias clouds; D: three steps of ITEMS and the prefix pass
    assert [len(cases[g]) for g in "ABCD"] == [12, 12, 9, 8]
    assert len(gpc.group_e()) == 6
    forms = {c.expect["form"] for g in "ABCD" for c in cases[g]}
    assert forms == {"one_launch", "buckets", "sparse", "chain"}
    ks = sorted({c.expect["n_buckets"] for c in cases["A"] + cases["B"] if c.expect["form"] == "buckets"})
    assert ks[0] == 256 and ks[-1] == 8192 and len(ks) >= 5
    assert {c.expect["compact_items"] for c in cases["D"]} == {1, 2, 4, 8}
    assert {c.expect["compact_prefix"] for c in cases["D"]} == {False, True}
    assert any(not c.dense for c in cases["A"]) and any(c.dense for c in cases["A"])


def _case_ids():
    # (collected without the library: the names are fixed, the sizes behind them are found when the test runs)
    return ["%s%d" % (g, i) for g, k in zip("ABCD", (12, 12, 9, 8)) for i in range(k)]


@pytest.mark.parametrize("cid", _case_ids())
def test_case_sits_where_its_name_says_and_the_oracle_sees_it(cases, po, cid):
    case = cases[cid[0]][int(cid[1:])]
    for what, ok in case.claims:
        assert ok, (case.name, what)
    cloud = case.cloud()   # (asserts the size and, through host_lattice, the lattice)
    assert len(cloud) == case.n and int((~np.isfinite(cloud).all(axis=1)).sum()) == (0 if case.dense else 3)
    plan = gpc.plan_of(case.dims, case.n)
    if case.contents:
        for what, ok in case.contents(cloud, plan):
            assert ok, (case.name, what)
    og = gpc.oracle_for(po, case).grid()
    assert tuple(og["div_b"]) == case.dims
    assert int((og["n"] >= gpc.MIN_PTS).sum()) >= (50 if case.dims != (gpc.RUN, 1, 1) else gpc.RUN), case.name
    for cnt in case.counts:
        assert (og["n"] == cnt).any(), (case.name, cnt)
    # the oracle numbers cells as the dealing rule assumes: x fastest from the box's corner
    fin = np.isfinite(cloud).all(axis=1)
    assert np.array_equal(np.unique(gpc.cells_of(cloud, case.dims, case.origin)[fin]), og["idx"])
    # the comparator: itself, one count off by one, one mean off by one ulp
    assert gpc.grid_mismatch(og, og) is None
    k = int(np.argmax(og["n"] >= gpc.MIN_PTS))
    bad = dict(og, n=og["n"].copy())
    bad["n"][k] += 1
    assert gpc.grid_mismatch(bad, og) == "n differ"
    bad = dict(og, mean=og["mean"].copy())
    bad["mean"][k, 2] = np.nextafter(bad["mean"][k, 2], np.inf)
    assert (gpc.grid_mismatch(bad, og) or "").startswith("means not bit-exact")
    bad = dict(og, icov=og["icov"].copy())
    bad["icov"][k] *= 1 + 1e-6
    assert (gpc.grid_mismatch(bad, og) or "").startswith("icov differs")


def test_filter_cases_sit_where_their_names_say(built_lib, po):
    for name, dims, n, seed, claims in gpc.group_e():
        for what, ok in claims:
            assert ok, (name, what)
        cloud = gpc.mixed_cloud(seed, n, dims, seed % 2 == 0)
        assert tuple(gpc.lattice_of(cloud)["div_b"]) == dims
    ref, ov = po.voxel_grid_filter(cloud, gpc.LEAF, is_dense=seed % 2 == 0)
    assert not ov and len(ref) > 1000
