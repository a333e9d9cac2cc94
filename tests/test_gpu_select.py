"""GPU: ndt_cloud_select / ndt_cloud_select_clouds / ndt_source_select_by_nvtl against the numpy restatement of the predicate
(tests/select_cases.py) and the definition of the boxes (tests/cloud_box_cases.reference_boxes).  Every comparison is exact --
record bits, order, indices, counts, boxes -- except the app's printed transform (1e-5, as the other app tests).

Sizes come from selectPlan: either side of a wave, of a block of threads, of a block's points, of the point count at which
the block cap is reached and points_per_block first grows, and of its next step.  A keep pattern is given to the device as a
key per point (1.0 keep, 0.0 drop) under the key range [0.5, 1.5], so that any pattern can be asked for."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import cloud_box_cases as cbc
import score_poses_cases as spc
import select_cases as sc
from test_gpu_centroid_fitness import app_settings
from test_gpu_pairs import build_app

pytestmark = pytest.mark.gpu

F = np.float32
KEEP_KEYS = dict(key_range=(0.5, 1.5))


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import _lib, ndt
    return ndt, _lib, built_lib


@pytest.fixture(scope="module")
def g(mods):
    return mods[0].NormalDistributionsTransform()


def raw(g, dc):
    """the cloud's 16-byte records as (n, 4) uint32"""
    n = len(dc)
    out = np.zeros((max(n, 1), 4), dtype=F)
    assert g._L.ndt_cloud_download(g._h, dc._c, out.ctypes.data, 16) == 0
    return out[:n].view(np.uint32).copy()


def xyz_of(records):
    return records.view(F)[:, :3]


def check_selection(g, records, mask, got, idx=None, what=None):
    """got = the selection of the cloud with `records` (n, 4) uint32 under the (n,) bool mask: records, order, indices, boxes, route"""
    want = records[mask]
    have = raw(g, got)
    assert len(got) == int(mask.sum()) and have.shape == want.shape, what
    assert np.array_equal(have, want), what
    if idx is not None:
        assert idx.dtype == np.int32 and np.array_equal(idx, np.flatnonzero(mask)), what
    boxes, route = got.bounds()
    ref = cbc.reference_boxes(xyz_of(want))
    assert cbc.same_boxes(boxes, ref), (what, cbc.boxes_text(boxes, ref))
    assert route == ("select" if mask.any() else "none"), (what, route)
    if not mask.any():
        assert cbc.same_boxes(boxes, cbc.EMPTY_BOXES)


def select_by_mask(g, dc, mask, **kw):
    return g.selectCloud(dc, keys=mask.astype(np.float64), indices=True, **KEEP_KEYS, **kw)


# ---------------------------------------------------------------------------------------------------- sizes and patterns
SIZE_NAMES = ("0", "1", "wave-1", "wave", "wave+1", "threads-1", "threads", "threads+1", "block-1", "block", "block+1", "two blocks",
              "two blocks+1", "five blocks+77", "cap", "cap+1", "step", "step+1")


def plan_sizes(plan):
    """name -> point count, from the plan itself (looked up inside the tests: the library is built by then)"""
    blocks1, ppb = plan(1)
    assert blocks1 == 1
    top = 300000
    assert plan(top)[1] > ppb + 1, "the block cap is not reached below 300 k points: these sizes do not cover it"

    def last_with(p):                                  # the largest n whose plan still has points_per_block == p
        lo, hi = 1, top
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if plan(mid)[1] <= p else (lo, mid - 1)
        return lo
    n_cap, n_step = last_with(ppb), last_with(ppb + 1)
    assert plan(n_cap + 1)[1] == ppb + 1 and plan(n_step + 1)[1] == ppb + 2
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, ppb - 1, ppb, ppb + 1, 2 * ppb, 2 * ppb + 1, 5 * ppb + 77, n_cap, n_cap + 1, n_step, n_step + 1]
    return dict(zip(SIZE_NAMES, sizes))


_clouds = {}


def cloud_of(n):
    """a cloud of n records with 12 distinct owners of the box values, NaN rows, and garbage behind z (cached)"""
    if n not in _clouds:
        hot = cbc.spread_hot(n)
        nan_rows = [r for r in (n // 3, n // 2 + 1) if 0 <= r < n and r not in hot]
        rec, owners = cbc.build_cloud(n, hot, floats=3, variant=cbc.VARIANTS[n % len(cbc.VARIANTS)], seed=n, nan_rows=nan_rows)
        _clouds[n] = (rec, owners)
    return _clouds[n]


def patterns(n, plan):
    blocks, ppb = plan(n)
    rng = np.random.default_rng(n + 1)
    out = {"all": np.ones(n, bool), "none": np.zeros(n, bool)}
    if n == 0:
        return out

    def only(*rows):
        m = np.zeros(n, bool)
        m[[r for r in rows if 0 <= r < n]] = True
        return m
    b = blocks // 2
    out["first"] = only(0)
    out["last"] = only(n - 1)
    out["first of a block"] = only(b * ppb)
    out["last of a block"] = only(min(n, (b + 1) * ppb) - 1)
    out["last of every block"] = only(*[min(n, (k + 1) * ppb) - 1 for k in range(blocks)])
    out["alternating"] = (np.arange(n) % 2).astype(bool)
    out["random half"] = rng.random(n) < 0.5
    wave = np.zeros(n, bool)                      # one whole wave of a block's pass, its neighbours empty
    w0 = b * ppb + 64 if b * ppb + 128 <= n else 0
    wave[w0:w0 + 64] = True
    out["one wave"] = wave
    owners = np.zeros(n, bool)                    # the 12 box values each owned by a different kept point, and a random third
    owners[list(cloud_of(n)[1].values())] = True
    out["box owners"] = owners | (rng.random(n) < 0.3)
    out["box owners only"] = owners
    return out


@pytest.mark.parametrize("size", SIZE_NAMES)
def test_keep_patterns_at_the_plan_boundaries(mods, g, size):
    plan = g.selectPlan
    n = plan_sizes(plan)[size]
    rec, owners = cloud_of(n)
    dc = g.uploadCloud(rec)
    records = raw(g, dc)
    assert np.array_equal(xyz_of(records).view(np.uint32), rec.view(np.uint32))
    for name, mask in patterns(n, plan).items():
        got, idx = select_by_mask(g, dc, mask)
        check_selection(g, records, mask, got, idx, (n, name))
        d = g.selectDiag()
        assert d == dict(launches=2 if n else 0, blocks=plan(n)[0], clouds=1), (n, name, d)
        if name.startswith("box owners") and len(owners) == 12:
            cbc.check_owners(xyz_of(records[mask]), {s: int(np.flatnonzero(np.flatnonzero(mask) == r)[0]) for s, r in owners.items()})
        got.release()
    # flags == 0: a copy, with boxes of its own
    got, idx = g.selectCloud(dc, indices=True)
    check_selection(g, records, np.ones(n, bool), got, idx, (n, "no flags"))
    assert n == 0 or got.data_ptr() != dc.data_ptr()


# ---------------------------------------------------------------------------------------------------- predicates
def test_edge_rows_under_every_test_on_the_device(mods, g):
    ndt, _lib, L = mods
    xyz, keys = sc.edge_cloud()
    big_xyz, big_keys = sc.random_cloud(3001, 9, odd_every=7)
    rng = np.random.default_rng(77)
    specs = sc.edge_specs() + [sc.random_spec(rng) for _ in range(25)]
    for pts, ks in ((xyz, keys), (big_xyz, big_keys)):
        dc = g.uploadCloud(pts)
        records = raw(g, dc)
        for s in specs:
            mask = sc.keep_mask(s, pts, ks)
            got, idx = g.selectCloud(dc, spec=sc.to_ctypes(s, _lib.SelectSpec), keys=ks, indices=True)
            check_selection(g, records, mask, got, idx, s)
    # the keyword form says the same
    dc = g.uploadCloud(xyz)
    records = raw(g, dc)
    got = g.selectCloud(dc, finite=True, range=(1, 5))
    check_selection(g, records, sc.keep_mask(sc.spec(sc.FINITE | sc.RANGE, r_min=1, r_max=5), xyz), got)
    got = g.selectCloud(dc, box=sc.BOX_UNIT, box_negate=True, range=(0, 5), centre=(1, 0, 0), range_negate=True, keys=keys, key_range=(0.25, 1),
                        key_negate=True)
    s = sc.spec(sc.BOX | sc.BOX_NEGATE | sc.RANGE | sc.RANGE_NEGATE | sc.KEY | sc.KEY_NEGATE, box_min=sc.BOX_UNIT[0], box_max=sc.BOX_UNIT[1],
                centre=(1, 0, 0), r_min=0, r_max=5, key_lo=0.25, key_hi=1)
    check_selection(g, records, sc.keep_mask(s, xyz, keys), got)


def test_refusals_with_a_cloud_in_hand(mods, g):
    ndt, _lib, L = mods
    dc = g.uploadCloud(sc.edge_cloud()[0])
    for s in sc.invalid_specs():
        out, nk = C.c_void_p(0x5A5A), C.c_size_t(77)
        bad = sc.to_ctypes(s, _lib.SelectSpec)
        assert L.ndt_cloud_select(g._h, dc._c, C.byref(bad), None, 0, C.byref(out), None, C.byref(nk)) == _lib.NDT_ERR_INVALID
        assert out.value is None and nk.value == 77
    keyed = sc.to_ctypes(sc.spec(sc.KEY, key_lo=0, key_hi=1), _lib.SelectSpec)
    out, nk = C.c_void_p(0x5A5A), C.c_size_t(77)
    assert L.ndt_cloud_select(g._h, dc._c, C.byref(keyed), None, 0, C.byref(out), None, C.byref(nk)) == _lib.NDT_ERR_INVALID  # KEY without keys
    assert out.value is None and nk.value == 77
    assert L.ndt_cloud_select(g._h, dc._c, None, None, 0, C.byref(out), None, C.byref(nk)) == _lib.NDT_ERR_INVALID
    outs, arr = (C.c_void_p * 2)(0x5A5A, 0x5A5A), (C.c_void_p * 2)(dc._c, None)
    ok = sc.to_ctypes(sc.spec(sc.FINITE), _lib.SelectSpec)
    assert L.ndt_cloud_select_clouds(g._h, arr, 2, C.byref(ok), outs, None) == _lib.NDT_ERR_INVALID            # a NULL entry
    assert outs[0] is None and outs[1] is None
    arr = (C.c_void_p * 2)(dc._c, dc._c)
    assert L.ndt_cloud_select_clouds(g._h, arr, 2, C.byref(keyed), outs, None) == _lib.NDT_ERR_INVALID         # KEY is refused
    with pytest.raises(ValueError):
        g.selectCloud(dc, keys=np.zeros(3), key_range=(0, 1))


# ---------------------------------------------------------------------------------------------------- input kinds
RANGE_SPEC = dict(finite=True, range=(2.0, 9.0), centre=(0.5, -0.5, 0.0))


def range_mask(xyz):
    return sc.keep_mask(sc.spec(sc.FINITE | sc.RANGE, centre=RANGE_SPEC["centre"], r_min=2.0, r_max=9.0), xyz)


def check_range(g, dc, kind, what):
    assert dc.bounds()[1] == kind, (what, dc.bounds()[1])
    records = raw(g, dc)
    mask = range_mask(xyz_of(records))
    assert 0 < mask.sum() < len(mask), what
    got, idx = g.selectCloud(dc, indices=True, **RANGE_SPEC)
    check_selection(g, records, mask, got, idx, what)
    return got, records[mask]


def test_every_kind_of_input_cloud(mods, g, tmp_path):
    ndt = mods[0]
    pts, _ = sc.random_cloud(30011, 4, odd_every=11)
    check_range(g, g.uploadCloud(pts[:5000]), cbc.upload_route(5000, 12), "uploaded (host route)")
    check_range(g, g.uploadCloud(pts), cbc.upload_route(30011, 12), "uploaded (device route)")
    filt, _ = g.voxelGridFilterCloud(pts, 0.7, is_dense=False)
    sel, want = check_range(g, filt, "filter_rows", "filter output")
    outs, _ = g.voxelGridFilterClouds([pts[:9000], pts[9000:9001], pts[9001:]], 0.7, is_dense=False)
    check_range(g, outs[0], "multi_words", "slice of a batched filter")
    check_range(g, outs[2], "multi_words", "slice of a batched filter")
    # a selection of a selection
    again, want2 = check_range(g, g.selectCloud(g.uploadCloud(pts), finite=True, range=(0, 11)), "select", "a selection")
    assert np.array_equal(raw(g, again), want2)
    # a staged scan: selected, then overwritten by the next scan -- the selection is a cloud of its own
    finite = pts[np.isfinite(pts).all(1)]
    for k, part in enumerate((finite[:12000], finite[12000:20000] + F(3)), 1):
        ndt.pcd_write_xyz(str(tmp_path / ("cloud_%d.pcd" % k)), part)
    seq = ndt.PcdSequence(str(tmp_path))
    seq.stage(0)
    assert seq.poll(0) == 2
    view = seq.next_cloud(g)[0]
    sel, want = check_range(g, view, "staged", "staged scan")
    view2 = seq.next_cloud(g)[0]
    check_range(g, view2, "staged", "the next staged scan")
    assert np.array_equal(raw(g, sel), want)
    boxes, route = sel.bounds()
    assert cbc.same_boxes(boxes, cbc.reference_boxes(xyz_of(want))) and route == "select"


# ---------------------------------------------------------------------------------------------------- consumers
def test_a_selection_is_the_cloud_an_upload_of_the_selected_rows_would_be(mods, pair):
    ndt = mods[0]
    t, s = pair
    mask = range_mask(s)
    assert 0 < mask.sum() < len(s)

    def both(make):
        """the same steps on two fresh handles: with the selection, with the upload of the host-selected rows"""
        res = []
        for form in ("select", "upload"):
            h = ndt.NormalDistributionsTransform()
            dc = h.selectCloud(h.uploadCloud(s), **RANGE_SPEC) if form == "select" else h.uploadCloud(s[mask])
            res.append(make(h, dc))
        return res
    # the records themselves, the fourth word included
    a, b = both(lambda h, dc: (raw(h, dc), dc.bounds()[0]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    def as_source(h, dc):
        h.setInputTarget(t)
        h.setInputSourceCloud(dc)
        h.align()
        return h.getFinalTransformation().tobytes(), h.getFinalNumIteration(), h.hasConverged()
    a, b = both(as_source)
    assert a == b

    def as_target(h, dc):
        h.setInputTargetCloud(dc)
        return h.grid()
    a, b = both(as_target)
    assert set(a) == set(b) and len(a["idx"]) > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k

    def through_filter(h, dc):
        h.voxelGridFilterBegin(dc, 0.5)
        out, ov = h.voxelGridFilterEnd()
        return raw(h, out), ov
    a, b = both(through_filter)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and len(a[0]) > 0

    def through_map(h, dc):
        h.mapUpdateCloud(dc, leaf_size=0.5)
        return h.mapGet()
    a, b = both(through_map)
    assert a.tobytes() == b.tobytes() and len(a) > 0

    def through_accumulate(h, dc):
        h.targetAccumulateCloud(dc)
        return bytes(h.targetAccumulateExport())
    a, b = both(through_accumulate)
    assert a == b and len(a) > 0


# ---------------------------------------------------------------------------------------------------- many clouds
def ragged(k):
    pts, _ = sc.random_cloud(9000, 12, odd_every=13)
    far = (pts[:300] + F(500)).astype(F)                                   # keeps nothing under RANGE_SPEC
    parts = [pts[:4097], pts[:0], far, pts[4097:4098], pts[4098:], pts[:0]]
    return {1: [parts[0]], 2: [parts[1], parts[4]], 5: parts[:5], 6: parts}[k]


@pytest.mark.parametrize("k", (1, 2, 5, 6))
def test_many_clouds_match_the_single_call(mods, g, k):
    parts = ragged(k)
    for order in (list(range(len(parts))), list(range(len(parts)))[::-1]):
        ins = [g.uploadCloud(parts[j]) for j in order]
        outs = g.selectClouds(ins, **RANGE_SPEC)
        d = g.selectDiag()
        assert d["launches"] == 2 and d["clouds"] == len(parts) and d["blocks"] == sum(g.selectPlan(len(parts[j]))[0] for j in order)
        singles = []
        for j, dc, out in zip(order, ins, outs):
            records = raw(g, dc)
            check_selection(g, records, range_mask(parts[j]), out, None, (k, j))
            one = g.selectCloud(dc, **RANGE_SPEC)
            assert np.array_equal(raw(g, one), raw(g, out)) and np.array_equal(one.bounds()[0], out.bounds()[0]) and one.bounds()[1] == out.bounds()[1]
            singles.append(raw(g, one))
        # the slices go one by one, in either order, while the others stay readable
        release = list(range(len(outs))) if order[0] == 0 else list(range(len(outs)))[::-1]
        for step, pos in enumerate(release):
            outs[pos].release()
            for other in release[step + 1:]:
                assert np.array_equal(raw(g, outs[other]), singles[other])
    assert g.selectClouds([], finite=True) == []


# ---------------------------------------------------------------------------------------------------- the NVTL form
def nvtl_mask(L, min_l, keep_unfound):
    found = L >= 0
    return (found & (L >= min_l)) | (~found & bool(keep_unfound))


def check_nvtl_form(g, src, T, what, thresholds=None):
    """sourceSelectByNVTL against the numpy selection of sourcePointNVTL's values, and against selectCloud with those values
    as device-resident keys"""
    L, _, n_found = g.sourcePointNVTL(T)
    found = L >= 0
    assert found.sum() == n_found and (L[~found] == -1.0).all() and 0 < n_found, what
    records = raw(g, g.uploadCloud(src))
    mid = float(np.sort(L[found])[n_found // 2])
    for min_l in thresholds or (-2.0, 0.0, mid, np.nextafter(mid, 1.0), float(L.max()), float(np.nextafter(L.max(), 1.0)), float("inf")):
        for keep_unfound in (True, False):
            mask = nvtl_mask(L, min_l, keep_unfound)
            got, nf = g.sourceSelectByNVTL(min_l, T, keep_unfound=keep_unfound)
            assert nf == n_found, what
            check_selection(g, records, mask, got, None, (what, min_l, keep_unfound))
            # the same through the public key test: found = 0 <= k
            dptr = g.sourcePointNVTL(T, device=True)[0]
            dc = g.uploadCloud(src)
            if keep_unfound:
                kw = dict(key_range=(0.0, np.nextafter(min_l, 0.0)), key_negate=True) if min_l > 0 else {}
            else:
                kw = dict(key_range=(max(min_l, 0.0), float("inf")))
            by_keys, idx = g.selectCloud(dc, keys=dptr, indices=True, **kw)
            check_selection(g, records, mask, by_keys, idx, (what, min_l, keep_unfound, "device keys"))
            assert np.array_equal(raw(g, by_keys), raw(g, got))
    return L


def test_source_select_by_nvtl_on_the_golden_pair(mods, pair, golden):
    ndt, _lib, _ = mods
    t, s = pair
    T = spc.poses(golden)[spc.I_GOLDEN]
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(t)
    g.setInputSource(s)
    L = check_nvtl_form(g, s, T, "golden pair")
    assert (L >= 0).any() and (L < 0).any()          # both kinds of point are in the pair
    # transform=None: the last align's final transformation
    g.align()
    got, _ = g.sourceSelectByNVTL(0.0, keep_unfound=False)
    Lf = g.sourcePointNVTL()[0]
    check_selection(g, raw(g, g.uploadCloud(s)), Lf >= 0, got, None, "final transformation")
    # a source with NaN rows (never found) and rows far from every voxel
    spoiled = spc.spoiled(s[:4000])
    g.setInputSource(spoiled)
    Ls = check_nvtl_form(g, spoiled, T, "spoiled source")
    assert (Ls[~np.isfinite(spoiled[:, :3]).all(1)] == -1.0).all()
    # an empty source
    g.setInputSource(s[:0])
    got, nf = g.sourceSelectByNVTL(0.5, T)
    assert len(got) == 0 and nf == 0 and got.bounds()[1] == "none"
    with pytest.raises(ndt.NdtError) as e:
        g.sourceSelectByNVTL(float("nan"), T)
    assert e.value.status == _lib.NDT_ERR_INVALID
    h = ndt.NormalDistributionsTransform()
    with pytest.raises(ndt.NdtError) as e:
        h.sourceSelectByNVTL(0.5, T)
    assert e.value.status == _lib.NDT_ERR_NO_INPUT


def test_source_select_by_nvtl_keeps_the_callers_order_of_an_ordered_source(mods, pair, golden):
    ndt = mods[0]
    t, s = pair
    T = spc.poses(golden)[spc.I_GOLDEN]
    rng = np.random.default_rng(70)
    big = (s[rng.integers(0, len(s), 70000)] + rng.normal(0, 0.02, (70000, 3))).astype(F)   # above the size sources are ordered from
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(t)
    g.setInputSource(big)
    L = g.sourcePointNVTL(T)[0]
    mid = float(np.median(L[L >= 0]))
    check_nvtl_form(g, big, T, "ordered source", thresholds=(mid,))


def test_source_select_by_nvtl_against_an_accumulated_target(mods, pair, golden):
    ndt = mods[0]
    t, s = pair
    T = spc.poses(golden)[spc.I_GOLDEN]
    g = ndt.NormalDistributionsTransform()
    g.targetAccumulate(t)
    g.setInputSource(s[:6000])
    acc0 = g.targetAccumulated()
    L = g.sourcePointNVTL(T)[0]
    check_nvtl_form(g, s[:6000], T, "accumulated target", thresholds=(float(np.median(L[L >= 0])),))
    assert g.targetAccumulated() == acc0
    # what the app does with it: the explained points go into the target at the pose
    kept, _ = g.sourceSelectByNVTL(float(np.median(L[L >= 0])), T)
    g.targetAccumulateCloud(kept, T)
    assert g.targetAccumulated() != acc0


# ---------------------------------------------------------------------------------------------------- untouched state
def test_the_calls_change_nothing_of_the_handle(mods, pair):
    ndt = mods[0]
    t, s = pair
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(t)
    g.setInputSource(s)
    g.align()
    g.mapUpdate(s[:3000], leaf_size=0.5)
    g.getNVTL()
    g.scorePoses([np.eye(4)])
    pending = g.uploadCloud(s[:5000])
    ref_filtered = raw(g, g.voxelGridFilterCloud(s[:5000], 0.5)[0])
    g.voxelGridFilterBegin(pending, 0.5)

    def state():
        return (g.getFinalTransformation().tobytes(), g.hasConverged(), g.getFinalNumIteration(), g.getTransformationProbability(),
                repr(g.stats()), g.grid_counts(), g.inputBounds("source")[0].tobytes(), g.inputBounds("source")[1], g.inputBounds("target")[0].tobytes(),
                g.mapSize(), g.scorePosesLaunches())
    before, nvtl_before = state(), g.nvtlLaunches()
    dc = g.uploadCloud(s)
    g.selectCloud(dc, **RANGE_SPEC)
    g.selectCloud(dc, keys=np.arange(len(s), dtype=np.float64), key_range=(10, 500), indices=True)
    g.selectClouds([dc, g.uploadCloud(s[:100])], **RANGE_SPEC)
    g.selectDiag()
    assert state() == before and g.nvtlLaunches() == nvtl_before
    g.sourceSelectByNVTL(0.1)
    assert state() == before          # (the NVTL form is an NVTL call: nvtlLaunches reports it)
    assert g.nvtlLaunches()[0] == 1
    out, ov = g.voxelGridFilterEnd()
    assert np.array_equal(raw(g, out), ref_filtered) and not ov
    T0 = g.getFinalTransformation().tobytes()
    g.align()
    assert g.getFinalTransformation().tobytes() == T0


# ---------------------------------------------------------------------------------------------------- the app
def test_map_sequence_range_and_reject(mods, reference_pcd, tmp_path):
    ndt = mods[0]
    d = tmp_path / "pcd"
    d.mkdir()
    scans = []
    for k, path in enumerate(reference_pcd, 1):
        xyz, _ = ndt.pcd_read_xyz(path)
        scans.append(np.ascontiguousarray(xyz[:, :3], dtype=F))
        with open(path, "rb") as src, open(str(d / ("cloud_%d.pcd" % k)), "wb") as dst:
            dst.write(src.read())
    exe = build_app(tmp_path, "map_sequence")
    L_MIN = 0.05
    plain = subprocess.check_output([exe, "--scan-to-map", str(d)], text=True)
    ranged = subprocess.check_output([exe, "--scan-to-map", "--range", "1", "30", str(d)], text=True)
    rejecting = subprocess.check_output([exe, "--scan-to-map", "--reject-unexplained", str(L_MIN), str(d)], text=True)
    assert "range kept:" not in plain and "rejected:" not in plain
    assert "rejected:" not in ranged and "range kept:" not in rejecting
    for args in (["--reject-unexplained", "0.05", str(d)], ["--range", "1", "30", str(d)],
                 ["--scan-to-map", "--load-target", str(tmp_path / "none.bin"), "--localize", "--reject-unexplained", "0.05", str(d)],
                 ["--scan-to-map", "--range", "5", "1", str(d)], ["--scan-to-map", "--reject-unexplained"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage: map_sequence" in r.stderr, args

    def transforms(out):
        lines = out.splitlines()
        return [np.array([[float(x) for x in lines[i + 1 + r].split()] for r in range(4)]) for i, ln in enumerate(lines) if ln.startswith("Transform ")]
    # --range: the same loop in Python, with the app's settings
    spec = sc.spec(sc.FINITE | sc.RANGE, r_min=1, r_max=30)
    kept = [tuple(int(x) for x in m) for m in re.findall(r"^range kept: (\d+)/(\d+)$", ranged, re.M)]
    assert kept == [(int(sc.keep_mask(spec, x).sum()), len(x)) for x in scans] and all(0 < a < b for a, b in kept)
    g = ndt.NormalDistributionsTransform()
    app_settings(g)
    want, prev = [], np.eye(4, dtype=F)
    for k, x in enumerate(scans):
        g.voxelGridFilterBegin(g.selectCloud(g.uploadCloud(x), finite=True, range=(1, 30)), 0.5)
        dc, _ = g.voxelGridFilterEnd()
        if k == 0:
            g.targetAccumulateCloud(dc)
            continue
        g.setInputSourceCloud(dc)
        g.align(prev)
        assert g.hasConverged()
        prev = g.getFinalTransformation().astype(F)
        want.append(prev)
        g.targetAccumulateCloud(dc, prev)
    got = transforms(ranged)
    print("range: app", got, "python", want)
    assert len(got) == len(want) == 1 and np.abs(got[0] - want[0]).max() <= 1e-5
    # --reject-unexplained: the count of the Python loop
    g = ndt.NormalDistributionsTransform()
    app_settings(g)
    want, prev = [], np.eye(4, dtype=F)
    for k, x in enumerate(scans):
        dc, _ = g.voxelGridFilterCloud(x, 0.5)
        if k == 0:
            g.targetAccumulateCloud(dc)
            continue
        g.setInputSourceCloud(dc)
        g.align(prev)
        assert g.hasConverged()
        prev = g.getFinalTransformation().astype(F)
        explained, _ = g.sourceSelectByNVTL(L_MIN)
        want.append((len(dc) - len(explained), len(dc)))
        g.targetAccumulateCloud(explained, prev)
    got = [tuple(int(x) for x in m) for m in re.findall(r"^rejected: (\d+)/(\d+)$", rejecting, re.M)]
    print("rejected: app", got, "python", want)
    assert got == want and len(got) == 1 and 0 < got[0][0] < got[0][1]
    assert [ln for ln in plain.splitlines() if ln.startswith("Loaded")] == [ln for ln in rejecting.splitlines() if ln.startswith("Loaded")]
