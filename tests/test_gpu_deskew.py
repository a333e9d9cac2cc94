"""GPU: ndt_cloud_deskew / ndt_cloud_deskew_clouds against the numpy restatement of the definition (tests/deskew_cases.py) and
the definition of the boxes (tests/cloud_box_cases.reference_boxes).

Every finite, timed record, coordinate a:  |q_gpu[a] - q_ref64[a]| <= 1/2 ulp32(q_gpu[a]) + 64 * 2^-53 * (|p|_1 + |s| |tau_ref|_1)
-- the one final rounding, plus at most 12 rounded f64 operations per path and sin / cos at the device library's documented
2 ulp, on both sides, doubled for margin (deskew_cases.bound).  Bit for bit: fourth words, records with a non-finite
coordinate, the NaN-ing and the count of untimed points, both boxes, the route; s == 0 rows by ==.

Sizes: 1 point, either side of a wave and of a block of threads; one point either side of EVERY step of the plan up to and
including the block cap (k = 1 ... 1024 blocks: test_every_step_of_the_plan, 64 cases of 16 steps over prefixes of one
cloud); beyond the cap, where points_per_block grows (to values that are no multiple of a wave), the first two steps; the
strided regime of a block (several passes over its range) with NDT_DESKEW_MAX_BLOCKS=3 in a child process
(tests/deskew_child.py).  Every case asserts through deskewDiag() that one launch of the planned blocks ran."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cloud_box_cases as cbc
import deskew_cases as dc
from test_deskew_host import to_ctypes, write_pcd
from test_gpu_centroid_fitness import app_settings
from test_gpu_pairs import build_app

pytestmark = pytest.mark.gpu

F = np.float32
EPOCH = 1.7e9


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import _lib, ndt
    return ndt, _lib, built_lib


@pytest.fixture(scope="module")
def g(mods):
    return mods[0].NormalDistributionsTransform()


def raw(g, cloud):
    """the cloud's 16-byte records as (n, 4) uint32"""
    n = len(cloud)
    out = np.zeros((max(n, 1), 4), dtype=F)
    assert g._L.ndt_cloud_download(g._h, cloud._c, out.ctypes.data, 16) == 0
    return out[:n].view(np.uint32).copy()


def xyz_of(records):
    return records.view(F)[:, :3]


def check_output(g, rec, times, m, out, nu, what):
    """out = the deskew of the cloud with records rec (n, 4) uint32: bits, bound, count, boxes, route; -> its records"""
    got = raw(g, out)
    assert len(out) == len(rec), what
    assert dc.expected_records(rec, times, m, got) == nu, (what, nu)
    worst = dc.check_moved(xyz_of(got), rec.view(F), times, m, what)
    boxes, route = out.bounds()
    ref = cbc.reference_boxes(xyz_of(got))
    assert cbc.same_boxes(boxes, ref), (what, cbc.boxes_text(boxes, ref))
    assert route == ("deskew" if len(rec) else "none"), (what, route)
    return got, worst


def deskew_checked(mods, g, cloud, times, m, what, device_times=None):
    """one deskewCloud with the launch asserted first; m: a deskew_cases motion"""
    ndt, _lib, _ = mods
    rec = raw(g, cloud)
    if device_times is None:
        out, nu = g.deskewCloud(cloud, to_ctypes(m, _lib), times)
    else:
        out, nu = g.deskewCloud(cloud, to_ctypes(m, _lib), device_times, device=True)
    d = g.deskewDiag()
    n = len(rec)
    assert d == dict(launches=1 if n else 0, blocks=ndt.host_deskew_plan(n)[0], clouds=1), (what, d)
    got, worst = check_output(g, rec, times, m, out, nu, what)
    return out, got, nu, worst


def launched(ndt, h, cloud, cm, times):
    """deskewCloud under the ctypes motion cm, with its one launch of the planned blocks asserted before anything else"""
    out, nu = h.deskewCloud(cloud, cm, times)
    n = len(cloud)
    d = h.deskewDiag()
    assert d == dict(launches=1 if n else 0, blocks=ndt.host_deskew_plan(n)[0], clouds=1), d
    return out, nu


MOTIONS = {
    "turn": lambda: dc.make_motion([0.02, -0.01, 0.3], [1.0, 0.05, -0.02], EPOCH, EPOCH + 0.1),
    "turn, seen from the end": lambda: dc.make_motion([0.02, -0.01, 0.3], [1.0, 0.05, -0.02], EPOCH, EPOCH + 0.1, EPOCH + 0.1),
    "translation only": lambda: dc.make_motion([0, 0, 0], [1.0, 0.2, 0.0], 0.0, 0.1, 0.05),
    "angle 1e-9": lambda: dc.make_motion([0, 1e-9, 0], [0.5, 0, 0], EPOCH, EPOCH + 0.1),
    "angle pi - 1e-3": lambda: dc.make_motion(np.array([1, 2, -2]) / 3 * (np.pi - 1e-3), [0.3, 0.1, 0], 5.0, 6.0, 5.5),
}


# ---------------------------------------------------------------------------------------------------- sizes
def plan_sizes(plan):
    blocks1, ppb = plan(1)
    assert blocks1 == 1 and ppb == 256
    sizes = [1, 63, 64, 65, 255, 256, 257]
    for k in range(2, 9):
        assert plan(k * ppb) == (k, ppb) and plan(k * ppb + 1) == (k + 1, ppb)
        sizes += [k * ppb, k * ppb + 1]
    cap = 1024
    assert plan(cap * ppb) == (cap, ppb) and plan(cap * ppb + 1)[1] == ppb + 1 and plan(cap * (ppb + 1) + 1)[1] == ppb + 2
    sizes += [5 * ppb + 77, (cap - 1) * ppb, (cap - 1) * ppb + 1, cap * ppb, cap * ppb + 1, cap * (ppb + 1), cap * (ppb + 1) + 1]
    return sizes


SIZE_IDS = list(range(28))


@pytest.mark.parametrize("k", SIZE_IDS)
def test_sizes_at_the_plan_boundaries(mods, g, k):
    ndt = mods[0]
    sizes = plan_sizes(ndt.host_deskew_plan)
    assert len(sizes) == len(SIZE_IDS)
    n = sizes[k]
    name = list(MOTIONS)[k % len(MOTIONS)]
    m = MOTIONS[name]()
    offset = (1e5, -1e5, 1e5) if k % 3 == 1 and "pi" not in name else (0, 0, 0)
    rec = dc.build_records(n, seed=k, offset=offset, odd_every=7 if n > 7 else 0)
    times = dc.build_times(n, m, seed=k, untimed_every=11 if n > 11 else 0, at_ref_every=13 if n > 13 else 0)
    _, _, nu, worst = deskew_checked(mods, g, g.uploadCloud(rec), times, m, (n, name))
    assert n < 12 or nu > 0
    print("n = %d, %s: worst error / bound %.3f, untimed %d" % (n, name, worst, nu))


# ---- every step of the plan up to and including the block cap: n = k * ppb and k * ppb + 1 for k = 1 ... 1024 -------------
# The records, times and the f64 restatement are made ONCE for the largest size; a cloud of n points is their first n rows
# (the definition is per point), so each of the 2048 sizes costs an upload, the launch, a download and vectorised compares.
STEP_CAP, STEP_CHUNKS = 1024, 64
_steps = {}


def step_data():
    if not _steps:
        n_max = STEP_CAP * 256 + 1
        m = MOTIONS["turn"]()
        rec = dc.build_records(n_max, seed=77, odd_every=7)
        times = dc.build_times(n_max, m, seed=78, untimed_every=11, at_ref_every=13)
        kind = dc.kinds(rec, times)
        ref = dc.reference_deskew(rec, times, m)
        allow = 64 * 2.0 ** -53 * (np.abs(rec[:, :3].astype(np.float64)).sum(1) + np.abs(dc.s_of(times, m)) * np.abs(dc.fields(m)[5]).sum())
        _steps.update(m=m, rec=rec, times=times, kind=kind, ref=ref, allow=allow, at_ref=(kind == 0) & (dc.s_of(times, m) == 0),
                      untimed=np.cumsum(kind == 2))
    return _steps


@pytest.mark.parametrize("chunk", range(STEP_CHUNKS))
def test_every_step_of_the_plan(mods, g, chunk):
    """one point either side of every step ndt_host_deskew_plan reports, up to and including the block cap"""
    ndt, _lib, _ = mods
    D = step_data()
    cm = to_ctypes(D["m"], _lib)
    per = STEP_CAP // STEP_CHUNKS
    worst = 0.0
    for k in range(chunk * per + 1, (chunk + 1) * per + 1):
        for n in (k * 256, k * 256 + 1):
            blocks, ppb = ndt.host_deskew_plan(n)
            assert (blocks, ppb) == ((k, 256) if n == k * 256 else (k + 1, 256) if k < STEP_CAP else (1021, 257)), (n, blocks, ppb)
            cloud = g.uploadCloud(D["rec"][:n])
            out, nu = g.deskewCloud(cloud, cm, D["times"][:n])
            assert g.deskewDiag() == dict(launches=1, blocks=blocks, clouds=1), n
            rec, got = raw(g, cloud), raw(g, out)
            kind = D["kind"][:n]
            # bit for bit: fourth words, copied rows, the NaN-ing and its count; s == 0 rows by ==
            assert nu == D["untimed"][n - 1] and got.shape == rec.shape, n
            assert np.array_equal(got[:, 3], rec[:, 3]) and np.array_equal(got[kind == 1], rec[kind == 1]), n
            assert (got[kind == 2][:, :3] == dc.QNAN_BITS).all(), n
            q = xyz_of(got)
            assert (q[D["at_ref"][:n]] == xyz_of(rec)[D["at_ref"][:n]]).all(), n
            # the bound of the module's header against the restatement's rows.  No mask: a copied row gives 0 or NaN, an untimed one
            # NaN, and a NaN is no violation (those rows were compared bit for bit above)
            with np.errstate(invalid="ignore"):
                err = np.abs(q.astype(np.float64) - D["ref"][:n])
                lim = 0.5 * np.spacing(np.abs(q)).astype(np.float64) + D["allow"][:n, None]
                assert not (err > lim).any(), (n, float(np.nanmax(err / lim)))
                worst = max(worst, float(np.nanmax(np.where(kind[:, None] == 0, err / lim, 0.0))))
            boxes, route = out.bounds()
            want = cbc.reference_boxes(q)
            assert cbc.same_boxes(boxes, want) and route == "deskew", (n, cbc.boxes_text(boxes, want))
    print("steps %d ... %d: worst error / bound %.3f" % (chunk * per + 1, (chunk + 1) * per, worst))


@pytest.mark.parametrize("n,variant", ((12, "plain"), (256 + 12, "plain"), (3 * 256 + 40, "far"), (1024 * 256 + 100, "inf"), (1024 * 257 + 30, "plain")))
def test_box_values_owned_by_single_points_of_the_last_block(mods, g, n, variant):
    """every one of the 12 box values has exactly one owner, and all owners sit in the last block: its row alone decides"""
    ndt = mods[0]
    blocks, ppb = ndt.host_deskew_plan(n)
    first_of_last = (blocks - 1) * ppb
    assert n - first_of_last >= 12
    hot = list(np.linspace(first_of_last, n - 1, 12).astype(int))
    rec, owners = cbc.build_cloud(n, hot, floats=4, variant=variant, seed=n)
    # a motion under which the other rows (within 10 of the centre, owners at 20 and 40) stay strictly inside; the owners are
    # measured at t_ref (s == 0: they stay where they are) or carry a NaN (copied as they are)
    m = dc.make_motion([0, 1e-9, 0] if variant == "far" else [0.01, 0, 0.02], [1.0, -0.5, 0.2], EPOCH, EPOCH + 0.1, EPOCH + 0.04)
    times = dc.build_times(n, m, seed=n, outside=False)
    times[hot] = m.t_ref
    out, got, nu, _ = deskew_checked(mods, g, g.uploadCloud(rec), times, m, (n, variant))
    assert nu == 0
    cbc.check_owners(xyz_of(got), owners)                   # (the output's boxes are still owned row by row, by the same rows)
    assert cbc.same_boxes(out.bounds()[0], cbc.reference_boxes(rec))


def test_the_strided_regime_in_a_child(mods):
    """NDT_DESKEW_MAX_BLOCKS=3: three blocks walk clouds of a few thousand points in several passes (tests/deskew_child.py)"""
    env = dict(os.environ, NDT_DESKEW_MAX_BLOCKS="3")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "deskew_child.py")
    r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["cases"] >= 4 and res["max_blocks_seen"] == 3 and res["max_ppb"] > 1024, res


# ---------------------------------------------------------------------------------------------------- inputs
@pytest.mark.parametrize("name", list(MOTIONS))
def test_motions_times_and_offsets(mods, g, name):
    from test_gpu_parity import _DeviceCopies
    m = MOTIONS[name]()
    n = 30011
    for offset in ((0, 0, 0), (1e5, 1e5, -1e5)):
        if "pi" in name and offset[0]:
            continue                                        # (half a turn about the origin from 100 km away overflows nothing, but is no scan)
        rec = dc.build_records(n, seed=3, offset=offset, odd_every=37)
        times = dc.build_times(n, m, seed=4, untimed_every=41, at_ref_every=43)       # a third of them outside the sweep
        assert (times[np.isfinite(times)] < m.t_begin).any() and (times[np.isfinite(times)] > m.t_end).any()
        cloud = g.uploadCloud(rec)
        out, got, nu, worst = deskew_checked(mods, g, cloud, times, m, (name, offset))
        print("%s at %r: worst error / bound %.3f" % (name, offset, worst))
        with _DeviceCopies() as dev:                        # the same times in device memory: the same bits
            d_times = dev.put(times.view(F))
            out2, got2, nu2, _ = deskew_checked(mods, g, cloud, times, m, (name, "device times"), device_times=d_times)
        assert np.array_equal(got, got2) and nu == nu2 and np.array_equal(out.bounds()[0], out2.bounds()[0])


def test_empty_cloud_and_refusals_with_a_cloud_in_hand(mods, g):
    import ctypes as C
    ndt, _lib, L = mods
    m = MOTIONS["turn"]()
    cm = to_ctypes(m, _lib)
    empty = g.uploadCloud(np.zeros((0, 3), F))
    out, nu = g.deskewCloud(empty, cm, np.zeros(0))
    assert len(out) == 0 and nu == 0 and out._c and g.deskewDiag() == dict(launches=0, blocks=0, clouds=1)
    boxes, route = out.bounds()
    assert cbc.same_boxes(boxes, cbc.EMPTY_BOXES) and route == "none"
    cloud = g.uploadCloud(dc.build_records(100, seed=1))
    good, _ = launched(ndt, g, cloud, cm, np.full(100, m.t_begin))
    before = g.deskewDiag()
    SENT = 0x5A5A5A5A
    t = np.zeros(100)
    from test_deskew_host import invalid_motions
    for motion_p, times_p in [(None, t.ctypes.data), (C.byref(cm), None)] + [(C.byref(b), t.ctypes.data) for b in invalid_motions(_lib)]:
        o, n_u = C.c_void_p(SENT), C.c_size_t(SENT)
        assert L.ndt_cloud_deskew(g._h, cloud._c, motion_p, times_p, 0, C.byref(o), C.byref(n_u)) == _lib.NDT_ERR_INVALID
        assert o.value is None and n_u.value == SENT
        outs, nus = (C.c_void_p * 2)(SENT, SENT), (C.c_size_t * 2)(SENT, SENT)
        ins = (C.c_void_p * 2)(empty._c, cloud._c)
        ms = (_lib.DeskewMotion * 2)(cm, cm)
        if motion_p is not None and times_p is not None:
            ms[1] = motion_p._obj
        st = L.ndt_cloud_deskew_clouds(g._h, ins, 2, ms if motion_p is not None else None, times_p, 0, outs, nus)
        assert st == _lib.NDT_ERR_INVALID and outs[0] is None and outs[1] is None and list(nus) == [SENT, SENT]
    outs, nus = (C.c_void_p * 2)(SENT, SENT), (C.c_size_t * 2)(SENT, SENT)
    assert L.ndt_cloud_deskew_clouds(g._h, (C.c_void_p * 2)(cloud._c, None), 2, (_lib.DeskewMotion * 2)(cm, cm), t.ctypes.data, 0, outs, nus) == _lib.NDT_ERR_INVALID
    assert outs[0] is None and outs[1] is None
    assert g.deskewDiag() == before and len(good) == 100


def test_every_kind_of_input_cloud(mods, g, tmp_path):
    ndt = mods[0]
    m = MOTIONS["turn"]()
    rec = dc.build_records(30011, seed=9, odd_every=11)

    def check(cloud, route, what):
        assert cloud.bounds()[1] == route, (what, cloud.bounds()[1])
        times = dc.build_times(len(cloud), m, seed=len(cloud), untimed_every=29)
        return deskew_checked(mods, g, cloud, times, m, what)
    check(g.uploadCloud(rec[:5000, :3]), cbc.upload_route(5000, 12), "uploaded (host route)")
    check(g.uploadCloud(rec), cbc.upload_route(30011, 16), "uploaded (device route, 16-byte records)")
    filt, _ = g.voxelGridFilterCloud(rec[:, :3], 0.7, is_dense=False)
    check(filt, "filter_rows", "filter output")
    outs, _ = g.voxelGridFilterClouds([rec[:9000, :3], rec[9000:9001, :3], rec[9001:, :3]], 0.7, is_dense=False)
    check(outs[0], "multi_words", "slice of a batched filter")
    check(g.selectCloud(g.uploadCloud(rec), finite=True, range=(0, 50)), "select", "a selection")
    # a deskew of a deskew
    first, got1, _, _ = check(g.uploadCloud(rec), cbc.upload_route(30011, 16), "uploaded")
    again, got2, _, _ = check(first, "deskew", "a previous deskew")
    assert np.array_equal(raw(g, first), got1)
    # a staged scan: compensated, then overwritten by the next scan -- the output is a cloud of its own
    finite = rec[np.isfinite(rec[:, :3]).all(1), :3]
    for k, part in enumerate((finite[:12000], finite[12000:20000] + F(3)), 1):
        ndt.pcd_write_xyz(str(tmp_path / ("cloud_%d.pcd" % k)), part)
    seq = ndt.PcdSequence(str(tmp_path))
    seq.stage(0)
    assert seq.poll(0) == 2
    view = seq.next_cloud(g)[0]
    out, got, _, _ = check(view, "staged", "staged scan")
    view2 = seq.next_cloud(g)[0]
    check(view2, "staged", "the next staged scan")
    assert np.array_equal(raw(g, out), got)
    boxes, route = out.bounds()
    assert cbc.same_boxes(boxes, cbc.reference_boxes(xyz_of(got))) and route == "deskew"


# ---------------------------------------------------------------------------------------------------- many clouds
def ragged(k):
    rec = dc.build_records(9000, seed=12, odd_every=13)
    parts = [rec[:4097], rec[:0], rec[4097:4098], rec[4098:8000], rec[:0], rec[8000:]]
    return {1: [parts[0]], 2: [parts[1], parts[3]], 5: parts[:5], 6: parts}[k]


@pytest.mark.parametrize("k", (1, 2, 5, 6))
def test_many_clouds_match_the_single_call(mods, g, k):
    ndt, _lib, _ = mods
    parts = ragged(k)
    names = list(MOTIONS)
    for order in (list(range(len(parts))), list(range(len(parts)))[::-1]):
        ins = [g.uploadCloud(parts[j]) for j in order]
        ms = [MOTIONS[names[j % len(names)]]() for j in order]
        ts = [dc.build_times(len(parts[j]), mj, seed=j, untimed_every=17 if len(parts[j]) > 17 else 0) for j, mj in zip(order, ms)]
        outs, nus = g.deskewClouds(ins, [to_ctypes(mj, _lib) for mj in ms], ts)
        d = g.deskewDiag()
        total = sum(len(parts[j]) for j in order)
        assert d == dict(launches=1 if total else 0, blocks=sum(ndt.host_deskew_plan(len(parts[j]))[0] for j in order), clouds=len(parts)), d
        singles = []
        for j, cloud, mj, tj, out, nu in zip(order, ins, ms, ts, outs, nus):
            check_output(g, raw(g, cloud), tj, mj, out, nu, (k, j))
            one, nu1 = launched(ndt, g, cloud, to_ctypes(mj, _lib), tj)
            assert np.array_equal(raw(g, one), raw(g, out)) and nu1 == nu
            assert np.array_equal(one.bounds()[0], out.bounds()[0]) and one.bounds()[1] == out.bounds()[1]
            singles.append(raw(g, one))
        # the slices go one by one, in either order, while the others stay readable
        release = list(range(len(outs))) if order[0] == 0 else list(range(len(outs)))[::-1]
        for step, pos in enumerate(release):
            outs[pos].release()
            for other in release[step + 1:]:
                assert np.array_equal(raw(g, outs[other]), singles[other])
    assert g.deskewClouds([], [], []) == ([], [])


# ---------------------------------------------------------------------------------------------------- consumers
SWEEP_W, SWEEP_TAU = np.array([0.002, -0.001, 0.03]), np.array([1.0, 0.05, -0.01])     # 10 m/s and 17 deg/s over 0.1 s


def skewed_source(ndt, s):
    """the golden source as a moving sensor would have measured it: every point at its own time (by azimuth) -> (records f32,
    times, the library's motion of the sweep)"""
    times = dc.azimuth_times(s, EPOCH, EPOCH + 0.1)
    skewed = dc.skew_scan(s, times, SWEEP_W, SWEEP_TAU, EPOCH, EPOCH + 0.1).astype(F)
    T = np.eye(4)
    T[:3, :3] = dc.exp_rot(SWEEP_W / np.linalg.norm(SWEEP_W), np.linalg.norm(SWEEP_W))
    T[:3, 3] = SWEEP_TAU
    return skewed, times, ndt.host_deskew_motion(T, EPOCH, EPOCH + 0.1)


def test_a_deskewed_cloud_is_the_cloud_an_upload_of_its_records_would_be(mods, pair):
    ndt = mods[0]
    t, s = pair
    skewed, times, cm = skewed_source(ndt, s)
    h0 = ndt.NormalDistributionsTransform()
    records = raw(h0, launched(ndt, h0, h0.uploadCloud(skewed), cm, times)[0])
    assert (records[:, 3] == np.array([1.0], F).view(np.uint32)[0]).all()

    def both(make):
        """the same steps on two fresh handles: with the deskew's output, with the upload of its downloaded records"""
        res = []
        for form in ("deskew", "upload"):
            h = ndt.NormalDistributionsTransform()
            cloud = launched(ndt, h, h.uploadCloud(skewed), cm, times)[0] if form == "deskew" else h.uploadCloud(xyz_of(records).copy())
            res.append(make(h, cloud))
        return res
    a, b = both(lambda h, cloud: (raw(h, cloud), cloud.bounds()[0]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    def as_source(h, cloud):
        h.setInputTarget(t)
        h.setInputSourceCloud(cloud)
        h.align()
        return h.getFinalTransformation().tobytes(), h.getFinalNumIteration(), h.hasConverged()
    a, b = both(as_source)
    assert a == b

    def as_target(h, cloud):
        h.setInputTargetCloud(cloud)
        return h.grid()
    a, b = both(as_target)
    assert set(a) == set(b) and len(a["idx"]) > 0
    for key in a:
        assert np.array_equal(a[key], b[key]), key

    def through_filter(h, cloud):
        h.voxelGridFilterBegin(cloud, 0.5)
        out, ov = h.voxelGridFilterEnd()
        return raw(h, out), ov
    a, b = both(through_filter)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and len(a[0]) > 0

    def through_map(h, cloud):
        h.mapUpdateCloud(cloud, leaf_size=0.5)
        return h.mapGet()
    a, b = both(through_map)
    assert a.tobytes() == b.tobytes() and len(a) > 0

    def through_accumulate(h, cloud):
        h.targetAccumulateCloud(cloud)
        return bytes(h.targetAccumulateExport())
    a, b = both(through_accumulate)
    assert a == b and len(a) > 0


def test_end_to_end_on_the_golden_pair(mods, pair):
    """the golden source, skewed by a known motion, deskewed and registered: the registration of the unskewed source again,
    within the project's parity line (1e-4 rotation, 1e-3 m) and in as many iterations"""
    from conftest import rot_err, trans_err
    ndt = mods[0]
    t, s = pair
    skewed, times, cm = skewed_source(ndt, s)
    assert np.abs(skewed - s).max() > 0.5

    def register(make):
        h = ndt.NormalDistributionsTransform()
        h.setResolution(1.0)
        h.setInputTarget(t)
        h.setInputSourceCloud(make(h))
        h.align()
        return h.getFinalTransformation(), h.getFinalNumIteration(), h.hasConverged()
    T_plain, it_plain, ok_plain = register(lambda h: h.uploadCloud(s))
    T_fixed, it_fixed, ok_fixed = register(lambda h: launched(ndt, h, h.uploadCloud(skewed), cm, times)[0])
    T_skewed, it_skewed, _ = register(lambda h: h.uploadCloud(skewed))
    assert ok_plain and ok_fixed
    print("deskewed vs unskewed: rot %.3g trans %.3g m, iterations %d / %d" % (rot_err(T_fixed, T_plain), trans_err(T_fixed, T_plain), it_fixed, it_plain))
    print("skewed, not compensated, vs unskewed: rot %.3g trans %.3g m, iterations %d" % (rot_err(T_skewed, T_plain), trans_err(T_skewed, T_plain), it_skewed))
    assert rot_err(T_fixed, T_plain) <= 1e-4 and trans_err(T_fixed, T_plain) <= 1e-3 and it_fixed == it_plain


# ---------------------------------------------------------------------------------------------------- untouched state
def test_the_calls_change_nothing_of_the_handle(mods, pair):
    ndt, _lib, _ = mods
    t, s = pair
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(t)
    g.setInputSource(s)
    g.align()
    g.mapUpdate(s[:3000], leaf_size=0.5)
    g.getNVTL()
    g.scorePoses([np.eye(4)])
    g.selectCloud(g.uploadCloud(s[:700]), finite=True)
    g.removeOutliers(g.uploadCloud(s[:700]), radius=0.5, min_neighbors=2)
    pending = g.uploadCloud(s[:5000])
    ref_filtered = raw(g, g.voxelGridFilterCloud(s[:5000], 0.5)[0])
    g.voxelGridFilterBegin(pending, 0.5)

    def state():
        return (g.getFinalTransformation().tobytes(), g.hasConverged(), g.getFinalNumIteration(), g.getTransformationProbability(),
                repr(g.stats()), g.grid_counts(), g.inputBounds("source")[0].tobytes(), g.inputBounds("source")[1], g.inputBounds("target")[0].tobytes(),
                g.mapSize(), g.scorePosesLaunches(), g.nvtlLaunches(), repr(g.selectDiag()), repr(g.outlierDiag()))
    before = state()
    skewed, times, cm = skewed_source(ndt, s)
    cloud = g.uploadCloud(skewed)
    launched(ndt, g, cloud, cm, times)
    g.deskewClouds([cloud, g.uploadCloud(skewed[:100])], [cm, cm], [times, times[:100]])
    assert g.deskewDiag() == dict(launches=1, blocks=ndt.host_deskew_plan(len(skewed))[0] + 1, clouds=2)
    assert state() == before
    out, ov = g.voxelGridFilterEnd()
    assert np.array_equal(raw(g, out), ref_filtered) and not ov
    T0 = g.getFinalTransformation().tobytes()
    g.align()
    assert g.getFinalTransformation().tobytes() == T0


# ---------------------------------------------------------------------------------------------------- the app
def test_map_sequence_deskew(mods, reference_pcd, tmp_path):
    """apps/map_sequence --scan-to-map --deskew t over three files with a time field against the same loop in Python"""
    ndt, _lib, _ = mods
    d = tmp_path / "pcd"
    d.mkdir()
    base = [np.ascontiguousarray(ndt.pcd_read_xyz(p)[0][:, :3], dtype=F) for p in reference_pcd]
    scans, stamps = [], []
    for k, xyz in enumerate((base[0], base[1], base[1]), 1):
        times = dc.azimuth_times(xyz, EPOCH + 0.1 * k, EPOCH + 0.1 * k + 0.1)
        if k == 3:                                          # the third scan is skewed (and two of its points carry no time)
            xyz = dc.skew_scan(xyz, times, [0, 0, 0.01], [0.3, 0.02, 0], EPOCH + 0.3, EPOCH + 0.4).astype(F)
            times[[5, 999]] = np.nan, np.inf
        write_pcd(str(d / ("sweep_%d.pcd" % k)), [("x", "<f4", "F", 1, xyz[:, 0]), ("y", "<f4", "F", 1, xyz[:, 1]), ("z", "<f4", "F", 1, xyz[:, 2]),
                                                  ("t", "<f8", "F", 1, times)], "binary")
        scans.append(xyz)
        stamps.append(times)
    exe = build_app(tmp_path, "map_sequence")
    out = subprocess.check_output([exe, "--scan-to-map", "--deskew", "t", str(d)], text=True)
    plain = subprocess.check_output([exe, "--scan-to-map", str(d)], text=True)
    assert "deskewed:" not in plain
    for args in (["--deskew", "t", str(d)], ["--scan-to-map", "--deskew"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "usage: map_sequence" in r.stderr, args
    r = subprocess.run([exe, "--scan-to-map", "--deskew", "absent", str(d)], capture_output=True, text=True)
    assert r.returncode != 0 and "no field absent" in r.stderr

    def transforms(text):
        lines = text.splitlines()
        return [np.array([[float(x) for x in lines[i + 1 + r].split()] for r in range(4)]) for i, ln in enumerate(lines) if ln.startswith("Transform ")]
    g = ndt.NormalDistributionsTransform()
    app_settings(g)
    poses, want, counts = [np.eye(4, dtype=F)], [], []
    for k, (x, ts) in enumerate(zip(scans, stamps)):
        cloud, dense = g.uploadCloud(x), True
        fin = ts[np.isfinite(ts)]
        if len(poses) >= 2 and fin.max() > fin.min():
            inc = (np.linalg.inv(poses[-2].astype(np.float64)) @ poses[-1].astype(np.float64)).astype(F)
            cloud, nu = launched(ndt, g, cloud, ndt.host_deskew_motion(inc, fin.min(), fin.max()), ts)
            counts.append((len(x) - nu, len(x)))
            dense = nu == 0
        g.voxelGridFilterBegin(cloud, 0.5, is_dense=dense)
        filtered, _ = g.voxelGridFilterEnd()
        if k == 0:
            g.targetAccumulateCloud(filtered)
            continue
        g.setInputSourceCloud(filtered)
        g.align(poses[-1])
        assert g.hasConverged()
        poses.append(g.getFinalTransformation().astype(F))
        want.append(poses[-1])
        g.targetAccumulateCloud(filtered, poses[-1])
    got = transforms(out)
    got_counts = [tuple(int(v) for v in m_) for m_ in re.findall(r"^deskewed: (\d+)/(\d+)$", out, re.M)]
    print("deskew: app", got, got_counts, "python", want, counts)
    assert got_counts == counts == [(len(scans[2]) - 2, len(scans[2]))]
    assert len(got) == len(want) == 2 and all(np.abs(a - b).max() <= 1e-5 for a, b in zip(got, want))
    # the second scan goes through as it is, the third does not
    assert np.abs(transforms(plain)[0] - got[0]).max() <= 1e-6 and np.abs(transforms(plain)[1] - got[1]).max() > 1e-4
