"""GPU: the two bounding boxes every cloud carries (DeviceCloud::bb_min / bb_max), read out as stored (ndt_cloud_bounds,
ndt_diag_input_bounds), of every producer at the sizes where its blocks, rounds and caps change -- against the numpy
reference of tests/cloud_box_cases.py (== on the f32 values), in clouds whose box values each have one owner on a row the
case is about.  Every case first asserts the producer (the route) it is named for.  Filter outputs are held against the
box of the oracle's voxel_grid_filter output.

The sizes are the cuts of the code as it stands (cloud_box_cases.py; NOTES.md "Who writes a cloud's boxes")."""
import numpy as np
import pytest

import cloud_box_cases as cb
from cloud_box_cases import EMPTY_BOXES, F32, boxes_text, build_cloud, reference_boxes, same_boxes, spread_hot
from test_gpu_parity import _DeviceCopies, mods  # noqa: F401

pytestmark = pytest.mark.gpu

K = cb.BLOCK
R1 = cb.REPACK_MAX_BLOCKS * K                 # 262 144: one row per thread of k_repack_bbox's 1 024 blocks
S16 = cb.REC16_MAX_BLOCKS * K                 # 65 536: one load per thread of k_bbox16's 256 blocks
T16 = cb.REC16_LOADS * S16                    # 524 288: one trip of its outer loop
SO = cb.OUT_BOX_BLOCKS * K                    # 16 384: one load per thread of the 64 blocks over a filter's output
TO = cb.REC16_LOADS * SO                      # 131 072: one trip there


def check(got, rec, route, what=None):
    boxes, r = got
    assert r == route, (what, r, route)  # the producer first
    ref = reference_boxes(rec) if len(rec) else EMPTY_BOXES
    assert same_boxes(boxes, ref), (what, r, boxes_text(boxes, ref))


def hot_rows(n, cut):
    """rows either side of every multiple of `cut` that a cloud of n reaches, the block edges, the ends"""
    last_cut = (n - 1) // cut * cut
    return spread_hot(n, must=[n - 1, last_cut, last_cut - 1, K - 1, K, n - 2, 0])


def variant(j):
    return cb.VARIANTS[j % len(cb.VARIANTS)]


# ---- host | device route -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floats", [3, 4, 8])
def test_host_and_device_route_either_side_of_the_stage_limit(mods, floats):
    ndt, _, _ = mods
    g = ndt.NormalDistributionsTransform()
    for j, n in enumerate((cb.HOST_STAGE_MAX, cb.HOST_STAGE_MAX + 1)):
        for v in (variant(j + floats), variant(j + floats + 2)):
            rec, _ = build_cloud(n, hot_rows(n, K), floats=floats, variant=v, seed=floats)
            on_host = "none" if n == 0 else cb.host_route()
            route = on_host if n <= cb.HOST_STAGE_MAX else "rec16_copy" if floats == 4 else "repack"
            assert route == cb.upload_route(n, 4 * floats)
            check(g.uploadCloud(rec).bounds(), rec, route, (n, floats, v))


# ---- k_repack_bbox: any stride, or 16-byte records off their boundary -------------------------------------------------
@pytest.mark.parametrize("n", [1, K - 1, K, K + 1, R1, R1 + 1])
def test_repack_kernel_at_its_block_and_cap_boundaries(mods, n):
    """1 024 blocks at most: row 262 144 is the second row of block 0's first thread, row 262 143 the last of block 1 023"""
    ndt, _, _ = mods
    g = ndt.NormalDistributionsTransform()
    with _DeviceCopies() as dev:
        for j, (floats, shift) in enumerate(((3, 0), (8, 0), (4, 1))):
            rec, _ = build_cloud(n, hot_rows(n, R1), floats=floats, variant=variant(j + n), seed=n)
            buf = np.concatenate([np.zeros(shift, F32), rec.ravel()])
            g.setInputSourceDevice(dev.put(buf) + 4 * shift, n, 4 * floats)
            assert cb.upload_route(n, 4 * floats, on_device=True, aligned=not shift) == "repack"
            check(g.inputBounds("source"), rec, "repack", (n, floats, shift))


# ---- k_bbox16, the copying form ------------------------------------------------------------------------------------------
REC16_SIZES = [1, K - 1, K, K + 1, S16, S16 + 1, 3 * S16 + 5, T16, T16 + 1]


@pytest.mark.parametrize("n", REC16_SIZES)
def test_rec16_copy_from_device_records(mods, n):
    """256 blocks at most, eight loads per thread: row 65 536 is a thread's second load, rows from 7 * 65 536 its eighth,
    row 524 288 the second trip of the outer loop"""
    ndt, _, _ = mods
    g = ndt.NormalDistributionsTransform()
    with _DeviceCopies() as dev:
        for j in range(2):
            must = [[n - 1, (n - 1) // S16 * S16, 7 * S16, T16 - 1], [n - 2, (n - 1) // S16 * S16 - 1, 7 * S16 + K, S16]][j]
            rec, _ = build_cloud(n, spread_hot(n, must=must), floats=4, variant=variant(j + n), seed=n + j)
            g.setInputSourceDevice(dev.put(rec), n, 16)
            check(g.inputBounds("source"), rec, cb.upload_route(n, 16, on_device=True), (n, j))


@pytest.mark.parametrize("n", [n for n in (S16, S16 + 1, T16 + 1) if n > cb.HOST_STAGE_MAX])
def test_rec16_copy_from_a_host_buffer(mods, n):
    """the same kernel behind the staging copy: plain rows behind a stream wait"""
    ndt, _, _ = mods
    g = ndt.NormalDistributionsTransform()
    rec, _ = build_cloud(n, spread_hot(n, must=[n - 1, (n - 1) // S16 * S16, S16 - 1, 7 * S16]), floats=4, variant=variant(n), seed=n)
    check(g.uploadCloud(rec).bounds(), rec, "rec16_copy", n)


# ---- k_bbox16 over clouds used where they lie: tagged rows, polled -------------------------------------------------------
@pytest.mark.parametrize("n", REC16_SIZES)
def test_clouds_by_reference_at_the_same_boundaries(mods, n):
    ndt, _, _ = mods
    g = ndt.NormalDistributionsTransform()
    with _DeviceCopies() as dev:
        for j in range(2):
            must = [[n - 1, (n - 1) // S16 * S16, 7 * S16, T16 - 1], [n - 2, (n - 1) // S16 * S16 - 1, 7 * S16 + K, S16]][j]
            rec, _ = build_cloud(n, spread_hot(n, must=must), floats=4, variant=variant(j + n + 1), seed=n + j)
            g.setInputSourceDeviceRef(dev.put(rec), n)
            check(g.inputBounds("source"), rec, "rec16_polled", (n, j))


@pytest.mark.parametrize("n", [1, K + 1, S16 + 1])
def test_target_by_reference(mods, n):
    ndt, _, _ = mods
    g = ndt.NormalDistributionsTransform()
    with _DeviceCopies() as dev:
        rec, _ = build_cloud(n, hot_rows(n, S16), floats=4, variant=variant(n), seed=n)
        g.setInputTargetDeviceRef(dev.put(rec), n, is_dense=False)  # (box [1]: box [0] of these clouds reaches FLT_MAX / inf)
        check(g.inputBounds("target"), rec, "rec16_polled", n)


def test_no_stale_row_and_no_stale_tag_leak(mods):
    """The polled rows are one page-locked block per handle.  A second, smaller input strictly inside the first's box must
    get its own boxes (rows of blocks the second launch does not have stay the first's), and so must an input after 300
    uploads have moved the tag."""
    ndt, _, _ = mods
    g = ndt.NormalDistributionsTransform()
    with _DeviceCopies() as dev:
        big, _ = build_cloud(S16 + 1, hot_rows(S16 + 1, S16), floats=4, seed=1)
        small, _ = build_cloud(300, hot_rows(300, K), floats=4, seed=2)
        small[:, :3] *= F32(0.25)
        tiny = np.array([[1, 2, 3, 0]], F32)
        d_big, d_small, d_tiny = dev.put(big), dev.put(small), dev.put(tiny)
        rb, rs = reference_boxes(big), reference_boxes(small)
        assert (rb[:, 0] < rs[:, 0]).all() and (rs[:, 1] < rb[:, 1]).all()
        for setter, which in ((g.setInputSourceDeviceRef, "source"), (lambda p, n: g.setInputTargetDeviceRef(p, n, is_dense=False), "target")):
            setter(d_big, len(big))
            check(g.inputBounds(which), big, "rec16_polled")
            setter(d_small, len(small))
            check(g.inputBounds(which), small, "rec16_polled")
        for _ in range(300):
            g.setInputSourceDeviceRef(d_tiny, 1)
        check(g.inputBounds("source"), tiny, "rec16_polled")
        g.setInputSourceDeviceRef(d_big, len(big))
        check(g.inputBounds("source"), big, "rec16_polled")
        g.setInputSourceDevice(d_small, len(small), 16)  # (the copying form polls the same block)
        check(g.inputBounds("source"), small, "rec16_copy")
        check(g.inputBounds("target"), small, "rec16_polled")  # ... and the target's stay what they were


# ---- filter outputs --------------------------------------------------------------------------------------------------------
LEAF = 0.5


def one_point_per_voxel(count, nx, ny, nz, seed, hot=(), origin=(0, 0, 0)):
    """`count` points, each alone in its voxel of LEAF, at most one voxel per (y, z) row of the lattice: the filter's output is
    these points in (z, y) order.  Output 0 owns min y and min z, the last output max y and max z, output hot[0] max x and
    output hot[1] min x; every other point keeps away from its voxel's faces.  -> (points in shuffled order, the output)"""
    rng = np.random.default_rng(seed)
    rows = np.sort(np.concatenate([[0, ny * nz - 1], 1 + rng.choice(ny * nz - 2, count - 2, replace=False)])) if count > 1 else np.array([0])
    ijk = np.stack([rng.integers(0, nx, count), rows % ny, rows // ny], axis=1).astype(np.float64)
    frac = rng.uniform(0.25, 0.75, (count, 3))
    frac[0, 1:], frac[-1, 1:] = 0.05, 0.95
    ijk[0, 0], ijk[-1, 0] = 1, 1  # (the corners' x stays inside)
    if len(hot) > 0:
        ijk[hot[0], 0], frac[hot[0], 0] = nx - 1, 0.95
    if len(hot) > 1:
        ijk[hot[1], 0], frac[hot[1], 0] = 0, 0.05
    out = ((ijk + frac + np.asarray(origin, np.float64)) * LEAF).astype(F32)
    return out[rng.permutation(count)], out


def filtered(po, pts, leaf=LEAF, is_dense=True):
    ref, ov = po.voxel_grid_filter(pts, leaf, is_dense=is_dense)
    assert not ov
    return ref


def check_output(dc, ref, route="filter_rows", what=None):
    boxes, r = dc.bounds()
    assert r == route, (what, r)
    assert len(dc) == len(ref), (what, len(dc), len(ref))
    want = reference_boxes(ref) if len(ref) else EMPTY_BOXES
    assert same_boxes(boxes, want), (what, boxes_text(boxes, want))
    assert np.array_equal(dc.numpy(), ref), what


def test_outputs_far_smaller_than_the_input(mods):
    """60 000 points into 27 voxels: 63 of the 64 blocks find nothing below the device's count and must write neutral rows"""
    ndt, po, _ = mods
    g = ndt.NormalDistributionsTransform()
    rng = np.random.default_rng(9)
    pts = rng.uniform(100, 130, (60000, 3)).astype(F32)
    ref = filtered(po, pts, 10.0)
    assert len(ref) == 27
    with _DeviceCopies() as dev:
        check_output(g.voxelGridFilterCloud(pts, 10.0)[0], ref)
        check_output(g.voxelGridFilterCloudDevice(dev.put(np.c_[pts, np.zeros(len(pts), F32)]), len(pts), 16, 10.0)[0], ref)
        g.voxelGridFilterBegin(g.uploadCloud(pts), 10.0)
        check_output(g.voxelGridFilterEnd()[0], ref)
        outs, _ = g.voxelGridFilterClouds([pts[:30000], pts[30000:]], 10.0)
        for dc, part in zip(outs, (pts[:30000], pts[30000:])):
            check_output(dc, filtered(po, part, 10.0), "multi_words")


@pytest.mark.parametrize("count,nx,side,index", [(SO, 8, 256, 0), (SO + 1, 8, 256, 0), (SO + 1, 8, 256, 2), (TO, 8, 512, 0), (TO + 1, 8, 512, 0),
                                                 (TO, 2, 512, 0), (TO + 1, 2, 512, 0)])
def test_output_counts_either_side_of_a_load_and_a_trip(mods, count, nx, side, index):
    """One point per voxel, so the output count is the input's: 16 384 | 16 385 is the second load of a thread of the 64
    blocks, 131 072 | 131 073 the second trip.  nx = 8: more than four cells per point, the dense chain (index 2: the sparse
    index); nx = 2 from 131 072 points: at most four cells per point, the bucket front end."""
    ndt, po, _ = mods
    g = ndt.NormalDistributionsTransform()
    g.setVoxelIndex(index)
    assert (nx * side * side <= 4 * count and count >= cb.FILTER_BUCKETS_FROM) == (nx == 2)
    assert nx * side * side <= 16 * count + (1 << 22)  # (not the sparse index by itself)
    pts, out = one_point_per_voxel(count, nx, side, side, seed=count + nx, hot=[(count - 1) // SO * SO, (count - 1) // SO * SO - 1])
    ref = filtered(po, pts)
    assert np.array_equal(ref, out)  # alone in its voxel, a point is its centroid
    check_output(g.voxelGridFilterCloud(pts, LEAF)[0], ref, what=(count, nx, index))
    if count in (SO + 1, TO + 1) and index == 0:
        g.voxelGridFilterBegin(g.uploadCloud(pts), LEAF)
        check_output(g.voxelGridFilterEnd()[0], ref, what="begin / end")


def test_empty_and_overflow_routes(mods):
    ndt, po, _ = mods
    g = ndt.NormalDistributionsTransform()
    none = np.full((700, 3), np.nan, F32)
    none[::3, 1] = 4.0
    none[1::3, 0] = np.inf
    dc, ov = g.voxelGridFilterCloud(none, LEAF, is_dense=False)
    assert not ov
    check_output(dc, np.zeros((0, 3), F32))
    rec, _ = build_cloud(5000, hot_rows(5000, K), variant="far", seed=4)
    ref, ov_ref = po.voxel_grid_filter(rec, 1e-4, is_dense=True)
    dc, ov = g.voxelGridFilterCloud(rec, 1e-4, is_dense=True)
    assert ov and ov_ref and len(dc) == len(rec)
    boxes, route = dc.bounds()
    assert route == "filter_rows"
    assert same_boxes(boxes, reference_boxes(rec)), boxes_text(boxes, reference_boxes(rec))  # the copied-through input's
    assert np.array_equal(dc.numpy(), rec[:, :3], equal_nan=True)


def test_a_small_result_after_a_large_one_has_its_own_boxes(mods):
    """the rows of a slot are reused: N1, begin / end and the map each keep one page-locked block per handle"""
    ndt, po, _ = mods
    g = ndt.NormalDistributionsTransform()
    big, _ = one_point_per_voxel(SO + 1, 8, 256, 256, seed=1, hot=[SO, 5])
    small, _ = one_point_per_voxel(300, 4, 20, 20, seed=2, hot=[299, 7], origin=(2, 100, 100))
    rb, rs = filtered(po, big), filtered(po, small)
    assert (reference_boxes(rb)[:, 0] < reference_boxes(rs)[:, 0]).all() and (reference_boxes(rs)[:, 1] < reference_boxes(rb)[:, 1]).all()
    # ... and many points in few voxels inside it: all 64 blocks run, one finds rows below the device's count
    few = (np.random.default_rng(3).uniform(0, 1.5, (40000, 3)) + [1.0, 50.0, 50.0]).astype(F32)
    rf = filtered(po, few)
    assert len(rf) == 27 and (reference_boxes(rb)[:, 0] < reference_boxes(rf)[:, 0]).all() and (reference_boxes(rf)[:, 1] < reference_boxes(rb)[:, 1]).all()
    runs = ((big, rb), (small, rs), (big, rb), (few, rf))
    for pts, ref in runs:
        check_output(g.voxelGridFilterCloud(pts, LEAF)[0], ref)
    for pts, ref in runs:
        g.voxelGridFilterBegin(g.uploadCloud(pts), LEAF)
        check_output(g.voxelGridFilterEnd()[0], ref)
    for pts, ref in runs:
        g.mapClear()
        g.mapUpdate(pts, None, LEAF)
        check(g.inputBounds("map"), ref, "filter_rows")
        assert np.array_equal(g.mapGet(), ref)


# ---- batched outputs ----------------------------------------------------------------------------------------------------
def test_ragged_batch_members_each_have_their_own_boxes(mods):
    """0, 1, 255, 257 and 16 385 points in one call: the largest member fixes the grid of the box kernel (64 blocks per member),
    an all-NaN member under either NaN rule, every member against the oracle's filter of it alone"""
    ndt, po, _ = mods
    g = ndt.NormalDistributionsTransform()
    rng = np.random.default_rng(21)
    lone, _ = one_point_per_voxel(SO + 1, 8, 256, 256, seed=3, hot=[SO, SO - 1])
    members = [np.zeros((0, 3), F32), np.array([[3.2, -1.1, 0.7]], F32), rng.uniform(-5, 5, (255, 3)).astype(F32),
               np.full((40, 3), np.nan, F32), rng.uniform(-9, 9, (257, 3)).astype(F32), np.full((40, 3), np.nan, F32), lone]
    dense = [True, True, True, True, False, False, True]
    members[4][5] = np.nan
    members[4][9, 2] = np.inf
    # (no point, or none that counts: an empty cloud -- the oracle is not asked what PCL makes of a dense cloud of NaNs)
    refs = [po.voxel_grid_filter(m, LEAF, is_dense=d)[0] if len(m) and not np.isnan(m).all() else np.zeros((0, 3), F32)
            for m, d in zip(members, dense)]
    assert [len(r) for r in refs][0::3] == [0, 0, SO + 1] and len(refs[5]) == 0
    with _DeviceCopies() as dev:
        cat = np.concatenate([np.c_[m, np.ones(len(m), F32)] for m in members])
        off = np.concatenate([[0], np.cumsum([len(m) for m in members])])
        forms = [("buffer", lambda: g.voxelGridFilterClouds(members, LEAF, is_dense=dense)),
                 ("clouds", lambda: g.voxelGridFilterClouds([g.uploadCloud(m) for m in members], LEAF, is_dense=dense)),
                 ("device", lambda: g.voxelGridFilterBatchDevice(dev.put(cat), off, 16, LEAF, is_dense=dense))]
        for name, call in forms:
            outs, ovs = call()
            assert not ovs.any()
            assert g.filterBatchDiag()["single_route"] == 0, name
            for k, (dc, ref) in enumerate(zip(outs, refs)):
                check_output(dc, ref, "multi_words" if len(ref) else "none", (name, k))


# ---- staged sequence ---------------------------------------------------------------------------------------------------
def test_staged_scans_carry_the_boxes_of_the_files_records(mods, tmp_path):
    ndt, _, clouds = mods
    g = ndt.NormalDistributionsTransform()
    recs = []
    for k, (n, v) in enumerate(((1, "plain"), (257, "inf"), (5000, "fltmax"), (70001, "denormal"))):
        rec, _ = build_cloud(n, hot_rows(n, K), variant=v, seed=k)
        recs.append(rec)
        clouds.write_pcd_xyz(str(tmp_path / ("cloud_%d.pcd" % (k + 1))), rec)
    seq = ndt.PcdSequence(str(tmp_path))
    seq.stage(0)
    assert seq.poll(0) == len(recs)
    for k, rec in enumerate(recs):
        dc, host, dense, num = seq.next_cloud(g)
        assert num == k + 1 and len(dc) == len(rec) and np.array_equal(host[:, :3].view(np.uint32), rec.view(np.uint32))
        check(dc.bounds(), rec, "staged", k)
        dc.release()
    assert seq.next_cloud(g) is None


# ---- the map ---------------------------------------------------------------------------------------------------------
def test_the_maps_boxes_after_every_update(mods):
    ndt, po, clouds = mods
    from toyslam_amd import _lib
    g = ndt.NormalDistributionsTransform()
    with pytest.raises(ndt.NdtError) as e:
        g.inputBounds("map")
    assert e.value.status == _lib.NDT_ERR_NO_INPUT
    rng = np.random.default_rng(31)
    ref = np.zeros((0, 3), F32)
    for k in range(3):
        scan = (rng.uniform(-20, 20, (30000, 3)) * [1, 1, 0.1]).astype(F32)
        T = clouds.make_T([3.0 * k, -2.0 * k, 0.1 * k], np.deg2rad([1.0 * k, -2.0 * k, 30.0 * k])).astype(F32)
        g.mapUpdate(scan, T, LEAF)
        moved = po.transform_cloud(np.c_[scan, np.ones(len(scan), F32)], T)[:, :3]
        ref = filtered(po, np.concatenate([ref, moved]))
        boxes, route = g.inputBounds("map")  # (first: the read-out itself waits for the queued update)
        got = g.mapGet()
        assert np.array_equal(got, ref), k
        check((boxes, route), got, "filter_rows", k)
    g.mapClear()
    with pytest.raises(ndt.NdtError):
        g.inputBounds("map")
