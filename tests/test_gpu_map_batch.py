"""GPU: ndt_map_update_clouds / ndt_map_update_batch -- many posed scans into the map in one call: transformPointCloud of
every scan, one += of all of them, ONE VoxelGrid filter.  Every comparison is bit for bit (np.array_equal) against the
oracle's transform_cloud + voxel_grid_filter of the concatenation [map | scan 0 | scan 1 | ...]."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_pairs import build_app, matrices, sequence
from test_gpu_parity import _DeviceCopies

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from oracle import pyoracle as po
    from toyslam_amd import clouds, ndt
    return ndt, po, clouds


def chain_poses(clouds, n=8):
    """the poses test_gpu_pairs.sequence walks (the same generator, the same draws): scan k moved by poses[k] is back in the world"""
    rng = np.random.default_rng(19)
    pose, out = np.eye(4), []
    for k in range(n):
        if k:
            pose = pose @ clouds.make_T(rng.uniform(-0.4, 0.4, 3) * [1, 1, 0.05], np.deg2rad(rng.uniform(-1.5, 1.5, 3) * [0.2, 0.2, 1]))
        rng.choice(60000, 30000, replace=False)
        rng.normal(0, 0.01, (30000, 3))
        out.append(pose.astype(np.float32))
    return out


@pytest.fixture(scope="module")
def seq(mods, tmp_path_factory):
    """8 scans of 30 000 points, raw and prefiltered at 0.5 m (the oracle's filter), their poses, and the PCD directory"""
    ndt, po, clouds = mods
    scans, d = sequence(clouds, ndt, tmp_path_factory.mktemp("seq"), n=8)
    poses = chain_poses(clouds, 8)
    back = clouds.apply_T(poses[7].astype(np.float64), scans[7])  # (the poses ARE the helper's: the last scan's ground is the world's, z = 0)
    assert (np.abs(back[:, 2]) < 0.06).mean() > 0.35 > (np.abs(scans[7][:, 2]) < 0.06).mean()
    filt = [po.voxel_grid_filter(sc, 0.5)[0] for sc in scans]
    return dict(raw=scans, filt=filt, poses=poses, dir=d)


def moved(po, scan, pose):
    return po.transform_cloud(np.c_[scan[:, :3], np.ones(len(scan), np.float32)], pose)[:, :3]


def moved_keeping_non_finite(po, scan, pose):
    """transformPointCloud of a cloud that is not dense: finite rows moved, the others left as they are"""
    out = scan[:, :3].copy()
    ok = np.isfinite(scan[:, :3]).all(axis=1)
    out[ok] = moved(po, scan[ok], pose)
    return out


def oracle_map(po, before, scans, poses, leaf, is_dense=True):
    cat = np.concatenate([before] + [moved(po, s, T) for s, T in zip(scans, poses)])
    return po.voxel_grid_filter(cat, leaf, is_dense=is_dense)


EMPTY = np.zeros((0, 3), np.float32)


# ---- 1, 8: the oracle on an empty map; not the loop's map; one pass
@pytest.mark.parametrize("leaf", [0.5, 0.2])
def test_one_call_is_the_oracles_one_filter_of_the_concatenation(mods, seq, leaf):
    ndt, po, clouds = mods
    g = ndt.NormalDistributionsTransform()
    dcs = [g.uploadCloud(c) for c in seq["filt"]]
    n_map, ov = g.mapUpdateClouds(dcs, seq["poses"], leaf_size=leaf)
    ref, ov_ref = oracle_map(po, EMPTY, seq["filt"], seq["poses"], leaf)
    got = g.mapGet()
    print("leaf %.1f: map %d points, oracle %d, overflow %s / %s" % (leaf, n_map, len(ref), ov, ov_ref))
    assert not ov and not ov_ref and n_map == len(ref)
    assert np.array_equal(got, ref)
    diag = g.mapBatchDiag()
    print("diag", diag)
    assert diag["transform_launches"] == 1 and diag["filters"] == 1 and diag["box_passes"] <= 1
    # the per-scan loop's map is another map (centroids of centroids): an implementation that loops inside would give it
    h = ndt.NormalDistributionsTransform()
    for dc, T in zip([h.uploadCloud(c) for c in seq["filt"]], seq["poses"]):
        h.mapUpdateCloud(dc, T, leaf_size=leaf)
    loop = h.mapGet()
    print("loop's map %d points, max |difference| %s" % (len(loop), np.abs(loop - got).max(axis=0) if loop.shape == got.shape else "-"))
    assert not np.array_equal(loop, got)


# ---- 2: onto a map, and the single call continues
@pytest.mark.parametrize("leaf", [0.5, 0.2])
def test_batch_onto_a_map_then_single_updates_continue(mods, seq, leaf):
    ndt, po, clouds = mods
    g = ndt.NormalDistributionsTransform()
    dcs = [g.uploadCloud(c) for c in seq["filt"]]
    ref = EMPTY
    for k in range(3):
        g.mapUpdateCloud(dcs[k], seq["poses"][k], leaf_size=leaf)
        ref, _ = oracle_map(po, ref, [seq["filt"][k]], [seq["poses"][k]], leaf)
    assert np.array_equal(g.mapGet(), ref)
    n_map, ov = g.mapUpdateClouds(dcs[3:], seq["poses"][3:], leaf_size=leaf)
    ref, ov_ref = oracle_map(po, ref, seq["filt"][3:], seq["poses"][3:], leaf)
    assert not ov and not ov_ref and n_map == len(ref)
    assert np.array_equal(g.mapGet(), ref)
    extra = clouds.make_T([0.5, 0.2, 0.0], np.deg2rad([0.1, 0.0, 2.0])).astype(np.float32)
    g.mapUpdateCloud(dcs[0], extra, leaf_size=leaf)
    ref, _ = oracle_map(po, ref, [seq["filt"][0]], [extra], leaf)
    assert np.array_equal(g.mapGet(), ref)


# ---- 3: a batch of one is the single call
def test_one_scan_is_the_single_call(mods, seq, pair):
    ndt, po, clouds = mods
    t, s = pair
    T = clouds.make_T([0.30, -0.20, 0.10], np.deg2rad([0.5, -0.3, 1.0])).astype(np.float32)
    far = np.array([[0, 0, 0], [1e6, 1e6, 1e6]], np.float32)
    away = (s[:2000] + np.float32([1e5, 0, 0])).astype(np.float32)  # onto a map: 1e7 x 1e4 x 2e3 voxels of 0.01 m, far above 2^31
    with _DeviceCopies() as dev:
        for first, scan, pose, leaf, want_ov in [(t, s, T, 0.5, False), (seq["filt"][0], seq["raw"][1], seq["poses"][1], 0.2, False),
                                                 (None, far, None, 0.01, True), (t, away, None, 0.01, True)]:
            rec = np.c_[scan, np.ones(len(scan), np.float32)]
            d_rec = dev.put(rec)
            results = []
            for form in ("cloud", "clouds", "host", "batch", "device", "batch_device"):
                g = ndt.NormalDistributionsTransform()
                if first is not None:
                    g.mapUpdate(first, None, leaf)
                P = None if pose is None else [pose]
                if form == "cloud":
                    r = g.mapUpdateCloud(g.uploadCloud(scan), pose, leaf)
                elif form == "clouds":
                    r = g.mapUpdateClouds([g.uploadCloud(scan)], P, leaf)
                elif form == "host":
                    r = g.mapUpdate(scan, pose, leaf)
                elif form == "batch":
                    r = g.mapUpdateBatch([scan], P, leaf)
                elif form == "device":
                    r = g.mapUpdateDevice(d_rec, len(scan), 16, pose, leaf)
                else:
                    r = g.mapUpdateBatchDevice(d_rec, [0, len(scan)], 16, P, leaf)
                results.append((form, r, g.mapGet()))
            for form, r, m in results:
                assert r == results[0][1], (form, r, results[0][1])
                assert r[1] == want_ov, (form, r)
                assert np.array_equal(m, results[0][2]), form
            if first is None and want_ov:
                assert results[1][1] == (2, True) and np.array_equal(results[1][2], far)  # PCL keeps the unfiltered concatenation


# ---- 4: all forms one answer
def test_all_forms_give_one_map(mods, seq):
    ndt, po, clouds = mods
    scans, poses = seq["raw"][:5], seq["poses"][:5]
    ref, _ = oracle_map(po, po.voxel_grid_filter(seq["raw"][7], 0.5)[0], scans, poses, 0.5)

    def fresh():
        g = ndt.NormalDistributionsTransform()
        g.mapUpdate(seq["raw"][7], None, 0.5)
        return g

    g = fresh()
    g.mapUpdateClouds([g.uploadCloud(c) for c in scans], poses, 0.5)
    assert np.array_equal(g.mapGet(), ref)
    off = np.concatenate([[0], np.cumsum([len(c) for c in scans])])
    with _DeviceCopies() as dev:
        for cols in (3, 4, 8):  # strides 12, 16, 32
            wide = [np.c_[c, np.full((len(c), cols - 3), 7.0, np.float32)] if cols > 3 else c for c in scans]
            g = fresh()
            n_map, ov = g.mapUpdateBatch(wide, poses, 0.5)
            assert n_map == len(ref) and not ov and np.array_equal(g.mapGet(), ref), cols
            assert g.mapBatchDiag() == dict(transform_launches=1, filters=1, box_passes=0)
            g = fresh()
            n_map, ov = g.mapUpdateBatchDevice(dev.put(np.concatenate(wide)), off, 4 * cols, poses, 0.5)
            assert n_map == len(ref) and not ov and np.array_equal(g.mapGet(), ref), cols
        # a buffer that starts behind records of somebody else: offsets[0] > 0
        g = fresh()
        lead = np.full((11, 4), np.nan, np.float32)
        g.mapUpdateBatchDevice(dev.put(np.concatenate([lead] + [np.c_[c, np.ones(len(c), np.float32)] for c in scans])), off + 11, 16, poses, 0.5)
        assert np.array_equal(g.mapGet(), ref)


# ---- 5: NaN rules
def test_nan_rules_per_scan(mods, seq):
    ndt, po, clouds = mods
    rng = np.random.default_rng(5)
    scans = [c.copy() for c in seq["raw"][:4]]
    for k in (1, 2):
        rows = rng.choice(len(scans[k]), 300, replace=False)
        scans[k][rows[:100], rng.integers(0, 3, 100)] = np.nan
        scans[k][rows[100:200], rng.integers(0, 3, 100)] = np.inf
        scans[k][rows[200:], :] = -np.inf
    poses = seq["poses"][:4]
    dense = [1, 0, 0, 1]
    cat = np.concatenate([moved(po, s, T) if d else moved_keeping_non_finite(po, s, T) for s, T, d in zip(scans, poses, dense)])
    ref, ov_ref = po.voxel_grid_filter(cat, 0.5, is_dense=False)
    print("NaN rules: %d points" % len(ref))
    assert not ov_ref and len(ref) > 0
    g = ndt.NormalDistributionsTransform()
    n_map, ov = g.mapUpdateClouds([g.uploadCloud(c) for c in scans], poses, 0.5, is_dense=dense)
    assert not ov and n_map == len(ref) and np.array_equal(g.mapGet(), ref)
    h = ndt.NormalDistributionsTransform()
    n_map, ov = h.mapUpdateBatch(scans, poses, 0.5, is_dense=dense)
    assert not ov and n_map == len(ref) and np.array_equal(h.mapGet(), ref)
    # ... and onto a dense map: the concatenation is dense only if the map was and every scan is
    h.mapClear()
    h.mapUpdate(seq["filt"][6], None, 0.5)
    h.mapUpdateBatch(scans, poses, 0.5, is_dense=dense)
    ref2, _ = po.voxel_grid_filter(np.concatenate([seq["filt"][6], cat]), 0.5, is_dense=False)
    assert np.array_equal(h.mapGet(), ref2)


# ---- 6: empty members
def test_empty_scans_change_nothing(mods, seq):
    ndt, po, clouds = mods
    scans, poses = seq["filt"][:3], seq["poses"][:3]
    ref, _ = oracle_map(po, EMPTY, scans, poses, 0.5)
    I = np.eye(4, dtype=np.float32)
    with_empties = [EMPTY, scans[0], EMPTY, EMPTY, scans[1], scans[2], EMPTY]
    their_poses = [poses[1], poses[0], I, poses[2], poses[1], poses[2], poses[0]]
    g = ndt.NormalDistributionsTransform()
    n_map, ov = g.mapUpdateClouds([g.uploadCloud(c) for c in with_empties], their_poses, 0.5)
    assert n_map == len(ref) and not ov and np.array_equal(g.mapGet(), ref)
    assert g.mapBatchDiag()["transform_launches"] == 1
    h = ndt.NormalDistributionsTransform()
    h.mapUpdateBatch(with_empties, their_poses, 0.5)
    assert np.array_equal(h.mapGet(), ref)
    # all empty: the map is filtered again, as the single call does with an empty scan -- here at another leaf size
    again, _ = po.voxel_grid_filter(ref, 0.8)
    n_map, ov = g.mapUpdateClouds([g.uploadCloud(EMPTY), g.uploadCloud(EMPTY)], None, 0.8)
    assert n_map == len(again) and np.array_equal(g.mapGet(), again)
    assert g.mapBatchDiag() == dict(transform_launches=0, filters=1, box_passes=0)
    h.mapUpdateBatch([EMPTY, EMPTY, EMPTY], None, 0.8)
    assert np.array_equal(h.mapGet(), again)
    # all empty onto an empty map: nothing at all
    e = ndt.NormalDistributionsTransform()
    assert e.mapUpdateBatch([EMPTY, EMPTY], None, 0.5) == (0, False) and e.mapGet().shape == (0, 3)
    assert e.mapUpdateClouds([e.uploadCloud(EMPTY)], None, 0.5) == (0, False)
    assert e.mapUpdateClouds([]) == (0, False)


# ---- 7: the filter's routes
CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toyslam_amd import ndt
d = np.load(sys.argv[2])
n = int(d["n"])
g = ndt.NormalDistributionsTransform()
g.mapUpdateClouds([g.uploadCloud(d["s%d" % k]) for k in range(n)], [d["T%d" % k] for k in range(n)], float(d["leaf"]))
np.save(sys.argv[3], g.mapGet())
print(json.dumps(g.mapBatchDiag()))
"""


def test_every_filter_route_gives_the_same_bytes(mods, seq, tmp_path):
    ndt, po, clouds = mods
    ref, _ = oracle_map(po, EMPTY, seq["filt"], seq["poses"], 0.5)
    data = dict(n=8, leaf=0.5)
    for k in range(8):
        data["s%d" % k], data["T%d" % k] = seq["filt"][k], seq["poses"][k]
    np.savez(str(tmp_path / "in.npz"), **data)
    for name, extra in (("chain", {"NDT_VF": "chain"}), ("buckets", {"NDT_VF_FROM": "0"}), ("default", {})):
        env = {k: v for k, v in os.environ.items() if k not in ("NDT_VF", "NDT_VF_FROM")}
        env.update(extra)
        out_path = str(tmp_path / (name + ".npy"))
        out = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "in.npz"), out_path], env=env, capture_output=True,
                             text=True, timeout=300)
        assert out.returncode == 0, (name, out.stderr)
        diag = json.loads(out.stdout.strip().splitlines()[-1])
        assert diag == dict(transform_launches=1, filters=1, box_passes=0), (name, diag)
        assert np.array_equal(np.load(out_path), ref), name


def test_forty_scans_onto_a_map_take_the_bucket_front_end(mods):
    """40 prefiltered node scans onto a non-empty map: far above the size from which the filter takes the bucket front end"""
    ndt, po, clouds = mods
    from test_gpu_filter_batch import node_scans
    raw = node_scans(clouds, 41, n_raw=60000, seed=3)
    poses, pose = [], np.eye(4)
    for k in range(41):  # node_scans' own walk
        if k:
            pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
        poses.append(pose.astype(np.float32))
    g = ndt.NormalDistributionsTransform()
    dcs, _ = g.voxelGridFilterClouds(raw, 0.5)
    filt = [dc.numpy() for dc in dcs]
    total = sum(len(c) for c in filt)
    print("41 prefiltered scans: %d points, %d per scan" % (total, total // 41))
    assert total - len(filt[0]) > 131072
    g.mapUpdateCloud(dcs[0], poses[0], 0.5)
    n_map, ov = g.mapUpdateClouds(dcs[1:], poses[1:], 0.5)
    first, _ = oracle_map(po, EMPTY, filt[:1], poses[:1], 0.5)
    ref, ov_ref = oracle_map(po, first, filt[1:], poses[1:], 0.5)
    assert not ov and not ov_ref and n_map == len(ref)
    assert np.array_equal(g.mapGet(), ref)
    assert g.mapBatchDiag() == dict(transform_launches=1, filters=1, box_passes=0)


# ---- 9: lifetime and bystanders
def test_inputs_may_go_at_once_and_bystanders_are_untouched(mods, seq, pair):
    ndt, po, clouds = mods
    t, s = pair
    g = ndt.NormalDistributionsTransform()
    g.setTransformationEpsilon(0.01)
    g.setMaximumIterations(40)
    r = g.alignPairs(seq["filt"][:3])
    fit = g.pairsFitness()
    g.setInputTarget(t)
    g.setInputSource(s)
    g.align()
    T, it, score = g.getFinalTransformation(), g.getFinalNumIteration(), g.getFitnessScore()
    pending = g.uploadCloud(seq["raw"][6])
    g.voxelGridFilterBegin(pending, 0.5)
    dcs = [g.uploadCloud(c) for c in seq["filt"]]
    n_map, ov = g.mapUpdateClouds(dcs, seq["poses"], 0.5)
    for dc in dcs:
        dc.release()  # the handle keeps every scan until the update is complete
    del dcs
    churn = [g.uploadCloud(c) for c in seq["raw"][:4]]  # (what the released blocks would be recycled for)
    ref, _ = oracle_map(po, EMPTY, seq["filt"], seq["poses"], 0.5)
    assert n_map == len(ref) and np.array_equal(g.mapGet(), ref)
    del churn
    done, ov = g.voxelGridFilterEnd()
    assert not ov and np.array_equal(done.numpy(), po.voxel_grid_filter(seq["raw"][6], 0.5)[0])
    assert np.array_equal(g.getFinalTransformation(), T) and g.getFinalNumIteration() == it
    assert g.getFitnessScore() == score
    assert np.array_equal(g.pairsFitness(), fit)
    g.align()  # target, source and grid are the ones set before the map call
    assert np.array_equal(g.getFinalTransformation(), T) and g.getFinalNumIteration() == it
    assert r["T"].shape == (2, 4, 4)
    # the buffer form: the caller's buffer is free when the call returns
    h = ndt.NormalDistributionsTransform()
    off = np.concatenate([[0], np.cumsum([len(c) for c in seq["filt"]])]).astype(np.uintp)
    with _DeviceCopies() as dev:
        cat = np.concatenate([np.c_[c, np.ones(len(c), np.float32)] for c in seq["filt"]])
        p = dev.put(cat)
        h.mapUpdateBatchDevice(p, off, 16, seq["poses"], 0.5)
        dev.hip.hipMemset.argtypes = [dev.C.c_void_p, dev.C.c_int, dev.C.c_size_t]
        assert dev.hip.hipMemset(p, 0xFF, cat.nbytes) == 0
    assert np.array_equal(h.mapGet(), ref)


# ---- calls that follow each other without a size query in between: the second finds the first still queued
def c_clouds(g, dcs, poses, leaf):
    """ndt_map_update_clouds itself: the wrapper would ask for the map's size, which waits for the update"""
    import ctypes as C
    arr = (C.c_void_p * len(dcs))(*[dc._c for dc in dcs])
    dense = np.ones(len(dcs), np.int32)
    P = np.ascontiguousarray(np.stack([np.asarray(T, np.float32).T.reshape(16) for T in poses]))
    ov = C.c_int(7)
    st = g._L.ndt_map_update_clouds(g._h, arr, len(dcs), dense.ctypes.data_as(C.POINTER(C.c_int)), P.ctypes.data_as(C.POINTER(C.c_float)),
                                    leaf, C.byref(ov))
    return st, ov.value


def c_buffer(g, ptr, offsets, poses, leaf, on_device=1, stride=16):
    import ctypes as C
    off = np.ascontiguousarray(offsets, dtype=np.uintp)
    n = len(off) - 1
    dense = np.ones(n, np.int32)
    P = np.ascontiguousarray(np.stack([np.asarray(T, np.float32).T.reshape(16) for T in poses]))
    ov = C.c_int(7)
    st = g._L.ndt_map_update_batch(g._h, C.c_void_p(ptr), off.ctypes.data_as(C.POINTER(C.c_size_t)), n, stride,
                                   dense.ctypes.data_as(C.POINTER(C.c_int)), P.ctypes.data_as(C.POINTER(C.c_float)), leaf, on_device,
                                   C.byref(ov))
    return st, ov.value


@pytest.mark.parametrize("first_form", ["clouds", "buffer"])
def test_back_to_back_calls_without_a_size_query(mods, seq, first_form):
    """A batched call queues its descriptor copy and returns; the next call must not touch what that copy still reads.
    Several rounds, the second call a device buffer (nothing blocking in front of its staging) of more scans than the first
    (its descriptors need a larger block), every map against the oracle."""
    ndt, po, clouds = mods
    filt, poses = seq["filt"], seq["poses"]
    rec = [np.c_[c, np.ones(len(c), np.float32)] for c in filt]

    def offsets(lo, hi):
        return np.concatenate([[0], np.cumsum([len(c) for c in filt[lo:hi]])]).astype(np.int64)

    with _DeviceCopies() as dev:
        d_a, d_b = dev.put(np.concatenate(rec[:3])), dev.put(np.concatenate(rec[3:]))
        g = ndt.NormalDistributionsTransform()
        dcs = [g.uploadCloud(c) for c in filt[:3]]
        ref = EMPTY
        for rnd in range(4):
            if first_form == "clouds":
                assert c_clouds(g, dcs, poses[:3], 0.5) == (0, 0)
            else:
                assert c_buffer(g, d_a, offsets(0, 3), poses[:3], 0.5) == (0, 0)
            assert c_buffer(g, d_b, offsets(3, 8), poses[3:], 0.5) == (0, 0)  # (no ndt_map_size in between)
            ref, _ = oracle_map(po, ref, filt[:3], poses[:3], 0.5)
            ref, _ = oracle_map(po, ref, filt[3:], poses[3:], 0.5)
            assert g.mapBatchDiag() == dict(transform_launches=1, filters=1, box_passes=0)
            assert np.array_equal(g.mapGet(), ref), rnd
        # ... and host buffers, three calls in a row
        h = ndt.NormalDistributionsTransform()
        cat = np.concatenate(rec)
        for lo, hi in ((0, 2), (2, 7), (7, 8)):
            part = np.ascontiguousarray(cat[offsets(0, lo)[-1]:offsets(0, hi)[-1]])
            assert c_buffer(h, part.ctypes.data, offsets(lo, hi), poses[lo:hi], 0.5, on_device=0) == (0, 0)
        ref = EMPTY
        for lo, hi in ((0, 2), (2, 7), (7, 8)):
            ref, _ = oracle_map(po, ref, filt[lo:hi], poses[lo:hi], 0.5)
        assert np.array_equal(h.mapGet(), ref)


def test_a_total_above_int_max_onto_a_queued_map_is_refused_before_the_buffer_is_read(mods, seq):
    """map + scans above INT_MAX points while the map's size is still open (an update queued, not waited for): refused once
    that update is settled and before anything of the call is copied -- the offsets reach far beyond the 16 bytes behind
    the pointer -- and the map is what the queued update made it."""
    ndt, po, clouds = mods
    from toyslam_amd import _lib
    g = ndt.NormalDistributionsTransform()
    dcs = [g.uploadCloud(c) for c in seq["filt"][:2]]
    assert c_clouds(g, dcs, seq["poses"][:2], 0.5) == (0, 0)  # queued: the size is not asked for
    ref, _ = oracle_map(po, EMPTY, seq["filt"][:2], seq["poses"][:2], 0.5)
    room = 2 ** 31 - 1 - len(ref)
    with _DeviceCopies() as dev:
        tiny = dev.put(np.ones((1, 4), np.float32))
        for on_device in (1, 0):
            ptr = tiny if on_device else np.ones((1, 4), np.float32).ctypes.data
            assert c_buffer(g, ptr, [0, 1, room + 1], seq["poses"][:2], 0.5, on_device=on_device) == (_lib.NDT_ERR_INVALID, 0)
            assert g.mapBatchDiag() == dict(transform_launches=0, filters=0, box_passes=0)
            assert np.array_equal(g.mapGet(), ref)
            assert c_clouds(g, dcs[:1], seq["poses"][:1], 0.5) == (0, 0)  # the map goes on
            ref, _ = oracle_map(po, ref, seq["filt"][:1], seq["poses"][:1], 0.5)
            room = 2 ** 31 - 1 - len(ref)


# ---- 10: the app
def test_pair_sequence_writes_the_map(mods, seq, tmp_path):
    ndt, po, clouds = mods
    exe = build_app(tmp_path, "pair_sequence")
    out_pcd = str(tmp_path / "out.pcd")
    keep = lambda out: [ln for ln in out.splitlines() if not ln.startswith("time:")]  # noqa: E731
    plain = subprocess.run([exe, str(seq["dir"])], capture_output=True, text=True, timeout=300)
    mapped = subprocess.run([exe, str(seq["dir"]), "--map", out_pcd], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and mapped.returncode == 0, (plain.stderr, mapped.stderr)
    no_name = subprocess.run([exe, str(seq["dir"]), "--map"], capture_output=True, text=True, timeout=300)
    assert no_name.returncode == 2 and "--map needs a file name" in no_name.stderr and no_name.stdout == ""
    map_lines = [ln for ln in mapped.stdout.splitlines() if ln.startswith("map:")]
    assert len(map_lines) == 1 and not any(ln.startswith("map:") for ln in plain.stdout.splitlines())
    assert [ln for ln in keep(mapped.stdout) if not ln.startswith("map:")] == keep(plain.stdout)
    chain = [np.eye(4, dtype=np.float32)] + [m.astype(np.float32) for m in matrices(mapped.stdout, "TransformSum")]
    assert len(chain) == 8
    g = ndt.NormalDistributionsTransform()
    dcs = [g.voxelGridFilterCloud(sc, 0.5)[0] for sc in seq["raw"]]
    n_map, ov = g.mapUpdateClouds(dcs, chain, 0.5)
    got, dense = ndt.pcd_read_xyz(out_pcd)
    assert map_lines[0] == "map: %d points" % n_map
    assert dense and np.array_equal(got, g.mapGet())
    assert np.array_equal(got, oracle_map(po, EMPTY, seq["filt"], chain, 0.5)[0])
