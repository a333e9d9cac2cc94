"""GPU: ndt_cloud_voxel_filter_batch / _clouds -- N1 of many clouds in one call.  Every cloud's result must be what
ndt_cloud_voxel_filter returns for it alone and what the oracle's pcl::VoxelGrid returns (np.array_equal), whatever the
other clouds, their order and the form of the call; the results must work downstream and live as long as they are held;
and the composite pass must be what ran."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_pairs import build_app, sequence
from test_gpu_parity import _DeviceCopies

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from oracle import pyoracle as po
    from toyslam_amd import clouds, ndt
    return ndt, po, clouds


def node_scans(clouds, n, n_raw=60000, seed=3):
    """tools/time_pairs.py's scans: a static world seen from a moving pose"""
    rng = np.random.default_rng(seed)
    world = clouds.target_surfaces(4 * n_raw, seed=77, extent=60.0)[:, :3].astype(np.float32)
    pose, out = np.eye(4), []
    for k in range(n):
        if k:
            pose = pose @ clouds.make_T([0.3, 0.05 * np.sin(k), 0.0], np.deg2rad([0.0, 0.0, 1.0]))
        pick = world[rng.choice(len(world), n_raw, replace=False)]
        out.append((clouds.apply_T(np.linalg.inv(pose), pick) + rng.normal(0, 0.01, pick.shape)).astype(np.float32))
    return out


def ragged(clouds):
    """(clouds, is_dense flags): every route of the single filter"""
    rng = np.random.default_rng(11)
    node = node_scans(clouds, 2)
    small = node[0][:15000].copy()                                                       # host-staged in the single call
    big = np.c_[rng.uniform(-30, 30, (200000, 2)), rng.uniform(0, 10, 200000)].astype(np.float32)  # bucket front end at 0.5
    wide = np.c_[rng.uniform(-150, 150, (60000, 2)), rng.uniform(-2, 8, 60000)].astype(np.float32)  # sparse route
    utm = (node[1][::3] * np.float32(0.2) + np.array([4.5e5, 5.0e6, 0.0], np.float32)).astype(np.float32)
    nan = node[1][:30000].copy()
    nan[::7] = np.nan
    nan[3::11, 1] = np.inf
    overflow = np.array([[0, 0, 0], [1e6, 1e6, 1e6]], np.float32)                         # copy-through, flag set
    empty = np.zeros((0, 3), np.float32)
    one = np.array([[1.25, -2.5, 3.75]], np.float32)
    all_nan = np.full((40, 3), np.nan, np.float32)
    cl = [node[0], small, big, wide, utm, nan, overflow, empty, one, all_nan, node[1]]
    dense = [True, True, True, True, True, False, True, True, True, False, True]
    return cl, dense


def single(g, c, leaf, dense):
    dc, ov = g.voxelGridFilterCloud(c, leaf, is_dense=dense)
    return dc.numpy(), ov


def check_against_single(g, po, cl, dense, leaf, outs, ovs, oracle=True):
    assert len(outs) == len(cl)
    for k, (c, d) in enumerate(zip(cl, dense)):
        ref, ref_ov = single(g, c, leaf, d)
        got = outs[k].numpy()
        assert np.array_equal(got, ref, equal_nan=True), (k, leaf, got.shape, ref.shape)
        assert bool(ovs[k]) == ref_ov, k
        if oracle:
            o, o_ov = po.voxel_grid_filter(c, leaf, is_dense=d)
            assert np.array_equal(got, o, equal_nan=True), (k, leaf, "oracle")
            assert bool(ovs[k]) == o_ov, k


@pytest.mark.parametrize("leaf", [0.5, 0.1])
def test_ragged_set_in_one_call(mods, leaf):
    ndt, po, clouds = mods
    cl, dense = ragged(clouds)
    g = ndt.NormalDistributionsTransform()
    outs, ovs = g.voxelGridFilterClouds(cl, leaf, is_dense=dense)
    assert ovs[6] and not ovs[:6].any()
    assert len(outs[7]) == 0 and len(outs[9]) == 0 and len(outs[8]) == 1
    check_against_single(g, po, cl, dense, leaf, outs, ovs)
    d = g.filterBatchDiag()
    assert d["passes"] >= 1 and d["single_route"] >= 2  # (the wide scan and the copy-through at least)


@pytest.mark.parametrize("leaf", [0.5, 0.3])
def test_reference_pair(mods, reference_pcd, leaf):
    ndt, po, clouds = mods
    cl, dn = zip(*[ndt.pcd_read_xyz(p) for p in reference_pcd])
    g = ndt.NormalDistributionsTransform()
    outs, ovs = g.voxelGridFilterClouds(list(cl), leaf, is_dense=list(dn))
    check_against_single(g, po, list(cl), list(dn), leaf, outs, ovs)


def test_all_forms_are_one_answer(mods):
    ndt, po, clouds = mods
    cl, dense = ragged(clouds)
    g = ndt.NormalDistributionsTransform()
    ref, ref_ov = g.voxelGridFilterClouds(cl, 0.5, is_dense=dense)
    ref = [o.numpy() for o in ref]
    offsets = np.r_[0, np.cumsum([len(c) for c in cl])]
    cat = np.concatenate(cl).astype(np.float32)
    with _DeviceCopies() as dev:
        for cols in (4, 8):  # stride 16 and stride 32
            rec = np.zeros((len(cat), cols), np.float32)
            rec[:, :3] = cat
            rec[:, 3:] = 7.0  # garbage behind xyz
            outs, ovs = g.voxelGridFilterBatchDevice(dev.put(rec), offsets, 4 * cols, 0.5, is_dense=dense)
            assert np.array_equal(ovs, ref_ov)
            for k in range(len(cl)):
                assert np.array_equal(outs[k].numpy(), ref[k], equal_nan=True), (cols, k)
    raw = [g.uploadCloud(c) for c in cl]
    outs, ovs = g.voxelGridFilterClouds(raw, 0.5, is_dense=dense)
    assert np.array_equal(ovs, ref_ov)
    for k in range(len(cl)):
        assert np.array_equal(outs[k].numpy(), ref[k], equal_nan=True), ("clouds", k)


def test_independence_of_order_and_company(mods):
    ndt, po, clouds = mods
    cl, dense = ragged(clouds)
    g = ndt.NormalDistributionsTransform()
    ref = [single(g, c, 0.5, d)[0] for c, d in zip(cl, dense)]
    rng = random.Random(5)
    for trial in range(4):
        idx = list(range(len(cl))) + [0, 5, 5]  # duplicates
        rng.shuffle(idx)
        idx = idx[: rng.randint(3, len(idx))]  # subsets
        outs, _ = g.voxelGridFilterClouds([cl[i] for i in idx], 0.5, is_dense=[dense[i] for i in idx])
        for o, i in zip(outs, idx):
            assert np.array_equal(o.numpy(), ref[i], equal_nan=True), (trial, i)


CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toyslam_amd import ndt
cl = [np.load(p) for p in sys.argv[3:]]
g = ndt.NormalDistributionsTransform()
outs, ovs = g.voxelGridFilterClouds(cl, 0.5)
np.savez(sys.argv[2], *[o.numpy() for o in outs])
print(json.dumps(g.filterBatchDiag()))
"""


def test_passes_and_the_single_route_by_budget(mods, tmp_path):
    """NDT_VF_BATCH_CELLS small (read once: a child process): several passes, a cloud beyond the budget on the single route,
    the same bits"""
    ndt, po, clouds = mods
    rng = np.random.default_rng(2)
    cl = [np.c_[rng.uniform(0, 10, (2000, 2)), rng.uniform(0, 2, 2000)].astype(np.float32) + np.float32(3 * k) for k in range(7)]
    cl.insert(3, np.c_[rng.uniform(0, 40, (5000, 2)), rng.uniform(0, 4, 5000)].astype(np.float32))  # ~51 k cells at 0.5
    g = ndt.NormalDistributionsTransform()
    ref = [single(g, c, 0.5, True)[0] for c in cl]
    paths = []
    for k, c in enumerate(cl):
        p = str(tmp_path / ("c%d.npy" % k))
        np.save(p, c)
        paths.append(p)
    env = dict(os.environ, NDT_VF_BATCH_CELLS="4000")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "out.npz")] + paths, env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    diag = json.loads(out.stdout.strip().splitlines()[-1])
    assert diag["passes"] > 1 and diag["single_route"] == 1, diag
    got = np.load(str(tmp_path / "out.npz"))
    for k in range(len(cl)):
        assert np.array_equal(got["arr_%d" % k], ref[k]), k


def test_downstream_consumers_see_the_same_clouds(mods):
    ndt, po, clouds = mods
    scans = node_scans(clouds, 4, n_raw=20000, seed=8)
    g = ndt.NormalDistributionsTransform()
    batch, _ = g.voxelGridFilterClouds(scans, 0.5)
    one = [g.voxelGridFilterCloud(s, 0.5)[0] for s in scans]

    def run(dcs):
        h = ndt.NormalDistributionsTransform()
        h.setTransformationEpsilon(0.01)
        h.setMaximumIterations(64)
        r = h.alignPairs(dcs)
        h.setInputTargetCloud(dcs[0])
        h.setInputSourceCloud(dcs[1])
        h.align()
        T1 = h.getFinalTransformation()
        h.promoteSourceToTarget()
        h.setInputSourceCloud(dcs[2])
        h.align()
        T2 = h.getFinalTransformation()
        h.mapUpdateCloud(dcs[0])
        h.mapUpdateCloud(dcs[3], pose=T1)
        return r["T"], T1, T2, h.mapGet()

    for a, b in zip(run(batch), run(one)):
        assert np.array_equal(a, b)


def _hip():
    import ctypes as C
    import re
    linked = [m.group(1) for m in re.finditer(r"(/\S*libamdhip64\.so[.\d]*)", open("/proc/self/maps").read()) if "/torch/" not in m.group(1)]
    hip = C.CDLL(linked[0] if linked else "libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value
    return free_bytes


def test_lifetime_of_the_slices(mods):
    import ctypes as C
    ndt, po, clouds = mods
    scans = node_scans(clouds, 6, n_raw=20000, seed=4)
    g = ndt.NormalDistributionsTransform()
    ref = [g.voxelGridFilterCloud(s, 0.5)[0].numpy() for s in scans]
    # released in random order: the others stay valid
    outs, _ = g.voxelGridFilterClouds(scans, 0.5)
    order = list(range(len(outs)))
    random.Random(3).shuffle(order)
    for i, k in enumerate(order):
        outs[k].release()
        for j in order[i + 1:]:
            assert np.array_equal(outs[j].numpy(), ref[j])
    # outputs that outlive the handle that made them, read by another handle (its own stream)
    L = g._L
    h2 = C.c_void_p()
    assert L.ndt_create(0, C.byref(h2)) == 0
    arr = (C.c_void_p * len(scans))()
    cat = np.concatenate(scans)
    off = np.r_[0, np.cumsum([len(s) for s in scans])].astype(np.uintp)
    dn = np.ones(len(scans), np.int32)
    assert L.ndt_cloud_voxel_filter_batch(h2, cat.ctypes.data, off.ctypes.data_as(C.POINTER(C.c_size_t)), len(scans), 12,
                                          dn.ctypes.data_as(C.POINTER(C.c_int)), 0.5, 0, arr, None) == 0
    L.ndt_destroy(h2)
    kept = [ndt.DeviceCloud(g, C.c_void_p(arr[k])) for k in range(len(scans))]
    for k in range(len(scans)):
        assert np.array_equal(kept[k].numpy(), ref[k])
    other = ndt.NormalDistributionsTransform()
    other.setInputTargetCloud(kept[0])
    other.setInputSourceCloud(kept[1])
    other.align()
    base = ndt.NormalDistributionsTransform()
    base.setInputTarget(ref[0])
    base.setInputSource(ref[1])
    base.align()
    assert np.array_equal(other.getFinalTransformation(), base.getFinalTransformation())
    del kept, other
    # the device's free memory: the same after the 2nd and the 50th call (the pool holds the sizes after the first)
    free_bytes = _hip()
    sub = scans[:4]
    for rep in range(50):
        o, _ = g.voxelGridFilterClouds(sub, 0.5)
        r, _ = g.voxelGridFilterClouds(o, 0.5)
        del o, r
        if rep == 1:
            f2 = free_bytes()
    f50 = free_bytes()
    assert abs(f50 - f2) < (32 << 20), (f2, f50)


def test_the_composite_path_ran(mods):
    ndt, po, clouds = mods
    scans = node_scans(clouds, 128)
    g = ndt.NormalDistributionsTransform()
    diag = {}
    for n in (8, 40, 128):
        outs, _ = g.voxelGridFilterClouds(scans[:n], 0.5)
        diag[n] = g.filterBatchDiag()
        raw = [g.uploadCloud(s) for s in scans[:n]]
        res, _ = g.voxelGridFilterClouds(raw, 0.5)
        diag[(n, "clouds")] = g.filterBatchDiag()
        if n == 40:
            for k in (0, 17, 39):
                ref = g.voxelGridFilterCloud(scans[k], 0.5)[0].numpy()
                assert np.array_equal(outs[k].numpy(), ref) and np.array_equal(res[k].numpy(), ref)
    for key, d in diag.items():
        assert d["single_route"] == 0, (key, d)
    assert diag[8]["passes"] == 1 and diag[40]["passes"] == 1, diag
    assert diag[8]["launches"] == diag[40]["launches"], diag
    assert diag[(8, "clouds")]["launches"] == diag[(40, "clouds")]["launches"], diag
    assert diag[8]["launches"] <= 16 and diag[(8, "clouds")]["launches"] <= 16, diag
    # 128 node scans hold more counters than one pass takes: the launches grow with the passes alone (12 each)
    for key, small in ((128, 8), ((128, "clouds"), (8, "clouds"))):
        assert diag[key]["launches"] == diag[small]["launches"] + 12 * (diag[key]["passes"] - 1), (key, diag)


def test_pair_sequence_batch_filter_prints_the_plain_run(mods, tmp_path):
    ndt, po, clouds = mods
    scans, d = sequence(clouds, ndt, tmp_path)
    ndt.pcd_write_xyz(str(d / "cloud_50.pcd"), np.full((5, 3), np.nan, np.float32))  # filters to nothing: dropped by both
    exe = build_app(tmp_path, "pair_sequence")
    keep = lambda out: [ln for ln in out.splitlines() if not ln.startswith("time:")]  # noqa: E731
    for extra in ([], ["--fitness"]):
        plain = subprocess.run([exe, str(d)] + extra, capture_output=True, text=True, timeout=300)
        batch = subprocess.run([exe, str(d), "--batch-filter"] + extra, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0 and batch.returncode == 0, (plain.stderr, batch.stderr)
        assert keep(batch.stdout) == keep(plain.stdout)
        assert sum(ln.startswith("Loaded") for ln in plain.stdout.splitlines()) == len(scans)
        assert any(ln.startswith("time: read + prefilter") for ln in batch.stdout.splitlines())
