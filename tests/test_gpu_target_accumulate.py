"""GPU: ndt_target_accumulate* -- posed scans merged into the voxel grid.  After any sequence of accumulate calls the
handle must behave like a handle whose target was set from the concatenation of the posed scans.  Every case is compared
against two references built from that concatenation (posed with the oracle's transform_cloud):
 (a) the live oracle: indices, counts, means and covariances bit for bit; icov and evals within test_gpu_parity's bounds;
 (b) a second GPU handle: every dumped field bit for bit, and eval (score, gradient, Hessian, neighbour count) at three
     poses for the four search methods, hessian_f64 and calculateScore bit for bit."""
import subprocess

import numpy as np
import pytest

from conftest import rot_err, trans_err
from test_gpu_map_batch import moved, moved_keeping_non_finite
from test_gpu_pairs import build_app, matrices, sequence
from test_gpu_parity import _DeviceCopies

pytestmark = pytest.mark.gpu

FIELDS = ("idx", "n", "mean", "cov", "icov", "evals", "min_b", "max_b", "div_b")
POSES = ([0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.05, -0.03, 0.01, 0.002, -0.001, 0.004], [-0.2, 0.1, 0.0, 0.0, 0.0, -0.01])
ROT_TOL, TRANS_TOL = 1e-4, 1e-3  # README, parity status


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from oracle import pyoracle as po
    from toyslam_amd import _lib, clouds, ndt
    return ndt, po, clouds, _lib


def methods(ndt):
    return (ndt.KDTREE, ndt.DIRECT26, ndt.DIRECT7, ndt.DIRECT1)


def handle(ndt, res=1.0, min_pts=6, voxel_index=0):
    g = ndt.NormalDistributionsTransform()
    g.setResolution(res)
    g.setMinPointPerVoxel(min_pts)
    g.setVoxelIndex(voxel_index)
    return g


def observe(ndt, g, src):
    """everything the references are compared on: the dump and, with a source and a voxel, the evaluations"""
    out = dict(grid=g.grid())
    if src is None or len(out["grid"]["idx"]) == 0:
        return out
    g.setInputSource(src)
    for m in methods(ndt):
        g.setNeighborhoodSearchMethod(m)
        out["eval", m] = [g.eval(p, True) for p in POSES]
        out["h64", m] = g.hessian_f64(POSES[1])
        out["score", m] = g.calculateScore(src)
    g.setNeighborhoodSearchMethod(ndt.DIRECT7)
    return out


def same_observation(ndt, a, b):
    for k in FIELDS:
        assert np.array_equal(a["grid"][k], b["grid"][k]), k
    assert a["grid"]["n_valid"] == b["grid"]["n_valid"]
    assert set(a) == set(b)
    for m in methods(ndt):
        if ("eval", m) not in a:
            continue
        for ea, eb in zip(a["eval", m], b["eval", m]):
            assert ea[0] == eb[0] and np.array_equal(ea[1], eb[1]) and np.array_equal(ea[2], eb[2]) and ea[3] == eb[3], m
        assert np.array_equal(a["h64", m], b["h64", m]), m
        assert a["score", m] == b["score", m], m


class Ref:
    """the two references of one concatenation, computed once"""

    def __init__(self, mods, cat, src=None, is_dense=True, res=1.0, min_pts=6, voxel_index=0):
        ndt, po, _, _ = mods
        self.ndt = ndt
        cat = np.ascontiguousarray(cat, dtype=np.float32)
        b = handle(ndt, res, min_pts, voxel_index)
        b.setInputTarget(cat, is_dense=is_dense)
        self.src = src
        self.second = observe(ndt, b, src)
        o = po.OracleNDT(resolution=res, min_points_per_voxel=min_pts)
        o.set_target(cat, is_dense=is_dense)
        self.oracle = o.grid()
        self.min_pts = min_pts

    def check(self, g, got=None):
        got = got if got is not None else observe(self.ndt, g, self.src)
        same_observation(self.ndt, got, self.second)                      # (b)
        gg, og = got["grid"], self.oracle                                 # (a)
        assert np.array_equal(gg["idx"], og["idx"]) and np.array_equal(gg["n"], og["n"])
        assert gg["n_valid"] == int((og["n"] >= self.min_pts).sum())
        if len(og["idx"]) == 0:
            return got
        for k in ("min_b", "max_b", "div_b"):
            assert np.array_equal(gg[k], og[k]), k
        assert np.array_equal(gg["mean"], og["mean"])
        inflated = (og["n"] >= self.min_pts) & (og["evals"][:, 0] < 0.01 * og["evals"][:, 2])
        print("oracle: %d voxels, %d inflated, max |cov - oracle| all %.3g, not inflated %.3g" %
              (len(og["idx"]), int(inflated.sum()), np.abs(gg["cov"] - og["cov"]).max(), np.abs(gg["cov"] - og["cov"])[~inflated].max(initial=0.0)))
        assert np.array_equal(gg["cov"], og["cov"])
        scale = np.abs(og["icov"]).max(axis=(1, 2), keepdims=True) + 1e-300
        assert (np.abs(gg["icov"] - og["icov"]) / scale).max() < 1e-10
        assert np.allclose(gg["evals"], og["evals"], rtol=1e-10, atol=1e-14)
        return got


def scene(clouds, n_scans, n_pts, seed, extent=24.0):
    """n_scans views of one world with their poses (scan k moved by poses[k] is back in the world), and a source"""
    rng = np.random.default_rng(seed)
    world = clouds.target_surfaces(6 * n_pts, seed=seed, extent=extent)[:, :3].astype(np.float32)
    pose, scans, poses = np.eye(4), [], []
    for k in range(n_scans):
        if k:
            pose = pose @ clouds.random_T(rng, 0.6, 2.0)
        pick = world[rng.choice(len(world), n_pts + 137 * k, replace=False)]
        scans.append(clouds.apply_T(np.linalg.inv(pose), pick).astype(np.float32))
        poses.append(pose.astype(np.float32))
    src = clouds.apply_T(np.linalg.inv(clouds.random_T(rng, 0.2, 0.5)), world[::11].copy()).astype(np.float32)
    return scans, poses, src


# ---- 1: four posed scans, one at a time in every form and all four in one call
def test_every_form_gives_the_concatenations_grid(mods):
    ndt, po, clouds, _ = mods
    scans, poses, src = scene(clouds, 4, 3000, seed=41)
    posed = [moved(po, s, T) for s, T in zip(scans, poses)]
    gh, gd, gc, gall = (handle(ndt) for _ in range(4))
    with _DeviceCopies() as dc:
        for k in range(4):
            ref = Ref(mods, np.concatenate(posed[:k + 1]), src)
            assert gh.targetAccumulate(scans[k], poses[k])["updates"] == k + 1
            rec = np.ascontiguousarray(np.c_[scans[k], np.ones(len(scans[k]), np.float32)], dtype=np.float32)
            gd.targetAccumulateDevice(dc.put(rec), len(rec), 16, poses[k])
            up = gc.uploadCloud(scans[k])
            st = gc.targetAccumulateCloud(up, poses[k])
            up.release()
            assert st["points"] == sum(len(s) for s in scans[:k + 1]) and st["voxels"] == len(ref.oracle["idx"])
            first = ref.check(gh)
            for g in (gd, gc):
                same_observation(ndt, observe(ndt, g, src), first)
    ups = [gall.uploadCloud(s) for s in scans]
    st = gall.targetAccumulateClouds(ups, poses)
    assert st["updates"] == 1 and st["points"] == sum(len(s) for s in scans)
    assert gall.targetAccumulateDiag()["touched_voxels"] == st["voxels"] == gall.targetAccumulateDiag()["new_voxels"]
    same_observation(ndt, observe(ndt, gall, src), first)


# ---- 2: voxels that cross min_points_per_voxel across updates
def in_cell(rng, cell, n, spread=0.8):
    return (np.asarray(cell, np.float32) + 0.1 + spread * rng.random((n, 3))).astype(np.float32)


def test_voxels_cross_min_points_across_updates(mods):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(7)
    # everything 500 km out: there the covariance formula of a voxel of 3000 collinear points cancels into a negative
    # eigenvalue (the oracle's nr_points = -1), and 3000 scattered points more make the voxel valid
    ox, oy = 500000, -500000
    a, b, c = (ox, oy + 1, 0), (ox + 2, oy + 1, 0), (ox + 4, oy + 1, 0)   # 3 + 3, 5 + 1, 2 + 2 + 2 points with min 6
    under = (ox + 1, oy + 3, 0)                   # stays under min_pts between valid neighbours that are probed
    around = np.concatenate([in_cell(rng, (ox + i, oy + j, 0), 30) for i, j in ((0, 3), (2, 3), (1, 2), (1, 4))])
    line_at = np.array([ox + 0.5, oy + 0.5, 0.5], np.float32)
    line = (line_at + np.c_[np.linspace(-0.3, 0.3, 3000), np.zeros(3000), np.zeros(3000)]).astype(np.float32)
    u = [np.concatenate([in_cell(rng, a, 3), in_cell(rng, b, 5), in_cell(rng, c, 2), in_cell(rng, under, 4), around, line]),
         np.concatenate([in_cell(rng, a, 3), in_cell(rng, b, 1), in_cell(rng, c, 2)]),
         np.concatenate([in_cell(rng, c, 2), (line_at + rng.uniform(-0.4, 0.4, (3000, 3))).astype(np.float32)])]
    src = np.concatenate([in_cell(rng, (ox + i, oy + j, 0), 25, 0.7) for i in range(5) for j in range(5)])
    g = handle(ndt)
    seen = []
    for k in range(3):
        g.targetAccumulate(u[k])
        got = Ref(mods, np.concatenate(u[:k + 1]), src).check(g)
        seen.append(dict(zip(got["grid"]["idx"].tolist(), got["grid"]["n"].tolist())))
    first = sorted(seen[0])[0]                   # the collinear voxel has the lowest y: the lowest linear index
    assert seen[0][first] == -1 and seen[2][first] == 6000, "the collinear voxel: rejected at first, valid later"
    assert sorted(v for v in seen[0].values() if 0 < v < 6) == [2, 3, 4, 5] and sorted(v for v in seen[2].values() if 0 < v < 6) == [4]


# ---- 3: runs of every length into one voxel, fresh and as a continuation
@pytest.mark.parametrize("run,offset", [(1, 0.0), (31, 0.0), (32, 0.0), (33, 0.0), (64, 0.0), (65, 0.0), (1000, 0.0), (5000, 0.0), (1000, 1e5)])
def test_runs_into_one_voxel(mods, run, offset):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(100 + run)
    off = np.array([offset, -offset, 0.0], np.float32)
    bg = (rng.random((2000, 3)) * [10, 10, 1]).astype(np.float32)
    bg = bg[~((bg[:, 0] >= 3) & (bg[:, 0] < 4) & (bg[:, 1] >= 3) & (bg[:, 1] < 4))]
    def crowd(n):
        return (rng.random((n, 3)) * [0.9, 0.9, 0.9] + [3.05, 3.05, 0.05]).astype(np.float32)
    u = [np.concatenate([bg[:1000], crowd(run), bg[1000:]]) + off, np.concatenate([crowd(run), bg[::9]]) + off]
    src = (rng.random((400, 3)) * [10, 10, 1]).astype(np.float32) + off
    g = handle(ndt)
    g.targetAccumulate(u[0])
    Ref(mods, u[0], src).check(g)
    g.targetAccumulate(u[1])
    got = Ref(mods, np.concatenate(u), src).check(g)
    assert got["grid"]["n"].max() >= 2 * run


# ---- 4: box growth
def slab(rng, lo, hi, n):
    return (np.asarray(lo, np.float32) + rng.random((n, 3)) * (np.asarray(hi, np.float32) - np.asarray(lo, np.float32))).astype(np.float32)


@pytest.mark.parametrize("axis,sign", [(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)])
@pytest.mark.parametrize("voxel_index", [0, 1, 2])
def test_box_growth_in_every_direction(mods, axis, sign, voxel_index):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(10 * axis + sign + 50)
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([10.0, 10.0, 3.0])
    base = slab(rng, lo, hi, 2500)
    glo, ghi = lo.copy(), hi.copy()
    if sign > 0:
        glo[axis], ghi[axis] = hi[axis], hi[axis] + 3.5
    else:
        glo[axis], ghi[axis] = lo[axis] - 3.5, lo[axis]   # a lower min_b shifts every linear index
    grow = slab(rng, glo, ghi, 2000)
    inside = slab(rng, lo + 1, hi - 1, 2000)
    src = slab(rng, lo - 1, hi + 1, 500)
    g = handle(ndt, voxel_index=voxel_index)
    g.targetAccumulate(base)
    assert not g.targetAccumulateDiag()["relinked"]       # nothing to relink yet
    before = Ref(mods, base, src, voxel_index=voxel_index).check(g)["grid"]
    g.targetAccumulate(grow)
    assert g.targetAccumulateDiag()["relinked"]
    after = Ref(mods, np.concatenate([base, grow]), src, voxel_index=voxel_index).check(g)["grid"]
    assert not np.array_equal(before["min_b"], after["min_b"]) or not np.array_equal(before["max_b"], after["max_b"])
    if sign < 0:
        assert after["idx"][-1] != before["idx"][-1]
    g.targetAccumulate(inside)
    d = g.targetAccumulateDiag()
    assert not d["relinked"] and not d["table_grown"] and d["touched_voxels"] > 0
    Ref(mods, np.concatenate([base, grow, inside]), src, voxel_index=voxel_index).check(g)


def test_growth_flips_the_automatic_table_form(mods):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(77)
    base = slab(rng, [0, 0, 0], [10, 10, 2], 2500)
    far = slab(rng, [4000, 4000, 0], [4003, 4003, 2], 300)   # 4004 x 4004 x 2 cells for 2800 points: the sparse form
    src = np.concatenate([slab(rng, [0, 0, 0], [10, 10, 2], 300), slab(rng, [4000, 4000, 0], [4003, 4003, 2], 100)])
    g = handle(ndt)
    g.targetAccumulate(base)
    Ref(mods, base, src).check(g)
    g.targetAccumulate(far)
    assert g.targetAccumulateDiag()["relinked"]
    Ref(mods, np.concatenate([base, far]), src).check(g)
    inside = slab(rng, [1, 1, 0.2], [9, 9, 1.8], 1200)       # the box stays: nothing but the touched entries is written
    g.targetAccumulate(inside)
    assert not g.targetAccumulateDiag()["relinked"]
    Ref(mods, np.concatenate([base, far, inside]), src).check(g)


# ---- 5: table and slot growth
@pytest.mark.parametrize("voxel_index", [1, 2])
def test_table_and_slot_growth(mods, monkeypatch, voxel_index):
    ndt, po, clouds, _ = mods
    monkeypatch.setenv("NDT_ACC_HASH_BITS", "4")
    monkeypatch.setenv("NDT_ACC_SLOTS", "8")
    rng = np.random.default_rng(5)
    u = [slab(rng, [8 * k, 0, 0], [8 * k + 8, 12, 1], 2000) for k in range(3)]   # 96 voxels each: 96, 192, 288 slots wanted
    src = slab(rng, [0, 0, 0], [24, 12, 1], 600)
    g = handle(ndt, voxel_index=voxel_index)
    grown = []
    for k in range(3):
        st = g.targetAccumulate(u[k])
        grown.append(g.targetAccumulateDiag()["table_grown"])
        Ref(mods, np.concatenate(u[:k + 1]), src, voxel_index=voxel_index).check(g)
    assert st["voxels"] >= 200 and grown[1] and grown[2]


def test_slots_grow_while_the_key_table_holds(mods, monkeypatch):
    ndt, po, clouds, _ = mods
    monkeypatch.setenv("NDT_ACC_HASH_BITS", "10")   # 1024 keys: at most half full up to 512 voxels
    monkeypatch.setenv("NDT_ACC_SLOTS", "16")
    rng = np.random.default_rng(6)
    u = [slab(rng, [4 * k, 0, 0], [4 * k + 3.99, 4.99, 0.99], 400) for k in range(2)]   # 20 voxels each: 32 slots, then 64
    src = slab(rng, [0, 0, 0], [8, 5, 1], 200)
    g = handle(ndt)
    g.targetAccumulate(u[0])
    assert not g.targetAccumulateDiag()["table_grown"]           # (nothing to copy yet)
    st = g.targetAccumulate(u[1])
    d = g.targetAccumulateDiag()
    assert st["voxels"] == 40 and d["new_voxels"] == 20 and d["table_grown"]
    assert d["launches"] == 1 + 7 + 2 + int(d["relinked"])       # the slot arrays are copied; no rehash launch
    Ref(mods, np.concatenate(u), src).check(g)


# ---- 6: is_dense = 0 with NaN / inf rows
def test_non_finite_rows_and_empty_clouds(mods):
    ndt, po, clouds, _ = mods
    scans, poses, src = scene(clouds, 3, 2500, seed=13)
    bad = [s.copy() for s in scans]
    for s in bad:
        s[::97] = np.nan
        s[5, 1] = np.inf
        s[9, 2] = -np.inf
        s[len(s) - 1, 0] = np.nan
    nan_only = np.full((40, 3), np.nan, np.float32)
    nan_only[3] = [np.inf, 0, 0]
    g = handle(ndt)
    g.targetAccumulate(nan_only, is_dense=False)               # a cloud of only such rows: a target with no voxel
    assert g.targetAccumulated() == dict(points=40, voxels=0, updates=1)
    cat = [nan_only]
    Ref(mods, np.concatenate(cat), None, is_dense=False).check(g)
    g.targetAccumulate(bad[0], poses[0], is_dense=False)       # moved
    cat.append(moved_keeping_non_finite(po, bad[0], poses[0]))
    Ref(mods, np.concatenate(cat), src, is_dense=False).check(g)
    g.targetAccumulate(bad[1], None, is_dense=False)           # unmoved
    cat.append(bad[1])
    Ref(mods, np.concatenate(cat), src, is_dense=False).check(g)
    ups = [g.uploadCloud(bad[2]), g.uploadCloud(np.zeros((0, 3), np.float32)), g.uploadCloud(nan_only), g.uploadCloud(bad[0])]
    g.targetAccumulateClouds(ups, [poses[2], poses[1], poses[1], poses[1]], is_dense=False)   # an empty cloud in the middle
    cat += [moved_keeping_non_finite(po, bad[2], poses[2]), nan_only, moved_keeping_non_finite(po, bad[0], poses[1])]
    ref = Ref(mods, np.concatenate(cat), src, is_dense=False)
    got = ref.check(g)
    assert g.targetAccumulated()["points"] == sum(len(c) for c in cat)
    # pose NULL against the identity matrix, and one call per cloud against the one pass
    g1, g2 = handle(ndt), handle(ndt)
    for h, T in ((g1, None), (g2, np.eye(4))):
        h.targetAccumulate(nan_only, T, is_dense=False)
        h.targetAccumulate(bad[0], poses[0], is_dense=False)
        h.targetAccumulate(bad[1], T, is_dense=False)
        for s, P in ((bad[2], poses[2]), (nan_only, poses[1]), (bad[0], poses[1])):
            h.targetAccumulate(s, P, is_dense=False)
        same_observation(ndt, observe(ndt, h, src), got)


# ---- 7: life cycle
def test_life_cycle(mods):
    ndt, po, clouds, _lib = mods
    scans, poses, src = scene(clouds, 4, 2500, seed=23)
    posed = [moved(po, s, T) for s, T in zip(scans, poses)]
    g = handle(ndt)
    g.setInputTarget(scans[3])                                  # a cloud target is replaced, not continued
    g.targetAccumulate(scans[0], poses[0])
    Ref(mods, posed[0], src).check(g)
    g.warmUp(3000)                                              # in the middle: changes nothing
    g.targetAccumulate(scans[1], poses[1])
    ref01 = Ref(mods, np.concatenate(posed[:2]), src)
    before = ref01.check(g)
    # refusals: documented codes, the target stays as it was
    g.setInputSource(src)
    g.align()
    for call, status in ((lambda: g.getFitnessScore(), _lib.NDT_ERR_NO_INPUT), (lambda: g.copy(), _lib.NDT_ERR_INVALID),
                         (lambda: handle(ndt).shareInputTarget(g), _lib.NDT_ERR_INVALID),
                         (lambda: g.targetAccumulate(np.r_[scans[2], [[1.2e6, 0, 0]]].astype(np.float32), poses[2]), _lib.NDT_ERR_INVALID),
                         (lambda: g.targetAccumulate(scans[2] + np.float32(5000.0)), _lib.NDT_ERR_GRID_OVERFLOW)):
        with pytest.raises(_lib.NdtError) as e:
            call()
        assert e.value.status == status, str(e.value)
        same_observation(ndt, observe(ndt, g, src), before)
    assert g.targetAccumulated() == dict(points=len(scans[0]) + len(scans[1]), voxels=len(before["grid"]["idx"]), updates=2)
    # a min-points change applies only after a reset
    g.setMinPointPerVoxel(3)
    g.targetAccumulate(scans[2], poses[2])
    Ref(mods, np.concatenate(posed[:3]), src, min_pts=6).check(g)
    g.targetAccumulateReset()
    assert g.targetAccumulated() == dict(points=0, voxels=0, updates=0)
    with pytest.raises(_lib.NdtError) as e:
        g.grid()
    assert e.value.status == _lib.NDT_ERR_NO_INPUT               # no target after a reset
    g.targetAccumulate(scans[2], poses[2])
    Ref(mods, posed[2], src, min_pts=3).check(g)
    # setInputTarget replaces the accumulated target; the next accumulate starts empty
    g.setMinPointPerVoxel(6)
    g.setInputTarget(posed[1])
    assert g.targetAccumulated() == dict(points=0, voxels=0, updates=0)
    g.targetAccumulate(scans[3], poses[3])
    Ref(mods, posed[3], src).check(g)
    # a resolution change drops the target
    g.setResolution(2.0)
    assert g.targetAccumulated() == dict(points=0, voxels=0, updates=0)
    with pytest.raises(_lib.NdtError) as e:
        g.grid()
    assert e.value.status == _lib.NDT_ERR_NO_INPUT
    g.targetAccumulate(scans[0], poses[0])
    Ref(mods, posed[0], src, res=2.0).check(g)
    # the first accumulate of a handle refused: the cloud target it held stays
    g2 = handle(ndt)
    g2.setInputTarget(posed[0])
    kept = observe(ndt, g2, src)
    with pytest.raises(_lib.NdtError):
        g2.targetAccumulate(np.array([[2e6, 0, 0]], np.float32))
    same_observation(ndt, observe(ndt, g2, src), kept)


# ---- 8: scan to map
def test_scan_to_map_follows_the_oracle_and_the_app(mods, tmp_path):
    ndt, po, clouds, _ = mods
    scans, d = sequence(clouds, ndt, tmp_path, n=6)
    filt = [po.voxel_grid_filter(sc, 0.5)[0] for sc in scans]
    g = handle(ndt)
    g.setStepSize(0.1)
    g.setTransformationEpsilon(0.01)
    g.setMaximumIterations(64)
    g.setNeighborhoodSearchMethod(ndt.DIRECT7)
    pose = np.eye(4, dtype=np.float32)
    g.targetAccumulate(filt[0], pose)
    placed, result = [filt[0]], []
    for k in range(1, 6):
        g.setInputSource(filt[k])
        g.align(pose)
        T, it = g.getFinalTransformation(), g.getFinalNumIteration()
        assert g.hasConverged()
        o = po.OracleNDT(resolution=1.0, step_size=0.1, trans_eps=0.01, max_iter=64, num_threads=8)
        o.set_target(np.concatenate(placed))
        o.set_source(filt[k])
        r = o.align(pose)
        print("scan %d: iterations gpu %d oracle %d, rot %.3g trans %.3g" % (k, it, r["iterations"], rot_err(T, r["T"]), trans_err(T, r["T"])))
        assert r["converged"] and it == r["iterations"], k
        assert rot_err(T, r["T"]) < ROT_TOL and trans_err(T, r["T"]) < TRANS_TOL, k
        pose = T.astype(np.float32)
        g.targetAccumulate(filt[k], pose)
        placed.append(moved(po, filt[k], pose))
        result.append(T)
    exe = build_app(tmp_path, "map_sequence")
    out = subprocess.check_output([exe, "--scan-to-map", str(d)], text=True)
    step, traj = matrices(out, "Transform "), matrices(out, "trajectory[")
    assert len(step) == 5 and len(traj) == 5 and "registrations 5 (not converged 0)" in out
    for k in range(5):
        assert rot_err(step[k], result[k]) < 1e-5 and trans_err(step[k], result[k]) < 1e-5, k
        assert np.array_equal(step[k], traj[k])               # a result IS the pose in the map: nothing is chained
    # without the switch: the node's scan-to-scan loop, as the parent prints it (test_gpu_pairs pins that loop to the oracle)
    plain = subprocess.check_output([exe, str(d)], text=True)
    plain_late = subprocess.check_output([exe, str(d), "0.5", "-", "node"], text=True)
    s0, s1 = matrices(plain, "Transform "), matrices(plain_late, "Transform ")
    assert len(s0) == 5 and all(np.array_equal(a, b) for a, b in zip(s0, s1))
    t0 = matrices(plain, "trajectory[")
    glob = None
    for k in range(5):
        glob = s0[k] if glob is None else ndt.host_chain_pose(glob, s0[k])
        assert rot_err(t0[k], glob) < 1e-5 and trans_err(t0[k], glob) < 1e-5
    assert not np.allclose(s0[2], step[2], atol=1e-3)           # (scan-to-scan steps are relative, scan-to-map poses absolute)
