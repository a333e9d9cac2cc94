"""GPU: ndt_target_accumulate_crop -- the accumulated target cropped to a box of cells.  After a crop, and after any later
accumulate calls and further crops, the handle must behave like a handle whose target was set from the concatenation, in the
original order, of every posed point accumulated so far whose cell lies inside every crop range applied after it was
accumulated.  Every case compares the cropped handle with test_gpu_target_accumulate's Ref of that filtered concatenation
(a second GPU handle bit for bit, and the live oracle); the cells come from numpy f32 floor(p * inv_leaf), never from the
library."""
import subprocess

import numpy as np
import pytest

from test_gpu_map_batch import moved
from test_gpu_pairs import build_app, matrices, sequence
from test_gpu_target_accumulate import Ref, handle, observe, same_observation, scene

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from oracle import pyoracle as po
    from toyslam_amd import _lib, clouds, ndt
    return ndt, po, clouds, _lib


def cells_of(p, res):
    return np.floor(np.asarray(p, np.float32)[:, :3] * (np.float32(1.0) / np.float32(res))).astype(np.int64)


class History:
    """the filtered concatenation: what was accumulated, in order, minus what the crops removed"""

    def __init__(self, ndt, res=1.0):
        self.ndt, self.res, self.parts = ndt, res, []

    def add(self, posed):
        self.parts.append(np.asarray(posed, np.float32)[:, :3])

    def crop(self, mn, mx):
        lo, hi = self.ndt.crop_cell_range(self.res, mn, mx)
        kept = []
        for p in self.parts:
            c = cells_of(p, self.res)
            kept.append(p[((c >= lo) & (c <= hi)).all(axis=1)])
        self.parts = kept
        return lo, hi

    def cat(self):
        return np.concatenate(self.parts) if self.parts else np.zeros((0, 3), np.float32)

    def voxels(self):
        return len(np.unique(cells_of(self.cat(), self.res), axis=0))


def crop_both(g, hist, mn, mx):
    before = g.targetAccumulated()
    n_before = hist.voxels()
    mn, mx = np.asarray(mn, np.float32), np.asarray(mx, np.float32)
    hist.crop(mn, mx)
    st = g.targetAccumulateCrop(mn, mx)
    d = g.targetCropDiag()
    assert st == dict(points=len(hist.cat()), voxels=hist.voxels(), updates=before["updates"])
    assert d["kept_voxels"] == hist.voxels() and d["removed_voxels"] == n_before - hist.voxels() and d["kept_points"] == len(hist.cat())
    assert d["relinked"] == (0 < hist.voxels() < n_before)
    assert d["launches"] == (5 if d["relinked"] else 2 if n_before else 0)
    return d


NAN_ONLY = np.full((8, 3), np.nan, np.float32)


def check_empty(mods, g):
    assert g.targetAccumulated()["voxels"] == 0 and g.targetAccumulated()["points"] == 0
    Ref(mods, NAN_ONLY, None, is_dense=False).check(g)


def slab(rng, lo, hi, n):
    return (np.asarray(lo, np.float32) + rng.random((n, 3)) * (np.asarray(hi, np.float32) - np.asarray(lo, np.float32))).astype(np.float32)


# ---- 1: a box through the scene; dump, evaluations, registration; the three table forms
@pytest.mark.parametrize("voxel_index", [0, 1, 2])
def test_basic_crop(mods, voxel_index):
    ndt, po, clouds, _ = mods
    scans, poses, src = scene(clouds, 4, 2500, seed=41)
    g = handle(ndt, voxel_index=voxel_index)
    hist = History(ndt)
    for s, T in zip(scans, poses):
        g.targetAccumulate(s, T)
        hist.add(moved(po, s, T))
    cat = hist.cat()
    mn, mx = np.quantile(cat, 0.2, axis=0).astype(np.float32), np.quantile(cat, 0.85, axis=0).astype(np.float32)
    d = crop_both(g, hist, mn, mx)
    assert d["removed_voxels"] > 100 and d["kept_voxels"] > 100
    ref = Ref(mods, hist.cat(), src, voxel_index=voxel_index)
    got = ref.check(g)
    if voxel_index == 0:
        g.warmUp(3000)                                           # leaves a cropped target as it was
        same_observation(ndt, observe(ndt, g, src), got)
    b = handle(ndt, voxel_index=voxel_index)
    b.setInputTarget(hist.cat())
    guess = clouds.make_T([0.15, -0.1, 0.02], [0.0, 0.0, 0.01]).astype(np.float32)
    results = []
    for h in (g, b):
        h.setInputSource(src)
        h.align(guess)
        results.append((h.getFinalTransformation(), h.getFinalNumIteration(), h.stats()["n_evals"], h.hasConverged()))
    assert np.array_equal(results[0][0], results[1][0]) and results[0][1:] == results[1][1:]
    poses_tab = [np.eye(4, dtype=np.float32), guess, results[0][0]]
    assert np.array_equal(g.scorePoses(poses_tab), b.scorePoses(poses_tab))


# ---- 2: the box contains the target
def test_keep_everything(mods):
    ndt, po, clouds, _ = mods
    scans, poses, src = scene(clouds, 3, 2500, seed=5)
    g = handle(ndt)
    hist = History(ndt)
    for s, T in zip(scans, poses):
        g.targetAccumulate(s, T)
        hist.add(moved(po, s, T))
    before = observe(ndt, g, src)
    stats = g.targetAccumulated()
    cat = hist.cat()
    for mn, mx in (([-INF] * 3, [INF] * 3), (cat.min(axis=0), cat.max(axis=0)), (cat.min(axis=0) - 50, [INF, 1e4, 3e38])):
        d = crop_both(g, hist, mn, mx)
        assert d["removed_voxels"] == 0 and not d["relinked"] and d["launches"] == 2
        assert g.targetAccumulated() == stats
        same_observation(ndt, observe(ndt, g, src), before)
    Ref(mods, cat, src).check(g, before)


# ---- 3: everything removed, then a scan; exactly one voxel
def test_remove_everything_and_a_single_voxel(mods):
    ndt, po, clouds, _ = mods
    scans, poses, src = scene(clouds, 3, 2500, seed=9)
    posed = [moved(po, s, T) for s, T in zip(scans, poses)]
    g = handle(ndt)
    hist = History(ndt)
    for k in range(2):
        g.targetAccumulate(scans[k], poses[k])
        hist.add(posed[k])
    d = crop_both(g, hist, [1000, 1000, 1000], [1001, 1001, 1001])
    assert d["kept_voxels"] == 0 and not d["relinked"]
    check_empty(mods, g)
    crop_both(g, hist, [-INF] * 3, [INF] * 3)                     # a crop of the empty target
    check_empty(mods, g)
    assert g.targetAccumulate(scans[2], poses[2])["updates"] == 3   # the box starts afresh
    hist.add(posed[2])
    Ref(mods, posed[2], src).check(g)
    g.targetAccumulate(scans[0], poses[0])
    hist.add(posed[0])
    # lo == hi: the fullest cell alone
    cells, counts = np.unique(cells_of(hist.cat(), 1.0), axis=0, return_counts=True)
    c = cells[np.argmax(counts)].astype(np.float32)
    d = crop_both(g, hist, c + 0.25, c + 0.75)
    assert d["kept_voxels"] == 1 and d["kept_points"] == counts.max() >= 6
    got = Ref(mods, hist.cat(), src).check(g)
    assert np.array_equal(got["grid"]["min_b"], got["grid"]["max_b"])
    g.targetAccumulate(scans[1], poses[1])
    hist.add(posed[1])
    Ref(mods, hist.cat(), src).check(g)


# ---- 4: removed cells receive points again and start from empty sums
@pytest.mark.parametrize("voxel_index", [0, 2])
def test_removed_cells_come_back(mods, voxel_index):
    ndt, po, clouds, _ = mods
    scans, poses, src = scene(clouds, 3, 2500, seed=17)
    posed = [moved(po, s, T) for s, T in zip(scans, poses)]
    g = handle(ndt, voxel_index=voxel_index)
    hist = History(ndt)
    for k in range(2):
        g.targetAccumulate(scans[k], poses[k])
        hist.add(posed[k])
    mid = np.median(hist.cat(), axis=0)
    crop_both(g, hist, [-INF, -INF, -INF], [mid[0] - 4, INF, INF])   # a quarter or so stays
    Ref(mods, hist.cat(), src, voxel_index=voxel_index).check(g)
    removed = cells_of(posed[2], 1.0)[:, 0] > np.floor(mid[0] - 4)
    assert removed.mean() > 0.5                                   # the scan falls mostly into removed cells
    g.targetAccumulate(scans[2], poses[2])
    hist.add(posed[2])
    assert g.targetAccumulateDiag()["new_voxels"] > 100
    Ref(mods, hist.cat(), src, voxel_index=voxel_index).check(g)
    crop_both(g, hist, [-INF, mid[1] - 3, -INF], [INF, INF, INF])    # another box
    Ref(mods, hist.cat(), src, voxel_index=voxel_index).check(g)


# ---- 5: points and bounds on a cell face and one ulp either side, 100 km from the origin; open sides
@pytest.mark.parametrize("res", [1.0, 0.3])
def test_box_faces(mods, res):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(31)
    off = np.array([1e5, -1e5, 0.0], np.float32)
    leaf = np.float32(res)
    c0 = cells_of(off[None] + np.float32(3.0), res)[0]            # a cell inside the scene
    near = np.float32(c0[0]) * leaf                                # about its lower x face; the face of the f32 binning is
    cand = [near]                                                  # the first float whose cell is c0: within a few ulps of it
    for _ in range(16):
        cand = [np.nextafter(cand[0], -INF)] + cand + [np.nextafter(cand[-1], INF)]
    cand = np.array(cand, np.float32)
    cx = cells_of(np.c_[cand, cand, cand], res)[:, 0]
    assert cx[0] == c0[0] - 1 and cx[-1] == c0[0]
    face = cand[np.argmax(cx == c0[0])]
    ulps = [np.nextafter(face, -INF), face, np.nextafter(face, INF)]
    bg = slab(rng, [0, 0, 0], [8, 8, 2], 2200) + off
    on_face = np.concatenate([np.c_[np.full(40, x, np.float32), slab(rng, [0, 0, 0], [8, 8, 2], 40)[:, 1:] + off[1:]] for x in ulps]).astype(np.float32)
    cloud = np.concatenate([bg[:1100], on_face, bg[1100:]]).astype(np.float32)
    src = slab(rng, [0, 0, 0], [8, 8, 2], 400) + off
    assert len({tuple(c) for c in cells_of(on_face, res)[:, :1]}) == 2   # the face points fall on both sides
    for axis_bound in ulps:
        for side in ("min", "max"):
            g = handle(ndt, res=res)
            hist = History(ndt, res)
            g.targetAccumulate(cloud)
            hist.add(cloud)
            mn, mx = np.array([-INF, -INF, -INF]), np.array([INF, INF, INF])
            (mn if side == "min" else mx)[0] = axis_bound
            d = crop_both(g, hist, mn, mx)
            assert d["removed_voxels"] > 0 and d["kept_voxels"] > 0
            Ref(mods, hist.cat(), src, res=res).check(g)
    # a closed box whose corners sit on faces, y and z too
    g = handle(ndt, res=res)
    hist = History(ndt, res)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    lo_face = (c0.astype(np.float32) - np.float32([1, 1, 0])) * leaf
    hi_face = (c0.astype(np.float32) + np.float32([2, 3, 1])) * leaf
    crop_both(g, hist, lo_face, hi_face)
    Ref(mods, hist.cat(), src, res=res).check(g)


# ---- 6: kept slot counts around the block and wave sizes; capacities that shrink and grow again
def lattice_cloud(rng, n_cells):
    """cell (i, 0, 0) holds 7 scattered points if i % 3 == 0, else one"""
    rows = []
    for i in range(n_cells):
        m = 7 if i % 3 == 0 else 1
        rows.append(np.c_[i + 0.1 + 0.8 * rng.random(m), 0.1 + 0.8 * rng.random(m), 0.1 + 0.8 * rng.random(m)])
    return np.concatenate(rows).astype(np.float32)


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("kept", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_plan_boundaries(mods, monkeypatch, kept, small):
    ndt, po, clouds, _ = mods
    if small:
        monkeypatch.setenv("NDT_ACC_SLOTS", "16")
        monkeypatch.setenv("NDT_ACC_HASH_BITS", "2")
    rng = np.random.default_rng(kept)
    min_pts = 6   # (the cells of one point stay under it: slots without a record are moved too)
    cloud = lattice_cloud(rng, 2 * kept + 3)
    src = np.c_[rng.random(300) * (2 * kept + 3), rng.random(300), rng.random(300)].astype(np.float32)
    g = handle(ndt, min_pts=min_pts)
    hist = History(ndt)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    d = crop_both(g, hist, [-INF, -INF, -INF], [kept - 0.5, INF, INF])
    assert d["kept_voxels"] == kept and d["removed_voxels"] == kept + 3
    Ref(mods, hist.cat(), src, min_pts=min_pts).check(g)
    g.targetAccumulate(cloud)                                     # the removed cells come back, the kept ones continue
    hist.add(cloud)
    if small:   # the crop shrank the capacities to what the kept slots need: this update has to grow them again
        cap, bits = 16, 2
        while cap < kept:
            cap *= 2
        while 2 * kept > (1 << bits):
            bits += 1
        want = 2 * kept + 3
        assert g.targetAccumulateDiag()["table_grown"] == (want > cap or 2 * want > (1 << bits))
        assert g.targetAccumulateDiag()["table_grown"]
    Ref(mods, hist.cat(), src, min_pts=min_pts).check(g)


def test_key_table_grows_while_the_slots_hold(mods, monkeypatch):
    ndt, po, clouds, _ = mods
    monkeypatch.setenv("NDT_ACC_SLOTS", "16")
    monkeypatch.setenv("NDT_ACC_HASH_BITS", "2")
    rng = np.random.default_rng(11)
    cloud = lattice_cloud(rng, 5)
    src = np.c_[rng.random(100) * 5, rng.random(100), rng.random(100)].astype(np.float32)
    g = handle(ndt)
    hist = History(ndt)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    d = crop_both(g, hist, [-INF, -INF, -INF], [0.5, INF, INF])      # one voxel stays: 16 slots again, but a key table of 4
    assert d["kept_voxels"] == 1
    g.targetAccumulate(cloud)                                       # 5 voxels: the slots hold them, 2 * 5 > 4
    hist.add(cloud)
    d = g.targetAccumulateDiag()
    assert d["table_grown"] and d["launches"] == 1 + 7 + 2 + int(d["relinked"]) + 1   # the rehash launch; no slot copy
    Ref(mods, hist.cat(), src).check(g)


# ---- 7: rejected voxels, voxels under min_pts and valid ones, kept and removed
def test_voxel_states_survive(mods):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(7)
    ox, oy = 500000, -500000     # out here a voxel of 3000 collinear points cancels into a negative eigenvalue: rejected

    def in_cell(cell, n, spread=0.8):
        return (np.asarray(cell, np.float32) + 0.1 + spread * rng.random((n, 3))).astype(np.float32)

    def line(cell):
        at = np.array([cell[0] + 0.5, cell[1] + 0.5, 0.5], np.float32)
        return (at + np.c_[np.linspace(-0.3, 0.3, 3000), np.zeros(3000), np.zeros(3000)]).astype(np.float32)

    parts = []
    for dx in (0, 20):           # the same block twice: the one at dx = 20 is cropped away.  Cells (ox - 2 .., oy - 2 ..)
        bx = ox - 2 + dx
        parts += [in_cell((bx + i, oy - 2 + j, 0), 30) for i in range(4) for j in range(4) if (i, j) not in ((1, 1), (2, 2))]
        parts += [in_cell((bx + 1, oy - 1, 0), 4), line((bx + 2, oy))]
    cloud = np.concatenate(parts)
    src = np.concatenate([in_cell((ox - 2 + dx + i, oy - 2 + j, 0), 20, 0.7) for dx in (0, 20) for i in range(4) for j in range(4)])
    g = handle(ndt)
    hist = History(ndt)
    g.targetAccumulate(cloud)
    hist.add(cloud)
    full = Ref(mods, cloud, src).check(g)["grid"]
    assert (full["n"] == -1).sum() >= 1 and ((full["n"] > 0) & (full["n"] < 6)).sum() == 2 and len(full["n"]) == 32
    crop_both(g, hist, [-INF, -INF, -INF], [ox + 10.0, INF, INF])
    got = Ref(mods, hist.cat(), src).check(g)    # (DIRECT1's neighbour counts are part of the observation)
    n = got["grid"]["n"]
    assert len(n) == 16 and (n == -1).sum() == 1 and ((n > 0) & (n < 6)).sum() == 1
    more = np.concatenate([in_cell((ox - 1, oy - 1, 0), 3), in_cell((ox + 19, oy - 1, 0), 3)])
    g.targetAccumulate(more)                                      # the kept voxel under min_pts continues (4 + 3 points) and
    hist.add(more)                                                # crosses it; its removed twin starts again from nothing
    n = Ref(mods, hist.cat(), src).check(g)["grid"]["n"]
    assert len(n) == 17 and sorted(n[(n > 0) & (n < 6)].tolist()) == [3]


# ---- 8: a window that follows the vehicle
def test_sliding_window(mods):
    ndt, po, clouds, _lib = mods
    rng = np.random.default_rng(88)
    res, half, steps = 0.1, 15.0, 12

    def scan():   # clusters of ten points (voxels of 0.1 m reach min_pts) over 28 x 28 x 3 m around the vehicle
        centres = slab(rng, [-14, -14, -1.5], [14, 14, 1.5], 220)
        return (np.repeat(centres, 10, axis=0) + rng.random((2200, 3)) * 0.03).astype(np.float32)

    g = handle(ndt, res=res)
    hist = History(ndt, res)
    uncropped = []
    counts, ref_counts = [], []
    for k in range(steps):
        T = clouds.make_T([60.0 * k / (steps - 1), 0.3 * k, 0.0], [0.0, 0.0, 0.01 * k]).astype(np.float32)
        s = scan()
        posed = moved(po, s, T)
        g.targetAccumulate(s, T)
        hist.add(posed)
        uncropped.append(posed)
        t = T[:3, 3]
        lo, hi = ndt.crop_cell_range(res, t - np.float32(half), t + np.float32(half))
        crop_both(g, hist, t - np.float32(half), t + np.float32(half))
        src = posed[::7] + np.float32(0.01)
        got = Ref(mods, hist.cat(), src, res=res).check(g)["grid"]
        counts.append(g.targetAccumulated()["voxels"])
        ref_counts.append(len(got["idx"]))
        assert ((got["max_b"] - got["min_b"]) <= (hi - lo) + 1).all()
    early, ref_early = max(counts[:3]), max(ref_counts[:3])
    assert all(c - early <= r - ref_early for c, r in zip(counts, ref_counts))
    assert max(counts) < 0.75 * len(np.unique(cells_of(np.concatenate(uncropped), res), axis=0))
    # the form of the table, by the library's own rule on the CPU: the window stays dense, the union of the run is sparse
    got_b = g.grid()
    win = ndt.host_lattice(res, ndt.crop_cell_centre(res, got_b["min_b"]), ndt.crop_cell_centre(res, got_b["max_b"]), 0, len(hist.cat()))
    assert win["status"] == _lib.NDT_OK and np.array_equal(win["min_b"], got_b["min_b"]) and not win["sparse"]
    union = np.concatenate(uncropped)
    whole = ndt.host_lattice(res, union.min(axis=0), union.max(axis=0), 0, len(union))
    assert whole["status"] == _lib.NDT_OK and whole["sparse"]


# ---- 9: many clouds in one pass after a crop
def test_clouds_after_a_crop(mods):
    ndt, po, clouds, _ = mods
    scans, poses, src = scene(clouds, 4, 2500, seed=29)
    posed = [moved(po, s, T) for s, T in zip(scans, poses)]
    a, b = handle(ndt), handle(ndt)
    hist = History(ndt)
    for k in range(2):
        hist.add(posed[k])
    mid = np.median(hist.cat(), axis=0)
    mn, mx = [mid[0] - 5, mid[1] - 6, -INF], [mid[0] + 6, INF, INF]
    for h in (a, b):
        for k in range(2):
            h.targetAccumulate(scans[k], poses[k])
    crop_both(a, hist, mn, mx)
    b.targetAccumulateCrop(mn, mx)
    ups = [a.uploadCloud(s) for s in scans[2:]]
    a.targetAccumulateClouds(ups, poses[2:])
    for k in (2, 3):
        up = b.uploadCloud(scans[k])
        b.targetAccumulateCloud(up, poses[k])
        up.release()
        hist.add(posed[k])
    got = Ref(mods, hist.cat(), src).check(a)
    same_observation(ndt, observe(ndt, b, src), got)


# ---- 10: the app
def timeless(out):
    return [ln for ln in out.splitlines() if not ln.startswith(("start-up", "time:", "window "))]


def test_map_sequence_window(mods, tmp_path):
    ndt, po, clouds, _ = mods
    scans, d = sequence(clouds, ndt, tmp_path, n=6)
    exe = build_app(tmp_path, "map_sequence")
    out = subprocess.check_output([exe, "--scan-to-map", "--window", "10", str(d)], text=True)
    assert len(matrices(out, "trajectory[")) == 5 and "registrations 5" in out
    line = [ln for ln in out.splitlines() if ln.startswith("window 10 m: the accumulated target reached ")]
    assert len(line) == 1 and 0 < int(line[0].split()[7]) <= 21 ** 3
    plain = subprocess.check_output([exe, "--scan-to-map", str(d)], text=True)
    assert "window" not in plain and len(matrices(plain, "trajectory[")) == 5
    # a window that removes nothing registers as the unchanged option does: the same lines but for the times
    wide = subprocess.check_output([exe, "--scan-to-map", str(d), "--window", "100000"], text=True)
    assert timeless(wide) == timeless(plain)
    assert subprocess.run([exe, "--window", "10", str(d)], capture_output=True).returncode == 2
