"""GPU: ndt_target_accumulate_export / _import / _save / _load -- voxels leave an accumulated target and enter another one bit
for bit.  After any sequence of accumulate, crop and import calls the handle must behave like a handle whose target was set
from one concatenation: every posed point accumulated directly and the points behind every imported voxel.  Every case
compares with test_gpu_target_accumulate's Ref of that concatenation (a second GPU handle bit for bit, and the live oracle)
and, where two targets hold the same points per cell, their exports byte for byte.  Every comparison but the app's is exact."""
import os
import subprocess

import numpy as np
import pytest

from conftest import rot_err, trans_err
from test_gpu_map_batch import moved
from test_gpu_pairs import build_app, matrices, sequence
from test_gpu_target_accumulate import Ref, handle, in_cell, observe, same_observation, scene, slab
from test_gpu_target_crop import History, cells_of, crop_both, lattice_cloud
from test_target_persist_host import make_blob

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
LIM = 1 << 20
EXPORT_LAUNCHES = 3   # mark, sort, gather (include/ndt_mi355.h)
IMPORT_LAUNCHES = 3   # check, place, finish; + 1 when the key table is rebuilt, + 1 when the look-up table is relinked


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from oracle import pyoracle as po
    from toyslam_amd import _lib, clouds, ndt
    return ndt, po, clouds, _lib


def row_cells(rows):
    return np.c_[rows["i"], rows["j"], rows["k"]].astype(np.int64).reshape(-1, 3)


def row_keys(rows):
    c = (row_cells(rows) + LIM).astype(np.uint64)
    return (c[:, 2] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 0]


def check_blob(ndt, blob, cat, res=1.0):
    """a blob against the points behind it: header, canonical order, cells and counts (the sums are checked through Ref)"""
    info, rows = ndt.acc_blob_info(blob), ndt.acc_blob_rows(blob)
    cells, counts = np.unique(cells_of(cat, res), axis=0, return_counts=True)
    assert info["n_voxels"] == len(rows) == len(cells) and len(blob) == 64 + 104 * len(rows)
    keys = row_keys(rows)
    assert (keys[1:] > keys[:-1]).all()
    order = np.lexsort((cells[:, 0], cells[:, 1], cells[:, 2]))       # k high, i low
    assert np.array_equal(row_cells(rows), cells[order]) and np.array_equal(rows["count"], counts[order])
    assert np.array_equal(info["lo"], cells.min(axis=0)) and np.array_equal(info["hi"], cells.max(axis=0))
    assert not rows["pad"].any()


def refused(_lib, call, word):
    with pytest.raises(_lib.NdtError) as e:
        call()
    assert e.value.status == _lib.NDT_ERR_INVALID and word in str(e.value), str(e.value)


# ---- 1: round trip
@pytest.mark.parametrize("voxel_index", [0, 1, 2])
def test_round_trip(mods, voxel_index):
    ndt, po, clouds, _ = mods
    scans, poses, src = scene(clouds, 4, 3000, seed=41)
    cat = np.concatenate([moved(po, s, T) for s, T in zip(scans, poses)])
    a = handle(ndt, voxel_index=voxel_index)
    for s, T in zip(scans, poses):
        a.targetAccumulate(s, T)
    before = observe(ndt, a, src)
    blob = a.targetAccumulateExport()
    assert a.targetExportDiag() == dict(voxels=len(before["grid"]["idx"]), points=len(cat), launches=EXPORT_LAUNCHES)
    check_blob(ndt, blob, cat)
    same_observation(ndt, observe(ndt, a, src), before)            # the target is not changed
    assert a.targetAccumulated()["updates"] == 4
    b = handle(ndt, voxel_index=voxel_index)
    assert b.targetAccumulateImport(blob) == dict(points=len(cat), voxels=len(before["grid"]["idx"]), updates=1)
    d = b.targetAccumulateDiag()
    assert d == dict(touched_voxels=len(before["grid"]["idx"]), new_voxels=len(before["grid"]["idx"]), relinked=False, table_grown=False,
                     launches=IMPORT_LAUNCHES)
    got = Ref(mods, cat, src, voxel_index=voxel_index).check(b)
    same_observation(ndt, got, before)
    assert b.targetAccumulateExport() == blob
    c = handle(ndt, voxel_index=voxel_index)
    ups = [c.uploadCloud(s) for s in scans]
    c.targetAccumulateClouds(ups, poses)
    assert c.targetAccumulateExport() == blob
    same_observation(ndt, observe(ndt, a, src), before)


# ---- 2: continuation
def test_continuation(mods):
    ndt, po, clouds, _ = mods
    scans, poses, src = scene(clouds, 4, 3000, seed=43)
    posed = [moved(po, s, T) for s, T in zip(scans, poses)]
    a, b, direct = handle(ndt), handle(ndt), handle(ndt)
    for k in range(2):
        a.targetAccumulate(scans[k], poses[k])
    b.targetAccumulateImport(a.targetAccumulateExport())
    for k in range(2, 4):
        b.targetAccumulate(scans[k], poses[k])
    for k in range(4):
        direct.targetAccumulate(scans[k], poses[k])
    assert b.targetAccumulated() == dict(points=sum(len(s) for s in scans), voxels=direct.targetAccumulated()["voxels"], updates=3)
    Ref(mods, np.concatenate(posed), src).check(b)
    assert b.targetAccumulateExport() == direct.targetAccumulateExport()


# ---- 3: the parameters are the importer's
def test_parameters_are_the_importers(mods):
    ndt, po, clouds, _ = mods
    scans, poses, src = scene(clouds, 3, 2500, seed=47)
    cat = np.concatenate([moved(po, s, T) for s, T in zip(scans, poses)])
    a, b = handle(ndt, min_pts=6), handle(ndt, min_pts=3)
    for s, T in zip(scans, poses):
        a.targetAccumulate(s, T)
    b.targetAccumulateImport(a.targetAccumulateExport())
    got = Ref(mods, cat, src, min_pts=3).check(b)
    assert got["grid"]["n_valid"] > a.grid()["n_valid"]


# ---- 4: disjoint merge
@pytest.mark.parametrize("voxel_index", [0, 2])
def test_disjoint_merge(mods, voxel_index):
    ndt, po, clouds, _lib = mods
    scans, poses, src = scene(clouds, 4, 3000, seed=53)
    posed = [moved(po, s, T) for s, T in zip(scans, poses)]
    cat = np.concatenate(posed)
    a = handle(ndt, voxel_index=voxel_index)
    for p in posed:
        a.targetAccumulate(p)
    c0 = int(np.median(cells_of(cat, 1.0)[:, 0]))                 # the plane of cells: X is i <= c0, Y is i > c0
    box_x = ([-INF, -INF, -INF], [ndt.crop_cell_centre(1.0, c0), INF, INF])
    box_y = ([ndt.crop_cell_centre(1.0, c0 + 1), -INF, -INF], [INF, INF, INF])
    blob_x, blob_y = a.targetAccumulateExport(*box_x), a.targetAccumulateExport(*box_y)
    in_x = [cells_of(p, 1.0)[:, 0] <= c0 for p in posed]
    check_blob(ndt, blob_x, np.concatenate([p[m] for p, m in zip(posed, in_x)]))
    check_blob(ndt, blob_y, np.concatenate([p[~m] for p, m in zip(posed, in_x)]))
    nothing = a.targetAccumulateExport([1e5, 1e5, 1e5], [1e5 + 1, 1e5 + 1, 1e5 + 1])
    assert len(nothing) == 64 and ndt.acc_blob_info(nothing)["n_voxels"] == 0
    ref = Ref(mods, cat, src, voxel_index=voxel_index)
    b = handle(ndt, voxel_index=voxel_index)
    for p, m in zip(posed, in_x):
        b.targetAccumulate(p[m])
    b.targetAccumulateImport(blob_y)
    got = ref.check(b)
    c = handle(ndt, voxel_index=voxel_index)
    c.targetAccumulateImport(blob_x)
    for p, m in zip(posed, in_x):
        c.targetAccumulate(p[~m])
    before = c.targetAccumulated()
    assert c.targetAccumulateImport(nothing) == before            # a blob of no rows: nothing changes, not even the update count
    same_observation(ndt, observe(ndt, c, src), got)
    whole = a.targetAccumulateExport()
    assert b.targetAccumulateExport() == whole and c.targetAccumulateExport() == whole   # canonical whatever the slot order
    stats = b.targetAccumulated()
    refused(_lib, lambda: b.targetAccumulateImport(blob_x), "cell already in the target")
    assert b.targetAccumulated() == stats
    same_observation(ndt, observe(ndt, b, src), got)


# ---- 5: voxel states cross
def test_voxel_states_cross(mods):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(7)
    ox, oy = 500000, -500000     # out here a voxel of 3000 collinear points cancels into a negative eigenvalue: rejected
    three = (ox, oy + 1, 0)
    around = np.concatenate([in_cell(rng, (ox + i, oy + j, 0), 30) for i, j in ((0, 3), (2, 3), (1, 2), (1, 4))])
    line_at = np.array([ox + 0.5, oy + 0.5, 0.5], np.float32)
    line = (line_at + np.c_[np.linspace(-0.3, 0.3, 3000), np.zeros(3000), np.zeros(3000)]).astype(np.float32)
    u0 = np.concatenate([in_cell(rng, three, 3), around, line])
    u1 = np.concatenate([in_cell(rng, three, 3), (line_at + rng.uniform(-0.4, 0.4, (3000, 3))).astype(np.float32)])
    src = np.concatenate([in_cell(rng, (ox + i, oy + j, 0), 25, 0.7) for i in range(4) for j in range(5)])
    a, b = handle(ndt), handle(ndt)
    a.targetAccumulate(u0)
    ref0 = Ref(mods, u0, src)
    first = ref0.check(a)["grid"]
    blob = a.targetAccumulateExport()
    check_blob(ndt, blob, u0)
    rows = ndt.acc_blob_rows(blob)
    assert sorted(rows["count"].tolist())[0] == 3 and rows["count"].max() == 3000
    b.targetAccumulateImport(blob)
    same_observation(ndt, observe(ndt, b, src), ref0.second)
    b.targetAccumulate(u1)
    after = Ref(mods, np.concatenate([u0, u1]), src).check(b)["grid"]   # (the f32 centroid sums are in the records the evaluations read)
    seen0, seen1 = dict(zip(first["idx"].tolist(), first["n"].tolist())), dict(zip(after["idx"].tolist(), after["n"].tolist()))
    lowest = sorted(seen0)[0]                                      # the collinear voxel has the lowest y: the lowest linear index
    assert seen0[lowest] == -1 and seen1[lowest] == 6000, "the collinear voxel: rejected when it crossed, valid later"
    assert sorted(v for v in seen0.values() if 0 < v < 6) == [3] and not [v for v in seen1.values() if 0 < v < 6]
    direct = handle(ndt)
    direct.targetAccumulate(u0)
    direct.targetAccumulate(u1)
    assert b.targetAccumulateExport() == direct.targetAccumulateExport()


def test_the_ends_of_the_lattice_cross(mods):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(9)

    def cell_points(i, n):   # x on the 1/8 grid: exact floats at 2^20
        return np.c_[i + rng.integers(1, 8, n) / 8.0, 0.1 + 0.8 * rng.random(n), 0.1 + 0.8 * rng.random(n)].astype(np.float32)

    cloud = np.concatenate([cell_points(LIM - 1, 9), cell_points(-LIM, 8), cell_points(0, 7)])
    assert set(cells_of(cloud, 1.0)[:, 0].tolist()) == {LIM - 1, -LIM, 0}
    a, b, c = handle(ndt), handle(ndt), handle(ndt)
    a.targetAccumulate(cloud)
    blob = a.targetAccumulateExport()
    check_blob(ndt, blob, cloud)
    info = ndt.acc_blob_info(blob)
    assert info["lo"][0] == -LIM and info["hi"][0] == LIM - 1
    b.targetAccumulateImport(blob)
    assert b.targetAccumulateExport() == blob
    got = Ref(mods, cloud, cloud[::2]).check(b)
    same_observation(ndt, got, observe(ndt, a, cloud[::2]))
    # one end at a time, by box, on top of the middle cell
    c.targetAccumulate(cloud[17:])
    c.targetAccumulateImport(a.targetAccumulateExport([LIM - 1.5, -INF, -INF], [INF, INF, INF]))
    c.targetAccumulateImport(a.targetAccumulateExport([-INF, -INF, -INF], [-LIM + 0.5, INF, INF]))
    assert c.targetAccumulated() == dict(points=24, voxels=3, updates=3)
    assert c.targetAccumulateExport() == blob
    same_observation(ndt, observe(ndt, c, cloud[::2]), got)


# ---- 6: plan boundaries
@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_plan_boundaries(mods, monkeypatch, rows, small):
    ndt, po, clouds, _ = mods
    if small:
        monkeypatch.setenv("NDT_ACC_SLOTS", "16")
        monkeypatch.setenv("NDT_ACC_HASH_BITS", "2")
    rng = np.random.default_rng(rows)
    cloud = lattice_cloud(rng, rows + 3)
    src = np.c_[rng.random(300) * (rows + 3), rng.random(300), rng.random(300)].astype(np.float32)
    low = cells_of(cloud, 1.0)[:, 0] < rows
    a, b = handle(ndt), handle(ndt)
    a.targetAccumulate(cloud)
    blob = a.targetAccumulateExport([-INF, -INF, -INF], [rows - 0.5, INF, INF])
    assert a.targetExportDiag() == dict(voxels=rows, points=int(low.sum()), launches=EXPORT_LAUNCHES)
    check_blob(ndt, blob, cloud[low])
    b.targetAccumulate(cloud[~low])                                # three voxels first: the import has slots to move and to relink
    st = b.targetAccumulateImport(blob)
    assert st == dict(points=len(cloud), voxels=rows + 3, updates=2)
    # capacities after the first update: 16 slots and a key table of 32 (at most half full with 16) when small
    rehash = small and 2 * (rows + 3) > 32
    grown = small and (rows + 3 > 16 or rehash)
    d = b.targetAccumulateDiag()
    assert d == dict(touched_voxels=rows, new_voxels=rows, relinked=True, table_grown=bool(grown), launches=IMPORT_LAUNCHES + 1 + int(rehash))
    Ref(mods, cloud, src).check(b)
    whole = a.targetAccumulateExport()
    assert a.targetExportDiag()["launches"] == EXPORT_LAUNCHES and b.targetAccumulateExport() == whole


# ---- 7: box and table
@pytest.mark.parametrize("axis,sign", [(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)])
@pytest.mark.parametrize("voxel_index", [0, 1, 2])
def test_import_grows_the_box(mods, axis, sign, voxel_index):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(10 * axis + sign + 50)
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([10.0, 10.0, 3.0])
    base = slab(rng, lo, hi, 2500)
    glo, ghi = lo.copy(), hi.copy()
    mn, mx = np.full(3, -INF, np.float32), np.full(3, INF, np.float32)
    if sign > 0:
        glo[axis], ghi[axis] = hi[axis], hi[axis] + 3.5
        mn[axis] = hi[axis] + 0.5
    else:
        glo[axis], ghi[axis] = lo[axis] - 3.5, lo[axis]
        mx[axis] = lo[axis] - 0.5
    grow = slab(rng, glo, ghi, 2000)
    grow = grow[(cells_of(grow, 1.0)[:, axis] >= hi[axis]) if sign > 0 else (cells_of(grow, 1.0)[:, axis] < lo[axis])]
    src = slab(rng, lo - 1, hi + 1, 500)
    a, b = handle(ndt, voxel_index=voxel_index), handle(ndt, voxel_index=voxel_index)
    a.targetAccumulate(base)
    a.targetAccumulate(grow)
    blob = a.targetAccumulateExport(mn, mx)
    check_blob(ndt, blob, grow)
    b.targetAccumulate(base)
    before = b.grid()
    b.targetAccumulateImport(blob)
    d = b.targetAccumulateDiag()
    assert d["relinked"] and d["launches"] == IMPORT_LAUNCHES + 1 and not d["table_grown"]
    after = Ref(mods, np.concatenate([base, grow]), src, voxel_index=voxel_index).check(b)["grid"]
    assert not np.array_equal(before["min_b"], after["min_b"]) or not np.array_equal(before["max_b"], after["max_b"])
    inside = slab(rng, lo + 1, hi - 1, 1500)
    b.targetAccumulate(inside)                                     # a point update continues on the imported box
    assert not b.targetAccumulateDiag()["relinked"]
    Ref(mods, np.concatenate([base, grow, inside]), src, voxel_index=voxel_index).check(b)


def test_import_flips_the_automatic_table_form(mods):
    ndt, po, clouds, _lib = mods
    rng = np.random.default_rng(77)
    base = slab(rng, [0, 0, 0], [10, 10, 2], 2500)
    far = slab(rng, [4000, 4000, 0], [4003, 4003, 2], 300)   # 4004 x 4004 x 2 cells for 2800 points: the sparse form
    src = np.concatenate([slab(rng, [0, 0, 0], [10, 10, 2], 300), slab(rng, [4000, 4000, 0], [4003, 4003, 2], 100)])
    a, b = handle(ndt), handle(ndt)
    a.targetAccumulate(far)
    b.targetAccumulate(base)
    cat = np.concatenate([base, far])
    assert not ndt.host_lattice(1.0, base.min(axis=0), base.max(axis=0), 0, len(base))["sparse"]
    assert ndt.host_lattice(1.0, cat.min(axis=0), cat.max(axis=0), 0, len(cat))["sparse"]
    b.targetAccumulateImport(a.targetAccumulateExport())
    assert b.targetAccumulateDiag()["relinked"]
    Ref(mods, cat, src).check(b)


@pytest.mark.parametrize("res", [1.0, 0.3])
def test_export_box_faces(mods, res):
    ndt, po, clouds, _ = mods
    rng = np.random.default_rng(31)
    off = np.array([1e5, -1e5, 0.0], np.float32)
    cloud = slab(rng, [0, 0, 0], [8, 8, 2], 2500) + off
    a = handle(ndt, res=res)
    a.targetAccumulate(cloud)
    cells = row_cells(ndt.acc_blob_rows(a.targetAccumulateExport()))
    assert np.array_equal(np.unique(cells, axis=0), np.unique(cells_of(cloud, res), axis=0))
    leaf = np.float32(res)
    c0 = cells_of((off + np.float32([3, 3, 1]))[None], res)[0]     # a cell inside the scene
    face = np.float32(c0[0]) * leaf                                # about the lower x face of cell c0: crop_cell_range decides
    bounds = [face]                                                # the face of the f32 binning is within a few ulps of it
    for _ in range(16):
        bounds = [np.nextafter(bounds[0], -INF)] + bounds + [np.nextafter(bounds[-1], INF)]
    edge = ndt.crop_cell_range(res, np.float32(bounds), np.float32(bounds))[0]
    assert edge[0] == c0[0] - 1 and edge[-1] == c0[0]
    sizes = set()
    for bound in bounds:
        for side in ("min", "max"):
            mn, mx = np.full(3, -INF, np.float32), np.full(3, INF, np.float32)
            (mn if side == "min" else mx)[0] = bound
            lo, hi = ndt.crop_cell_range(res, mn, mx)
            want = cells[((cells >= lo) & (cells <= hi)).all(axis=1)]
            got = row_cells(ndt.acc_blob_rows(a.targetAccumulateExport(mn, mx)))
            assert len(want) and len(want) < len(cells) and np.array_equal(got, want), (bound, side)
            sizes.add((side, len(got)))
    assert len(sizes) == 4                                         # the face lies among the bounds: both sides of it were exported
    # a closed box with corners on faces, y and z too; and one that selects nothing
    lo_face, hi_face = (c0.astype(np.float32) - np.float32([1, 1, 0])) * leaf, (c0.astype(np.float32) + np.float32([2, 3, 1])) * leaf
    lo, hi = ndt.crop_cell_range(res, lo_face, hi_face)
    got = row_cells(ndt.acc_blob_rows(a.targetAccumulateExport(lo_face, hi_face)))
    assert np.array_equal(got, cells[((cells >= lo) & (cells <= hi)).all(axis=1)]) and len(got)
    nothing = a.targetAccumulateExport(off + 100, off + 101)
    assert len(nothing) == 64 and ndt.acc_blob_info(nothing)["n_voxels"] == 0 and not ndt.acc_blob_info(nothing)["hi"].any()
    assert a.targetExportDiag() == dict(voxels=0, points=0, launches=EXPORT_LAUNCHES)


# ---- 8: rows refused on the device
def test_row_refusals_on_the_device(mods):
    ndt, po, clouds, _lib = mods
    rng = np.random.default_rng(3)
    cloud = slab(rng, [0, 0, 0], [6, 6, 2], 1500)
    mine = slab(rng, [20, 0, 0], [26, 6, 2], 1500)
    src = slab(rng, [19, 0, 0], [27, 6, 2], 300)
    a, b = handle(ndt), handle(ndt)
    a.targetAccumulate(cloud)
    b.targetAccumulate(mine)
    rows = ndt.acc_blob_rows(a.targetAccumulateExport()).copy()
    n = len(rows)
    assert n > 40
    cells = row_cells(rows)
    lo, hi = cells.min(axis=0), cells.max(axis=0)
    bad = []
    r = rows.copy()
    r[[10, 11]] = r[[11, 10]]
    bad.append((make_blob(ndt, r), "ascending"))
    bad.append((make_blob(ndt, np.concatenate([rows[:5], rows[4:]])), "ascending"))       # a duplicated row
    r = rows.copy()
    r["count"][7] = 0
    bad.append((make_blob(ndt, r), "count"))
    r = rows.copy()
    r["d"][n - 1, 4] = np.nan
    bad.append((make_blob(ndt, r), "non-finite"))
    r = rows.copy()
    r["f"][0, 2] = np.inf
    bad.append((make_blob(ndt, r), "non-finite"))
    r = rows.copy()
    r["k"][n - 1] = hi[2] + 1                                       # the last row: keys stay ascending
    bad.append((make_blob(ndt, r, lo=lo, hi=hi), "outside the cell box"))
    wide = hi.copy()
    wide[0] += 1
    bad.append((make_blob(ndt, rows, lo=lo, hi=wide), "tight box"))
    before, stats = observe(ndt, b, src), b.targetAccumulated()
    fresh = handle(ndt)
    for blob, word in bad:
        assert ndt.acc_blob_info(blob)["n_voxels"] in (n, n + 1)    # nothing the device-free checks see
        refused(_lib, lambda: b.targetAccumulateImport(blob), word)
        assert b.targetAccumulated() == stats
        refused(_lib, lambda: fresh.targetAccumulateImport(blob), word)
        assert fresh.targetAccumulated() == dict(points=0, voxels=0, updates=0)
    same_observation(ndt, observe(ndt, b, src), before)
    with pytest.raises(_lib.NdtError) as e:
        fresh.grid()
    assert e.value.status == _lib.NDT_ERR_NO_INPUT                  # a refused first import starts no target
    b.targetAccumulateImport(make_blob(ndt, rows))                  # the rows as they were, through the same builder
    Ref(mods, np.concatenate([mine, cloud]), src).check(b)


# ---- 9: life cycle
def test_life_cycle(mods, tmp_path):
    ndt, po, clouds, _lib = mods
    scans, poses, src = scene(clouds, 3, 2500, seed=23)
    posed = [moved(po, s, T) for s, T in zip(scans, poses)]
    a = handle(ndt)
    for k in range(2):
        a.targetAccumulate(scans[k], poses[k])
    blob = a.targetAccumulateExport()
    b = handle(ndt)
    b.setInputTarget(scans[2])                                      # a cloud target is replaced, not continued
    b.setMinPointPerVoxel(6)
    b.targetAccumulateImport(blob)
    ref01 = Ref(mods, np.concatenate(posed[:2]), src)
    before = ref01.check(b)
    b.warmUp(3000)
    same_observation(ndt, observe(ndt, b, src), before)
    for call in (lambda: b.copy(), lambda: handle(ndt).shareInputTarget(b)):
        with pytest.raises(_lib.NdtError) as e:
            call()
        assert e.value.status == _lib.NDT_ERR_INVALID
    # save and load: the file is the blob; an unwritable path is refused with its name
    path = tmp_path / "map.ndtacc"
    b.targetAccumulateSave(path)
    assert path.read_bytes() == blob and [p.name for p in tmp_path.iterdir()] == ["map.ndtacc"]
    with pytest.raises(_lib.NdtError) as e:
        b.targetAccumulateSave(tmp_path / "nowhere" / "map.ndtacc")
    assert e.value.status == _lib.NDT_ERR_INVALID and "nowhere" in str(e.value) and "No such file" in str(e.value)
    c = handle(ndt)
    assert c.targetAccumulateLoad(path) == b.targetAccumulated()
    same_observation(ndt, observe(ndt, c, src), before)
    refused(_lib, lambda: handle(ndt, res=0.5).targetAccumulateLoad(path), "resolution")
    # a crop after an import, and an import after a crop that removed everything
    hist = History(ndt)
    hist.add(posed[0])
    hist.add(posed[1])
    cat = hist.cat()
    crop_both(b, hist, np.quantile(cat, 0.2, axis=0), np.quantile(cat, 0.85, axis=0))
    Ref(mods, hist.cat(), src).check(b)
    b.targetAccumulate(scans[2], poses[2])
    hist.add(posed[2])
    Ref(mods, hist.cat(), src).check(b)
    crop_both(b, hist, [1000, 1000, 1000], [1001, 1001, 1001])
    assert b.targetAccumulated()["voxels"] == 0
    assert len(b.targetAccumulateExport()) == 64                    # an empty target exports the header alone
    st = b.targetAccumulateImport(blob)
    assert st["points"] == len(cat) and st["updates"] == 3
    same_observation(ndt, observe(ndt, b, src), before)
    ref01.check(b)
    # a resolution change drops the target
    b.setResolution(2.0)
    assert b.targetAccumulated() == dict(points=0, voxels=0, updates=0)
    with pytest.raises(_lib.NdtError) as e:
        b.grid()
    assert e.value.status == _lib.NDT_ERR_NO_INPUT
    refused(_lib, lambda: b.targetAccumulateImport(blob), "resolution")


# ---- 10: paging loses nothing
def test_paging_loses_nothing(mods, tmp_path):
    ndt, po, clouds, _ = mods
    from toyslam_amd.tiles import TilePager
    rng = np.random.default_rng(88)
    n_out = 12
    xs = [60.0 * k / (n_out - 1) for k in range(n_out)]
    xs = xs + xs[::-1]                                              # twelve scans along 60 m and back along the same line
    # a scan reaches 2.4 m along the way and the vehicle goes 5.46 m between two scans: under the 8 m a window of tiles of
    # 8 cells at 1 m keeps around the vehicle's tile, so every update falls into the window of the move before it
    scans = [slab(rng, [-2.4, -7, -3], [2.4, 7, 3], 3000) for _ in xs]
    poses = [clouds.make_T([x, 0.3, 0.2], [0.0, 0.0, 0.0]).astype(np.float32) for x in xs]
    p, q = handle(ndt), handle(ndt)
    pager = TilePager(p, tmp_path / "tiles", tile_cells=8, radius_tiles=1)
    everything = []
    aligned = 0
    for k, (s, T) in enumerate(zip(scans, poses)):
        if k in (14, 18, 22):                                       # on the way back: the window holds what came back from disk
            win = History(ndt)
            win.parts = list(everything)
            win.crop(*pager.window_box(pager.tile))
            assert p.targetAccumulated()["voxels"] == win.voxels() and p.targetAccumulated()["points"] == len(win.cat())
            r = handle(ndt)
            r.setInputTarget(win.cat())
            guess = (T @ clouds.make_T([0.1, -0.05, 0.02], [0.0, 0.0, 0.01])).astype(np.float32)
            results = []
            for h in (p, r):
                h.setInputSource(s[::3])
                h.align(guess)
                results.append((h.getFinalTransformation(), h.getFinalNumIteration(), h.stats()["n_evals"]))
            assert np.array_equal(results[0][0], results[1][0]) and results[0][1:] == results[1][1:], k
            aligned += 1
        posed = moved(po, s, T)
        lo, hi = ndt.crop_cell_range(1.0, *pager.window_box(pager.tile)) if pager.tile is not None else (None, None)
        if lo is not None:
            c = cells_of(posed, 1.0)
            assert ((c >= lo) & (c <= hi)).all(), "the scene of this test: every update inside the current window"
        p.targetAccumulate(s, T)
        q.targetAccumulate(s, T)
        everything.append(posed)
        pager.move_to(T[:3, 3])
        assert p.targetAccumulated()["voxels"] <= pager.window_cells()
    assert aligned == 3
    assert p.targetAccumulated()["voxels"] < q.targetAccumulated()["voxels"]
    pager.flush()
    files = sorted(os.listdir(tmp_path / "tiles"))
    assert len(files) > 27 and all(f.endswith(".ndtacc") for f in files)
    rows = np.concatenate([ndt.acc_blob_rows((tmp_path / "tiles" / f).read_bytes()) for f in files])
    rows = rows[np.argsort(row_keys(rows), kind="stable")]
    want = ndt.acc_blob_rows(q.targetAccumulateExport())
    assert len(rows) == len(want) and rows.tobytes() == want.tobytes()


# ---- 11: the app
def test_map_sequence_saves_and_loads(mods, tmp_path):
    ndt, po, clouds, _ = mods
    scans, d = sequence(clouds, ndt, tmp_path, n=6)
    exe = build_app(tmp_path, "map_sequence")
    f = tmp_path / "map.ndtacc"
    out = subprocess.check_output([exe, "--scan-to-map", "--save-target", str(f), str(d)], text=True)
    line = [ln for ln in out.splitlines() if ln.startswith("accumulated target saved: ")]
    assert len(line) == 1 and "registrations 5 (not converged 0)" in out
    blob = f.read_bytes()
    info = ndt.acc_blob_info(blob)
    assert line[0] == "accumulated target saved: %d voxels, %d bytes" % (info["n_voxels"], len(blob)) and info["n_voxels"] > 1000
    g = handle(ndt)
    g.setStepSize(0.1)
    g.setTransformationEpsilon(0.01)
    g.setMaximumIterations(64)
    g.setNeighborhoodSearchMethod(ndt.DIRECT7)
    g.targetAccumulateLoad(f)
    assert g.targetAccumulateExport() == blob
    loc = subprocess.check_output([exe, "--scan-to-map", "--load-target", str(f), "--localize", str(d)], text=True)
    step, traj = matrices(loc, "Transform "), matrices(loc, "trajectory[")
    assert len(step) == 6 and len(traj) == 6 and "registrations 6 (not converged 0)" in loc
    filt = [po.voxel_grid_filter(sc, 0.5)[0] for sc in scans]
    pose = np.eye(4, dtype=np.float32)
    for k in range(6):                                              # the same loop here: guess = previous pose, identity first
        g.setInputSource(filt[k])
        g.align(pose)
        assert g.hasConverged()
        pose = g.getFinalTransformation().astype(np.float32)
        print("scan %d: rot %.3g trans %.3g" % (k, rot_err(step[k], pose), trans_err(step[k], pose)))
        assert rot_err(step[k], pose) < 1e-5 and trans_err(step[k], pose) < 1e-5, k
        assert np.array_equal(step[k], traj[k])
    assert g.targetAccumulateExport() == blob                       # localising changed nothing
    # loading and mapping on: the run continues the map and can save it again
    f2 = tmp_path / "map2.ndtacc"
    more = subprocess.check_output([exe, "--scan-to-map", "--load-target", str(f), "--save-target", str(f2), str(d)], text=True)
    assert "registrations 6 (not converged 0)" in more
    assert ndt.acc_blob_info(f2.read_bytes())["n_voxels"] >= info["n_voxels"]
    for wrong in (["--save-target", str(f), str(d)], ["--load-target", str(f), str(d)], ["--scan-to-map", "--localize", str(d)],
                  ["--scan-to-map", "--save-target"], ["--scan-to-map", str(d), "--load-target"]):
        assert subprocess.run([exe] + wrong, capture_output=True).returncode == 2, wrong
