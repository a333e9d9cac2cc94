"""GPU: the kernels that move points -- k_transform (one scan into the map; align()'s output cloud) and k_transform_multi
(many scans, each with its own run of blocks) -- and the box the map's filter is given without a pass over the moved points
(join_moved_box: the scans' boxes under their poses, padded), at the sizes where their blocks and strides change.

Two views of the moved records.  Filtered: the map after the call against the oracle's transform_cloud + voxel_grid_filter
of the concatenation, bit for bit, with every point alone in its voxel (points at least 0.5 m apart, voxels of 0.25 m with
a diagonal of 0.433 m), so a wrong or missing record is a wrong or missing row.  Unfiltered: a leaf so small that the voxel
indices overflow makes the filter pass its input through, as PCL does -- the map then IS the moved records, in order, and
each is held against the oracle's record bit for bit and against an f64 numpy transform within gamma_4 (|R| |p| + |t|) per
coordinate: every term goes through at most four f32 roundings (a product and three sums, unfused), u = 2^-24.  That bound
is derived, not measured."""
import numpy as np
import pytest

import cloud_box_cases as cb
from cloud_box_cases import F32
from test_gpu_parity import _DeviceCopies, mods  # noqa: F401

pytestmark = pytest.mark.gpu

K = cb.BLOCK
T1 = cb.TRANSFORM_MAX_BLOCKS * K  # 524 288: one row per thread of the 2 048 blocks a scan gets at most
LEAF = 0.25                       # 1 / LEAF is exact in f32: a voxel face is a multiple of 0.25
EMPTY = np.zeros((0, 3), F32)


def lattice_scan(n, seed, origin=(0.0, 0.0, 0.0)):
    """n points on distinct sites of a 0.6 m lattice, each within 0.05 m of its site: any two are at least 0.5 m apart, under
    every rigid transform -- more than the diagonal of a voxel of LEAF, so no two share one"""
    rng = np.random.default_rng(seed)
    m = int(np.ceil(n ** (1.0 / 3.0))) + 1
    sites = rng.choice(m ** 3, n, replace=False)
    ijk = np.stack([sites % m, sites // m % m, sites // (m * m)], axis=1)
    return (ijk * 0.6 + rng.uniform(-0.05, 0.05, (n, 3)) + np.asarray(origin)).astype(F32)


def with_non_finite_rows(scan):
    """rows a cloud that is not dense may hold: transformPointCloud leaves them as they are, the filter drops them"""
    scan = scan.copy()
    n = len(scan)
    if n > 3:
        scan[1, 0] = np.nan
        scan[n // 2] = np.inf
        scan[n - 2, 2] = -np.inf
    return scan


def moved(po, scan, T, dense=True):
    out = scan[:, :3].copy()
    ok = np.ones(len(scan), bool) if dense else np.isfinite(scan[:, :3]).all(axis=1)
    out[ok] = po.transform_cloud(np.c_[scan[ok, :3], np.ones(int(ok.sum()), F32)], T)[:, :3]
    return out


def within_f64_allowance(got, scan, T):
    ok = np.isfinite(scan[:, :3]).all(axis=1)
    ref, tol = cb.moved_f64(scan[ok], T)
    err = np.abs(got[ok].astype(np.float64) - ref)
    assert (err <= tol).all(), (err.max(), tol.min())


def pass_through_leaf(pts):
    """a leaf for which dx * dy * dz is about 1e12 (far above INT32_MAX, every factor far below it)"""
    fin = pts[np.isfinite(pts).all(axis=1)]
    ext = (fin.max(axis=0) - fin.min(axis=0)).astype(np.float64)
    assert (ext > 0.01).all()
    return float((ext.prod() / 1e12) ** (1.0 / 3.0))


def pose(clouds, t, deg):
    return clouds.make_T(t, np.deg2rad(deg)).astype(F32)


def run_scans(mods, scans, poses, dense, form="clouds", launches=1):
    """the scans moved into an empty map: unfiltered, then filtered, each against the oracle"""
    ndt, po, clouds = mods
    flags = [dense] * len(scans) if np.ndim(dense) == 0 else list(dense)
    want = [moved(po, s, T, d) for s, T, d in zip(scans, poses, flags)]
    cat = np.concatenate(want) if want else EMPTY
    all_dense = all(flags)
    g = ndt.NormalDistributionsTransform()

    def update(leaf):
        if form == "clouds":
            return g.mapUpdateClouds([g.uploadCloud(s) for s in scans], poses, leaf, is_dense=flags)
        return g.mapUpdateBatch(scans, poses, leaf, is_dense=flags)

    n_fin = int(np.isfinite(cat).all(axis=1).sum())
    if n_fin > 1:
        tiny = pass_through_leaf(cat)
        assert po.voxel_grid_filter(cat, tiny, is_dense=all_dense)[1]
        n_map, ov = update(tiny)
        assert ov and n_map == len(cat)
        assert g.mapBatchDiag()["transform_launches"] == launches
        got = g.mapGet()
        assert np.array_equal(got, cat, equal_nan=True)  # every moved record, in order
        first = 0
        for s, T in zip(scans, poses):
            within_f64_allowance(got[first:first + len(s)], s, T)
            first += len(s)
        g.mapClear()
    ref, ov_ref = po.voxel_grid_filter(cat, LEAF, is_dense=all_dense)
    n_map, ov = update(LEAF)
    assert not ov and not ov_ref
    assert g.mapBatchDiag() == dict(transform_launches=launches, filters=1, box_passes=0)
    assert len(ref) == n_fin  # every point alone in its voxel
    assert n_map == len(ref) and np.array_equal(g.mapGet(), ref)
    if len(cat) == 1:  # (too few points for a box that overflows: the map's one row is the moved record)
        k = [len(sc) for sc in scans].index(1)
        within_f64_allowance(g.mapGet(), scans[k], poses[k])
    return g


# ---- k_transform: one scan with points ------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("n", [1, K - 1, K, K + 1, T1, T1 + 1])
def test_one_scan_at_k_transforms_block_and_stride_boundaries(mods, n, dense):
    """2 048 blocks at most: row 524 288 is the second row of block 0's first thread"""
    _, _, clouds = mods
    scan = lattice_scan(n, seed=n)
    if not dense:
        scan = with_non_finite_rows(scan)
    T = pose(clouds, [12.5, -7.25, 3.0], [20.0, -35.0, 50.0])
    run_scans(mods, [scan], [T], dense)
    if n == K + 1:  # an empty scan beside it: still the one-scan kernel
        run_scans(mods, [EMPTY, scan, EMPTY], [T, T, T], dense)


# ---- k_transform_multi: every scan its own run of blocks, its own pose ---------------------------------------------------
def scan_set(sizes, seed, gap=2.0):
    """scans on lattices of their own, side by side along x with `gap` metres between them: near enough for the whole set to
    stay far below INT32_MAX / 2 voxels of LEAF under the poses below (the guessed box is then used as it is), and -- as the
    count of the oracle's output shows in every case -- with no two moved points in one voxel"""
    out, x = [], 0.0
    for k, n in enumerate(sizes):
        out.append(lattice_scan(n, seed + k, origin=(x, 0.0, 0.0)) if n else EMPTY)
        if n:
            x += 0.6 * (int(np.ceil(n ** (1.0 / 3.0))) + 1) + gap
    return out


def poses_for(clouds, count):
    """every scan a pose of its own: a little further and a little more turned than the one before"""
    return [pose(clouds, [0.3 * k, -0.2 * k, 0.05 * k], [0.5 * k, -0.7 * k, 1.3 * k]) for k in range(count)]


SETS = {"three_of_one": [1, 1, 1], "mixed": [K, K + 1, 1, T1 + 1], "sixty_five_of_one": [1] * 65,
        "empty_between": [0, K + 1, 0, 0, 3 * K + 7, 0, 1, 0]}


@pytest.mark.parametrize("form", ["clouds", "buffer"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_scan_sets_through_k_transform_multi(mods, name, form):
    _, _, clouds = mods
    scans = scan_set(SETS[name], seed=len(name))
    run_scans(mods, scans, poses_for(clouds, len(scans)), True, form=form)


@pytest.mark.parametrize("form", ["clouds", "buffer"])
def test_mixed_nan_rules_per_scan(mods, form):
    _, _, clouds = mods
    scans = scan_set([K + 1, 2 * K, 700, K - 1], seed=77)
    dense = [True, False, False, True]
    scans = [s if d else with_non_finite_rows(s) for s, d in zip(scans, dense)]
    run_scans(mods, scans, poses_for(clouds, 4), dense, form=form)


# ---- the guessed box must hold every moved point ----------------------------------------------------------------------
GUESS_POSES = {"identity": ([0, 0, 0], [0, 0, 0]), "x45": ([1, 2, 3], [45, 0, 0]), "y45": ([1, 2, 3], [0, 45, 0]), "z45": ([1, 2, 3], [0, 0, 45]),
               "general": ([-4, 9, 2], [33, -21, 117]), "t1e3": ([1e3, -1e3, 1e3], [3, 2, 1]), "t1e5": ([1e5, 1e5, -1e5], [0, 0, 30])}


@pytest.mark.parametrize("name", sorted(GUESS_POSES))
def test_guessed_box_holds_every_moved_point(mods, name):
    """every point is alone in its voxel, the extreme ones too: one that falls outside the guessed box is a missing row (or one
    merged into a neighbouring row).  box_passes == 0: the guess was what the filter used."""
    _, _, clouds = mods
    t, deg = GUESS_POSES[name]
    T = pose(clouds, t, deg)
    one = lattice_scan(8000, seed=5)
    run_scans(mods, [one], [T], True)
    pair = [lattice_scan(3000, seed=6), lattice_scan(2999, seed=7, origin=(30.0, -30.0, 5.0))]
    run_scans(mods, pair, [T, pose(clouds, np.asarray(t) + [5, 5, 5], deg)], True)


def corner_below_a_face(po, T):
    """a point (x, y, 0) whose f32 image under T (45 degrees about z) has an x on or above a voxel face that the f64 image,
    rounded to f32, lies below: x is solved for images at a face, then walked a few ulps either way"""
    T64 = T.astype(np.float64)
    y = F32(12.3)
    faces = np.arange(380, 420) * LEAF
    xs = [((faces - T64[0, 3] - T64[0, 1] * float(y)) / T64[0, 0]).astype(F32)]
    for _ in range(30):
        xs.append(np.nextafter(xs[-1], F32(np.inf)))
        xs.insert(0, np.nextafter(xs[0], F32(-np.inf)))
    x = np.concatenate(xs)
    pts = np.c_[x, np.full(len(x), y), np.zeros(len(x), F32)].astype(F32)
    img32 = po.transform_cloud(np.c_[pts, np.ones(len(pts), F32)], T)[:, 0]
    img64 = (pts[:, 0].astype(np.float64) * T64[0, 0] + pts[:, 1].astype(np.float64) * T64[0, 1] + T64[0, 3]).astype(F32)
    hit = np.flatnonzero(np.floor(img32 * F32(1.0 / LEAF)) > np.floor(img64 * F32(1.0 / LEAF)))
    assert len(hit) > 0, "no candidate crosses a face"
    return pts[hit[0]]


def test_an_extreme_point_beyond_the_moved_corner_of_its_box_is_kept(mods):
    """The moved point is three f32 products and three f32 sums; the moved corner of the scan's box is f64.  Here the scan's
    (max x, min y) corner IS a point, turned by 45 degrees about z, and chosen so that its f32 image lies on or above a
    voxel face that the f64 image of the corner lies below: without the pad of the guessed box the lattice would end one
    column too early and the point's linear index would be that of the first column of the next row -- where this scan has
    a second point (`wrap`), so the two would come out as one centroid.  (Alone in that cell the point would keep its place
    in the output's order: a row that is merely one column short shows only through such a neighbour.)"""
    ndt, po, clouds = mods
    T = pose(clouds, [100.0, 0.0, 0.0], [0.0, 0.0, 45.0])
    T64 = T.astype(np.float64)
    inv = F32(1.0 / LEAF)
    corner = corner_below_a_face(po, T)
    cell = lambda p: np.floor(moved(po, np.atleast_2d(p), T) * inv).astype(np.int64)  # noqa: E731
    c_cell = cell(corner)[0]
    # `wrap`: the scan's (min x, max y) corner, its image in the middle of a voxel of the next y row, far below every other x
    q = np.array([75.0 + 0.4 * LEAF, (c_cell[1] + 1.5) * LEAF, 0.0])
    wrap = (T64[:3, :3].T @ (q - T64[:3, 3])).astype(F32)
    scan = lattice_scan(4000, seed=8, origin=(float(corner[0]) - 11.0, float(corner[1]) + 1.0, 0.0))
    scan = np.concatenate([scan[:1000], corner[None, :], scan[1000:3000], wrap[None, :], scan[3000:]])
    b = cb.reference_boxes(scan)
    assert b[1, 1, 0] == corner[0] and b[1, 0, 1] == corner[1]  # the corner owns max x and min y,
    assert b[1, 0, 0] == wrap[0] and b[1, 1, 1] == wrap[1]       # `wrap` min x and max y
    cells = cell(scan)
    w_cell = cell(wrap)[0]
    assert (w_cell[1:] == c_cell[1:] + [1, 0]).all() and (cells[:, 0] >= w_cell[0]).all() and (cells[:, 0] == w_cell[0]).sum() == 1
    # the lattice of the box without a pad: f32(f64 image of the box's corners), as join_moved_box joins them
    corners = np.array([[b[1, i, 0], b[1, j, 1], 0.0] for i in (0, 1) for j in (0, 1)], np.float64) @ T64[:3, :3].T + T64[:3, 3]
    lo, hi = np.floor(corners.min(axis=0).astype(F32) * inv), np.floor(corners.max(axis=0).astype(F32) * inv)
    div_x = int(hi[0] - lo[0]) + 1
    assert c_cell[0] - lo[0] == div_x and w_cell[0] == lo[0]  # one column beyond it: the index of `wrap`'s cell
    g = run_scans(mods, [scan], [T], True)
    assert g.mapBatchDiag()["box_passes"] == 0


def test_near_index_overflow_the_exact_box_decides(mods):
    """two small scans some 285 m apart on every axis at a leaf of 0.25 m: about 1 150 voxels a side, more than INT32_MAX / 2 and
    fewer than INT32_MAX in all -- the padded guess is too near the overflow test, so one pass over the moved points gives
    the exact box (k_bbox), and the map is the oracle's all the same"""
    ndt, po, clouds = mods
    scans = [lattice_scan(500, seed=1), lattice_scan(501, seed=2)]
    poses = [pose(clouds, [0, 0, 0], [0, 0, 10]), pose(clouds, [280.0, 280.0, 280.0], [5, 0, 0])]
    cat = np.concatenate([moved(po, s, T) for s, T in zip(scans, poses)])
    ref, ov_ref = po.voxel_grid_filter(cat, LEAF)
    assert not ov_ref and len(ref) == 1001
    g = ndt.NormalDistributionsTransform()
    n_map, ov = g.mapUpdateClouds([g.uploadCloud(s) for s in scans], poses, LEAF)
    assert g.mapBatchDiag() == dict(transform_launches=1, filters=1, box_passes=1)
    assert not ov and n_map == len(ref) and np.array_equal(g.mapGet(), ref)


# ---- align()'s output cloud ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, K - 1, K, K + 1, T1 + 1])
def test_aligned_cloud_is_the_source_under_the_final_transformation(mods, pair, n):
    ndt, po, clouds = mods
    t, _ = pair
    rng = np.random.default_rng(n)
    lo, hi = t.min(axis=0), t.max(axis=0)
    src = (t[rng.integers(0, len(t), n)] + rng.normal(0, 0.05, (n, 3))).astype(F32) if n > 1 else ((lo + hi) / 2)[None, :].astype(F32)
    g = ndt.NormalDistributionsTransform()
    g.setMaximumIterations(1)
    g.setInputTarget(t)
    g.setInputSource(src)
    guess = pose(clouds, [0.2, -0.1, 0.05], [0.5, -0.3, 1.0])
    out = g.align(guess=guess, n_out=n)
    T = g.getFinalTransformation()
    assert np.isfinite(T).all() and (n == 1 or not np.array_equal(T, guess))  # (a step was taken: not the guess's cloud)
    want = po.transform_cloud(np.c_[src, np.ones(n, F32)], T)
    assert np.array_equal(out[:, :3], want[:, :3]) and (out[:, 3] == 1.0).all()
    within_f64_allowance(out[:, :3], src, T)
