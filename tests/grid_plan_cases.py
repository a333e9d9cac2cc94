"""Clouds that sit ON the boundaries of the target-grid build's plan, shared by tests/test_grid_plan_cases.py (CPU: placement
and the oracle side), tests/test_gpu_grid_plans.py (GPU) and tests/grid_plan_child.py (GPU, under switched plans).

Sizes and boxes are FOUND by asking the library (ndt.host_grid_plan = ndt_host_grid_plan, ndt.host_lattice), never copied
from its formulae; every case carries `claims`, the statements about its plan that its name makes, and `expect`, the plan the
library must report after the build (gridBuild = ndt_diag_grid_build).  What a build must COMPUTE never comes from the plan:
it is the oracle's grid and the oracle's evaluation.

A lattice of exactly dx x dy x dz cells of pitch 1 is made by keeping every point inside [lo + EPS, hi - EPS] and adding the
two corner points; cells are numbered x fastest.  Where a case fills chosen buckets, the cell -> bucket map is the dealing
rule stated with K1Deal (runs of eight cells dealt round-robin: bucket = (cell >> 3) mod K, local cell = ((cell >> 3) / K) * 8
+ cell mod 8); the CPU test checks the resulting contents by counting, and the GPU test checks results against the oracle only."""
import numpy as np

LEAF = 1.0
ORIGIN = np.array([-7.0, 3.0, -2.0])
EPS = 1.0 / 64.0
MIN_PTS = 6
RUN = 8                      # cells per dealt run (checked against the plan's answer by run_bits_hold)
BOX_A = (64, 64, 16)
N_SOURCE = 2000
POSE = np.array([0.11, -0.07, 0.05, 0.008, -0.004, 0.015])
# The arrival-order cases of group C lie kilometres from the origin.  A voxel's covariance is a difference of sums of squares
# (one pass, as in the reference): there the sums of a few dozen points round in f64, and the order they are added in reaches
# the f32 records -- next to the origin every order gives the same bits and an unstable placement would go unseen.  A rotation
# of the source about the origin would carry it out of the box, so their pose is a translation.
ORIGIN_FAR = np.array([4096.0 - 7.0, -8192.0 + 3.0, 2048.0 - 2.0])
POSE_FAR = np.array([0.11, -0.07, 0.05, 0.0, 0.0, 0.0])
PLAN_FIELDS = ("n_buckets", "cells_per_bucket", "pts_per_block", "n_blocks", "wmax", "lds_cap")
ORDERS = ("sorted", "reversed", "round_robin")


def _ndt():
    from toyslam_amd import ndt
    return ndt


def n_cells_of(dims):
    return int(dims[0]) * int(dims[1]) * int(dims[2])


def plan_of(dims, n):
    return _ndt().host_grid_plan(n_cells_of(dims), n, dims)


def lattice_of(cloud, voxel_index=0):
    fin = cloud[np.isfinite(cloud).all(axis=1)]
    return _ndt().host_lattice(LEAF, fin.min(axis=0), fin.max(axis=0), voxel_index, len(cloud))


def form_of(dims, n, voxel_index):
    """The form build_grid must take, from the library's two host answers."""
    lo = ORIGIN + EPS
    hi = ORIGIN + np.asarray(dims) - EPS
    if _ndt().host_lattice(LEAF, lo, hi, voxel_index, n)["sparse"]:
        return "sparse"
    p = plan_of(dims, n)
    return "chain" if not p["bucket_form"] else "one_launch" if p["one_launch"] else "buckets"


def expect_of(dims, n, voxel_index):
    p = plan_of(dims, n)
    form = form_of(dims, n, voxel_index)
    e = dict(form=form, n_points=n, n_cells=n_cells_of(dims))
    if form == "buckets":
        e.update({k: p[k] for k in PLAN_FIELDS})
    if form == "one_launch":
        e.update(n_buckets=p["n_buckets"], cells_per_bucket=p["cells_per_bucket"])
    if form != "sparse":
        e.update({k: p[k] for k in ("lut_cells", "compact_items", "compact_tiles", "compact_prefix")})
    return e


# ---- geometry -----------------------------------------------------------------------------------------------------------
def cells_of(cloud, dims, origin=ORIGIN):
    """Linear cell (x fastest) of every finite point, -1 for the others."""
    c = np.asarray(cloud, dtype=np.float64)
    fin = np.isfinite(c).all(axis=1)
    i = np.floor(np.where(fin[:, None], c, origin) - origin).astype(np.int64)
    lin = i[:, 0] + dims[0] * (i[:, 1] + dims[1] * i[:, 2])
    return np.where(fin, lin, -1)


def points_in_cells(rng, cells, dims, spread=0.4, origin=ORIGIN):
    cells = np.asarray(cells, dtype=np.int64)
    ix, iy, iz = cells % dims[0], (cells // dims[0]) % dims[1], cells // (dims[0] * dims[1])
    u = 0.5 + rng.uniform(-spread, spread, (len(cells), 3))
    return (origin + np.c_[ix, iy, iz] + u).astype(np.float32)


def bucket_of(cells, K):
    return (np.asarray(cells) >> 3) % K


def local_of(cells, K):
    c = np.asarray(cells)
    return ((c >> 3) // K) * RUN + (c & 7)


def cell_at(bucket, local, K):
    return (((local >> 3) * K + bucket) << 3) | (local & 7)


def mixed_cells(rng, n, dims, K=0, avoid=()):
    """Cells of n points: half uniform over the box, half in clusters of about twelve points per cell; none in the buckets
    `avoid` of a deal over K buckets."""
    nc = n_cells_of(dims)
    avoid = np.asarray(sorted(avoid), dtype=np.int64)

    def draw(m):
        out = rng.integers(0, nc, m)
        while len(avoid):
            bad = np.isin(bucket_of(out, K), avoid)
            if not bad.any():
                break
            out[bad] = rng.integers(0, nc, int(bad.sum()))
        return out
    n_cl = n // 2
    centres = draw(max(1, n_cl // 12))
    return np.concatenate([draw(n - n_cl), centres[rng.integers(0, len(centres), n_cl)]])


def finish_cloud(pts, dims, dense, origin=ORIGIN):
    """The two corner points at both ends, every point inside the box, and (dense=False) three non-finite points."""
    lo = (origin + EPS).astype(np.float32)
    hi = (origin + np.asarray(dims) - EPS).astype(np.float32)
    c = np.clip(np.asarray(pts, dtype=np.float32), lo, hi)
    c[0], c[-1] = lo, hi
    if not dense:
        n = len(c)
        c[n // 3] = np.nan
        c[n // 2, 1] = np.inf
        c[n - 2, 2] = -np.inf
    return np.ascontiguousarray(c)


def mixed_cloud(seed, n, dims, dense=True):
    rng = np.random.default_rng(seed)
    cells = mixed_cells(rng, n, dims)
    rng.shuffle(cells)
    return finish_cloud(points_in_cells(rng, cells, dims), dims, dense)


def reorder(cloud, dims, order, origin=ORIGIN):
    """The cloud's points between the two corners in one of ORDERS by cell (a cell's points keep their relative order)."""
    inner = cloud[1:-1]
    cells = cells_of(inner, dims, origin)
    by_cell = np.argsort(cells, kind="stable")
    if order == "sorted":
        perm = by_cell
    elif order == "reversed":
        perm = by_cell[np.argsort(-cells[by_cell], kind="stable")]
    else:  # round robin over the cells: first points of every cell, then the second points, ...
        sc = cells[by_cell]
        first = np.r_[0, np.flatnonzero(np.diff(sc)) + 1]
        rank = np.arange(len(sc)) - np.repeat(first, np.diff(np.r_[first, len(sc)]))
        perm = by_cell[np.lexsort((sc, rank))]
    return np.ascontiguousarray(np.concatenate([cloud[:1], inner[perm], cloud[-1:]]))


def source_of(cloud, seed=5):
    rng = np.random.default_rng(seed)
    fin = cloud[np.isfinite(cloud).all(axis=1)]
    return np.ascontiguousarray(fin[rng.choice(len(fin), min(N_SOURCE, len(fin)), replace=False)])


# ---- the chooser ----------------------------------------------------------------------------------------------------------
def steps(f, lo, hi, coarse=64):
    """Every b in (lo, hi] with f(b) != f(b - 1), for f piecewise constant with pieces of at least `coarse` arguments."""
    out = []
    a, fa = lo, f(lo)
    while a < hi:
        b = min(hi, a + coarse)
        fb = f(b)
        if fb != fa:
            l, r = a, b  # f(l) == fa, f(r) != fa
            while r - l > 1:
                m = (l + r) // 2
                if f(m) == fa:
                    l = m
                else:
                    r = m
            out.append(r)
            a, fa = r, f(r)
        else:
            a = b
    return out


def first_dz(dx, dy, pred, hi=1200):
    """The smallest dz >= 2 with pred((dx, dy, dz)) and not pred((dx, dy, dz - 1))."""
    for dz in range(2, hi):
        if pred((dx, dy, dz)) and not pred((dx, dy, dz - 1)):
            return dz
    raise AssertionError("no step found for a box of %d x %d x dz" % (dx, dy))


class Case:
    def __init__(self, name, group, dims, n, make, voxel_index=0, dense=True, claims=(), counts=(), contents=None, far=False):
        self.name, self.group, self.dims, self.n, self.voxel_index, self.dense = name, group, tuple(dims), n, voxel_index, dense
        self.origin, self.pose = (ORIGIN_FAR, POSE_FAR) if far else (ORIGIN, POSE)
        self._make, self._cloud = make, None
        self.claims = list(claims)       # (what the name says, whether the library's plan says so too)
        self.counts = tuple(counts)      # point counts that some voxel of the oracle's grid must have
        self.contents = contents         # (cloud, plan) -> [(statement, bool)]: bucket contents, by counting
        self.expect = expect_of(self.dims, n, voxel_index)

    def cloud(self):
        if self._cloud is None:
            c = self._make()
            assert len(c) == self.n, (self.name, len(c), self.n)
            lat = lattice_of(c, self.voxel_index)
            assert tuple(lat["div_b"]) == self.dims, (self.name, lat["div_b"])
            c.setflags(write=False)
            self._cloud = c
        return self._cloud

    def __repr__(self):
        return self.name


def _pair(name, group, f_lo, f_hi, claim):
    """Two cases either side of a step; `claim(plan_lo, plan_hi)` -> [(statement, bool)] is attached to both."""
    lo, hi = f_lo("%s-below" % name), f_hi("%s-above" % name)
    cl = claim(plan_of(lo.dims, lo.n), plan_of(hi.dims, hi.n), lo, hi)
    lo.claims += cl
    hi.claims += cl
    return [lo, hi]


def group_a():
    """Point count over BOX_A: both sides of every step of the plan between the one-launch form and 300 000 points."""
    dims = BOX_A
    P = lambda n: plan_of(dims, n)
    out = []

    def case(n, seed):
        dense = seed % 2 == 0
        return lambda name: Case(name, "A", dims, n, lambda: mixed_cloud(seed, n, dims, dense), dense=dense)
    b = steps(lambda n: P(n)["one_launch"], 1000, 100000)
    assert len(b) == 1
    b_one = b[0]
    out += _pair("A-one_launch_to_buckets", "A", case(b_one - 1, 11), case(b_one, 12), lambda lo, hi, *_: [
        ("one-launch form below", lo["one_launch"]), ("bucket form above", hi["bucket_form"] and not hi["one_launch"]),
        ("empty trailing blocks above", hi["n_blocks"] > -(-b_one // hi["pts_per_block"]))])
    # the first size above where the real blocks fill the grid of blocks exactly; one more point: a block with one point
    ppb = P(b_one)["pts_per_block"]
    full = next(n for n in range(-(-b_one // ppb) * ppb, 400000, ppb) if P(n)["n_blocks"] * P(n)["pts_per_block"] == n)
    out += _pair("A-last_block_full_to_one_point", "A", case(full, 13), case(full + 1, 14), lambda lo, hi, *_: [
        ("every block full below", lo["n_blocks"] * lo["pts_per_block"] == full),
        ("last real block holds one point above", (full + 1) % hi["pts_per_block"] == 1),
        ("same points per block", lo["pts_per_block"] == hi["pts_per_block"])])
    ks = steps(lambda n: P(n)["n_buckets"], b_one, 300000)
    for i, bk in enumerate(ks):
        out += _pair("A-K_step%d" % (i + 1), "A", case(bk - 1, 15 + 2 * i), case(bk, 16 + 2 * i), lambda lo, hi, *_: [
            ("bucket count changes", lo["n_buckets"] != hi["n_buckets"]), ("bucket form on both sides", lo["bucket_form"] and hi["bucket_form"])])
    return out, dict(one_launch=b_one, full=full, k_steps=ks)


def group_b():
    """Cell count: lattices either side of every step of the plan in the cell count."""
    out = []

    def case(dims, n, seed, vi=0):
        return lambda name: Case(name, "B", dims, n, lambda: mixed_cloud(seed, n, dims, seed % 2 == 0), voxel_index=vi, dense=seed % 2 == 0)

    def pair(name, dx, dy, n, pred, claim, seed, vi=0):
        dz = first_dz(dx, dy, lambda d: pred(plan_of(d, n), d))
        return _pair(name, "B", case((dx, dy, dz - 1), n, seed, vi), case((dx, dy, dz), n, seed + 1, vi), claim)
    n = 50000
    out += pair("B-C_wmax_to_2wmax", 64, 64, n, lambda p, d: p["cells_per_bucket"] > p["wmax"], lambda lo, hi, *_: [
        ("a pass spans the bucket below", lo["cells_per_bucket"] == lo["wmax"]), ("buckets wider than a pass above", hi["cells_per_bucket"] > hi["wmax"])], 31)
    out += pair("B-Cmax_K_step", 128, 128, n, lambda p, d: p["n_buckets"] > 256, lambda lo, hi, *_: [
        ("fullest buckets below", lo["n_buckets"] == 256 and lo["cells_per_bucket"] == hi["cells_per_bucket"]),
        ("more buckets above", hi["n_buckets"] > lo["n_buckets"]), ("the pass cap is the smallest", hi["lds_cap"] <= 1024)], 33)
    out += pair("B-small_cloud_leaves_one_launch", 128, 128, 5000, lambda p, d: not p["one_launch"], lambda lo, hi, *_: [
        ("one-launch form below, more than 256 buckets", lo["one_launch"] and lo["n_buckets"] > 256),
        ("bucket form at 5000 points above", hi["bucket_form"] and not hi["one_launch"])], 35)
    sp = lambda d: _ndt().host_lattice(LEAF, ORIGIN + EPS, ORIGIN + np.asarray(d) - EPS, 0, n)["sparse"]
    dz = first_dz(256, 256, sp)
    out += _pair("B-auto_dense_to_sparse", "B", case((256, 256, dz - 1), n, 37), case((256, 256, dz), n, 38), lambda lo, hi, a, b: [
        ("dense below", a.expect["form"] == "buckets"), ("sparse above", b.expect["form"] == "sparse")])
    out += pair("B-forced_dense_K_max", 256, 256, n, lambda p, d: p["n_buckets"] > 4096, lambda lo, hi, *_: [
        ("K doubles to the largest", hi["n_buckets"] == 2 * lo["n_buckets"]), ("bucket form", lo["bucket_form"] and hi["bucket_form"])], 39, vi=1)
    out += pair("B-forced_dense_buckets_to_chain", 512, 256, n, lambda p, d: not p["bucket_form"], lambda lo, hi, a, b: [
        ("bucket form with the most buckets below", a.expect["form"] == "buckets" and lo["n_buckets"] == 8192),
        ("dense chain above", b.expect["form"] == "chain")], 41, vi=1)
    return out


# ---- group C: bucket contents -----------------------------------------------------------------------------------------------
def _contents_cloud(seed, dims, n, K, fill, order):
    """fill: {bucket: [(local cell, points)]}; the rest of the n points is a mixed cloud outside those buckets and the corners'."""
    rng = np.random.default_rng(seed)
    nc = n_cells_of(dims)
    corner_b = {int(bucket_of(0, K)), int(bucket_of(nc - 1, K))}
    assert not corner_b & set(fill)
    cells = []
    for b, lst in sorted(fill.items()):
        for local, cnt in lst:
            c = cell_at(b, local, K)
            assert 0 <= c < nc and bucket_of(c, K) == b and local_of(c, K) == local
            cells.append(np.full(cnt, c, dtype=np.int64))
    cells = np.concatenate(cells)
    rest = n - 2 - len(cells)
    assert rest > 0, rest
    cells = np.concatenate([cells, mixed_cells(rng, rest, dims, K, set(fill) | corner_b)])
    rng.shuffle(cells)
    inner = points_in_cells(rng, cells, dims, origin=ORIGIN_FAR)
    pad = np.zeros((1, 3), np.float32)
    return reorder(finish_cloud(np.concatenate([pad, inner, pad]), dims, True, ORIGIN_FAR), dims, order, ORIGIN_FAR)


def group_c():
    dims, n = BOX_A, 60000
    p = plan_of(dims, n)
    K, C, cap = p["n_buckets"], p["cells_per_bucket"], p["lds_cap"]
    team = cap // 33
    nc = n_cells_of(dims)
    top = lambda b, r: (((nc >> 3) - 1 - b) // K) * RUN + r   # a local cell in the bucket's last run inside the box
    fill = {
        3: [(0, MIN_PTS - 1), (1, MIN_PTS), (9, 32), (10, 33), (top(3, 7), 33)],
        17: [(5, cap)], 18: [(top(18, 5), cap + 1)], 19: [(40, 6000)],
        33: [(l, 32) for l in range(64)],                                    # 2048 points: the one-shot limit
        34: [(l, 32) for l in range(64)] + [(200, 1)],                       # 2049
        49: [(l, cap // 8) for l in range(8)] + [(l, 100) for l in range(8, 13)],               # first pass ends at cap exactly
        50: [(0, cap // 8 + 1)] + [(l, cap // 8) for l in range(1, 8)] + [(l, 100) for l in range(8, 13)],  # one point over
        65: [(2 * l, 33) for l in range(team)],                              # as many 33-point cells as one pass holds
    }

    def contents(cloud, plan):
        cells = cells_of(cloud, dims, ORIGIN_FAR)
        b, l = bucket_of(cells, plan["n_buckets"]), local_of(cells, plan["n_buckets"])
        size = np.bincount(b, minlength=plan["n_buckets"])
        lead = lambda k, m: int(((b == k) & (l < m)).sum())
        return [("the plan the contents were made for", (plan["n_buckets"], plan["cells_per_bucket"], plan["lds_cap"]) == (K, C, cap)),
                ("cap a multiple of 8, one-shot limit inside it", cap % 8 == 0 and 2049 <= cap and C <= plan["wmax"]),
                ("a bucket of 2048 points", size[33] == 2048), ("a bucket of 2049 points", size[34] == 2049),
                ("leading cells hold lds_cap points, the bucket more", lead(49, 8) == cap and size[49] > cap),
                ("leading cells hold lds_cap + 1 points", lead(50, 8) == cap + 1 and lead(50, 7) < cap),
                ("cells of 33 points fill one pass", size[65] == 33 * team and size[65] <= cap < size[65] + 33),
                ("single cells at and over the cap", size[17] == cap and size[18] == cap + 1 and size[19] == 6000)]
    out = []
    for i, order in enumerate(ORDERS):
        out.append(Case("C-contents-%s" % order, "C", dims, n, lambda o=order: _contents_cloud(71, dims, n, K, fill, o),
                        claims=[("bucket form", p["bucket_form"] and not p["one_launch"])],
                        counts=(MIN_PTS - 1, MIN_PTS, 32, 33, cap, cap + 1, 6000), contents=contents, far=True))
    # the whole cloud in one run of eight cells: one full bucket, every other bucket empty
    rdims, rn = (RUN, 1, 1), 50000
    rp = plan_of(rdims, rn)

    def run_cloud(order):
        rng = np.random.default_rng(72)
        cells = rng.integers(0, RUN, rn)
        return reorder(finish_cloud(points_in_cells(rng, cells, rdims, origin=ORIGIN_FAR), rdims, True, ORIGIN_FAR), rdims, order, ORIGIN_FAR)

    def run_contents(cloud, plan):
        b = bucket_of(cells_of(cloud, rdims, ORIGIN_FAR), plan["n_buckets"])
        return [("every point in one bucket of many", plan["n_buckets"] >= 256 and np.bincount(b).max() == rn and len(np.unique(b)) == 1)]
    for order in ORDERS:
        out.append(Case("C-one_run-%s" % order, "C", rdims, rn, lambda o=order: run_cloud(o),
                        claims=[("bucket form", rp["bucket_form"] and not rp["one_launch"])], contents=run_contents, far=True))
    return out


def _alias_buckets_cloud(seed, dims, n, K, dense=True):
    """Consecutive points cycle over the buckets whose numbers agree in the low 8 bits (bucket 5, 5 + 256, ...); a third of the
    cloud is a mixed background behind them."""
    rng = np.random.default_rng(seed)
    nc = n_cells_of(dims)
    m = (n - 2) * 2 // 3
    i = np.arange(m)
    group = np.arange(5, K, 256)
    b = group[i % len(group)]
    q = (i // (len(group) * 96)) % max(1, (nc >> 3) // K - 1)   # 96 rounds per row of runs: at least twelve points per cell
    cells = ((q * K + b) << 3) | ((i // len(group)) % RUN)
    assert cells.max() < nc
    cells = np.concatenate([cells, mixed_cells(rng, n - 2 - m, dims)])
    pad = np.zeros((1, 3), np.float32)
    return finish_cloud(np.concatenate([pad, points_in_cells(rng, cells, dims), pad]), dims, dense)


def _alias_locals_cloud(seed, dims, n, K, C):
    """Consecutive points alternate between local cells 256 apart inside one bucket; the bucket changes every 512 points."""
    rng = np.random.default_rng(seed)
    nc = n_cells_of(dims)
    m = (n - 2) * 2 // 3
    i = np.arange(m)
    b = 1 + (i // 512) % (K - 2)
    local = (i // (512 * (K - 2))) * 16 % 256 + (i % 2) * 256 + (i // 2) % RUN
    assert local.max() < C
    cells = cell_at(b, local, K)
    keep = cells < nc
    cells = np.concatenate([cells[keep], mixed_cells(rng, n - 2 - int(keep.sum()), dims)])
    pad = np.zeros((1, 3), np.float32)
    return finish_cloud(np.concatenate([pad, points_in_cells(rng, cells, dims), pad]), dims, True)


def group_c_alias():
    out = []
    n = 70000
    p = plan_of(BOX_A, n)

    def alias_contents(dims):
        def f(cloud, plan):
            b = bucket_of(cells_of(cloud, dims), plan["n_buckets"])[1:]
            same_low = (b[1:] & 255) == (b[:-1] & 255)
            return [("consecutive points in different buckets with equal low 8 bits", int((same_low & (b[1:] != b[:-1])).sum()) > len(b) // 2)]
        return f
    out.append(Case("C-alias_buckets-first_ballot_bit", "C", BOX_A, n, lambda: _alias_buckets_cloud(81, BOX_A, n, p["n_buckets"]),
                    claims=[("bucket form, one ballot bit", p["bucket_form"] and 256 < p["n_buckets"] <= 512)], contents=alias_contents(BOX_A)))
    # (the boxes of group B: the largest lattice of the bucket form, the first whose buckets are wider than a pass)
    bn = 50000
    bdims = (512, 256, first_dz(512, 256, lambda d: not plan_of(d, bn)["bucket_form"]) - 1)
    bp = plan_of(bdims, bn)
    out.append(Case("C-alias_buckets-every_ballot_bit", "C", bdims, bn,
                    lambda: _alias_buckets_cloud(82, bdims, bn, bp["n_buckets"]), voxel_index=1,
                    claims=[("bucket form, the most buckets", bp["bucket_form"] and bp["n_buckets"] == 8192)], contents=alias_contents(bdims)))

    class wide:
        n = 50000
        dims = (64, 64, first_dz(64, 64, lambda d: plan_of(d, 50000)["cells_per_bucket"] > plan_of(d, 50000)["wmax"]))
    wp = plan_of(wide.dims, wide.n)

    def local_contents(cloud, plan):
        cells = cells_of(cloud, wide.dims)[1:]
        b, l = bucket_of(cells, plan["n_buckets"]), local_of(cells, plan["n_buckets"])
        hit = (b[1:] == b[:-1]) & (np.abs(l[1:] - l[:-1]) % 256 == 0) & (l[1:] != l[:-1])
        return [("consecutive points in local cells 256 apart of one bucket", int(hit.sum()) > len(b) // 4)]
    out.append(Case("C-alias_locals", "C", wide.dims, wide.n,
                    lambda: _alias_locals_cloud(83, wide.dims, wide.n, wp["n_buckets"], wp["cells_per_bucket"]),
                    claims=[("buckets of more than 256 cells, wider than a pass", wp["cells_per_bucket"] > wp["wmax"] >= 512)], contents=local_contents))
    return out


def group_d():
    """Record compaction: 66 000 points over boxes of 60 x 60 x dz cells either side of every step of its tile plan."""
    n, out = 66000, []
    tile = lambda d: (plan_of(d, n)["compact_items"], plan_of(d, n)["compact_prefix"])
    zs = [dz for dz in range(2, 1100) if tile((60, 60, dz)) != tile((60, 60, dz - 1))]
    for i, dz in enumerate(zs):
        def case(d, seed):
            return lambda name: Case(name, "D", d, n, lambda: mixed_cloud(seed, n, d, True))
        out += _pair("D-tile_step%d" % (i + 1), "D", case((60, 60, dz - 1), 51 + 2 * i), case((60, 60, dz), 52 + 2 * i), lambda lo, hi, a, b: [
            ("the tile plan changes", (lo["compact_items"], lo["compact_prefix"]) != (hi["compact_items"], hi["compact_prefix"])),
            ("bucket form, compaction deferred", a.expect["form"] == b.expect["form"] == "buckets" and n > 65536)])
    return out, zs


def group_e():
    """The voxel filter's route: (name, dims, n, seed, claims)."""
    out = []
    P = lambda d, n: plan_of(d, n)
    b = steps(lambda n: P(BOX_A, n)["filter_buckets"], 100000, 200000)
    assert len(b) == 1
    n = b[0]
    out.append(("E-points-below", BOX_A, n - 1, 61, [("general chain", not P(BOX_A, n - 1)["filter_buckets"])]))
    out.append(("E-points-above", BOX_A, n, 62, [("bucket front end", P(BOX_A, n)["filter_buckets"])]))
    dz = first_dz(128, 128, lambda d: not P(d, n)["filter_buckets"])
    out.append(("E-cells_per_point-below", (128, 128, dz - 1), n, 63, [("bucket front end", P((128, 128, dz - 1), n)["filter_buckets"])]))
    out.append(("E-cells_per_point-above", (128, 128, dz), n, 64, [("general chain", not P((128, 128, dz), n)["filter_buckets"])]))
    dz = first_dz(64, 64, lambda d: P(d, n)["filter_chunks"] > 1)
    out.append(("E-one_chunk", (64, 64, dz - 1), n, 65, [("one chunk", P((64, 64, dz - 1), n)["filter_chunks"] == 1)]))
    out.append(("E-two_chunks", (64, 64, dz), n, 66, [("two chunks", P((64, 64, dz), n)["filter_chunks"] == 2)]))
    return out


_GROUPS = {}


def cases_of(group):
    """The cases of group A, B, C or D (made once per process: the searches cost a few thousand host calls)."""
    if group not in _GROUPS:
        _GROUPS[group] = dict(A=lambda: group_a()[0], B=group_b, C=lambda: group_c() + group_c_alias(), D=lambda: group_d()[0])[group]()
    return _GROUPS[group]


def all_cases():
    return {g: cases_of(g) for g in "ABCD"}


def run_bits_hold():
    """The dealing rule above assumes runs of eight cells: a plan's buckets then hold a multiple of eight cells, and a box of
    one run has a single occupied bucket (checked on the GPU through the results)."""
    p = plan_of(BOX_A, 60000)
    return p["cells_per_bucket"] % RUN == 0


# ---- the comparator -----------------------------------------------------------------------------------------------------
# Covariances, inverse covariances and eigenvalues of the dump against the oracle's: tools/fuzz_grid.py holds 1e-8 of the largest
# magnitude.  Over every case of this file, in every form of the build, the largest deviation measured against the oracle was
# 0 for cov and icov (bit for bit) and 1.44e-15 for the eigenvalues (NOTES.md, "Grid build at its plan boundaries"), so this
# file holds ten times that: cov and icov bit for bit, eigenvalues 1.5e-14.
GRID_REL = dict(cov=0.0, icov=0.0, evals=1.5e-14)


def grid_mismatch(a, b, min_pts=MIN_PTS, rel=GRID_REL):
    """None if grid a (under test) is grid b (the oracle's), else what differs: idx, n, min_b, div_b equal; mean bit for bit; cov /
    icov / evals of the voxels with min_pts points and more with the same finiteness pattern and within rel[k] of the largest
    magnitude (rel: GRID_REL, or one figure for all three -- tools/fuzz_grid.py's line is 1e-8)."""
    if not isinstance(rel, dict):
        rel = dict(cov=rel, icov=rel, evals=rel)
    for k in ("min_b", "div_b", "idx", "n"):
        if not np.array_equal(a[k], b[k]):
            return k + " differ"
    if not np.array_equal(a["mean"], b["mean"]):
        return "means not bit-exact (max %.3g)" % np.abs(a["mean"] - b["mean"]).max()
    ok = b["n"] >= min_pts
    for k in ("cov", "icov", "evals"):
        x, y = a[k][ok], b[k][ok]
        fin = np.isfinite(y)
        if not np.array_equal(fin, np.isfinite(x)):
            return k + " finiteness"
        if fin.any() and np.abs(x[fin] - y[fin]).max() > rel[k] * np.abs(y[fin]).max():
            return "%s differs (rel %.3g)" % (k, np.abs(x[fin] - y[fin]).max() / np.abs(y[fin]).max())
    return None


def grid_deviation(a, b, min_pts=MIN_PTS):
    ok = b["n"] >= min_pts
    out = {}
    for k in ("cov", "icov", "evals"):
        x, y = a[k][ok], b[k][ok]
        fin = np.isfinite(y) & np.isfinite(x)
        out[k] = float(np.abs(x[fin] - y[fin]).max() / np.abs(y[fin]).max()) if fin.any() else 0.0
    return out


def evals_identical(a, b):
    return a[0] == b[0] and a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def eval_deviation(a, b):
    """Largest relative deviation of score, gradient and Hessian of evaluation a from b (each against its largest magnitude)."""
    dev = 0.0
    for x, y in ((a[0], b[0]), (a[1], b[1]), (a[2], b[2])):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        dev = max(dev, float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-30)))
    return dev


def oracle_for(po, case_or_cloud, dense=True):
    o = po.OracleNDT(resolution=LEAF, min_points_per_voxel=MIN_PTS, num_threads=16)
    cloud = case_or_cloud.cloud() if isinstance(case_or_cloud, Case) else case_or_cloud
    dense = case_or_cloud.dense if isinstance(case_or_cloud, Case) else dense
    ov = o.set_target(cloud, is_dense=dense)
    assert not ov
    return o


def handle_for(ndt, case, voxel_index=None):
    g = ndt.NormalDistributionsTransform()
    g.setResolution(LEAF)
    g.setMinPointPerVoxel(MIN_PTS)
    g.setVoxelIndex(case.voxel_index if voxel_index is None else voxel_index)
    g.setInputTarget(case.cloud(), is_dense=case.dense)
    return g


def check_case(ndt, po, case, placed=True, eval_rel=2e-6):
    """Checks (a), (b), (c) of one case on the GPU -> (failures, report).  placed=False (a switched plan): the build must be what the
    host plan of this process says, but need not sit where the case is named for; it is held to the oracle all the same."""
    fails, rep = [], {}
    g = handle_for(ndt, case)
    gb = g.gridBuild()
    rep["build"] = gb
    for k, v in case.expect.items():
        if gb[k] != v:
            fails.append("gridBuild()[%r] = %r, the library's host plan says %r" % (k, gb[k], v))
    if placed:
        fails += ["claim does not hold: " + s for s, ok in case.claims if not ok]
    # (c) first: the dump below runs k_finalize over the leaf arrays with the grid's own record arrays as its output, so after
    # grid() the handle no longer holds the records the build wrote
    src = source_of(case.cloud())
    g.setInputSource(src)
    ev = g.eval(case.pose, True)
    o = oracle_for(po, case)
    og = o.grid()
    gg = g.grid()
    why = grid_mismatch(gg, og)
    if why:
        fails.append("grid against the oracle: " + why)
    else:
        rep["grid_dev"] = grid_deviation(gg, og)
    o.set_source(src)
    other_index = 1 if gb["form"] == "sparse" else 2
    g2 = handle_for(ndt, case, other_index)
    g2.setInputSource(src)
    rep["other_form"] = g2.gridBuild()["form"]
    if rep["other_form"] == gb["form"]:
        fails.append("the cross-check handle was built in the same form")
    if not evals_identical(ev, g2.eval(case.pose, True)):
        fails.append("evaluation sums differ between the %s and the %s build (records not identical)" % (gb["form"], rep["other_form"]))
    oe = o.eval(case.pose, True)
    rep["eval_dev"] = eval_deviation(ev, oe)
    if ev[3] != oe[3]:
        fails.append("neighbour count %r against the oracle's %r" % (ev[3], oe[3]))
    if not (rep["eval_dev"] <= eval_rel):
        fails.append("evaluation against the oracle: rel %.3g > %.3g" % (rep["eval_dev"], eval_rel))
    rep["valid"] = int((og["n"] >= MIN_PTS).sum())
    return fails, rep
