"""Inputs and the reference for the per-query tests of getFitnessScore's exact nearest-neighbour search
(tests/test_gpu_fitness_edges.py; the helpers' own tests: tests/test_fitness_cases.py).  numpy only, no GPU.

  nearest_d2   the reference: brute force in the kernel's arithmetic, f32 (dx*dx + dy*dy) + dz*dz, per query
  GridModel    a model of the grid geometry that CLASSIFIES a query (which shell of cells holds its true neighbour, is it
               inside the box, how far from a cell face) -- never the expected value
  *_case(s)    the generators: arrays plus the class of every query

A fitness value of a scan of ONE query is that query's squared nearest distance as f32, widened to f64: exact."""
import numpy as np

F = np.float32
DBL_MAX = float(np.finfo(np.float64).max)
K_TEAM_SHELLS = 2   # fitness_body: shells 0..2 by the query's team of 8 lanes, shells 3.. by the whole wave
K_KNN_MIN_RING = 3  # ndt_search.hpp: shells every query may try before one scan over all points


# ------------------------------------------------------------------------------------------------ the reference
def nearest_d2(target, queries, pairs_per_step=1 << 22):
    """(d2, arg): per query the smallest f32 (dx*dx + dy*dy) + dz*dz over the FINITE target points and the index (into
    `target`) of the first point that attains it; (inf, -1) for a query without a finite distance (no finite target point,
    a non-finite query).  A distance that overflows f32 is inf, as it is on the device."""
    t_all = np.ascontiguousarray(np.asarray(target)[:, :3], dtype=F)
    keep = np.nonzero(np.isfinite(t_all).all(axis=1))[0]
    t = t_all[keep]
    q = np.ascontiguousarray(np.asarray(queries)[:, :3], dtype=F)
    best = np.full(len(q), np.inf, dtype=F)
    arg = np.full(len(q), -1, dtype=np.int64)
    if len(t) == 0 or len(q) == 0:
        return best, arg
    qs = max(1, min(len(q), 4096))
    ts = max(1, pairs_per_step // qs)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, len(q), qs):
            qa = q[a:a + qs]
            b_best, b_arg = best[a:a + qs], arg[a:a + qs]  # views
            for c in range(0, len(t), ts):
                tc = t[c:c + ts]
                dx = qa[:, None, 0] - tc[None, :, 0]
                dy = qa[:, None, 1] - tc[None, :, 1]
                dz = qa[:, None, 2] - tc[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                assert d2.dtype == F
                d2[np.isnan(d2)] = np.inf  # (a non-finite query: no neighbour to report)
                k = d2.argmin(axis=1)
                m = d2[np.arange(len(qa)), k]
                upd = m < b_best  # strict: the first point wins a tie
                b_best[upd] = m[upd]
                b_arg[upd] = keep[c + k[upd]]
    return best, arg


def member_value(d2, max_range=DBL_MAX):
    """getFitnessScore of a scan whose queries have the squared nearest distances d2 (nearest_d2's): the f64 mean of those
    that are <= max_range, DBL_MAX if there is none."""
    d = np.asarray(d2, dtype=F).astype(np.float64)
    ok = d <= max_range  # (inf: a query without a neighbour, or a distance that overflowed f32)
    return float(d[ok].sum() / ok.sum()) if ok.any() else DBL_MAX


def one_point_values(d2, max_range=DBL_MAX):
    """The values of len(d2) members of one query each."""
    d = np.asarray(d2, dtype=F).astype(np.float64)
    return np.where(d <= max_range, d, DBL_MAX)


def se3_f32(T, xyz):
    """[PCL] Transformer<float>::se3 in f32, every product and sum rounded on its own: x*r0 + (y*r1 + (z*r2 + t)).  With a
    pure translation that is x + t."""
    T = np.asarray(T, dtype=F)
    x, y, z = (np.asarray(xyz)[:, i].astype(F) for i in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([x * T[i, 0] + (y * T[i, 1] + (z * T[i, 2] + T[i, 3])) for i in range(3)], axis=1).astype(F)


def translation(t):
    T = np.eye(4, dtype=F)
    T[:3, 3] = np.asarray(t, dtype=F)
    return T


def fitness_blocks(n):
    """The launch plan the tests assert against fitnessLaunches(): 32 query teams per block, at most 2048 blocks."""
    return max(1, min(2048, -(-n // 32)))


# ------------------------------------------------------------------------------------------------ the geometry model
class GridModel:
    """The cell space of a target's grid: min_b / max_b / div_b (from g.grid(), or from the points by the build's own rule:
    floor(min * inv_leaf), floor(max * inv_leaf) in f32) and the leaf (the resolution).  Classifies; is never the expected
    value."""

    def __init__(self, min_b, max_b, resolution):
        self.leaf = F(resolution)
        self.inv_leaf = F(1.0) / self.leaf
        self.min_b = np.asarray(min_b, dtype=np.int64)
        self.max_b = np.asarray(max_b, dtype=np.int64)
        self.div_b = self.max_b - self.min_b + 1

    @classmethod
    def from_grid(cls, grid, resolution):
        m = cls(grid["min_b"], grid["max_b"], resolution)
        assert np.array_equal(m.div_b, np.asarray(grid["div_b"], dtype=np.int64))
        return m

    @classmethod
    def from_points(cls, target, resolution):
        t = np.asarray(target)[:, :3].astype(F)
        t = t[np.isfinite(t).all(axis=1)]
        inv = F(1.0) / F(resolution)
        return cls(np.floor(t.min(axis=0) * inv), np.floor(t.max(axis=0) * inv), resolution)

    @property
    def r_lim(self):
        return int(self.div_b.max())

    def r_max(self, n_sorted):
        """max_shells: shells walked before the scan over all points."""
        by_cost = (int(np.sqrt(np.sqrt(F(2.0) * F(n_sorted)))) - 1) // 2
        return min(self.r_lim, max(K_KNN_MIN_RING, by_cost))

    @property
    def slack(self):
        """index_slack: what the shell bound gives away for the build-time / search-time index rounding."""
        max_abs = max(float(np.abs(self.min_b * float(self.leaf)).max()), float(np.abs((self.max_b + 1) * float(self.leaf)).max()))
        return 1e-3 * float(self.leaf) + 4e-6 * max_abs

    def box(self):
        """(lo, hi) corners of the cell space, f32."""
        return (self.min_b.astype(F) * self.leaf).astype(F), ((self.max_b + 1).astype(F) * self.leaf).astype(F)

    def point_cell(self, p):
        """The cell a target point was binned into: floor(x * inv_leaf) - min_b, f32."""
        p = np.asarray(p)[:, :3].astype(F)
        return (np.floor(p * self.inv_leaf) - self.min_b.astype(F)).astype(np.int64)

    def query_cell(self, q):
        """(cell clamped into the box, inside, margin): the search's floor(x / leaf), whether that cell is in the box, and for
        a query inside the distance to the nearest face of its cell (0 outside), as query_cell computes them."""
        q = np.asarray(q)[:, :3].astype(F)
        with np.errstate(over="ignore", invalid="ignore"):
            raw = np.nan_to_num(np.floor(q / self.leaf), nan=0.0, posinf=2.0 ** 31 - 1, neginf=-2.0 ** 31)
            raw = np.clip(raw, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
        cl = np.clip(raw, self.min_b, self.max_b)
        inside = (cl == raw).all(axis=1)
        f = (q - raw.astype(F) * self.leaf).astype(F)
        margin = np.maximum(np.minimum(f, self.leaf - f).min(axis=1), F(0.0))
        return cl - self.min_b, inside, np.where(inside, margin, F(0.0)).astype(F)

    def classify(self, target, queries, d2=None, arg=None):
        """dict per query: shell (Chebyshev cell distance from the query's clamped cell to its true neighbour's cell, -1
        without a neighbour), inside, margin, d2, arg."""
        if d2 is None:
            d2, arg = nearest_d2(target, queries)
        cell, inside, margin = self.query_cell(queries)
        shell = np.full(len(cell), -1, dtype=np.int64)
        has = arg >= 0
        if has.any():
            pc = self.point_cell(np.asarray(target)[arg[has]])
            shell[has] = np.abs(pc - cell[has]).max(axis=1)
        return dict(shell=shell, inside=inside, margin=margin, d2=d2, arg=arg, cell=cell)


def ulp_steps(x, k):
    """x moved by k f32 ulps (k may be negative or 0)."""
    x = np.asarray(x, dtype=F).copy()
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def surfaces(n, seed, extent):
    from toyslam_amd import clouds
    return clouds.target_surfaces(n, seed=seed, extent=extent)[:, :3].astype(F)


def spoil(q, every=7):
    """A copy of the queries with NaN / inf points among them (not counted by getFitnessScore)."""
    q = q.copy()
    q[every // 2::every] = np.nan
    q[1::2 * every + 1, 1] = np.inf
    q[4::3 * every + 2, 2] = -np.inf
    return q


# ------------------------------------------------------------------------------------------------ group 1: the launch plan
PLAN_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257,
              1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)
CAP_SIZES = (65535, 65536, 65537, 131073)  # 2048 blocks reached at 65 505 queries: the teams stride from 65 537 on
PLAN_RES = 1.0


def plan_target():
    return surfaces(2000, seed=41, extent=20.0)


def plan_queries(n, seed=42):
    """The first n of one fixed stream of queries in and around plan_target's box (so a prefix's reference is a slice)."""
    rng = np.random.default_rng(seed)
    m = max(CAP_SIZES)
    q = np.c_[rng.uniform(-13, 13, (m, 2)), rng.uniform(-3, 13, m)].astype(F)
    return q[:n].copy()


def plan_spoiled(n):
    """A third of the sizes carry NaN / inf source points."""
    return (PLAN_SIZES + CAP_SIZES).index(n) % 3 == 1


# ------------------------------------------------------------------------------------------------ group 2: the reduce
REDUCE_BLOCKS = (1, 2, 31, 32, 33, 127, 128, 129, 2047, 2048)


def reduce_members(seed=43):
    """Members (scans of plan_queries' stream) whose block counts are REDUCE_BLOCKS, shuffled, with empty and non-finite
    members between them -> (scans, blocks of each: an empty member has none; a member of non-finite points has the
    blocks of its size, which accept nothing)."""
    rng = np.random.default_rng(seed)
    pool = plan_queries(max(CAP_SIZES), seed=44)
    scans = []
    for b in REDUCE_BLOCKS:
        n = 32 * b - int(rng.integers(0, 32)) if b < 2048 else 65536  # any size of b blocks; 2048: at the cap
        a = int(rng.integers(0, len(pool) - n))
        scans.append(pool[a:a + n].copy())
    scans += [np.zeros((0, 3), F), np.full((5, 3), np.nan, F), np.zeros((0, 3), F), np.full((40, 3), np.inf, F)]
    order = rng.permutation(len(scans))
    scans = [scans[i] for i in order]
    return scans, [fitness_blocks(len(s)) if len(s) else 0 for s in scans]


# ------------------------------------------------------------------------------------------------ group 3: team -> wave
SLAB_RES = 1.0


def slab_target(seed=45):
    """A dense slab x in [0, 4) x [0, 20)^2, four points in every cell, plus one point near each far corner of [0, 20)^3:
    the box then holds 16 empty layers."""
    rng = np.random.default_rng(seed)
    ii, jj, kk = np.meshgrid(np.arange(4), np.arange(20), np.arange(20), indexing="ij")
    cells = np.stack([ii.ravel(), jj.ravel(), kk.ravel()], axis=1).astype(np.float64)
    pts = (np.repeat(cells, 4, axis=0) + rng.uniform(0.05, 0.95, (4 * len(cells), 3)))
    far = np.array([[19.5, y, z] for y in (0.5, 19.5) for z in (0.5, 19.5)])
    return np.concatenate([pts, far]).astype(F)


def handoff_queries(mask_bits, seed):
    """len(mask_bits) queries against slab_target: far (the nearest point is beyond the team's shells: shell >= 3, farther
    than any bound the team reaches) where the bit is set, near (found within shells 0..2 with room to spare) elsewhere."""
    rng = np.random.default_rng(seed)
    n = len(mask_bits)
    near = np.c_[rng.uniform(0.2, 3.8, n), rng.uniform(1, 19, (n, 2))]
    far = np.c_[rng.uniform(8, 12, n), rng.uniform(6, 14, (n, 2))]
    return np.where(np.asarray(mask_bits, dtype=bool)[:, None], far, near).astype(F)


def handoff_members():
    """256 scans of 8 queries: query j of member m is far iff bit j of m is set."""
    return [handoff_queries([(m >> j) & 1 for j in range(8)], seed=1000 + m) for m in range(256)]


def handoff_masks64(seed=46, count=6):
    rng = np.random.default_rng(seed)
    masks = [rng.integers(0, 2, 64) for _ in range(count - 2)]
    masks += [np.r_[np.zeros(63, int), 1], np.r_[1, np.zeros(63, int)]]  # one far query, in the last / first slot
    return masks


def is_far(model, cls):
    """Not finished by the team: neighbour's cell beyond shell 2 and farther than the largest bound of shell 2."""
    lim = (K_TEAM_SHELLS + 0.5) * float(model.leaf)
    return (cls["shell"] > K_TEAM_SHELLS) & (cls["d2"].astype(np.float64) > lim * lim)


def is_near(model, cls):
    """Finished by the team whatever the margin: found within shells 0..2, nearer than shell 2's bound less the slack."""
    lim = K_TEAM_SHELLS * float(model.leaf) - model.slack
    return (cls["shell"] <= K_TEAM_SHELLS) & (cls["d2"].astype(np.float64) <= 0.99 * lim * lim)


# ------------------------------------------------------------------------------------------------ group 4: the last shell
SHELL_RES = 1.0
SHELL_SIZES = (3280, 3281, 7320, 7321)  # either side of two steps of max_shells' cost term: asserted, not assumed


def by_cost_steps(lo=300, hi=20000):
    """Every n_sorted in [lo, hi] at which max_shells' cost term goes up, from the model of the code."""
    bc = lambda n: (int(np.sqrt(np.sqrt(F(2.0) * F(n)))) - 1) // 2
    return [n for n in range(lo + 1, hi + 1) if bc(n) != bc(n - 1)]


def shell_target(n, seed=47):
    """n points in two sheets of 12 x 12 cells, x in [0, 1) and x in [15, 16): what lies between is empty, so a query in
    x-cell k < 8 has its neighbour in shell k.  Every cell holds a point near its centre."""
    rng = np.random.default_rng(seed)
    jj, kk = np.meshgrid(np.arange(12), np.arange(12), indexing="ij")
    cells = np.concatenate([np.stack([np.full(144, x), jj.ravel(), kk.ravel()], axis=1) for x in (0, 15)]).astype(np.float64)
    centre = cells + 0.5 + rng.uniform(-0.1, 0.1, cells.shape)
    rest = cells[np.arange(n - len(cells)) % len(cells)] + rng.uniform(0.02, 0.98, (n - len(cells), 3))
    return np.concatenate([centre, rest]).astype(F)


def shell_queries(target, n_sorted, seed=48):
    """-> (queries, kind): kind names what each query was built as ("own", "shell1".."shell3", "rmax", "rmax+1", "exact",
    "face", "edge", "corner"); the tests classify them with the model and assert the classes are all there."""
    rng = np.random.default_rng(seed)
    model = GridModel.from_points(target, SHELL_RES)
    r_max = model.r_max(n_sorted)
    qs, kind = [], []

    def add(name, q):
        qs.append(np.atleast_2d(np.asarray(q, dtype=np.float64)))
        kind.extend([name] * len(qs[-1]))

    m = 24
    add("own", np.c_[np.full(m, 0.5), rng.integers(3, 9, (m, 2)) + 0.5] + rng.uniform(-0.02, 0.02, (m, 3)))
    for name, k in (("shell1", 1), ("shell2", 2), ("shell3", 3), ("rmax", r_max), ("rmax+1", r_max + 1)):
        add(name, np.c_[k + rng.uniform(0.3, 0.7, m), rng.uniform(3, 9, (m, 2))])
    add("exact", target[rng.choice(len(target), m, replace=False)])
    for k in (0, 1, 2, 4, 7):
        j = rng.integers(3, 9, (m // 3, 2)).astype(np.float64)
        add("face", np.c_[np.full(len(j), k), j + rng.uniform(0.2, 0.8, j.shape)])
        add("edge", np.c_[np.full(len(j), k), j[:, 0], j[:, 1] + rng.uniform(0.2, 0.8, len(j))])
        add("corner", np.c_[np.full(len(j), k), j])
    return np.concatenate(qs).astype(F), np.array(kind)


def rlim_target(L, seed=49):
    """Points in the two opposite corner cells of a box of L^3 cells (L = 1: one cell): r_lim = L."""
    rng = np.random.default_rng(seed + L)
    a = rng.uniform(0.1, 0.9, (3, 3))
    b = rng.uniform(0.1, 0.9, (3, 3)) + (L - 1)
    return np.concatenate([a, b]).astype(F)


def rlim_queries(L, n=300, seed=50):
    """Half in and around the box, half inside it."""
    rng = np.random.default_rng(seed + L)
    return np.concatenate([rng.uniform(-2.5, L + 2.5, (n // 2, 3)), rng.uniform(0, L, (n - n // 2, 3))]).astype(F)


# ------------------------------------------------------------------------------------------------ group 5: awkward targets
def around(target, n, seed, res):
    """n queries for any target: uniform over its box grown by half its size (at least three leaves), a tenth of them on
    target points, a tenth far outside."""
    rng = np.random.default_rng(seed)
    t = np.asarray(target)[:, :3].astype(np.float64)
    t = t[np.isfinite(t).all(axis=1)]
    lo, hi = t.min(axis=0), t.max(axis=0)
    grow = np.maximum(0.5 * (hi - lo), 3.0 * res)
    q = rng.uniform(lo - grow, hi + grow, (n, 3))
    k = n // 10
    q[:k] = t[rng.integers(0, len(t), k)]
    q[k:2 * k] = hi + rng.uniform(10, 300, (k, 3)) * res * rng.choice([-1.0, 1.0], (k, 3))
    return q.astype(F)


def awkward_cases():
    """-> list of (name, target, resolution, is_dense, queries)."""
    rng = np.random.default_rng(51)
    out = []

    def add(name, t, res=1.0, dense=True, n=250, q=None):
        t = np.asarray(t, dtype=F)
        out.append((name, t, res, dense, around(t, n, 52 + len(out), res) if q is None else np.asarray(q, dtype=F)))

    add("one_point", [[0.3, -1.2, 4.0]])
    add("two_points", [[0.3, -1.2, 4.0], [7.9, 3.1, 4.2]])
    add("three_coincident", [[1.5, 2.5, -0.5]] * 3)
    add("one_cell_res50", rng.uniform(5, 15, (500, 3)), res=50.0)
    add("line_x", np.c_[rng.uniform(0, 40, 200), np.full((200, 2), 0.5)])
    add("line_z", np.c_[np.full((200, 2), 0.5), rng.uniform(0, 40, 200)])
    add("plane", np.c_[rng.uniform(0, 30, (1500, 2)), np.full(1500, 0.5)])
    for c in (1, 15, 16, 17, 127, 128, 129):  # scan_run's step: 16 for a team of 8, 128 for the wave
        t = np.concatenate([rng.uniform(0.05, 0.95, (c, 3)), [[7.5, 7.5, 7.5]]])
        add("cell_of_%d" % c, t, q=np.concatenate([around(t, 200, 60 + c, 1.0), t]))  # every point is asked for: d = 0
    for n in (255, 256, 257):  # wave_nearest's step is 256 points; the queries sit mid-box, ten shells from any point
        t = np.concatenate([rng.uniform(0.05, 0.95, (n - 1, 3)), [[24.5, 24.5, 24.5]]])
        q = np.concatenate([rng.uniform(9, 16, (180, 3)), around(t, 60, 70 + n, 1.0)])
        add("scan_all_%d" % n, t, q=q)
    base = surfaces(1500, seed=53, extent=10.0)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3], dtype=F)
    add("nan_front", np.concatenate([np.tile(bad, (10, 1)), base]), dense=False)
    add("nan_back", np.concatenate([base, np.tile(bad, (10, 1))]), dense=False)
    sc = base.copy()
    sc[3::17] = np.nan
    sc[5::29, 1] = np.inf
    add("nan_scattered", sc, dense=False)
    add("doubled", np.concatenate([base, base]))
    far = (base.astype(np.float64) + 1e5).astype(F)
    add("100km", far)
    return out


# ------------------------------------------------------------------------------------------------ group 6: cell faces
FACE_RESOLUTIONS = (0.1, 0.3, 1.0, 1.0 / 3.0)
FACE_OFFSETS = ("0", "+ulp", "-ulp", "+0.4", "-0.4", "+0.6", "-0.6")


def face_tables(res):
    """(base, vals, table): k * res for k = -2..2; those and their two f32 neighbours (15 values); table[o] = vals moved by
    FACE_OFFSETS[o]."""
    r = F(res)
    base = (np.arange(-2, 3).astype(F) * r).astype(F)
    vals = np.concatenate([ulp_steps(base, -1), base, ulp_steps(base, 1)])
    offs = [vals, ulp_steps(vals, 1), ulp_steps(vals, -1), (vals + F(0.4) * r).astype(F), (vals - F(0.4) * r).astype(F),
            (vals + F(0.6) * r).astype(F), (vals - F(0.6) * r).astype(F)]
    return base, vals, np.stack(offs)


def face_case(res, seed=54, n_queries=1500):
    """-> (target, queries, on_face): target points at every combination of k * res and one f32 ulp either side of it,
    k = -2..2 per axis; queries at such coordinates +- {0, 1 ulp, 0.4 res, 0.6 res} per axis (a seeded choice of the
    combinations, and every 'same offset on all axes' one).  on_face[i]: query i has a coordinate exactly on k * res."""
    rng = np.random.default_rng(seed)
    base, vals, table = face_tables(res)  # 15 values per axis, 7 offsets
    target = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), axis=-1).reshape(-1, 3).astype(F)
    same = np.stack([np.stack([table[o, v]] * 3) for o in range(7) for v in range(15)])  # (105, 3)
    o = rng.integers(0, 7, (n_queries - len(same), 3))
    o[::2] = rng.integers(0, 3, o[::2].shape)  # every other one on or an ulp off a face on all three axes
    v = rng.integers(0, 15, (n_queries - len(same), 3))
    q = np.concatenate([same, table[o, v]]).astype(F)
    on_face = np.isin(q, base).any(axis=1)
    return target, q, on_face


MISBINNED_RESOLUTIONS = (0.1, 0.3, 1.0 / 3.0)


def misbinned_case(res, k0=3000, sites=48):
    """Target points that sit OUTSIDE the cell they are binned into, with queries only the slack of the shell search saves.
    About a kilometre from the origin one f32 ulp is a few 1e-5 m, and for many k the point one ulp below the face k * leaf is
    binned into cell k (floor(x * inv_leaf), the product rounded up to k).  Per site: P, such a point; Q, in cell k - 1, a third
    of a leaf below the face; R, in Q's own cell, at a distance between |QP| and Q's distance to cell k's box.  After shell 0
    the bound is |QR|^2; cell k's box is farther than that, its point P is nearer.
    -> (target [P0, R0, P1, R1, ..], queries, gap2): gap2[i] = the squared f32 distance from query i to cell k's box."""
    leaf = F(res)
    inv = F(1.0) / leaf
    tgt, qs, gap2 = [], [], []
    k, last = k0, k0
    while len(qs) < sites:
        k += 1
        assert k < k0 + 4000
        lo = F(F(k) * leaf)
        p = np.nextafter(lo, F(-np.inf))
        if k < last + 5 or np.floor(F(p * inv)) != F(k):
            continue  # sites five cells apart at least; a face that bins its lower neighbour below has no such point
        last = k
        qx = F(lo - F(0.33) * leaf)
        y = F(F(0.5) * leaf)
        gap = F(lo - qx)                          # axis_gap without the slack
        d_p = float(p) - float(qx)                # exact: both are f32 of the same binade
        assert 0 < d_p < float(gap)
        b = F(0.5 * (d_p + float(gap)))
        tgt += [[p, y, y], [qx, F(y + b), y]]
        qs.append([qx, y, y])
        gap2.append(F(gap * gap))
    return np.array(tgt, dtype=F), np.array(qs, dtype=F), np.array(gap2, dtype=F)


# ------------------------------------------------------------------------------------------------ group 7: outside the box
OUTSIDE_DISTANCES = ("ulp", 0.5, 10.0, 1e4, 1e6, 1e9)  # in leaves of 1 m
DIRECTIONS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


def outside_queries(model, seed=55):
    """-> (queries, direction index, distance index; -1 for the overflow query): from the box's faces outwards along each
    axis, each edge and corner diagonal (all 26 directions, so every octant), at every distance of OUTSIDE_DISTANCES; last,
    one query 1e20 m away, whose squared distance overflows f32."""
    rng = np.random.default_rng(seed)
    lo, hi = model.box()
    qs, di, ki = [], [], []
    for d_i, d in enumerate(DIRECTIONS):
        for k_i, dist in enumerate(OUTSIDE_DISTANCES):
            q = rng.uniform(lo + 1, hi - 1).astype(F)  # the coordinates the direction leaves alone: inside
            for ax in range(3):
                if d[ax] == 0:
                    continue
                edge = hi[ax] if d[ax] > 0 else lo[ax]
                q[ax] = ulp_steps(edge, d[ax]) if dist == "ulp" else F(edge + F(d[ax] * dist * float(model.leaf)))
            qs.append(q)
            di.append(d_i)
            ki.append(k_i)
    qs.append(np.array([1e20, 0.0, 0.0], dtype=F))
    di.append(-1)
    ki.append(-1)
    return np.array(qs, dtype=F), np.array(di), np.array(ki)


# ------------------------------------------------------------------------------------------------ group 8: the build forms
FORMS_RES = 1.0


def forms_targets():
    """(small, large): about 3000 points (the one-launch build) and about 60 000 (above it: the bucket form)."""
    return surfaces(3000, seed=56, extent=20.0), surfaces(60000, seed=57, extent=40.0)


def forms_queries(target, seed=58):
    """About 1500 queries of the classes of groups 4 to 7 for any target: in and around the box, on target points, on cell
    faces / edges / corners and an ulp off them, in empty parts of the box, and outside at every distance."""
    rng = np.random.default_rng(seed)
    model = GridModel.from_points(target, FORMS_RES)
    lo, hi = (x.astype(np.float64) for x in model.box())
    t = np.asarray(target, dtype=np.float64)
    parts = [around(target, 500, seed + 1, FORMS_RES).astype(np.float64),
             t[rng.choice(len(t), 100, replace=False)],
             rng.uniform(lo, hi, (350, 3))]
    on = np.floor(rng.uniform(lo, hi, (390, 3)))  # cell corners; then faces and edges, then an ulp off
    on[130:260, 2] += rng.uniform(0.1, 0.9, 130)
    on[260:, 1:] += rng.uniform(0.1, 0.9, (130, 2))
    on = on.astype(F)
    parts += [on[0::3], ulp_steps(on[1::3], 1), ulp_steps(on[2::3], -1)]
    parts.append(outside_queries(model, seed + 2)[0])
    return np.concatenate([np.asarray(p, dtype=F) for p in parts]).astype(F)
