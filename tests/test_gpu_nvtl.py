"""GPU: the nearest-voxel transformation likelihood (k_nvtl, k_nvtl_poses; ndt_calculate_nvtl, ndt_get_nvtl, ndt_nvtl_poses,
ndt_source_point_nvtl, ndt_diag_nvtl; alignMultistart(metric="nvtl"); map_sequence --nvtl).

Values are held to tests/nvtl_cases.py -- numpy written from the definition, pinned by tests/test_nvtl_cases.py -- at rel 1e-11
(every term is positive: no cancellation in the sums), the found counts exactly; and to each other BIT FOR BIT: pose g of
nvtlPoses, calculateNVTL of the oracle-moved cloud g and the reduction of sourcePointNVTL(P[g]) share the f32 transform, the
walk of the points and the reduction.  The two switches that are read once per process (NDT_K2_MAX_BLOCKS,
NDT_SCORE_POSES_CHUNK) are exercised in a child process each (tests/nvtl_child.py computes, this file compares)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import centroid_fitness_cases as cc
import nvtl_cases as nc
import nvtl_child as child
import score_poses_cases as spc
from conftest import ROOT
from test_gpu_centroid_fitness import app_settings
from test_gpu_pairs import build_app

pytestmark = pytest.mark.gpu

F = np.float32
REL = 1e-11
PLAN_SIZES = (1, 255, 256, 257, 1025)
PLAN_POSES = (spc.I_IDENTITY, spc.I_GOLDEN, 2, 3, 4, spc.I_YAW90, spc.I_FAR)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def close(got, want, rel=REL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all(np.abs(got - want) <= rel * np.abs(want)))


def worst(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.where(want != 0, np.abs(got - want) / np.abs(want), np.abs(got - want))
    return float(r.max()) if r.size else 0.0


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from oracle import pyoracle as po
    from toyslam_amd import _lib, ndt
    return ndt, po, _lib


class Scene:
    """The bundled pair under the four neighbour rules: a GPU handle, an oracle and the numpy reference per rule, and the
    reference's answers per (rule, source size, pose), computed once."""

    def __init__(self, mods, pair, golden):
        self.ndt, self.po, self._lib = mods
        self.t, self.s = pair
        self.P = spc.poses(golden)
        self.handles, self.grids, self.refs, self.clouds = {}, {}, {}, {}

    def handle(self, method):
        if method not in self.handles:
            g = self.ndt.NormalDistributionsTransform()
            g.setNeighborhoodSearchMethod(getattr(self.po, method))
            g.setInputTarget(self.t)
            self.handles[method] = g
        return self.handles[method]

    def grid(self, method):
        if method not in self.grids:
            o = self.po.OracleNDT(num_threads=16, search_method=getattr(self.po, method))
            o.set_target(self.t)
            o.set_source(self.s[:10])
            self.grids[method] = nc.Grid.of_oracle(o, method, self.t)
        return self.grids[method]

    def moved(self, n, k):
        """pcl::transformPointCloud(source[:n], pose k), by the oracle"""
        if (n, k) not in self.clouds:
            self.clouds[(n, k)] = spc.moved(self.po, self.s[:n], self.P[k])
        return self.clouds[(n, k)]

    def ref(self, method, n, k):
        """-> (L per point, NVTL, n_found) of source[:n] under pose k"""
        if (method, n, k) not in self.refs:
            self.refs[(method, n, k)] = self.grid(method).nvtl(self.moved(n, k))
        return self.refs[(method, n, k)]


@pytest.fixture(scope="module")
def scene(mods, pair, golden):
    return Scene(mods, pair, golden)


def check_poses(scene, method, n, which, got, found, identities=True):
    """got[j], found[j] = nvtlPoses of pose which[j] over source[:n] (the handle's current source): against the reference, and
    against calculateNVTL of the moved cloud and sourcePointNVTL's reduction (the same bits)."""
    g = scene.handle(method)
    for j, k in enumerate(which):
        ctx = "%s n=%d pose %d" % (method, n, k)
        L, want, want_found = scene.ref(method, n, k)
        print("%s: nvtl %.17g reference %.17g found %d/%d" % (ctx, got[j], want, found[j], n))
        assert close(got[j], want), ctx
        assert int(found[j]) == want_found, ctx
        if k == spc.I_FAR:
            assert got[j] == 0.0 and found[j] == 0, ctx
        if identities:
            one, one_found = g.calculateNVTL(scene.moved(n, k))
            assert same_bits([got[j]], [one]) and one_found == found[j], ctx + ": %r != calculateNVTL's %r" % (float(got[j]).hex(), float(one).hex())
            per_point, red, red_found = g.sourcePointNVTL(scene.P[k])
            assert same_bits([got[j]], [red]) and red_found == found[j], ctx + ": %r != sourcePointNVTL's %r" % (float(got[j]).hex(), float(red).hex())


# ------------------------------------------------------------------ whole source
@pytest.mark.parametrize("method", spc.METHODS)
def test_poses_match_the_reference_and_the_other_calls(scene, method):
    g = scene.handle(method)
    n = len(scene.s)
    g.setInputSource(scene.s)
    got, found = g.nvtlPoses(scene.P, counts=True)
    assert got.shape == found.shape == (spc.N_POSES,) and np.isfinite(got).all()
    if "NDT_K2_MAX_BLOCKS" not in os.environ and "NDT_SCORE_POSES_CHUNK" not in os.environ:
        assert g.nvtlLaunches() == (1, spc.N_POSES * g.evalPlan(n)["launch_blocks"])
    check_poses(scene, method, n, range(spc.N_POSES), got, found)
    assert all(got[k] > 0.0 and found[k] > 0 for k in spc.near_indices())
    if method == "DIRECT1":   # the divisor is exercised: some points have no neighbour, some have
        assert all(0 < found[k] < n for k in spc.near_indices())
    assert same_bits(g.nvtlPoses(scene.P), got)
    # the order of the poses is the order of the values; a single pose is its entry of the table
    perm = np.random.default_rng(11).permutation(spc.N_POSES)
    v, c = g.nvtlPoses([scene.P[k] for k in perm], counts=True)
    assert same_bits(v, got[perm]) and np.array_equal(c, found[perm])
    assert same_bits(g.nvtlPoses([scene.P[spc.I_GOLDEN]]), got[spc.I_GOLDEN:spc.I_GOLDEN + 1])


def test_get_nvtl_is_the_final_transformation_case(scene):
    g = scene.ndt.NormalDistributionsTransform()
    g.setInputTarget(scene.t)
    g.setInputSource(scene.s)
    before = g.getNVTL()                                          # before any align: the identity
    assert same_bits([before[0]], g.nvtlPoses([np.eye(4)])) and before[1] > 0
    g.align()
    T = g.getFinalTransformation()
    value, found = g.getNVTL()
    v, c = g.nvtlPoses([T], counts=True)
    assert same_bits([value], v) and found == c[0] and g.nvtlLaunches()[0] == 1
    per_point, red, red_found = g.sourcePointNVTL()               # no transform: the final transformation too
    assert same_bits([value], [red]) and red_found == found
    L, want, want_found = scene.grid("DIRECT7").nvtl(spc.moved(scene.po, scene.s, T))
    print("after align: nvtl %.17g reference %.17g found %d/%d (identity: %.6f)" % (value, want, found, len(scene.s), before[0]))
    assert close(value, want) and found == want_found and value > before[0]


# ------------------------------------------------------------------ per point
def hip_download(ptr, n):
    linked = [m.group(1) for m in re.finditer(r"(/\S*libamdhip64\.so[.\d]*)", open("/proc/self/maps").read()) if "/torch/" not in m.group(1)]
    hip = C.CDLL(linked[0] if linked else "libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(n, dtype=np.float64)
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("method", spc.METHODS)
def test_per_point_values(scene, method):
    g = scene.handle(method)
    ref = scene.grid(method)
    c = spc.spoiled(scene.s[:3000])                               # NaN / +inf / -inf rows and an absurdly far one
    bad = [len(c) // 3, len(c) // 2, len(c) - 1, len(c) // 5]
    g.setInputSource(c)
    assert g.sourcePointCount() == len(c)
    for k in (spc.I_IDENTITY, spc.I_GOLDEN, 3, spc.I_YAW90, spc.I_FAR):
        ctx = "%s pose %d" % (method, k)
        out, value, found = g.sourcePointNVTL(scene.P[k])
        L, want, want_found = ref.nvtl(spc.moved(scene.po, c, scene.P[k]))
        hit = L >= 0
        print("%s: found %d/%d nvtl %.17g reference %.17g worst per-point rel %.3g" % (ctx, found, len(c), value, want, worst(out[hit], L[hit])))
        assert out.shape == (len(c),) and found == want_found and int((out >= 0).sum()) == found, ctx
        assert np.array_equal(out == -1.0, ~hit) and np.all(out[~hit] == -1.0), ctx
        assert np.all(out[bad] == -1.0), ctx
        assert close(out[hit], L[hit]), ctx
        assert close(value, want), ctx
        if found:
            assert value == pytest.approx(float(np.mean(out[out >= 0])), rel=1e-12), ctx
        else:
            assert value == 0.0 and k == spc.I_FAR, ctx
        ptr, v2, f2 = g.sourcePointNVTL(scene.P[k], device=True)
        assert same_bits(hip_download(ptr, len(c)), out) and same_bits([v2], [value]) and f2 == found, ctx
        assert same_bits(g.nvtlPoses([scene.P[k]]), [value]), ctx


# ------------------------------------------------------------------ block plan
@pytest.mark.parametrize("n", PLAN_SIZES)
def test_values_at_the_block_plan_sizes(scene, n):
    """One point, one block less a lane, exactly, plus a lane, and a fifth block of one point."""
    for method in spc.METHODS:
        g = scene.handle(method)
        g.setInputSource(scene.s[:n])
        got, found = g.nvtlPoses([scene.P[k] for k in PLAN_POSES], counts=True)
        blocks = g.evalPlan(n)["launch_blocks"]
        if "NDT_K2_MAX_BLOCKS" not in os.environ:
            assert blocks == (n + 255) // 256
        assert g.nvtlLaunches() == (1, len(PLAN_POSES) * blocks)
        check_poses(scene, method, n, PLAN_POSES, got, found)
        g.calculateNVTL(scene.moved(n, spc.I_GOLDEN))
        assert g.nvtlLaunches() == (1, blocks)
        out, value, f = g.sourcePointNVTL(scene.P[spc.I_GOLDEN])
        assert g.nvtlLaunches() == (1, blocks)
        assert close(out[out >= 0], scene.ref(method, n, spc.I_GOLDEN)[0][out >= 0]) and int((out >= 0).sum()) == f


# ------------------------------------------------------------------ the switches read once per process
def run_child(mode, tmp_path, **env):
    out = tmp_path / (mode + ".json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nvtl_child.py"), mode, str(out)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    with open(out) as f:
        return json.load(f)


def unhex(v):
    return np.array([float.fromhex(x) for x in v])


def test_values_where_the_walk_is_strided(scene, tmp_path):
    """NDT_K2_MAX_BLOCKS=3: from 769 points a thread walks several points."""
    res = run_child("capped", tmp_path, NDT_K2_MAX_BLOCKS="3")
    for method in spc.METHODS:
        for n in child.CAPPED_SIZES:
            r = res["%s/%d" % (method, n)]
            assert r["plan_blocks"] == 3 and (r["launches"], r["blocks"]) == (1, 3 * len(child.POSES)), (method, n)
            got = unhex(r["poses"])
            check_poses(scene, method, n, child.POSES, got, r["found"], identities=False)
            assert same_bits(got, unhex(r["single"])) and r["single_found"] == r["found"], (method, n)
            assert same_bits(got, unhex(r["reduced"])), (method, n)
            for j, k in enumerate(child.POSES):
                out, L = unhex(r["per_point"][j]), scene.ref(method, n, k)[0]
                assert np.array_equal(out == -1.0, L == -1.0) and close(out[L >= 0], L[L >= 0]), (method, n, k)


def test_chunked_values_are_the_unchunked_ones(scene, tmp_path):
    """NDT_SCORE_POSES_CHUNK=2: five poses take three launches and give the bits of the one-launch call."""
    g = scene.handle("DIRECT7")
    g.setInputSource(scene.s)
    whole, found = g.nvtlPoses([scene.P[k] for k in child.POSES], counts=True)
    if "NDT_SCORE_POSES_CHUNK" not in os.environ:
        assert g.nvtlLaunches()[0] == 1
    r = run_child("chunked", tmp_path, NDT_SCORE_POSES_CHUNK="2")
    assert r["launches"] == 3 and r["blocks"] == len(child.POSES) * r["plan_blocks"]
    assert same_bits(unhex(r["poses"]), whole) and r["found"] == [int(x) for x in found]


# ------------------------------------------------------------------ target forms
def form_values(g, scene, src):
    """what a handle with a target returns for the plan poses, under every search method: values, counts, per-point bits"""
    out = []
    g.setInputSource(src)
    for method in spc.METHODS:
        g.setNeighborhoodSearchMethod(getattr(scene.po, method))
        v, c = g.nvtlPoses([scene.P[k] for k in PLAN_POSES], counts=True)
        pp = g.sourcePointNVTL(scene.P[spc.I_GOLDEN])
        cn = g.calculateNVTL(scene.moved(len(src), spc.I_GOLDEN))
        out.append((bits(v).tolist(), c.tolist(), bits(pp[0]).tolist(), float(pp[1]).hex(), pp[2], float(cn[0]).hex(), cn[1]))
    return out


def test_sparse_index_and_accumulated_targets_give_the_same_bits(scene):
    ndt = scene.ndt
    src = scene.s[:4000]
    scene.moved(len(src), spc.I_GOLDEN)

    def cloud_target(points, voxel_index):
        g = ndt.NormalDistributionsTransform()
        g.setVoxelIndex(voxel_index)
        g.setInputTarget(points)
        return g

    dense = form_values(cloud_target(scene.t, 1), scene, src)
    assert all(sum(c) > 0 for _, c, *_ in dense)
    assert form_values(cloud_target(scene.t, 2), scene, src) == dense, "the sparse voxel index"
    # the target accumulated in two halves: the cloud target of the concatenation
    half = len(scene.t) // 2
    for voxel_index in (1, 2):
        g = ndt.NormalDistributionsTransform()
        g.setVoxelIndex(voxel_index)
        g.targetAccumulate(scene.t[:half])
        g.targetAccumulate(scene.t[half:])
        assert form_values(g, scene, src) == dense, "accumulated, voxel index %d" % voxel_index
        # ... and after a crop that removes voxels: the cloud target of the points in the kept cells
        centre = scene.t[:, :3].mean(axis=0)
        lo, hi = centre - [12.0, 9.0, 50.0], centre + [10.0, 14.0, 50.0]
        g.targetAccumulateCrop(lo, hi)
        clo, chi = ndt.crop_cell_range(1.0, lo, hi)
        cells = cc.cells_of(scene.t, 1.0)
        kept = scene.t[((cells >= clo) & (cells <= chi)).all(axis=1)]
        assert 1000 < len(kept) < len(scene.t) - 1000
        cropped = form_values(g, scene, src)
        assert cropped != dense
        assert cropped == form_values(cloud_target(kept, voxel_index), scene, src), "cropped, voxel index %d" % voxel_index


# ------------------------------------------------------------------ edges and state
def result_bits(g):
    T, conv, it, tp = g._result()
    return T.tobytes(), conv, it, float(tp).hex(), tuple(sorted(g.stats().items())), g.scorePosesLaunches()


def test_edges_and_the_handles_state(scene):
    ndt, _lib = scene.ndt, scene._lib
    P = [scene.P[k] for k in PLAN_POSES]
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(scene.t)
    g.setInputSource(scene.s)
    g.align()
    g.scorePoses(P)
    state = result_bits(g)
    assert state[1] and state[2] > 0 and state[5][0] == 1

    def unchanged(ctx):
        assert result_bits(g) == state, ctx

    g.getNVTL()
    unchanged("getNVTL")
    g.nvtlPoses(P, counts=True)
    unchanged("nvtlPoses")
    g.calculateNVTL(scene.s[:500])
    unchanged("calculateNVTL")
    g.sourcePointNVTL()
    g.sourcePointNVTL(P[1], device=True)
    unchanged("sourcePointNVTL")
    g.nvtlLaunches()
    g.alignMultistart(P, 2, metric="nvtl")
    assert result_bits(g)[:4] == state[:4]                        # (alignGuesses' statistics follow a batch; the result stays)

    def nothing(h, n_source, launched):
        """every call on h finds nothing: (0.0, 0), -1.0 per point -- and leaves h's result, statistics and counters alone"""
        was = result_bits(h)
        v, c = h.nvtlPoses(P, counts=True)
        assert same_bits(v, np.zeros(len(P))) and not c.any() and result_bits(h) == was
        assert (h.nvtlLaunches()[0] > 0) == launched
        assert h.getNVTL() == (0.0, 0) and result_bits(h) == was
        out, value, found = h.sourcePointNVTL()
        assert out.shape == (n_source,) and np.all(out == -1.0) and (value, found) == (0.0, 0) and result_bits(h) == was
        ptr, value, found = h.sourcePointNVTL(P[1], device=True)
        assert (value, found) == (0.0, 0) and (n_source == 0 or np.all(hip_download(ptr, n_source) == -1.0))
        assert h.calculateNVTL(np.zeros((0, 3), F)) == (0.0, 0) and h.calculateNVTL(np.full((9, 3), np.nan, F)) == (0.0, 0)
        assert result_bits(h) == was

    # an empty grid: a target of 3 points at min_points_per_voxel 6 -- gridded like any other, every probe misses
    h = ndt.NormalDistributionsTransform()
    h.setInputTarget(np.array([[0, 0, 0], [10, 0, 0], [5, 5, 5]], F))
    assert h.grid_counts()["n_valid"] == 0
    h.setInputSource(scene.s[:300])
    nothing(h, 300, True)
    assert h.calculateNVTL(scene.s[:300]) == (0.0, 0)
    # a target of no points: nothing to launch
    h = ndt.NormalDistributionsTransform()
    h.setInputTarget(np.zeros((0, 3), F))
    h.setInputSource(scene.s[:300])
    nothing(h, 300, False)
    assert h.calculateNVTL(scene.s[:300]) == (0.0, 0)
    # a source of no points, an all-NaN source, an empty and an all-NaN cloud against a real target
    h = scene.handle("DIRECT7")
    h.setInputSource(np.zeros((0, 3), F))
    nothing(h, 0, False)
    h.setInputSource(np.full((700, 3), np.nan, F))
    nothing(h, 700, True)
    assert h.calculateNVTL(np.zeros((0, 3), F)) == (0.0, 0)
    assert h.calculateNVTL(np.full((700, 3), np.nan, F)) == (0.0, 0)
    # no target, then no source
    h = ndt.NormalDistributionsTransform()
    calls = (lambda: h.nvtlPoses(P), h.getNVTL, h.sourcePointNVTL, lambda: h.alignMultistart(P, 2, metric="nvtl"))
    for call in calls + (lambda: h.calculateNVTL(scene.s[:10]),):
        with pytest.raises(ndt.NdtError) as e:
            call()
        assert e.value.status == _lib.NDT_ERR_NO_INPUT
    h.setInputTarget(scene.t)
    for call in calls:
        with pytest.raises(ndt.NdtError) as e:
            call()
        assert e.value.status == _lib.NDT_ERR_NO_INPUT
    assert h.calculateNVTL(scene.s[:10])[1] > 0                   # (a cloud needs no source)


# ------------------------------------------------------------------ multistart by NVTL
def test_multistart_ranked_by_nvtl(scene):
    ndt = scene.ndt
    cand = scene.P + spc.far_poses(7)
    g = ndt.NormalDistributionsTransform()
    g.setInputTarget(scene.t)
    g.setInputSource(scene.s)
    values = g.nvtlPoses(cand)
    want_picked = spc.argsort_top(values, 4)
    assert list(ndt.host_pick_top(values, 4)) == list(want_picked) and want_picked[0] == spc.I_GOLDEN
    got = g.alignMultistart(cand, 4, metric="nvtl")
    assert list(got["picked"]) == list(want_picked)
    ref = g.alignGuesses([cand[k] for k in want_picked])
    assert got["T"].tobytes() == ref["T"].tobytes() and list(got["iterations"]) == list(ref["iterations"])
    assert list(got["converged"]) == list(ref["converged"]) and same_bits(got["trans_probability"], ref["trans_probability"])
    assert got["best"] == int(want_picked[int(np.nanargmax(got["trans_probability"]))])
    # the default metric is what it was
    by_score = g.alignMultistart(cand, 4)
    assert list(by_score["picked"]) == list(spc.argsort_top(g.scorePoses(cand), 4))
    assert by_score["T"].tobytes() == g.alignMultistart(cand, 4, metric="score")["T"].tobytes()


# ------------------------------------------------------------------ the app
def test_map_sequence_prints_the_nvtl(scene, reference_pcd, tmp_path):
    ndt = scene.ndt
    d = tmp_path / "pcd"
    d.mkdir()
    scans = []
    for k, path in enumerate(reference_pcd, 1):
        xyz, _ = ndt.pcd_read_xyz(path)
        scans.append(xyz)
        with open(path, "rb") as src, open(str(d / ("cloud_%d.pcd" % k)), "wb") as dst:
            dst.write(src.read())
    exe = build_app(tmp_path, "map_sequence")
    plain = subprocess.check_output([exe, "--scan-to-map", str(d)], text=True)
    flagged = subprocess.check_output([exe, "--scan-to-map", "--nvtl", str(d)], text=True)
    lines = [ln for ln in flagged.splitlines() if ln.startswith("nvtl: ")]
    assert len(lines) == 1 and "registrations 1" in flagged and "nvtl" not in plain
    timed = lambda ln: ln.startswith("time:") or ln.startswith("start-up") or " ms" in ln
    assert [ln for ln in plain.splitlines() if not timed(ln)] == [ln for ln in flagged.splitlines() if not timed(ln) and not ln.startswith("nvtl: ")]
    assert subprocess.run([exe, "--nvtl", str(d)], capture_output=True).returncode == 2           # goes with --scan-to-map
    # the same loop in Python, with the app's settings
    g = ndt.NormalDistributionsTransform()
    app_settings(g)
    want, prev = [], np.eye(4, dtype=F)
    for k, sc in enumerate(scans):
        dc, _ = g.voxelGridFilterCloud(sc, 0.5)
        if k == 0:
            g.targetAccumulateCloud(dc)
            continue
        g.setInputSourceCloud(dc)
        g.align(prev)
        want.append(g.getNVTL() + (g.sourcePointCount(),))
        if g.hasConverged():
            prev = g.getFinalTransformation().astype(F)
            g.targetAccumulateCloud(dc, prev)
    m = re.fullmatch(r"nvtl: (\S+) found (\d+)/(\d+)", lines[0])
    print("nvtl: app %s python %r" % (lines[0], want))
    assert m and float(m.group(1)) == pytest.approx(want[0][0], rel=1e-5)
    assert (int(m.group(2)), int(m.group(3))) == want[0][1:] and 0 < want[0][1] <= want[0][2]
