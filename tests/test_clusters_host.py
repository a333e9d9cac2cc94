"""CPU: the cluster entries (ndt_cloud_cluster, ndt_cloud_extract_clusters, ndt_cloud_extract_clusters_clouds, ndt_diag_clusters,
ndt_host_cluster_spec_check, ndt_host_cluster_plan) -- declared, exported and wrapped; the validity of a spec at each bound; the
link kernel's plan at its boundaries; every refusal done before any device work, with its outputs untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cluster_cases as cc
from conftest import ROOT

NEW = ("ndt_cloud_cluster", "ndt_cloud_extract_clusters", "ndt_cloud_extract_clusters_clouds", "ndt_diag_clusters",
       "ndt_host_cluster_spec_check", "ndt_host_cluster_plan")
SENTINEL = 0x5A5A5A5A
NAN, INF = float("nan"), float("inf")
BIG = 2 ** 31 - 1


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def spec_of(_lib, tolerance=0.5, min_size=1, max_size=BIG):
    return _lib.ClusterSpec(tolerance, min_size, max_size)


def invalid_specs(_lib):
    bad = [dict(tolerance=t) for t in (0.0, -0.0, -1.0, NAN, INF, -INF)]
    bad += [dict(min_size=0), dict(min_size=-1), dict(min_size=-BIG - 1), dict(min_size=5, max_size=4), dict(min_size=1, max_size=0),
            dict(min_size=BIG, max_size=BIG - 1), dict(min_size=2, max_size=-3)]
    return [spec_of(_lib, **b) for b in bad]


def test_entries_are_declared_exported_and_wrapped(mods):
    L, _lib, ndt = mods
    with open(os.path.join(ROOT, "include", "ndt_mi355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\(" % name, header), name + " is not declared in include/ndt_mi355.h"
    g = ndt.NormalDistributionsTransform
    for method in ("clusterSpec", "clusterCloud", "extractClusters", "extractClustersClouds", "diagClusters", "clusterPlan", "clusterSpecCheck"):
        assert callable(getattr(g, method))
    assert C.sizeof(_lib.ClusterSpec) == 12 and _lib.ClusterSpec.max_size.offset == 8
    assert C.sizeof(_lib.ClusterInfo) == 64 and _lib.ClusterInfo.first.offset == 8 and _lib.ClusterInfo.box_min.offset == 12
    assert _lib.ClusterInfo.box_max.offset == 24 and _lib.ClusterInfo.centroid.offset == 40
    assert C.sizeof(_lib.ClusterSummary) == 40 and _lib.ClusterSummary.largest.offset == 32
    # the wrapper's table and the reference's are the C struct, field by field
    for dt in (g.CLUSTER_DTYPE, cc.CLUSTER_DTYPE):
        assert dt.itemsize == 64 and [dt.fields[f][1] for f in ("root", "size", "first", "box_min", "box_max", "centroid")] == [0, 4, 8, 12, 24, 40]
    section = re.sub(r"[\s*]+", " ", header[header.index("Euclidean cluster extraction"):header.index("accumulating target: posed scans")])
    assert "no bit parity with pcl" in section.lower() and "the definitions below are the contract" in section


def test_spec_check_at_each_bound(mods):
    L, _lib, ndt = mods
    check = ndt.NormalDistributionsTransform.clusterSpecCheck
    for s in invalid_specs(_lib):
        assert not check(s), (s.tolerance, s.min_size, s.max_size)
    assert L.ndt_host_cluster_spec_check(None) == _lib.NDT_ERR_INVALID
    for ok in (spec_of(_lib), spec_of(_lib, 1e-30, 1, 1), spec_of(_lib, 3e38, BIG, BIG), spec_of(_lib, float(np.nextafter(np.float32(0), np.float32(1))), 7, 7),
               spec_of(_lib, 0.5, 1, BIG), spec_of(_lib, 0.5, 10, 11)):
        assert check(ok), (ok.tolerance, ok.min_size, ok.max_size)
    g = ndt.NormalDistributionsTransform
    s = g.clusterSpec(0.5, 10)
    assert (s.tolerance, s.min_size, s.max_size) == (0.5, 10, BIG) and check(s)
    s = g.clusterSpec(0.1, 3, 90)
    assert (s.tolerance, s.min_size, s.max_size) == (float(np.float32(0.1)), 3, 90) and check(s)
    assert not check(g.clusterSpec(0.5, 0)) and not check(g.clusterSpec(0.5, 4, 3))


def test_plan_at_its_boundaries(mods):
    L, _lib, ndt = mods
    assert "NDT_CLUSTER_MAX_BLOCKS" not in os.environ
    plan = ndt.NormalDistributionsTransform.clusterPlan
    team, cap = 8, 4096
    assert plan(0) == (0, 0)
    for n, want in ((1, (1, 8)), (7, (1, 8)), (8, (1, 8)), (9, (2, 8)), (16, (2, 8)), (17, (3, 8)), (64, (8, 8)), (65, (9, 8)),
                    (team * cap - 1, (cap, 8)), (team * cap, (cap, 8)), (team * cap + 1, (cap, 16)), (2 * team * cap, (cap, 16)),
                    (2 * team * cap + 1, (cap, 24)), (2 ** 31 - 1, (cap, 8 * -(-(2 ** 28) // cap)))):
        assert plan(n) == want, (n, plan(n), want)
    for n in list(range(1, 70)) + [team * cap + d for d in range(-9, 10)] + [100000, 2000000, 2 ** 31 - 1]:
        blocks, qpb = plan(n)
        passes = -(-n // team)
        # block b takes the passes b, b + blocks, ...: every pass is taken, no block is idle, and qpb is the busiest block's share
        assert 1 <= blocks <= cap and blocks == min(passes, cap) and qpb == team * -(-passes // blocks)
    b, q = C.c_int(-3), C.c_int(-3)
    assert L.ndt_host_cluster_plan(2 ** 31, C.byref(b), C.byref(q)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_cluster_plan(5, None, C.byref(q)) == _lib.NDT_ERR_INVALID
    assert L.ndt_host_cluster_plan(5, C.byref(b), None) == _lib.NDT_ERR_INVALID
    assert (b.value, q.value) == (-3, -3)


class Args:
    """sentinel-filled outputs of the three device entries"""

    def __init__(self, _lib, n=4):
        self.out = C.c_void_p(SENTINEL)
        self.outs = (C.c_void_p * n)(*([SENTINEL] * n))
        self.idx = np.full(n, -7, np.int32)
        self.labels = np.full(n, -7, np.int32)
        self.roots = np.full(n, -7, np.int32)
        self.table = np.full(n * 16, -7, np.int32)  # n rows of 64 bytes
        self.n_kept = C.c_size_t(SENTINEL)
        self.n_kepts = (C.c_size_t * n)(*([SENTINEL] * n))
        self.sums = (_lib.ClusterSummary * n)()
        self._lib = _lib
        for s in self.sums:
            s.n_finite = s.n_components = s.n_clusters = s.n_clustered = s.largest = SENTINEL

    def p32(self, a):
        return a.ctypes.data_as(C.POINTER(C.c_int32))

    def table_p(self):
        return self.table.ctypes.data_as(C.POINTER(self._lib.ClusterInfo))

    def untouched(self, out_null=False, outs_null=0):
        return ((self.out.value is None if out_null else self.out.value == SENTINEL)
                and all(self.outs[k] is None for k in range(outs_null)) and all(self.outs[k] == SENTINEL for k in range(outs_null, len(self.outs)))
                and all((a == -7).all() for a in (self.idx, self.labels, self.roots, self.table)) and self.n_kept.value == SENTINEL
                and all(v == SENTINEL for v in self.n_kepts)
                and all((s.n_finite, s.n_components, s.n_clusters, s.n_clustered, s.largest) == (SENTINEL,) * 5 for s in self.sums))


def test_refusals_leave_the_outputs_untouched(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    ok = spec_of(_lib)
    # ndt_cloud_cluster: NULL handle / in / spec / labels, NULL clusters with a capacity
    for h, spec_p, labels, table in ((None, C.byref(ok), True, True), (g._h, C.byref(ok), True, True), (g._h, None, True, True),
                                     (g._h, C.byref(ok), False, True), (g._h, C.byref(ok), True, False)):
        a = Args(_lib)
        st = L.ndt_cloud_cluster(h, None, spec_p, C.c_void_p(a.labels.ctypes.data) if labels else None, 0, C.c_void_p(a.roots.ctypes.data),
                                 a.table_p() if table else None, 4, a.p32(a.idx), a.sums)
        assert st == _lib.NDT_ERR_INVALID and a.untouched()
    # ndt_cloud_extract_clusters: NULL handle / out / in
    a = Args(_lib)
    assert L.ndt_cloud_extract_clusters(None, None, C.byref(ok), 0, C.byref(a.out), a.p32(a.idx), C.byref(a.n_kept), a.sums) == _lib.NDT_ERR_INVALID
    assert a.untouched(out_null=True)
    a = Args(_lib)
    assert L.ndt_cloud_extract_clusters(g._h, None, C.byref(ok), 0, None, a.p32(a.idx), C.byref(a.n_kept), a.sums) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    for negate in (0, 1):
        a = Args(_lib)
        assert L.ndt_cloud_extract_clusters(g._h, None, C.byref(ok), negate, C.byref(a.out), a.p32(a.idx), C.byref(a.n_kept), a.sums) == _lib.NDT_ERR_INVALID
        assert a.untouched(out_null=True)
    # ndt_cloud_extract_clusters_clouds: NULL handle / out / in / spec / entry, too many clouds, an invalid spec
    null_entries = (C.c_void_p * 4)()
    a = Args(_lib)
    assert L.ndt_cloud_extract_clusters_clouds(None, null_entries, 4, C.byref(ok), 0, a.outs, a.n_kepts, a.sums) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    assert L.ndt_cloud_extract_clusters_clouds(g._h, null_entries, 4, C.byref(ok), 0, None, a.n_kepts, a.sums) == _lib.NDT_ERR_INVALID
    assert a.untouched()
    assert L.ndt_cloud_extract_clusters_clouds(g._h, null_entries, 65536, C.byref(ok), 0, a.outs, a.n_kepts, a.sums) == _lib.NDT_ERR_INVALID
    assert a.untouched()                        # (refused before the 65 536 outputs it does not have are written)
    for spec_p, in_p in ((C.byref(ok), None), (None, null_entries), (C.byref(ok), null_entries)):
        a = Args(_lib)
        assert L.ndt_cloud_extract_clusters_clouds(g._h, in_p, 4, spec_p, 1, a.outs, a.n_kepts, a.sums) == _lib.NDT_ERR_INVALID
        assert a.untouched(outs_null=4)
    for bad in invalid_specs(_lib):
        a = Args(_lib)
        assert L.ndt_cloud_extract_clusters_clouds(g._h, null_entries, 0, C.byref(bad), 0, a.outs, a.n_kepts, a.sums) == _lib.NDT_ERR_INVALID
        assert a.untouched()
        assert L.ndt_cloud_extract_clusters_clouds(g._h, null_entries, 4, C.byref(bad), 0, a.outs, a.n_kepts, a.sums) == _lib.NDT_ERR_INVALID
        assert a.untouched(outs_null=4)
    n = C.c_size_t(SENTINEL)
    assert L.ndt_diag_clusters(None, *([C.byref(n)] * 5)) == _lib.NDT_ERR_INVALID
    for hole in range(5):
        ptrs = [C.byref(n)] * 5
        ptrs[hole] = None
        assert L.ndt_diag_clusters(g._h, *ptrs) == _lib.NDT_ERR_INVALID and n.value == SENTINEL


def test_no_clouds_is_ok_without_a_device(mods):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    a = Args(_lib)
    assert L.ndt_cloud_extract_clusters_clouds(g._h, None, 0, C.byref(spec_of(_lib)), 0, a.outs, a.n_kepts, a.sums) == _lib.NDT_OK
    assert a.untouched()
    assert g.extractClustersClouds([], 0.5, 10) == ([], [])
    assert g.diagClusters() == dict(index_builds=0, launches=0, link_blocks=0, scanned_queries=0, cas_retries=0)
    assert g.selectDiag() == dict(launches=0, blocks=0, clouds=0)
    assert g.outlierDiag() == dict(index_builds=0, value_launches=0, value_blocks=0, scanned_queries=0)


def test_device_calls_need_a_device(mods):
    L, _lib, ndt = mods
    if L.ndt_device_count() > 0:
        return  # (with a device no cloud-free call gets past the argument checks: tests/test_gpu_clusters.py takes over)
    g = ndt.NormalDistributionsTransform()
    with pytest.raises(ndt.NdtError) as e:
        g.uploadCloud(np.zeros((3, 3), np.float32))  # no cloud can exist here, so the single-cloud entries have nothing to take
    assert e.value.status == _lib.NDT_ERR_NO_DEVICE
