"""The two users of the one team k-nearest search (ndt_search.hpp team_knn) against each other: the STATISTICAL outlier
value of a point is the mean distance to its K nearest OTHER points, and GICP's covariance pass finds the K + 1 nearest
points of the cloud, the query itself first at distance 0.  Both compute dist2_f32 over the same points, so

    neighborValues(cloud, mean_k=K)  ==  (sqrt(f64(d2[:, 1])) + ... + sqrt(f64(d2[:, K]))) / K      bit for bit,

d2 being the neighbour distances of g.covariances(0, neighbors=True) under setCorrespondenceRandomness(K + 1).  The clouds
hold distinct finite points (a duplicate would let the self-drop and the index tie rule pick differently); on exactly these
the oracle's kNN and the numpy restatement of the filter agree bit for bit as well -- the CPU test below."""
import numpy as np
import pytest

import outlier_cases as oc
from oracle import pyoracle as po

KS = (1, 8, 9, 20)
# clusters a few cells wide, 20 m apart, and single points between them: their neighbours are beyond every shell walk
CLUSTERS = oc.clustered((90, 1, 80, 1, 70, 1, 55, 2), seed=11, gap=20.0)


def clouds_of(K):
    """a partly filled and a just-overfull wave of eight teams, and the cloud whose isolated queries take the two-pass scan"""
    return {"n = K + 2": oc.surface(K + 2, 4000 + K, scale=2.0), "n = K + 9": oc.surface(K + 9, 4100 + K, scale=2.0), "clusters": CLUSTERS}


def mean_of_neighbours(d2, K):
    """the STATISTICAL value from GICP's ascending neighbour rows: column 0 is the query itself"""
    terms = np.sqrt(d2[:, 1:].astype(np.float64))
    assert terms.shape[1] == K
    return np.cumsum(terms, axis=1)[:, -1] / K  # (cumsum adds in order)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("K", KS)
def test_the_two_references_agree_on_these_clouds(K):
    for name, xyz in clouds_of(K).items():
        assert np.isfinite(xyz).all() and len(np.unique(xyz, axis=0)) == len(xyz), (K, name)
        idx, d2 = po.gicp_knn(xyz, xyz, K + 1)
        assert np.array_equal(idx[:, 0], np.arange(len(xyz))) and (d2[:, 0] == 0).all() and (d2[:, 1] > 0).all(), (K, name)
        assert same_bits(mean_of_neighbours(d2, K), oc.knn_mean_distances(xyz, K)), (K, name)


@pytest.fixture(scope="module")
def mods(built_lib):
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import gicp, ndt
    return ndt.NormalDistributionsTransform(), gicp.GeneralizedIterativeClosestPoint()


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_outlier_values_are_gicps_neighbour_distances(mods, K):
    n, g = mods
    g.setCorrespondenceRandomness(K + 1)
    for name, xyz in clouds_of(K).items():
        values, stats = n.neighborValues(n.uploadCloud(xyz), mean_k=K)
        scanned = n.outlierDiag()["scanned_queries"]
        g.setInputTarget(xyz)
        _, idx, d2 = g.covariances(0, neighbors=True)
        assert stats["n_finite"] == len(xyz) and d2.shape == (len(xyz), K + 1), (K, name)
        assert np.array_equal(idx[:, 0], np.arange(len(xyz))) and (d2[:, 0] == 0).all(), (K, name)
        want = mean_of_neighbours(d2, K)
        print(K, name, "scanned queries", scanned, "values that differ", int((values != want).sum()))
        assert same_bits(values, want), (K, name)
        if name == "clusters":
            assert scanned > 0, (K, name)
