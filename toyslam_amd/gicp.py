"""Python host-side mirror of pclomp::GeneralizedIterativeClosestPoint over the C-ABI (include/gicp_mi355.h).

Method names follow the reference class (ndt_omp/include/pclomp/gicp_omp.h:52-378) and the
pcl::Registration methods its one caller uses (ndt_omp/apps/align.cpp:14-33,80-86).  All compute runs
in libndt_mi355.so on the GPU; nothing here falls back to numpy.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .ndt import _cloud, _colmajor, _d, _f, _from_colmajor, _i, pairs_array


class GeneralizedIterativeClosestPoint:
    """Drop-in shaped like pclomp::GeneralizedIterativeClosestPoint<PointT, PointT>."""

    def __init__(self, device=0):
        self._L = _lib.lib()
        h = C.c_void_p()
        check(self._L.gicp_create(device, C.byref(h)))
        self._h = h
        self._k = 20
        self._n = [0, 0]

    def __del__(self):
        try:
            self._L.gicp_destroy(self._h)
        except Exception:
            pass

    def setCorrespondenceRandomness(self, k):
        check(self._L.gicp_set_correspondence_randomness(self._h, int(k)))
        self._k = int(k)

    def setRotationEpsilon(self, eps):
        check(self._L.gicp_set_rotation_epsilon(self._h, float(eps)))

    def setMaximumOptimizerIterations(self, n):
        check(self._L.gicp_set_maximum_optimizer_iterations(self._h, int(n)))

    def setTransformationEpsilon(self, eps):
        check(self._L.gicp_set_transformation_epsilon(self._h, float(eps)))

    def setMaximumIterations(self, n):
        check(self._L.gicp_set_maximum_iterations(self._h, int(n)))

    def setMaxCorrespondenceDistance(self, d):
        check(self._L.gicp_set_max_correspondence_distance(self._h, float(d)))

    def setInputTarget(self, cloud):
        c = _cloud(cloud)
        self._map = None
        check(self._L.gicp_set_input_target(self._h, c.ctypes.data, c.shape[0], c.strides[0]))
        self._n[0] = c.shape[0]

    def setInputSource(self, cloud):
        c = _cloud(cloud)
        check(self._L.gicp_set_input_source(self._h, c.ctypes.data, c.shape[0], c.strides[0]))
        self._n[1] = c.shape[0]

    def setInputTargetCloud(self, dc):
        """setInputTarget from a cloud resident in HBM (ndt.DeviceCloud: uploadCloud, voxelGridFilterCloud*, ...): by
        reference, no download (gicp_set_input_target_cloud)."""
        self._n[0] = 0
        self._map = None
        check(self._L.gicp_set_input_target_cloud(self._h, dc._c))
        self._n[0] = len(dc)

    def setInputSourceCloud(self, dc):
        self._n[1] = 0
        check(self._L.gicp_set_input_source_cloud(self._h, dc._c))
        self._n[1] = len(dc)

    VOXEL_COV_MODES = {"plane": _lib.GICP_VOXEL_COV_PLANE, "raw": _lib.GICP_VOXEL_COV_RAW}

    def setInputTargetGrid(self, ndt, cov_mode="plane"):
        """setInputTarget from a voxel grid (gicp_set_input_target_grid): the target becomes the CURRENT target grid of the
        NormalDistributionsTransform `ndt` -- built from a cloud, or accumulated (targetAccumulate*) -- and every later call reads
        it as it is then; nothing is built over the map.  cov_mode: "plane" (I - (1 - epsilon) n n^T per voxel, recommended) or
        "raw" (the voxel's covariance).  The handle borrows `ndt` (a reference is kept here); None drops the binding."""
        self._n[0] = 0
        if ndt is None:
            check(self._L.gicp_set_input_target_grid(self._h, None, 0))
            self._map = None
            return
        mode = self.VOXEL_COV_MODES[cov_mode] if isinstance(cov_mode, str) else int(cov_mode)
        check(self._L.gicp_set_input_target_grid(self._h, ndt._h, mode))
        self._map = ndt

    def targetGridVoxels(self):
        """The voxel set D the next registration against the grid target would use (gicp_target_grid_voxels): ((n, 4) float32 of
        x, y, z, 1, (n, 3, 3) float64 covariances, (n,) int64 linear voxel indices), ascending index."""
        n = C.c_size_t(0)
        check(self._L.gicp_target_grid_voxels(self._h, None, None, None, 0, C.byref(n)))
        V = n.value
        xyz1 = np.zeros((max(V, 1), 4), dtype=np.float32)
        cov = np.zeros((max(V, 1), 3, 3))
        idx = np.zeros(max(V, 1), dtype=np.int64)
        check(self._L.gicp_target_grid_voxels(self._h, _f(xyz1), _d(cov), idx.ctypes.data_as(C.POINTER(C.c_int64)), V, C.byref(n)))
        return xyz1[:V].copy(), cov[:V].copy(), idx[:V].copy()

    def diagTargetGrid(self):
        """The grid target's bookkeeping (gicp_diag_target_grid): dict of refreshes (mark / scan / gather passes so far), voxels,
        excursion, correspond_blocks."""
        a = [C.c_size_t(0) for _ in range(3)]
        e = C.c_float(0.0)
        check(self._L.gicp_diag_target_grid(self._h, C.byref(a[0]), C.byref(a[1]), C.byref(e), C.byref(a[2])))
        return dict(refreshes=a[0].value, voxels=a[1].value, excursion=e.value, correspond_blocks=a[2].value)

    def alignPairsClouds(self, clouds, pairs=None, guesses=None, max_range=None):
        """GICP of (target, source) pairs of resident clouds (gicp_align_pairs_clouds): every named cloud indexed once, the
        k-NN covariances of all of them from one launch, then one registration per pair with this handle's parameters.
        clouds: list of ndt.DeviceCloud; pairs: (P, 2) cloud indices (target, source), None = the consecutive pairs (k-1, k);
        guesses: one 4x4 per pair or None; max_range: getFitnessScore's, None = no limit.  Returns a dict with one entry per
        pair: T (P, 4, 4), converged, iterations, correspondences, fitness."""
        return self._align_pairs(self._L.gicp_align_pairs_clouds, clouds, pairs, guesses, max_range)

    def alignPairsLockstep(self, clouds, pairs=None, guesses=None, max_range=None):
        """alignPairsClouds with the registrations advanced together (gicp_align_pairs_lockstep): per step one correspondence
        launch and one objective launch for all pairs in flight.  Same arguments, same return dict, same bits per pair."""
        return self._align_pairs(self._L.gicp_align_pairs_lockstep, clouds, pairs, guesses, max_range)

    def _align_pairs(self, call, clouds, pairs, guesses, max_range):
        P = pairs_array(len(clouds), pairs)
        n = P.shape[0]
        g = None
        if guesses is not None:
            g = np.ascontiguousarray(np.stack([_colmajor(x) for x in guesses])) if n else np.zeros((1, 16), np.float32)
            if n and g.shape[0] != n:
                raise ValueError("one guess per pair")
        m = max(n, 1)
        T = np.zeros((m, 16), dtype=np.float32)
        conv, it, corr = (np.zeros(m, dtype=np.int32) for _ in range(3))
        fit = np.zeros(m, dtype=np.float64)
        arr = (C.c_void_p * max(len(clouds), 1))(*[c._c for c in clouds])
        check(call(self._h, arr, len(clouds), _i(P) if n else None, n, _f(g) if g is not None else None,
                   float(np.finfo(np.float64).max if max_range is None else max_range), _f(T), _i(conv), _i(it), _i(corr), _d(fit)))
        self._pairs_n = {i: len(clouds[i]) for i in set(P.reshape(-1).tolist())}
        return dict(T=np.stack([_from_colmajor(T[k]) for k in range(n)]) if n else np.zeros((0, 4, 4), np.float32),
                    converged=conv[:n].astype(bool), iterations=it[:n].copy(), correspondences=corr[:n].copy(),
                    fitness=fit[:n].copy())

    def alignGuesses(self, guesses, max_range=None):
        """This handle's source onto its target from every guess (list of 4x4), all advanced together (gicp_align_guesses).
        Entry g of the returned dict -- T (G, 4, 4), converged, iterations, correspondences, fitness -- is what align(guess g),
        stats() and getFitnessScore(max_range) give; getFinalTransformation() and stats() are left as they were."""
        n = len(guesses)
        g = np.ascontiguousarray(np.stack([_colmajor(x) for x in guesses])) if n else np.zeros((1, 16), np.float32)
        m = max(n, 1)
        T = np.zeros((m, 16), dtype=np.float32)
        conv, it, corr = (np.zeros(m, dtype=np.int32) for _ in range(3))
        fit = np.zeros(m, dtype=np.float64)
        check(self._L.gicp_align_guesses(self._h, _f(g), n, float(np.finfo(np.float64).max if max_range is None else max_range),
                                         _f(T), _i(conv), _i(it), _i(corr), _d(fit)))
        return dict(T=np.stack([_from_colmajor(T[k]) for k in range(n)]) if n else np.zeros((0, 4, 4), np.float32),
                    converged=conv[:n].astype(bool), iterations=it[:n].copy(), correspondences=corr[:n].copy(),
                    fitness=fit[:n].copy())

    def diagLockstep(self):
        """What the last alignPairsLockstep / alignGuesses did: dict of steps, correspond_launches, functor_launches,
        max_members_in_step (gicp_diag_lockstep)."""
        a = [C.c_size_t(0) for _ in range(4)]
        check(self._L.gicp_diag_lockstep(self._h, *[C.byref(x) for x in a]))
        return dict(steps=a[0].value, correspond_launches=a[1].value, functor_launches=a[2].value, max_members_in_step=a[3].value)

    def pairsCovariances(self, c):
        """The k-NN covariances the last alignPairsClouds computed for cloud c: (n, 3, 3) (gicp_pairs_covariances)."""
        n = getattr(self, "_pairs_n", {}).get(int(c), 0)
        cov = np.zeros((max(n, 1), 3, 3))
        check(self._L.gicp_pairs_covariances(self._h, int(c), _d(cov)))
        return cov[:n]

    def diagPairs(self):
        """What the last alignPairsClouds did: dict of index_builds, knn_launches, knn_blocks (gicp_diag_pairs)."""
        a = [C.c_size_t(0) for _ in range(3)]
        check(self._L.gicp_diag_pairs(self._h, *[C.byref(x) for x in a]))
        return dict(index_builds=a[0].value, knn_launches=a[1].value, knn_blocks=a[2].value)

    def pairsTime(self):
        """Host wall clock of the last alignPairsClouds' two halves: dict of prepare_ms, register_ms (gicp_diag_pairs_time)."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        check(self._L.gicp_diag_pairs_time(self._h, C.byref(a), C.byref(b)))
        return dict(prepare_ms=a.value, register_ms=b.value)

    def setSourceCovariances(self, cov):
        """gicp_omp.h:165-168.  cov: (n, 3, 3) symmetric matrices, one per source point; None clears them."""
        c = None if cov is None else np.ascontiguousarray(cov, dtype=np.float64).reshape(-1, 9)
        check(self._L.gicp_set_source_covariances(self._h, None if c is None else _d(c), 0 if c is None else len(c)))

    def setTargetCovariances(self, cov):
        """gicp_omp.h:186-189."""
        c = None if cov is None else np.ascontiguousarray(cov, dtype=np.float64).reshape(-1, 9)
        check(self._L.gicp_set_target_covariances(self._h, None if c is None else _d(c), 0 if c is None else len(c)))

    def align(self, guess=None, want_cloud=False):
        g = None if guess is None else _colmajor(guess)
        T = np.zeros(16, dtype=np.float32)
        conv, it = C.c_int(0), C.c_int(0)
        out = np.zeros((self._n[1], 4), dtype=np.float32) if want_cloud else None
        check(self._L.gicp_align(self._h, None if g is None else _f(g), _f(T), C.byref(conv), C.byref(it),
                                 None if out is None else out.ctypes.data))
        return out

    def _result(self):
        T = np.zeros(16, dtype=np.float32)
        conv, it = C.c_int(0), C.c_int(0)
        check(self._L.gicp_get_result(self._h, _f(T), C.byref(conv), C.byref(it)))
        return _from_colmajor(T), bool(conv.value), it.value

    def hasConverged(self):
        return self._result()[1]

    def getFinalTransformation(self):
        return self._result()[0]

    def getFinalNumIteration(self):
        return self._result()[2]

    def getFitnessScore(self, max_range=np.finfo(np.float64).max):
        v = C.c_double(0.0)
        check(self._L.gicp_get_fitness_score(self._h, float(max_range), C.byref(v)))
        return v.value

    def stats(self):
        a = [C.c_int(0) for _ in range(4)]
        check(self._L.gicp_get_stats(self._h, *[C.byref(x) for x in a]))
        return {"n_f": a[0].value, "n_df": a[1].value, "n_fdf": a[2].value, "correspondences": a[3].value}

    # --- inspection (parity tests) ---
    def covariances(self, which, neighbors=False):
        n = self._n[which]
        if which == 0 and getattr(self, "_map", None) is not None:  # a grid target: one covariance per voxel of D
            v = C.c_size_t(0)
            check(self._L.gicp_target_grid_voxels(self._h, None, None, None, 0, C.byref(v)))
            n = v.value
        cov = np.zeros((n, 3, 3))
        if neighbors:
            idx = np.zeros((n, self._k), dtype=np.int32)
            d2 = np.zeros((n, self._k), dtype=np.float32)
            check(self._L.gicp_covariances(self._h, which, _d(cov), _i(idx), _f(d2)))
            return cov, idx, d2
        check(self._L.gicp_covariances(self._h, which, _d(cov), None, None))
        return cov

    PLAN_FIELDS = ("knn_blocks", "correspond_blocks", "functor_blocks", "server_blocks")

    def plan(self, n):
        """How the launchers cut n points into blocks (gicp_diag_plan): dict of knn_blocks, correspond_blocks,
        functor_blocks, server_blocks."""
        v = np.zeros(4, dtype=np.int32)
        check(self._L.gicp_diag_plan(self._h, int(n), _i(v)))
        return dict(zip(self.PLAN_FIELDS, (int(x) for x in v)))

    def step_correspond(self, guess=None, transformation=None):
        g = None if guess is None else _colmajor(guess)
        t = None if transformation is None else _colmajor(transformation)
        corr = np.zeros(self._n[1], dtype=np.int32)
        maha = np.zeros((self._n[1], 9), dtype=np.float32)
        m = C.c_int(0)
        check(self._L.gicp_step_correspond(self._h, None if g is None else _f(g), None if t is None else _f(t), _i(corr),
                                           _f(maha), C.byref(m)))
        return m.value, corr, maha

    def step_functor(self, mode, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        f = C.c_double(0.0)
        g = np.zeros(6)
        check(self._L.gicp_step_functor(self._h, int(mode), _d(x), C.byref(f), _d(g)))
        return f.value, g


def host_apply_state(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    T = np.zeros(16, dtype=np.float32)
    _lib.lib().gicp_host_apply_state(_d(x), _f(T))
    return _from_colmajor(T)
