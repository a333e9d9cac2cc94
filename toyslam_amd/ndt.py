"""Python host-side mirror of pclomp::NormalDistributionsTransform over the C-ABI.

Method names follow the reference class (ndt_omp/include/pclomp/ndt_omp.h:70-502
and the pcl::Registration methods its callers use) so that tests read like the
reference's call sites (ndt_omp/apps/align.cpp:14-33,
lidar_subscriber/src/ndt_omp_mapping_node.cpp:151-169).  All compute happens in
libndt_mi355.so on the GPU; nothing here falls back to numpy.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import COMM_ID_BYTES, DIRECT1, DIRECT7, DIRECT26, KDTREE, NdtError, check  # noqa: F401


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _cloud(a):
    """(N, >=3) float32 C-contiguous view; stride = row bytes (16 for XYZ+pad, 32 for XYZI...)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("cloud must be (N, >=3)")
    return a


def _colmajor(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float32).T).reshape(16)


def _from_colmajor(v):
    return np.asarray(v, dtype=np.float32).reshape(4, 4).T.copy()


class DeviceCloud:
    """An ndt_cloud: a cloud resident in HBM with its bounding boxes (include/ndt_mi355.h, "clouds that stay in HBM")."""

    def __init__(self, owner, c):
        self._owner, self._c, self._L = owner, c, owner._L

    def __len__(self):
        n = C.c_size_t(0)
        check(self._L.ndt_cloud_size(self._c, C.byref(n)))
        return n.value

    def data_ptr(self):
        p, n = C.c_void_p(None), C.c_size_t(0)
        check(self._L.ndt_cloud_data(self._c, C.byref(p), C.byref(n)))
        return p.value or 0

    def numpy(self):
        n = len(self)
        out = np.zeros((max(n, 1), 4), dtype=np.float32)
        check(self._L.ndt_cloud_download(self._owner._h, self._c, out.ctypes.data, 16))
        return out[:n, :3].copy()

    def bounds(self):
        """The cloud's two bounding boxes exactly as stored, and the producer that wrote them (ndt_cloud_bounds):
        -> ((2, 2, 3) float32 [box][min | max][xyz], route name of _lib.BOX_ROUTES)."""
        out, route = np.zeros(12, dtype=np.float32), C.c_int(-1)
        check(self._L.ndt_cloud_bounds(self._c, _f(out), C.byref(route)))
        return out.reshape(2, 2, 3), _lib.BOX_ROUTES[route.value]

    def release(self):
        if self._c:
            self._L.ndt_cloud_release(self._c)
            self._c = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def _dense_flags(is_dense, n):
    """(n,) int32 NaN rules of a batched filter: one bool for every cloud, or one per cloud."""
    if np.ndim(is_dense) == 0:
        return np.full(max(n, 1), int(bool(is_dense)), dtype=np.int32)
    f = np.asarray(is_dense).astype(bool).reshape(-1)
    if f.shape[0] != n:
        raise ValueError("one is_dense flag per cloud")
    return np.ascontiguousarray(f, dtype=np.int32) if n else np.zeros(1, dtype=np.int32)


def _handle_array(clouds):
    """A list of DeviceCloud as the array of ndt_cloud a *_clouds entry takes -> (the list, its length, the array)."""
    clouds = list(clouds)
    return clouds, len(clouds), (C.c_void_p * max(len(clouds), 1))(*[c._c for c in clouds])


def _out_array(n):
    """The array of ndt_cloud a *_clouds entry fills."""
    return (C.c_void_p * max(n, 1))()


def pairs_array(n_clouds, pairs=None):
    """(P, 2) int32 C-contiguous (target, source) cloud indices; None = the consecutive pairs (k-1, k) of n_clouds clouds."""
    if pairs is None:
        return np.ascontiguousarray(np.stack([np.arange(0, max(n_clouds - 1, 0)), np.arange(1, max(n_clouds, 1))], axis=1),
                                    dtype=np.int32).reshape(-1, 2)
    return np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))


EVAL_PLAN_FIELDS = ("ppb", "fused_blocks", "launch_blocks", "server_blocks", "batch_blocks")


class NormalDistributionsTransform:
    """Drop-in shaped like pclomp::NormalDistributionsTransform<PointT, PointT>."""

    def __init__(self, device=0, _handle=None):
        self._L = _lib.lib()
        self._device = device
        if _handle is None:
            h = C.c_void_p()
            check(self._L.ndt_create(device, C.byref(h)))
            self._h = h
        else:
            self._h = _handle
        self._keep = []  # keeps callback objects alive

    def __del__(self):
        try:
            self._L.ndt_destroy(self._h)
        except Exception:
            pass

    def copy(self):
        """Copy-construction (the nodes return the object by value): shares the device grid."""
        h = C.c_void_p()
        check(self._L.ndt_clone(self._h, C.byref(h)))
        return NormalDistributionsTransform(_handle=h)

    # ---- pclomp setters / getters (ndt_omp.h:115-209) -------------------------
    def setNumThreads(self, n):
        check(self._L.ndt_set_num_threads(self._h, int(n)))

    def setResolution(self, r):
        check(self._L.ndt_set_resolution(self._h, float(r)))

    def getResolution(self):
        return self._L.ndt_get_resolution(self._h)

    def setStepSize(self, s):
        check(self._L.ndt_set_step_size(self._h, float(s)))

    def getStepSize(self):
        return self._L.ndt_get_step_size(self._h)

    def setOutlierRatio(self, r):
        check(self._L.ndt_set_outlier_ratio(self._h, float(r)))

    def getOutlierRatio(self):
        return self._L.ndt_get_outlier_ratio(self._h)

    def setNeighborhoodSearchMethod(self, m):
        check(self._L.ndt_set_neighborhood_search_method(self._h, int(m)))

    def setTransformationEpsilon(self, e):
        check(self._L.ndt_set_transformation_epsilon(self._h, float(e)))

    def setMaximumIterations(self, n):
        check(self._L.ndt_set_maximum_iterations(self._h, int(n)))

    def setMinPointPerVoxel(self, n):
        check(self._L.ndt_set_min_points_per_voxel(self._h, int(n)))

    def setCovEigValueInflationRatio(self, r):
        check(self._L.ndt_set_cov_eig_value_inflation_ratio(self._h, float(r)))

    # ---- inputs -------------------------------------------------------------------
    def setInputTarget(self, cloud, is_dense=True):
        a = _cloud(cloud)
        check(self._L.ndt_set_input_target(self._h, a.ctypes.data, a.shape[0], a.shape[1] * 4, int(is_dense)))

    def setInputSource(self, cloud):
        a = _cloud(cloud)
        check(self._L.ndt_set_input_source(self._h, a.ctypes.data, a.shape[0], a.shape[1] * 4))

    def setInputTargetDevice(self, dev_ptr, n, stride_bytes, is_dense=True):
        check(self._L.ndt_set_input_target_device(self._h, C.c_void_p(dev_ptr), n, stride_bytes, int(is_dense)))

    def setInputTargetDeviceRef(self, dev_ptr, n, is_dense=True):
        """The cloud (n 16-byte records in HBM) is used where it lies: keep it alive and unchanged while it is the target."""
        check(self._L.ndt_set_input_target_device_ref(self._h, C.c_void_p(dev_ptr), n, int(is_dense)))

    def setInputSourceDeviceRef(self, dev_ptr, n):
        check(self._L.ndt_set_input_source_device_ref(self._h, C.c_void_p(dev_ptr), n))

    def setInputSourceDevice(self, dev_ptr, n, stride_bytes):
        check(self._L.ndt_set_input_source_device(self._h, C.c_void_p(dev_ptr), n, stride_bytes))

    # ---- registration -------------------------------------------------------------
    def align(self, guess=None, n_out=None):
        """align(output[, guess]).  Returns the aligned cloud (N,4) when n_out is given, else None."""
        g = None if guess is None else _colmajor(guess)
        out = np.zeros((n_out, 4), dtype=np.float32) if n_out else None
        check(self._L.ndt_align(self._h, _f(g) if g is not None else None, None, None, None, None,
                                out.ctypes.data if out is not None else None, 16))
        return out

    def _result(self):
        T = np.zeros(16, dtype=np.float32)
        conv, it = C.c_int(0), C.c_int(0)
        tp = C.c_double(0)
        check(self._L.ndt_get_result(self._h, _f(T), C.byref(conv), C.byref(it), C.byref(tp)))
        return _from_colmajor(T), bool(conv.value), it.value, tp.value

    def hasConverged(self):
        return self._result()[1]

    def getFinalTransformation(self):
        return self._result()[0]

    def getFinalNumIteration(self):
        return self._result()[2]

    def getTransformationProbability(self):
        return self._result()[3]

    def stats(self):
        ne, nh = C.c_int(0), C.c_int(0)
        nn = C.c_double(0)
        check(self._L.ndt_get_stats(self._h, C.byref(ne), C.byref(nh), C.byref(nn)))
        return dict(n_evals=ne.value, n_hessian_recomputes=nh.value, mean_neighbors=nn.value)

    def output_device(self):
        p = C.c_void_p()
        n = C.c_size_t(0)
        check(self._L.ndt_get_output_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def calculateScore(self, cloud):
        a = _cloud(cloud)
        s = C.c_double(0)
        check(self._L.ndt_calculate_score(self._h, a.ctypes.data, a.shape[0], a.shape[1] * 4, C.byref(s)))
        return s.value

    # ---- scan prefilter (pcl::VoxelGrid) --------------------------------------------
    def voxelGridFilter(self, cloud, leaf_size, is_dense=True):
        """pcl::VoxelGrid::filter on the GPU: (V, 3) float32 centroids in ascending voxel-index order.
        Raises NdtError(GRID_OVERFLOW) where PCL warns and passes the input through."""
        a = _cloud(cloud)
        out = np.zeros((max(a.shape[0], 1), 4), dtype=np.float32)
        n = C.c_size_t(0)
        check(self._L.ndt_voxel_grid_filter(self._h, a.ctypes.data, a.shape[0], a.shape[1] * 4, int(is_dense),
                                            float(leaf_size), out.ctypes.data, 16, C.byref(n)))
        return out[:n.value, :3].copy()

    def voxelGridFilterDevice(self, dev_ptr, n, stride_bytes, leaf_size, out_dev_ptr, is_dense=True):
        m = C.c_size_t(0)
        check(self._L.ndt_voxel_grid_filter_device(self._h, C.c_void_p(dev_ptr), n, stride_bytes, int(is_dense),
                                                   float(leaf_size), C.c_void_p(out_dev_ptr), C.byref(m)))
        return m.value

    def getFitnessScore(self, max_range=np.finfo(np.float64).max):
        """pcl::Registration::getFitnessScore of the last align (exact NN search on the GPU)."""
        v = C.c_double(0)
        check(self._L.ndt_get_fitness_score(self._h, float(max_range), C.byref(v)))
        return v.value

    # ---- global map (N2) ------------------------------------------------------------
    def mapClear(self):
        check(self._L.ndt_map_clear(self._h))

    def mapUpdate(self, scan, pose=None, leaf_size=0.5, is_dense=True):
        """update_global_map of the mapping nodes: transform the scan by `pose`, append it to the
        HBM-resident map, voxel-filter the map.  Returns (map size, overflowed)."""
        a = _cloud(scan)
        T = None if pose is None else _colmajor(pose)
        ov = C.c_int(0)
        check(self._L.ndt_map_update(self._h, a.ctypes.data, a.shape[0], a.shape[1] * 4, int(is_dense),
                                     _f(T) if T is not None else None, float(leaf_size), C.byref(ov)))
        return self.mapSize(), bool(ov.value)

    def mapUpdateDevice(self, dev_ptr, n, stride_bytes, pose=None, leaf_size=0.5, is_dense=True):
        T = None if pose is None else _colmajor(pose)
        ov = C.c_int(0)
        check(self._L.ndt_map_update_device(self._h, C.c_void_p(dev_ptr), n, stride_bytes, int(is_dense),
                                            _f(T) if T is not None else None, float(leaf_size), C.byref(ov)))
        return self.mapSize(), bool(ov.value)

    def mapSize(self):
        n = C.c_size_t(0)
        check(self._L.ndt_map_size(self._h, C.byref(n)))
        return n.value

    def mapGet(self):
        n = self.mapSize()
        out = np.zeros((max(n, 1), 4), dtype=np.float32)
        check(self._L.ndt_map_get(self._h, out.ctypes.data, 16))
        return out[:n, :3].copy()

    # ---- clouds that stay in HBM (ndt_cloud) ------------------------------------------
    def voxelGridFilterCloud(self, cloud, leaf_size, is_dense=True):
        """N1 with the result left in HBM: -> (DeviceCloud, overflowed)."""
        a = _cloud(cloud)
        c, ov = C.c_void_p(None), C.c_int(0)
        check(self._L.ndt_cloud_voxel_filter(self._h, a.ctypes.data, a.shape[0], a.shape[1] * 4, int(is_dense), float(leaf_size), 0,
                                             C.byref(c), C.byref(ov)))
        return DeviceCloud(self, c), bool(ov.value)

    def voxelGridFilterCloudDevice(self, dev_ptr, n, stride_bytes, leaf_size, is_dense=True):
        """The same with the input already in HBM."""
        c, ov = C.c_void_p(None), C.c_int(0)
        check(self._L.ndt_cloud_voxel_filter(self._h, C.c_void_p(dev_ptr), n, stride_bytes, int(is_dense), float(leaf_size), 1,
                                             C.byref(c), C.byref(ov)))
        return DeviceCloud(self, c), bool(ov.value)

    def voxelGridFilterBegin(self, dc, leaf_size, is_dense=True):
        """N1 of an ndt_cloud, first half: queued on the handle's filter stream, not waited for."""
        check(self._L.ndt_cloud_voxel_filter_begin(self._h, dc._c, int(is_dense), float(leaf_size)))

    def voxelGridFilterEnd(self):
        c, ov = C.c_void_p(None), C.c_int(0)
        check(self._L.ndt_cloud_voxel_filter_end(self._h, C.byref(c), C.byref(ov)))
        return DeviceCloud(self, c), bool(ov.value)

    def voxelGridFilterClouds(self, clouds, leaf_size, is_dense=True):
        """N1 of many clouds in one call (ndt_cloud_voxel_filter_batch / _clouds).  clouds: a list of (N_k, >=3) host arrays
        (concatenated once: the buffer form) or of DeviceCloud (the clouds form), not a mix; is_dense: one bool, or one per
        cloud.  Cloud k's result is what voxelGridFilterCloud returns for it alone, the same bits.
        -> (list of DeviceCloud, (n,) bool overflow flags)."""
        clouds = list(clouds)
        resident = [isinstance(c, DeviceCloud) for c in clouds]
        if any(resident) and not all(resident):
            raise ValueError("clouds must be all DeviceCloud or all host arrays, not a mix")
        n = len(clouds)
        dense = _dense_flags(is_dense, n)
        out = _out_array(n)
        ov = np.zeros(max(n, 1), dtype=np.int32)
        if n and all(resident):
            arr = (C.c_void_p * n)(*[c._c for c in clouds])
            check(self._L.ndt_cloud_voxel_filter_clouds(self._h, arr, n, _i(dense), float(leaf_size), out, _i(ov)))
        else:
            cols = {np.asarray(c).shape[1] if np.asarray(c).ndim == 2 else -1 for c in clouds}
            if len(cols) > 1:
                raise ValueError("all clouds must have the same column count")
            cat = _cloud(np.concatenate(clouds, axis=0)) if clouds else np.zeros((0, 4), np.float32)
            offsets = np.zeros(n + 1, dtype=np.uintp)
            offsets[1:] = np.cumsum([len(c) for c in clouds])
            check(self._L.ndt_cloud_voxel_filter_batch(self._h, cat.ctypes.data, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), n,
                                                       cat.shape[1] * 4, _i(dense), float(leaf_size), 0, out, _i(ov)))
        return self._wrap(out, n), ov[:n].astype(bool)

    def voxelGridFilterBatchDevice(self, dev_ptr, offsets, stride_bytes, leaf_size, is_dense=True):
        """The buffer form over records already in HBM: cloud k = records [offsets[k], offsets[k+1]) at dev_ptr."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uintp)
        n = len(offsets) - 1
        dense = _dense_flags(is_dense, n)
        out = _out_array(n)
        ov = np.zeros(max(n, 1), dtype=np.int32)
        check(self._L.ndt_cloud_voxel_filter_batch(self._h, C.c_void_p(dev_ptr), offsets.ctypes.data_as(C.POINTER(C.c_size_t)), n,
                                                   int(stride_bytes), _i(dense), float(leaf_size), 1, out, _i(ov)))
        return self._wrap(out, n), ov[:n].astype(bool)

    def _wrap(self, out, n):
        """The first n ndt_cloud of an output array as DeviceCloud of this handle."""
        return [DeviceCloud(self, C.c_void_p(p)) for p in list(out)[:n]]

    def _diag(self, fn, *fields):
        """The diagnostics entry fn(handle, out...) as a dict in the order of its arguments.  A field is a name (a size_t) or
        (name, ctypes type, conversion)."""
        fields = [(f, C.c_size_t, int) if isinstance(f, str) else f for f in fields]
        vals = [t(0) for _, t, _ in fields]
        check(fn(self._h, *[C.byref(v) for v in vals]))
        return {name: conv(v.value) for (name, _, conv), v in zip(fields, vals)}

    def filterBatchDiag(self):
        """What the last voxelGridFilterClouds / voxelGridFilterBatchDevice did (ndt_diag_filter_batch)."""
        return self._diag(self._L.ndt_diag_filter_batch, "passes", "single_route", "launches")

    def warmUp(self, expected_scan_points=0):
        check(self._L.ndt_warm_up(self._h, int(expected_scan_points)))

    def uploadCloud(self, cloud):
        a = _cloud(cloud)
        c = C.c_void_p(None)
        check(self._L.ndt_cloud_upload(self._h, a.ctypes.data, a.shape[0], a.shape[1] * 4, C.byref(c)))
        return DeviceCloud(self, c)

    def setInputSourceCloud(self, dc):
        check(self._L.ndt_set_input_source_cloud(self._h, dc._c))

    def setInputTargetCloud(self, dc, is_dense=True):
        check(self._L.ndt_set_input_target_cloud(self._h, dc._c, int(is_dense)))

    def promoteSourceToTarget(self, is_dense=True):
        """The current input source becomes the input target (cloud k of pair (k-1, k) is the target of pair (k, k+1))."""
        check(self._L.ndt_promote_source_to_target(self._h, int(is_dense)))

    def mapUpdateCloud(self, dc, pose=None, leaf_size=0.5, is_dense=True):
        T = None if pose is None else _colmajor(pose)
        ov = C.c_int(0)
        check(self._L.ndt_map_update_cloud(self._h, dc._c, int(is_dense), _f(T) if T is not None else None, float(leaf_size), C.byref(ov)))
        return self.mapSize(), bool(ov.value)

    # ---- many posed scans into the map in one call (ndt_map_update_clouds / _batch) -----------
    @staticmethod
    def _poses(poses, n):
        """(n, 16) float32 column-major poses of a batched map update, or None (the identity for every scan)."""
        if poses is None:
            return None
        poses = list(poses)
        if len(poses) != n:
            raise ValueError("one pose per scan")
        if n == 0:
            return None
        return np.ascontiguousarray(np.stack([_colmajor(T) for T in poses]))

    def mapUpdateClouds(self, clouds, poses=None, leaf_size=0.5, is_dense=True):
        """N2 of many scans in one call: every DeviceCloud moved by its pose, all appended to the map in the list's order, ONE
        voxel filter of the concatenation (not the per-scan loop's map: see ndt_map_update_clouds).  poses: one 4x4 per scan,
        None = the identity for all; is_dense: one bool, or one per scan.  Returns (map size, overflowed)."""
        clouds = list(clouds)
        if not all(isinstance(c, DeviceCloud) for c in clouds):
            raise ValueError("clouds must be DeviceCloud objects (host arrays: mapUpdateBatch)")
        n = len(clouds)
        P = self._poses(poses, n)
        dense = _dense_flags(is_dense, n)
        arr = _handle_array(clouds)[2]
        ov = C.c_int(0)
        check(self._L.ndt_map_update_clouds(self._h, arr, n, _i(dense), _f(P) if P is not None else None, float(leaf_size), C.byref(ov)))
        return self.mapSize(), bool(ov.value)

    def mapUpdateBatch(self, scans, poses=None, leaf_size=0.5, is_dense=True):
        """The same from a list of (N_k, >=3) host arrays, concatenated once and sent up with one copy (ndt_map_update_batch)."""
        scans = [np.asarray(c) for c in scans]
        n = len(scans)
        cols = {c.shape[1] if c.ndim == 2 else -1 for c in scans}
        if len(cols) > 1:
            raise ValueError("all scans must have the same column count")
        P = self._poses(poses, n)
        dense = _dense_flags(is_dense, n)
        cat = _cloud(np.concatenate(scans, axis=0)) if scans else np.zeros((0, 4), np.float32)
        offsets = np.zeros(n + 1, dtype=np.uintp)
        offsets[1:] = np.cumsum([len(c) for c in scans])
        ov = C.c_int(0)
        check(self._L.ndt_map_update_batch(self._h, cat.ctypes.data, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), n, cat.shape[1] * 4,
                                           _i(dense), _f(P) if P is not None else None, float(leaf_size), 0, C.byref(ov)))
        return self.mapSize(), bool(ov.value)

    def mapUpdateBatchDevice(self, dev_ptr, offsets, stride_bytes, poses=None, leaf_size=0.5, is_dense=True):
        """The buffer form over records already in HBM: scan k = records [offsets[k], offsets[k+1]) at dev_ptr."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uintp)
        n = len(offsets) - 1
        if n < 0:
            raise ValueError("offsets must hold n_scans + 1 entries")
        P = self._poses(poses, n)
        dense = _dense_flags(is_dense, n)
        ov = C.c_int(0)
        check(self._L.ndt_map_update_batch(self._h, C.c_void_p(dev_ptr), offsets.ctypes.data_as(C.POINTER(C.c_size_t)), n, int(stride_bytes),
                                           _i(dense), _f(P) if P is not None else None, float(leaf_size), 1, C.byref(ov)))
        return self.mapSize(), bool(ov.value)

    def inputBounds(self, which):
        """The bounding boxes of "source", "target" or "map" as stored, and their producer (ndt_diag_input_bounds):
        -> ((2, 2, 3) float32 [box][min | max][xyz], route name)."""
        out, route = np.zeros(12, dtype=np.float32), C.c_int(-1)
        check(self._L.ndt_diag_input_bounds(self._h, ("source", "target", "map").index(which), _f(out), C.byref(route)))
        return out.reshape(2, 2, 3), _lib.BOX_ROUTES[route.value]

    def mapBatchDiag(self):
        """What the last mapUpdateClouds / mapUpdateBatch / mapUpdateBatchDevice did (ndt_diag_map_batch)."""
        return self._diag(self._L.ndt_diag_map_batch, "transform_launches", "filters", "box_passes")

    # ---- accumulating target: posed scans merged into the voxel grid (ndt_target_accumulate*) ----
    def targetAccumulate(self, scan, pose=None, is_dense=True):
        """The scan moved by `pose` (4x4, None = identity) is merged into the handle's accumulated target: afterwards the handle
        behaves as if its target had been set from the concatenation of every accumulated scan.  The first call replaces the
        target the handle held.  Returns targetAccumulated()."""
        a = _cloud(scan)
        T = None if pose is None else _colmajor(pose)
        check(self._L.ndt_target_accumulate(self._h, a.ctypes.data, a.shape[0], a.shape[1] * 4, int(is_dense),
                                            _f(T) if T is not None else None))
        return self.targetAccumulated()

    def targetAccumulateDevice(self, dev_ptr, n, stride_bytes, pose=None, is_dense=True):
        T = None if pose is None else _colmajor(pose)
        check(self._L.ndt_target_accumulate_device(self._h, C.c_void_p(dev_ptr), n, stride_bytes, int(is_dense),
                                                   _f(T) if T is not None else None))
        return self.targetAccumulated()

    def targetAccumulateCloud(self, dc, pose=None, is_dense=True):
        T = None if pose is None else _colmajor(pose)
        check(self._L.ndt_target_accumulate_cloud(self._h, dc._c, int(is_dense), _f(T) if T is not None else None))
        return self.targetAccumulated()

    def targetAccumulateClouds(self, clouds, poses=None, is_dense=True):
        """Many DeviceClouds in ONE pass (one sort, one merge), in the list's order; poses: one 4x4 per cloud, None = the
        identity for all.  The same bits as one targetAccumulateCloud per cloud."""
        clouds = list(clouds)
        if not all(isinstance(c, DeviceCloud) for c in clouds):
            raise ValueError("clouds must be DeviceCloud objects")
        n = len(clouds)
        P = self._poses(poses, n)
        arr = _handle_array(clouds)[2]
        check(self._L.ndt_target_accumulate_clouds(self._h, arr, n, int(is_dense), _f(P) if P is not None else None))
        return self.targetAccumulated()

    def targetAccumulateReset(self):
        check(self._L.ndt_target_accumulate_reset(self._h))

    def targetAccumulated(self):
        """-> dict(points, voxels, updates) of the accumulated target (zeros without one)."""
        p, v, u = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        check(self._L.ndt_target_accumulated(self._h, C.byref(p), C.byref(v), C.byref(u)))
        return dict(points=p.value, voxels=v.value, updates=u.value)

    def targetAccumulateDiag(self):
        """What the last targetAccumulate* call did (ndt_diag_target_accumulate)."""
        return self._diag(self._L.ndt_diag_target_accumulate, "touched_voxels", "new_voxels", ("relinked", C.c_int, bool),
                          ("table_grown", C.c_int, bool), "launches")

    def targetAccumulateCrop(self, min_xyz, max_xyz):
        """Crop the accumulated target to the box [min_xyz, max_xyz] (ndt_target_accumulate_crop): a voxel stays exactly when
        its cell lies in crop_cell_range(resolution, min_xyz, max_xyz); afterwards the handle behaves as if the points of
        the other cells had never been accumulated.  -inf / +inf leave a side open.  Returns targetAccumulated()."""
        mn, mx = (np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (min_xyz, max_xyz))
        check(self._L.ndt_target_accumulate_crop(self._h, _f(mn), _f(mx)))
        return self.targetAccumulated()

    def targetCropDiag(self):
        """What the last targetAccumulateCrop did (ndt_diag_target_crop)."""
        return self._diag(self._L.ndt_diag_target_crop, "kept_voxels", "removed_voxels", "kept_points", ("relinked", C.c_int, bool), "launches")

    # ---- clearing by rays: drop the voxels a scan sees through (ndt_target_accumulate_clear_rays*) ----
    def _ray_args(self, clouds, poses, origins, min_rays, margin, min_range, max_range):
        clouds = [clouds] if isinstance(clouds, DeviceCloud) else list(clouds)
        if not all(isinstance(c, DeviceCloud) for c in clouds):
            raise ValueError("clouds must be DeviceCloud objects")
        n = len(clouds)
        if poses is not None and np.asarray(poses).ndim == 2:
            poses = [poses]
        if origins is not None and np.asarray(origins).ndim == 1:
            origins = [origins]
        P = self._poses(poses, n)
        O = None
        if origins is not None and n:
            O = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1)
            if len(O) != 3 * n:
                raise ValueError("one origin (3 floats) per cloud")
        spec = ray_spec(self.getResolution(), min_rays, margin, min_range, max_range)
        arr = _handle_array(clouds)[2]
        return arr, n, (_f(P) if P is not None else None), (_f(O) if O is not None else None), spec, (P, O)

    def targetClearRays(self, clouds, poses=None, origins=None, min_rays=2, margin=None, min_range=0.0, max_range=None):
        """Drop the voxels of the accumulated target that the scans see through (ndt_target_accumulate_clear_rays_clouds): every
        DeviceCloud is moved by its pose (4x4, None = identity) and a ray is walked from its sensor origin (None = the pose's
        translation) to every posed point, up to `margin` metres (None = the resolution) before it; a voxel goes when at least
        min_rays rays of the call cross its cell and no point of the call lies in it.  max_range None: the largest the
        resolution allows.  One DeviceCloud or a list; all clouds of a list go through one pass.  Returns targetAccumulated()."""
        arr, n, P, O, spec, keep = self._ray_args(clouds, poses, origins, min_rays, margin, min_range, max_range)
        check(self._L.ndt_target_accumulate_clear_rays_clouds(self._h, arr, n, P, O, C.byref(spec)))
        return self.targetAccumulated()

    def targetRayCounts(self, clouds, poses=None, origins=None, min_rays=2, margin=None, min_range=0.0, max_range=None):
        """The ray pass of targetClearRays without the removal (ndt_target_accumulate_ray_counts): per voxel of the target, in
        ascending key, -> dict(cells (V, 3) int32, miss (V,) uint32, hit (V,) bool).  The target is not changed."""
        arr, n, P, O, spec, keep = self._ray_args(clouds, poses, origins, min_rays, margin, min_range, max_range)
        V = self.targetAccumulated()["voxels"]
        cells, miss, hit = np.zeros((V, 3), np.int32), np.zeros(V, np.uint32), np.zeros(V, np.uint8)
        nv = C.c_size_t(0)
        check(self._L.ndt_target_accumulate_ray_counts(self._h, arr, n, P, O, C.byref(spec), _i(cells), miss.ctypes.data_as(C.POINTER(C.c_uint)),
                                                       hit.ctypes.data_as(C.POINTER(C.c_ubyte)), V, C.byref(nv)))
        return dict(cells=cells[:nv.value], miss=miss[:nv.value], hit=hit[:nv.value].astype(bool))

    def targetClearRaysDiag(self):
        """What the last targetClearRays / targetRayCounts that reached the device did (ndt_diag_target_clear_rays)."""
        return self._diag(self._L.ndt_diag_target_clear_rays, "rays_cast", "rays_skipped", ("cells_visited", C.c_uint64, int), "touched_voxels",
                          "removed_voxels", "kept_voxels", "kept_points", ("relinked", C.c_int, bool), "launches")

    @staticmethod
    def _box(min_xyz, max_xyz):
        if (min_xyz is None) != (max_xyz is None):
            raise ValueError("give both bounds, or neither for every voxel")
        if min_xyz is None:
            return None, None
        mn, mx = (np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (min_xyz, max_xyz))
        return mn, mx

    def targetAccumulateExport(self, min_xyz=None, max_xyz=None):
        """The voxels of the accumulated target whose cells lie in crop_cell_range(resolution, min_xyz, max_xyz) -- all of
        them without bounds -- as a blob (ndt_target_accumulate_export; layout: ACC_ROW_DTYPE, acc_blob_info).  The target
        is not changed.  -> bytes."""
        mn, mx = self._box(min_xyz, max_xyz)
        cap = 64 + ACC_ROW_DTYPE.itemsize * self.targetAccumulated()["voxels"]   # room for every voxel: one call
        buf = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        check(self._L.ndt_target_accumulate_export(self._h, _f(mn) if mn is not None else None, _f(mx) if mx is not None else None,
                                                   buf.ctypes.data, cap, C.byref(n)))
        return buf[:n.value].tobytes()

    def targetAccumulateImport(self, blob):
        """The voxels of a blob into the accumulated target (ndt_target_accumulate_import): an accumulate call whose input is
        voxels.  A handle without an accumulated target starts one; every cell of the blob must be absent from the target.
        Returns targetAccumulated()."""
        b = np.frombuffer(bytes(blob), dtype=np.uint8)
        check(self._L.ndt_target_accumulate_import(self._h, b.ctypes.data if len(b) else None, len(b)))
        return self.targetAccumulated()

    def targetAccumulateSave(self, path, min_xyz=None, max_xyz=None):
        """targetAccumulateExport into the file `path` (written beside it and renamed)."""
        mn, mx = self._box(min_xyz, max_xyz)
        check(self._L.ndt_target_accumulate_save(self._h, _f(mn) if mn is not None else None, _f(mx) if mx is not None else None,
                                                 os.fsencode(path)))

    def targetAccumulateLoad(self, path):
        """targetAccumulateImport of the file `path`.  Returns targetAccumulated()."""
        check(self._L.ndt_target_accumulate_load(self._h, os.fsencode(path)))
        return self.targetAccumulated()

    def targetExportDiag(self):
        """What the last targetAccumulateExport / Save did (ndt_diag_target_export)."""
        return self._diag(self._L.ndt_diag_target_export, "voxels", "points", "launches")

    # ---- batch (map-build) ---------------------------------------------------------
    def alignBatch(self, clouds=None, guesses=None, device_ptr=None, offsets=None, stride_bytes=16):
        """Register many sources against the one target in lock-step.

        clouds: list of (N_k, >=3) arrays (host), or device_ptr + offsets for HBM-resident data."""
        if clouds is not None:
            cols = {c.shape[1] for c in clouds}
            if len(cols) != 1:
                raise ValueError("all clouds must have the same column count")
            cat = _cloud(np.concatenate(clouds, axis=0))
            offsets = np.zeros(len(clouds) + 1, dtype=np.uintp)
            offsets[1:] = np.cumsum([c.shape[0] for c in clouds])
            ptr, stride, fn = cat.ctypes.data, cat.shape[1] * 4, self._L.ndt_align_batch
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.uintp)
            ptr, stride, fn = C.c_void_p(device_ptr), stride_bytes, self._L.ndt_align_batch_device
        B = len(offsets) - 1
        g = None
        if guesses is not None:
            g = np.ascontiguousarray(np.stack([_colmajor(x) for x in guesses]))
        T = np.zeros((B, 16), dtype=np.float32)
        conv = np.zeros(B, dtype=np.int32)
        it = np.zeros(B, dtype=np.int32)
        tp = np.zeros(B, dtype=np.float64)
        check(fn(self._h, ptr, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), B, stride,
                 _f(g) if g is not None else None, _f(T), _i(conv), _i(it), _d(tp)))
        return dict(T=np.stack([_from_colmajor(T[k]) for k in range(B)]), converged=conv.astype(bool),
                    iterations=it, trans_probability=tp)

    def alignPairs(self, clouds, pairs=None, guesses=None, is_dense=True):
        """Register (target, source) pairs of clouds in lock-step, every pair against the grid of its own target
        (ndt_align_pairs*).  clouds: list of (N_k, >=3) host arrays, or of DeviceCloud (ndt_cloud); pairs: (P, 2) cloud
        indices (target, source), None = the consecutive pairs (k-1, k); at most 65535 pairs per call.  Returns alignBatch's
        dict, one entry per pair."""
        resident = [isinstance(c, DeviceCloud) for c in clouds]
        if any(resident) and not all(resident):
            raise ValueError("clouds must be all DeviceCloud or all host arrays, not a mix")
        P = pairs_array(len(clouds), pairs)
        n = P.shape[0]
        g = None
        if guesses is not None:
            g = np.ascontiguousarray(np.stack([_colmajor(x) for x in guesses]))
            if g.shape[0] != n:
                raise ValueError("one guess per pair")
        T = np.zeros((n, 16), dtype=np.float32)
        conv = np.zeros(n, dtype=np.int32)
        it = np.zeros(n, dtype=np.int32)
        tp = np.zeros(n, dtype=np.float64)
        out = (_f(g) if g is not None else None, _f(T), _i(conv), _i(it), _d(tp))
        if clouds and all(isinstance(c, DeviceCloud) for c in clouds):
            arr = (C.c_void_p * len(clouds))(*[c._c for c in clouds])
            check(self._L.ndt_align_pairs_clouds(self._h, arr, len(clouds), int(is_dense), _i(P), n, *out))
        else:
            cols = {np.asarray(c).shape[1] for c in clouds}
            if len(cols) > 1:
                raise ValueError("all clouds must have the same column count")
            cat = _cloud(np.concatenate(clouds, axis=0)) if clouds else np.zeros((0, 4), np.float32)
            offsets = np.zeros(len(clouds) + 1, dtype=np.uintp)
            offsets[1:] = np.cumsum([len(c) for c in clouds])
            check(self._L.ndt_align_pairs(self._h, cat.ctypes.data, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), len(clouds),
                                          cat.shape[1] * 4, int(is_dense), _i(P), n, *out))
        return dict(T=np.stack([_from_colmajor(T[k]) for k in range(n)]) if n else np.zeros((0, 4, 4), np.float32),
                    converged=conv.astype(bool), iterations=it, trans_probability=tp)

    def pairsFitness(self, transforms=None, max_range=np.finfo(np.float64).max):
        """getFitnessScore of every pair of the last alignPairs (ndt_pairs_fitness_scores), all in one launch: pair k's source
        moved by transforms[k] (None = that call's final transformations) against pair k's target.  Returns (P,) float64."""
        T = None
        if transforms is not None:
            T = np.ascontiguousarray(np.stack([_colmajor(x) for x in transforms]), dtype=np.float32)
        n = C.c_size_t(0)  # the pairs the library holds (those of the last alignPairs): what it reads and writes
        check(self._L.ndt_pairs_count(self._h, C.byref(n)))
        P = n.value
        if T is not None and T.shape[0] != P:
            raise ValueError("one transform per pair of the last alignPairs")
        out = np.zeros(max(P, 1), dtype=np.float64)
        check(self._L.ndt_pairs_fitness_scores(self._h, _f(T) if T is not None else None, float(max_range), _d(out)))
        return out[:P].copy()

    def fitnessLaunches(self):
        """(launches, blocks of the largest) of the last pairsFitness / batchFitness (ndt_diag_fitness_launches)."""
        return tuple(self._diag(self._L.ndt_diag_fitness_launches, "launches", "blocks").values())

    def batchFitness(self, clouds=None, transforms=None, max_range=np.finfo(np.float64).max, device_ptr=None, offsets=None,
                     stride_bytes=16):
        """getFitnessScore of many scans against this handle's target (ndt_batch_fitness_scores*), scan k moved by
        transforms[k]; clouds / device_ptr + offsets as alignBatch takes them.  Returns (B,) float64."""
        if clouds is not None:
            cat = _cloud(np.concatenate(clouds, axis=0)) if len(clouds) else np.zeros((0, 4), np.float32)
            offsets = np.zeros(len(clouds) + 1, dtype=np.uintp)
            offsets[1:] = np.cumsum([len(c) for c in clouds])
            ptr, stride, fn = cat.ctypes.data, cat.shape[1] * 4, self._L.ndt_batch_fitness_scores
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.uintp)
            ptr, stride, fn = C.c_void_p(device_ptr), stride_bytes, self._L.ndt_batch_fitness_scores_device
        B = len(offsets) - 1
        if transforms is None:
            raise ValueError("batchFitness needs one transform per scan")
        T = np.ascontiguousarray(np.stack([_colmajor(x) for x in transforms]), dtype=np.float32) if B else np.zeros((0, 16), np.float32)
        if T.shape[0] != B:
            raise ValueError("one transform per scan")
        out = np.zeros(max(B, 1), dtype=np.float64)
        check(fn(self._h, ptr, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), B, stride, _f(T) if B else None, float(max_range),
                 _d(out)))
        return out[:B].copy()

    # ---- the target's centroid cloud and getFitnessScore against it (any target, accumulated ones too) -------
    def gridCentroids(self):
        """The centroid cloud of the target (ndt_grid_centroids): ((V, 4) float32 of x, y, z, 1, (V,) int64 linear voxel indices),
        one point per voxel that reached min_points_per_voxel, in ascending index."""
        n = C.c_size_t(0)
        check(self._L.ndt_grid_centroids(self._h, None, None, 0, C.byref(n)))
        V = n.value
        xyz1 = np.zeros((max(V, 1), 4), dtype=np.float32)
        idx = np.zeros(max(V, 1), dtype=np.int64)
        if V:
            check(self._L.ndt_grid_centroids(self._h, _f(xyz1), idx.ctypes.data_as(C.POINTER(C.c_int64)), V, C.byref(n)))
        return xyz1[:V].copy(), idx[:V].copy()

    def gridCentroidsCloud(self):
        """The same cloud as a resident DeviceCloud (ndt_grid_centroids_cloud)."""
        c = C.c_void_p(None)
        check(self._L.ndt_grid_centroids_cloud(self._h, C.byref(c)))
        return DeviceCloud(self, c)

    def centroidFitnessScore(self, max_range=np.finfo(np.float64).max):
        """getFitnessScore of the source under the last align's final transformation against the target's centroid cloud
        (ndt_get_centroid_fitness_score): works on an accumulated target, which keeps no points."""
        out = C.c_double(0)
        check(self._L.ndt_get_centroid_fitness_score(self._h, float(max_range), C.byref(out)))
        return out.value

    def batchCentroidFitness(self, clouds=None, transforms=None, max_range=np.finfo(np.float64).max, device_ptr=None, offsets=None,
                             stride_bytes=16):
        """The centroid fitness of many scans against this handle's target (ndt_batch_centroid_fitness_scores*), scan k moved
        by transforms[k]; arguments as batchFitness takes them.  Returns (B,) float64."""
        if clouds is not None:
            cat = _cloud(np.concatenate(clouds, axis=0)) if len(clouds) else np.zeros((0, 4), np.float32)
            offsets = np.zeros(len(clouds) + 1, dtype=np.uintp)
            offsets[1:] = np.cumsum([len(c) for c in clouds])
            ptr, stride, fn = cat.ctypes.data, cat.shape[1] * 4, self._L.ndt_batch_centroid_fitness_scores
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.uintp)
            ptr, stride, fn = C.c_void_p(device_ptr), stride_bytes, self._L.ndt_batch_centroid_fitness_scores_device
        B = len(offsets) - 1
        if transforms is None:
            raise ValueError("batchCentroidFitness needs one transform per scan")
        T = np.ascontiguousarray(np.stack([_colmajor(x) for x in transforms]), dtype=np.float32) if B else np.zeros((0, 16), np.float32)
        if T.shape[0] != B:
            raise ValueError("one transform per scan")
        out = np.zeros(max(B, 1), dtype=np.float64)
        check(fn(self._h, ptr, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), B, stride, _f(T) if B else None, float(max_range),
                 _d(out)))
        return out[:B].copy()

    def centroidFitnessDiag(self):
        """What the last centroidFitnessScore / batchCentroidFitness did (ndt_diag_centroid_fitness)."""
        return self._diag(self._L.ndt_diag_centroid_fitness, "launches", "excursion_passes", ("excursion", C.c_float, float), "max_blocks")

    # ---- one source, many poses (ndt_score_poses / ndt_align_guesses / ndt_align_multistart) -------
    @staticmethod
    def _pose_table(poses):
        """(G, 16) float32 column-major table of G 4x4 transforms (a list, or one (G, 4, 4) array; G may be 0)."""
        a = np.asarray(poses, dtype=np.float32)
        if a.size == 0:
            return np.zeros((0, 16), dtype=np.float32)
        if a.ndim != 3 or a.shape[1:] != (4, 4):
            raise ValueError("poses must be G transforms of 4x4")
        return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1, 16)

    def scorePoses(self, transforms):
        """calculateScore of the input source moved by each of the 4x4 transforms, all poses in one launch per chunk:
        (G,) float64, entry g the bits of calculateScore(transformPointCloud(source, transforms[g]))."""
        T = self._pose_table(transforms)
        G = T.shape[0]
        out = np.zeros(max(G, 1), dtype=np.float64)
        check(self._L.ndt_score_poses(self._h, _f(T) if G else None, G, _d(out)))
        return out[:G].copy()

    def scorePosesLaunches(self):
        """(launches, blocks of all of them) of the last scorePoses (ndt_diag_score_poses)."""
        return tuple(self._diag(self._L.ndt_diag_score_poses, "launches", "blocks").values())

    # ---- nearest-voxel transformation likelihood (ndt_calculate_nvtl / ndt_get_nvtl / ndt_nvtl_poses / ndt_source_point_nvtl)
    def calculateNVTL(self, cloud):
        """(nvtl, n_found) of `cloud`, used as given, against the target: per point the likelihood of its best-fitting
        neighbour voxel, averaged over the points that have a neighbour at all; (0.0, 0) when none has."""
        a = _cloud(cloud)
        v, nf = C.c_double(0), C.c_size_t(0)
        check(self._L.ndt_calculate_nvtl(self._h, a.ctypes.data, a.shape[0], a.shape[1] * 4, C.byref(v), C.byref(nf)))
        return v.value, nf.value

    def getNVTL(self):
        """(nvtl, n_found) of the input source moved by the last align's final transformation (ndt_get_nvtl)."""
        v, nf = C.c_double(0), C.c_size_t(0)
        check(self._L.ndt_get_nvtl(self._h, C.byref(v), C.byref(nf)))
        return v.value, nf.value

    def nvtlPoses(self, transforms, counts=False):
        """NVTL of the input source moved by each of the 4x4 transforms, all poses in one launch per chunk: (G,) float64,
        entry g the bits of calculateNVTL(transformPointCloud(source, transforms[g])).  counts=True: (nvtl, n_found)."""
        T = self._pose_table(transforms)
        G = T.shape[0]
        out = np.zeros(max(G, 1), dtype=np.float64)
        nf = np.zeros(max(G, 1), dtype=np.uintp)
        check(self._L.ndt_nvtl_poses(self._h, _f(T) if G else None, G, _d(out), nf.ctypes.data_as(C.POINTER(C.c_size_t))))
        return (out[:G].copy(), nf[:G].astype(np.int64)) if counts else out[:G].copy()

    def sourcePointCount(self):
        """Points of the input source (ndt_source_point_count); 0 without one."""
        n = C.c_size_t(0)
        check(self._L.ndt_source_point_count(self._h, C.byref(n)))
        return n.value

    def sourcePointNVTL(self, transform=None, device=False):
        """(per_point, nvtl, n_found): the likelihood of every source point under `transform` (None: the last align's final
        transformation) in the caller's point order, -1.0 where a point has no neighbour voxel, and the reduction of the same
        launch.  device=True: per_point is the device pointer (valid until the next sourcePointNVTL) instead of an array."""
        T = None if transform is None else _colmajor(transform)
        n = self.sourcePointCount()
        out = None if device else np.zeros(max(n, 1), dtype=np.float64)
        dptr, v, nf = C.c_void_p(), C.c_double(0), C.c_size_t(0)
        check(self._L.ndt_source_point_nvtl(self._h, _f(T) if T is not None else None, _d(out) if out is not None else None,
                                            C.byref(dptr), C.byref(v), C.byref(nf)))
        return (dptr.value if device else out[:n].copy()), v.value, nf.value

    def nvtlLaunches(self):
        """(launches, blocks of all of them) of the last NVTL call that reached the device (ndt_diag_nvtl)."""
        return tuple(self._diag(self._L.ndt_diag_nvtl, "launches", "blocks").values())

    # ---- selection of the points of resident clouds (ndt_cloud_select / _clouds / ndt_source_select_by_nvtl) ---------------
    @staticmethod
    def selectSpec(finite=False, box=None, box_negate=False, range=None, centre=(0, 0, 0), range_negate=False, key_range=None,
                   key_negate=False):
        """The ndt_select_spec of the keyword form: box = (min_xyz, max_xyz), range = (r_min, r_max) about `centre`,
        key_range = (key_lo, key_hi); the *_negate switches set their bit whether or not the test is given (the library
        refuses a negation without its test)."""
        s = _lib.SelectSpec()
        flags = _lib.SELECT_FINITE if finite else 0
        if box is not None:
            flags |= _lib.SELECT_BOX
            mn, mx = np.asarray(box[0], dtype=np.float32).reshape(3), np.asarray(box[1], dtype=np.float32).reshape(3)
            s.box_min[:], s.box_max[:] = mn.tolist(), mx.tolist()
        if range is not None:
            flags |= _lib.SELECT_RANGE
            s.centre[:] = np.asarray(centre, dtype=np.float32).reshape(3).tolist()
            s.r_min, s.r_max = float(np.float32(range[0])), float(np.float32(range[1]))
        if key_range is not None:
            flags |= _lib.SELECT_KEY
            s.key_lo, s.key_hi = float(key_range[0]), float(key_range[1])
        flags |= (_lib.SELECT_BOX_NEGATE if box_negate else 0) | (_lib.SELECT_RANGE_NEGATE if range_negate else 0)
        flags |= _lib.SELECT_KEY_NEGATE if key_negate else 0
        s.flags = flags
        return s

    def selectCloud(self, dc, finite=False, box=None, box_negate=False, range=None, centre=(0, 0, 0), range_negate=False, keys=None,
                    key_range=None, key_negate=False, indices=False, spec=None):
        """The points of the resident cloud `dc` that pass every enabled test, in dc's order, as a new DeviceCloud with exact
        boxes (ndt_cloud_select; the tests are defined in include/ndt_mi355.h).  keys: one float64 per point (an array), or
        the device pointer of such values (an int, e.g. sourcePointNVTL(device=True)[0]).  spec: a ready _lib.SelectSpec
        instead of the keywords.  indices=True: -> (DeviceCloud, (n_kept,) int32 indices of the kept points, ascending)."""
        if spec is None:
            spec = self.selectSpec(finite, box, box_negate, range, centre, range_negate, key_range, key_negate)
        n = len(dc)
        on_device, kp, keep = 0, None, None
        if keys is not None:
            if isinstance(keys, (int, np.integer)):
                on_device, kp = 1, C.c_void_p(int(keys))
            else:
                keep = np.ascontiguousarray(keys, dtype=np.float64).reshape(-1)
                if keep.shape[0] != n:
                    raise ValueError("one key per point")
                kp = C.c_void_p(keep.ctypes.data) if n else C.c_void_p(np.zeros(1).ctypes.data)
        idx = np.zeros(max(n, 1), dtype=np.int32) if indices else None
        c, nk = C.c_void_p(None), C.c_size_t(0)
        check(self._L.ndt_cloud_select(self._h, dc._c, C.byref(spec), kp, on_device, C.byref(c),
                                       idx.ctypes.data_as(C.POINTER(C.c_int32)) if indices else None, C.byref(nk)))
        out = DeviceCloud(self, c)
        return (out, idx[:nk.value].copy()) if indices else out

    def selectClouds(self, clouds, finite=False, box=None, box_negate=False, range=None, centre=(0, 0, 0), range_negate=False,
                     spec=None):
        """selectCloud of every DeviceCloud of the list under one spec, two launches in all (ndt_cloud_select_clouds; no key
        test): a list of DeviceCloud, entry k what selectCloud gives for clouds[k] alone, the same bits."""
        if spec is None:
            spec = self.selectSpec(finite, box, box_negate, range, centre, range_negate)
        clouds, n, arr = _handle_array(clouds)
        out, nk = _out_array(n), (C.c_size_t * max(n, 1))()
        check(self._L.ndt_cloud_select_clouds(self._h, arr, n, C.byref(spec), out, nk))
        return self._wrap(out, n)

    def sourceSelectByNVTL(self, min_likelihood, transform=None, keep_unfound=True):
        """The input source's own points (unmoved, caller's order) that the target explains under `transform` (None: the last
        align's final transformation): kept iff (a neighbour voxel was found and L >= min_likelihood) or (none was found and
        keep_unfound).  The per-point values stay on the device.  -> (DeviceCloud, n_found).  Counts as an NVTL call for
        nvtlLaunches."""
        T = None if transform is None else _colmajor(transform)
        c, nk, nf = C.c_void_p(None), C.c_size_t(0), C.c_size_t(0)
        check(self._L.ndt_source_select_by_nvtl(self._h, _f(T) if T is not None else None, float(min_likelihood), int(bool(keep_unfound)),
                                                C.byref(c), C.byref(nk), C.byref(nf)))
        return DeviceCloud(self, c), nf.value

    def selectDiag(self):
        """What the last selection that reached the device did (ndt_diag_select)."""
        return self._diag(self._L.ndt_diag_select, "launches", "blocks", "clouds")

    @staticmethod
    def selectPlan(n):
        """(blocks, points_per_block) of the selection of a cloud of n points (ndt_host_select_plan; host only)."""
        b, p = C.c_int(0), C.c_int(0)
        check(_lib.lib().ndt_host_select_plan(int(n), C.byref(b), C.byref(p)))
        return b.value, p.value

    @staticmethod
    def selectPoint(spec, xyz, key=0.0):
        """Is the point xyz (three float32) with key `key` kept under the _lib.SelectSpec `spec`?  (ndt_host_select_point: the
        predicate the kernels evaluate; host only.)"""
        p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(3)
        keep = C.c_int(-1)
        check(_lib.lib().ndt_host_select_point(C.byref(spec), _f(p), float(key), C.byref(keep)))
        return bool(keep.value)

    # ---- motion compensation of resident scans by point time (ndt_cloud_deskew / _clouds) --------------------------------
    def deskewCloud(self, dc, motion, times, device=False):
        """The resident cloud `dc` as seen from the sensor frame at motion.t_ref, every record moved by the sensor's pose at
        its own time (ndt_cloud_deskew; the definition is in include/ndt_mi355.h): a new DeviceCloud of len(dc) records in
        dc's order with exact boxes.  motion: a _lib.DeskewMotion (host_deskew_motion).  times: one float64 per point (an
        array), or with device=True the device pointer of such values (an int).  -> (DeviceCloud, n_untimed)."""
        n = len(dc)
        keep = None
        if device:
            tp = C.c_void_p(int(times))
        else:
            keep = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
            if keep.shape[0] != n:
                raise ValueError("one time per point")
            tp = C.c_void_p(keep.ctypes.data) if n else None
        c, nu = C.c_void_p(None), C.c_size_t(0)
        check(self._L.ndt_cloud_deskew(self._h, dc._c, C.byref(motion), tp, int(bool(device)), C.byref(c), C.byref(nu)))
        return DeviceCloud(self, c), nu.value

    def deskewClouds(self, clouds, motions, times):
        """deskewCloud of every DeviceCloud of the list under its own motion, one launch in all (ndt_cloud_deskew_clouds).
        times: a list of per-cloud float64 arrays, or one array packed in cloud order.  -> (list of DeviceCloud, list of
        n_untimed), entry k what deskewCloud gives for clouds[k] alone, the same bits."""
        (clouds, n, arr), motions = _handle_array(clouds), list(motions)
        if len(motions) != n:
            raise ValueError("one motion per cloud")
        if isinstance(times, (list, tuple)):
            times = np.concatenate([np.asarray(t, dtype=np.float64).reshape(-1) for t in times]) if times else np.zeros(0)
        keep = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        if keep.shape[0] != sum(len(c) for c in clouds):
            raise ValueError("one time per point")
        ms = (_lib.DeskewMotion * max(n, 1))(*motions)
        out, nu = _out_array(n), (C.c_size_t * max(n, 1))()
        check(self._L.ndt_cloud_deskew_clouds(self._h, arr, n, ms, C.c_void_p(keep.ctypes.data) if keep.shape[0] else None, 0, out, nu))
        return self._wrap(out, n), list(nu)[:n]

    def deskewDiag(self):
        """What the last motion compensation that reached the device did (ndt_diag_deskew)."""
        return self._diag(self._L.ndt_diag_deskew, "launches", "blocks", "clouds")

    # ---- outlier removal of resident clouds (ndt_cloud_neighbor_values / ndt_cloud_remove_outliers / _clouds) ------------
    @staticmethod
    def outlierSpec(radius=None, min_neighbors=None, mean_k=None, stddev_mul=None, negate=False):
        """The ndt_outlier_spec of the keyword form: radius and min_neighbors (RADIUS), or mean_k and stddev_mul
        (STATISTICAL); exactly one of the two pairs."""
        if (radius is None) == (mean_k is None):
            raise ValueError("give radius / min_neighbors or mean_k / stddev_mul")
        s = _lib.OutlierSpec()
        s.negate = int(bool(negate))
        if radius is not None:
            s.method, s.radius, s.min_neighbors = _lib.OUTLIER_RADIUS, float(np.float32(radius)), int(1 if min_neighbors is None else min_neighbors)
        else:
            s.method, s.mean_k, s.stddev_mul = _lib.OUTLIER_STATISTICAL, int(mean_k), float(1.0 if stddev_mul is None else stddev_mul)
        return s

    @staticmethod
    def _outlier_stats(st):
        return dict(n_finite=st.n_finite, n_valid=st.n_valid, mean=st.mean, stddev=st.stddev, threshold=st.threshold)

    def neighborValues(self, dc, radius=None, min_neighbors=None, mean_k=None, stddev_mul=None, device=False, spec=None):
        """The value the outlier filters judge every point of the resident cloud `dc` by (ndt_cloud_neighbor_values; defined
        in include/ndt_mi355.h): with radius, the number of other finite points within it; with mean_k, the mean distance
        to the mean_k nearest other finite points.  NaN for a point that is not finite.  -> ((n,) float64, stats dict).
        device: the address (an int) of n float64 of the caller's own memory on the handle's device, which then receives
        the values instead: -> (that address, stats dict)."""
        if spec is None:
            spec = self.outlierSpec(radius, min_neighbors, mean_k, stddev_mul)
        n = len(dc)
        st = _lib.OutlierStats()
        if device is not False and device is not None:
            check(self._L.ndt_cloud_neighbor_values(self._h, dc._c, C.byref(spec), C.c_void_p(int(device)), 1, C.byref(st)))
            return int(device), self._outlier_stats(st)
        out = np.zeros(max(n, 1), dtype=np.float64)
        check(self._L.ndt_cloud_neighbor_values(self._h, dc._c, C.byref(spec), C.c_void_p(out.ctypes.data), 0, C.byref(st)))
        return out[:n].copy(), self._outlier_stats(st)

    def removeOutliers(self, dc, radius=None, min_neighbors=None, mean_k=None, stddev_mul=None, negate=False, indices=False,
                       spec=None):
        """The points of the resident cloud `dc` the radius or the statistical outlier filter keeps, in dc's order, as a new
        DeviceCloud with exact boxes (ndt_cloud_remove_outliers); the per-point values stay on the device.
        -> (DeviceCloud, stats dict); indices=True: (DeviceCloud, stats, (n_kept,) int32 indices of the kept points)."""
        if spec is None:
            spec = self.outlierSpec(radius, min_neighbors, mean_k, stddev_mul, negate)
        n = len(dc)
        idx = np.zeros(max(n, 1), dtype=np.int32) if indices else None
        c, nk, st = C.c_void_p(None), C.c_size_t(0), _lib.OutlierStats()
        check(self._L.ndt_cloud_remove_outliers(self._h, dc._c, C.byref(spec), C.byref(c),
                                                idx.ctypes.data_as(C.POINTER(C.c_int32)) if indices else None, C.byref(nk), C.byref(st)))
        out = DeviceCloud(self, c)
        return (out, self._outlier_stats(st), idx[:nk.value].copy()) if indices else (out, self._outlier_stats(st))

    def removeOutliersClouds(self, clouds, radius=None, min_neighbors=None, mean_k=None, stddev_mul=None, negate=False, spec=None):
        """removeOutliers of every DeviceCloud of the list under one spec: one value launch and the selection's two
        (ndt_cloud_remove_outliers_clouds).  -> (list of DeviceCloud, list of stats dicts), entry k what removeOutliers
        gives for clouds[k] alone, the same bits."""
        if spec is None:
            spec = self.outlierSpec(radius, min_neighbors, mean_k, stddev_mul, negate)
        clouds, n, arr = _handle_array(clouds)
        out, nk, st = _out_array(n), (C.c_size_t * max(n, 1))(), (_lib.OutlierStats * max(n, 1))()
        check(self._L.ndt_cloud_remove_outliers_clouds(self._h, arr, n, C.byref(spec), out, nk, st))
        return self._wrap(out, n), [self._outlier_stats(st[k]) for k in range(n)]

    def outlierDiag(self):
        """What the last outlier call that reached the device did (ndt_diag_outliers)."""
        return self._diag(self._L.ndt_diag_outliers, "index_builds", "value_launches", "value_blocks", "scanned_queries")

    @staticmethod
    def outlierPlan(n):
        """(blocks, queries_per_block) of the value kernel over a cloud of n points (ndt_host_outlier_plan; host only)."""
        b, q = C.c_int(0), C.c_int(0)
        check(_lib.lib().ndt_host_outlier_plan(int(n), C.byref(b), C.byref(q)))
        return b.value, q.value

    @staticmethod
    def outlierSpecCheck(spec):
        """Is the _lib.OutlierSpec valid?  (ndt_host_outlier_spec_check; host only.)"""
        return _lib.lib().ndt_host_outlier_spec_check(C.byref(spec)) == _lib.NDT_OK

    # ---- the plane of resident clouds (ndt_cloud_plane_counts / ndt_cloud_segment_plane / _clouds / _plane_distances) ------
    @staticmethod
    def _plane_result(r):
        return dict(found=bool(r.found), refined=bool(r.refined), coeff=np.array(list(r.coeff), dtype=np.float64), best=r.best,
                    best_count=r.best_count, n_inliers=r.n_inliers, n_finite=r.n_finite, n_degenerate=r.n_degenerate,
                    n_rejected=r.n_rejected)

    @staticmethod
    def _plane_triples(triples, spec):
        if triples is None:
            return None, None
        t = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1)
        if t.size != 3 * spec.n_hypotheses:
            raise ValueError("triples must hold 3 * n_hypotheses indices")
        return t, t.ctypes.data_as(C.POINTER(C.c_int32))

    def planeCounts(self, dc, spec, triples=None):
        """Every plane hypothesis of the resident cloud `dc` under the _lib.PlaneSpec (plane_spec(...)), scored against all its
        points (ndt_cloud_plane_counts; defined in include/ndt_mi355.h).  triples: (n_hypotheses, 3) int32 of the caller's own
        in place of the sampler's.  -> (coeffs (H, 4) float64, states (H,) int32: 0 valid, 1 degenerate, 2 rejected,
        counts (H,) uint32)."""
        H = spec.n_hypotheses
        keep, tp = self._plane_triples(triples, spec)
        co, st, cn = np.zeros((max(H, 1), 4), dtype=np.float64), np.zeros(max(H, 1), dtype=np.int32), np.zeros(max(H, 1), dtype=np.uint32)
        check(self._L.ndt_cloud_plane_counts(self._h, dc._c, C.byref(spec), tp, _d(co), st.ctypes.data_as(C.POINTER(C.c_int32)),
                                             cn.ctypes.data_as(C.POINTER(C.c_uint32))))
        return co[:H], st[:H], cn[:H]

    def segmentPlane(self, dc, spec, triples=None, inliers=True, others=True):
        """The dominant plane of the resident cloud `dc` by RANSAC over spec.n_hypotheses hypotheses, every one scored
        (ndt_cloud_segment_plane).  -> (result dict, DeviceCloud of the inliers or None, DeviceCloud of the other finite points
        or None), both in dc's order with exact boxes; the signed distances stay on the device."""
        keep, tp = self._plane_triples(triples, spec)
        r, ci, co = _lib.PlaneResult(), C.c_void_p(None), C.c_void_p(None)
        check(self._L.ndt_cloud_segment_plane(self._h, dc._c, C.byref(spec), tp, C.byref(r), C.byref(ci) if inliers else None,
                                              C.byref(co) if others else None))
        return self._plane_result(r), DeviceCloud(self, ci) if inliers else None, DeviceCloud(self, co) if others else None

    def segmentPlaneClouds(self, clouds, spec, inliers=True, others=True):
        """segmentPlane of every DeviceCloud of the list under one spec, every cloud its own plane, in one model launch, one
        count launch and the selection's launches in all (ndt_cloud_segment_plane_clouds).  -> (list of result dicts, list of
        inlier clouds or None, list of other clouds or None), entry k what segmentPlane gives for clouds[k] alone."""
        clouds, n, arr = _handle_array(clouds)
        res = (_lib.PlaneResult * max(n, 1))()
        oi, oo = _out_array(n), _out_array(n)
        check(self._L.ndt_cloud_segment_plane_clouds(self._h, arr, n, C.byref(spec), res, oi if inliers else None, oo if others else None))
        return [self._plane_result(res[k]) for k in range(n)], self._wrap(oi, n) if inliers else None, self._wrap(oo, n) if others else None

    def planeDistances(self, dc, coeff, device=False):
        """The signed distance of every point of the resident cloud `dc` from the plane coeff = (nx, ny, nz, d) -- the height
        above a ground plane (ndt_cloud_plane_distances); NaN for a point that is not finite.  -> (n,) float64.  device: the
        address (an int) of n float64 on the handle's device, which then receives the values: -> that address."""
        c = np.ascontiguousarray(coeff, dtype=np.float64).reshape(4)
        n = len(dc)
        if device is not False and device is not None:
            check(self._L.ndt_cloud_plane_distances(self._h, dc._c, _d(c), C.c_void_p(int(device)), 1))
            return int(device)
        out = np.zeros(max(n, 1), dtype=np.float64)
        check(self._L.ndt_cloud_plane_distances(self._h, dc._c, _d(c), C.c_void_p(out.ctypes.data), 0))
        return out[:n].copy()

    def planeDiag(self):
        """What the last plane call that reached the device did (ndt_diag_plane)."""
        return self._diag(self._L.ndt_diag_plane, "launches", "select_launches", "count_blocks", "clouds")

    # ---- Euclidean cluster extraction of resident clouds (ndt_cloud_cluster / ndt_cloud_extract_clusters / _clouds) ----------
    CLUSTER_DTYPE = np.dtype([("root", np.int32), ("size", np.int32), ("first", np.uint32), ("box_min", np.float32, 3),
                              ("box_max", np.float32, 3), ("centroid", np.float64, 3)], align=True)

    @staticmethod
    def clusterSpec(tolerance, min_size=1, max_size=None):
        """The ndt_cluster_spec of the keyword form: points nearer than `tolerance` belong together; a component of
        min_size ... max_size points (max_size None: no upper limit) is a cluster."""
        s = _lib.ClusterSpec()
        s.tolerance, s.min_size, s.max_size = float(np.float32(tolerance)), int(min_size), int(2 ** 31 - 1 if max_size is None else max_size)
        return s

    @staticmethod
    def _cluster_summary(st):
        return dict(n_finite=st.n_finite, n_components=st.n_components, n_clusters=st.n_clusters, n_clustered=st.n_clustered,
                    largest=st.largest)

    def clusterCloud(self, dc, tolerance=None, min_size=1, max_size=None, capacity=None, indices=True, roots=False, device=False,
                     spec=None):
        """The Euclidean clusters of the resident cloud `dc` (ndt_cloud_cluster; defined in include/ndt_mi355.h): the connected
        components of "nearer than tolerance" over the finite points whose size lies in min_size ... max_size, numbered by
        descending size (equal sizes: by their smallest point index).
        -> (labels (n,) int32: the cluster number, -1 in no cluster or not finite; table: a structured array (CLUSTER_DTYPE:
        root, size, first, box_min, box_max, centroid) of the min(C, capacity) largest clusters -- capacity None: all of them;
        indices (n_clustered,) int32: the clustered points grouped by cluster, ascending inside one, row c of the table
        covering indices[first : first + size], or None with indices=False; summary dict).  roots=True adds the (n,) int32
        roots -- the smallest index of every point's component, -1 for a point that is not finite -- as a fifth entry.
        device: the address (an int) of n int32 on the handle's device (with roots=True of 2 n: labels, then roots), which
        then receives the labels instead; the first entry is that address.
        One cluster's cloud is selectCloud(dc, keys=labels, key_range=(c, c)).  spec: a ready _lib.ClusterSpec."""
        if spec is None:
            spec = self.clusterSpec(tolerance, min_size, max_size)
        n = len(dc)
        st = _lib.ClusterSummary()
        on_device = device is not False and device is not None
        idx = np.zeros(max(n, 1), dtype=np.int32) if indices else None
        ip32 = C.POINTER(C.c_int32)
        if on_device:
            lp, rp = C.c_void_p(int(device)), C.c_void_p(int(device) + 4 * n) if roots else None
        else:
            lab = np.full(max(n, 1), -1, dtype=np.int32)
            rts = np.full(max(n, 1), -1, dtype=np.int32) if roots else None
            lp, rp = C.c_void_p(lab.ctypes.data), C.c_void_p(rts.ctypes.data) if roots else None

        if capacity is None:  # as many rows as there are clusters: at most one per min_size points
            capacity = n // max(spec.min_size, 1)
        capacity = int(capacity)
        rows = np.zeros(max(capacity, 1) * self.CLUSTER_DTYPE.itemsize, dtype=np.uint8)  # (bytes: a copy keeps a row's padding too)
        check(self._L.ndt_cloud_cluster(self._h, dc._c, C.byref(spec), lp, int(on_device), rp,
                                        rows.ctypes.data_as(C.POINTER(_lib.ClusterInfo)) if capacity else None, capacity,
                                        idx.ctypes.data_as(ip32) if indices else None, C.byref(st)))
        table = rows[:min(capacity, st.n_clusters) * self.CLUSTER_DTYPE.itemsize].copy().view(self.CLUSTER_DTYPE)
        out = [int(device) if on_device else lab[:n].copy(), table, idx[:st.n_clustered].copy() if indices else None, self._cluster_summary(st)]
        if roots:
            out.append(int(device) + 4 * n if on_device else rts[:n].copy())
        return tuple(out)

    def extractClusters(self, dc, tolerance=None, min_size=1, max_size=None, negate=False, indices=False, spec=None):
        """The points of the resident cloud `dc` that belong to a cluster (clusterCloud's label >= 0; negate: the finite points
        that belong to none), in dc's order, as a new DeviceCloud with exact boxes (ndt_cloud_extract_clusters); the per-point
        keys stay on the device, and no cluster is numbered.
        -> (DeviceCloud, summary dict); indices=True: (DeviceCloud, summary, (n_kept,) int32 indices of the kept points)."""
        if spec is None:
            spec = self.clusterSpec(tolerance, min_size, max_size)
        n = len(dc)
        idx = np.zeros(max(n, 1), dtype=np.int32) if indices else None
        c, nk, st = C.c_void_p(None), C.c_size_t(0), _lib.ClusterSummary()
        check(self._L.ndt_cloud_extract_clusters(self._h, dc._c, C.byref(spec), int(bool(negate)), C.byref(c),
                                                 idx.ctypes.data_as(C.POINTER(C.c_int32)) if indices else None, C.byref(nk), C.byref(st)))
        out = DeviceCloud(self, c)
        return (out, self._cluster_summary(st), idx[:nk.value].copy()) if indices else (out, self._cluster_summary(st))

    def extractClustersClouds(self, clouds, tolerance=None, min_size=1, max_size=None, negate=False, spec=None):
        """extractClusters of every DeviceCloud of the list under one spec: every kernel of the extraction launched once, and
        the selection's two (ndt_cloud_extract_clusters_clouds).  -> (list of DeviceCloud, list of summary dicts), entry k
        what extractClusters gives for clouds[k] alone, the same bits."""
        if spec is None:
            spec = self.clusterSpec(tolerance, min_size, max_size)
        clouds, n, arr = _handle_array(clouds)
        out, nk, st = _out_array(n), (C.c_size_t * max(n, 1))(), (_lib.ClusterSummary * max(n, 1))()
        check(self._L.ndt_cloud_extract_clusters_clouds(self._h, arr, n, C.byref(spec), int(bool(negate)), out, nk, st))
        return self._wrap(out, n), [self._cluster_summary(st[k]) for k in range(n)]

    def diagClusters(self):
        """What the last cluster call that reached the device did (ndt_diag_clusters)."""
        return self._diag(self._L.ndt_diag_clusters, "index_builds", "launches", "link_blocks", "scanned_queries", "cas_retries")

    @staticmethod
    def clusterPlan(n):
        """(blocks, queries_per_block) of the link kernel over a cloud of n points (ndt_host_cluster_plan; host only)."""
        b, q = C.c_int(0), C.c_int(0)
        check(_lib.lib().ndt_host_cluster_plan(int(n), C.byref(b), C.byref(q)))
        return b.value, q.value

    @staticmethod
    def clusterSpecCheck(spec):
        """Is the _lib.ClusterSpec valid?  (ndt_host_cluster_spec_check; host only.)"""
        return _lib.lib().ndt_host_cluster_spec_check(C.byref(spec)) == _lib.NDT_OK

    # ---- surface normals and curvature of resident clouds (ndt_cloud_estimate_normals / ndt_cloud_select_by_normals) ------
    @staticmethod
    def normalSpec(k=None, radius=None, min_neighbors=3, viewpoint=(0.0, 0.0, 0.0)):
        """The ndt_normal_spec of the keyword form: the k nearest neighbours (the point itself included), or every point within
        `radius`; fewer than min_neighbors members: no normal; normals point towards `viewpoint`."""
        if (k is None) == (radius is None):
            raise ValueError("give either k or radius")
        s = _lib.NormalSpec()
        s.method = _lib.NORMAL_KNN if k is not None else _lib.NORMAL_RADIUS
        s.k, s.radius, s.min_neighbors = int(k or 0), float(np.float32(radius or 0.0)), int(min_neighbors)
        s.viewpoint[:] = [float(v) for v in viewpoint]
        return s

    @staticmethod
    def normalFilter(curvature=None, axis=None, cos=None, negate=False):
        """The ndt_normal_filter of the keyword form: curvature = (lo, hi) keeps lo <= curvature <= hi; axis (a unit vector)
        with cos = (lo, hi) keeps lo <= |n . axis| <= hi; negate inverts the outcome for the points that have a normal."""
        f = _lib.NormalFilter()
        if curvature is not None:
            f.flags |= _lib.NORMAL_KEEP_CURVATURE
            f.curvature_lo, f.curvature_hi = float(np.float32(curvature[0])), float(np.float32(curvature[1]))
        if axis is not None:
            f.flags |= _lib.NORMAL_KEEP_ANGLE
            f.axis[:] = [float(v) for v in axis]
            f.cos_lo, f.cos_hi = (0.0, 1.0) if cos is None else (float(cos[0]), float(cos[1]))
        if negate:
            f.flags |= _lib.NORMAL_KEEP_NEGATE
        return f

    @staticmethod
    def _normal_stats(st):
        return dict(n_finite=st.n_finite, n_valid=st.n_valid, n_collinear=st.n_collinear, max_neighbors=st.max_neighbors)

    def estimateNormals(self, dc, k=None, radius=None, min_neighbors=3, viewpoint=(0.0, 0.0, 0.0), counts=True, device=False, spec=None):
        """Unit normal and surface variation of every point of the resident cloud `dc` (ndt_cloud_estimate_normals; defined in
        include/ndt_mi355.h).  -> (normals (n, 4) float32: nx, ny, nz, curvature -- four NaNs where there is no normal;
        counts (n,) int32: the neighbours of every point, or None with counts=False; stats dict).
        device: the address (an int) of 4 n float32 on the handle's device (with counts=True followed by n int32), which then
        receives the outputs; the first entry is that address, the second the address of the counts or None."""
        if spec is None:
            spec = self.normalSpec(k, radius, min_neighbors, viewpoint)
        n = len(dc)
        st = _lib.NormalStats()
        if device is not False and device is not None:
            np_, cp = int(device), int(device) + 16 * n if counts else None
            check(self._L.ndt_cloud_estimate_normals(self._h, dc._c, C.byref(spec), C.c_void_p(np_), C.c_void_p(cp) if counts else None, 1,
                                                     C.byref(st)))
            return np_, cp, self._normal_stats(st)
        nr = np.zeros((max(n, 1), 4), dtype=np.float32)
        ct = np.zeros(max(n, 1), dtype=np.int32) if counts else None
        check(self._L.ndt_cloud_estimate_normals(self._h, dc._c, C.byref(spec), C.c_void_p(nr.ctypes.data),
                                                 C.c_void_p(ct.ctypes.data) if counts else None, 0, C.byref(st)))
        return nr[:n].copy(), ct[:n].copy() if counts else None, self._normal_stats(st)

    def estimateNormalsClouds(self, clouds, k=None, radius=None, min_neighbors=3, viewpoint=(0.0, 0.0, 0.0), counts=True, spec=None):
        """estimateNormals of every DeviceCloud of the list under one spec in ONE normals launch
        (ndt_cloud_estimate_normals_clouds).  -> (list of (n_k, 4) float32, list of (n_k,) int32 or None, list of stats dicts),
        entry k what estimateNormals gives for clouds[k] alone, the same bits."""
        if spec is None:
            spec = self.normalSpec(k, radius, min_neighbors, viewpoint)
        clouds, n, arr = _handle_array(clouds)
        sizes = [len(c) for c in clouds]
        first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        total = int(first[-1])
        nr = np.zeros((max(total, 1), 4), dtype=np.float32)
        ct = np.zeros(max(total, 1), dtype=np.int32) if counts else None
        st = (_lib.NormalStats * max(n, 1))()
        check(self._L.ndt_cloud_estimate_normals_clouds(self._h, arr, n, C.byref(spec), C.c_void_p(nr.ctypes.data),
                                                        C.c_void_p(ct.ctypes.data) if counts else None, 0, st))
        return ([nr[first[j]:first[j + 1]].copy() for j in range(n)],
                [ct[first[j]:first[j + 1]].copy() for j in range(n)] if counts else None, [self._normal_stats(st[j]) for j in range(n)])

    def selectByNormals(self, dc, spec, filter=None, indices=False):
        """The points of the resident cloud `dc` whose normal record passes the _lib.NormalFilter (normalFilter(...); None: every
        point that has a normal), in dc's order, as a new DeviceCloud with exact boxes (ndt_cloud_select_by_normals); normals
        and keys stay on the device.
        -> (DeviceCloud, stats dict); indices=True: (DeviceCloud, stats, (n_kept,) int32 indices of the kept points)."""
        if filter is None:
            filter = _lib.NormalFilter()
        n = len(dc)
        idx = np.zeros(max(n, 1), dtype=np.int32) if indices else None
        c, nk, st = C.c_void_p(None), C.c_size_t(0), _lib.NormalStats()
        check(self._L.ndt_cloud_select_by_normals(self._h, dc._c, C.byref(spec), C.byref(filter), C.byref(c),
                                                  idx.ctypes.data_as(C.POINTER(C.c_int32)) if indices else None, C.byref(nk), C.byref(st)))
        out = DeviceCloud(self, c)
        return (out, self._normal_stats(st), idx[:nk.value].copy()) if indices else (out, self._normal_stats(st))

    def selectByNormalsClouds(self, clouds, spec, filter=None):
        """selectByNormals of every DeviceCloud of the list under one spec and filter: one normals launch and the selection's
        two (ndt_cloud_select_by_normals_clouds).  -> (list of DeviceCloud, list of stats dicts), entry k what selectByNormals
        gives for clouds[k] alone, the same bits."""
        if filter is None:
            filter = _lib.NormalFilter()
        clouds, n, arr = _handle_array(clouds)
        out, nk, st = _out_array(n), (C.c_size_t * max(n, 1))(), (_lib.NormalStats * max(n, 1))()
        check(self._L.ndt_cloud_select_by_normals_clouds(self._h, arr, n, C.byref(spec), C.byref(filter), out, nk, st))
        return self._wrap(out, n), [self._normal_stats(st[j]) for j in range(n)]

    def normalDiag(self):
        """What the last normals call that reached the device did (ndt_diag_normals)."""
        return self._diag(self._L.ndt_diag_normals, "index_builds", "launches", "blocks", "scanned_queries")

    @staticmethod
    def normalPlan(n):
        """(blocks, queries_per_block) of the normals kernel over a cloud of n points (ndt_host_normal_plan; host only)."""
        b, q = C.c_int(0), C.c_int(0)
        check(_lib.lib().ndt_host_normal_plan(int(n), C.byref(b), C.byref(q)))
        return b.value, q.value

    @staticmethod
    def normalSpecCheck(spec):
        """Is the _lib.NormalSpec valid?  (ndt_host_normal_spec_check; host only.)"""
        return _lib.lib().ndt_host_normal_spec_check(C.byref(spec)) == _lib.NDT_OK

    @staticmethod
    def normalFilterCheck(filter):
        """Is the _lib.NormalFilter valid?  (ndt_host_normal_filter_check; host only.)"""
        return _lib.lib().ndt_host_normal_filter_check(C.byref(filter)) == _lib.NDT_OK

    # ---- pose covariance (ndt_pose_covariance / ndt_pairs_pose_covariances) ----------------------------------------------
    def poseCovariance(self, transform=None, method="sandwich", scale=1.0, info=False):
        """6x6 covariance of the pose x y z roll pitch yaw of the input source at `transform` (None: the last align's final
        transformation): method "sandwich" = A^-1 B_c A^-1 (no tuning constant) or "laplace" = scale A^-1.  All NaN when the
        pose is not determined (fewer than 6 points found, or A not positive definite).  info=True: (cov, dict with A, B, g,
        n_found, eig_min, eig_max, indefinite)."""
        T = None if transform is None else _colmajor(transform)
        cov = np.zeros(36)
        I = _lib.PoseInformation()
        check(self._L.ndt_pose_covariance(self._h, _f(T) if T is not None else None, _cov_method(method), float(scale), _d(cov),
                                          C.byref(I)))
        cov = cov.reshape(6, 6)
        return (cov, _pose_information(I)) if info else cov

    def pairsPoseCovariances(self, transforms=None, method="sandwich", scale=1.0, info=False):
        """poseCovariance of every pair of the last alignPairs, all pairs in one launch of the gradient kernel: pair k's source
        at transforms[k] (None = that call's final transformations) against pair k's target.  (P, 6, 6); info=True: also a
        list of P dicts."""
        T = None
        if transforms is not None:
            T = np.ascontiguousarray(np.stack([_colmajor(x) for x in transforms]), dtype=np.float32)
        n = C.c_size_t(0)
        check(self._L.ndt_pairs_count(self._h, C.byref(n)))
        P = n.value
        if T is not None and T.shape[0] != P:
            raise ValueError("one transform per pair of the last alignPairs")
        cov = np.zeros((max(P, 1), 36))
        I = (_lib.PoseInformation * max(P, 1))()
        check(self._L.ndt_pairs_pose_covariances(self._h, _f(T) if T is not None else None, _cov_method(method), float(scale),
                                                 _d(cov), C.cast(I, C.c_void_p)))
        cov = cov[:P].reshape(P, 6, 6).copy()
        return (cov, [_pose_information(I[k]) for k in range(P)]) if info else cov

    def poseCovarianceLaunches(self):
        """(gradient-kernel launches, blocks that worked) of the last pose covariance call that reached the device."""
        return tuple(self._diag(self._L.ndt_diag_pose_covariance, "launches", "blocks").values())

    def alignGuesses(self, guesses):
        """Register the input source from each of the 4x4 guesses in lock-step (ndt_align_guesses).  Returns alignBatch's
        dict, one entry per guess, plus best = index of the largest transformation probability (-1 if none)."""
        g = self._pose_table(guesses)
        G = g.shape[0]
        T = np.zeros((max(G, 1), 16), dtype=np.float32)
        conv = np.zeros(max(G, 1), dtype=np.int32)
        it = np.zeros(max(G, 1), dtype=np.int32)
        tp = np.zeros(max(G, 1), dtype=np.float64)
        best = C.c_int(-1)
        check(self._L.ndt_align_guesses(self._h, _f(g) if G else None, G, _f(T), _i(conv), _i(it), _d(tp), C.byref(best)))
        return dict(T=np.stack([_from_colmajor(T[k]) for k in range(G)]) if G else np.zeros((0, 4, 4), np.float32),
                    converged=conv[:G].astype(bool), iterations=it[:G].copy(), trans_probability=tp[:G].copy(), best=best.value)

    def alignMultistart(self, candidates, keep, metric="score"):
        """scorePoses over the candidates, the `keep` best of them (host_pick_top) as the guesses of one alignGuesses
        (ndt_align_multistart).  Returns alignGuesses' dict over the picked members, plus picked = their candidate indices;
        best indexes the candidates.  metric="nvtl": the candidates are ranked by nvtlPoses instead (composed here from
        nvtlPoses, host_pick_top and alignGuesses)."""
        if metric not in ("score", "nvtl"):
            raise ValueError("metric must be 'score' or 'nvtl'")
        c = self._pose_table(candidates)
        n, keep = c.shape[0], int(keep)
        if keep < 0:
            raise ValueError("keep must be >= 0")
        if metric == "nvtl":
            cand = c.reshape(-1, 4, 4).transpose(0, 2, 1)
            picked = host_pick_top(self.nvtlPoses(cand), keep) if n and keep else np.zeros(0, dtype=np.int32)
            r = self.alignGuesses(cand[picked])
            r["picked"] = picked
            r["best"] = int(picked[r["best"]]) if r["best"] >= 0 else -1
            return r
        room = max(min(keep, n), 1)
        picked = np.zeros(room, dtype=np.int32)
        T = np.zeros((room, 16), dtype=np.float32)
        conv = np.zeros(room, dtype=np.int32)
        it = np.zeros(room, dtype=np.int32)
        tp = np.zeros(room, dtype=np.float64)
        n_picked, best = C.c_size_t(0), C.c_int(-1)
        check(self._L.ndt_align_multistart(self._h, _f(c) if n else None, n, keep, _i(picked), C.byref(n_picked), _f(T), _i(conv),
                                           _i(it), _d(tp), C.byref(best)))
        P = n_picked.value
        return dict(T=np.stack([_from_colmajor(T[k]) for k in range(P)]) if P else np.zeros((0, 4, 4), np.float32),
                    converged=conv[:P].astype(bool), iterations=it[:P].copy(), trans_probability=tp[:P].copy(),
                    picked=picked[:P].copy(), best=best.value)

    def pairsGrid(self, c):
        """The grid the last alignPairs built for target cloud c, in the layout of grid()."""
        nl, nv = C.c_size_t(0), C.c_size_t(0)
        check(self._L.ndt_pairs_grid_size(self._h, int(c), C.byref(nl), C.byref(nv)))
        n = nl.value
        idx = np.zeros(n, dtype=np.int64)
        npts = np.zeros(n, dtype=np.int32)
        mean = np.zeros((n, 3))
        cov = np.zeros((n, 3, 3))
        icov = np.zeros((n, 3, 3))
        evals = np.zeros((n, 3))
        if n:
            check(self._L.ndt_pairs_grid_dump(self._h, int(c), idx.ctypes.data_as(C.POINTER(C.c_int64)), _i(npts), _d(mean),
                                              _d(cov), _d(icov), _d(evals)))
        mb, xb, db = (np.zeros(3, dtype=np.int32) for _ in range(3))
        check(self._L.ndt_pairs_grid_info(self._h, int(c), _i(mb), _i(xb), _i(db)))
        return dict(idx=idx, n=npts, mean=mean, cov=cov, icov=icov, evals=evals, min_b=mb, max_b=xb, div_b=db,
                    n_valid=nv.value)

    def alignBatchSharded(self, clouds=None, first_scan=0, total_scans=None, guesses=None, device_ptr=None, offsets=None,
                          stride_bytes=16):
        """The lock-step batch with the scans sharded over ranks (ndt_align_batch_sharded*): this rank holds scans
        [first_scan, first_scan + n_local) of total_scans; needs a communicator (commInitRank) or an all-reduce hook.
        Outputs cover all total_scans scans and are identical on every rank."""
        if clouds is not None:
            cat = _cloud(np.concatenate(clouds, axis=0)) if clouds else np.zeros((0, 4), np.float32)
            offsets = np.zeros(len(clouds) + 1, dtype=np.uintp)
            offsets[1:] = np.cumsum([c.shape[0] for c in clouds])
            ptr, stride, fn = cat.ctypes.data, cat.shape[1] * 4, self._L.ndt_align_batch_sharded
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.uintp)
            ptr, stride, fn = C.c_void_p(device_ptr), stride_bytes, self._L.ndt_align_batch_sharded_device
        n_local = len(offsets) - 1
        B = int(total_scans if total_scans is not None else n_local)
        g = None
        if guesses is not None:
            g = np.ascontiguousarray(np.stack([_colmajor(x) for x in guesses]))
            assert g.shape[0] == B
        T = np.zeros((B, 16), dtype=np.float32)
        conv = np.zeros(B, dtype=np.int32)
        it = np.zeros(B, dtype=np.int32)
        tp = np.zeros(B, dtype=np.float64)
        check(fn(self._h, ptr, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), n_local, int(first_scan), B, stride,
                 _f(g) if g is not None else None, _f(T), _i(conv), _i(it), _d(tp)))
        return dict(T=np.stack([_from_colmajor(T[k]) for k in range(B)]), converged=conv.astype(bool),
                    iterations=it, trans_probability=tp)

    # ---- multi-GPU: native RCCL communicator (ndt_comm_*) -----------------------------
    def commInitRank(self, unique_id, rank, world_size):
        """unique_id: the COMM_ID_BYTES bytes rank 0 got from comm_get_unique_id()."""
        buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        check(self._L.ndt_comm_init_rank(self._h, C.cast(buf, C.c_void_p), int(rank), int(world_size)))

    def commDestroy(self):
        check(self._L.ndt_comm_destroy(self._h))

    def commStats(self):
        r, w, ls = C.c_int(0), C.c_int(0), C.c_int(0)
        n = C.c_longlong(0)
        check(self._L.ndt_comm_stats(self._h, C.byref(r), C.byref(w), C.byref(n), C.byref(ls)))
        return dict(rank=r.value, world=w.value, collectives=n.value, lock_steps=ls.value)

    def shareInputSource(self, donor):
        """Register the source cloud `donor` has uploaded (ndt_share_input_source)."""
        check(self._L.ndt_share_input_source(self._h, donor._h))

    def shareInputTarget(self, donor):
        """Take the target cloud and the voxel grid `donor` built (no copy, no rebuild)."""
        check(self._L.ndt_share_input_target(self._h, donor._h))

    def setCuPartition(self, partition):
        """0 whole device, 1 registration partition, 2 side partition (ndt_set_cu_partition)."""
        check(self._L.ndt_set_cu_partition(self._h, int(partition)))

    def getCuPartition(self):
        a, b = C.c_int(0), C.c_int(0)
        check(self._L.ndt_get_cu_partition(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def setInputSourceRaw(self, host_ptr, n, stride_bytes=16):
        """setInputSource from a raw host pointer (e.g. the page-locked buffer of a PcdSequence scan)."""
        check(self._L.ndt_set_input_source(self._h, C.c_void_p(host_ptr), n, stride_bytes))

    def setVoxelIndex(self, mode):
        """0 = dense / sparse voxel index chosen by occupancy, 1 = dense table, 2 = sparse (sorted build + hash look-up)."""
        check(self._L.ndt_set_voxel_index(self._h, int(mode)))

    def setBatchGroups(self, n):
        """Independent lock-step groups alignBatch runs as (0 = automatic, 1 = one loop)."""
        check(self._L.ndt_set_batch_groups(self._h, int(n)))

    def setAllreduce(self, fn, on_device=False):
        """fn(buffer_address, n_doubles, on_device) -> 0 on success; None removes the hook."""
        if fn is None:
            cb = _lib.ALLREDUCE_FN(0)
        else:
            def tramp(buf, n, dev, _user):
                try:
                    return int(fn(buf, n, bool(dev)) or 0)
                except Exception:  # never unwind through C
                    import traceback
                    traceback.print_exc()
                    return 1
            cb = _lib.ALLREDUCE_FN(tramp)
        self._keep = [cb]
        check(self._L.ndt_set_allreduce(self._h, cb, None, int(on_device)))

    def diag_stamps(self, p, max_waves=1 << 16):
        p = np.ascontiguousarray(p, dtype=np.float64)
        st = np.zeros((max_waves, 8), dtype=np.uint64)
        n = C.c_size_t(max_waves)
        check(self._L.ndt_diag_stamps(self._h, _d(p), st.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(n)))
        return st[:n.value]

    def evalPlan(self, n):
        """How this handle cuts an evaluation of n source points (ndt_diag_eval_plan): dict of ppb, fused_blocks,
        launch_blocks, server_blocks, batch_blocks."""
        v = [C.c_int(0) for _ in range(5)]
        check(self._L.ndt_diag_eval_plan(self._h, int(n), *[C.byref(x) for x in v]))
        return dict(zip(EVAL_PLAN_FIELDS, (x.value for x in v)))

    def gridBuild(self):
        """What built this handle's target grid (ndt_diag_grid_build): dict of form (a name of GRID_FORMS), n_points, n_cells,
        the stored plan, the finish's wmax / lds_cap, lut_cells, the compaction's tile plan and compact_pending."""
        form, nb, cpb, ppb, blk, wmax, cap, items, prefix, pending = (C.c_int(0) for _ in range(10))
        n = C.c_size_t(0)
        cells, lut, tiles = (C.c_longlong(0) for _ in range(3))
        check(self._L.ndt_diag_grid_build(self._h, C.byref(form), C.byref(n), C.byref(cells), C.byref(nb), C.byref(cpb), C.byref(ppb),
                                          C.byref(blk), C.byref(wmax), C.byref(cap), C.byref(lut), C.byref(items), C.byref(tiles),
                                          C.byref(prefix), C.byref(pending)))
        return dict(form=GRID_FORMS[form.value], n_points=n.value, n_cells=cells.value, n_buckets=nb.value,
                    cells_per_bucket=cpb.value, pts_per_block=ppb.value, n_blocks=blk.value, wmax=wmax.value, lds_cap=cap.value,
                    lut_cells=lut.value, compact_items=items.value, compact_tiles=tiles.value, compact_prefix=bool(prefix.value),
                    compact_pending=bool(pending.value))

    def diag_server_roundtrip(self, p, n_iter=200):
        p = np.ascontiguousarray(p, dtype=np.float64)
        us = np.zeros(3)
        check(self._L.ndt_diag_server_roundtrip(self._h, _d(p), n_iter, _d(us)))
        return dict(nop_us=us[0], no_hessian_us=us[1], with_hessian_us=us[2])

    def diag_selfdrive(self, p, rounds=200):
        """Rounds driven from the device (no host in the loop, no solver step): us per round without / with the body."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        us = np.zeros(2)
        check(self._L.ndt_diag_selfdrive(self._h, _d(p), rounds, _d(us)))
        return dict(protocol_only_us=us[0], with_hessian_body_us=us[1])

    def selftest_reduce(self, n_blocks=3):
        out = np.zeros((n_blocks, _lib.EVAL_STRIDE))
        check(self._L.ndt_selftest_reduce(self._h, n_blocks, _d(out)))
        return out

    def selftest_server_idle(self, p, stall_ms):
        p = np.ascontiguousarray(p, dtype=np.float64)
        served = C.c_int(-1)
        scores = np.zeros(3)
        check(self._L.ndt_selftest_server_idle(self._h, _d(p), int(stall_ms), C.byref(served), _d(scores)))
        return bool(served.value), scores

    def setEvaluationPath(self, persistent):
        """True (default): one persistent kernel per registration; False: one launch per evaluation."""
        check(self._L.ndt_set_evaluation_path(self._h, int(bool(persistent))))

    def setEvaluationReuse(self, on):
        """True (default, NDT_EVAL_REUSE): a request that repeats the last answered one of its kind byte for byte is not
        sent to the device again (the trials a line search repeats at an unchanged pose); same results, same stats()."""
        check(self._L.ndt_set_evaluation_reuse(self._h, int(bool(on))))

    def evalReuse(self):
        """(served, reused) of the last align / batch / pairs call: evaluations the device answered, summed over the
        members, and steps the solvers fed themselves; served + reused == n_evals + n_hessian_recomputes of stats()."""
        served, reused = C.c_longlong(0), C.c_longlong(0)
        check(self._L.ndt_diag_eval_reuse(self._h, C.byref(served), C.byref(reused)))
        return served.value, reused.value

    def evalServer(self, p, kind, n_times=2):
        """The evaluation of `kind` (0, 1, 2 = f64 Hessian) at pose p asked n_times of one running evaluation server
        (ndt_diag_eval_server) -> (n_times, 43) float64: score, g[6], H[36]."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        rows = np.zeros((int(n_times), 43))
        check(self._L.ndt_diag_eval_server(self._h, _d(p), int(kind), int(n_times), _d(rows)))
        return rows

    def profile(self, on):
        check(self._L.ndt_profile_enable(self._h, int(on)))

    def profile_read(self, kind=0, reset=True):
        """(launches, total_ms) of the kernel of `kind` (0/1/2: per-evaluation launches of profile(1);
        3: the per-registration persistent kernel of profile(2)), from HIP events on the handle's stream."""
        n = C.c_longlong(0)
        ms = C.c_double(0)
        check(self._L.ndt_profile_read(self._h, kind, C.byref(n), C.byref(ms), int(reset)))
        return n.value, ms.value

    # ---- inspection ------------------------------------------------------------------
    def eval(self, p, compute_hessian=True, T=None):
        p = np.ascontiguousarray(p, dtype=np.float64)
        score, nn = C.c_double(0), C.c_double(0)
        g = np.zeros(6)
        H = np.zeros(36) if compute_hessian else None
        if T is None:
            check(self._L.ndt_eval(self._h, _d(p), C.byref(score), _d(g), _d(H) if compute_hessian else None,
                                   C.byref(nn)))
        else:
            Tc = _colmajor(T)
            check(self._L.ndt_eval_with_matrix(self._h, _f(Tc), _d(p), C.byref(score), _d(g),
                                               _d(H) if compute_hessian else None, C.byref(nn)))
        return score.value, g, (H.reshape(6, 6) if compute_hessian else None), nn.value

    def hessian_f64(self, p):
        p = np.ascontiguousarray(p, dtype=np.float64)
        H = np.zeros(36)
        check(self._L.ndt_eval_hessian_f64(self._h, _d(p), _d(H)))
        return H.reshape(6, 6)

    def grid_counts(self):
        """Occupied / valid voxel counts of the target grid."""
        nl, nv = C.c_size_t(0), C.c_size_t(0)
        check(self._L.ndt_grid_size(self._h, C.byref(nl), C.byref(nv)))
        return dict(n_leaves=nl.value, n_valid=nv.value)

    def grid(self):
        nl, nv = C.c_size_t(0), C.c_size_t(0)
        check(self._L.ndt_grid_size(self._h, C.byref(nl), C.byref(nv)))
        n = nl.value
        idx = np.zeros(n, dtype=np.int64)
        npts = np.zeros(n, dtype=np.int32)
        mean = np.zeros((n, 3))
        cov = np.zeros((n, 3, 3))
        icov = np.zeros((n, 3, 3))
        evals = np.zeros((n, 3))
        if n:
            check(self._L.ndt_grid_dump(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), _i(npts), _d(mean), _d(cov),
                                        _d(icov), _d(evals)))
        mb, xb, db = (np.zeros(3, dtype=np.int32) for _ in range(3))
        check(self._L.ndt_grid_info(self._h, _i(mb), _i(xb), _i(db)))
        return dict(idx=idx, n=npts, mean=mean, cov=cov, icov=icov, evals=evals, min_b=mb, max_b=xb, div_b=db,
                    n_valid=nv.value)


def comm_get_unique_id():
    """ncclGetUniqueId through the C-ABI (rank 0): COMM_ID_BYTES bytes to carry to every rank."""
    buf = (C.c_char * COMM_ID_BYTES)()
    check(_lib.lib().ndt_comm_get_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf.raw)


# ---- host-only scalar pieces (no GPU needed) ---------------------------------------
def host_solve6(H, b):
    H = np.ascontiguousarray(H, dtype=np.float64).reshape(36)
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros(6)
    _lib.lib().ndt_host_solve6(_d(H), _d(b), _d(x))
    return x


def pcd_read_xyz(path):
    """loadPCDFile<PointXYZ> through the C-ABI: ((N, 3) float32, is_dense)."""
    L = _lib.lib()
    n, nf, kind = C.c_size_t(0), C.c_int(0), C.c_int(0)
    check(L.ndt_pcd_read_header(os.fsencode(path), C.byref(n), C.byref(nf), C.byref(kind)))
    out = np.zeros((max(n.value, 1), 4), dtype=np.float32)
    dense = C.c_int(1)
    check(L.ndt_pcd_read_xyz(os.fsencode(path), out.ctypes.data, n.value, 16, C.byref(n), C.byref(dense)))
    return out[:n.value, :3].copy(), bool(dense.value)


def pcd_write_xyz(path, xyz, binary=True):
    a = _cloud(xyz)
    check(_lib.lib().ndt_pcd_write_xyz(os.fsencode(path), a.ctypes.data, a.shape[0], a.shape[1] * 4, int(binary)))


def host_chain_pose(pose, transform):
    """pose * transform in Eigen's f32 rounding (the nodes' trajectory chaining)."""
    out = np.zeros(16, dtype=np.float32)
    _lib.lib().ndt_host_chain_pose(_f(_colmajor(pose)), _f(_colmajor(transform)), _f(out))
    return _from_colmajor(out)


def host_lattice(leaf, mn, mx, voxel_index=0, n_points=0):
    """The voxel lattice of pitch leaf over the box [mn, mx] (ndt_host_lattice): status, min_b, max_b, div_b, n_cells, and
    whether a target of n_points points over it gets the sparse voxel index in mode voxel_index."""
    mn, mx = (np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (mn, mx))
    mb, xb, db = (np.zeros(3, dtype=np.int32) for _ in range(3))
    cells, sparse = C.c_longlong(0), C.c_int(0)
    st = _lib.lib().ndt_host_lattice(float(leaf), _f(mn), _f(mx), _i(mb), _i(xb), _i(db), C.byref(cells), int(voxel_index),
                                     int(n_points), C.byref(sparse))
    return dict(status=st, min_b=mb, max_b=xb, div_b=db, n_cells=cells.value, sparse=bool(sparse.value))


GRID_FORMS = ("empty", "chain", "buckets", "one_launch", "sparse")


def host_grid_plan(n_cells, n_points, div_b=None):
    """The plan of a target-grid build of n_points points over n_cells cells (ndt_host_grid_plan; no GPU): dict of bucket_form,
    n_buckets, cells_per_bucket, pts_per_block, n_blocks, one_launch, wmax, lds_cap, and -- with div_b, the lattice's cells per
    axis -- lut_cells, compact_items, compact_tiles, compact_prefix; filter_buckets / filter_chunks: the voxel filter's route."""
    bf, nb, cpb, ppb, blk, one, wmax, cap, items, prefix, fb, fc = (C.c_int(0) for _ in range(12))
    lut, tiles = C.c_longlong(0), C.c_longlong(0)
    db = None if div_b is None else np.ascontiguousarray(div_b, dtype=np.int32).reshape(3)
    check(_lib.lib().ndt_host_grid_plan(int(n_cells), int(n_points), None if db is None else _i(db), C.byref(bf), C.byref(nb),
                                        C.byref(cpb), C.byref(ppb), C.byref(blk), C.byref(one), C.byref(wmax), C.byref(cap),
                                        C.byref(lut), C.byref(items), C.byref(tiles), C.byref(prefix), C.byref(fb), C.byref(fc)))
    return dict(bucket_form=bool(bf.value), n_buckets=nb.value, cells_per_bucket=cpb.value, pts_per_block=ppb.value,
                n_blocks=blk.value, one_launch=bool(one.value), wmax=wmax.value, lds_cap=cap.value, lut_cells=lut.value,
                compact_items=items.value, compact_tiles=tiles.value, compact_prefix=bool(prefix.value),
                filter_buckets=bool(fb.value), filter_chunks=fc.value)


def _cov_method(method):
    try:
        return {"laplace": _lib.COV_LAPLACE, "sandwich": _lib.COV_SANDWICH}[method]
    except KeyError:
        raise ValueError("method must be 'laplace' or 'sandwich'") from None


def _pose_information(I):
    return dict(A=np.array(I.A).reshape(6, 6), B=np.array(I.B).reshape(6, 6), g=np.array(I.g), n_found=int(I.n_found),
                eig_min=float(I.eig_min), eig_max=float(I.eig_max), indefinite=bool(I.flags & _lib.COV_INDEFINITE))


def host_pose_covariance(A, B, g, n_found, method="sandwich", scale=1.0):
    """Steps 7 and 8 of the pose covariance's definition on the host (ndt_host_pose_covariance): (cov (6, 6), eig_min,
    eig_max, indefinite)."""
    A, B, g = (np.ascontiguousarray(x, dtype=np.float64) for x in (A, B, g))
    cov = np.zeros(36)
    lo, hi, fl = C.c_double(0), C.c_double(0), C.c_int(0)
    check(_lib.lib().ndt_host_pose_covariance(_d(A), _d(B), _d(g), int(n_found), _cov_method(method), float(scale), _d(cov),
                                              C.byref(lo), C.byref(hi), C.byref(fl)))
    return cov.reshape(6, 6), lo.value, hi.value, bool(fl.value & _lib.COV_INDEFINITE)


def host_pose_to_matrix(p):
    p = np.ascontiguousarray(p, dtype=np.float64)
    T = np.zeros(16, dtype=np.float32)
    _lib.lib().ndt_host_pose_to_matrix(_d(p), _f(T))
    return _from_colmajor(T)


def host_matrix_to_pose(T):
    Tc = _colmajor(T)
    p = np.zeros(6)
    _lib.lib().ndt_host_matrix_to_pose(_f(Tc), _d(p))
    return p


def host_angle_derivatives(p):
    p = np.ascontiguousarray(p, dtype=np.float64)
    j = np.zeros((8, 3), dtype=np.float32)
    h = np.zeros((15, 3), dtype=np.float32)
    jd = np.zeros((8, 3))
    hd = np.zeros((15, 3))
    _lib.lib().ndt_host_angle_derivatives(_d(p), _f(j), _f(h), _d(jd), _d(hd))
    return j, h, jd, hd


def host_pick_top(scores, keep):
    """Indices of the `keep` largest finite scores, best first, ties to the lower index (ndt_host_pick_top)."""
    s = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    keep = int(keep)
    idx = np.zeros(max(min(keep, s.shape[0]), 1), dtype=np.int32)
    n = C.c_size_t(0)
    _lib.lib().ndt_host_pick_top(_d(s), s.shape[0], keep, _i(idx), C.byref(n))
    return idx[:n.value].copy()


def host_acc_pack_cell(i, j, k):
    """Key of the absolute voxel (i, j, k) in the accumulated target's table (ndt_host_acc_pack_cell); NdtError outside
    [-2^20, 2^20)."""
    key = C.c_uint64(0)
    check(_lib.lib().ndt_host_acc_pack_cell(int(i), int(j), int(k), C.byref(key)))
    return key.value


def host_acc_unpack_cell(key):
    i, j, k = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.lib().ndt_host_acc_unpack_cell(C.c_uint64(int(key)), C.byref(i), C.byref(j), C.byref(k))
    return i.value, j.value, k.value


ACC_CELL_LIMIT = 1 << 20  # the accumulating target's lattice: cells of [-2^20, 2^20) on every axis


def crop_cell_range(resolution, min_xyz, max_xyz):
    """The cells ndt_target_accumulate_crop keeps, restated in numpy f32: per axis lo = floor(min * inv_leaf) and
    hi = floor(max * inv_leaf) with inv_leaf = 1.0f / resolution -- the f32 product rounded before the floor, as a point is
    binned -- saturated to [-2^20, 2^20).  -> (lo, hi), int64 arrays of the bounds' shape."""
    inv = np.float32(1.0) / np.float32(resolution)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for b in (min_xyz, max_xyz):
            p = np.asarray(b, dtype=np.float32) * inv
            out.append(np.clip(np.floor(p), -ACC_CELL_LIMIT, ACC_CELL_LIMIT - 1).astype(np.int64))
    return out[0], out[1]


def crop_cell_centre(resolution, cell):
    """(cell + 0.5f) * leaf in f32: the float a cropped target carries for a corner cell of its box; it floors back to the
    cell on the lattice of pitch `resolution` for every cell of [-2^20, 2^20)."""
    return (np.asarray(cell).astype(np.float32) + np.float32(0.5)) * np.float32(resolution)


# a row of an exported accumulated target (include/ndt_mi355.h): the absolute cell, the count, the f64 sums sx sy sz cxx cxy cxz
# cyy cyz czz (Identity seed included), the f32 centroid sums, a zero
ACC_ROW_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("k", "<i4"), ("count", "<i4"), ("d", "<f8", (9,)), ("f", "<f4", (3,)), ("pad", "<f4")])
ACC_BLOB_HEADER_BYTES = 64


def acc_blob_info(blob):
    """Header of a blob that passes the device-free checks (ndt_host_acc_blob_info; NdtError otherwise)
    -> dict(resolution, n_voxels, lo, hi)."""
    b = np.frombuffer(bytes(blob), dtype=np.uint8)
    res, n = C.c_float(0), C.c_size_t(0)
    lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    check(_lib.lib().ndt_host_acc_blob_info(b.ctypes.data if len(b) else None, len(b), C.byref(res), C.byref(n), _i(lo), _i(hi)))
    return dict(resolution=res.value, n_voxels=n.value, lo=lo, hi=hi)


def acc_blob_checksum(data):
    """The blob's hash over the 8-byte words of `data` (ndt_host_acc_blob_checksum): a blob's checksum field is this of its
    bytes [0, 56) followed by its rows."""
    b = np.frombuffer(bytes(data), dtype=np.uint8)
    out = C.c_uint64(0)
    check(_lib.lib().ndt_host_acc_blob_checksum(b.ctypes.data if len(b) else None, len(b), C.byref(out)))
    return out.value


def acc_blob_rows(blob):
    """The rows of a blob as a structured array (ACC_ROW_DTYPE), a read-only view of its bytes; the header is not checked."""
    return np.frombuffer(blob, dtype=ACC_ROW_DTYPE, offset=ACC_BLOB_HEADER_BYTES)


def host_thread_budget():
    """(CPUs in the affinity mask, cgroup CPU bandwidth in CPUs or 0.0 for unlimited, LOCAL_WORLD_SIZE) as the library probes them."""
    a, w, q = C.c_int(0), C.c_int(0), C.c_double(0)
    _lib.lib().ndt_host_thread_budget(C.byref(a), C.byref(q), C.byref(w))
    return a.value, q.value, w.value


def host_thread_plan(affinity_cpus, quota_cpus, local_world_size):
    """(pool threads, max batch groups) the library would use for that budget (pure)."""
    p, g = C.c_int(0), C.c_int(0)
    _lib.lib().ndt_host_thread_plan(int(affinity_cpus), float(quota_cpus), int(local_world_size), C.byref(p), C.byref(g))
    return p.value, g.value


def host_gauss(resolution, outlier_ratio):
    d = np.zeros(3)
    _lib.lib().ndt_host_gauss(float(resolution), float(outlier_ratio), _d(d))
    return d


def host_run_driver(evaluator, n_source, guess=None, resolution=1.0, step_size=0.1, outlier_ratio=0.55,
                    trans_eps=0.1, max_iter=35, reuse=False):
    """Run the PRODUCT Newton/More-Thuente driver against a Python evaluator
    evaluator(kind, T(4x4), p(6)) -> (score, g(6), H(6x6)).  reuse=True: with evaluation reuse
    (ndt_host_run_driver_reuse); the result then carries n_reused, the steps the driver fed itself."""
    def tramp(_user, kind, Tp, pp, score, g, H):
        try:
            T = _from_colmajor(np.ctypeslib.as_array(Tp, shape=(16,)))
            p = np.ctypeslib.as_array(pp, shape=(6,)).copy()
            s, gg, HH = evaluator(kind, T, p)
            score[0] = s
            for k in range(6):
                g[k] = gg[k]
            HH = np.asarray(HH, dtype=np.float64).reshape(36)
            for k in range(36):
                H[k] = HH[k]
            return 0
        except Exception:
            import traceback
            traceback.print_exc()
            return 1
    cb = _lib.EVAL_CB(tramp)
    g = None if guess is None else _colmajor(guess)
    T = np.zeros(16, dtype=np.float32)
    conv, it, ne, nh = (C.c_int(0) for _ in range(4))
    tp = C.c_double(0)
    args = (cb, None, n_source, _f(g) if g is not None else None, resolution, step_size, outlier_ratio, trans_eps, max_iter,
            _f(T), C.byref(conv), C.byref(it), C.byref(tp), C.byref(ne), C.byref(nh))
    nr = C.c_int(0)
    if reuse:
        check(_lib.lib().ndt_host_run_driver_reuse(*args, C.byref(nr)))
    else:
        check(_lib.lib().ndt_host_run_driver(*args))
    out = dict(T=_from_colmajor(T), converged=bool(conv.value), iterations=it.value, trans_probability=tp.value,
               n_evals=ne.value, n_hessian_recomputes=nh.value)
    if reuse:
        out["n_reused"] = nr.value
    return out


def extract_file_number(stem):
    """extract_file_number of the mapping node (ndt_omp_mapping_node.cpp:231-239)."""
    return _lib.lib().ndt_host_extract_file_number(stem.encode())


class PcdSequence:
    """The numbered *.pcd scans of a directory in the mapping node's order (process_new_clouds,
    ndt_omp_mapping_node.cpp:110-136), the next file being read in the background."""

    def __init__(self, directory):
        self._L = _lib.lib()
        h = C.c_void_p()
        check(self._L.ndt_pcd_sequence_open(os.fsencode(directory), C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            self._L.ndt_pcd_sequence_close(self._h)
        except Exception:
            pass

    def poll(self, loaded_clouds):
        n = C.c_size_t(0)
        check(self._L.ndt_pcd_sequence_poll(self._h, loaded_clouds, C.byref(n)))
        return n.value

    def next(self):
        """-> (xyz (n,3) float32 copy, is_dense, file_number) or None when nothing is queued."""
        p, n, dense, num = C.c_void_p(), C.c_size_t(0), C.c_int(1), C.c_int(-1)
        check(self._L.ndt_pcd_sequence_next(self._h, C.byref(p), C.byref(n), C.byref(dense), C.byref(num)))
        if not p.value:
            return None
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n.value, 4))
        return a[:, :3].copy(), bool(dense.value), num.value

    def stage(self, device=0):
        """From now on the reading threads copy every scan to `device` as soon as its file is parsed (next_device)."""
        check(self._L.ndt_pcd_sequence_stage(self._h, int(device)))

    def next_device(self):
        """-> (device address, host address, n, is_dense, file_number) of the next staged scan (16-byte records, valid until
        the following call of a next* method), or None when nothing is queued."""
        d, p, n, dense, num = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_int(1), C.c_int(-1)
        check(self._L.ndt_pcd_sequence_next_device(self._h, C.byref(d), C.byref(p), C.byref(n), C.byref(dense), C.byref(num)))
        if not p.value:
            return None
        return d.value, p.value, n.value, bool(dense.value), num.value

    def next_cloud(self, owner):
        """-> (DeviceCloud view of the next staged scan for the handle `owner`, (n, 4) float32 copy of its host records,
        is_dense, file_number), or None when nothing is queued.  The view is valid until the following next* call."""
        c, p, n, dense, num = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_int(1), C.c_int(-1)
        check(self._L.ndt_pcd_sequence_next_cloud(self._h, C.byref(c), C.byref(p), C.byref(n), C.byref(dense), C.byref(num)))
        if not c.value:
            return None
        rec = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n.value, 4)).copy()
        return DeviceCloud(owner, c), rec, bool(dense.value), num.value

    def next_raw(self):
        """-> (host address of n x (x, y, z, 1.0f) records, n, is_dense, file_number) or None.  The records sit in one of
        the sequence's two (page-locked) buffers and stay valid until the following call of next / next_raw."""
        p, n, dense, num = C.c_void_p(), C.c_size_t(0), C.c_int(1), C.c_int(-1)
        check(self._L.ndt_pcd_sequence_next(self._h, C.byref(p), C.byref(n), C.byref(dense), C.byref(num)))
        if not p.value:
            return None
        return p.value, n.value, bool(dense.value), num.value


def repack_fields(data, n, point_step, off_x=0, off_y=4, off_z=8):
    """PointCloud2-style records (bytes-like, any step / offsets) -> ((n, 4) float32 x,y,z,1, is_dense)."""
    buf = np.frombuffer(data, dtype=np.uint8)
    assert buf.size >= n * point_step
    out = np.zeros((n, 4), dtype=np.float32)
    dense = C.c_int(1)
    check(_lib.lib().ndt_host_repack_fields(buf.ctypes.data, n, point_step, off_x, off_y, off_z, out.ctypes.data, C.byref(dense)))
    return out, bool(dense.value)


def host_repack_bbox(records, n, stride_bytes, avx2=False):
    """The host upload's repack + bounding-box pass on its own (ndt_host_repack_bbox; no device).  records: a uint8 / float32
    array whose first byte is the first record's x; nothing behind byte (n - 1) * stride_bytes + 12 is promised to exist.
    -> ((n, 4) float32 records x, y, z, 1, (2, 2, 3) float32 boxes [box][min | max][xyz])."""
    buf = np.asarray(records)
    assert buf.flags.c_contiguous and (n == 0 or buf.nbytes >= (n - 1) * stride_bytes + 12)
    raw = np.zeros(4 * max(n, 1) + 4, dtype=np.float32)
    skip = ((-raw.ctypes.data) % 16) // 4  # (the records go to a 16-byte boundary)
    out = raw[skip:skip + 4 * n].reshape(n, 4)
    bounds = np.zeros(12, dtype=np.float32)
    check(_lib.lib().ndt_host_repack_bbox(buf.ctypes.data if n else None, n, stride_bytes, int(bool(avx2)),
                                          out.ctypes.data if n else None, _f(bounds)))
    return out.copy(), bounds.reshape(2, 2, 3)


# ---- motion compensation: the host-only pieces (no GPU needed) ------------------------------------------------------------
def host_deskew_motion(T, t_begin, t_end, t_ref=None):
    """The _lib.DeskewMotion of a sweep [t_begin, t_end] over which the sensor moves by the 4x4 T (its pose at t_end in its
    frame at t_begin), output frame at t_ref (None: t_begin) -- ndt_host_deskew_motion."""
    m = _lib.DeskewMotion()
    check(_lib.lib().ndt_host_deskew_motion(_f(_colmajor(T)), float(t_begin), float(t_end), float(t_begin if t_ref is None else t_ref),
                                            C.byref(m)))
    return m


def host_deskew_point(motion, xyz, t):
    """ndt_host_deskew_point, the function the kernel calls: -> ((3,) float32, untimed)."""
    p, q, u = np.ascontiguousarray(xyz, dtype=np.float32).reshape(3), np.zeros(3, dtype=np.float32), C.c_int(-1)
    check(_lib.lib().ndt_host_deskew_point(C.byref(motion), _f(p), float(t), _f(q), C.byref(u)))
    return q, bool(u.value)


def ray_spec(resolution, min_rays=2, margin=None, min_range=0.0, max_range=None):
    """An ndt_ray_spec: margin None = the resolution, max_range None = the largest the resolution allows (65536 cells)."""
    res = np.float32(resolution)
    return _lib.RaySpec(float(min_range), float(np.float32(65536.0) * res if max_range is None else max_range),
                        float(res if margin is None else margin), int(min_rays))


def ray_spec_check(resolution, min_rays=2, margin=None, min_range=0.0, max_range=None):
    """Whether the spec is valid for a target of this resolution (ndt_host_ray_spec_check) -> (ok, message)."""
    spec = ray_spec(resolution, min_rays, margin, min_range, max_range)
    st = _lib.lib().ndt_host_ray_spec_check(C.byref(spec), float(resolution))
    return st == _lib.NDT_OK, ("" if st == _lib.NDT_OK else _lib.lib().ndt_last_error().decode("utf-8", "replace"))


def ray_cells(origin, point, resolution, margin=0.0, capacity=None):
    """The cells one ray visits, walked by the body the kernel uses (ndt_host_ray_cells; no range test) -> (n, 3) int32; a ray
    that is not cast gives (0, 3)."""
    o, p = (np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (origin, point))
    n = C.c_size_t(0)
    if capacity is None:
        check(_lib.lib().ndt_host_ray_cells(_f(o), _f(p), float(resolution), float(margin), None, 0, C.byref(n)))
        capacity = n.value
    cells = np.zeros((max(int(capacity), 1), 3), np.int32)
    check(_lib.lib().ndt_host_ray_cells(_f(o), _f(p), float(resolution), float(margin), _i(cells), int(capacity), C.byref(n)))
    return cells[:n.value]


def host_ray_plan(n):
    """(blocks, passes) of the ray kernel over the n points of a call (ndt_host_ray_plan)."""
    b, p = C.c_int(0), C.c_int(0)
    check(_lib.lib().ndt_host_ray_plan(int(n), C.byref(b), C.byref(p)))
    return b.value, p.value


def plane_spec(distance_threshold, n_hypotheses, seed=0, axis=None, eps_angle=0.0, refine=False):
    """An ndt_plane_spec: axis None = any plane; else only planes whose normal lies within eps_angle (radians) of the axis."""
    s = _lib.PlaneSpec()
    s.distance_threshold, s.n_hypotheses, s.seed = float(np.float32(distance_threshold)), int(n_hypotheses), int(seed) & (2**64 - 1)
    s.use_axis, s.refine = int(axis is not None), int(bool(refine))
    if axis is not None:
        s.axis[0], s.axis[1], s.axis[2] = (float(np.float32(v)) for v in axis)
        s.eps_angle = float(np.float32(eps_angle))
    return s


def plane_spec_check(spec):
    """Is the _lib.PlaneSpec valid?  (ndt_host_plane_spec_check)"""
    return _lib.lib().ndt_host_plane_spec_check(C.byref(spec)) == _lib.NDT_OK


def host_plane_sample(seed, h, n):
    """The three point indices of hypothesis h over a cloud of n points (ndt_host_plane_sample) -> (3,) int32."""
    idx = np.zeros(3, dtype=np.int32)
    check(_lib.lib().ndt_host_plane_sample(int(seed) & (2**64 - 1), int(h), int(n), idx.ctypes.data_as(C.POINTER(C.c_int32))))
    return idx


def host_plane_model(spec, a, b, c, same_index=False):
    """The model of the triple (a, b, c) under the spec (ndt_host_plane_model, the function the kernel calls)
    -> ((4,) float64, state: 0 valid, 1 degenerate, 2 rejected)."""
    pa, pb, pc = (np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (a, b, c))
    co, st = np.zeros(4, dtype=np.float64), C.c_int(-1)
    check(_lib.lib().ndt_host_plane_model(C.byref(spec), _f(pa), _f(pb), _f(pc), int(bool(same_index)), _d(co), C.byref(st)))
    return co, st.value


def host_plane_distance(coeff, xyz):
    """The signed distance of the f32 point xyz from the plane coeff (ndt_host_plane_distance)."""
    c, p, s = np.ascontiguousarray(coeff, dtype=np.float64).reshape(4), np.ascontiguousarray(xyz, dtype=np.float32).reshape(3), C.c_double(0.0)
    check(_lib.lib().ndt_host_plane_distance(_d(c), _f(p), C.byref(s)))
    return s.value


def host_plane_fit(spec, count, S1, S2, a):
    """The fit of the refinement from the inliers' sums about a (ndt_host_plane_fit): S1 = sum q, S2 = sum q q^T as
    (xx, xy, xz, yy, yz, zz).  -> (taken, (4,) float64 coefficients, (3,) ascending eigenvalues)."""
    s1, s2, aa = (np.ascontiguousarray(v, dtype=np.float64).reshape(k) for v, k in ((S1, 3), (S2, 6), (a, 3)))
    co, lam, tk = np.zeros(4, dtype=np.float64), np.zeros(3, dtype=np.float64), C.c_int(-1)
    check(_lib.lib().ndt_host_plane_fit(C.byref(spec), float(count), _d(s1), _d(s2), _d(aa), _d(co), _d(lam), C.byref(tk)))
    return bool(tk.value), co, lam


def host_plane_plan(n, n_hypotheses):
    """The count kernel's grid over a cloud of n points (ndt_host_plane_plan)
    -> dict(tile_points, hyp_per_block, tiles, hyp_blocks, tile_blocks); the grid is tile_blocks * hyp_blocks."""
    v = [C.c_int(0) for _ in range(5)]
    check(_lib.lib().ndt_host_plane_plan(int(n), int(n_hypotheses), *[C.byref(x) for x in v]))
    return dict(zip(("tile_points", "hyp_per_block", "tiles", "hyp_blocks", "tile_blocks"), (x.value for x in v)))


def host_deskew_plan(n):
    """(blocks, points_per_block) of the motion compensation of a cloud of n points (ndt_host_deskew_plan)."""
    b, p = C.c_int(0), C.c_int(0)
    check(_lib.lib().ndt_host_deskew_plan(int(n), C.byref(b), C.byref(p)))
    return b.value, p.value


POINTFIELD_TYPES = {"int8": 1, "uint8": 2, "int16": 3, "uint16": 4, "int32": 5, "uint32": 6, "float32": 7, "float64": 8}


def extract_field(data, n, point_step, offset, datatype):
    """One scalar field of PointCloud2-style records (bytes-like, any step / offset) as (n,) float64 -- the companion of
    repack_fields for the per-point time.  datatype: a sensor_msgs/PointField code 1 ... 8 or a name of POINTFIELD_TYPES."""
    buf = np.frombuffer(data, dtype=np.uint8)
    assert buf.size >= n * point_step
    out = np.zeros(max(n, 1), dtype=np.float64)
    code = POINTFIELD_TYPES.get(datatype, datatype)
    check(_lib.lib().ndt_host_extract_field(buf.ctypes.data if buf.size else None, n, point_step, offset, int(code), _d(out)))
    return out[:n].copy()


def pcd_read_field(path, name):
    """One named scalar field of a PCD file as (n,) float64 (ndt_pcd_read_field)."""
    L = _lib.lib()
    n, nf, kind = C.c_size_t(0), C.c_int(0), C.c_int(0)
    check(L.ndt_pcd_read_header(os.fsencode(path), C.byref(n), C.byref(nf), C.byref(kind)))
    out = np.zeros(max(n.value, 1), dtype=np.float64)
    check(L.ndt_pcd_read_field(os.fsencode(path), name.encode(), _d(out), n.value, C.byref(n)))
    return out[:n.value].copy()
