/* ndt_mi355.h -- C-ABI of the MI355X-native NDT scan-matching core.
 *
 * This is the drop-in boundary for ToySLAM's
 *   pclomp::NormalDistributionsTransform<PointSource, PointTarget>
 * (reference: ndt_omp/include/pclomp/ndt_omp.h:70-502, implementation
 * ndt_omp_impl.hpp, voxel grid voxel_grid_covariance_omp{.h,_impl.hpp}).
 * The header-only adapter include/pclomp/ndt_omp.h re-declares that class on
 * top of these entry points; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - plain C types only; every function returns an ndt_status (0 = ok) unless
 *    noted; ndt_last_error() gives a thread-local message for the last failure.
 *  - point buffers: `n` records of `stride_bytes` bytes, three f32 x,y,z at
 *    offset 0 of each record (pcl::PointXYZ: stride 16; PointXYZI/XYZRGB: 32).
 *  - 4x4 transforms are 16 f32 in COLUMN-major order (Eigen::Matrix4f::data()).
 *  - 6x6 Hessians are 36 f64 row-major; pose vectors are
 *    [tx, ty, tz, roll, pitch, yaw] f64 (ndt_omp_impl.hpp:107-111).
 *  - a handle is thread-compatible (one caller at a time), like the reference
 *    object; distinct handles may be used from distinct threads.
 *  - there is NO CPU fallback: every compute entry point fails with
 *    NDT_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef NDT_MI355_H_
#define NDT_MI355_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ndt_context* ndt_handle;

typedef enum {
  NDT_OK = 0,
  NDT_ERR_INVALID = 1,       /* bad argument / call order                          */
  NDT_ERR_NO_DEVICE = 2,     /* no usable HIP device (never falls back to the CPU) */
  NDT_ERR_HIP = 3,           /* HIP runtime error, see ndt_last_error()            */
  NDT_ERR_GRID_OVERFLOW = 4, /* dx*dy*dz > INT32_MAX: voxel_grid_covariance_omp_impl.hpp:75-84 */
  NDT_ERR_NO_INPUT = 5,      /* target/source missing: _impl.hpp:54-60             */
  NDT_ERR_COMM = 6           /* collective callback failed                         */
} ndt_status;

/* pclomp::NeighborSearchMethod, ndt_omp.h:52-57 (same numeric values). */
typedef enum { NDT_KDTREE = 0, NDT_DIRECT26 = 1, NDT_DIRECT7 = 2, NDT_DIRECT1 = 3 } ndt_search_method;

const char* ndt_last_error(void);
/* Number of usable gfx950 devices (0 when none; never an error). */
int ndt_device_count(void);

/* ---- lifetime ----------------------------------------------------------- */
/* NormalDistributionsTransform() ctor, ndt_omp_impl.hpp:47-76: resolution 1.0,
 * step 0.1, outlier 0.55, epsilon 0.1, max_iterations 35, DIRECT7.
 * `device` = HIP device ordinal.  Creating a handle does not touch the GPU
 * until the first target/source upload. */
ndt_status ndt_create(int device, ndt_handle* out);
/* Copy-construction (ndt_omp_mapping_node.cpp:151-169 returns the object by
 * value): parameters and results are copied, the immutable device grid and the
 * source cloud are shared (ref-counted). */
ndt_status ndt_clone(ndt_handle src, ndt_handle* out);
void ndt_destroy(ndt_handle h);

/* ---- parameters (setters mirror ndt_omp.h:115-191 + pcl::Registration) ---- */
ndt_status ndt_set_resolution(ndt_handle h, float resolution);       /* ndt_omp.h:132-142, rebuilds the grid if a source is set */
ndt_status ndt_set_step_size(ndt_handle h, double step_size);        /* :165-169 */
ndt_status ndt_set_outlier_ratio(ndt_handle h, double ratio);        /* :183-187 */
ndt_status ndt_set_transformation_epsilon(ndt_handle h, double eps); /* pcl::Registration */
ndt_status ndt_set_maximum_iterations(ndt_handle h, int n);          /* pcl::Registration */
ndt_status ndt_set_neighborhood_search_method(ndt_handle h, int m);  /* :189-191; unknown values act as DIRECT7 (the reference's `default:`) */
ndt_status ndt_set_num_threads(ndt_handle h, int n);                 /* :115-117; stored, unused on the GPU */
ndt_status ndt_set_min_points_per_voxel(ndt_handle h, int n);        /* voxel_grid_covariance_omp.h:227-239 (clamped to >= 3) */
ndt_status ndt_set_cov_eig_value_inflation_ratio(ndt_handle h, double r); /* .h:253-257 */
float ndt_get_resolution(ndt_handle h);
double ndt_get_step_size(ndt_handle h);
double ndt_get_outlier_ratio(ndt_handle h);

/* ---- inputs --------------------------------------------------------------
 * setInputTarget (ndt_omp.h:122-127): uploads the cloud and builds the voxel
 * grid on the GPU (VoxelGridCovariance::applyFilter, _impl.hpp:48-370).
 * `is_dense` = pcl::PointCloud::is_dense (non-finite points are skipped when 0). */
ndt_status ndt_set_input_target(ndt_handle h, const void* pts, size_t n, size_t stride_bytes, int is_dense);
ndt_status ndt_set_input_source(ndt_handle h, const void* pts, size_t n, size_t stride_bytes);
/* Same, for clouds already resident in HBM (device pointers on the handle's device). */
ndt_status ndt_set_input_target_device(ndt_handle h, const void* d_pts, size_t n, size_t stride_bytes, int is_dense);
ndt_status ndt_set_input_source_device(ndt_handle h, const void* d_pts, size_t n, size_t stride_bytes);
/* Same, BY REFERENCE: the cloud -- dense 16-byte records (x, y, z, anything) on a 16-byte boundary in HBM, pcl::PointXYZ's
 * layout -- is used where it lies instead of being copied: the caller keeps the memory alive and unchanged for as long as
 * it is this handle's input (or the input of a handle cloned from it / sharing it), exactly what pcl::Registration's
 * setInputTarget(ConstPtr) / setInputSource(ConstPtr) promise (ndt_omp.h:122-127: the base class keeps the shared pointer,
 * it never copies the cloud).  Saves the 16 MB -> 16 MB copy of a 1 M-point target; only the bounding boxes are computed. */
ndt_status ndt_set_input_target_device_ref(ndt_handle h, const void* d_pts, size_t n, int is_dense);
ndt_status ndt_set_input_source_device_ref(ndt_handle h, const void* d_pts, size_t n);
/* The voxel index behind the target grid and the prefilter (the reference's std::map<size_t, Leaf> keyed by the linear
 * voxel index, voxel_grid_covariance_omp.h:201): 0 = chosen by occupancy (default), 1 = dense table over the bounding
 * box, 2 = sparse (sort-based build, hash look-up; what a fine leaf over a wide box needs: the 0.1 m prefilter of
 * apps/align.cpp:60-69, kilometre-sized maps).  Results are bit-identical either way. */
ndt_status ndt_set_voxel_index(ndt_handle h, int mode);

/* One uploaded (and spatially ordered) source cloud serving several handles on the same device, the way ndt_clone
 * shares it: `dst` registers the cloud `src` holds.  The levels of a multi-resolution pyramid (BASELINE configs[4]:
 * 2.0 -> 1.0 -> 0.5 m grids over one target, one handle per grid) take every scan from one upload this way, and a
 * second donor handle can upload the next scan on its own stream meanwhile. */
ndt_status ndt_share_input_source(ndt_handle dst, ndt_handle src);
/* The same for the target: `dst` takes the target cloud AND the voxel grid `src` built from it (no copy, no rebuild;
 * resolution, min_points_per_voxel and the eigenvalue ratio of `dst` become the grid's). */
ndt_status ndt_share_input_target(ndt_handle dst, ndt_handle src);

/* CU partitions: overlapping the NEXT scan's preparation with the CURRENT registration.
 * A registration keeps the whole chip busy for its duration -- the persistent evaluation kernel holds one workgroup per CU,
 * the per-evaluation kernels of a multi-million-point scan fill every CU -- so the upload, spatial ordering and target grid
 * build of the following scan, issued meanwhile by another handle on another stream, wait behind it (the reference's nodes
 * do the two strictly one after the other: ndt_omp_mapping_node.cpp:151-169, 195-211).  With partitions the two never
 * compete: the handle's stream is created with a CU mask (hipExtStreamCreateWithCUMask),
 *   0  the whole device (default);
 *   1  the registration partition: all CUs but the last NDT_SIDE_CUS (default 32) -- for the handles that align;
 *   2  the side partition: those NDT_SIDE_CUS CUs -- for handles that only prepare inputs (ndt_set_input_*,
 *      ndt_voxel_grid_filter*, ndt_map_update*) and hand them over with ndt_share_input_source / ndt_share_input_target.
 * The latency kernels cut a scan into one workgroup per CU of the handle's partition, so a partitioned handle adds the same
 * per-point terms in another (still fixed) order: sums equal to the unpartitioned handle's to the last bits of an f64, as
 * between the lock-step batches and ndt_align; grids, voxel filters and map updates are bit-identical in any partition.
 * Call before the handle is used, or between calls (the handle waits for its work in flight and moves to the stream of the new partition; it keeps the streams it has had until ndt_destroy).
 * ndt_get_cu_partition reports the partition and the CUs the stream really got (the device's count when masks are
 * unavailable). */
ndt_status ndt_set_cu_partition(ndt_handle h, int partition);
ndt_status ndt_get_cu_partition(ndt_handle h, int* partition, int* n_cus);

/* ---- registration --------------------------------------------------------
 * pcl::Registration::align(output, guess) -> computeTransformation
 * (ndt_omp_impl.hpp:80-171) with the More-Thuente line search (:772-932).
 * guess == NULL means Identity.  out_cloud (optional, host memory) receives the source
 * transformed by the last line-search trial, n_source records of
 * out_stride_bytes (x,y,z,1.0f written at offset 0).  With out_cloud == NULL the call
 * returns as soon as the result is known; the aligned cloud is then completed in stream
 * order and ndt_get_output_device waits for it. */
ndt_status ndt_align(ndt_handle h, const float* guess, float* final_transformation, int* has_converged,
                     int* final_num_iteration, double* transformation_probability, void* out_cloud,
                     size_t out_stride_bytes);
/* Results of the last align (hasConverged / getFinalTransformation /
 * getFinalNumIteration / getTransformationProbability). */
ndt_status ndt_get_result(ndt_handle h, float* final_transformation, int* has_converged, int* final_num_iteration,
                          double* transformation_probability);
/* Device pointer (n_source x float4) of the last align's transformed source. */
ndt_status ndt_get_output_device(ndt_handle h, const void** d_cloud, size_t* n);
/* Work counters of the last align: derivative evaluations E, f64 Hessian
 * recomputes, mean valid neighbours per point (h-bar) of the last evaluation.
 * After ndt_align_batch: the scan evaluations / f64 recomputes of all members
 * together and h-bar over all of their evaluations. */
ndt_status ndt_get_stats(ndt_handle h, int* n_evals, int* n_hessian_recomputes, double* mean_neighbors);

/* calculateScore(cloud), ndt_omp_impl.hpp:935-983 (cloud is used as given). */
ndt_status ndt_calculate_score(ndt_handle h, const void* cloud, size_t n, size_t stride_bytes, double* score);

/* [PCL 1.10] pcl::Registration::getFitnessScore(max_range) (printed by apps/align.cpp:24-33 and
 * ndt_rosbag_mapping_node.cpp:133): the source transformed by the last align's final transformation,
 * nearest target point of each (exact search, f32 squared distances as FLANN's L2_Simple), mean of the
 * squared distances that are <= max_range (PCL compares the SQUARED distance with max_range; kept),
 * DBL_MAX when none qualifies.  Runs on the GPU over the target's voxel grid; pass DBL_MAX for PCL's
 * default.  Non-finite source points are skipped. */
ndt_status ndt_get_fitness_score(ndt_handle h, double max_range, double* fitness);

/* ---- scan prefilter (row N1 of the scope table) -----------------------------
 * pcl::VoxelGrid<PointT>::filter -- one centroid per occupied voxel, output in ascending
 * voxel-index order -- as every caller runs it before NDT (ndt_omp/apps/align.cpp:60-69,
 * ndt_omp_mapping_node.cpp:142-148,203-210; [PCL 1.10] filters/impl/voxel_grid.hpp).  xyz only.
 * `out` must hold n records of out_stride_bytes (x,y,z,1.0f at offset 0); *n_out = voxels written.
 * When the voxel index space would overflow int32 PCL warns and passes the input through: the
 * input is then copied to `out`, *n_out = n and NDT_ERR_GRID_OVERFLOW is returned. */
ndt_status ndt_voxel_grid_filter(ndt_handle h, const void* pts, size_t n, size_t stride_bytes, int is_dense, float leaf_size,
                                 void* out, size_t out_stride_bytes, size_t* n_out);
/* Same with input and output (n x float4) resident in HBM. */
ndt_status ndt_voxel_grid_filter_device(ndt_handle h, const void* d_pts, size_t n, size_t stride_bytes, int is_dense,
                                        float leaf_size, void* d_out_float4, size_t* n_out);

/* ---- global map accumulation (row N2 of the scope table) ---------------------
 * update_global_map of the mapping nodes (ndt_omp_mapping_node.cpp:195-211,
 * ndt_rosbag_mapping_node.cpp:146-161): pcl::transformPointCloud(scan, pose) -> global_map += it ->
 * global_map = VoxelGrid(leaf).filter(global_map).  The map lives in HBM with the handle; `pose` is a
 * column-major 4x4 (NULL = identity).  *overflowed = 1 when the leaf is too small for the map's
 * bounding box: PCL then keeps the unfiltered concatenation, and so does this.
 * ndt_host_chain_pose is the nodes' `pose = pose * transform` (:88-99 / :62-68) in Eigen's f32 rounding. */
ndt_status ndt_map_clear(ndt_handle h);
ndt_status ndt_map_update(ndt_handle h, const void* scan, size_t n, size_t stride_bytes, int is_dense, const float* pose,
                          float leaf_size, int* overflowed);
ndt_status ndt_map_update_device(ndt_handle h, const void* d_scan, size_t n, size_t stride_bytes, int is_dense,
                                 const float* pose, float leaf_size, int* overflowed);
ndt_status ndt_map_size(ndt_handle h, size_t* n);
ndt_status ndt_map_get(ndt_handle h, void* out, size_t out_stride_bytes); /* x,y,z,1.0f per point */
ndt_status ndt_map_get_device(ndt_handle h, const void** d_pts_float4, size_t* n);
void ndt_host_chain_pose(const float* pose /*16*/, const float* transform /*16*/, float* out /*16, may alias*/);
/* The voxel lattice of pitch `leaf` over the box [mn, mx] as every grid build, the accumulating target, the voxel filter and
 * the source ordering compute it (voxel_grid_covariance_omp_impl.hpp:75-103), and whether a target of n_points points
 * over it gets the sparse voxel index under ndt_set_voxel_index mode voxel_index.  Host only.  NDT_ERR_GRID_OVERFLOW
 * (outputs untouched) where the reference's integer indices would overflow, NDT_ERR_INVALID for a leaf that is not
 * positive or a NULL corner.  Any output may be NULL. */
ndt_status ndt_host_lattice(float leaf, const float* mn /*3*/, const float* mx /*3*/, int* min_b /*3*/, int* max_b /*3*/,
                            int* div_b /*3*/, long long* n_cells, int voxel_index, long long n_points, int* sparse);

/* What a node does once, at start-up, instead of inside its first scans: the device context, the library's code object (tens
 * of milliseconds on first use), the handle's page-locked result / staging slots, and one pass through the loop's calls
 * (voxel filter, target grid, registration, map update) on a synthetic scan of `expected_scan_points` points, so that every
 * kernel has been launched once and the handle's memory pool holds blocks of the sizes the real scans will ask for.
 * The handle's inputs, last result and map are left as they were. */
ndt_status ndt_warm_up(ndt_handle h, size_t expected_scan_points);

/* ---- clouds that stay in HBM: the node loop without host round trips -----------------------------------------------
 * In all three mapping nodes a filtered scan is used four times: as the output of the prefilter
 * (ndt_omp_mapping_node.cpp:142-148), as the source of the registration against its predecessor (:151-169), as the target of
 * the registration of its successor (cloud k is clouds_[current_index_] of one pair and clouds_[current_index_ - 1] of the
 * next, :77-79), and as what update_global_map adds to the map (:195-211).  Through host buffers that is one download and
 * three uploads, repacks and bounding-box passes of the same points.  An `ndt_cloud` is that scan as an object: dense
 * 16-byte records in HBM together with their bounding boxes, reference-counted (a handle that takes it as an input holds a
 * reference of its own, so releasing the caller's reference is always safe).
 *   ndt_cloud_voxel_filter      N1 with the result left in HBM (pts: host memory, or device memory when on_device != 0)
 *   ndt_cloud_upload            a host cloud as it is
 *   ndt_set_input_source_cloud / ndt_set_input_target_cloud / ndt_map_update_cloud
 *                               the three consumers, by reference: no copy, no repack, no bounding-box pass
 *   ndt_promote_source_to_target  the handle's current input source becomes its input target (cloud k of the pair
 *                               (k-1, k) is the target of the pair (k, k+1)); the voxel grid is built from the
 *                               resident points -- for callers that kept no ndt_cloud, e.g. after ndt_set_input_source
 * Results are bit-identical to the host-buffer entry points (same kernels on the same points).  A cloud belongs to the
 * device of the handle that made it; handles on other streams of that device may use it (the library orders the streams). */
typedef struct ndt_cloud_s* ndt_cloud;
ndt_status ndt_cloud_voxel_filter(ndt_handle h, const void* pts, size_t n, size_t stride_bytes, int is_dense, float leaf_size,
                                  int on_device, ndt_cloud* out, int* overflowed);
/* N1 of an ndt_cloud in two halves: _begin queues the whole filter on a stream of the handle's own and returns at once,
 * _end waits for it and hands out the result -- in between the caller registers the PREVIOUS scan (the prefilter of scan
 * k + 1 runs beside the registration of scan k).  One prefilter at a time per handle.  Same result as ndt_cloud_voxel_filter. */
ndt_status ndt_cloud_voxel_filter_begin(ndt_handle h, ndt_cloud in, int is_dense, float leaf_size);
ndt_status ndt_cloud_voxel_filter_end(ndt_handle h, ndt_cloud* out, int* overflowed);
/* N1 of many clouds in one call: pcl::VoxelGrid::filter of n_clouds clouds at one leaf size.  out[k] receives cloud k's
 * centroids as a new ndt_cloud and overflowed[k] (may be NULL) PCL's "leaf size too small" flag -- what
 * ndt_cloud_voxel_filter returns for that cloud alone, the same bits, whatever the other clouds and their order.
 * Buffer form: cloud k is points [offsets[k], offsets[k+1]) of pts (host memory, or device memory when on_device != 0).
 * is_dense: n_clouds NaN rules, NULL = 0 for every cloud.  Every out[k] is a cloud of its own (ndt_cloud_release; releasing
 * one leaves the others valid; an empty input gives an empty cloud, never NULL).  Synchronises the handle's stream; the
 * handle's target, source, grid, results and a begun ndt_cloud_voxel_filter_begin are left as they were.
 * NDT_ERR_INVALID before any device work: NULL handle or out, !(leaf_size > 0), NULL offsets / in with clouds,
 * decreasing offsets, a bad stride, NULL pts with points, a NULL entry of in, more than 65535 clouds.
 * On any error every out[k] is NULL and nothing is kept. */
ndt_status ndt_cloud_voxel_filter_batch(ndt_handle h, const void* pts, const size_t* offsets /* n_clouds+1 */, size_t n_clouds,
                                        size_t stride_bytes, const int* is_dense, float leaf_size, int on_device,
                                        ndt_cloud* out /* n_clouds */, int* overflowed /* n_clouds or NULL */);
/* the same over clouds already resident in HBM (ndt_cloud_upload, ndt_pcd_sequence_next_cloud views, earlier outputs) */
ndt_status ndt_cloud_voxel_filter_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const int* is_dense,
                                         float leaf_size, ndt_cloud* out, int* overflowed);
/* diagnostics of the handle's last batched filter: composite passes, clouds that took the single-cloud route, and the
 * launches, fills and copies the call queued outside that route */
ndt_status ndt_diag_filter_batch(ndt_handle h, size_t* passes, size_t* single_route, size_t* launches);
ndt_status ndt_cloud_upload(ndt_handle h, const void* pts, size_t n, size_t stride_bytes, ndt_cloud* out);
ndt_status ndt_cloud_size(ndt_cloud c, size_t* n);
ndt_status ndt_cloud_data(ndt_cloud c, const void** d_pts_float4, size_t* n);               /* the records in HBM */
ndt_status ndt_cloud_download(ndt_handle h, ndt_cloud c, void* out, size_t out_stride_bytes); /* x,y,z,1.0f per point */
void ndt_cloud_release(ndt_cloud c);
/* Every cloud carries two bounding boxes, computed where the cloud is made and never again: box [0] over the coordinates
 * that are not NaN (what getMinMax3D sees for an is_dense cloud), box [1] over the points whose three coordinates are
 * finite (the !is_dense rule).  Every lattice -- grid build, voxel filter, source ordering, the map's guessed box, GICP's
 * extents -- is laid over one of them.  ndt_box_route names the producer that wrote a cloud's boxes. */
typedef enum {
  NDT_BOX_ROUTE_NONE = 0,         /* no producer ran: an empty cloud, the initial (FLT_MAX, -FLT_MAX) boxes               */
  NDT_BOX_ROUTE_HOST_SCALAR = 1,  /* host upload, one point per step                                                      */
  NDT_BOX_ROUTE_HOST_AVX2 = 2,    /* host upload, two points per step                                                     */
  NDT_BOX_ROUTE_REPACK = 3,       /* device, records of any stride (k_repack_bbox): per-block rows behind a stream wait   */
  NDT_BOX_ROUTE_REC16_COPY = 4,   /* device, aligned 16-byte records copied (k_bbox16<true>); device buffers: rows polled */
  NDT_BOX_ROUTE_REC16_POLLED = 5, /* a cloud by reference (k_bbox16<false>): nothing copied, tagged rows polled           */
  NDT_BOX_ROUTE_FILTER_ROWS = 6,  /* output of a voxel filter: rows of at most 64 blocks, the count read on the device    */
  NDT_BOX_ROUTE_MULTI_WORDS = 7,  /* member of a batched call (k_repack_bbox_multi): order-encoded words, atomic max      */
  NDT_BOX_ROUTE_STAGED = 8,       /* scan of a staged PCD sequence: boxes by the reading thread                           */
  NDT_BOX_ROUTE_SELECT = 9,       /* output of a selection (k_select_place): per-block rows of the kept points            */
  NDT_BOX_ROUTE_DESKEW = 10       /* output of a motion compensation (k_deskew): per-block rows of the records written    */
} ndt_box_route;
/* the cloud's boxes exactly as stored: out = {min xyz, max xyz} of box [0], then of box [1]; an empty box is
 * (FLT_MAX, -FLT_MAX).  *route (may be NULL) = the ndt_box_route that wrote them.  No device work. */
ndt_status ndt_cloud_bounds(ndt_cloud c, float out[12], int* route);
/* the same for a handle's inputs: which = 0 the input source, 1 the input target's cloud, 2 the map (a queued map update
 * is waited for first; NDT_ERR_NO_INPUT when the map's boxes are not known: no update yet, or ndt_map_clear).
 * NDT_ERR_NO_INPUT when that input is not set. */
ndt_status ndt_diag_input_bounds(ndt_handle h, int which, float out[12], int* route);
/* Host only, no device: the host upload's repack + bounding-box pass itself (the function upload_cloud calls for clouds of
 * at most NDT_HOST_STAGE_MAX points), avx2 = 0 the one-point form, 1 the two-point form (NDT_ERR_INVALID where the CPU
 * has no AVX2).  n records of stride_bytes (>= 12, a multiple of 4; x y z first) -> out_records: n records (x, y, z, 1.0f)
 * on a 16-byte boundary; out_bounds as ndt_cloud_bounds writes them.  Records of 12 bytes: nothing behind the last
 * record is read. */
ndt_status ndt_host_repack_bbox(const void* pts, size_t n, size_t stride_bytes, int avx2, float* out_records, float out_bounds[12]);
ndt_status ndt_set_input_source_cloud(ndt_handle h, ndt_cloud c);
ndt_status ndt_set_input_target_cloud(ndt_handle h, ndt_cloud c, int is_dense);
ndt_status ndt_map_update_cloud(ndt_handle h, ndt_cloud scan, int is_dense, const float* pose, float leaf_size, int* overflowed);
/* N2 of many scans in one call.  PCL: for k in order { transformPointCloud(scan k, poses[16k..]); map += it; } then ONE
 * VoxelGrid::filter(leaf) of the concatenation [map | scan 0 | scan 1 | ...] -- one transform launch for all scans and one
 * filter, where a loop of ndt_map_update_cloud re-filters the growing map once per scan.
 * NOT the loop's map: a voxel of this map is the centroid of ALL points that fell into it (the map's and every scan's); the
 * loop keeps centroids of centroids.  Both occupy the same voxels, the coordinates differ (by up to a good part of the leaf
 * size).  The mapping nodes' map, bit for bit, is what the per-scan calls give.
 * - The map after the call is, bit for bit, pcl::VoxelGrid::filter of that concatenation, scan k moved as transformPointCloud
 *   moves it (a non-finite point of a scan with is_dense[k] == 0 is left as it is by the transform and dropped by the filter).
 *   The concatenation is dense only if the map was and every scan is.  is_dense: one flag per scan, NULL = 0 for all;
 *   poses: 16 column-major floats per scan, NULL = the identity for all.
 * - n_scans == 1 is ndt_map_update_cloud / ndt_map_update / ndt_map_update_device of that scan: same map, same *overflowed,
 *   same bits.  Overflow ("leaf size too small"): the unfiltered concatenation is kept and *overflowed = 1.
 * - n_scans == 0 is NDT_OK, touches nothing and needs no device.  Scans of zero points are allowed; if all are empty the map
 *   is filtered again, as the single call does with an empty scan.
 * - Completion as ndt_map_update_cloud: queued on the map's stream; size and boxes are settled by the next call that needs
 *   them (ndt_map_size, ndt_map_get*, the next update).  The handle keeps a reference to every scan until then: releasing
 *   the caller's references right after the call is safe.  The buffer form copies: its buffer is free on return.
 * - The handle's target, source, grid, last result, a begun ndt_cloud_voxel_filter_begin and the pairs state stay as they
 *   were; ndt_map_update* continues on the same map afterwards.
 * - NDT_ERR_INVALID before any device work, map untouched: NULL handle, !(leaf_size > 0), NULL scans / offsets with
 *   n_scans > 0, a NULL entry of scans, decreasing offsets, a stride below 12 or not a multiple of 4, NULL pts with points,
 *   more than 65 535 scans, a total (map + scans) above INT_MAX points (with an update still queued, the map's size is
 *   known only once that update has been waited for: the refusal then comes behind that wait, and still before anything of
 *   this call is copied or queued).  After any later error the map is what it was. */
ndt_status ndt_map_update_clouds(ndt_handle h, const ndt_cloud* scans, size_t n_scans, const int* is_dense /* n_scans or NULL = 0 */,
                                 const float* poses /* n_scans*16 column-major, NULL = identity for all */, float leaf_size,
                                 int* overflowed);
/* buffer form: scan k is points [offsets[k], offsets[k+1]) of pts (host memory, or device memory when on_device != 0) */
ndt_status ndt_map_update_batch(ndt_handle h, const void* pts, const size_t* offsets /* n_scans+1 */, size_t n_scans,
                                size_t stride_bytes, const int* is_dense, const float* poses, float leaf_size, int on_device,
                                int* overflowed);
/* diagnostics of the handle's last ndt_map_update_clouds / _batch call: transform launches (1 whatever the number of scans),
 * filters of the concatenation (1), exact bounding-box passes (0, or 1 when the scans' boxes under their poses did not do) */
ndt_status ndt_diag_map_batch(ndt_handle h, size_t* transform_launches, size_t* filters, size_t* box_passes);
ndt_status ndt_promote_source_to_target(ndt_handle h, int is_dense);

/* ---- selection: dropping points from a resident cloud ---------------------------------------------------------------------
 * pcl::removeNaNFromPointCloud (FINITE), pcl::CropBox with setNegative (BOX, BOX_NEGATE; on a cloud that is not dense:
 * BOX | FINITE), a min / max range crop (RANGE), and pcl::PassThrough on a computed per-point value (KEY) -- of an ndt_cloud,
 * with the result left in HBM as an ndt_cloud: a stable compaction of the kept 16-byte records (all four words as they are)
 * and the two bounding boxes of the kept points.  A point (x, y, z as stored, f32) with key k (f64) is kept iff every
 * enabled test passes (the definition is toyslam_amd/csrc/ndt_select.hpp, one function for host and device):
 *   FINITE  all three coordinates finite
 *   BOX     inside = box_min[a] <= p[a] && p[a] <= box_max[a] on all three axes (f32 compares: a NaN coordinate is never
 *           inside); passes iff inside, with BOX_NEGATE iff not inside (a NaN point is then kept, unless FINITE is set too)
 *   RANGE   dx = x - centre[0] ..., d2 = (dx*dx + dy*dy) + dz*dz in f32, every operation rounded on its own (no fused
 *           multiply-add); inside = r_min*r_min <= d2 && d2 <= r_max*r_max (products in f32; r_max = +inf is allowed; a NaN
 *           d2 is never inside); RANGE_NEGATE inverts as for the box
 *   KEY     inside = key_lo <= k && k <= key_hi; KEY_NEGATE inverts; a NaN key fails the test in both senses
 * flags == 0 keeps every point (the result is a copy).  A spec is invalid if it has unknown flag bits, a *_NEGATE bit without
 * its test, with BOX a NaN bound or box_min[a] > box_max[a], with RANGE a NaN centre / r_min / r_max, r_min < 0 or
 * r_min > r_max, with KEY a NaN bound or key_lo > key_hi. */
enum {
  NDT_SELECT_FINITE = 1,
  NDT_SELECT_BOX = 2,
  NDT_SELECT_BOX_NEGATE = 4,
  NDT_SELECT_RANGE = 8,
  NDT_SELECT_RANGE_NEGATE = 16,
  NDT_SELECT_KEY = 32,
  NDT_SELECT_KEY_NEGATE = 64
};
typedef struct {
  unsigned flags;
  float box_min[3], box_max[3]; /* BOX   */
  float centre[3], r_min, r_max; /* RANGE */
  double key_lo, key_hi;        /* KEY   */
} ndt_select_spec;
/* - ndt_cloud_select: *out is a new cloud of its own (ndt_cloud_release) holding the kept records of `in`, in in's order, with
 *   boxes exact over the kept points (route NDT_BOX_ROUTE_SELECT) -- bit for bit what ndt_cloud_upload of the host-selected
 *   records would be, and usable by every consumer of an ndt_cloud.  Nothing kept: an empty cloud, never NULL, with the initial
 *   boxes and route NONE.  keys: n_in doubles, host memory or (keys_on_device != 0) device memory; may be NULL without KEY.
 *   kept_idx (host, capacity n_in, may be NULL) receives the kept points' indices, ascending; *n_kept (may be NULL) their
 *   number.  The call returns after its own work is done (a borrowed view of a staged sequence may be overwritten afterwards).
 * - ndt_cloud_select_clouds: one spec for n_clouds clouds, two launches in all; out[k] and n_kept[k] are what ndt_cloud_select
 *   gives for cloud k alone, the same bits whatever the other clouds and their order.  Every out[k] is a cloud of its own
 *   (releasing one leaves the others valid).  KEY is refused.  n_clouds == 0 is NDT_OK, touches nothing and needs no device.
 *   On any error every out[k] is NULL.
 * - ndt_source_select_by_nvtl: ndt_source_point_nvtl under `transform` (NULL: the last align's final transformation), then
 *   the selection of the handle's source with those values as device-resident keys (they never visit the host): a point is
 *   kept iff (found and L >= min_likelihood) or (not found and keep_unfound).  *out holds the SOURCE'S OWN records, unmoved,
 *   in the caller's point order -- what ndt_target_accumulate_cloud or ndt_map_update_cloud take at the registered pose.
 *   *n_found (may be NULL) is the NVTL call's count, *n_kept (may be NULL) the selection's.  Refuses what ndt_source_point_nvtl
 *   refuses, a NULL out and a NaN min_likelihood.  It is an NVTL call to ndt_diag_nvtl and overwrites the values the last
 *   ndt_source_point_nvtl's d_out names.
 * - ndt_diag_select, of the last of the three calls above that reached the device: kernel launches (2, whatever the number of
 *   clouds; 0 when no cloud had a point), the blocks of each launch, the clouds.
 * None of them changes the handle's target, source, grid, last result, statistics, map, a begun
 * ndt_cloud_voxel_filter_begin or the pairs state.
 * NDT_ERR_INVALID before any device work, outputs untouched apart from *out = NULL (every out[k] = NULL): a NULL handle, in,
 * spec or out, an invalid spec, KEY without keys, a NULL entry of in, more than 65 535 clouds, a cloud of another device, more
 * than INT_MAX points.  After those checks NDT_ERR_NO_DEVICE without a gfx950 device. */
ndt_status ndt_cloud_select(ndt_handle h, ndt_cloud in, const ndt_select_spec* spec, const double* keys /* n_in, or NULL without KEY */,
                            int keys_on_device, ndt_cloud* out, int32_t* kept_idx /* host, capacity n_in, or NULL */,
                            size_t* n_kept /* or NULL */);
ndt_status ndt_cloud_select_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_select_spec* spec,
                                   ndt_cloud* out /* n_clouds */, size_t* n_kept /* n_clouds or NULL */);
ndt_status ndt_source_select_by_nvtl(ndt_handle h, const float* transform /* 16 or NULL: last align's */, double min_likelihood,
                                     int keep_unfound, ndt_cloud* out, size_t* n_kept, size_t* n_found);
ndt_status ndt_diag_select(ndt_handle h, size_t* launches, size_t* blocks, size_t* clouds);
/* Host only, no device: the predicate itself (*keep = 0 / 1; NDT_ERR_INVALID for an invalid spec), and the launch plan of a
 * cloud of n_points -- blocks of 256 threads, each owning one contiguous range of *points_per_block points (the last one the
 * rest); at most 1024 blocks, beyond which points_per_block grows. */
ndt_status ndt_host_select_point(const ndt_select_spec* spec, const float xyz[3], double key, int* keep);
ndt_status ndt_host_select_plan(size_t n_points, int* blocks, int* points_per_block);

/* ---- deskew: motion compensation of a resident scan by the time of every point -------------------------------------------
 * A sweep covers [t_begin, t_end].  Over it the sensor moves by the rotation vector w = angle * axis (radians) and the
 * translation tau (metres, in the sensor frame at t_begin): its pose at time t, relative to its pose at t_begin, is
 * (Exp(u w), u tau) with u = (t - t_begin) / (t_end - t_begin) -- the constant-velocity model of LOAM's TransformToStart,
 * the rotation interpolated on the geodesic, the translation linearly.  The output is the scan as seen from the sensor frame
 * at t_ref.  All rotations share one axis k, so a point p (the stored f32 record widened to f64) with time t_i becomes
 *   s     = (t_i - t_ref) / (t_end - t_begin)                 one subtraction, one division (the denominator computed once)
 *   theta = s * angle
 *   q     = p*cos(theta) + (k x p)*sin(theta) + k*(k . p)*(1 - cos(theta)) + s*tau_ref
 * with tau_ref = Exp(-u_ref w) tau computed once on the host.  Everything is evaluated in f64, every operation rounded on its
 * own (no fused multiply-add), and each coordinate is rounded once to f32; the fourth word of the record is carried as it is.
 * Times outside the sweep extrapolate: there is no clamp.  The definition is ONE function for host and device
 * (toyslam_amd/csrc/ndt_deskew.hpp); the two differ only by their libraries' sin / cos.
 *   - a record with a non-finite coordinate is copied unchanged, all four words bit for bit, whatever its time
 *   - a finite record with a non-finite time gets x = y = z = NaN (the quiet NaN 0x7fc00000), keeps its fourth word and is
 *     counted in *n_untimed; the !is_dense rules downstream then drop it
 *   - s == 0 gives q == p as f32 values (by ==, not bit for bit: a negative zero may become positive)
 * A motion is invalid if a field is not finite, t_end <= t_begin, angle lies outside [0, pi] or |axis| differs from 1 by more
 * than 1e-12. */
typedef struct {
  double t_begin, t_end, t_ref; /* finite, t_end > t_begin */
  double axis[3], angle;        /* unit axis ((1,0,0) when angle == 0), 0 <= angle <= pi */
  double tau_ref[3];            /* translation per unit s, already in the t_ref frame */
} ndt_deskew_motion;
/* - ndt_cloud_deskew: *out is a new cloud of its own (ndt_cloud_release) holding the n_in records of `in`, in in's order, moved
 *   as above, with both boxes exact over the records it wrote (route NDT_BOX_ROUTE_DESKEW) -- bit for bit what
 *   ndt_cloud_upload of the downloaded records would carry -- and usable by every consumer of an ndt_cloud.  An empty input
 *   gives an empty cloud, never NULL, with the initial boxes and route NONE.  times: n_in doubles, host memory or
 *   (times_on_device != 0) device memory; may be NULL for an empty cloud.  *n_untimed (may be NULL): the finite records whose
 *   time is not.  One kernel launch; the call returns after its own work is done (a borrowed view of a staged sequence may be
 *   overwritten afterwards).
 * - ndt_cloud_deskew_clouds: cloud k under motions[k]; times holds the clouds' times packed in cloud order (all on the host or
 *   all on the device).  One kernel launch in all.  out[k] and n_untimed[k] (n_untimed may be NULL) are the same bits as the
 *   single call for cloud k alone, whatever the other clouds and their order.  Every out[k] is a cloud of its own.
 *   n_clouds == 0 is NDT_OK, touches nothing and needs no device.  On any error every out[k] is NULL.
 * - ndt_diag_deskew, of the last of the two calls that reached the device: kernel launches (1 whatever the number of clouds;
 *   0 when no cloud had a point), its blocks, the clouds.
 * Neither changes the handle's target, source, grid, last result, statistics, map, a begun ndt_cloud_voxel_filter_begin, the
 * pairs state or what ndt_diag_select / ndt_diag_outliers report.
 * NDT_ERR_INVALID before any device work, outputs untouched apart from *out = NULL (every out[k] = NULL): a NULL handle, in,
 * motion or out, NULL times with points, an invalid motion, a NULL entry of in, more than 65 535 clouds, a cloud of another
 * device, more than INT_MAX points.  After those checks NDT_ERR_NO_DEVICE without a gfx950 device.
 * Development switch NDT_DESKEW_MAX_BLOCKS (read once): caps the blocks a cloud gets (the results do not depend on it). */
ndt_status ndt_cloud_deskew(ndt_handle h, ndt_cloud in, const ndt_deskew_motion* motion, const double* times /* n_in */,
                            int times_on_device, ndt_cloud* out, size_t* n_untimed /* or NULL */);
ndt_status ndt_cloud_deskew_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_deskew_motion* motions /* n_clouds */,
                                   const double* times /* packed in cloud order */, int times_on_device, ndt_cloud* out /* n_clouds */,
                                   size_t* n_untimed /* n_clouds or NULL */);
ndt_status ndt_diag_deskew(ndt_handle h, size_t* launches, size_t* blocks, size_t* clouds);
/* Host only, no device.
 * - ndt_host_deskew_motion: the motion of a sweep from T (16 floats, column-major: the sensor's pose at t_end in its frame at
 *   t_begin, e.g. the last registration increment under a constant-velocity assumption).  The rotation's logarithm is taken in
 *   f64: angle = atan2(|v|, (trace - 1) / 2) with v the vector of the antisymmetric part; the axis is v / |v| up to a quarter
 *   turn and beyond it comes from the symmetric part ((R + R^T)/2 - cos I) / (1 - cos) = k k^T (largest diagonal entry first,
 *   signs from v), because the antisymmetric part vanishes towards pi; angle == 0 gives the axis (1, 0, 0).
 *   tau_ref = Exp(-u_ref w) tau, u_ref = (t_ref - t_begin) / (t_end - t_begin).  NDT_ERR_INVALID: NULL T or out, a value that
 *   is not finite, t_end <= t_begin.
 * - ndt_host_deskew_point: the definition itself (the function the kernel calls) for one point; *untimed (may be NULL) = 1
 *   where the point is finite and its time is not.  NDT_ERR_INVALID for an invalid motion.
 * - ndt_host_deskew_plan: the launch plan of a cloud of n_points -- blocks of 256 threads, each owning one contiguous range of
 *   *points_per_block points (the last one the rest); at most 1024 blocks (NDT_DESKEW_MAX_BLOCKS: fewer), beyond which
 *   points_per_block grows. */
ndt_status ndt_host_deskew_motion(const float T[16], double t_begin, double t_end, double t_ref, ndt_deskew_motion* out);
ndt_status ndt_host_deskew_point(const ndt_deskew_motion* motion, const float xyz[3], double t, float out[3], int* untimed);
ndt_status ndt_host_deskew_plan(size_t n_points, int* blocks, int* points_per_block);

/* ---- outlier removal of resident clouds: the neighbourhood filters ----------------------------------------------------
 * Modelled on pcl::RadiusOutlierRemoval and pcl::StatisticalOutlierRemoval.  Neither class is part of the reference and PCL
 * itself was not at hand: NO bit parity with PCL is claimed, the definitions below are the contract.
 * A cloud has n records (x, y, z as stored, f32; the fourth word is carried along).  F = the indices whose three coordinates
 * are finite.  d2(i, j) = (dx*dx + dy*dy) + dz*dz in f32, every operation rounded on its own (no fused multiply-add).  The
 * "other points" of i are the j in F with j != i BY INDEX: duplicates of a point are neighbours at distance 0.
 *   RADIUS       r2 = radius*radius in f32; count_i = the other points with d2(i, j) <= r2; value_i = (double)count_i.
 *                Kept iff i in F and count_i >= min_neighbors (negate: count_i < min_neighbors).
 *   STATISTICAL  |F| > mean_k: value_i = (the sum, in f64 and in ascending order of d2, of sqrt((double)d2) over the mean_k
 *                smallest d2 of i's other points) / mean_k -- a pure function of the cloud; n_valid = |F|; mean = the mean of
 *                the values over F; stddev = sqrt(sum (v - mean)^2 / (n_valid - 1)), 0 when n_valid < 2 (per-block (count, sum,
 *                M2) merged by Chan's rule: no cancellation); threshold = mean + stddev_mul * stddev.
 *                |F| <= mean_k: every value is 0, n_valid = 0, mean = stddev = threshold = 0.
 *                Kept iff i in F and value_i <= threshold (negate: value_i > threshold).  The threshold a call returns is the
 *                one it compared with, bit for bit.
 * A point outside F has value NaN and is never kept, in either sense.
 * An invalid spec (NDT_ERR_INVALID before any device work): an unknown method, a radius that is not finite or <= 0,
 * min_neighbors < 0, mean_k outside 1 ... 256, a stddev_mul that is not finite. */
enum { NDT_OUTLIER_RADIUS = 1, NDT_OUTLIER_STATISTICAL = 2 };
typedef struct {
  int method, negate;
  float radius;      /* RADIUS      */
  int min_neighbors; /* RADIUS      */
  int mean_k;        /* STATISTICAL */
  double stddev_mul; /* STATISTICAL */
} ndt_outlier_spec;
typedef struct {
  size_t n_finite, n_valid;
  double mean, stddev, threshold; /* RADIUS: n_valid = n_finite, mean = stddev = 0, threshold = min_neighbors */
} ndt_outlier_stats;
/* - ndt_cloud_neighbor_values: value_i of every point of `in` into values (n_in doubles: host memory, or device memory with
 *   values_on_device != 0), and the statistics (stats may be NULL).
 * - ndt_cloud_remove_outliers: *out is a new cloud of its own holding the kept records of `in`, in in's order, all four words
 *   as they are, with exact boxes -- bit for bit what ndt_cloud_upload of the host-selected rows gives, as ndt_cloud_select
 *   promises.  The values are device-resident keys of that selection and never visit the host.  Nothing kept: an empty cloud,
 *   never NULL.  kept_idx (host, capacity n_in, may be NULL), *n_kept and *stats (may be NULL) as named.
 * - ndt_cloud_remove_outliers_clouds: one value launch over all clouds and the selection's two launches; out[k], n_kept[k]
 *   and stats[k] are the same bits as the single call for cloud k alone, whatever the other clouds and their order (every
 *   cloud has its own threshold).  n_clouds == 0 is NDT_OK, touches nothing and needs no device.  On any error every out[k]
 *   is NULL.
 * - ndt_diag_outliers, of the last of the three calls above that reached the device: point indices built, launches and
 *   blocks of the value kernel, and the queries that left the shell walk for the scan over the whole cloud.
 * None of them changes the handle's target, source, grid, last result, statistics, map, a begun
 * ndt_cloud_voxel_filter_begin, the pairs state or what ndt_diag_select reports.
 * NDT_ERR_INVALID before any device work, outputs untouched apart from *out = NULL (every out[k] = NULL): a NULL handle, in,
 * spec, values or out, an invalid spec, a NULL entry of in, more than 65 535 clouds, a cloud of another device, more than
 * INT_MAX points.  After those checks NDT_ERR_NO_DEVICE without a gfx950 device.
 * Development switch NDT_OUTLIER_MAX_BLOCKS: caps the blocks a cloud gets in the value kernel (the results do not depend on it). */
ndt_status ndt_cloud_neighbor_values(ndt_handle h, ndt_cloud in, const ndt_outlier_spec* spec,
                                     double* values /* n_in; host, or device with values_on_device */, int values_on_device,
                                     ndt_outlier_stats* stats /* or NULL */);
ndt_status ndt_cloud_remove_outliers(ndt_handle h, ndt_cloud in, const ndt_outlier_spec* spec, ndt_cloud* out,
                                     int32_t* kept_idx /* host, capacity n_in, or NULL */, size_t* n_kept /* or NULL */,
                                     ndt_outlier_stats* stats /* or NULL */);
ndt_status ndt_cloud_remove_outliers_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_outlier_spec* spec,
                                            ndt_cloud* out /* n_clouds */, size_t* n_kept /* n_clouds or NULL */,
                                            ndt_outlier_stats* stats /* n_clouds or NULL */);
ndt_status ndt_diag_outliers(ndt_handle h, size_t* index_builds, size_t* value_launches, size_t* value_blocks, size_t* scanned_queries);
/* Host only, no device: the validity of a spec (NDT_OK / NDT_ERR_INVALID), and the value kernel's plan for a cloud of
 * n_points -- blocks of one wave, eight queries (teams of eight lanes) per pass; one pass per block up to 4096 blocks, beyond
 * which the blocks stride over the passes.  *queries_per_block: the most queries one block works on. */
ndt_status ndt_host_outlier_spec_check(const ndt_outlier_spec* spec);
ndt_status ndt_host_outlier_plan(size_t n_points, int* blocks, int* queries_per_block);

/* ---- the plane of a resident cloud: RANSAC segmentation (the ground of a scan) ------------------------------------------
 * Modelled on pcl::SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE followed by pcl::ExtractIndices.  PCL's
 * RNG and its probabilistic early exit are not reproducible: NO bit parity with PCL is claimed, the definitions below are the
 * contract (ONE set of functions for host and device, toyslam_amd/csrc/ndt_plane.hpp).  All arithmetic is f64, every
 * operation rounded on its own (no fused multiply-add); coordinates are the stored f32 values widened.
 *   sample   the three indices of hypothesis h over a cloud of n points: idx_j = splitmix64(seed + 3 h + j) mod n, j = 0, 1, 2,
 *            with z = x + 0x9e3779b97f4a7c15; z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9; z = (z ^ z >> 27) * 0x94d049bb133111eb;
 *            splitmix64(x) = z ^ z >> 31 (u64 arithmetic).  A caller may pass its own triples instead: 3 * n_hypotheses int32
 *            in host memory; an index outside [0, n) makes the call NDT_ERR_INVALID.
 *   model    of a triple (a, b, c): u = b - a, v = c - a, m = u x v, len2 = (mx*mx + my*my) + mz*mz, uu and vv summed in the
 *            same order.  DEGENERATE (state 1, coefficients 0): two of the three indices equal, a point that is not finite,
 *            or !(len2 > 1e-8 * (uu * vv)).  Otherwise n = m / sqrt(len2), oriented: with an axis, a^ = axis / |axis| and
 *            cos_eps = cos((double)eps_angle) computed once on the host in f64, n is flipped so that n . a^ >= 0 and the
 *            hypothesis is REJECTED (state 2; its coefficients are still reported) unless n . a^ >= cos_eps; without an axis n
 *            is flipped so that its last non-zero component in the order z, y, x is positive.  d = -((nx*ax + ny*ay) + nz*az)
 *            with the oriented n.  A cloud of fewer than 3 points has only degenerate hypotheses.
 *   distance s = ((nx*px + ny*py) + nz*pz) + d; a point is an inlier iff -T <= s && s <= T, T = (double)distance_threshold.  A
 *            point that is not finite gives a NaN or infinite s and is never an inlier.
 *   choice   count(h) = the inliers of a VALID hypothesis (state 0), 0 for the others.  The best hypothesis is the valid one
 *            with the largest count, the lowest h among equals.  There is no early exit: every hypothesis is scored, the
 *            result is a pure function of (cloud, spec, triples).  No valid hypothesis: found = 0, best = -1, the coefficients
 *            are 0, the inlier cloud is empty and the other cloud holds every finite point (their keys are +inf).
 *   refine   (refine != 0 and found)  I = the inliers of the best plane, a = its first sample point, q = p - a;
 *            S1 = sum q (3 sums), S2 = sum q q^T (6 sums) over I -- on the device per block of 256 threads over a contiguous
 *            chunk (4096 points; beyond 64 blocks the chunk grows), a fixed tree per block, the blocks' rows added in block
 *            order on the host: deterministic, no floating-point atomics.  Covariance S2/|I| - (S1/|I|)(S1/|I|)^T; the normal
 *            is the eigenvector of its smallest eigenvalue (cyclic Jacobi in f64, ndt_host_plane_fit), oriented as above;
 *            d = -n . (a + S1/|I|).  The fit is taken when |I| >= 3, every number is finite and lambda_mid > 1e-12 lambda_max;
 *            otherwise the unrefined plane stays and refined = 0.  The angle test is not repeated.  The inliers are then
 *            those of the refined plane.
 * An invalid spec (NDT_ERR_INVALID before any device work): a distance_threshold that is not finite or <= 0, n_hypotheses
 * outside 1 ... 65 536, use_axis or refine other than 0 / 1, with use_axis an axis that is not finite or all zero or an
 * eps_angle outside 0 ... pi/2. */
typedef struct {
  float distance_threshold;
  int n_hypotheses;
  uint64_t seed;
  int use_axis;
  float axis[3];
  float eps_angle; /* radians */
  int refine;
} ndt_plane_spec;
typedef struct {
  int found, refined;
  double coeff[4];              /* nx, ny, nz, d of the plane the inliers were taken against */
  int best;                     /* the chosen hypothesis, -1 without one */
  size_t best_count, n_inliers; /* n_inliers == best_count without refinement */
  size_t n_finite, n_degenerate, n_rejected;
} ndt_plane_result;
/* - ndt_cloud_plane_counts: per hypothesis its model (coeffs: 4 * n_hypotheses doubles, may be NULL), its state (states:
 *   n_hypotheses int32, may be NULL) and its count (counts: n_hypotheses uint32), all host memory.  It changes nothing.
 * - ndt_cloud_segment_plane: *result as defined; *inliers and *others (either may be NULL: that cloud is not made) are new
 *   clouds of their own produced by the compaction of ndt_cloud_select with the signed distances as device-resident keys --
 *   KEY over [-T, T] gives the inliers, KEY | KEY_NEGATE | FINITE the others -- with that call's promises: records in in's
 *   order, all four words kept, exact boxes (bit for bit what ndt_cloud_upload of the host-selected rows gives), nothing kept
 *   gives an empty cloud, never NULL.  Rows that are not finite are in neither cloud.  The keys never visit the host.
 * - ndt_cloud_segment_plane_clouds: every cloud gets its own plane; triples always come from the sampler.  One model launch,
 *   one count launch, one choice launch, one key launch (with refinement one sums launch more) and two selection launches per
 *   kind of output cloud in all, whatever n_clouds.  results[k], inliers[k], others[k] are the same bits as the single call
 *   for cloud k alone, whatever the other clouds and their order.  n_clouds == 0 is NDT_OK, touches nothing and needs no
 *   device.  On any error every output cloud is NULL.
 * - ndt_cloud_plane_distances: s of every point of `in` under coeff into values (n_in doubles: host memory, or device memory
 *   with values_on_device != 0); a row that is not finite gives NaN.  The height above the ground, ready for a KEY selection
 *   of a height band.  A coeff that is not finite or has a zero normal is NDT_ERR_INVALID.
 * - ndt_diag_plane, of the last of the four calls above that reached the device: the plane kernels launched (counts: model,
 *   count, choice = 3; segmentation: + keys = 4, with a refinement that was asked for + sums = 5; distances: 1; when no
 *   cloud has a point the model and the choice launch alone = 2, distances: 0), the launches of the selections behind them
 *   (2 per kind of output cloud asked for, 0 when no cloud has a point), the blocks of the count launch, and the clouds.
 * None of them changes the handle's target, source, grid, last result, statistics, map, a begun
 * ndt_cloud_voxel_filter_begin, the pairs state or what ndt_diag_select / ndt_diag_outliers report.
 * NDT_ERR_INVALID before any device work, outputs untouched apart from the output clouds = NULL: a NULL handle, in, spec,
 * result(s), counts, coeff or values, an invalid spec, a triple index outside the cloud, a NULL entry of in, more than 65 535
 * clouds, a cloud of another device, more than INT_MAX points.  After those checks NDT_ERR_NO_DEVICE without a gfx950 device.
 * Development switches: NDT_PLANE_MAX_BLOCKS caps the count blocks a cloud gets, NDT_PLANE_MERGE=rows makes the count blocks
 * write partial rows that the choice launch sums in order instead of one integer atomic per lane (both read at every call;
 * no result depends on either). */
ndt_status ndt_cloud_plane_counts(ndt_handle h, ndt_cloud in, const ndt_plane_spec* spec, const int32_t* triples /* or NULL */,
                                  double* coeffs /* 4 * n_hypotheses or NULL */, int32_t* states /* n_hypotheses or NULL */,
                                  uint32_t* counts /* n_hypotheses */);
ndt_status ndt_cloud_segment_plane(ndt_handle h, ndt_cloud in, const ndt_plane_spec* spec, const int32_t* triples /* or NULL */,
                                   ndt_plane_result* result, ndt_cloud* inliers /* or NULL */, ndt_cloud* others /* or NULL */);
ndt_status ndt_cloud_segment_plane_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_plane_spec* spec,
                                          ndt_plane_result* results /* n_clouds */, ndt_cloud* inliers /* n_clouds or NULL */,
                                          ndt_cloud* others /* n_clouds or NULL */);
ndt_status ndt_cloud_plane_distances(ndt_handle h, ndt_cloud in, const double coeff[4],
                                     double* values /* n_in; host, or device with values_on_device */, int values_on_device);
ndt_status ndt_diag_plane(ndt_handle h, size_t* launches, size_t* select_launches, size_t* count_blocks, size_t* clouds);
/* Host only, no device: the validity of a spec; the sample (idx[3]; NDT_ERR_INVALID for n_points == 0 or h < 0); the model of
 * three points under a spec (*state 0 / 1 / 2, coeff[4]); the signed distance; the fit of the refinement from count, S1[3],
 * S2[6] (xx, xy, xz, yy, yz, zz) and a[3] (*taken = 0: refused, coeff untouched; lambda[3], may be NULL: the eigenvalues in
 * ascending order); and the count kernel's grid for a cloud of n_points -- tiles of *tile_points points x blocks of
 * *hyp_per_block hypotheses (256 threads, a lane per hypothesis), one block per pair up to 4096 blocks (NDT_PLANE_MAX_BLOCKS:
 * fewer), beyond which *tile_blocks < *tiles and the blocks stride over the tiles; the grid is *tile_blocks * *hyp_blocks. */
ndt_status ndt_host_plane_spec_check(const ndt_plane_spec* spec);
ndt_status ndt_host_plane_sample(uint64_t seed, int h, size_t n_points, int32_t idx[3]);
ndt_status ndt_host_plane_model(const ndt_plane_spec* spec, const float a[3], const float b[3], const float c[3], int same_index,
                                double coeff[4], int* state);
ndt_status ndt_host_plane_distance(const double coeff[4], const float xyz[3], double* s);
ndt_status ndt_host_plane_fit(const ndt_plane_spec* spec, double count, const double S1[3], const double S2[6], const double a[3],
                              double coeff[4], double* lambda /* 3 or NULL */, int* taken);
ndt_status ndt_host_plane_plan(size_t n_points, int n_hypotheses, int* tile_points, int* hyp_per_block, int* tiles, int* hyp_blocks,
                               int* tile_blocks);

/* ---- Euclidean cluster extraction of resident clouds: what stands on the ground, split into objects -------------------
 * Modelled on pcl::EuclideanClusterExtraction.  The class is not part of the reference and PCL itself was not at hand: NO bit
 * parity with PCL is claimed, the definitions below are the contract.
 * F, d2(i, j) and the "other points" of i are those of the outlier section above: d2 = (dx*dx + dy*dy) + dz*dz in f32, every
 * operation rounded on its own (no fused multiply-add), and j != i BY INDEX.  d2(i, j) == d2(j, i) bit for bit, so the
 * relation below is symmetric by construction.
 *   tol2       = tolerance*tolerance in f32.
 *   i ~ j      iff both are in F, i != j and d2(i, j) <= tol2 (duplicates of a point are joined: their distance is 0).
 *   component  a connected component of the graph (F, ~).  Its ROOT is its smallest point index, its SIZE its number of points.
 *   cluster    a component with min_size <= size <= max_size.  The clusters are numbered 0 ... C-1 by descending size, equal
 *              sizes by ascending root.
 *   label_i    the number of i's cluster; -1 when i's component is no cluster, and when i is not in F.
 *   root_i     the root of i's component; -1 when i is not in F.
 * An invalid spec (NDT_ERR_INVALID before any device work): a tolerance that is not finite or <= 0, or min_size, max_size for
 * which 1 <= min_size <= max_size does not hold. */
typedef struct {
  float tolerance;
  int min_size, max_size;
} ndt_cluster_spec;
/* One row of the cluster table: `first` is the offset of the cluster's run in `indices` (row c covers indices[first .. first +
 * size)); the box is the f32 min / max of the cluster's stored coordinates, exact; the centroid is the f64 sum of the widened
 * coordinates over the cluster's points divided by the size -- thread t of a block of 256 adds the run's entries t, t + 256,
 * ... in that order and the threads are added in a fixed tree, a shape that depends on the size alone: the same bits on every
 * run and whatever else is in the call.  No floating-point atomics anywhere. */
typedef struct {
  int32_t root, size;
  uint32_t first;
  float box_min[3], box_max[3];
  double centroid[3];
} ndt_cluster_info;
typedef struct {
  size_t n_finite, n_components, n_clusters; /* |F|, the components, C */
  size_t n_clustered, largest;               /* the points with label >= 0; the largest component, a cluster or not */
} ndt_cluster_summary;
/* - ndt_cloud_cluster: label_i into labels and (roots != NULL) root_i into roots, n_in int32 each, both in host memory or
 *   (labels_on_device != 0) both in device memory.  The first min(C, cluster_capacity) rows of the table into clusters (host;
 *   may be NULL with cluster_capacity == 0): the largest clusters, so "the 32 largest" is one call; summary->n_clusters always
 *   reports C.  indices (host, capacity n_in, may be NULL) receives the n_clustered clustered points grouped by cluster number,
 *   ascending inside a cluster -- PCL's vector<PointIndices>, flattened.  *summary may be NULL.
 * - ndt_cloud_extract_clusters: *out is a new cloud of its own holding the points with label >= 0 -- with negate != 0 the points
 *   of F with label < 0; a point outside F is never kept -- in in's order, all four words as they are, with exact boxes: bit
 *   for bit what ndt_cloud_upload of the host-selected rows gives, as ndt_cloud_select promises.  The per-point keys (1: in a
 *   cluster, 0: in none, NaN: not finite) are device-resident keys of that selection (KEY over [1, 1], or KEY | KEY_NEGATE) and
 *   never visit the host.  Nothing kept: an empty cloud, never NULL.  It needs the sizes alone: no ordering sort, no table.
 *   kept_idx (host, capacity n_in, may be NULL), *n_kept and *summary (may be NULL) as named.
 * - ndt_cloud_extract_clusters_clouds: one spec for many clouds; every kernel of the extraction is launched once whatever
 *   n_clouds, and the selection adds its two launches.  out[k], n_kept[k] and summaries[k] are the same bits as the single call
 *   for cloud k alone, whatever the other clouds and their order.  n_clouds == 0 is NDT_OK, touches nothing and needs no
 *   device.  On any error every out[k] is NULL.
 * - ndt_diag_clusters, of the last of the three calls above that reached the device: point indices built; launches of the
 *   extraction's own kernels (parents, link, flatten, keys = 4; 3 when no cloud has a finite point, 0 when none has a point;
 *   ndt_cloud_cluster adds the label pass, with C > 0 the two numbering passes, and the table pass when rows are written: up
 *   to 8 -- the sorts, the scans and the selection are not counted); the blocks of the link launch; the queries that left the
 *   shell walk for the scan over the whole cloud; and the compare-and-swaps of the union-find that failed and were retried
 *   (it varies from run to run; no result depends on it).
 * None of them changes the handle's target, source, grid, last result, statistics, map, a begun
 * ndt_cloud_voxel_filter_begin, the pairs state or what ndt_diag_select / ndt_diag_outliers / ndt_diag_plane report.
 * NDT_ERR_INVALID before any device work, outputs untouched apart from *out = NULL (every out[k] = NULL): a NULL handle, in,
 * spec, labels or out, NULL clusters with cluster_capacity > 0, an invalid spec, a NULL entry of in, more than 65 535 clouds,
 * a cloud of another device, more than INT_MAX points.  After those checks NDT_ERR_NO_DEVICE without a gfx950 device.
 * Development switch NDT_CLUSTER_MAX_BLOCKS (read at every call): caps the blocks a cloud gets in the link kernel (no result
 * depends on it). */
ndt_status ndt_cloud_cluster(ndt_handle h, ndt_cloud in, const ndt_cluster_spec* spec,
                             int32_t* labels /* n_in; host, or device with labels_on_device */, int labels_on_device,
                             int32_t* roots /* n_in, placed like labels, or NULL */, ndt_cluster_info* clusters /* cluster_capacity */,
                             size_t cluster_capacity, int32_t* indices /* host, capacity n_in, or NULL */,
                             ndt_cluster_summary* summary /* or NULL */);
ndt_status ndt_cloud_extract_clusters(ndt_handle h, ndt_cloud in, const ndt_cluster_spec* spec, int negate, ndt_cloud* out,
                                      int32_t* kept_idx /* host, capacity n_in, or NULL */, size_t* n_kept /* or NULL */,
                                      ndt_cluster_summary* summary /* or NULL */);
ndt_status ndt_cloud_extract_clusters_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_cluster_spec* spec, int negate,
                                             ndt_cloud* out /* n_clouds */, size_t* n_kept /* n_clouds or NULL */,
                                             ndt_cluster_summary* summaries /* n_clouds or NULL */);
ndt_status ndt_diag_clusters(ndt_handle h, size_t* index_builds, size_t* launches, size_t* link_blocks, size_t* scanned_queries,
                             size_t* cas_retries);
/* Host only, no device: the validity of a spec (NDT_OK / NDT_ERR_INVALID), and the link kernel's plan for a cloud of n_points
 * -- blocks of one wave, eight queries (teams of eight lanes) per pass; one pass per block up to 4096 blocks
 * (NDT_CLUSTER_MAX_BLOCKS: fewer), beyond which the blocks stride over the passes.  *queries_per_block: the most queries one
 * block works on. */
ndt_status ndt_host_cluster_spec_check(const ndt_cluster_spec* spec);
ndt_status ndt_host_cluster_plan(size_t n_points, int* blocks, int* queries_per_block);

/* ---- surface normals and curvature of resident clouds: the flat points, the walls, the edges ---------------------------
 * Modelled on pcl::NormalEstimation (setKSearch / setRadiusSearch, setViewPoint).  The class is not part of the reference and
 * PCL itself was not at hand: NO bit parity with PCL is claimed, the definitions below are the contract (the step from a
 * neighbourhood's sums to the record is ONE function for host and device, toyslam_amd/csrc/ndt_normals.hpp).
 * A cloud has n records (x, y, z as stored, f32; the fourth word is ignored).  F and d2(i, j) are those of the outlier section
 * above: F the indices whose three coordinates are finite, d2 = (dx*dx + dy*dy) + dz*dz in f32, every operation rounded on its
 * own (no fused multiply-add).
 *   N_i        the neighbourhood of i in F; the point itself is always a member, at distance 0 (as with PCL).
 *              NDT_NORMAL_KNN: the first min(k, |F|) indices of F in ascending (d2(i, j), j) order.
 *              NDT_NORMAL_RADIUS: the j in F with d2(i, j) <= r2, r2 = radius*radius in f32.   m_i = |N_i|.
 *   sums       about the query, in f64: e_j = (double)p_j - (double)p_i per coordinate, S1 = sum e_j (3 numbers), S2 = sum
 *              e_j e_j^T (6 numbers: xx xy xz yy yz zz), every product and addition rounded on its own.  The ORDER of the sums
 *              is the implementation's, a function of the cloud and the spec alone: KNN adds the neighbours of rank s, s + 8,
 *              ... (s = 0 ... 7) in that order and the eight partial sums in a fixed tree; RADIUS adds them in the order of a
 *              point index built from the cloud and the radius, every cell's points in ascending index.  No floating-point
 *              atomics anywhere.
 *   record     from (p_i, m, S1, S2):  mu = S1 / m, C = S2 / m - mu mu^T (symmetric); C solved by cyclic Jacobi in f64, the
 *              eigenvalues ascending l0 <= l1 <= l2, t = l0 + l1 + l2.  The point is VALID iff m >= min_neighbors, every entry
 *              of C is finite and t > 0.  n = the eigenvector of l0, renormalised in f64; s = n . ((double)viewpoint -
 *              (double)p_i): s < 0 flips n, s == 0 makes the component of largest magnitude (the first on ties) positive.
 *              curvature = max(l0, 0) / t.  The record is (float)n.x, (float)n.y, (float)n.z, (float)curvature, each rounded
 *              once: pcl::Normal's layout, 16 bytes per point.  An invalid point and a point outside F get four quiet NaNs
 *              (0x7fc00000); a point outside F has count 0, an invalid point of F its m_i.
 *   collinear  l1 <= 1e-12 * l2: the neighbourhood is a line.  The record is still valid -- whatever unit vector orthogonal to
 *              the line the solver returns -- and such points are counted in n_collinear.
 * An invalid spec (NDT_ERR_INVALID before any device work): an unknown method, k outside 3 ... 256 under KNN, a radius that is
 * not finite or <= 0 under RADIUS, min_neighbors < 3, a viewpoint that is not finite. */
enum { NDT_NORMAL_KNN = 1, NDT_NORMAL_RADIUS = 2 };
typedef struct {
  int method;
  int k;               /* KNN: 3 ... 256, the point itself included */
  float radius;        /* RADIUS: finite, > 0 */
  int min_neighbors;   /* >= 3; fewer members: no normal */
  double viewpoint[3]; /* finite; (0,0,0) = the sensor of a raw scan */
} ndt_normal_spec;
typedef struct {
  size_t n_finite, n_valid, n_collinear, max_neighbors; /* |F|, the valid records, the collinear ones among them, max m_i */
} ndt_normal_stats;
/* The filter of ndt_cloud_select_by_normals.  A point is kept iff its record is valid and every enabled test passes; NEGATE
 * inverts the outcome for valid records only; an invalid record is never kept; flags == 0 keeps every point that has a normal.
 *   CURVATURE  curvature_lo <= c && c <= curvature_hi on the stored f32.
 *   ANGLE      a = |(nx*ax + ny*ay) + nz*az| in f64 on the stored f32 record widened; cos_lo <= a && a <= cos_hi.
 * An invalid filter (NDT_ERR_INVALID): unknown bits; of an enabled test NaN bounds or lo > hi; with ANGLE an axis whose length
 * differs from 1 by more than 1e-12 (the deskew rule), or cosine bounds outside [0, 1]. */
enum { NDT_NORMAL_KEEP_CURVATURE = 1, NDT_NORMAL_KEEP_ANGLE = 2, NDT_NORMAL_KEEP_NEGATE = 4 };
typedef struct {
  unsigned flags;
  float curvature_lo, curvature_hi;
  double axis[3], cos_lo, cos_hi;
} ndt_normal_filter;
/* - ndt_cloud_estimate_normals: the record of every point into normals (4 * n_in floats) and m_i into counts (n_in int32, may
 *   be NULL), both in host memory or (on_device != 0) both in device memory.  *stats may be NULL.
 * - ndt_cloud_estimate_normals_clouds: one spec for many clouds, the outputs packed in cloud order (cloud k's records behind
 *   those of the clouds before it).  ONE normals launch whatever n_clouds.  Every cloud's records, counts and stats are the same
 *   bits as the single call for it alone, whatever the other clouds and their order.  n_clouds == 0 is NDT_OK, touches nothing
 *   and needs no device.
 * - ndt_cloud_select_by_normals: *out is a new cloud of its own holding the points the filter keeps, in in's order, all four
 *   words as they are, with exact boxes: bit for bit what ndt_cloud_upload of the host-selected rows gives, as ndt_cloud_select
 *   promises.  The keep decision is written on the device by the normals launch itself as the key of that selection (1: kept,
 *   0: not kept, NaN: not finite; KEY over [1, 1]); normals and keys never visit the host.  Nothing kept: an empty cloud, never
 *   NULL.  kept_idx (host, capacity n_in, may be NULL), *n_kept and *stats (may be NULL) as named.
 * - ndt_cloud_select_by_normals_clouds: the same for many clouds: one normals launch and the selection's two.  out[k],
 *   n_kept[k] and stats[k] are the same bits as the single call for cloud k alone.  On any error every out[k] is NULL.
 * - ndt_diag_normals, of the last of the four calls above that reached the device: point indices built (one per cloud with a
 *   point), normals launches (1; 0 when no cloud has a point), its blocks, and the queries that left the shell walk for the
 *   scan over the whole cloud.
 * The same bits: a cloud's records, counts and stats are bit-identical across the single and the list call, host and device
 * outputs, and every value of NDT_NORMAL_MAX_BLOCKS.
 * None of them changes the handle's target, source, grid, last result, statistics, map, a begun
 * ndt_cloud_voxel_filter_begin, the pairs state or what ndt_diag_select / ndt_diag_outliers / ndt_diag_plane /
 * ndt_diag_clusters report.
 * NDT_ERR_INVALID before any device work, outputs untouched apart from *out = NULL (every out[k] = NULL): a NULL handle, in,
 * spec, filter, normals or out, an invalid spec or filter, a NULL entry of in, more than 65 535 clouds, a cloud of another
 * device, more than INT_MAX points.  After those checks NDT_ERR_NO_DEVICE without a gfx950 device.
 * Development switch NDT_NORMAL_MAX_BLOCKS (read at every call; default and maximum 4096): caps the blocks a cloud gets in the
 * normals kernel (no result depends on it). */
ndt_status ndt_cloud_estimate_normals(ndt_handle h, ndt_cloud in, const ndt_normal_spec* spec,
                                      float* normals /* 4 * n_in; host, or device with on_device */,
                                      int32_t* counts /* n_in, placed like normals, or NULL */, int on_device,
                                      ndt_normal_stats* stats /* or NULL */);
ndt_status ndt_cloud_estimate_normals_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_normal_spec* spec,
                                             float* normals /* 4 * total points */, int32_t* counts /* total points or NULL */,
                                             int on_device, ndt_normal_stats* stats /* n_clouds or NULL */);
ndt_status ndt_cloud_select_by_normals(ndt_handle h, ndt_cloud in, const ndt_normal_spec* spec, const ndt_normal_filter* filter,
                                       ndt_cloud* out, int32_t* kept_idx /* host, capacity n_in, or NULL */,
                                       size_t* n_kept /* or NULL */, ndt_normal_stats* stats /* or NULL */);
ndt_status ndt_cloud_select_by_normals_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_normal_spec* spec,
                                              const ndt_normal_filter* filter, ndt_cloud* out /* n_clouds */,
                                              size_t* n_kept /* n_clouds or NULL */, ndt_normal_stats* stats /* n_clouds or NULL */);
ndt_status ndt_diag_normals(ndt_handle h, size_t* index_builds, size_t* launches, size_t* blocks, size_t* scanned_queries);
/* Host only, no device: the validity of a spec and of a filter (NDT_OK / NDT_ERR_INVALID); the kernel's plan for a cloud of
 * n_points -- blocks of one wave, eight queries (teams of eight lanes) per pass; one pass per block up to 4096 blocks
 * (NDT_NORMAL_MAX_BLOCKS: fewer), beyond which the blocks stride over the passes; *queries_per_block: the most queries one
 * block works on; the record of a point from its sums, the definition itself (out[4]; *collinear, may be NULL: 1 for a valid
 * record of a line); and the filter's decision on a record (*keep 0 / 1). */
ndt_status ndt_host_normal_spec_check(const ndt_normal_spec* spec);
ndt_status ndt_host_normal_filter_check(const ndt_normal_filter* filter);
ndt_status ndt_host_normal_plan(size_t n_points, int* blocks, int* queries_per_block);
ndt_status ndt_host_normal_from_sums(const ndt_normal_spec* spec, const float xyz[3], int m, const double S1[3], const double S2[6],
                                     float out[4], int* collinear /* or NULL */);
ndt_status ndt_host_normal_keep(const ndt_normal_filter* filter, const float record[4], int* keep);

/* ---- accumulating target: posed scans merged into the voxel grid (scan-to-MAP registration) --------------------------
 * Every other target of this library is built from ONE cloud; a mapping node that wants to register a scan against the map
 * would have to keep every posed point and rebuild the grid from the growing concatenation before each scan.  Here the
 * handle's target becomes an ACCUMULATED grid: per voxel the running first-pass sums of applyFilter (count, f64 sum /
 * outer-product sums seeded Identity, f32 centroid sums, _impl.hpp:209-263) and the finished record.  No points are kept:
 * memory is O(voxels), an update costs O(points of the update).
 * - Equivalence.  After any sequence of accumulate calls the handle behaves like a handle with the same parameters whose
 *   target was set from the concatenation -- in call order, and in cloud order within _clouds -- of the clouds moved by their
 *   poses: ndt_grid_size / _info / _dump return the same leaves, counts, means, covariances, inverse covariances and
 *   eigenvalues, and ndt_eval*, ndt_eval_hessian_f64, ndt_calculate_score, ndt_score_poses, ndt_calculate_nvtl, ndt_get_nvtl,
 *   ndt_nvtl_poses, ndt_source_point_nvtl, ndt_pose_covariance, ndt_align, ndt_align_guesses,
 *   ndt_align_multistart and ndt_align_batch* the same bits, for all four search methods (the evaluation kernels see an
 *   ordinary grid: the padded dense table, or the hash keyed by the reference's linear index; ndt_set_voxel_index chooses
 *   between the two as for a cloud target, by the points accumulated so far).  `pose` is a column-major 4x4, NULL =
 *   identity; the transform is N2's pcl::transformPointCloud in f32 (the device code of ndt_map_update*).  A non-finite
 *   row is left as it is by the transform and lands in no voxel (the is_dense == 0 rule; a cloud passed as dense must not
 *   hold one, as for ndt_set_input_target).
 * - _clouds: all clouds go through ONE pass (one transform launch, one key launch, one sort, one merge); the result has
 *   the bits of the same clouds accumulated one call at a time.  poses: 16 floats per cloud, NULL = identity for all.
 * - The first accumulate call on a handle REPLACES whatever target it held (it starts empty; a cloud target is not
 *   continued).  ndt_set_input_target*, ndt_share_input_target into the handle and ndt_promote_source_to_target replace the
 *   accumulated target; _reset empties it and leaves the handle with no target.  ndt_warm_up leaves it as it was.
 * - Resolution, min_points_per_voxel and the eigenvalue ratio are captured when a target starts (the first accumulate
 *   after create, reset or a replaced target); later changes of the last two apply from the next reset, as they apply from
 *   the next build for a cloud target.  ndt_set_resolution to a different value DROPS the accumulated target: there is no
 *   cloud to rebuild from.
 * - What needs the target's points, or shares the immutable grid with another handle, returns an error and changes
 *   nothing: ndt_get_fitness_score (and ndt_batch_fitness_scores*) NDT_ERR_NO_INPUT -- ndt_get_centroid_fitness_score, against
 *   the voxel centroids the target does keep, is the fitness of such a target; ndt_clone of, and
 *   ndt_share_input_target from, such a handle NDT_ERR_INVALID (ndt_target_accumulate_export + _import, below, give another
 *   handle the same map).
 * - Refused before anything of the target changes -- NDT_ERR_INVALID: a NULL handle, NULL points or clouds with a non-zero
 *   count, a NULL entry of clouds, a bad stride, more than INT_MAX points in one call, a finite point whose cell index
 *   floor(x / leaf) lies outside [-2^20, 2^20) on any axis (inside that range the reference's f32 index arithmetic,
 *   _impl.hpp:218-223, is exact and independent of the bounding box; outside it the voxel of a point would depend on the
 *   box); NDT_ERR_GRID_OVERFLOW: the union of the boxes would have more than INT_MAX cells.
 * - n == 0, or only empty clouds: NDT_OK, nothing changes, no device needed.
 * - ndt_target_accumulated: rows accumulated (non-finite ones included), occupied voxels, updates; zeros without an
 *   accumulated target.  ndt_diag_target_accumulate, of the last accumulate call: voxels it touched, voxels it created,
 *   whether every table entry was rewritten (the box, or the table's form or size, changed), whether the key table or the
 *   slot arrays were doubled, and the launches it queued (sort and scans count one each).
 * Development switches, read when a target starts: NDT_ACC_HASH_BITS (log2 of the initial key table, default 16) and
 * NDT_ACC_SLOTS (initial voxel slots, default 32768); both double on demand. */
ndt_status ndt_target_accumulate(ndt_handle h, const void* pts, size_t n, size_t stride_bytes, int is_dense, const float* pose);
ndt_status ndt_target_accumulate_device(ndt_handle h, const void* d_pts, size_t n, size_t stride_bytes, int is_dense, const float* pose);
ndt_status ndt_target_accumulate_cloud(ndt_handle h, ndt_cloud c, int is_dense, const float* pose);
ndt_status ndt_target_accumulate_clouds(ndt_handle h, const ndt_cloud* clouds, size_t n_clouds, int is_dense, const float* poses /* n*16 or NULL */);
ndt_status ndt_target_accumulate_reset(ndt_handle h);
ndt_status ndt_target_accumulated(ndt_handle h, size_t* n_points, size_t* n_voxels, size_t* n_updates);
ndt_status ndt_diag_target_accumulate(ndt_handle h, size_t* touched_voxels, size_t* new_voxels, int* relinked, int* table_grown, size_t* launches);
/* Crop the accumulated target to an axis-aligned box: a scan-to-map loop keeps a bounded map (a window around the vehicle)
 * instead of a target that only grows.  A voxel's sums depend only on the points of its own cell and on their order, so
 * dropping whole voxels leaves every kept voxel bit for bit what it would be had the dropped points never been accumulated.
 * - Cell range.  Per axis lo = floor(min * inv_leaf) and hi = floor(max * inv_leaf) with inv_leaf = 1.0f / resolution of the
 *   running target: the f32 product rounded before the floor, the arithmetic that bins a point.  Both are saturated to
 *   [-2^20, 2^20), so -INFINITY / +INFINITY leave a side open.
 * - Keep rule.  A voxel is kept exactly when its absolute cell lies in [lo, hi] on all three axes -- the cells a point inside
 *   the box could fall into.  Every other voxel is removed whatever its state (under min_points_per_voxel, valid, rejected).
 * - Equivalence.  After a crop, and after any later accumulate calls and further crops, the handle behaves like a handle with
 *   the same parameters whose target was set from the concatenation, in the original order, of every posed point accumulated
 *   so far whose cell lies inside every crop range applied AFTER that point was accumulated: the same dump (indices, counts,
 *   means, covariances, inverse covariances, eigenvalues, min_b / max_b / div_b) and the same bits from every evaluation and
 *   registration call listed above, for all four search methods.
 * - Box.  After a crop the box is the tight cell box of the kept voxels (what the concatenation's box gives: floor is
 *   monotone); a later update unions its own box with it as before.  The points' float extent is unknown after a crop, so
 *   the target then carries its box as the centres of the corner cells, (cell + 0.5f) * leaf, which floor back to those
 *   cells for |cell| < 2^20.  The reference's dx*dy*dz overflow refusal (NDT_ERR_GRID_OVERFLOW) is from then on decided from
 *   these cell extents, not from the points' extent: it can differ from the concatenation's only at the INT32_MAX edge.
 * - Bookkeeping.  ndt_target_accumulated's n_points becomes the sum of the kept voxels' counts (non-finite rows accumulated
 *   earlier lie in no voxel and are forgotten), n_voxels the kept voxels; n_updates is unchanged.  The dense-or-sparse rule
 *   of ndt_set_voxel_index is applied again with the new cell and point counts: a target that went sparse because its box
 *   grew comes back to the dense table.  Slot arrays and key table shrink to the smallest capacities (power-of-two multiples
 *   of the initial ones) that hold the kept voxels.
 * - Nothing removed: NDT_OK; nothing of the target is written, no table rewritten (removed_voxels == 0, relinked == 0).
 * - Everything removed: NDT_OK; the target is empty as after accumulating only non-finite points -- no box, 0 voxels, the
 *   captured parameters kept; the next accumulate starts its box afresh.
 * - A removed cell that receives points again starts from empty sums.
 * - Refused before anything changes and without a device -- NDT_ERR_INVALID: a NULL handle, NULL bounds, a NaN bound,
 *   min > max on an axis; NDT_ERR_NO_INPUT: no live accumulated target.
 * - One crop is mark + scan over the SLOTS, one read-back, and (if anything goes) compaction, key-table and look-up-table
 *   rebuild: five launches whatever was accumulated, none over points.  ndt_warm_up leaves a cropped target as it was.
 * ndt_diag_target_crop, of the last crop: voxels kept and removed, points kept, whether the tables were rebuilt, launches
 * (the scan counts one). */
ndt_status ndt_target_accumulate_crop(ndt_handle h, const float min_xyz[3], const float max_xyz[3]);
ndt_status ndt_diag_target_crop(ndt_handle h, size_t* kept_voxels, size_t* removed_voxels, size_t* kept_points, int* relinked, size_t* launches);
/* Clearing by rays: the accumulated target forgets what a later scan sees THROUGH.  The target keeps no points, so the
 * occupancy-map remedy is the one available: a scan whose beams pass through a voxel's cell and hit something behind it is
 * evidence that the cell is empty (a car that was parked and left, a pedestrian's trail, a door that has opened).
 * A call takes one or more resident clouds, each with a pose (column-major 4x4, NULL = identity) and a sensor origin o (three
 * f32 values in the map frame, NULL = the pose's translation), and a spec.
 * - Posed points.  Every finite record is moved by its pose with N2's f32 transform (what ndt_target_accumulate* does): p.  A
 *   non-finite row (or a row the pose moves to a non-finite p) gives no ray and no hit and is counted nowhere.
 * - Hit set H: the build cell floor(p * inv_leaf) (f32, the arithmetic that bins a point) of every posed point of the call,
 *   whatever its range.  A point whose build cell lies outside [-2^20, 2^20) on an axis gives no hit and no ray; it is not an
 *   error (it counts as a skipped ray).
 * - The ray of a point.  All arithmetic is f64, every operation rounded on its own.  L = (double)resolution of the running
 *   target, d = p - o, len = sqrt(dx*dx + dy*dy + dz*dz) summed in that order.  The ray is cast exactly when len > 0,
 *   min_range <= len <= max_range and t_end = 1 - margin / len > 0; otherwise it is skipped.  A cast ray covers o + t d for t in
 *   [0, t_end]: the last `margin` metres before the hit are never walked.
 * - The walk.  The start cell m has m_k L <= o_k < (m_k + 1) L on every axis (the products are exact in f64).  On an axis with
 *   d_k != 0: s_k = sign(d_k), f_k = m_k + (s_k > 0), t_k = (f_k L - o_k) / d_k; on any other axis t_k = +inf.  Repeat: take the
 *   axis a with the smallest t_a (the lowest axis wins a tie); stop unless t_a <= t_end; m_a += s_a, f_a += s_a; t_a is
 *   recomputed from the formula, never accumulated.  The visited cells are the start cell and every m after a step.  The walk
 *   also ends when m leaves [-2^20, 2^20); a start cell outside that range visits nothing.
 * - Decision.  miss(v) = the cast rays of the whole call, over all its clouds, that visit the cell of voxel v (a ray visits a
 *   cell at most once).  A voxel is removed exactly when miss(v) >= min_rays and its cell is not in H, whatever its state
 *   (under min_points_per_voxel, valid, rejected).
 * - Equivalence: the crop's, with "inside the crop range" replaced by "not removed": afterwards the handle behaves like a
 *   handle whose target was set from the concatenation, in the original order, of every accumulated point whose voxel no later
 *   crop or clearing removed -- the same dump, the same bits from every evaluation and registration call listed above, for all
 *   four search methods.  Box (the tight cell box of the kept voxels), n_points (the kept counts), the dense-or-sparse choice,
 *   the capacities, a removed cell that receives points again, ndt_warm_up: as after a crop.
 * - Nothing removed: NDT_OK, nothing of the target is written (n_points becomes the sum of the voxels' counts, as after a
 *   crop that removes nothing: non-finite rows accumulated earlier are forgotten).  Everything removed: the empty target of
 *   a crop that removes everything.
 * - Refused before anything changes and without a device -- NDT_ERR_INVALID: a NULL handle, a NULL spec, NULL clouds with a
 *   non-zero count, a NULL entry of clouds, a non-finite pose or origin, a spec that fails ndt_host_ray_spec_check for the
 *   target's resolution (all three lengths finite, 0 <= min_range <= max_range, max_range > 0, margin >= 0, min_rays >= 1,
 *   max_range / resolution <= 65536: a walk is at most 3 x 65537 steps), more than INT_MAX points in one call;
 *   NDT_ERR_NO_INPUT: no live accumulated target (checked after the NULL and finiteness checks, before the spec).
 *   Zero clouds, or only empty clouds: NDT_OK, nothing changes, no device needed.
 * - _clouds: all clouds go through ONE pass and the misses are summed over all of them; poses: 16 floats per cloud, origins: 3
 *   floats per cloud, either may be NULL.
 * - Device side: ONE ray launch over all points of all clouds (transform, hit flag, walk with a key-table probe per visited
 *   cell, integer miss counts: independent of order), the keep-flag launch and its scan, one read-back, and -- if anything
 *   goes and anything stays -- the crop's compaction, key-table and look-up-table rebuild: 3 launches when nothing or everything
 *   is removed, 6 otherwise, whatever the number of clouds and points (1 for a target without voxels).
 * - ndt_target_accumulate_ray_counts runs the same ray pass (1 launch) and removes nothing: nothing of the target is written.
 *   One row per voxel of the target in ascending key (the export's order): its cell (3 ints), its miss count, whether its cell
 *   is in H.  *n_voxels (may be NULL) = the rows; cells == NULL: only that.  capacity (in rows) too small: NDT_ERR_INVALID.
 * - ndt_diag_target_clear_rays, of the last of these calls that reached the device: rays cast and skipped (together the
 *   finite rows), the total of cells visited by cast rays, voxels with miss >= 1, voxels removed and kept and points kept
 *   (_ray_counts: what a clearing would have done), whether the tables were rebuilt, launches (the scan counts one).
 * Host only: ndt_host_ray_spec_check (the validity of a spec for a resolution); ndt_host_ray_cells walks ONE ray with the body
 * the kernel uses and applies no range test (len > 0 and t_end > 0 still hold, else *n = 0): *n = the cells visited, written
 * to cells (3 ints each) when it is not NULL; more cells than capacity: NDT_ERR_INVALID with *n set; ndt_host_ray_plan: the
 * grid of the ray kernel for the n_points of a call -- blocks of 256 threads, a thread per point up to 1024 blocks, beyond
 * which thread g takes the points g, g + 256 * blocks, ...; *passes = the most points one thread takes.
 * Development switches, read per call: NDT_RAYS_MAX_BLOCKS caps the blocks of the ray kernel; NDT_RAYS_MERGE=0 adds every miss
 * with an atomic of its own instead of merging the equal slots of a wave (the results depend on neither). */
typedef struct ndt_ray_spec {
  float min_range, max_range; /* metres: rays shorter or longer are skipped */
  float margin;               /* metres before the hit that are never walked */
  int min_rays;               /* misses a voxel needs to be removed */
} ndt_ray_spec;
ndt_status ndt_target_accumulate_clear_rays(ndt_handle h, ndt_cloud cloud, const float* pose, const float* origin, const ndt_ray_spec* spec);
ndt_status ndt_target_accumulate_clear_rays_clouds(ndt_handle h, const ndt_cloud* clouds, size_t n_clouds, const float* poses /* n*16 or NULL */,
                                                   const float* origins /* n*3 or NULL */, const ndt_ray_spec* spec);
ndt_status ndt_target_accumulate_ray_counts(ndt_handle h, const ndt_cloud* clouds, size_t n_clouds, const float* poses, const float* origins,
                                            const ndt_ray_spec* spec, int* cells /* 3 per row, or NULL */, unsigned* misses, unsigned char* hit,
                                            size_t capacity, size_t* n_voxels);
ndt_status ndt_diag_target_clear_rays(ndt_handle h, size_t* rays_cast, size_t* rays_skipped, uint64_t* cells_visited, size_t* touched_voxels,
                                      size_t* removed_voxels, size_t* kept_voxels, size_t* kept_points, int* relinked, size_t* launches);
ndt_status ndt_host_ray_spec_check(const ndt_ray_spec* spec, float resolution);
ndt_status ndt_host_ray_cells(const float origin[3], const float point[3], float resolution, float margin, int* cells, size_t capacity, size_t* n);
ndt_status ndt_host_ray_plan(size_t n_points, int* blocks, int* passes);
/* Export and import: voxels leave an accumulated target and enter another one (or the same one later) bit for bit -- a map
 * saved to a file and loaded by a later run, a second handle with the same map (ndt_clone / ndt_share_input_target keep
 * refusing accumulated targets: export + import is the way), tiles paged out when a crop window moves on and paged back in
 * when it returns.  A voxel's state is its absolute cell, its count and the twelve running sums; finishing it reads nothing
 * else, and it depends only on the points of its own cell and on their order.
 * - The blob (little-endian).  Header, 64 bytes: char magic[8] = "NDTACC1\0" at 0; u32 version = 1 at 8; u32 row_bytes = 104
 *   at 12; f32 resolution at 16; u32 0 at 20; u64 n_voxels at 24; i32 lo[3] at 32 and i32 hi[3] at 44, the tight cell box of
 *   the rows (all zero when n_voxels == 0); u64 checksum at 56.  Then n_voxels rows of 104 bytes: i32 i, j, k, count;
 *   f64 d[9] = sx sy sz cxx cxy cxz cyy cyz czz (the Identity seed included); f32 f[3], the centroid sums; f32 0.
 *   Rows are in strictly ascending key (ndt_host_acc_pack_cell: k high, i low), which is ascending linear index: a blob is
 *   canonical -- two targets that hold the same points per cell in the same order export identical bytes, whatever their
 *   history or slot order.  Checksum: h = 0xcbf29ce484222325, then per 8-byte word w of bytes [0, 56) followed by the rows
 *   h = (h ^ w) * 0x100000001b3 mod 2^64.  The blob holds no min_points_per_voxel and no eigenvalue ratio: the sums do not
 *   depend on them, and the importing target finishes the voxels under its own captured values.
 * - Export.  Both bounds NULL: every voxel.  Otherwise the cell range of ndt_target_accumulate_crop (same arithmetic, same
 *   saturation, the same refusals of NaN and min > max; exactly one NULL bound is NDT_ERR_INVALID).  Every voxel whose cell
 *   lies in the range is exported whatever its state.  The target is not changed: nothing of it is written.  *bytes = the
 *   size of the blob; buf == NULL: only that.  capacity too small: NDT_ERR_INVALID, nothing written.  No live accumulated
 *   target: NDT_ERR_NO_INPUT.  A selection of no voxel, or a target without voxels, gives the valid 64-byte blob.
 *   Device side: mark over the slots (the crop's kernel), hipCUB's stable sort of the (key, slot) pairs, one gather kernel
 *   that writes the rows in sorted order -- THREE launches whatever the number of voxels (ONE, the mark, for buf == NULL;
 *   none for a target without voxels) -- one read-back for the count, then the copy of the rows; the host writes the header
 *   and the checksum.  ndt_diag_target_export, of the last export or save: rows, the sum of their counts, launches.
 * - Import is an accumulate call in voxel form, with the start rule of ndt_target_accumulate*: a handle without a live
 *   accumulated target starts one (resolution, min_points_per_voxel and eigenvalue ratio captured; a cloud target is
 *   replaced, not continued), a live one is continued.  The blob's resolution must have the bits of that target's
 *   resolution, and every cell of the blob must be ABSENT from the target.  Imports and point updates may follow each other
 *   in any order.  New voxels take the slots after the existing ones, in blob order.  The box becomes the union of the
 *   current box with the centres of the blob's corner cells, (cell + 0.5f) * leaf; NDT_ERR_GRID_OVERFLOW and the
 *   dense-or-sparse rule are decided as in an update.  n_points grows by the sum of the rows' counts, n_voxels by the rows,
 *   n_updates by one; ndt_diag_target_accumulate reports the import as an update (touched = new = rows).
 * - Equivalence.  After any sequence of accumulate, crop and import calls the handle behaves like a handle with the same
 *   parameters whose target was set from one concatenation: every posed point accumulated directly and the points behind
 *   every imported voxel, each under the crops applied after it came in; within a cell the points in the order they were
 *   first accumulated, wherever that happened.  The same dump and the same bits from every evaluation and registration
 *   call listed above, for all four search methods.
 * - A blob of no rows: NDT_OK, nothing changes, no device needed.
 * - Import refuses, before anything changes and without a device, each with its own message -- NDT_ERR_INVALID: a NULL
 *   handle or blob, fewer than 64 bytes, the magic, the version, row_bytes, bytes != 64 + 104 * n_voxels, the checksum, a
 *   resolution that is not finite and positive, lo > hi or a box outside [-2^20, 2^20), a resolution other than the
 *   target's, more than 2^30 voxels in the target afterwards.  After ONE check launch over the uploaded rows and the one
 *   read-back, still before anything changes: a cell outside the header's box or a header box that is not the tight box of
 *   the rows, count < 1, a non-finite sum, keys not strictly ascending (duplicates included), a cell already in the target.
 *   Then growth and relink as an update, one placement launch and one finish launch over the new slots: 3 launches, plus one
 *   when the key table is rebuilt and one when the look-up table is relinked, whatever the number of voxels.
 * - _save is _export into a host buffer written to `path` through a temporary file in the same directory and a rename;
 *   _load is the whole file read and imported.  I/O failures: NDT_ERR_INVALID with the path and strerror.
 * ndt_host_acc_blob_info: the header of a blob that passes the device-free checks.  ndt_host_acc_blob_checksum: the hash
 * above over `bytes` (a multiple of 8) of data.  Both host only. */
ndt_status ndt_target_accumulate_export(ndt_handle h, const float min_xyz[3], const float max_xyz[3], void* buf, size_t capacity, size_t* bytes);
ndt_status ndt_target_accumulate_import(ndt_handle h, const void* blob, size_t bytes);
ndt_status ndt_target_accumulate_save(ndt_handle h, const float min_xyz[3], const float max_xyz[3], const char* path);
ndt_status ndt_target_accumulate_load(ndt_handle h, const char* path);
ndt_status ndt_diag_target_export(ndt_handle h, size_t* voxels, size_t* points, size_t* launches);
ndt_status ndt_host_acc_blob_info(const void* blob, size_t bytes, float* resolution, size_t* n_voxels, int lo[3], int hi[3]);
ndt_status ndt_host_acc_blob_checksum(const void* data, size_t bytes, uint64_t* out);
/* the key of the accumulated target's voxel table: the absolute cell (i, j, k), 21 bits per axis, k in the high bits so
 * that keys ascend with the linear voxel index.  Host only.  NDT_ERR_INVALID outside [-2^20, 2^20). */
ndt_status ndt_host_acc_pack_cell(int i, int j, int k, uint64_t* key);
void ndt_host_acc_unpack_cell(uint64_t key, int* i, int* j, int* k);

/* ---- PCD files (row N3 of the scope table) -----------------------------------
 * What pcl::io::loadPCDFile<pcl::PointXYZ> hands the callers (ndt_omp/apps/align.cpp:48-55,
 * ndt_omp_mapping_node.cpp:140, ndt_omp_node.cpp:82) and what pcl::io::savePCDFileBinary writes
 * (lidar_subscriber_node.cpp:46): PCD v0.7, DATA ascii | binary | binary_compressed; x, y, z are
 * picked by field name, other fields (intensity, rgb, ...) are skipped.  Host only, no device needed.
 * data_kind: 0 ascii, 1 binary, 2 binary_compressed.  Records written to `out` are x,y,z(,1.0f when
 * stride_bytes >= 16); *is_dense = every point finite (PCDReader's rule). */
ndt_status ndt_pcd_read_header(const char* path, size_t* n_points, int* n_fields, int* data_kind);
ndt_status ndt_pcd_read_xyz(const char* path, void* out, size_t capacity_points, size_t stride_bytes, size_t* n_points,
                            int* is_dense);
ndt_status ndt_pcd_write_xyz(const char* path, const void* pts, size_t n, size_t stride_bytes, int binary);
/* One named scalar field of a PCD file as doubles (the per-point time of a lidar driver's records, for ndt_cloud_deskew): TYPE F
 * of 4 / 8 bytes, I and U of 1, 2, 4 and 8 bytes, all three DATA kinds.  *n (may be NULL) = the file's points, also when
 * capacity is too small.  NDT_ERR_INVALID: a NULL path or name, NULL out with capacity, a file that cannot be parsed, a field
 * that is absent or has COUNT != 1, a type / size pair outside the list, more points than capacity. */
ndt_status ndt_pcd_read_field(const char* path, const char* name, double* out, size_t capacity_points, size_t* n_points);

/* A directory of numbered scans, as the mapping node consumes it (lidar_subscriber/src/ndt_omp_mapping_node.cpp):
 * process_new_clouds (:110-136) lists the *.pcd files whose number -- the integer after the last '_' of the file
 * stem (extract_file_number, :231-239) -- is >= loaded_clouds + 1 and loads them in ascending order; the node calls
 * it once at start-up and then once per second (:28-34, directory polling).  ndt_pcd_sequence_poll is that listing;
 * ndt_pcd_sequence_next hands out the queued files one by one as x, y, z, 1.0f records (16 bytes) in page-locked host
 * memory, and while the caller works on one scan the next file is read and parsed by a background thread (the two
 * buffers alternate; a scan stays valid until the following call of ndt_pcd_sequence_next).
 * next: *pts == NULL when nothing is queued.  A file that cannot be parsed returns NDT_ERR_INVALID and is skipped,
 * like load_and_filter_cloud's nullptr (:138-141).  Works without a device (pageable buffers then). */
typedef struct ndt_pcd_sequence* ndt_pcd_sequence_handle;
ndt_status ndt_pcd_sequence_open(const char* directory, ndt_pcd_sequence_handle* out);
ndt_status ndt_pcd_sequence_poll(ndt_pcd_sequence_handle s, size_t loaded_clouds, size_t* n_new_files);
ndt_status ndt_pcd_sequence_next(ndt_pcd_sequence_handle s, const void** pts, size_t* n, int* is_dense, int* file_number);
/* Scans staged into HBM by the reader: after ndt_pcd_sequence_stage(s, device) every scan is copied to the device as soon as
 * its file has been read (by the reading thread, on a copy stream of the sequence's own), and ndt_pcd_sequence_next_device
 * hands out the device records (16 bytes each, valid until the next call) together with the host ones -- the upload of scan
 * k + 1 runs while the caller registers scan k.  *d_pts == NULL with NDT_OK: nothing queued, as _next. */
ndt_status ndt_pcd_sequence_stage(ndt_pcd_sequence_handle s, int device);
ndt_status ndt_pcd_sequence_next_device(ndt_pcd_sequence_handle s, const void** d_pts, const void** host_pts, size_t* n, int* is_dense,
                                        int* file_number);
/* The same scan as an ndt_cloud: a VIEW of the staged records (the sequence owns the memory: valid until the next call of
 * a _next* function) that carries the bounding boxes the reading thread computed on the host while the copy ran -- a
 * prefilter of it needs nothing from the device before its kernels can be queued.  *cloud == NULL with NDT_OK: nothing
 * queued.  Release the view with ndt_cloud_release. */
ndt_status ndt_pcd_sequence_next_cloud(ndt_pcd_sequence_handle s, ndt_cloud* cloud, const void** host_pts, size_t* n, int* is_dense,
                                       int* file_number);
void ndt_pcd_sequence_close(ndt_pcd_sequence_handle s);
/* extract_file_number (:231-239) */
int ndt_host_extract_file_number(const char* file_stem);
/* pcl::fromROSMsg(sensor_msgs::PointCloud2, PointCloud<PointXYZ>) for the layouts lidar drivers publish
 * (ndt_rosbag_mapping_node.cpp:45-50): n records of point_step bytes with three f32 fields at byte offsets
 * off_x, off_y, off_z -- any step and any offsets, aligned or not (e.g. the 22-byte x,y,z,intensity,ring,time
 * records of a Velodyne driver) -- repacked into x, y, z, 1.0f records of 16 bytes, which is what every other
 * entry point takes with stride 16.  Host only.  *is_dense = every coordinate finite. */
ndt_status ndt_host_repack_fields(const void* data, size_t n, size_t point_step, size_t off_x, size_t off_y, size_t off_z,
                                  void* out_xyz1, int* is_dense);
/* The companion for one scalar field of such records (the time of a point): n values at byte `offset` of records of
 * point_step bytes -- any step and offset, aligned or not -- widened to doubles.  datatype: the sensor_msgs/PointField code,
 * 1 INT8, 2 UINT8, 3 INT16, 4 UINT16, 5 INT32, 6 UINT32, 7 FLOAT32, 8 FLOAT64 (little-endian).  Host only.  NDT_ERR_INVALID: an
 * unknown datatype, a field that does not fit into the record, NULL data / out with n > 0. */
ndt_status ndt_host_extract_field(const void* data, size_t n, size_t point_step, size_t offset, int datatype, double* out);

/* ---- batch (map-build mode: many sources against the one target) ----------
 * Registers n_scans sources in lock-step, one fused derivative launch per
 * line-search step for the whole batch.  Scan k is points
 * [offsets[k], offsets[k+1]) of `pts`.  guesses == NULL -> Identity.
 * Per-scan outputs are arrays of n_scans entries (any may be NULL). */
ndt_status ndt_align_batch(ndt_handle h, const void* pts, const size_t* offsets /* n_scans+1 */, size_t n_scans,
                           size_t stride_bytes, const float* guesses /* n_scans*16 or NULL */,
                           float* final_transformations /* n_scans*16 */, int* has_converged,
                           int* final_num_iteration, double* transformation_probability);
ndt_status ndt_align_batch_device(ndt_handle h, const void* d_pts, const size_t* offsets, size_t n_scans,
                                  size_t stride_bytes, const float* guesses, float* final_transformations,
                                  int* has_converged, int* final_num_iteration, double* transformation_probability);

/* How many independent lock-step groups ndt_align_batch* runs the batch as (each on a stream and a host thread of
 * its own, so one group's host-side Newton / More-Thuente steps and launches hide behind the other groups' kernels):
 * 0 = automatic (2 from 16 scans, 4 from 192), 1 = one lock-step loop.  Every scan's result is independent of the
 * members of its group and of the grouping: every scan is ordered on a lattice of its own and summed in its own blocks, so
 * a scan gets the same bits in any batch, group or rank.  Batches with an exchange step (communicator / all-reduce hook)
 * always run as one loop. */
ndt_status ndt_set_batch_groups(ndt_handle h, int n_groups);

/* ---- pairs (scan-to-scan: every pair against the voxel grid of its own target) -----------------------------------
 * Registers n_pairs (target, source) pairs of clouds in lock-step.  Cloud c is points [offsets[c], offsets[c+1]) of
 * `pts`; pairs[2*k] = target cloud, pairs[2*k+1] = source cloud of pair k.  A cloud named as target by several pairs is
 * gridded once; a cloud may be the target and the source of one pair.  Parameters (resolution, step, epsilon, iterations,
 * search method, min points per voxel ...) come from the handle; is_dense is the targets' NaN rule.  guesses == NULL ->
 * Identity.  Per-pair outputs have n_pairs entries; any output may be NULL.
 * Every pair gets the registration a handle with that target and source would get from ndt_align (a target without a valid
 * voxel included), and the same bits in any call: whatever the other pairs, their order or the grouping
 * (ndt_set_batch_groups).  The handle's own target, source, grid and last result are left as they were; ndt_get_stats
 * reports the pairs call.  The grids stay on the handle until the next pairs call (ndt_pairs_grid_*) or ndt_destroy.
 * NDT_ERR_INVALID before any device work: NULL offsets / pairs / clouds with a non-zero count, offsets that decrease, a
 * pair index >= n_clouds, more than 65535 pairs (one call's limit: split larger sets into several calls), a handle with a
 * communicator or an all-reduce hook (pairs are not sharded). */
ndt_status ndt_align_pairs(ndt_handle h, const void* pts, const size_t* offsets /* n_clouds+1 */, size_t n_clouds,
                           size_t stride_bytes, int is_dense, const int* pairs /* 2*n_pairs */, size_t n_pairs,
                           const float* guesses /* n_pairs*16 or NULL */, float* final_transformations /* n_pairs*16 */,
                           int* has_converged, int* final_num_iteration, double* transformation_probability);
/* the same over clouds already resident in HBM (e.g. from ndt_cloud_voxel_filter) */
ndt_status ndt_align_pairs_clouds(ndt_handle h, const ndt_cloud* clouds, size_t n_clouds, int is_dense, const int* pairs,
                                  size_t n_pairs, const float* guesses, float* final_transformations, int* has_converged,
                                  int* final_num_iteration, double* transformation_probability);
/* the grid the last pairs call built for cloud c (NDT_ERR_NO_INPUT if c was no target of it): as ndt_grid_size /
 * ndt_grid_info / ndt_grid_dump */
ndt_status ndt_pairs_grid_size(ndt_handle h, size_t cloud, size_t* n_leaves, size_t* n_valid);
ndt_status ndt_pairs_grid_info(ndt_handle h, size_t cloud, int* min_b /*3*/, int* max_b /*3*/, int* div_b /*3*/);
ndt_status ndt_pairs_grid_dump(ndt_handle h, size_t cloud, int64_t* idx, int* nr_points, double* mean, double* cov,
                               double* icov, double* evals);
/* getFitnessScore of every pair of the last ndt_align_pairs* call: pair k's source moved by transforms[16k..] (column-major,
 * NULL = that call's final transformations) against pair k's target, as ndt_get_fitness_score would compute it on a handle
 * holding that target and source after an align ending at that transform -- the same bits.  All pairs in one launch.
 * NDT_ERR_NO_INPUT when the last pairs call failed or had no pair (the sources, grids and transformations a successful
 * call keeps are dropped when the next one begins, or by ndt_destroy); NDT_ERR_INVALID for a NULL handle or fitness. */
ndt_status ndt_pairs_fitness_scores(ndt_handle h, const float* transforms /* n_pairs*16 or NULL */, double max_range,
                                    double* fitness /* n_pairs */);
/* the number of pairs ndt_pairs_fitness_scores would score (those of the last pairs call; 0 after a failed or empty one):
 * how many transforms it reads and fitness values it writes */
ndt_status ndt_pairs_count(ndt_handle h, size_t* n_pairs);
/* the same for n_scans clouds against the handle's target (ndt_align_batch's layout; transforms required).  Keeps nothing
 * and runs no collective, even on a handle with a communicator.  NDT_ERR_INVALID before any device work: NULL handle,
 * offsets or (with scans) transforms / fitness, offsets that decrease, a bad stride, more than 65535 scans;
 * NDT_ERR_NO_INPUT without a target. */
ndt_status ndt_batch_fitness_scores(ndt_handle h, const void* pts, const size_t* offsets /* n_scans+1 */, size_t n_scans,
                                    size_t stride_bytes, const float* transforms /* n_scans*16 */, double max_range,
                                    double* fitness /* n_scans */);
ndt_status ndt_batch_fitness_scores_device(ndt_handle h, const void* d_pts, const size_t* offsets, size_t n_scans,
                                           size_t stride_bytes, const float* transforms, double max_range, double* fitness);
/* diagnostics: the k_fitness_multi launches of the handle's last ndt_pairs_fitness_scores / ndt_batch_fitness_scores* call
 * and the blocks of the largest (its partial rows, kEvalStride doubles each, are all that call held at once) */
ndt_status ndt_diag_fitness_launches(ndt_handle h, size_t* launches, size_t* max_blocks);

/* ---- the centroid cloud of the target, and getFitnessScore against it ----------------------------------------------------
 * The CENTROID CLOUD C of the handle's target -- built from a cloud or accumulated -- is the reference's voxel_centroids_: one
 * point per voxel that reached min_points_per_voxel (a voxel rejected afterwards, nr_points == -1 in ndt_grid_dump, IS in it:
 * the reference pushes the centroid before it looks at the eigenvalues; a voxel under min_points_per_voxel is not), each the
 * voxel's f32 centroid -- the f32 coordinate sums in arrival order divided by float(count) -- in ascending linear voxel index
 * (for an accumulated target over its current box, as ndt_grid_dump reports it).  An accumulated target keeps no points, but
 * it keeps C: this is the fitness a scan-to-map loop reads after ndt_align.
 * - ndt_grid_centroids: C as x, y, z, 1.0f per point and (idx != NULL) the linear indices; *n = its size in every case.
 *   xyz1 == NULL: only *n.  capacity < *n: NDT_ERR_INVALID, neither array written.  One mark + scan + gather over the voxel
 *   table (sparse index: the occupied hash slots sorted by key instead of the scan) and the read-back of the count.
 * - ndt_grid_centroids_cloud: C as a resident ndt_cloud in the same order (ndt_cloud_release it), usable wherever an
 *   ndt_cloud is: ndt_set_input_target_cloud, ndt_cloud_download, gicp_set_input_*_cloud ...  An empty C is a cloud of 0 points.
 * - ndt_get_centroid_fitness_score: what ndt_get_fitness_score would return on a handle whose target POINTS are C -- the
 *   handle's source moved in f32 by the last align's final transformation, every finite point's nearest point of C by f32
 *   (dx*dx + dy*dy) + dz*dz, the f64 mean of the squared distances <= max_range; DBL_MAX when none qualifies, C is empty or
 *   the source has no finite point.  Same readiness rule (a target and a source: NDT_ERR_NO_INPUT otherwise).  The search is
 *   exact for every query and every centroid position: it walks shells of cells through the target's own voxel table (no
 *   index is built, nothing is rebuilt when the map changes), and gives way by the grid's EXCURSION -- the largest per-axis
 *   distance by which a centroid of C lies outside the box of its own cell (an f32 running sum drifts far from the origin;
 *   0 when every centroid is inside).  The excursion takes one launch over the table and is cached per grid: computed once
 *   for a cloud target, again by the next fitness call after every ndt_target_accumulate*, _import, _load or _crop.
 * - ndt_batch_centroid_fitness_scores*: the same for n_scans clouds, scan k moved by transforms[16k..] (ndt_batch_fitness_scores'
 *   layout and refusals: NDT_ERR_INVALID before any device work for a NULL handle, offsets or (with scans) transforms /
 *   fitness, offsets that decrease, a bad stride, more than 65535 scans or INT_MAX points; NDT_ERR_NO_INPUT without a
 *   target; n_scans == 0: NDT_OK, no device needed).  All members in one search launch plus one reduce launch; sums in a
 *   fixed order, so results are identical run to run, and a scan's value does not depend on the scans around it.
 * - ndt_diag_centroid_fitness, of the last fitness call above: the launches it queued (search, reduce, and the excursion
 *   pass if it ran), the excursion passes among them (0 or 1), the excursion in metres it searched with, and the blocks of
 *   its search launch.  Any pointer may be NULL.
 * None of these calls changes the handle's target, source, grid, last result or statistics. */
ndt_status ndt_grid_centroids(ndt_handle h, float* xyz1 /* capacity*4 or NULL */, int64_t* idx /* capacity or NULL */, size_t capacity,
                              size_t* n);
ndt_status ndt_grid_centroids_cloud(ndt_handle h, ndt_cloud* out);
ndt_status ndt_get_centroid_fitness_score(ndt_handle h, double max_range, double* fitness);
ndt_status ndt_batch_centroid_fitness_scores(ndt_handle h, const void* pts, const size_t* offsets /* n_scans+1 */, size_t n_scans,
                                             size_t stride_bytes, const float* transforms /* n_scans*16 */, double max_range,
                                             double* fitness /* n_scans */);
ndt_status ndt_batch_centroid_fitness_scores_device(ndt_handle h, const void* d_pts, const size_t* offsets, size_t n_scans,
                                                    size_t stride_bytes, const float* transforms, double max_range, double* fitness);
ndt_status ndt_diag_centroid_fitness(ndt_handle h, size_t* launches, size_t* excursion_passes, float* excursion, size_t* max_blocks);

/* ---- one source, many poses (re-localisation in a map, loop-closure checks, recovery after a dropped scan) ------------
 * The caller holds candidate poses of the handle's input source and wants the one that registers.
 *
 * ndt_score_poses: calculateScore (ndt_omp_impl.hpp:935-983) of the handle's input source moved by each of n_poses transforms
 * (column-major 4x4 f32, as ndt_align's guess), against the handle's target grid, search method and Gauss constants.
 * scores[g] is what ndt_calculate_score returns for pcl::transformPointCloud(source, transforms + 16 g) -- the same bits --
 * without the host transform, the upload and the launches per pose: one launch scores up to NDT_SCORE_POSES_CHUNK poses
 * (default 4096, 1 .. 65535; fewer while a chunk's partial rows would exceed 256 MiB), one read-back per launch.  The source
 * is walked in the caller's order; non-finite points count in the divisor and add nothing; an empty grid gives 0.0, a pose
 * that moves every point out of the grid gives 0.0, a source of no points gives NaN (0 / 0 in the reference).
 * n_poses == 0: NDT_OK, nothing written, no device needed.  NDT_ERR_INVALID before any device work: NULL handle, NULL
 * transforms or scores with n_poses > 0, a handle with a communicator or an all-reduce hook.  Then NDT_ERR_NO_DEVICE without
 * a gfx950 device, NDT_ERR_NO_INPUT without a target or a source. */
ndt_status ndt_score_poses(ndt_handle h, const float* transforms /* n_poses*16 */, size_t n_poses, double* scores /* n_poses */);
/* diagnostics: the k_score_poses launches of the handle's last ndt_score_poses call that reached the device, and the blocks
 * of all of them together (poses x the blocks ndt_calculate_score walks a cloud of the source's size with) */
ndt_status ndt_diag_score_poses(ndt_handle h, size_t* launches, size_t* blocks);
/* ndt_align of the handle's source against its target from each of n_guesses guesses, in lock-step (one source in HBM,
 * every member a view of it).  Outputs as ndt_align_batch's, any may be NULL; *best = index of the largest
 * transformation_probability (NaN never wins, ties to the lower index, -1 if none -- also for n_guesses == 0, which writes
 * nothing else).  Member g's outputs are, bit for bit, those of member g of ndt_align_batch over the source repeated
 * n_guesses times (a source of 65 536 points and more is read from the handle's own ordered copy: the order a batch gives
 * it while its box has at most 4e6 cells of the resolution).  One lock-step loop (no batch groups); at most 65535 guesses.  Argument and state errors as
 * ndt_score_poses.  The handle's own last result (ndt_get_result) is left as it was; ndt_get_stats follows ndt_align_batch. */
ndt_status ndt_align_guesses(ndt_handle h, const float* guesses /* n_guesses*16 */, size_t n_guesses, float* final_transformations,
                             int* has_converged, int* final_num_iteration, double* transformation_probability, int* best);
/* indices of the `keep` largest finite scores, best first, ties to the lower index; *n_out <= keep (fewer when fewer are
 * finite).  Host only. */
void ndt_host_pick_top(const double* scores, size_t n, size_t keep, int* idx_out /* min(keep, n) */, size_t* n_out);
/* ndt_score_poses over the candidates, ndt_host_pick_top, ndt_align_guesses from the picked ones.  picked[k] = candidate
 * index of member k; the per-member outputs have *n_picked entries (room for min(keep, n_candidates)); *best indexes the
 * candidates (-1 if none: no candidate, keep == 0, or no finite score).  Any output may be NULL. */
ndt_status ndt_align_multistart(ndt_handle h, const float* candidates /* n_candidates*16 */, size_t n_candidates, size_t keep,
                                int* picked, size_t* n_picked, float* final_transformations, int* has_converged,
                                int* final_num_iteration, double* transformation_probability, int* best);

/* ---- nearest-voxel transformation likelihood (NVTL): is this pose right? ----------------------------------------------
 * calculateScore averages a point's terms over ALL its neighbour voxels and divides by ALL points of the scan: its value
 * moves with the search method's neighbour count and with how much of the scan overlaps the (possibly partly loaded) map.
 * NVTL takes, per point, the best-fitting neighbour voxel and averages over the points that have a neighbour at all, so a
 * fixed acceptance threshold holds across maps; per point it tells a point the map does not explain (a moving object).
 *
 * Definition.  Inputs: a point p (f32, used as given), the handle's target grid, its search method and (d1, d2, d3) =
 * gauss_constants(resolution, outlier_ratio).
 *  1. p has the neighbour set of calculateScore (ndt_calculate_score), exactly: empty for a non-finite p or a p more than a
 *     cell outside the grid's box; DIRECT1 / DIRECT7 / DIRECT26: the valid voxels at the method's cell offsets; KDTREE: the
 *     voxels of the centroid cloud in the 3x3x3 block whose f32 centroid is closer than the resolution.
 *  2. Each neighbour record r gives q_r = x^T C_r^-1 x in f64, x = double(p) - mean_r, with the f64 inverse covariance and
 *     calculateScore's association: (c00 x0 + c01 x1) + c02 x2 per row, then (x0 c0 + x1 c1) + x2 c2.
 *  3. q_min starts at +inf and becomes q_r whenever q_r < q_min, in neighbour order: a NaN q_r never wins.
 *  4. L(p) = -d1 exp(-d2 q_min / 2) when the set is not empty: one exp per point.  For d2 > 0 (every outlier ratio in (0, 1))
 *     this is max_r(-d1 exp(-d2 q_r / 2)), the usual wording; the q_min form is the definition for every d2.  A point with
 *     an empty set is NOT FOUND and adds nothing.
 *  5. NVTL = (sum of L(p) over the found points) / n_found, in f64, summed in a fixed order (per-thread walk of the points,
 *     block fold, fixed-order sum of the blocks): identical run to run.  n_found == 0 -- an empty grid, an empty cloud, every
 *     point far away or non-finite -- gives 0.0: never NaN, never an error.
 *
 * - ndt_calculate_nvtl: of `cloud`, used as given (the sibling of ndt_calculate_score).  *n_found may be NULL.
 * - ndt_get_nvtl: of the handle's source moved in f32 by the last align's final transformation (ndt_get_fitness_score's
 *   transformation; the identity before any align).
 * - ndt_nvtl_poses: of the handle's source under each of n_poses transforms (ndt_score_poses' layout, chunking --
 *   NDT_SCORE_POSES_CHUNK and the 256 MiB bound -- and checks), one launch per chunk.  nvtl[g] has the bits of
 *   ndt_calculate_nvtl of pcl::transformPointCloud(source, transforms + 16 g), of ndt_source_point_nvtl's reduction for that
 *   pose, and (for the final transformation) of ndt_get_nvtl.  n_found (n_poses entries) may be NULL.
 * - ndt_source_point_nvtl: L(p) of every source point under `transform` (NULL: the last align's final transformation), in the
 *   caller's point order, -1.0 for a point that was not found (L itself is never negative).  out (host, n_source doubles)
 *   and d_out (receives a device pointer to the same values, valid until the next ndt_source_point_nvtl on the handle or its
 *   destruction) may each be NULL; *nvtl / *n_found (may be NULL) are the reduction of the same launch.
 *   ndt_source_point_count sizes `out`: the points of the handle's input source, 0 without one (host only, no device needed).
 * - ndt_diag_nvtl, of the last of the four calls above that reached the device: its launches (k_nvtl / k_nvtl_poses) and the
 *   blocks of all of them together.
 * NDT_ERR_INVALID before any device work: a NULL handle, a NULL nvtl (ndt_calculate_nvtl, ndt_get_nvtl), a NULL cloud with
 * n > 0, a bad stride, more than INT_MAX points; for ndt_nvtl_poses what ndt_score_poses refuses, and n_poses == 0 is NDT_OK,
 * writes nothing and needs no device.  Then NDT_ERR_NO_DEVICE without a gfx950 device, then NDT_ERR_NO_INPUT without a target
 * (or, for the three calls that read it, a source).  No call changes the handle's target, source, grid, last result
 * (ndt_get_result), statistics (ndt_get_stats) or the ndt_diag_score_poses counters.  Dense and sparse voxel index, cloud and
 * accumulated targets alike. */
ndt_status ndt_calculate_nvtl(ndt_handle h, const void* cloud, size_t n, size_t stride_bytes, double* nvtl, size_t* n_found);
ndt_status ndt_get_nvtl(ndt_handle h, double* nvtl, size_t* n_found);
ndt_status ndt_nvtl_poses(ndt_handle h, const float* transforms /* n_poses*16 */, size_t n_poses, double* nvtl /* n_poses */,
                          size_t* n_found /* n_poses or NULL */);
ndt_status ndt_source_point_count(ndt_handle h, size_t* n_source);
ndt_status ndt_source_point_nvtl(ndt_handle h, const float* transform /* 16 or NULL */, double* out /* n_source or NULL */,
                                 const double** d_out, double* nvtl, size_t* n_found);
ndt_status ndt_diag_nvtl(ndt_handle h, size_t* launches, size_t* blocks);

/* ---- pose covariance: how well is each of the six pose components determined? -----------------------------------------
 * A filter that fuses the registered pose with odometry, GNSS or an IMU needs a 6x6 covariance per registration, a pose-graph
 * back end one information matrix per edge.  Two estimates, over the pose ordered x y z roll pitch yaw:
 *   Laplace  : cov = scale A^-1.  The NDT score is not a normalised log-likelihood, so `scale` is the caller's to tune.
 *   sandwich : cov = A^-1 B_c A^-1 (the M-estimator covariance).  Unchanged when the objective is scaled: no tuning constant;
 *              a direction A hardly constrains (a corridor, a plane) comes out with a large variance.
 *
 * Definition.  Inputs: the handle's source, target grid, search method and (d1, d2, d3) = gauss_constants(resolution,
 * outlier_ratio); a 4x4 f32 column-major `transform` (NULL: the last align's final transformation, the identity before any
 * align); the pose p = ndt_host_matrix_to_pose(transform).
 *  1. Source point x_i is moved in f32 by `transform` (as ndt_eval_with_matrix moves it) to x'_i, which has the neighbour set
 *     computeHessian gives it: empty for a non-finite x'_i or one outside the grid, else the search method's voxels.
 *  2. J_i is computeHessian's f64 3x6 point Jacobian (identity | angle columns), built from the UNMOVED x_i and the f64
 *     angle-derivative table at p (ndt_host_angle_derivatives' j_ang_d), each entry (a0 x + a1 y) + a2 z.
 *  3. Neighbour record r: xt = double(x'_i) - mean_r, Cx = C_r^-1 xt with computeHessian's association ((c0 x0 + c1 x1) + c2 x2
 *     per row), w_r = d2 exp(-d2 (xt . Cx) / 2); the neighbour is skipped when w_r > 1, w_r < 0 or w_r is NaN; else
 *     w_r <- w_r d1.
 *  4. g_i[k] = sum over r of w_r (Cx . J_i[:,k]), k = 0..5, all f64, in neighbour order; the dot product is
 *     (Cx0 J0k + Cx1 J1k) + Cx2 J2k with J's structural zeros and ones not multiplied (g_i[0..2] add w_r Cx itself).  A point
 *     with no neighbour that contributes is NOT FOUND and adds nothing.
 *  5. g = sum_i g_i (6), B = sum_i g_i g_i^T (upper triangle, 21) and n_found, summed in the fixed order of the evaluation
 *     kernels (per-thread walk of the points, block fold, fixed-order sum of the blocks): identical run to run.
 *  6. H = what ndt_eval_hessian_f64 computes for the same moved cloud and p (for a transform that is ndt_host_pose_to_matrix(p)
 *     exactly: that call's bits); A = -(H + H^T) / 2.
 *  7. B_c = B - g g^T / n_found; n_found == 0: B_c = B, the zero matrix.
 *  8. Host algebra in f64 on the six Jacobi eigenpairs (lambda_k, v_k) of A.  NDT_COV_INDEFINITE is set when n_found < 6 or
 *     min lambda <= 1e-12 max lambda (that includes max lambda <= 0, and a NaN); then all 36 entries of cov are NaN.
 *     Otherwise A^-1 = V diag(1 / lambda) V^T, Laplace cov = scale A^-1, sandwich cov = A^-1 B_c A^-1, either symmetrised as
 *     (M + M^T) / 2.
 *
 * - ndt_pose_covariance: of the handle's source against its target.  cov: 36 doubles, row-major.  info (may be NULL) receives
 *   A, the uncentred B and g, n_found, the extreme eigenvalues of A and the flags.  `scale` is ignored by the sandwich; for
 *   Laplace it must be finite and > 0.
 * - ndt_pairs_pose_covariances: of every pair of the last ndt_align_pairs* call, against the grid that call built for the
 *   pair's target, at transforms + 16 k (NULL: the pair's final transformation): one launch of the gradient kernel for all
 *   pairs.  cov: n_pairs * 36, info: n_pairs entries or NULL.  Pair k's outputs have the bits ndt_pose_covariance gives on a
 *   handle that holds that pair (for sources below the size at which a handle re-orders its source, 65 536 points).
 * - ndt_host_pose_covariance: steps 7 and 8 alone, host only (A, B: 36 row-major each, g: 6); eig_min, eig_max and flags may
 *   be NULL.  The device calls' cov is this function of their info, bit for bit.
 * - ndt_diag_pose_covariance: launches of the gradient kernel (k_grad_outer / k_grad_outer_multi) in the last of the two device
 *   calls that reached the device, and the blocks that did work in them.
 * NDT_ERR_INVALID before any device work: a NULL handle, a NULL cov, an unknown method, a bad Laplace scale, a handle with a
 * communicator or an all-reduce hook.  Then NDT_ERR_NO_DEVICE, then NDT_ERR_NO_INPUT without a target or a source (pairs: when
 * the last pairs call failed, had no pair or was never made).  An empty grid or an empty source is NDT_OK with n_found = 0,
 * the flag set and a NaN cov.  Neither call changes the target, source, grid, last result, ndt_get_stats or the other diag
 * counters.  Dense and sparse voxel index; cloud, accumulated and cropped targets alike. */
typedef struct {
  double A[36], B[36], g[6]; /* row-major; B is uncentred */
  size_t n_found;
  double eig_min, eig_max;   /* of A */
  int flags;                 /* NDT_COV_INDEFINITE */
} ndt_pose_information;
enum { NDT_COV_LAPLACE = 0, NDT_COV_SANDWICH = 1 };
enum { NDT_COV_INDEFINITE = 1 };
ndt_status ndt_pose_covariance(ndt_handle h, const float* transform /* 16 or NULL */, int method, double scale, double* cov /* 36 */,
                               ndt_pose_information* info /* or NULL */);
ndt_status ndt_pairs_pose_covariances(ndt_handle h, const float* transforms /* n_pairs*16 or NULL */, int method, double scale,
                                      double* cov /* n_pairs*36 */, ndt_pose_information* info /* n_pairs or NULL */);
ndt_status ndt_host_pose_covariance(const double* A, const double* B, const double* g, size_t n_found, int method, double scale,
                                    double* cov, double* eig_min, double* eig_max, int* flags);
ndt_status ndt_diag_pose_covariance(ndt_handle h, size_t* launches, size_t* blocks);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ---------------------------
 * The reference is a single process (ndt_omp_impl.hpp:206 is its only parallel construct); this is the exchange step
 * north_star adds.  Registrations of different scans are independent, so ndt_align_batch* on every rank over its own
 * share of the scans needs NO collective (what bench.py measures at N > 1).  Two uses of a communicator remain:
 *  - ndt_align_batch_sharded*: the literal lock-step form -- the batch has total_scans scans, this rank holds scans
 *    [first_scan, first_scan + n_local) (offsets: n_local + 1 entries into ITS points); every rank steps all
 *    total_scans Newton / More-Thuente state machines, rows of the scans a rank does not hold are zero, and ONE in-place
 *    SUM all-reduce of the [total_scans][NDT_EVAL_STRIDE] f64 buffer per lock-step gives every rank every row.
 *    guesses and the per-scan outputs have total_scans entries and come out identical on every rank.
 *  - ndt_align with a communicator set: the source cloud each rank holds is a SHARD of one big scan (target replicated);
 *    the 32-f64 row of every evaluation is all-reduced, so all ranks walk the same registration.
 * PRECONDITION of both: every rank holds the SAME target (same points, same parameters) -- the grid is replicated, not
 * exchanged.  A rank whose target has no voxel at all still joins the exchange of a sharded batch with zero rows; in the
 * point-sharded ndt_align such a rank returns without a collective, which is consistent only when every rank's target
 * is that empty one.  If a peer never joins a collective the waiting rank gives up after NDT_BATCH_TIMEOUT_S (60)
 * seconds, aborts its communicator (ncclCommAbort, so that its stream drains) and returns NDT_ERR_COMM.
 * The collective is issued from C++ on the handle's own stream (no host synchronisation around it); librccl is loaded
 * on first use.  ndt_comm_get_unique_id (rank 0) wraps ncclGetUniqueId; the caller carries the NDT_COMM_ID_BYTES to
 * the other ranks (MPI, a file, torch.distributed ...), then every rank calls ndt_comm_init_rank on its own device. */
#define NDT_COMM_ID_BYTES 128
ndt_status ndt_comm_get_unique_id(void* id_out /* NDT_COMM_ID_BYTES */);
ndt_status ndt_comm_init_rank(ndt_handle h, const void* id, int rank, int world_size);
ndt_status ndt_comm_destroy(ndt_handle h);
/* rank / world size of the handle's communicator (-1 / 0 without one), collectives issued since ndt_comm_init_rank,
 * lock-steps of the last ndt_align_batch* call (any may be NULL) */
ndt_status ndt_comm_stats(ndt_handle h, int* rank, int* world_size, long long* n_collectives, int* lock_steps);
ndt_status ndt_align_batch_sharded(ndt_handle h, const void* pts, const size_t* offsets /* n_local+1 */, size_t n_local,
                                   size_t first_scan, size_t total_scans, size_t stride_bytes,
                                   const float* guesses /* total_scans*16 or NULL */, float* final_transformations /* total_scans*16 */,
                                   int* has_converged, int* final_num_iteration, double* transformation_probability);
ndt_status ndt_align_batch_sharded_device(ndt_handle h, const void* d_pts, const size_t* offsets, size_t n_local,
                                          size_t first_scan, size_t total_scans, size_t stride_bytes, const float* guesses,
                                          float* final_transformations, int* has_converged, int* final_num_iteration,
                                          double* transformation_probability);

/* Caller-supplied exchange step (tests over gloo; any collective library the caller already has):
 * after every fused evaluation the packed [n_rows][NDT_EVAL_STRIDE] f64 result
 * buffer is handed to `fn` for an in-place SUM all-reduce across ranks
 * (the device buffer when `on_device` != 0, a host copy otherwise).  Not stream-ordered: the library synchronises
 * around the call.  A communicator set with ndt_comm_init_rank takes precedence.  fn returns 0 on success. */
#define NDT_EVAL_STRIDE 32 /* score, g[6], H upper-tri[21], n_neighbors, 3 spare */
typedef int (*ndt_allreduce_fn)(void* buf, size_t n_doubles, int on_device, void* user);
ndt_status ndt_set_allreduce(ndt_handle h, ndt_allreduce_fn fn, void* user, int on_device);

/* ---- inspection / test entry points --------------------------------------
 * One computeDerivatives evaluation (ndt_omp_impl.hpp:179-285) at pose p; the
 * source is transformed by T(p) as computeStepLengthMT does (:827-837).
 * H may be NULL (compute_hessian = false). */
ndt_status ndt_eval(ndt_handle h, const double* p, double* score, double* gradient, double* hessian,
                    double* mean_neighbors);
/* Same with an explicit 4x4 (column-major) applied to the source while the
 * angle derivatives come from p -- the initial evaluation of align with a
 * non-identity guess (:95-119). */
ndt_status ndt_eval_with_matrix(ndt_handle h, const float* T, const double* p, double* score, double* gradient,
                                double* hessian, double* mean_neighbors);
/* computeHessian (:540-645): the all-f64 Hessian at pose p. */
ndt_status ndt_eval_hessian_f64(ndt_handle h, const double* p, double* hessian);

/* Target grid (VoxelGridCovariance::leaves_): number of occupied voxels and a
 * dump in ascending linear-index order.  cov/icov are row-major 3x3 f64;
 * nr_points is -1 for rejected voxels as in _impl.hpp:337-341,360-364. */
ndt_status ndt_grid_size(ndt_handle h, size_t* n_leaves, size_t* n_valid);
ndt_status ndt_grid_info(ndt_handle h, int* min_b /*3*/, int* max_b /*3*/, int* div_b /*3*/);
ndt_status ndt_grid_dump(ndt_handle h, int64_t* idx, int* nr_points, double* mean, double* cov, double* icov,
                         double* evals);

/* Live kernel timing with HIP events recorded on the handle's own stream (bench.py's roofline leg).
 * on = 1: ndt_align runs one launch per evaluation and brackets each with an event pair; kind 0 =
 *         derivatives with Hessian, 1 = without, 2 = f64 Hessian.  ndt_align_batch brackets the
 *         derivative kernels of every lock-step with one pair: kind 0, n_launches = lock-steps.
 *         With a communicator set (ndt_align_batch_sharded) every lock-step is split three ways: kind 0 the
 *         derivative kernels, kind 4 k_reduce + ncclAllReduce, kind 5 k_publish_rows (all on the library stream),
 *         and kind 6 the host's wall time for the whole lock-step (descriptors, launches, wait, solver steps), in ms.
 * on = 2: ndt_align keeps its persistent kernel (one launch per registration, the kernel of the
 *         timed region) and brackets that launch with one event pair; kind 3.
 * Off (0) by default: the event records cost host time. */
ndt_status ndt_profile_enable(ndt_handle h, int on);

/* How ndt_align evaluates: 1 (default) = one persistent kernel per registration, fed one command
 * per evaluation through a pinned mailbox; 0 = one kernel launch per evaluation.  Both run the same
 * device code over the same thread partition and return bit-identical results (tests pin that);
 * the setting only trades latency.  The NDT_PERSISTENT environment variable sets the default.
 * Unless this call has insisted on 1, a registration that starts while another ndt_align of this process is
 * in flight on the same device uses the launch path: the persistent kernel holds its CUs for a whole registration, so
 * concurrent callers would otherwise take turns at it; calling this with 1 insists on the persistent kernel. */
ndt_status ndt_set_evaluation_path(ndt_handle h, int persistent);
/* Evaluation reuse (on by default; NDT_EVAL_REUSE=0 turns the default off).  What is reused: the answer to the last request of
 * the same kind, when the next request (kind, matrix T, pose p) equals it byte for byte -- the trials a More-Thuente line
 * search repeats once its step is clamped to transformation_epsilon / 2.  Why it is exact: an evaluation is a function of
 * its request (fixed-order sums, bit-identical from run to run), so the device would return the same bits.
 * ndt_align, ndt_align_batch*, ndt_align_pairs*, ndt_align_guesses and ndt_align_multistart use it; results and ndt_get_stats
 * (the algorithm's counts, reused steps included) do not change.  Never used under ndt_profile_enable(h, 1), with a
 * communicator or an all-reduce hook, nor by ndt_host_run_driver: there the number of evaluations is itself observed.
 * ndt_diag_eval_reuse: of the last align / batch call, *served evaluations the device answered (summed over members) and
 * *reused steps the solvers fed themselves; served + reused = n_evals + n_hessian_recomputes of ndt_get_stats. */
ndt_status ndt_set_evaluation_reuse(ndt_handle h, int on);
ndt_status ndt_diag_eval_reuse(ndt_handle h, long long* served, long long* reused);
/* Diagnostic: the evaluation of `kind` (0 with Hessian, 1 without, 2 f64 Hessian) at pose p, asked n_times of one running
 * evaluation server; rows receives n_times x 43 doubles (score, g[6], H[36] row-major; H is zero for kind 1).  What evaluation
 * reuse rests on can be read from it: the rows are equal bit for bit (ndt_eval is the launch path's counterpart). */
ndt_status ndt_diag_eval_server(ndt_handle h, const double* p, int kind, int n_times, double* rows);
ndt_status ndt_profile_read(ndt_handle h, int kind, long long* n_launches, double* total_ms, int reset);

/* Device self-test of the wave64 fold reduction used by every kernel epilogue: n_blocks blocks
 * of known per-thread values; block_sums receives n_blocks x NDT_EVAL_STRIDE doubles (slots 0..28). */
ndt_status ndt_selftest_reduce(ndt_handle h, int n_blocks, double* block_sums);
/* liveness of the persistent evaluation server: one evaluation, a host stall of stall_ms (the server's patience is
 * 20 ms), one more request (*served_after_stall = 0 when the server had left, as it must for stall_ms > 20), then the
 * same evaluation through the launch path and through a fresh server; scores[3] = the three results. */
ndt_status ndt_selftest_server_idle(ndt_handle h, const double* p, int stall_ms, int* served_after_stall, double* scores);

/* Diagnostic (development aid): one DIRECT7 evaluation at pose p by the s_memtime-stamped build of
 * the derivative kernel.  stamps receives n_waves x 8 u64 (shader cycles at: entry, point
 * arrived, LUT arrived, first record arrived, neighbour math done, wave fold done, block done);
 * *n_waves in: capacity, out: waves written. */
ndt_status ndt_diag_stamps(ndt_handle h, const double* p, unsigned long long* stamps, size_t* n_waves);

/* Diagnostic: how this handle (its CU count and partition, ndt_get_cu_partition) cuts an evaluation of n source points, form by
 * form: *ppb points per 512-thread block of the one-launch kernel and of the evaluation server, *fused_blocks the one-launch
 * kernel's grid, *launch_blocks the grid of the separate derivative / f64-Hessian kernels (256 points per block and pass),
 * *server_blocks the evaluation server's grid, *batch_blocks the blocks of an n-point member of a lock-step batch or of a
 * pair.  A grid that covers fewer than n points in one pass is walked grid-strided.  The values come from the functions the
 * launchers call; no device work beyond opening the device.  For tests that place a scan on a boundary of a plan. */
ndt_status ndt_diag_eval_plan(ndt_handle h, size_t n, int* ppb, int* fused_blocks, int* launch_blocks, int* server_blocks,
                              int* batch_blocks);

/* The plan of a target-grid build of n_points points over a lattice of n_cells cells (ndt_host_lattice), as build_grid and
 * the launches decide it.  Host only; the values come from the functions the build itself calls (the NDT_K1_* development
 * switches included).  *bucket_form: the grid is within the bucket form's range (a dense voxel index then takes it; beyond, the
 * dense chain of count / scan / scatter / k_finalize builds it); *n_buckets K and *cells_per_bucket C: the cell space dealt
 * to K buckets of C cells (bucket = (cell >> 3) mod K); *pts_per_block and *n_blocks: the blocks of the two point passes
 * (n_blocks is a multiple of eight, trailing blocks may be empty); *one_launch: the cloud is small enough for the one-launch
 * form; *wmax and *lds_cap: cells one pass of the bucket form's finish may span and points it holds in LDS.  With div_b (the
 * lattice's cells per axis; may be NULL, the following are then 0): *lut_cells the padded look-up table's size, and the record
 * compaction's tiles over it: *compact_items table entries per thread (1, 2, 4, 8), *compact_tiles tiles, *compact_prefix
 * whether the separate prefix pass over the tile sums runs.  *filter_buckets: the voxel filter of such a cloud (dense route)
 * runs on the bucket front end, *filter_chunks: blocks of its bitmap prefix pass.  Any output may be NULL. */
ndt_status ndt_host_grid_plan(long long n_cells, long long n_points, const int* div_b /*3 or NULL*/, int* bucket_form, int* n_buckets,
                              int* cells_per_bucket, int* pts_per_block, int* n_blocks, int* one_launch, int* wmax, int* lds_cap,
                              long long* lut_cells, int* compact_items, long long* compact_tiles, int* compact_prefix,
                              int* filter_buckets, int* filter_chunks);
/* Diagnostic: what built the handle's current target grid.  *form: 0 nothing (an empty grid, an accumulated target), 1 the dense
 * chain (count / scan / scatter / k_finalize), 2 the bucket form, 3 the one-launch form of small clouds, 4 the sparse index.
 * The plan the build stored (forms 2 and 3; pts_per_block and n_blocks: form 2) and the finish's *wmax / *lds_cap as in
 * ndt_host_grid_plan (form 3: the one-launch kernel's own cap); *lut_cells and the compaction's tile plan for a grid with a
 * dense table (forms 1 to 3, else 0); *compact_pending: the records still carry the build's numbering and will be compacted
 * before the second registration.  No device work.  Any output may be NULL. */
ndt_status ndt_diag_grid_build(ndt_handle h, int* form, size_t* n_points, long long* n_cells, int* n_buckets, int* cells_per_bucket,
                               int* pts_per_block, int* n_blocks, int* wmax, int* lds_cap, long long* lut_cells, int* compact_items,
                               long long* compact_tiles, int* compact_prefix, int* compact_pending);

/* Diagnostic: round-trip latency of the persistent evaluation server, averaged over n_iter commands:
 * us[0] = no-op round (protocol only), us[1] = derivatives without Hessian, us[2] = with Hessian. */
ndt_status ndt_diag_server_roundtrip(ndt_handle h, const double* p, int n_iter, double* us);
/* Diagnostic: `rounds` evaluations at pose p driven from the DEVICE (the last arriving block adds the part sums and posts the
 * next command itself; no Newton / line-search step): us[0] per round without the per-point body, us[1] with the
 * with-Hessian body -- the floor a device-side solver would start from.  DIRECT7 only. */
ndt_status ndt_diag_selfdrive(ndt_handle h, const double* p, int rounds, double* us);

/* Host-side scalar pieces of the driver (no GPU needed), exported so that the
 * CPU test-suite can check them against the oracle. */
void ndt_host_solve6(const double* H /*36 row-major*/, const double* b /*6*/, double* x /*6*/); /* JacobiSVD.solve, :127-129 */
void ndt_host_pose_to_matrix(const double* p /*6*/, float* T /*16 col-major*/);                  /* :146-149, 827-830 */
void ndt_host_matrix_to_pose(const float* T /*16 col-major*/, double* p /*6*/);                  /* :103-111 */
void ndt_host_angle_derivatives(const double* p /*6*/, float* j_ang /*8*3*/, float* h_ang /*15*3*/,
                                double* j_ang_d /*8*3*/, double* h_ang_d /*15*3*/);              /* :288-395 */
void ndt_host_gauss(float resolution, double outlier_ratio, double* d /*3: d1,d2,d3*/);          /* :86-93 */
/* Host threads a lock-step batch may use.  ndt_host_thread_budget probes this process: CPUs in its affinity mask, the
 * cgroup's CPU bandwidth in CPUs (cpu.max / cfs_quota; 0 = unlimited) and LOCAL_WORLD_SIZE (ranks sharing the node, 1
 * when unset).  ndt_host_thread_plan is the pure rule applied to such a budget: share = min(affinity, floor(quota)) /
 * local_world_size (at least 1); *pool_threads = clamp(share / 2, 1, 16) workers for the per-step solver work (they
 * block when idle), *max_batch_groups = clamp(share, 1, 8) independent lock-step groups (a host thread each).
 * NDT_HOST_THREADS / NDT_BATCH_GROUPS / ndt_set_batch_groups override. */
void ndt_host_thread_budget(int* affinity_cpus, double* quota_cpus, int* local_world_size);
void ndt_host_thread_plan(int affinity_cpus, double quota_cpus, int local_world_size, int* pool_threads, int* max_batch_groups);
/* Runs the Newton + More-Thuente driver against a caller-supplied evaluator
 * (test hook: lets the CPU suite drive the PRODUCT driver with oracle
 * evaluations).  kind: 0 = derivatives with Hessian, 1 = without, 2 = f64
 * Hessian only.  T is the 4x4 (col-major) to apply to the source. */
typedef int (*ndt_eval_cb)(void* user, int kind, const float* T, const double* p, double* score, double* g, double* H);
ndt_status ndt_host_run_driver(ndt_eval_cb cb, void* user, size_t n_source, const float* guess, float resolution,
                               double step_size, double outlier_ratio, double trans_eps, int max_iter,
                               float* final_transformation, int* has_converged, int* final_num_iteration,
                               double* transformation_probability, int* n_evals, int* n_hessian_recomputes);
/* The same driver with evaluation reuse on (ndt_set_evaluation_reuse): a request byte-equal to the last answered one of its
 * kind is not passed to cb; the driver takes that answer again, which is exact for an evaluator that is a function of its
 * request.  cb is called n_evals + n_hessian_recomputes - *n_reused times; every other output is as ndt_host_run_driver's. */
ndt_status ndt_host_run_driver_reuse(ndt_eval_cb cb, void* user, size_t n_source, const float* guess, float resolution,
                                     double step_size, double outlier_ratio, double trans_eps, int max_iter,
                                     float* final_transformation, int* has_converged, int* final_num_iteration,
                                     double* transformation_probability, int* n_evals, int* n_hessian_recomputes, int* n_reused);

#ifdef __cplusplus
}
#endif
#endif /* NDT_MI355_H_ */
