/* gicp_mi355.h -- C-ABI of the MI355X GICP core (libndt_mi355.so), SURVEY 8(f) row N4.
 *
 * Drop-in boundary for pclomp::GeneralizedIterativeClosestPoint<PointT,PointT>, the second registration
 * class of the reference's libndt_omp (ndt_omp/include/pclomp/gicp_omp.h, gicp_omp_impl.hpp; used by
 * ndt_omp/apps/align.cpp:80-86).  Plain pointers and sizes only; every entry point names the reference
 * member it replaces.  include/pclomp/gicp_omp.h maps the PCL class onto these 1:1.
 *
 * Status codes and the error string are those of ndt_mi355.h (ndt_last_error()).  A handle is
 * thread-compatible: one thread at a time.
 */
#ifndef GICP_MI355_H_
#define GICP_MI355_H_

#include "ndt_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gicp_context* gicp_handle;

/* ctor, gicp_omp.h:106-122: k_correspondences 20, gicp_epsilon 0.001, rotation_epsilon 2e-3,
 * max_inner_iterations 20, max_iterations 200, transformation_epsilon 5e-4, corr_dist_threshold 5 m */
ndt_status gicp_create(int device, gicp_handle* out);
void gicp_destroy(gicp_handle h);

/* setCorrespondenceRandomness (gicp_omp.h:229): 1 <= k <= 64 on this implementation */
ndt_status gicp_set_correspondence_randomness(gicp_handle h, int k);
/* setRotationEpsilon (:213) */
ndt_status gicp_set_rotation_epsilon(gicp_handle h, double eps);
/* setMaximumOptimizerIterations (:241) */
ndt_status gicp_set_maximum_optimizer_iterations(gicp_handle h, int n);
/* pcl::Registration::setTransformationEpsilon / setMaximumIterations / setMaxCorrespondenceDistance */
ndt_status gicp_set_transformation_epsilon(gicp_handle h, double eps);
ndt_status gicp_set_maximum_iterations(gicp_handle h, int n);
ndt_status gicp_set_max_correspondence_distance(gicp_handle h, double d);

/* setInputTarget (gicp_omp.h:156-160) / setInputSource (:128-143): host buffers of n points, xyz as three
 * f32 at the start of each stride_bytes record.  Drops the cloud's covariances, as the reference does.
 * Points must be finite (pcl::KdTreeFLANN requires it of its queries); NDT_ERR_INVALID otherwise. */
ndt_status gicp_set_input_target(gicp_handle h, const void* pts, size_t n, size_t stride_bytes);
ndt_status gicp_set_input_source(gicp_handle h, const void* pts, size_t n, size_t stride_bytes);
/* setSourceCovariances / setTargetCovariances (gicp_omp.h:165-168,186-189): one 3x3 f64 matrix per point of the cloud set
 * before ([n][9] row-major; symmetric, the upper triangle is used) instead of the k-NN covariances computeCovariances
 * (gicp_omp_impl.hpp:48-116) would produce; setting the cloud again resets them, n == 0 / NULL clears them. */
ndt_status gicp_set_source_covariances(gicp_handle h, const double* cov, size_t n);
ndt_status gicp_set_target_covariances(gicp_handle h, const double* cov, size_t n);

/* setInputTarget / setInputSource BY REFERENCE from a cloud resident in HBM (ndt_cloud_upload, ndt_cloud_voxel_filter*,
 * batched filter outputs, sequence views): no download, no host pass over the points.  Same index, covariances,
 * correspondences and registration -- the same bits -- as gicp_set_input_target / _source on the same points.
 * The handle holds a reference of its own (the caller may release the cloud).  A cloud with a non-finite point:
 * NDT_ERR_INVALID (found on the device: one counting pass, one word read back), as is a NULL or empty cloud; the handle then
 * has no such input, as after a refused host call.  Resets the covariances like the host setters. */
ndt_status gicp_set_input_target_cloud(gicp_handle h, ndt_cloud c);
ndt_status gicp_set_input_source_cloud(gicp_handle h, ndt_cloud c);

/* setInputTarget from a VOXEL GRID: the target becomes the current target grid of the NDT handle `map` -- cloud-built in any
 * form (dense, sparse), accumulated (ndt_target_accumulate*), cropped or imported -- and GICP registers against its voxel
 * distributions (voxelised, distribution-to-distribution GICP; scan-to-map GICP when the grid is an accumulated map).
 * Correspondences are found through the grid's own voxel table: no index is built over the map, nothing is rebuilt when it grows.
 *
 * The target set D: the voxels of the grid that the DIRECT neighbour searches see -- a voxel is in D when its table entry is a
 * record; a voxel that reached min_points_per_voxel but was rejected, and a voxel still under min_points_per_voxel, are not.
 * D is ordered by ascending linear voxel index: a subset of the centroid cloud of ndt_grid_centroids, in its order.  A
 * correspondence (gicp_step_correspond's corr) is an ordinal in D.  Voxel v contributes
 *   - as target point its f32 centroid, the bits ndt_grid_centroids returns for it;
 *   - as target covariance a 3x3 f64 matrix, by cov_mode:
 *       GICP_VOXEL_COV_RAW   the inverse of the voxel's f64 inverse covariance (Eigen's cofactor inverse, as everywhere in the
 *                            library): the voxel's (regularised) covariance in m^2;
 *       GICP_VOXEL_COV_PLANE I - (1 - gicp_epsilon) n n^T, n the unit eigenvector of the largest eigenvalue of the inverse
 *                            covariance (the f64 Jacobi routine of the k-NN covariances): GICP's (1, 1, epsilon) regularisation
 *                            along the voxel's normal, the scale of the source's k-NN covariances.  Recommended.
 * The GICP handle BORROWS `map`: the caller keeps it alive while it is bound and uses both handles from one thread at a time;
 * both must be on the same device.  Every call that needs the target -- gicp_align, gicp_get_fitness_score,
 * gicp_step_correspond, gicp_step_functor, gicp_covariances(which = 0), gicp_target_grid_voxels -- reads map's grid as it is
 * THEN, ordered behind the work queued on map's stream by an event (the device is not synchronised).  D's arrays are made in one
 * mark / scan / gather pass and cached; the pass runs again when the grid has changed (an update, a crop, an import, a reset)
 * or map holds another grid (ndt_set_input_target*).  After such a change gicp_step_functor wants a new gicp_step_correspond.
 * gicp_set_input_target* and gicp_set_input_target_grid(h, NULL, ..) drop the binding.  Everything `map` holds is left as it
 * is (the grid's cached centroid excursion, which ndt_get_centroid_fitness_score shares, may be computed here).
 * NDT_ERR_INVALID before any device work: NULL h, an unknown cov_mode, handles on different devices.  On a grid target also:
 * gicp_set_target_covariances; gicp_covariances(which = 0) with neighbour lists; gicp_align_guesses (the batch forms take cloud
 * targets).  NDT_ERR_NO_INPUT at use: map has no target, or D is empty. */
enum { GICP_VOXEL_COV_PLANE = 0, GICP_VOXEL_COV_RAW = 1 };
ndt_status gicp_set_input_target_grid(gicp_handle h, ndt_handle map, int cov_mode);
/* D as the next registration would use it: *n voxels; xyz1 [n][4] f32 (x, y, z, 1), cov9 [n][9] row-major f64, idx [n] linear
 * voxel indices (any may be NULL; all NULL: the count alone).  capacity < *n: NDT_ERR_INVALID, *n written, no array is. */
ndt_status gicp_target_grid_voxels(gicp_handle h, float* xyz1, double* cov9, int64_t* idx, size_t capacity, size_t* n);
/* the handle's grid target: the mark / scan / gather passes run so far, the voxels of D, the grid's centroid excursion (m) the
 * search gives way by, and the blocks of the last k_correspond_voxel launch (gicp_diag_plan's second entry) */
ndt_status gicp_diag_target_grid(gicp_handle h, size_t* refreshes, size_t* voxels, float* excursion, size_t* correspond_blocks);

/* GICP of n_pairs (target, source) pairs of resident clouds: pairs[2k] = target, pairs[2k+1] = source of pair k.
 * Every cloud NAMED by a pair is indexed once and gets its k-NN covariances once, whatever the number of pairs that
 * name it and in whichever role -- the covariances of ALL named clouds from one launch (k_knn_covariances_multi; a further
 * launch per 2^20 blocks = 8.4 M points) -- then the pairs are registered one after the other by the existing outer loop
 * (k_correspond, the objective server, host BFGS).
 * Pair k gets what a fresh gicp_handle with the same parameters gets from gicp_set_input_target(points of the target),
 * gicp_set_input_source(points of the source), gicp_align(guess k) and gicp_get_fitness_score(max_range): the same
 * bits, whatever the other pairs, their order and the order of the clouds.  Parameters (k, epsilons, iteration limits,
 * gate) are the handle's.  Caller-supplied covariances (gicp_set_*_covariances) are not used by this call.
 * guesses: n_pairs*16 column-major or NULL = identity.  Outputs have n_pairs entries, any may be NULL; fitness NULL =
 * not computed.  The handle's own target, source, covariances, last result and stats are left as they were (only the
 * scratch of gicp_step_correspond is reused: gicp_step_functor wants a new step afterwards).
 * The handle keeps a reference to every named cloud, with its index and covariances, until the next pairs call or
 * gicp_destroy (gicp_pairs_covariances reads them).
 * NDT_ERR_INVALID before any device work, nothing written: NULL handle; NULL clouds / pairs with a non-zero count; a
 * NULL entry of clouds; a pair index < 0 or >= n_clouds; more than 65535 pairs; a NAMED cloud with fewer points than
 * k_correspondences (the message names the cloud; an unnamed one may be any size, empty included).
 * NDT_ERR_INVALID after the device's finite check (one launch over all named clouds, one count per cloud read back): a
 * named cloud with a non-finite point.  On any error no output is written and nothing is kept.  n_pairs == 0: NDT_OK, no
 * device needed. */
ndt_status gicp_align_pairs_clouds(gicp_handle h, const ndt_cloud* clouds, size_t n_clouds, const int* pairs, size_t n_pairs,
                                   const float* guesses, double max_range, float* final_T, int* converged,
                                   int* n_iterations, int* correspondences, double* fitness);

/* inspection of the last successful pairs call (dropped by the next one or gicp_destroy; NDT_ERR_NO_INPUT otherwise
 * or when `cloud` was not named): the covariances it computed for cloud `cloud`, [n][9] row-major as gicp_covariances */
ndt_status gicp_pairs_covariances(gicp_handle h, size_t cloud, double* cov);
/* index builds (== named clouds), k_knn_covariances_multi launches, and the blocks of those launches together */
ndt_status gicp_diag_pairs(gicp_handle h, size_t* index_builds, size_t* knn_launches, size_t* knn_blocks);
/* host wall clock of the last successful pairs call's two halves, in ms: the preparation (finite check, index builds, the
 * covariance launch, waited for) and the registrations with their fitness scores (tools/time_gicp_pairs.py) */
ndt_status gicp_diag_pairs_time(gicp_handle h, double* prepare_ms, double* register_ms);

/* gicp_align_pairs_clouds with the registrations ADVANCED TOGETHER instead of one after the other: the same arguments, the
 * same checks and messages, the same preparation (one function serves both calls), the same records for
 * gicp_pairs_covariances / gicp_diag_pairs / gicp_diag_pairs_time, the same "nothing written on error" -- and for pair k
 * the same bits, whatever the other pairs, their order and the window.  Every pair in flight runs the existing outer
 * loop and BFGS on a host thread of its own; a step is one k_correspond_multi launch for the members that need new
 * correspondences and one k_functor_multi launch that evaluates every waiting member's objective at its own pose in its
 * own mode (no persistent kernel, no waiting on the device).  At most 32 pairs are in flight (NDT_GICP_LOCKSTEP_MEMBERS:
 * 1 ... 256); when one ends the next pair starts at the following step.  A list that repeats (target, source) with
 * different guesses is a multi-start: the clouds are prepared once.  The handle's own inputs, covariances, result,
 * statistics and step scratch are left as they were. */
ndt_status gicp_align_pairs_lockstep(gicp_handle h, const ndt_cloud* clouds, size_t n_clouds, const int* pairs, size_t n_pairs,
                                     const float* guesses, double max_range, float* final_T, int* converged,
                                     int* n_iterations, int* correspondences, double* fitness);
/* The handle's own source registered onto its own target from each of n_guesses guesses (n*16 column-major), all of them
 * members of one lock-step.  The covariances are computed once -- the handle's k-NN ones, or the ones the caller set.
 * Output g (n_guesses entries each, any may be NULL; fitness NULL = not computed) has the bits of gicp_align(guess g)
 * followed by gicp_get_stats / gicp_get_fitness_score(max_range) on this handle.  gicp_get_result, gicp_get_stats and the
 * handle's covariances are left as they were.  n_guesses == 0: NDT_OK, no device and no inputs needed.  Otherwise
 * NDT_ERR_NO_INPUT without both inputs; NDT_ERR_INVALID: more than 65535 guesses, NULL guesses.  Nothing written on error. */
ndt_status gicp_align_guesses(gicp_handle h, const float* guesses /* n*16 */, size_t n_guesses, double max_range,
                              float* final_T, int* converged, int* n_iterations, int* correspondences, double* fitness);
/* the last successful lock-step call of either kind (NDT_ERR_NO_INPUT otherwise): its steps, the steps with a
 * k_correspond_multi launch, its k_functor_multi launches (one per step), and the most members one step carried */
ndt_status gicp_diag_lockstep(gicp_handle h, size_t* steps, size_t* correspond_launches, size_t* functor_launches,
                              size_t* max_members_in_step);

/* pcl::Registration::align(output, guess) -> computeTransformation (gicp_omp_impl.hpp:372-517).
 * guess / final_T: column-major 4x4 f32 (Eigen::Matrix4f::data()), guess may be NULL (identity).
 * out_cloud: NULL or n_source records of stride 16 bytes (x, y, z, 1). */
ndt_status gicp_align(gicp_handle h, const float* guess, float* final_T, int* converged, int* n_iterations, void* out_cloud);

/* hasConverged / getFinalTransformation state of the last align */
ndt_status gicp_get_result(gicp_handle h, float* final_T, int* converged, int* n_iterations);
/* pcl::Registration::getFitnessScore(max_range) after align */
ndt_status gicp_get_fitness_score(gicp_handle h, double max_range, double* fitness);
/* functor calls of the last align (operator(), df, fdf) and its last correspondence count */
ndt_status gicp_get_stats(gicp_handle h, int* n_f, int* n_df, int* n_fdf, int* correspondences);

/* --- inspection entry points (parity tests) ---------------------------------------------- */
/* computeCovariances (gicp_omp_impl.hpp:48-116) of the target (which = 0) or the source (1):
 * cov [n][9] row-major f64; nn_idx / nn_d2 optional [n][k] (ascending distance, then index). */
ndt_status gicp_covariances(gicp_handle h, int which, double* cov, int* nn_idx, float* nn_d2);
/* One correspondence step (:405-456) for `transformation` (column-major, NULL = identity) on the source
 * moved by `guess`: corr[i] = target index or -1, maha [n_source][9] row-major f32. */
ndt_status gicp_step_correspond(gicp_handle h, const float* guess, const float* transformation, int* corr, float* maha,
                                int* n_correspondences);
/* OptimizationFunctorWithIndices (:241-368) at x over the correspondences of the last step:
 * mode 0 operator() -> *f; 1 df -> g[6]; 2 fdf -> *f, g[6]. */
ndt_status gicp_step_functor(gicp_handle h, int mode, const double* x, double* f, double* g);
/* How the launchers cut n points into blocks: out = grids of the kNN / covariance pass (n = points of the cloud), the
 * correspondence step, the functor kernel and the objective server (n = source points) -- the very values the launches
 * use, NDT_GICP_MAX_BLOCKS included. */
ndt_status gicp_diag_plan(gicp_handle h, size_t n, int out[4]);
/* applyState on the identity (:519-532): column-major 4x4 */
void gicp_host_apply_state(const double* x, float* T);

#ifdef __cplusplus
}
#endif
#endif /* GICP_MI355_H_ */
