// gicp_capi.hip -- C-ABI glue of the GICP row (include/gicp_mi355.h): the handle's lifetime, its parameters, the last
// result and statistics, the block plan, and the development switches every GICP unit reads (gicp_internal.hpp lists the units).
#include "gicp_internal.hpp"

namespace ndtc {
// what the index leaf size aims for (points per occupied cell; NDT_GICP_PPC overrides it for tuning runs): with the
// margin bound most queries finish inside their own cell, so fuller cells cost little and far queries need fewer shells
const double kGicpPointsPerCell = std::getenv("NDT_GICP_PPC") ? std::atof(std::getenv("NDT_GICP_PPC")) : 12.0;
// development switch: caps the grids of all four GICP kernels (0 = each kernel's own limit), so that their grid-strided
// regime is reached at a few thousand points -- as NDT_K2_MAX_BLOCKS does for the NDT kernels
const int kGicpMaxBlocks = std::getenv("NDT_GICP_MAX_BLOCKS") ? std::max(0, std::atoi(std::getenv("NDT_GICP_MAX_BLOCKS"))) : 0;
// development switch: the blocks one k_knn_covariances_multi launch carries (default gicp::kKnnMultiMaxBlocks), so that the
// split of a pairs call's covariance pass into several launches is reached with a few thousand points
const int kGicpMultiMaxBlocks = std::getenv("NDT_GICP_MULTI_MAX_BLOCKS") ? std::max(1, std::atoi(std::getenv("NDT_GICP_MULTI_MAX_BLOCKS")))
                                                                         : gicp::kKnnMultiMaxBlocks;
}  // namespace ndtc

// a parameter setter: the handle's null check and the assignment
template <class T>
static ndt_status gicp_set_param(gicp_context* h, T gicp::Params::*field, T value) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  h->prm.*field = value;
  return NDT_OK;
}

extern "C" {
ndt_status gicp_create(int device, gicp_handle* out) {
  if (!out || device < 0) return fail(NDT_ERR_INVALID, "bad arguments");
  gicp_context* h = new gicp_context();
  h->tgt.device = device;
  h->src.device = device;
  *out = h;
  return NDT_OK;
}

void gicp_destroy(gicp_handle h) { delete h; }

ndt_status gicp_set_correspondence_randomness(gicp_handle h, int k) {
  if (!h || k < 1 || k > gicp::kMaxK) return fail(NDT_ERR_INVALID, "k_correspondences must be in [1, 64]");
  // (covariances already computed stay, as in the reference: computeTransformation only computes them while they are
  // empty, gicp_omp_impl.hpp:386-397, and only setInputSource / setInputTarget reset them)
  h->prm.k_correspondences = k;
  return NDT_OK;
}
ndt_status gicp_set_rotation_epsilon(gicp_handle h, double eps) { return gicp_set_param(h, &gicp::Params::rotation_epsilon, eps); }
ndt_status gicp_set_maximum_optimizer_iterations(gicp_handle h, int n) { return gicp_set_param(h, &gicp::Params::max_inner_iterations, n); }
ndt_status gicp_set_transformation_epsilon(gicp_handle h, double eps) { return gicp_set_param(h, &gicp::Params::transformation_epsilon, eps); }
ndt_status gicp_set_maximum_iterations(gicp_handle h, int n) { return gicp_set_param(h, &gicp::Params::max_iterations, n); }
ndt_status gicp_set_max_correspondence_distance(gicp_handle h, double d) { return gicp_set_param(h, &gicp::Params::corr_dist_threshold, d); }

ndt_status gicp_get_result(gicp_handle h, float* final_T, int* converged, int* n_iterations) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  if (final_T) std::memcpy(final_T, h->final_T, sizeof(h->final_T));
  if (converged) *converged = h->result.converged ? 1 : 0;
  if (n_iterations) *n_iterations = h->result.nr_iterations;
  return NDT_OK;
}

ndt_status gicp_get_stats(gicp_handle h, int* n_f, int* n_df, int* n_fdf, int* correspondences) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  if (n_f) *n_f = h->result.n_f;
  if (n_df) *n_df = h->result.n_df;
  if (n_fdf) *n_fdf = h->result.n_fdf;
  if (correspondences) *correspondences = h->result.correspondences;
  return NDT_OK;
}

ndt_status gicp_diag_plan(gicp_handle h, size_t n, int out[4]) {
  if (!h || !out || n > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "bad arguments");
  const int ni = static_cast<int>(n);
  out[0] = gicp::knn_blocks(ni, kGicpMaxBlocks);
  out[1] = gicp::correspond_blocks(ni, kGicpMaxBlocks);
  out[2] = gicp::functor_blocks(ni, kGicpMaxBlocks);
  out[3] = gicp::server_blocks(ni, kGicpMaxBlocks);
  return NDT_OK;
}

void gicp_host_apply_state(const double* x, float* T) {
  float rm[16];
  gicp::apply_state(x, rm);
  colmajor_from_rowmajor(rm, T);
}
}  // extern "C"
