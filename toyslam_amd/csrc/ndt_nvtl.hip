// ndt_nvtl.hip -- nearest-voxel transformation likelihood (NVTL) against the handle's target: of a cloud used as given
// (ndt_calculate_nvtl), of the handle's source under the last align's final transformation (ndt_get_nvtl), under many poses in
// one launch per chunk (ndt_nvtl_poses), per source point (ndt_source_point_nvtl; ndt_source_point_count sizes its buffer),
// and what the last such call did (ndt_diag_nvtl).  The definition is in include/ndt_mi355.h; the kernels (k_nvtl,
// k_nvtl_poses) are in ndt_kernels.hip.
//   one cloud  : nvtl_launch -- k_nvtl over derivative_blocks(n) blocks (ndt_calculate_score's walk), launch_reduce, one wait;
//                slot 0 = sum of L over the found points, slot 1 = their count
//   many poses : ndt_score_poses' shape -- the pose table of a chunk through page-locked memory, k_nvtl_poses over
//                (blocks, poses of the chunk), one launch_reduce and one wait per chunk; chunks by poses_chunk (ndt_score.hip)
// Nothing of the handle's target, source, grid, last result, statistics or ndt_diag_score_poses counters is touched: the
// scratch is the partial rows and the pinned result rows every evaluation overwrites, and the handle's nv_* members.
#include "ndt_internal.hpp"

namespace ndtc {

static double nvtl_of(const double* row) { return row[1] > 0 ? row[0] / row[1] : 0.0; }  // n_found == 0: 0.0, never NaN

// the readiness every NVTL call shares, after its own argument checks: a device, then a target (and a source)
ndt_status nvtl_ready(ndt_context* h, bool need_source) {
  ndt_status s = ensure_device(h);
  if (s) return s;
  if (!h->grid || !h->target) return fail(NDT_ERR_NO_INPUT, "no input target");
  if (need_source && !h->source) return fail(NDT_ERR_NO_INPUT, "no input source");
  h->nv_launches = 0;
  h->nv_blocks = 0;
  return NDT_OK;
}

// NVTL of the n device points at d_pts, moved by the column-major T first (null: used as given).  d_out (may be null): n
// doubles of device memory that receive L per point, -1.0 where the point has no neighbour.
ndt_status nvtl_launch(ndt_context* h, const float4* d_pts, size_t n, const float* T_colmajor, double* d_out, double* nvtl,
                       size_t* n_found) {
  if (nvtl) *nvtl = 0.0;
  if (n_found) *n_found = 0;
  if (n == 0) return NDT_OK;
  if (h->grid->empty) {  // no voxel, no neighbour: every point unfound, nothing to launch
    if (d_out) {
      const std::vector<double> none(n, -1.0);
      HIP_TRY(hipMemcpyAsync(d_out, none.data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));  // (`none` is pageable and about to go)
    }
    return NDT_OK;
  }
  ndt_status s = ensure_host_rows(h, 1);
  if (s) return s;
  const ndt::Gauss gs = ndt::gauss_constants(h->resolution, h->outlier_ratio);
  const int nblk = ndt::derivative_blocks(static_cast<int>(n), NDT_DIRECT1);  // ndt_calculate_score's grid: the same walk
  float T12[12];
  if (T_colmajor) colmajor_to_T12(T_colmajor, T12);
  HIP_TRY(h->partials.reserve(static_cast<size_t>(nblk) * ndt::kEvalStride));
  HIP_TRY(hipMemsetAsync(h->partials.p, 0, static_cast<size_t>(nblk) * ndt::kEvalStride * sizeof(double), h->stream));
  HIP_TRY(ndt::launch_nvtl(d_pts, static_cast<int>(n), h->grid->view(), T_colmajor ? T12 : nullptr, gs.d1, gs.d2, h->search,
                           kd_radius2(h->resolution), nblk, d_out, h->partials.p, h->stream));
  HIP_TRY(ndt::launch_reduce(h->partials.p, nblk, 1, nullptr, h->host_result, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->nv_launches = 1;
  h->nv_blocks = static_cast<size_t>(nblk);
  if (nvtl) *nvtl = nvtl_of(h->host_result);
  if (n_found) *n_found = static_cast<size_t>(h->host_result[1]);
  return NDT_OK;
}

}  // namespace ndtc

extern "C" {

ndt_status ndt_calculate_nvtl(ndt_handle h, const void* cloud, size_t n, size_t stride, double* nvtl, size_t* n_found) {
  if (!h || !nvtl) return fail(NDT_ERR_INVALID, "bad arguments");
  if (n > 0 && !cloud) return fail(NDT_ERR_INVALID, "null point buffer");
  if (stride < 12 || stride % 4) return fail(NDT_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  if (n > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  ndt_status s = nvtl_ready(h, false);
  if (s) return s;
  std::shared_ptr<DeviceCloud> c;
  s = upload_cloud(h, cloud, n, stride, false, c);
  if (s) return s;
  return nvtl_launch(h, c->pts.p, n, nullptr, nullptr, nvtl, n_found);
}

ndt_status ndt_get_nvtl(ndt_handle h, double* nvtl, size_t* n_found) {
  if (!h || !nvtl) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = nvtl_ready(h, true);
  if (s) return s;
  return nvtl_launch(h, h->source->pts.p, h->source->n, h->final_T, nullptr, nvtl, n_found);
}

ndt_status ndt_source_point_count(ndt_handle h, size_t* n) {
  if (!h || !n) return fail(NDT_ERR_INVALID, "bad arguments");
  *n = h->source ? h->source->n : 0;
  return NDT_OK;
}

ndt_status ndt_source_point_nvtl(ndt_handle h, const float* transform, double* out, const double** d_out, double* nvtl, size_t* n_found) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  ndt_status s = nvtl_ready(h, true);
  if (s) return s;
  const size_t n = h->source->n;
  HIP_TRY(h->nv_points.reserve(n));
  s = nvtl_launch(h, h->source->pts.p, n, transform ? transform : h->final_T, h->nv_points.p, nvtl, n_found);
  if (s) return s;
  if (out && n) HIP_TRY(hipMemcpy(out, h->nv_points.p, n * sizeof(double), hipMemcpyDeviceToHost));  // (the stream has been waited for)
  if (d_out) *d_out = h->nv_points.p;
  return NDT_OK;
}

ndt_status ndt_nvtl_poses(ndt_handle h, const float* transforms, size_t n_poses, double* nvtl, size_t* n_found) {
  ndt_status s = many_poses_checks(h, transforms, n_poses, nvtl, "transforms or nvtl");
  if (s) return s;
  if (n_poses == 0) return NDT_OK;
  s = nvtl_ready(h, true);
  if (s) return s;
  const size_t n = h->source->n;
  if (n == 0 || h->grid->empty) {  // no point or no voxel: nothing is found
    for (size_t g = 0; g < n_poses; g++) {
      nvtl[g] = 0.0;
      if (n_found) n_found[g] = 0;
    }
    return NDT_OK;
  }
  const ndt::Gauss gs = ndt::gauss_constants(h->resolution, h->outlier_ratio);
  const int nblk = ndt::derivative_blocks(static_cast<int>(n), NDT_DIRECT1);  // nvtl_launch's grid: the same walk
  const size_t row_bytes = static_cast<size_t>(nblk) * ndt::kEvalStride * sizeof(double);
  const size_t chunk = poses_chunk(n_poses, row_bytes);
  s = ensure_host_rows(h, chunk);
  if (s) return s;
  s = pinned_at_least(h->nv_pinned, h->nv_pinned_bytes, chunk * 12 * sizeof(float), h->stream);
  if (s) return s;
  HIP_TRY(h->nv_poses.reserve(chunk * 12));
  HIP_TRY(h->partials.reserve(chunk * nblk * ndt::kEvalStride));
  float* T12 = static_cast<float*>(h->nv_pinned);
  for (size_t g0 = 0; g0 < n_poses; g0 += chunk) {
    const size_t m = std::min(chunk, n_poses - g0);
    for (size_t g = 0; g < m; g++) colmajor_to_T12(transforms + 16 * (g0 + g), T12 + 12 * g);
    HIP_TRY(hipMemcpyAsync(h->nv_poses.p, T12, m * 12 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->partials.p, 0, m * row_bytes, h->stream));
    HIP_TRY(ndt::launch_nvtl_poses(h->source->pts.p, static_cast<int>(n), h->grid->view(), h->nv_poses.p, static_cast<int>(m), gs.d1, gs.d2,
                                   h->search, kd_radius2(h->resolution), nblk, h->partials.p, h->stream));
    HIP_TRY(ndt::launch_reduce(h->partials.p, nblk, static_cast<int>(m), nullptr, h->host_result, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // (the pose table and the rows are the next chunk's to overwrite)
    for (size_t g = 0; g < m; g++) {
      const double* row = h->host_result + g * ndt::kEvalStride;
      nvtl[g0 + g] = nvtl_of(row);
      if (n_found) n_found[g0 + g] = static_cast<size_t>(row[1]);
    }
    h->nv_launches++;
    h->nv_blocks += m * static_cast<size_t>(nblk);
  }
  return NDT_OK;
}

ndt_status ndt_diag_nvtl(ndt_handle h, size_t* launches, size_t* blocks) {
  if (!h || !launches || !blocks) return fail(NDT_ERR_INVALID, "bad arguments");
  *launches = h->nv_launches;
  *blocks = h->nv_blocks;
  return NDT_OK;
}

}  // extern "C"
