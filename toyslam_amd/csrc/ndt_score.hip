// ndt_score.hip -- calculateScore: of a cloud against the handle's target (ndt_calculate_score), of the handle's source under
// many poses in one launch per chunk (ndt_score_poses) and what the last such call did (ndt_diag_score_poses).
#include "ndt_internal.hpp"

extern "C" {

ndt_status ndt_calculate_score(ndt_handle h, const void* cloud, size_t n, size_t stride, double* score) {
  if (!h || !score) return fail(NDT_ERR_INVALID, "bad arguments");
  if (!h->grid || !h->target) return fail(NDT_ERR_NO_INPUT, "no input target");
  std::shared_ptr<DeviceCloud> c;
  ndt_status s = upload_cloud(h, cloud, n, stride, false, c);
  if (s) return s;
  if (n == 0 || h->grid->empty) {
    *score = n ? 0.0 : std::numeric_limits<double>::quiet_NaN();  // 0/0 in the reference
    return NDT_OK;
  }
  s = ensure_host_rows(h, 1);
  if (s) return s;
  const ndt::Gauss gs = ndt::gauss_constants(h->resolution, h->outlier_ratio);
  const int nblk = ndt::derivative_blocks(static_cast<int>(n), NDT_DIRECT1);
  HIP_TRY(h->partials.reserve(static_cast<size_t>(nblk) * ndt::kEvalStride));
  HIP_TRY(hipMemsetAsync(h->partials.p, 0, static_cast<size_t>(nblk) * ndt::kEvalStride * sizeof(double), h->stream));
  HIP_TRY(ndt::launch_calc_score(c->pts.p, static_cast<int>(n), h->grid->view(), gs.d1, gs.d2, gs.d3, h->search, kd_radius2(h->resolution), nblk,
                                 h->partials.p, h->stream));
  HIP_TRY(ndt::launch_reduce(h->partials.p, nblk, 1, nullptr, h->host_result, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *score = h->host_result[0] / static_cast<double>(n);
  return NDT_OK;
}

}  // extern "C"

// poses per launch (grid.y) of a call with n_poses, a pose's partial rows taking row_bytes: NDT_SCORE_POSES_CHUNK (read once,
// 1 .. 65535, default 4096), fewer while a chunk's rows would pass 256 MiB (4096 poses x 1024 blocks would be 1 GiB)
size_t ndtc::poses_chunk(size_t n_poses, size_t row_bytes) {
  static const size_t v = [] {
    const char* e = getenv("NDT_SCORE_POSES_CHUNK");
    return static_cast<size_t>(std::max(1, std::min(65535, e ? atoi(e) : 4096)));
  }();
  return std::min(n_poses, std::max<size_t>(1, std::min(v, (size_t(256) << 20) / row_bytes)));
}

extern "C" {

ndt_status ndt_score_poses(ndt_handle h, const float* transforms, size_t n_poses, double* scores) {
  ndt_status s = many_poses_checks(h, transforms, n_poses, scores, "transforms or scores");
  if (s) return s;
  if (n_poses == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  if (!h->grid || !h->target) return fail(NDT_ERR_NO_INPUT, "no input target");
  if (!h->source) return fail(NDT_ERR_NO_INPUT, "no input source");
  h->sp_launches = 0;
  h->sp_blocks = 0;
  const size_t n = h->source->n;
  if (n == 0 || h->grid->empty) {  // ndt_calculate_score's edges: 0 / 0 in the reference; no voxel, no term
    for (size_t g = 0; g < n_poses; g++) scores[g] = n ? 0.0 : std::numeric_limits<double>::quiet_NaN();
    return NDT_OK;
  }
  const ndt::Gauss gs = ndt::gauss_constants(h->resolution, h->outlier_ratio);
  const int nblk = ndt::derivative_blocks(static_cast<int>(n), NDT_DIRECT1);  // ndt_calculate_score's grid: the same walk
  const size_t row_bytes = static_cast<size_t>(nblk) * ndt::kEvalStride * sizeof(double);
  const size_t chunk = poses_chunk(n_poses, row_bytes);
  s = ensure_host_rows(h, chunk);
  if (s) return s;
  s = pinned_at_least(h->sp_pinned, h->sp_pinned_bytes, chunk * 12 * sizeof(float), h->stream);
  if (s) return s;
  HIP_TRY(h->sp_poses.reserve(chunk * 12));
  HIP_TRY(h->partials.reserve(chunk * nblk * ndt::kEvalStride));
  float* T12 = static_cast<float*>(h->sp_pinned);
  for (size_t g0 = 0; g0 < n_poses; g0 += chunk) {
    const size_t m = std::min(chunk, n_poses - g0);
    for (size_t g = 0; g < m; g++) colmajor_to_T12(transforms + 16 * (g0 + g), T12 + 12 * g);
    HIP_TRY(hipMemcpyAsync(h->sp_poses.p, T12, m * 12 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->partials.p, 0, m * row_bytes, h->stream));
    HIP_TRY(ndt::launch_score_poses(h->source->pts.p, static_cast<int>(n), h->grid->view(), h->sp_poses.p, static_cast<int>(m), gs.d1, gs.d2,
                                    gs.d3, h->search, kd_radius2(h->resolution), nblk, h->partials.p, h->stream));
    HIP_TRY(ndt::launch_reduce(h->partials.p, nblk, static_cast<int>(m), nullptr, h->host_result, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // (the pose table and the rows are the next chunk's to overwrite)
    for (size_t g = 0; g < m; g++) scores[g0 + g] = h->host_result[g * ndt::kEvalStride] / static_cast<double>(n);
    h->sp_launches++;
    h->sp_blocks += m * static_cast<size_t>(nblk);
  }
  return NDT_OK;
}

ndt_status ndt_diag_score_poses(ndt_handle h, size_t* launches, size_t* blocks) {
  if (!h || !launches || !blocks) return fail(NDT_ERR_INVALID, "bad arguments");
  *launches = h->sp_launches;
  *blocks = h->sp_blocks;
  return NDT_OK;
}

}  // extern "C"
