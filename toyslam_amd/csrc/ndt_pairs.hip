// ndt_pairs.hip -- C-ABI: lock-step registration of (target, source) pairs of clouds, every pair against the voxel grid of
// its own target (ndt_align_pairs*, the scan-to-previous-scan shape of ndt_omp_node / ndt_omp_mapping_node), and the
// inspection of the grids such a call built.
//   inputs : every cloud on the device (an upload per cloud, or the caller's ndt_clouds); the clouds named as sources
//            concatenated and ordered exactly as ndt_align_batch orders its scans (order_cloud, one lattice per cloud)
//   grids  : every cloud named as a target gridded once (build_grids): all the small ones (k1_small's range) from ONE
//            k1_small_multi launch, the others through build_grid, the path ndt_set_input_target takes -- either way the
//            grid a handle of its own would hold -- kept in h->pairs_grids until the next pairs call
//   loop   : ndt_batch.hip's lock_step / run_groups with a per-member GridView table (k_pairs_step,
//            ndt_pairs_kernels.hip); a pair whose target has no voxel gets zero rows, as a single registration does
//   kept   : every pair's source (the caller's point order), its target's grid and its final transformation, until the next
//            pairs call: ndt_pairs_fitness_scores (ndt_fitness.hip) scores the pairs from them
// The handle's own target, source, grid and last result are not touched.
#include "ndt_internal.hpp"

namespace ndtc {

static ndt_status pairs_checks(ndt_handle h, size_t n_clouds, const int* pairs, size_t n_pairs) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (n_pairs && !pairs) return fail(NDT_ERR_INVALID, "null pairs");
  if (n_pairs > 65535) return fail(NDT_ERR_INVALID, "at most 65535 pairs per call");
  for (size_t k = 0; k < 2 * n_pairs; k++)
    if (pairs[k] < 0 || static_cast<size_t>(pairs[k]) >= n_clouds) return fail(NDT_ERR_INVALID, "pair names a cloud that does not exist");
  if (h->comm || h->allreduce) return fail(NDT_ERR_INVALID, "pairs are not sharded: the handle has a communicator or an all-reduce hook");
  return NDT_OK;
}

// Grids of the targets, then the lock-step over the pairs.  `clouds`: every cloud on the device (bounding boxes known).
static ndt_status align_pairs_impl(ndt_handle h, const std::vector<std::shared_ptr<DeviceCloud>>& clouds, int is_dense,
                                   const int* pairs, size_t n_pairs, const float* guesses, float* final_T, int* conv, int* iters,
                                   double* tprob) {
  const size_t n_clouds = clouds.size();
  // ---- one grid per target cloud: the small ones from one launch, the others one by one (build_grids)
  std::vector<std::shared_ptr<DeviceGrid>> grids(n_clouds);
  {
    std::vector<int> tid;
    std::vector<std::shared_ptr<DeviceCloud>> tc;
    for (size_t k = 0; k < n_pairs; k++) {
      const int t = pairs[2 * k];
      if (std::find(tid.begin(), tid.end(), t) != tid.end()) continue;
      tid.push_back(t);
      tc.push_back(clouds[t]);
    }
    std::vector<std::shared_ptr<DeviceGrid>> built;
    size_t n_small = 0;
    h->pairs_grids.clear();
    ndt_status s = build_grids(h, tc, is_dense, built, &n_small);
    if (s) return s;
    for (size_t j = 0; j < tid.size(); j++) grids[tid[j]] = built[j];
    h->pairs_grids = grids;
  }
  // ---- the clouds named as sources, each once, concatenated in order of first use and ordered as a batch orders its scans
  std::vector<long long> seg_of(n_clouds, -1);
  std::vector<size_t> offsets(1, 0);
  std::vector<int> seg_cloud;
  for (size_t k = 0; k < n_pairs; k++) {
    const int c = pairs[2 * k + 1];
    if (seg_of[c] >= 0) continue;
    seg_of[c] = static_cast<long long>(seg_cloud.size());
    seg_cloud.push_back(c);
    offsets.push_back(offsets.back() + clouds[c]->n);
  }
  const size_t n_seg = seg_cloud.size();
  auto src = std::make_shared<DeviceCloud>();
  src->n = offsets.back();
  if (src->n > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many source points");
  HIP_TRY(src->pts.reserve(src->n));
  for (size_t j = 0; j < n_seg; j++) {
    const DeviceCloud& c = *clouds[seg_cloud[j]];
    if (c.n) HIP_TRY(hipMemcpyAsync(src->pts.p + offsets[j], c.pts.p, c.n * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
  }
  ndt_status s = order_cloud(h, src.get(), offsets.data(), n_seg);
  if (s) return s;
  const bool use_sorted = src->n_sorted > 0 && !src->scan_counts.empty();
  LockStepMembers m;
  m.pts = use_sorted ? src->sorted.p : src->pts.p;
  m.offset.resize(n_pairs);
  m.count.resize(n_pairs);
  m.n_raw.resize(n_pairs);
  std::vector<ndt::GridView> views(n_pairs);
  std::vector<char> empty(n_pairs);
  for (size_t k = 0; k < n_pairs; k++) {
    const size_t j = static_cast<size_t>(seg_of[pairs[2 * k + 1]]);
    m.n_raw[k] = offsets[j + 1] - offsets[j];
    m.offset[k] = static_cast<int>(use_sorted ? src->scan_starts[j] : offsets[j]);
    m.count[k] = static_cast<int>(use_sorted ? src->scan_counts[j] : m.n_raw[k]);
    const DeviceGrid& g = *grids[pairs[2 * k]];
    empty[k] = g.empty ? 1 : 0;
    views[k] = g.empty ? ndt::GridView{} : g.view();
  }
  m.views = views.data();
  m.empty = empty.data();
  // ---- lock-step: one loop, or independent groups on worker handles (ndt_set_batch_groups / NDT_BATCH_GROUPS, as a batch)
  // (the final transformations land in a buffer of our own as well: ndt_pairs_fitness_scores wants them, the caller may not)
  std::vector<float> T_all(16 * n_pairs);
  const size_t groups = batch_group_count(h, n_pairs);
  if (groups <= 1 || h->profiling) s = lock_step(h, m, n_pairs, guesses, T_all.data(), conv, iters, tprob);
  else s = run_groups(
      h, n_pairs, groups,
      [&](size_t lo, size_t hi) {
        double n = 0;
        for (size_t k = lo; k < hi; k++) n += static_cast<double>(m.n_raw[k]);
        return n;
      },
      [&](ndt_context* w, size_t lo, size_t hi) {
        LockStepMembers part;
        part.pts = m.pts;
        part.offset.assign(m.offset.begin() + lo, m.offset.begin() + hi);
        part.count.assign(m.count.begin() + lo, m.count.begin() + hi);
        part.n_raw.assign(m.n_raw.begin() + lo, m.n_raw.begin() + hi);
        part.views = m.views + lo;
        part.empty = m.empty + lo;
        return lock_step(w, part, hi - lo, guesses ? guesses + 16 * lo : nullptr, T_all.data() + 16 * lo,
                         conv ? conv + lo : nullptr, iters ? iters + lo : nullptr, tprob ? tprob + lo : nullptr);
      });
  if (s) return s;
  if (final_T) std::memcpy(final_T, T_all.data(), T_all.size() * sizeof(float));
  // what ndt_pairs_fitness_scores needs: each pair's source as the caller gave it, its target's grid, its result
  h->pairs_sources.resize(n_pairs);
  h->pairs_targets.resize(n_pairs);
  for (size_t k = 0; k < n_pairs; k++) {
    h->pairs_sources[k] = clouds[pairs[2 * k + 1]];
    h->pairs_targets[k] = grids[pairs[2 * k]];
  }
  h->pairs_T.swap(T_all);
  return NDT_OK;
}

// the retained state of the last pairs call (ndt_pairs_fitness_scores), dropped when a new call begins
static void pairs_forget(ndt_handle h) {
  if (!h) return;
  h->pairs_sources.clear();
  h->pairs_targets.clear();
  h->pairs_T.clear();
}

// the grid the last pairs call built for cloud c
static ndt_status pairs_grid(ndt_handle h, size_t c, DeviceGrid*& g) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (c >= h->pairs_grids.size() || !h->pairs_grids[c]) return fail(NDT_ERR_NO_INPUT, "the last pairs call built no grid for this cloud");
  g = h->pairs_grids[c].get();
  return NDT_OK;
}

}  // namespace ndtc

extern "C" {

ndt_status ndt_align_pairs(ndt_handle h, const void* pts, const size_t* offsets, size_t n_clouds, size_t stride_bytes,
                           int is_dense, const int* pairs, size_t n_pairs, const float* guesses, float* final_T, int* conv,
                           int* iters, double* tprob) {
  pairs_forget(h);
  ndt_status s = pairs_checks(h, n_clouds, pairs, n_pairs);
  if (s) return s;
  if (n_clouds && !offsets) return fail(NDT_ERR_INVALID, "null offsets");
  for (size_t c = 0; c < n_clouds; c++)
    if (offsets[c + 1] < offsets[c]) return fail(NDT_ERR_INVALID, "offsets must be non-decreasing");
  if (n_clouds && offsets[n_clouds] > offsets[0] && !pts) return fail(NDT_ERR_INVALID, "null point buffer");
  if (stride_bytes < 12 || stride_bytes % 4) return fail(NDT_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  if (n_pairs == 0) {
    h->pairs_grids.clear();
    return NDT_OK;
  }
  s = ensure_device(h);
  if (s) return s;
  // the clouds the pairs name, each uploaded on its own (its bounding boxes are its target grid's); the others are skipped
  std::vector<char> used(n_clouds, 0);
  for (size_t k = 0; k < 2 * n_pairs; k++) used[pairs[k]] = 1;
  std::vector<std::shared_ptr<DeviceCloud>> clouds(n_clouds);
  for (size_t c = 0; c < n_clouds; c++) {
    if (!used[c]) {
      clouds[c] = std::make_shared<DeviceCloud>();
      continue;
    }
    const unsigned char* base = static_cast<const unsigned char*>(pts) + offsets[c] * stride_bytes;
    s = upload_cloud(h, base, offsets[c + 1] - offsets[c], stride_bytes, false, clouds[c]);
    if (s) return s;
  }
  return align_pairs_impl(h, clouds, is_dense, pairs, n_pairs, guesses, final_T, conv, iters, tprob);
}

ndt_status ndt_align_pairs_clouds(ndt_handle h, const ndt_cloud* cl, size_t n_clouds, int is_dense, const int* pairs,
                                  size_t n_pairs, const float* guesses, float* final_T, int* conv, int* iters, double* tprob) {
  pairs_forget(h);
  ndt_status s = pairs_checks(h, n_clouds, pairs, n_pairs);
  if (s) return s;
  if (n_clouds && !cl) return fail(NDT_ERR_INVALID, "null clouds");
  for (size_t c = 0; c < n_clouds; c++)
    if (!cl[c] || !cl[c]->c) return fail(NDT_ERR_INVALID, "null cloud");
  if (n_pairs == 0) {
    h->pairs_grids.clear();
    return NDT_OK;
  }
  s = ensure_device(h);
  if (s) return s;
  std::vector<std::shared_ptr<DeviceCloud>> clouds(n_clouds);
  for (size_t c = 0; c < n_clouds; c++) {
    s = cloud_use_on(h, cl[c]->c.get());
    if (s) return s;
    clouds[c] = cl[c]->c;
  }
  return align_pairs_impl(h, clouds, is_dense, pairs, n_pairs, guesses, final_T, conv, iters, tprob);
}

ndt_status ndt_pairs_grid_size(ndt_handle h, size_t cloud, size_t* n_leaves, size_t* n_valid) {
  DeviceGrid* g = nullptr;
  const ndt_status s = pairs_grid(h, cloud, g);
  return s ? s : grid_size(h, g, n_leaves, n_valid);
}
ndt_status ndt_pairs_grid_info(ndt_handle h, size_t cloud, int* min_b, int* max_b, int* div_b) {
  DeviceGrid* g = nullptr;
  const ndt_status s = pairs_grid(h, cloud, g);
  if (!s) grid_info(g, min_b, max_b, div_b);
  return s;
}
ndt_status ndt_pairs_grid_dump(ndt_handle h, size_t cloud, int64_t* idx, int* nr_points, double* mean, double* cov, double* icov,
                               double* evals) {
  DeviceGrid* g = nullptr;
  const ndt_status s = pairs_grid(h, cloud, g);
  return s ? s : grid_dump(h, g, idx, nr_points, mean, cov, icov, evals);
}

}  // extern "C"
