// ndt_fitness.hip -- C-ABI: getFitnessScore of many members at once (ndt_pairs_fitness_scores: every pair of the last
// ndt_align_pairs* call; ndt_batch_fitness_scores*: many scans against the handle's target).
//   indices : the search index of every target grid involved (ensure_indices: two waits in all, however many grids)
//   kernel  : k_fitness_multi, every member in one launch (members of no work -- no point, no searchable target point --
//             get no block and DBL_MAX); a member's blocks and their rows are those of a single k_fitness launch, its
//             sums k_reduce's over those rows, so each value is fitness_impl's bit for bit
//   memory  : the members are split into launches of at most kFitnessChunkBlocks blocks (NDT_FITNESS_CHUNK_BLOCKS), the
//             partial rows of one launch at a time; the results do not depend on the split
// The handle's own target, source, grid and last result are not touched.
#include "ndt_internal.hpp"

namespace ndtc {

// blocks of one k_fitness_multi launch (x kEvalStride doubles of partial rows: 64 MB); a member is never split, so a launch
// holds at least one whole member (at most 2048 blocks) whatever the bound
static constexpr int kFitnessChunkBlocks = 262144;
static int fitness_chunk_blocks() {
  static const int v = [] {
    const char* e = getenv("NDT_FITNESS_CHUNK_BLOCKS");  // development switch: small values force many launches
    const int x = e ? atoi(e) : 0;
    return x > 0 ? std::min(x, kFitnessChunkBlocks) : kFitnessChunkBlocks;
  }();
  return v;
}

// [PCL] Registration::getFitnessScore of the dense device cloud d_src moved by T against the target of the grid g (on h's
// stream, with h's scratch)
ndt_status fitness_against(ndt_context* h, DeviceGrid* g, const float4* d_src, int n, const float* T_colmajor, double max_range,
                           double* fitness) {
  if (g->accumulated) return fail(NDT_ERR_NO_INPUT, "getFitnessScore needs the target's points: an accumulated target keeps none");
  *fitness = std::numeric_limits<double>::max();  // nr == 0 in the reference
  ndt_status s = grid_counts(h, g);
  if (s) return s;
  if (n == 0 || g->empty || g->n_sorted == 0) return NDT_OK;
  s = ensure_cell2leaf(h, g);
  if (s) return s;
  s = ensure_host_rows(h, 1);
  if (s) return s;
  float T12[12];
  colmajor_to_T12(T_colmajor, T12);
  const int nblk = fitness_blocks(n);
  HIP_TRY(h->partials.reserve(static_cast<size_t>(nblk) * ndt::kEvalStride));
  ndt::PointIndex ix;
  fill_point_index(g, ix);
  HIP_TRY(ndt::launch_fitness(d_src, n, T12, ix, max_range, nblk, h->partials.p, h->stream));
  HIP_TRY(ndt::launch_reduce(h->partials.p, nblk, 1, nullptr, h->host_result, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->host_result[1] > 0) *fitness = h->host_result[0] / h->host_result[1];
  return NDT_OK;
}
// ... against h's own target
ndt_status fitness_impl(ndt_context* h, const float4* d_src, int n, const float* T_colmajor, double max_range, double* fitness) {
  return fitness_against(h, h->grid.get(), d_src, n, T_colmajor, max_range, fitness);
}

ndt_status fitness_many(ndt_context* h, const std::vector<FitnessJob>& jobs, double max_range, double* out) {
  for (size_t k = 0; k < jobs.size(); k++) out[k] = std::numeric_limits<double>::max();  // nr == 0 in the reference
  h->fit_launches = 0;
  h->fit_max_blocks = 0;
  std::vector<DeviceGrid*> grids;
  for (const FitnessJob& j : jobs)
    if (j.n && j.g) grids.push_back(const_cast<DeviceGrid*>(j.g));
  ndt_status s = ensure_indices(h, grids);
  if (s) return s;
  // the members with work, and the launches (chunks) they fall into
  std::vector<ndt::FitnessMember> mem;
  std::vector<size_t> of;  // member -> job
  std::vector<int> starts;  // per chunk: its members' first blocks relative to the chunk, and its block count
  std::vector<size_t> chunk_m0(1, 0), chunk_s0(1, 0);
  std::vector<int> chunk_blocks;
  int cur = 0, max_blocks = 0;
  const int bound = fitness_chunk_blocks();
  for (size_t k = 0; k < jobs.size(); k++) {
    const FitnessJob& j = jobs[k];
    if (j.n == 0 || !j.g || j.g->empty || j.g->n_sorted == 0) continue;
    const int n = static_cast<int>(j.n);
    const int nblk = fitness_blocks(n);  // fitness_impl's grid
    if (cur > 0 && cur + nblk > bound) {  // close the chunk
      starts.push_back(cur);
      chunk_blocks.push_back(cur);
      max_blocks = std::max(max_blocks, cur);
      chunk_m0.push_back(mem.size());
      chunk_s0.push_back(starts.size());
      cur = 0;
    }
    ndt::FitnessMember m;
    fill_point_index(j.g, m.ix);
    m.src = j.src;
    m.n = n;
    colmajor_to_T12(j.T, m.T);
    mem.push_back(m);
    of.push_back(k);
    starts.push_back(cur);
    cur += nblk;
  }
  if (mem.empty()) return NDT_OK;
  starts.push_back(cur);
  chunk_blocks.push_back(cur);
  max_blocks = std::max(max_blocks, cur);
  const size_t n_mem = mem.size();
  s = ensure_host_rows(h, (2 * n_mem + ndt::kEvalStride - 1) / ndt::kEvalStride);
  if (s) return s;
  DevBuf<ndt::FitnessMember> d_mem;
  DevBuf<int> d_starts;
  HIP_TRY(d_mem.reserve(n_mem));
  HIP_TRY(d_starts.reserve(starts.size()));
  HIP_TRY(hipMemcpyAsync(d_mem.p, mem.data(), n_mem * sizeof(ndt::FitnessMember), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(d_starts.p, starts.data(), starts.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h->partials.reserve(static_cast<size_t>(max_blocks) * ndt::kEvalStride));
  h->fit_launches = chunk_blocks.size();
  h->fit_max_blocks = static_cast<size_t>(max_blocks);
  for (size_t c = 0; c < chunk_blocks.size(); c++) {  // (the launches reuse the partial rows in stream order)
    const size_t m0 = chunk_m0[c], m1 = c + 1 < chunk_m0.size() ? chunk_m0[c + 1] : n_mem;
    HIP_TRY(ndt::launch_fitness_multi(d_mem.p + m0, d_starts.p + chunk_s0[c], static_cast<int>(m1 - m0), chunk_blocks[c], max_range,
                                      h->partials.p, h->host_result + 2 * m0, h->stream));
  }
  HIP_TRY(hipStreamSynchronize(h->stream));  // (also: `mem` and `starts` are pageable, the copies have read them)
  for (size_t i = 0; i < n_mem; i++)
    if (h->host_result[2 * i + 1] > 0) out[of[i]] = h->host_result[2 * i] / h->host_result[2 * i + 1];
  return NDT_OK;
}

static ndt_status batch_fitness_impl(ndt_handle h, const void* pts, const size_t* offsets, size_t n_scans, size_t stride,
                                     bool on_device, const float* transforms, double max_range, double* fitness) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!offsets) return fail(NDT_ERR_INVALID, "null offsets");
  if (n_scans && !fitness) return fail(NDT_ERR_INVALID, "null fitness");
  if (n_scans && !transforms) return fail(NDT_ERR_INVALID, "null transforms");
  if (n_scans > 65535) return fail(NDT_ERR_INVALID, "at most 65535 scans per call");
  for (size_t k = 0; k < n_scans; k++)
    if (offsets[k + 1] < offsets[k]) return fail(NDT_ERR_INVALID, "offsets must be non-decreasing");
  if (stride < 12 || stride % 4) return fail(NDT_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  const size_t n_pts = offsets[n_scans] - offsets[0];
  if (n_pts && !pts) return fail(NDT_ERR_INVALID, "null point buffer");
  if (!h->grid || !h->target) return fail(NDT_ERR_NO_INPUT, "no input target");
  if (h->grid->accumulated) return fail(NDT_ERR_NO_INPUT, "getFitnessScore needs the target's points: an accumulated target keeps none");
  if (n_scans == 0) return NDT_OK;
  ndt_status s = ensure_device(h);
  if (s) return s;
  std::shared_ptr<DeviceCloud> cloud;  // the scans in the caller's order, one upload
  s = upload_cloud(h, n_pts ? static_cast<const unsigned char*>(pts) + offsets[0] * stride : nullptr, n_pts, stride, on_device, cloud);
  if (s) return s;
  std::vector<FitnessJob> jobs(n_scans);
  for (size_t k = 0; k < n_scans; k++) {
    jobs[k].g = h->grid.get();
    jobs[k].src = cloud->pts.p + (offsets[k] - offsets[0]);
    jobs[k].n = offsets[k + 1] - offsets[k];
    jobs[k].T = transforms + 16 * k;
  }
  return fitness_many(h, jobs, max_range, fitness);
}

}  // namespace ndtc

extern "C" {

ndt_status ndt_get_fitness_score(ndt_handle h, double max_range, double* fitness) {
  if (!h || !fitness) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = check_ready(h);
  if (s) return s;
  return fitness_impl(h, h->source->pts.p, static_cast<int>(h->source->n), h->final_T, max_range, fitness);
}

ndt_status ndt_pairs_fitness_scores(ndt_handle h, const float* transforms, double max_range, double* fitness) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  const size_t n = h->pairs_sources.size();
  if (n == 0) return fail(NDT_ERR_NO_INPUT, "no pairs: the last ndt_align_pairs* call failed, had no pair or was never made");
  if (!fitness) return fail(NDT_ERR_INVALID, "null fitness");
  ndt_status s = ensure_device(h);
  if (s) return s;
  std::vector<FitnessJob> jobs(n);
  for (size_t k = 0; k < n; k++) {
    DeviceCloud* c = h->pairs_sources[k].get();
    // A caller's ndt_cloud made on another handle's stream: ordered against this one (the pairs call did so already; a
    // stream destroyed since -- its handle gone -- has nothing left to wait for, and is not waited on).
    if (!c->made_on || !DevPool::instance().retired(c->made_on)) {
      s = cloud_use_on(h, c);
      if (s) return s;
    }
    jobs[k].g = h->pairs_targets[k].get();
    jobs[k].src = c->pts.p;
    jobs[k].n = c->n;
    jobs[k].T = (transforms ? transforms : h->pairs_T.data()) + 16 * k;
  }
  return fitness_many(h, jobs, max_range, fitness);
}

ndt_status ndt_pairs_count(ndt_handle h, size_t* n_pairs) {
  if (!h || !n_pairs) return fail(NDT_ERR_INVALID, "bad arguments");
  *n_pairs = h->pairs_sources.size();
  return NDT_OK;
}

ndt_status ndt_diag_fitness_launches(ndt_handle h, size_t* launches, size_t* max_blocks) {
  if (!h || !launches || !max_blocks) return fail(NDT_ERR_INVALID, "bad arguments");
  *launches = h->fit_launches;
  *max_blocks = h->fit_max_blocks;
  return NDT_OK;
}

ndt_status ndt_batch_fitness_scores(ndt_handle h, const void* pts, const size_t* offsets, size_t n_scans, size_t stride_bytes,
                                    const float* transforms, double max_range, double* fitness) {
  return batch_fitness_impl(h, pts, offsets, n_scans, stride_bytes, false, transforms, max_range, fitness);
}

ndt_status ndt_batch_fitness_scores_device(ndt_handle h, const void* d_pts, const size_t* offsets, size_t n_scans,
                                           size_t stride_bytes, const float* transforms, double max_range, double* fitness) {
  return batch_fitness_impl(h, d_pts, offsets, n_scans, stride_bytes, true, transforms, max_range, fitness);
}

}  // extern "C"
