// ndt_select.hip -- dropping points from resident clouds (ndt_cloud_select, ndt_cloud_select_clouds,
// ndt_source_select_by_nvtl; the predicate is ndt_select.hpp): an order-preserving compaction of the kept 16-byte records
// and the two bounding boxes of the kept points, in two launches whatever the number of clouds.
//   plan   : every cloud gets blocks of its own (select_plan: 256 threads, one contiguous range of points_per_block points
//            per block, at most 1024 blocks per cloud); a call is a table of segments (cloud -> first block, points, where
//            its ballot words start), and a block finds its segment by bisection.  A block never spans two clouds.
//   count  : k_select_count evaluates the predicate once per point, keeps the 64-bit ballot of every wave pass (one word
//            per 64 points: the second launch reads n / 8 bytes instead of the points it drops) and the block's kept count.
//   place  : k_select_place sums the counts of the blocks before it IN ITS CLOUD (at most 1023 words) for its base, ranks
//            the kept lanes of a ballot with mbcnt, copies the kept records -- all four words as they are -- to
//            base + rank, optionally the point's index, and folds the boxes of what it kept into a per-block row.  The last
//            block of a cloud writes the cloud's total.
// No block waits for another: the two launches are ordered by the stream and nothing else.  Totals and box rows are
// written straight into page-locked memory and read behind the call's one wait; the host folds the rows.
// The member table, the box fold (device and host), the output slices and the entry preambles are ndt_cloud_ops.hpp / .hip's.
#include "ndt_internal.hpp"
#include "ndt_select.hpp"

#include "ndt_device.hpp"

namespace ndtc {
namespace {

constexpr int kSelBlock = ndt::kSelectBlock;
constexpr int kSelWaves = kSelBlock / 64;

struct SelSeg {
  const float4* in;
  float4* out;
  const double* keys;  // null without KEY
  const double* key_range;  // null, or two device doubles that take the place of the spec's key_lo / key_hi for this cloud
  int* idx;            // null: no indices wanted
  unsigned long long word0;  // the cloud's first ballot word
  int n, ppb, wpb;           // points, points per block, ballot words per block
  int first_block, n_blocks;
  int slot;                  // where the cloud's total goes
};

__global__ __launch_bounds__(kSelBlock) void k_select_count(SelSeg one, const SelSeg* __restrict__ segs, int n_segs, ndt_select_spec spec,
                                                            unsigned long long* __restrict__ ballots, unsigned* __restrict__ counts) {
  __shared__ unsigned wave_count[kSelWaves];
  const SelSeg g = ndt::block_member(one, segs, n_segs, blockIdx.x, &SelSeg::first_block);
  if (g.key_range) {  // a key range of the cloud's own, computed on the device (the outlier filters' thresholds)
    spec.key_lo = g.key_range[0];
    spec.key_hi = g.key_range[1];
  }
  const int lb = static_cast<int>(blockIdx.x) - g.first_block;
  long long start;
  const int len = ndt::block_range(lb, g.ppb, g.n, &start);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned long long* bw = ballots + g.word0 + static_cast<size_t>(lb) * g.wpb;
  const bool keyed = (spec.flags & NDT_SELECT_KEY) != 0;
  unsigned kept = 0;
  for (int r0 = 0; r0 < len; r0 += kSelBlock) {
    const int i = r0 + static_cast<int>(threadIdx.x);
    bool keep = false;
    if (i < len) {
      const float4 p = g.in[start + i];
      const double k = keyed ? g.keys[start + i] : 0.0;
      keep = ndt::select_keep(spec, p.x, p.y, p.z, k);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0 && r0 + wave * 64 < len) bw[(r0 >> 6) + wave] = m;
    kept += static_cast<unsigned>(__popcll(m));
  }
  if (lane == 0) wave_count[wave] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int w = 0; w < kSelWaves; w++) t += wave_count[w];
    counts[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(kSelBlock) void k_select_place(SelSeg one, const SelSeg* __restrict__ segs, int n_segs,
                                                            const unsigned long long* __restrict__ ballots,
                                                            const unsigned* __restrict__ counts, float* __restrict__ rows,
                                                            unsigned* __restrict__ totals) {
  __shared__ unsigned wave_sum[kSelWaves];
  __shared__ float wave_box[kSelWaves][12];
  const SelSeg g = ndt::block_member(one, segs, n_segs, blockIdx.x, &SelSeg::first_block);
  const int lb = static_cast<int>(blockIdx.x) - g.first_block;
  long long start;
  const int len = ndt::block_range(lb, g.ppb, g.n, &start);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // the base: what the blocks before this one, in this cloud, kept
  unsigned part = 0;
  for (int j = threadIdx.x; j < lb; j += kSelBlock) part += counts[g.first_block + j];
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0) wave_sum[wave] = part;
  __syncthreads();
  unsigned run = 0;
  for (int w = 0; w < kSelWaves; w++) run += wave_sum[w];
  ndt::TwoBox<kSelWaves> box;  // of the kept records
  const unsigned long long* bw = ballots + g.word0 + static_cast<size_t>(lb) * g.wpb;
  for (int r0 = 0; r0 < len; r0 += kSelBlock) {
    const int w0 = r0 >> 6;
    const int nw = min(kSelWaves, (len - r0 + 63) >> 6);  // ballot words of this pass
    unsigned before = 0, total = 0;
    unsigned long long mine = 0;
    for (int q = 0; q < nw; q++) {
      const unsigned long long m = bw[w0 + q];
      const unsigned c = static_cast<unsigned>(__popcll(m));
      if (q < wave) before += c;
      if (q == wave) mine = m;
      total += c;
    }
    if ((mine >> lane) & 1ull) {
      const long long i = start + r0 + static_cast<int>(threadIdx.x);
      const unsigned rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(mine >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(mine), 0u));
      const size_t dst = static_cast<size_t>(run) + before + rank;
      const float4 p = g.in[i];
      g.out[dst] = p;
      if (g.idx) g.idx[dst] = static_cast<int>(i);
      box.add(p);
    }
    run += total;
  }
  box.to_lds(wave_box);
  __syncthreads();
  if (threadIdx.x < 12) rows[static_cast<size_t>(blockIdx.x) * 12 + threadIdx.x] = box.block_value(wave_box, threadIdx.x);
  if (lb == g.n_blocks - 1 && threadIdx.x == 0) totals[g.slot] = run;
}

}  // namespace

// The two launches over all jobs and the call's one wait.  idx_host (page-locked, may be null): the indices of jobs[0] are
// copied there, all n of them, in front of the wait.
ndt_status select_run(ndt_handle h, std::vector<SelJob>& jobs, const ndt_select_spec& spec, int* idx_host) {
  hipStream_t st = h->stream;
  h->sel_launches = h->sel_blocks = 0;
  h->sel_clouds = jobs.size();
  MemberTable<SelSeg> segs;
  long long total_blocks = 0;
  unsigned long long total_words = 0;
  for (size_t k = 0; k < jobs.size(); k++) {
    SelJob& j = jobs[k];
    j.kept = 0;
    if (j.n == 0) continue;
    SelSeg g{};
    int blocks = 0, ppb = 0;
    ndt::select_plan(j.n, &blocks, &ppb);
    g.in = j.in;
    g.out = j.out;
    g.keys = j.keys;
    g.key_range = j.key_range;
    g.idx = j.idx;
    g.word0 = total_words;
    g.n = static_cast<int>(j.n);
    g.ppb = ppb;
    g.wpb = (ppb + 63) / 64;
    g.first_block = static_cast<int>(total_blocks);
    g.n_blocks = blocks;
    g.slot = static_cast<int>(k);
    segs.host.push_back(g);
    total_blocks += blocks;
    total_words += static_cast<unsigned long long>(blocks) * g.wpb;
  }
  if (!segs.host.empty()) {
    if (total_blocks > std::numeric_limits<int>::max()) return fail(NDT_ERR_INVALID, "too many points");
    const size_t nb = static_cast<size_t>(total_blocks);
    // page-locked: [segment table | totals, one per job | box rows, one per block]
    const size_t seg_bytes = (segs.bytes() + 15) / 16 * 16;
    const size_t tot_bytes = (jobs.size() * sizeof(unsigned) + 15) / 16 * 16;
    const size_t row_bytes = nb * 12 * sizeof(float);
    ndt_status s = pinned_at_least(h->sel_pinned, h->sel_pinned_bytes, seg_bytes + tot_bytes + row_bytes, st);
    if (s) return s;
    unsigned char* pin = static_cast<unsigned char*>(h->sel_pinned);
    unsigned* totals = reinterpret_cast<unsigned*>(pin + seg_bytes);
    float* rows = reinterpret_cast<float*>(pin + seg_bytes + tot_bytes);
    std::memcpy(pin, segs.host.data(), segs.bytes());
    std::memset(totals, 0, tot_bytes);
    DevBuf<unsigned long long> ballots;
    DevBuf<unsigned> counts;
    if ((s = segs.upload(st, pin))) return s;
    HIP_TRY(ballots.reserve(static_cast<size_t>(total_words)));
    HIP_TRY(counts.reserve(nb));
    hipLaunchKernelGGL(k_select_count, dim3(static_cast<unsigned>(nb)), dim3(kSelBlock), 0, st, segs.one(), segs.table(), segs.n(), spec, ballots.p, counts.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_select_place, dim3(static_cast<unsigned>(nb)), dim3(kSelBlock), 0, st, segs.one(), segs.table(), segs.n(), ballots.p, counts.p, rows, totals);
    HIP_TRY(hipGetLastError());
    if (idx_host && jobs[0].idx && jobs[0].n)
      HIP_TRY(hipMemcpyAsync(idx_host, jobs[0].idx, jobs[0].n * sizeof(int), hipMemcpyDeviceToHost, st));
    h->sel_launches = 2;
    h->sel_blocks = nb;
    HIP_TRY(hipStreamSynchronize(st));
    for (const SelSeg& g : segs.host) {
      SelJob& j = jobs[static_cast<size_t>(g.slot)];
      j.kept = totals[g.slot];
      if (j.res && j.kept) fold_box_rows(j.res, rows, 12, g.first_block, g.n_blocks, NDT_BOX_ROUTE_SELECT);
    }
  }
  for (SelJob& j : jobs)
    if (j.res) j.res->n = j.kept;
  return NDT_OK;
}

// one cloud's records (n at d_in; keys on the device or null) into a new cloud; what ndt_cloud_select and the NVTL form share
ndt_status select_one(ndt_handle h, const float4* d_in, size_t n, const ndt_select_spec& spec, const double* d_keys,
                      std::shared_ptr<DeviceCloud>& out, int32_t* kept_idx, size_t* n_kept, const double* d_key_range) {
  auto c = new_cloud(h);
  std::vector<SelJob> jobs(1);
  DevBuf<int> d_idx;
  int* idx_host = nullptr;
  if (n) {
    HIP_TRY(c->pts.reserve(n));
    if (kept_idx) {
      HIP_TRY(d_idx.reserve(n));
      if (ndt_status s = out_block_at_least(h, n * sizeof(int))) return s;
      idx_host = static_cast<int*>(h->out_pinned);
    }
  }
  jobs[0].in = d_in;
  jobs[0].n = n;
  jobs[0].keys = d_keys;
  jobs[0].key_range = d_key_range;
  jobs[0].out = c->pts.p;
  jobs[0].idx = kept_idx ? d_idx.p : nullptr;
  jobs[0].res = c.get();
  Drain drain{h->stream};  // (on a failure nothing queued may still write into what goes back to the pool)
  if (ndt_status s = select_run(h, jobs, spec, idx_host)) return s;
  drain.done = true;  // (the run has waited)
  if (kept_idx && jobs[0].kept) std::memcpy(kept_idx, idx_host, jobs[0].kept * sizeof(int32_t));
  if (n_kept) *n_kept = jobs[0].kept;
  out = c;
  return NDT_OK;
}

}  // namespace ndtc

extern "C" {

ndt_status ndt_cloud_select(ndt_handle h, ndt_cloud in, const ndt_select_spec* spec, const double* keys, int keys_on_device,
                            ndt_cloud* out, int32_t* kept_idx, size_t* n_kept) {
  if (out) *out = nullptr;
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = cloud_entry(h, in, [&]() -> ndt_status {
    if (ndt_status e = spec_checks(spec, ndt::select_spec_error)) return e;
    if ((spec->flags & NDT_SELECT_KEY) && !keys) return fail(NDT_ERR_INVALID, "a KEY selection needs keys");
    return NDT_OK;
  });
  if (s) return s;
  const size_t n = in->c->n;
  DevBuf<double> d_keys;
  const double* kp = nullptr;
  if ((spec->flags & NDT_SELECT_KEY) && n && (s = doubles_in(h->stream, keys, n, keys_on_device, d_keys, &kp))) return s;
  std::shared_ptr<DeviceCloud> c;
  s = select_one(h, in->c->pts.p, n, *spec, kp, c, kept_idx, n_kept);
  if (s) return s;
  *out = new ndt_cloud_s{c};
  return NDT_OK;
}

ndt_status ndt_cloud_select_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_select_spec* spec, ndt_cloud* out,
                                   size_t* n_kept) {
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = clouds_begin(n_clouds, out);
  if (s) return s;
  if (n_clouds && !in) return fail(NDT_ERR_INVALID, "null clouds");
  if ((s = spec_checks(spec, ndt::select_spec_error))) return s;
  if (spec->flags & NDT_SELECT_KEY) return fail(NDT_ERR_INVALID, "the many-clouds selection takes no KEY test");
  std::vector<size_t> first;
  if ((s = clouds_total(h, in, n_clouds, first))) return s;
  if (n_clouds == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  OutSlices outs;
  std::vector<SelJob> jobs(n_clouds);
  if ((s = outs.reserve(h, first))) return s;
  for (size_t k = 0; k < n_clouds; k++) {
    DeviceCloud* c = in[k]->c.get();
    if ((s = cloud_use_on(h, c))) return s;
    jobs[k].in = c->pts.p;
    jobs[k].n = c->n;
    jobs[k].out = outs.at(k);
    jobs[k].res = outs.cloud(k);
  }
  Drain drain{h->stream};  // (on a failure nothing queued may still write into what goes back to the pool)
  if ((s = select_run(h, jobs, *spec, nullptr))) return s;
  drain.done = true;  // (the run has waited)
  for (size_t k = 0; k < n_clouds; k++) {
    out[k] = outs.publish(k, jobs[k].kept);
    if (n_kept) n_kept[k] = jobs[k].kept;
  }
  return NDT_OK;
}

ndt_status ndt_source_select_by_nvtl(ndt_handle h, const float* transform, double min_likelihood, int keep_unfound, ndt_cloud* out,
                                     size_t* n_kept, size_t* n_found) {
  if (out) *out = nullptr;
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  if (min_likelihood != min_likelihood) return fail(NDT_ERR_INVALID, "min_likelihood must not be NaN");
  ndt_status s = nvtl_ready(h, true);
  if (s) return s;
  const size_t n = h->source->n;
  HIP_TRY(h->nv_points.reserve(n));
  size_t found = 0;
  s = nvtl_launch(h, h->source->pts.p, n, transform ? transform : h->final_T, h->nv_points.p, nullptr, &found);
  if (s) return s;
  // The per-point value is L >= 0 of a found point and -1.0 of the others, so "found" is 0 <= k.
  //   keep_unfound == 0 : kept iff max(min_likelihood, 0) <= k
  //   keep_unfound != 0 : dropped iff 0 <= k < min_likelihood -- the negated range [0, the double below min_likelihood]
  ndt_select_spec spec{};
  if (!keep_unfound) {
    spec.flags = NDT_SELECT_KEY;
    spec.key_lo = std::max(min_likelihood, 0.0);
    spec.key_hi = std::numeric_limits<double>::infinity();
  } else if (min_likelihood > 0.0) {
    spec.flags = NDT_SELECT_KEY | NDT_SELECT_KEY_NEGATE;
    spec.key_lo = 0.0;
    spec.key_hi = std::nextafter(min_likelihood, 0.0);
  }
  std::shared_ptr<DeviceCloud> c;
  s = select_one(h, h->source->pts.p, n, spec, h->nv_points.p, c, nullptr, n_kept);
  if (s) return s;
  if (n_found) *n_found = found;
  *out = new ndt_cloud_s{c};
  return NDT_OK;
}

ndt_status ndt_diag_select(ndt_handle h, size_t* launches, size_t* blocks, size_t* clouds) {
  if (!h || !launches || !blocks || !clouds) return fail(NDT_ERR_INVALID, "bad arguments");
  *launches = h->sel_launches;
  *blocks = h->sel_blocks;
  *clouds = h->sel_clouds;
  return NDT_OK;
}

ndt_status ndt_host_select_point(const ndt_select_spec* spec, const float xyz[3], double key, int* keep) {
  if (!xyz || !keep) return fail(NDT_ERR_INVALID, "bad arguments");
  if (ndt_status s = spec_checks(spec, ndt::select_spec_error)) return s;
  *keep = ndt::select_keep(*spec, xyz[0], xyz[1], xyz[2], key) ? 1 : 0;
  return NDT_OK;
}

ndt_status ndt_host_select_plan(size_t n_points, int* blocks, int* points_per_block) {
  if (!blocks || !points_per_block) return fail(NDT_ERR_INVALID, "bad arguments");
  if (n_points > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  ndt::select_plan(n_points, blocks, points_per_block);
  return NDT_OK;
}

}  // extern "C"
