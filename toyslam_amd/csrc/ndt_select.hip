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

// (a call of one cloud -- the usual one -- hands its segment over as a kernel argument: no table to copy up first)
__global__ __launch_bounds__(kSelBlock) void k_select_count(SelSeg one, const SelSeg* __restrict__ segs, int n_segs, ndt_select_spec spec,
                                                            unsigned long long* __restrict__ ballots, unsigned* __restrict__ counts) {
  __shared__ unsigned wave_count[kSelWaves];
  const SelSeg g = n_segs == 1 ? one : segs[ndt::member_at(n_segs, blockIdx.x, [&](int s) { return segs[s].first_block; })];
  if (g.key_range) {  // a key range of the cloud's own, computed on the device (the outlier filters' thresholds)
    spec.key_lo = g.key_range[0];
    spec.key_hi = g.key_range[1];
  }
  const int lb = static_cast<int>(blockIdx.x) - g.first_block;
  const long long start = static_cast<long long>(lb) * g.ppb;
  const int len = static_cast<int>(min(static_cast<long long>(g.ppb), g.n - start));
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

__device__ __forceinline__ float wave_min(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(kSelBlock) void k_select_place(SelSeg one, const SelSeg* __restrict__ segs, int n_segs,
                                                            const unsigned long long* __restrict__ ballots,
                                                            const unsigned* __restrict__ counts, float* __restrict__ rows,
                                                            unsigned* __restrict__ totals) {
  __shared__ unsigned wave_sum[kSelWaves];
  __shared__ float wave_box[kSelWaves][12];
  const SelSeg g = n_segs == 1 ? one : segs[ndt::member_at(n_segs, blockIdx.x, [&](int s) { return segs[s].first_block; })];
  const int lb = static_cast<int>(blockIdx.x) - g.first_block;
  const long long start = static_cast<long long>(lb) * g.ppb;
  const int len = static_cast<int>(min(static_cast<long long>(g.ppb), g.n - start));
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // the base: what the blocks before this one, in this cloud, kept
  unsigned part = 0;
  for (int j = threadIdx.x; j < lb; j += kSelBlock) part += counts[g.first_block + j];
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0) wave_sum[wave] = part;
  __syncthreads();
  unsigned run = 0;
  for (int w = 0; w < kSelWaves; w++) run += wave_sum[w];
  // box [0]: per coordinate over the values that are not NaN (fminf / fmaxf drop a NaN operand); box [1]: finite points
  float mn0[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx0[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float mn1[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx1[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
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
      const float v[3] = {p.x, p.y, p.z};
      const bool fin = __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z);
#pragma unroll
      for (int a = 0; a < 3; a++) {
        mn0[a] = fminf(mn0[a], v[a]);
        mx0[a] = fmaxf(mx0[a], v[a]);
        if (fin) {
          mn1[a] = fminf(mn1[a], v[a]);
          mx1[a] = fmaxf(mx1[a], v[a]);
        }
      }
    }
    run += total;
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float r0v = wave_min(mn0[a]), r1v = wave_max(mx0[a]), r2v = wave_min(mn1[a]), r3v = wave_max(mx1[a]);
    if (lane == 0) {
      wave_box[wave][a] = r0v;
      wave_box[wave][3 + a] = r1v;
      wave_box[wave][6 + a] = r2v;
      wave_box[wave][9 + a] = r3v;
    }
  }
  __syncthreads();
  if (threadIdx.x < 12) {
    const int t = threadIdx.x;
    const bool is_min = (t % 6) < 3;
    float v = wave_box[0][t];
    for (int w = 1; w < kSelWaves; w++) v = is_min ? fminf(v, wave_box[w][t]) : fmaxf(v, wave_box[w][t]);
    rows[static_cast<size_t>(blockIdx.x) * 12 + t] = v;
  }
  if (lb == g.n_blocks - 1 && threadIdx.x == 0) totals[g.slot] = run;
}

}  // namespace

// The two launches over all jobs and the call's one wait.  idx_host (page-locked, may be null): the indices of jobs[0] are
// copied there, all n of them, in front of the wait.
ndt_status select_run(ndt_handle h, std::vector<SelJob>& jobs, const ndt_select_spec& spec, int* idx_host) {
  hipStream_t st = h->stream;
  h->sel_launches = h->sel_blocks = 0;
  h->sel_clouds = jobs.size();
  std::vector<SelSeg> segs;
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
    segs.push_back(g);
    total_blocks += blocks;
    total_words += static_cast<unsigned long long>(blocks) * g.wpb;
  }
  if (!segs.empty()) {
    if (total_blocks > std::numeric_limits<int>::max()) return fail(NDT_ERR_INVALID, "too many points");
    const size_t nb = static_cast<size_t>(total_blocks);
    // page-locked: [segment table | totals, one per job | box rows, one per block]
    const size_t seg_bytes = (segs.size() * sizeof(SelSeg) + 15) / 16 * 16;
    const size_t tot_bytes = (jobs.size() * sizeof(unsigned) + 15) / 16 * 16;
    const size_t row_bytes = nb * 12 * sizeof(float);
    ndt_status s = pinned_at_least(h->sel_pinned, h->sel_pinned_bytes, seg_bytes + tot_bytes + row_bytes, st);
    if (s) return s;
    unsigned char* pin = static_cast<unsigned char*>(h->sel_pinned);
    unsigned* totals = reinterpret_cast<unsigned*>(pin + seg_bytes);
    float* rows = reinterpret_cast<float*>(pin + seg_bytes + tot_bytes);
    std::memcpy(pin, segs.data(), segs.size() * sizeof(SelSeg));
    std::memset(totals, 0, tot_bytes);
    DevBuf<unsigned char> d_segs;
    DevBuf<unsigned long long> ballots;
    DevBuf<unsigned> counts;
    const int n_segs = static_cast<int>(segs.size());
    if (n_segs > 1) {
      HIP_TRY(d_segs.reserve(seg_bytes));
      HIP_TRY(hipMemcpyAsync(d_segs.p, pin, seg_bytes, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(ballots.reserve(static_cast<size_t>(total_words)));
    HIP_TRY(counts.reserve(nb));
    const SelSeg* ds = reinterpret_cast<const SelSeg*>(d_segs.p);
    hipLaunchKernelGGL(k_select_count, dim3(static_cast<unsigned>(nb)), dim3(kSelBlock), 0, st, segs[0], ds, n_segs, spec, ballots.p, counts.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_select_place, dim3(static_cast<unsigned>(nb)), dim3(kSelBlock), 0, st, segs[0], ds, n_segs, ballots.p, counts.p, rows, totals);
    HIP_TRY(hipGetLastError());
    if (idx_host && jobs[0].idx && jobs[0].n)
      HIP_TRY(hipMemcpyAsync(idx_host, jobs[0].idx, jobs[0].n * sizeof(int), hipMemcpyDeviceToHost, st));
    h->sel_launches = 2;
    h->sel_blocks = nb;
    HIP_TRY(hipStreamSynchronize(st));
    for (const SelSeg& g : segs) {
      SelJob& j = jobs[static_cast<size_t>(g.slot)];
      j.kept = totals[g.slot];
      if (!j.res || j.kept == 0) continue;
      for (int b = g.first_block; b < g.first_block + g.n_blocks; b++)
        for (int v = 0; v < 2; v++)
          for (int a = 0; a < 3; a++) {
            j.res->bb_min[v][a] = std::min(j.res->bb_min[v][a], rows[static_cast<size_t>(b) * 12 + v * 6 + a]);
            j.res->bb_max[v][a] = std::max(j.res->bb_max[v][a], rows[static_cast<size_t>(b) * 12 + v * 6 + 3 + a]);
          }
      j.res->box_route = NDT_BOX_ROUTE_SELECT;
    }
  }
  for (SelJob& j : jobs)
    if (j.res) j.res->n = j.kept;
  return NDT_OK;
}

std::shared_ptr<DeviceCloud> select_new_cloud(ndt_handle h) {
  auto c = std::make_shared<DeviceCloud>();
  c->device = h->device;
  c->made_on = h->stream;
  return c;
}

// what every selection refuses of its spec
static ndt_status spec_checks(const ndt_select_spec* spec) {
  if (!spec) return fail(NDT_ERR_INVALID, "null spec");
  if (const char* why = ndt::select_spec_error(*spec)) return fail(NDT_ERR_INVALID, why);
  return NDT_OK;
}
ndt_status select_cloud_checks(ndt_handle h, ndt_cloud c) {
  if (!c || !c->c) return fail(NDT_ERR_INVALID, "null cloud");
  if (c->c->device >= 0 && c->c->device != h->device) return fail(NDT_ERR_INVALID, "the cloud lives on another device");
  if (c->c->n > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  return NDT_OK;
}

// one cloud's records (n at d_in; keys on the device or null) into a new cloud; what ndt_cloud_select and the NVTL form share
ndt_status select_one(ndt_handle h, const float4* d_in, size_t n, const ndt_select_spec& spec, const double* d_keys,
                      std::shared_ptr<DeviceCloud>& out, int32_t* kept_idx, size_t* n_kept, const double* d_key_range) {
  auto c = select_new_cloud(h);
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
  ndt_status s = select_run(h, jobs, spec, idx_host);
  if (s) {
    (void)hipStreamSynchronize(h->stream);  // (nothing queued may still write into what goes back to the pool)
    return s;
  }
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
  ndt_status s = select_cloud_checks(h, in);
  if (!s) s = spec_checks(spec);
  if (s) return s;
  if ((spec->flags & NDT_SELECT_KEY) && !keys) return fail(NDT_ERR_INVALID, "a KEY selection needs keys");
  s = ensure_device(h);
  if (!s) s = cloud_use_on(h, in->c.get());
  if (s) return s;
  const size_t n = in->c->n;
  DevBuf<double> d_keys;
  const double* kp = nullptr;
  if ((spec->flags & NDT_SELECT_KEY) && n) {
    if (keys_on_device) {
      kp = keys;
    } else {
      HIP_TRY(d_keys.reserve(n));
      HIP_TRY(hipMemcpyAsync(d_keys.p, keys, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
      kp = d_keys.p;
    }
  }
  std::shared_ptr<DeviceCloud> c;
  s = select_one(h, in->c->pts.p, n, *spec, kp, c, kept_idx, n_kept);
  if (s) return s;
  *out = new ndt_cloud_s{c};
  return NDT_OK;
}

ndt_status ndt_cloud_select_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_select_spec* spec, ndt_cloud* out,
                                   size_t* n_kept) {
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  if (n_clouds > 65535) return fail(NDT_ERR_INVALID, "at most 65535 clouds per call");
  for (size_t k = 0; k < n_clouds; k++) out[k] = nullptr;
  if (n_clouds && !in) return fail(NDT_ERR_INVALID, "null clouds");
  ndt_status s = spec_checks(spec);
  if (s) return s;
  if (spec->flags & NDT_SELECT_KEY) return fail(NDT_ERR_INVALID, "the many-clouds selection takes no KEY test");
  size_t total = 0;
  for (size_t k = 0; k < n_clouds; k++) {
    if ((s = select_cloud_checks(h, in[k]))) return s;
    total += in[k]->c->n;
  }
  if (total > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  if (n_clouds == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  // the outputs are slices of one block (room for every input point), kept alive by the slices' `owner`
  auto blk = select_new_cloud(h);
  std::vector<std::shared_ptr<DeviceCloud>> res(n_clouds);
  std::vector<SelJob> jobs(n_clouds);
  HIP_TRY(blk->pts.reserve(std::max<size_t>(total, 1)));
  blk->n = total;
  size_t first = 0;
  for (size_t k = 0; k < n_clouds; k++) {
    DeviceCloud* c = in[k]->c.get();
    if ((s = cloud_use_on(h, c))) return s;
    res[k] = select_new_cloud(h);
    jobs[k].in = c->pts.p;
    jobs[k].n = c->n;
    jobs[k].out = blk->pts.p + first;
    jobs[k].res = res[k].get();
    first += c->n;
  }
  s = select_run(h, jobs, *spec, nullptr);
  if (s) {
    (void)hipStreamSynchronize(h->stream);  // (nothing queued may still write into what goes back to the pool)
    return s;
  }
  for (size_t k = 0; k < n_clouds; k++) {
    res[k]->pts.borrow(jobs[k].out, jobs[k].kept);
    res[k]->owner = blk;
    out[k] = new ndt_cloud_s{res[k]};
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
  if (ndt_status s = spec_checks(spec)) return s;
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
