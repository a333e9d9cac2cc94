// ndt_outliers.hip -- the neighbourhood filters of resident clouds (ndt_cloud_neighbor_values, ndt_cloud_remove_outliers,
// ndt_cloud_remove_outliers_clouds; contract: include/ndt_mi355.h, shared host / device definitions: ndt_outliers.hpp).
// Modelled on pcl::RadiusOutlierRemoval / pcl::StatisticalOutlierRemoval; no bit parity with PCL is claimed.
//   index  : one PointIndex per input cloud (build_grid, index_only, not dense: rows that are not finite are simply not in
//            it); the leaf follows the cloud's density (STATISTICAL, GICP's rule) or the radius (RADIUS).  Time only: no
//            result depends on the leaf.
//   values : k_outlier_values, one launch whatever the number of clouds (a member table; a block finds its member by
//            bisection and then does what a block of a single-cloud launch does).  One wave per block, a team of eight lanes
//            per query, the exact shell search of ndt_search.hpp.
//            STATISTICAL is team_knn under KnnDistances (the search GICP's covariance pass runs too): a per-team LDS list of
//            the mean_k smallest DISTANCES (the value depends on the multiset of distances alone, so no positions, no tie
//            rule); the query itself is the one zero-distance candidate dropped.  The mean of the distances is taken here.
//            RADIUS counts the candidates within r2, shells pruned by the radius; counts are integers, exact by construction.
//            Queries the shells cannot finish within max_shells go to one scan over the whole cloud by the wave.
//   stats  : k_outlier_stats reduces fixed chunks of the values to (count, sum, M2 about the chunk's mean), k_outlier_merge
//            merges the rows in order by Chan's rule and writes mean, stddev, threshold and the key range of the selection --
//            f64, no floating-point atomics, a plan that depends on n alone.
//   select : the compaction of ndt_select.hip with the values as device-resident keys and, per cloud, the key range the merge
//            wrote: the values never visit the host.
#include "ndt_internal.hpp"
#include "ndt_outliers.hpp"

#include "ndt_device.hpp"
#include "ndt_search.hpp"

namespace ndtc {
namespace {

using ndt::PointIndex;
constexpr int kTeams = ndt::kOutlierTeams;
constexpr int kBlock = 64;  // one wave
static_assert(kTeams == ndt::kTeamsPerWave && kTeams * ndt::kTeam == kBlock, "a block is one wave of eight teams");

// rounding: an unvisited point at true distance D may compute a d2 a few 1e-7 (relative) below D*D.  The bounds that decide
// what is NOT looked at keep 1e-5 clear of the values they are compared with, so what is looked at decides alone.
constexpr float kClear = 1.00001f;

// STATISTICAL's neighbours (ndt_search.hpp team_knn): the mean_k smallest DISTANCES to the other points -- the value depends
// on their multiset alone, so no positions and no tie rule; the query itself is the one zero-distance candidate dropped
struct KnnDistances {
  static constexpr bool kPositions = false, kDropSelf = true, kCountScans = true;
  static constexpr float kClear = ndtc::kClear;
};

struct OutMember {
  PointIndex ix;   // mode 1: pts and n only
  double* values;  // n
  int first_block, n_blocks;
  int mode;  // 0: search; 1: no search -- a finite point's value is 0 (|F| <= mean_k, or no finite point at all)
};
struct StatMember {
  const double* values;
  double* row;  // [6]: n_valid, mean, stddev, threshold, key_lo, key_hi
  int n, chunk;
  int first_block, n_blocks;
  int degenerate;  // |F| <= mean_k: statistics and threshold are 0
};

// Block `block` of the `n_blocks` that cut cloud `ix`: eight queries per pass, strided by n_blocks.
__device__ __forceinline__ void outlier_block(const PointIndex& ix, int mode, int method, int k, float radius, float r2, int block,
                                              int n_blocks, double* __restrict__ values, unsigned* __restrict__ scanned) {
#pragma clang fp contract(off)
  using namespace ndt;
  extern __shared__ unsigned char ol_lds[];
  const int lane = threadIdx.x, sub = lane & (kTeam - 1), team = lane / kTeam;
  double* od = knn_row<double>(ol_lds, k, KnnDistances::kPositions, team);  // [8][k] distances, ascending
  const bool stat = method == NDT_OUTLIER_STATISTICAL;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (mode == 1) {
    for (int i = block * kBlock + lane; i < ix.n; i += n_blocks * kBlock) values[i] = finite3(ix.pts[i]) ? 0.0 : nan;
    return;
  }
  const ShellLimits lim = shell_limits(ix);
  // The loop is uniform across the wave (a team without a query idles): the whole-cloud scan is wave-wide.
  for (int base = block * kTeams; base < ix.n; base += n_blocks * kTeams) {
    const int i = base + team;  // uniform within a team
    const bool live = i < ix.n;
    const float4 q = live ? ix.pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool search = live && finite3(q);
    double value = nan;
    if (stat) {
      const int cnt = team_knn<KnnDistances>(ix, lim, k, ol_lds, q, search, scanned,
                                             [&](int rank, float d, int) { od[rank] = sqrt(static_cast<double>(d)); });
      if (search) {
        lds_fence();
        if (sub == 0) {
          double sum = 0.0;
          for (int j = 0; j < cnt; j++) sum += od[j];
          value = sum / static_cast<double>(k);
        }
        lds_fence();
      }
    } else {
      // RADIUS.  The shells out to the first whose reach clears the radius; beyond max_shells, the scan over the cloud.
      int ci = 0, cj = 0, ck = 0;
      float margin = 0.f;
      if (search) query_cell(ix.geom, q.x, q.y, q.z, ci, cj, ck, margin);
      int count_in = 0;  // lane
      auto consider = [&](float d, unsigned, bool ok) { count_in += (ok && d <= r2) ? 1 : 0; };
      const float far = radius * kClear;
      int r_need = 0;
      bool scan = false;
      if (search) {
        const float x = far - margin + ix.slack;
        r_need = x > 0.0f ? static_cast<int>(fminf(x / lim.leaf, 1.0e6f)) : 0;
        r_need = min(r_need, lim.r_lim);
        while (r_need < lim.r_lim && !(static_cast<float>(r_need) * lim.leaf + margin - ix.slack > far)) r_need++;
        scan = r_need > lim.r_max;
        if (!scan)
          for (int r = 0; r <= r_need; r++) team_shell(ix, ci, cj, ck, r, sub, q.x, q.y, q.z, consider, r2 * (kClear * kClear));
      }
      int total = team_sum(count_in);
      unsigned long long open_teams = __ballot(scan && sub == 0);
      if (open_teams && lane == 0) atomicAdd(scanned, static_cast<unsigned>(__popcll(open_teams)));
      while (open_teams) {
        const int src_lane = __builtin_ctzll(open_teams);
        open_teams &= open_teams - 1;
        const float ox = __shfl(q.x, src_lane, kWave), oy = __shfl(q.y, src_lane, kWave), oz = __shfl(q.z, src_lane, kWave);
        int c4 = 0;
        wave_scan_all(ix, ox, oy, oz, [&](float d, int, bool ok) { c4 += (ok && d <= r2) ? 1 : 0; });
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) c4 += __shfl_xor(c4, off, kWave);
        if (team == src_lane / kTeam) total = c4;
      }
      if (search) value = static_cast<double>(total - 1);  // the query itself is within any radius of itself
    }
    if (live && sub == 0) values[i] = value;
  }
}

// (a call of one cloud hands its member over as a kernel argument: no table to copy up first)
__global__ __launch_bounds__(kBlock) void k_outlier_values(OutMember one, const OutMember* __restrict__ members, int n_members, int method,
                                                           int k, float radius, float r2, unsigned* __restrict__ scanned) {
  // (not ndt::block_member: one body fed by a select between the argument and a table entry -- an OutMember carries a whole
  // PointIndex -- took the kernel from 75 to 124 VGPRs and from 6 to 4 waves per SIMD; two calls keep each path's own registers)
  const int b = static_cast<int>(blockIdx.x);
  if (n_members == 1) {
    if (b < one.n_blocks) outlier_block(one.ix, one.mode, method, k, radius, r2, b, one.n_blocks, one.values, scanned);
    return;
  }
  const int lo = ndt::member_at(n_members, b, [&](int c) { return members[c].first_block; });
  const OutMember m = members[lo];
  const int local = b - m.first_block;
  if (local >= m.n_blocks) return;
  outlier_block(m.ix, m.mode, method, k, radius, r2, local, m.n_blocks, m.values, scanned);
}

// rows[block] = (count, sum, M2 about sum / count) of the block's chunk of its member's values; NaN values are no values
__global__ __launch_bounds__(ndt::kOutlierStatBlock) void k_outlier_stats(const StatMember* __restrict__ members, int n_members,
                                                                        double* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ double sh[ndt::kOutlierStatBlock];
  const int b = static_cast<int>(blockIdx.x);
  const int lo = ndt::member_at(n_members, b, [&](int c) { return members[c].first_block; });
  const StatMember m = members[lo];
  const int lb = b - m.first_block;
  if (lb >= m.n_blocks) return;
  long long start;
  const int len = ndt::block_range(lb, m.chunk, m.n, &start);
  double cnt = 0.0, sum = 0.0;
  for (int j = threadIdx.x; j < len; j += ndt::kOutlierStatBlock) {
    const double v = m.values[start + j];
    if (v == v) {
      cnt += 1.0;
      sum += v;
    }
  }
  cnt = ndt::block_sum<ndt::kOutlierStatBlock>(cnt, sh);
  sum = ndt::block_sum<ndt::kOutlierStatBlock>(sum, sh);
  const double mean = cnt > 0.0 ? sum / cnt : 0.0;
  double m2 = 0.0;
  for (int j = threadIdx.x; j < len; j += ndt::kOutlierStatBlock) {
    const double v = m.values[start + j];
    if (v == v) m2 += (v - mean) * (v - mean);
  }
  m2 = ndt::block_sum<ndt::kOutlierStatBlock>(m2, sh);
  if (threadIdx.x == 0) {
    rows[static_cast<size_t>(b) * 3 + 0] = cnt;
    rows[static_cast<size_t>(b) * 3 + 1] = sum;
    rows[static_cast<size_t>(b) * 3 + 2] = m2;
  }
}

// one thread per member: its rows merged in block order (Chan), then mean, stddev, threshold and the selection's key range
__global__ __launch_bounds__(64) void k_outlier_merge(const StatMember* __restrict__ members, int n_members, const double* __restrict__ rows,
                                                      double stddev_mul) {
#pragma clang fp contract(off)
  const int t = static_cast<int>(blockIdx.x) * 64 + static_cast<int>(threadIdx.x);
  if (t >= n_members) return;
  const StatMember m = members[t];
  double na = 0.0, mean = 0.0, m2 = 0.0;
  if (!m.degenerate)
    for (int b = 0; b < m.n_blocks; b++) {
      const double* r = rows + static_cast<size_t>(m.first_block + b) * 3;
      const double nb = r[0];
      if (nb == 0.0) continue;
      const double mean_b = r[1] / nb, n = na + nb, delta = mean_b - mean;
      mean = mean + delta * (nb / n);
      m2 = (m2 + r[2]) + (delta * delta) * (na * nb / n);
      na = n;
    }
  const double sd = na >= 2.0 ? sqrt(m2 / (na - 1.0)) : 0.0;
  const double thr = mean + stddev_mul * sd;
  m.row[0] = na;
  m.row[1] = mean;
  m.row[2] = sd;
  m.row[3] = thr;
  m.row[4] = -__longlong_as_double(0x7ff0000000000000ll);
  m.row[5] = thr;
}

int max_blocks_switch() {  // development switch, read once: small values reach the strided regime with small clouds
  static const int v = env_block_cap("NDT_OUTLIER_MAX_BLOCKS", ndt::kOutlierMaxBlocks);
  return v;
}

// What one call works on: the clouds, where each one's values go, and what comes back
struct OutlierRun {
  std::vector<std::shared_ptr<DeviceCloud>> clouds;
  std::vector<double*> d_values;          // per cloud: n doubles of device memory (ignored where n == 0)
  std::vector<ndt_outlier_stats> stats;   // per cloud, valid after the stream has been waited for (finish())
  DevBuf<double> d_rows;                  // per cloud [6]: the merge's row (STATISTICAL); +4: the selection's key range
  // kept until the wait
  std::vector<std::shared_ptr<DeviceGrid>> grids;
  MemberTable<OutMember> mem;
  std::vector<StatMember> smem;
  std::vector<double> rows_host;
  unsigned scanned_host = 0;
  DevBuf<unsigned char> d_smem;
  DevBuf<double> d_partials;
  DevBuf<unsigned> d_scanned;
  std::vector<size_t> n_finite;
  std::vector<char> degenerate;
};

// Everything up to and including the merge, queued on h's stream; the read-backs are queued too but NOT waited for.
ndt_status outlier_queue(ndt_handle h, const ndt_outlier_spec& spec, OutlierRun& R) {
  hipStream_t st = h->stream;
  const size_t nc = R.clouds.size();
  const bool stat = spec.method == NDT_OUTLIER_STATISTICAL;
  h->ol_index_builds = h->ol_value_launches = h->ol_value_blocks = h->ol_scanned = 0;
  R.stats.assign(nc, ndt_outlier_stats{});
  R.grids.resize(nc);
  R.n_finite.assign(nc, 0);
  R.degenerate.assign(nc, 1);
  // ---- the indices
  for (size_t k = 0; k < nc; k++) {
    const std::shared_ptr<DeviceCloud>& c = R.clouds[k];
    if (c->n == 0) continue;
    ndt_status s;
    if (stat) {
      s = index_cloud_by_density(h, c, false, 0.f, nullptr, R.grids[k]);
    } else {
      s = build_grid(h, c, GridSpec{index_leaf_clamped(*c, spec.radius), 1, h->eig_ratio, 0, false, true}, R.grids[k]);
      if (!s) s = grid_counts(h, R.grids[k].get());
    }
    if (s) return s;
    h->ol_index_builds++;
    DeviceGrid* g = R.grids[k].get();
    if (!g->empty && g->n_sorted) {
      if ((s = ensure_cell2leaf(h, g))) return s;
      R.n_finite[k] = g->n_sorted;
    }
    R.degenerate[k] = R.n_finite[k] == 0 || (stat && R.n_finite[k] <= static_cast<size_t>(spec.mean_k));
  }
  // ---- the value launch
  long long blocks = 0, sblocks = 0;
  for (size_t k = 0; k < nc; k++) {
    const DeviceCloud* c = R.clouds[k].get();
    if (c->n == 0) continue;
    OutMember m{};
    if (R.degenerate[k]) {
      m.ix.pts = c->pts.p;
      m.ix.n = static_cast<int>(c->n);
      m.mode = 1;
    } else {
      fill_point_index(R.grids[k].get(), m.ix);
    }
    int nb = 0, qpb = 0;
    ndt::outlier_plan(c->n, &nb, &qpb);
    m.values = R.d_values[k];
    m.first_block = static_cast<int>(blocks);
    m.n_blocks = std::min(nb, max_blocks_switch());
    blocks += m.n_blocks;
    R.mem.host.push_back(m);
    if (stat) {
      StatMember sm{};
      sm.values = R.d_values[k];
      sm.n = static_cast<int>(c->n);
      ndt::outlier_stat_plan(c->n, &sm.n_blocks, &sm.chunk);
      sm.first_block = static_cast<int>(sblocks);
      sm.degenerate = R.degenerate[k];
      sblocks += sm.n_blocks;
      R.smem.push_back(sm);  // (row: below, once the rows are allocated)
    }
  }
  HIP_TRY(R.d_rows.reserve(std::max<size_t>(nc, 1) * 6));
  if (R.mem.host.empty()) return NDT_OK;
  if (blocks > std::numeric_limits<int>::max()) return fail(NDT_ERR_INVALID, "too many points");
  const int n_mem = R.mem.n();
  HIP_TRY(R.d_scanned.reserve(1));
  HIP_TRY(hipMemsetAsync(R.d_scanned.p, 0, sizeof(unsigned), st));
  if (ndt_status s = R.mem.upload(st)) return s;
  const int kk = stat ? spec.mean_k : 0;
  const size_t lds = stat ? ndt::knn_lds_bytes<double>(kk, KnnDistances::kPositions) : 0;
  hipLaunchKernelGGL(k_outlier_values, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), lds, st, R.mem.one(),
                     R.mem.table(), n_mem, spec.method, kk, spec.radius, spec.radius * spec.radius,
                     R.d_scanned.p);
  HIP_TRY(hipGetLastError());
  h->ol_value_launches = 1;
  h->ol_value_blocks = static_cast<size_t>(blocks);
  HIP_TRY(hipMemcpyAsync(&R.scanned_host, R.d_scanned.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  // ---- the statistics
  if (stat) {
    size_t j = 0;
    for (size_t k = 0; k < nc; k++)
      if (R.clouds[k]->n) R.smem[j++].row = R.d_rows.p + 6 * k;
    HIP_TRY(R.d_smem.reserve(R.smem.size() * sizeof(StatMember)));
    HIP_TRY(hipMemcpyAsync(R.d_smem.p, R.smem.data(), R.smem.size() * sizeof(StatMember), hipMemcpyHostToDevice, st));
    HIP_TRY(R.d_partials.reserve(static_cast<size_t>(sblocks) * 3));
    const StatMember* dsm = reinterpret_cast<const StatMember*>(R.d_smem.p);
    hipLaunchKernelGGL(k_outlier_stats, dim3(static_cast<unsigned>(sblocks)), dim3(ndt::kOutlierStatBlock), 0, st, dsm, n_mem, R.d_partials.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_outlier_merge, dim3(static_cast<unsigned>((n_mem + 63) / 64)), dim3(64), 0, st, dsm, n_mem, R.d_partials.p,
                       spec.stddev_mul);
    HIP_TRY(hipGetLastError());
    R.rows_host.assign(nc * 6, 0.0);
    for (size_t k = 0; k < nc; k++)  // (a cloud without a point has no row on the device)
      if (R.clouds[k]->n)
        HIP_TRY(hipMemcpyAsync(&R.rows_host[6 * k], R.d_rows.p + 6 * k, 6 * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  return NDT_OK;
}

// after the stream has been waited for: the statistics of every cloud, the diagnostics
void outlier_finish(ndt_handle h, const ndt_outlier_spec& spec, OutlierRun& R) {
  const bool stat = spec.method == NDT_OUTLIER_STATISTICAL;
  for (size_t k = 0; k < R.clouds.size(); k++) {
    ndt_outlier_stats& s = R.stats[k];
    s.n_finite = R.n_finite[k];
    if (!stat) {
      s.n_valid = s.n_finite;
      s.threshold = static_cast<double>(spec.min_neighbors);
    } else if (!R.degenerate[k]) {
      s.n_valid = s.n_finite;
      s.mean = R.rows_host[6 * k + 1];
      s.stddev = R.rows_host[6 * k + 2];
      s.threshold = R.rows_host[6 * k + 3];
    }
  }
  h->ol_scanned = R.scanned_host;
}

// the selection that goes with a spec: the values are the keys
ndt_select_spec key_spec(const ndt_outlier_spec& spec) {
  ndt_select_spec s{};
  s.flags = NDT_SELECT_KEY | (spec.negate ? NDT_SELECT_KEY_NEGATE : 0);
  if (spec.method == NDT_OUTLIER_RADIUS) {
    s.key_lo = static_cast<double>(spec.min_neighbors);
    s.key_hi = std::numeric_limits<double>::infinity();
  } else {  // (the range of every cloud comes from the device: [-inf, its threshold])
    s.key_lo = -std::numeric_limits<double>::infinity();
    s.key_hi = std::numeric_limits<double>::infinity();
  }
  return s;
}

ndt_status spec_checks(const ndt_outlier_spec* spec) { return ndtc::spec_checks(spec, ndt::outlier_spec_error); }

}  // namespace
}  // namespace ndtc

extern "C" {

ndt_status ndt_cloud_neighbor_values(ndt_handle h, ndt_cloud in, const ndt_outlier_spec* spec, double* values, int values_on_device,
                                     ndt_outlier_stats* stats) {
  if (!h || !values) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = cloud_entry(h, in, [&] { return spec_checks(spec); });
  if (s) return s;
  OutlierRun R;
  DoublesOut vals;
  if ((s = vals.reserve(values, in->c->n, values_on_device))) return s;
  R.clouds.push_back(in->c);
  R.d_values.push_back(vals.at());
  {
    Drain drain{h->stream};
    s = outlier_queue(h, *spec, R);
    if (!s) s = vals.fetch(h->stream);
    if (s) return s;
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  outlier_finish(h, *spec, R);
  if (stats) *stats = R.stats[0];
  return NDT_OK;
}

ndt_status ndt_cloud_remove_outliers(ndt_handle h, ndt_cloud in, const ndt_outlier_spec* spec, ndt_cloud* out, int32_t* kept_idx,
                                     size_t* n_kept, ndt_outlier_stats* stats) {
  if (out) *out = nullptr;
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = cloud_entry(h, in, [&] { return spec_checks(spec); });
  if (s) return s;
  const size_t n = in->c->n;
  OutlierRun R;
  DevBuf<double> d_vals;
  if (n) HIP_TRY(d_vals.reserve(n));
  R.clouds.push_back(in->c);
  R.d_values.push_back(d_vals.p);
  std::shared_ptr<DeviceCloud> c;
  size_t kept = 0;
  {
    Drain drain{h->stream};
    SelDiagKeep keep(h);
    s = outlier_queue(h, *spec, R);
    if (s) return s;
    const bool own_range = spec->method == NDT_OUTLIER_STATISTICAL && n;
    s = select_one(h, in->c->pts.p, n, key_spec(*spec), d_vals.p, c, kept_idx, &kept, own_range ? R.d_rows.p + 4 : nullptr);
    if (s) return s;
  }
  outlier_finish(h, *spec, R);
  if (n_kept) *n_kept = kept;
  if (stats) *stats = R.stats[0];
  *out = new ndt_cloud_s{c};
  return NDT_OK;
}

ndt_status ndt_cloud_remove_outliers_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_outlier_spec* spec, ndt_cloud* out,
                                            size_t* n_kept, ndt_outlier_stats* stats) {
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = clouds_begin(n_clouds, out);
  if (s) return s;
  if (n_clouds && !in) return fail(NDT_ERR_INVALID, "null clouds");
  if ((s = spec_checks(spec))) return s;
  std::vector<size_t> first;
  if ((s = clouds_total(h, in, n_clouds, first))) return s;
  if (n_clouds == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  OutlierRun R;
  DevBuf<double> d_vals;
  HIP_TRY(d_vals.reserve(std::max<size_t>(first[n_clouds], 1)));
  OutSlices outs;
  std::vector<SelJob> jobs(n_clouds);
  if ((s = outs.reserve(h, first))) return s;
  for (size_t k = 0; k < n_clouds; k++) {
    if ((s = cloud_use_on(h, in[k]->c.get()))) return s;
    R.clouds.push_back(in[k]->c);
    R.d_values.push_back(d_vals.p + first[k]);
  }
  {
    Drain drain{h->stream};
    SelDiagKeep keep(h);
    s = outlier_queue(h, *spec, R);
    if (s) return s;
    for (size_t k = 0; k < n_clouds; k++) {
      DeviceCloud* c = in[k]->c.get();
      jobs[k].in = c->pts.p;
      jobs[k].n = c->n;
      jobs[k].keys = d_vals.p + first[k];
      jobs[k].key_range = spec->method == NDT_OUTLIER_STATISTICAL ? R.d_rows.p + 6 * k + 4 : nullptr;
      jobs[k].out = outs.at(k);
      jobs[k].res = outs.cloud(k);
    }
    s = select_run(h, jobs, key_spec(*spec), nullptr);
    if (s) return s;
  }
  outlier_finish(h, *spec, R);
  for (size_t k = 0; k < n_clouds; k++) {
    out[k] = outs.publish(k, jobs[k].kept);
    if (n_kept) n_kept[k] = jobs[k].kept;
    if (stats) stats[k] = R.stats[k];
  }
  return NDT_OK;
}

ndt_status ndt_diag_outliers(ndt_handle h, size_t* index_builds, size_t* value_launches, size_t* value_blocks, size_t* scanned_queries) {
  if (!h || !index_builds || !value_launches || !value_blocks || !scanned_queries) return fail(NDT_ERR_INVALID, "bad arguments");
  *index_builds = h->ol_index_builds;
  *value_launches = h->ol_value_launches;
  *value_blocks = h->ol_value_blocks;
  *scanned_queries = h->ol_scanned;
  return NDT_OK;
}

ndt_status ndt_host_outlier_spec_check(const ndt_outlier_spec* spec) { return spec_checks(spec); }

ndt_status ndt_host_outlier_plan(size_t n_points, int* blocks, int* queries_per_block) {
  if (!blocks || !queries_per_block) return fail(NDT_ERR_INVALID, "bad arguments");
  if (n_points > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  ndt::outlier_plan(n_points, blocks, queries_per_block);
  return NDT_OK;
}

}  // extern "C"
