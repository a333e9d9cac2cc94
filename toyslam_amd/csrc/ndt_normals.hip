// ndt_normals.hip -- surface normals and curvature of resident clouds (ndt_cloud_estimate_normals / _clouds,
// ndt_cloud_select_by_normals / _clouds; contract: include/ndt_mi355.h, the shared host / device definitions: ndt_normals.hpp).
// Modelled on pcl::NormalEstimation; no bit parity with PCL is claimed.
//   index   : one PointIndex per input cloud, built as ndt_outliers.hip builds it (index_only, not dense: rows that are not
//             finite are simply not in it); the leaf follows the cloud's density (KNN) or the radius (RADIUS).  No result depends
//             on the leaf.  RADIUS sums in the index's own order, and the chain places a cell's points in the order they arrive:
//             k_normal_order_keys and one stable sort put every cell's points in ascending point index first, so that the order
//             of the sums is a function of the cloud and the spec alone.
//   normals : k_normals, the hot path, one launch whatever the number of clouds (a member table; a block finds its member by
//             bisection and then does what a block of a single-cloud launch does).  One wave per block, a team of eight lanes per
//             query, the exact search of ndt_search.hpp.
//             KNN is team_knn under KnnNeighbours: the ordered point indices go to the team's LDS row and ALL eight lanes gather
//             -- lane s the ranks s, s + 8, ... with four loads in flight -- into nine f64 accumulators, added across the team
//             by three xor-shuffles in a fixed tree.
//             RADIUS is the shell walk of the RADIUS outlier filter, shells pruned by the radius, its visitor handed the record
//             the walk has just loaded (team_shell<.., true>, wave_scan_all_pts): nothing per neighbour lives in LDS.  Queries
//             the shells cannot finish within max_shells go to one scan over the whole cloud by the wave.
//             Lane 0 of a team then runs normal_from_sums and writes the 16-byte record with one store, the count, and -- for
//             the selections -- the keep key.  Tallies by integer atomics, one per wave.
//   select  : the compaction of ndt_select.hip with those keys, device-resident.
// No floating-point atomics, no inline assembly.
#include "ndt_internal.hpp"
#include "ndt_normals.hpp"

#include "ndt_device.hpp"
#include "ndt_prims.hpp"
#include "ndt_search.hpp"

namespace ndtc {
namespace {

using ndt::PointIndex;
constexpr int kTeams = ndt::kNormalTeams;
constexpr int kBlock = 64;  // one wave
constexpr int kOrderBlock = 256;
constexpr int kTally = 3;   // per cloud: valid records, collinear ones, the largest neighbourhood
static_assert(kTeams == ndt::kTeamsPerWave && kTeams * ndt::kTeam == kBlock, "a block is one wave of eight teams");

// rounding: an unvisited point at true distance D may compute a d2 a few 1e-7 (relative) below D*D.  The bounds that decide
// what is NOT looked at keep 1e-5 clear of the values they are compared with, so what is looked at decides alone.
constexpr float kClear = 1.00001f;

// KNN's neighbours (ndt_search.hpp team_knn): the k nearest in (distance, point index) order, the query -- a point of the
// cloud -- among them
struct KnnNeighbours {
  static constexpr bool kPositions = true, kDropSelf = false, kCountScans = true;
  static constexpr float kClear = ndtc::kClear;
};

// what the kernel is handed of a spec and a filter
struct NormalParams {
  double viewpoint[3];
  ndt_normal_filter filter;
  int method, k, min_neighbors;
  float radius, r2;
};

struct NrmMember {
  PointIndex ix;    // mode 1: pts and n only
  float4* normals;  // n records, or null (a selection)
  int* counts;      // n, or null
  double* keys;     // n, or null
  unsigned* tally;  // [kTally]
  int first_block, n_blocks;
  int mode;  // 0: search; 1: no finite point at all -- every record is NaN, every count 0
};

// the nine sums of a neighbourhood about its query, one lane's share
struct Sums {
  double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // S1 x y z, S2 xx xy xz yy yz zz
  __device__ __forceinline__ void add(const float4& t, float qx, float qy, float qz) {
#pragma clang fp contract(off)
    const double ex = static_cast<double>(t.x) - static_cast<double>(qx), ey = static_cast<double>(t.y) - static_cast<double>(qy),
                 ez = static_cast<double>(t.z) - static_cast<double>(qz);
    s[0] += ex;
    s[1] += ey;
    s[2] += ez;
    s[3] += ex * ex;
    s[4] += ex * ey;
    s[5] += ex * ez;
    s[6] += ey * ey;
    s[7] += ey * ez;
    s[8] += ez * ez;
  }
  // the lanes [0, WIDTH) of every aligned group added in a fixed tree: every lane of the group ends with the same bits
  template <int WIDTH>
  __device__ __forceinline__ void fold() {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 1; off < WIDTH; off <<= 1) {
#pragma unroll
      for (int a = 0; a < 9; a++) s[a] += __shfl_xor(s[a], off, ndt::kWave);
    }
  }
};

// Block `block` of the `n_blocks` that cut cloud `ix`: eight queries per pass, strided by n_blocks.  KNN: the method, at
// compile time -- each method's kernel keeps its own registers (one body for both: 114 VGPRs).
template <bool KNN>
__device__ __forceinline__ void normals_block(const PointIndex& ix, int mode, const NormalParams& P, int block, int n_blocks,
                                              float4* __restrict__ normals, int* __restrict__ counts, double* __restrict__ keys,
                                              unsigned* __restrict__ tally, unsigned* __restrict__ scanned) {
#pragma clang fp contract(off)
  using namespace ndt;
  extern __shared__ unsigned char nr_lds[];
  const int lane = threadIdx.x, sub = lane & (kTeam - 1), team = lane / kTeam;
  const float qnan = __uint_as_float(0x7fc00000u);
  const double dnan = __longlong_as_double(0x7ff8000000000000ll);
  if (mode == 1) {
    for (int i = block * kBlock + lane; i < ix.n; i += n_blocks * kBlock) {
      if (normals) normals[i] = make_float4(qnan, qnan, qnan, qnan);
      if (counts) counts[i] = 0;
      if (keys) keys[i] = dnan;
    }
    return;
  }
  int* ordered = knn_row<int>(nr_lds, P.k, KnnNeighbours::kPositions, team);  // [8][k] point indices, ascending (distance, index)
  const ShellLimits lim = shell_limits(ix);
  unsigned t_valid = 0, t_line = 0, t_max = 0;  // lane 0 of a team: its queries' share of the tallies
  // The loop is uniform across the wave (a team without a query idles): the whole-cloud scan is wave-wide.
  for (int base = block * kTeams; base < ix.n; base += n_blocks * kTeams) {
    const int i = base + team;  // uniform within a team
    const bool live = i < ix.n;
    const float4 q = live ? ix.pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool search = live && finite3(q);
    Sums acc;  // lane
    int m = 0;
    if constexpr (KNN) {
      const int cnt = team_knn<KnnNeighbours>(ix, lim, P.k, nr_lds, q, search, scanned,
                                              [&](int rank, float, int p) { ordered[rank] = ix.sorted_idx[p]; });
      if (search) {
        lds_fence();
        // every lane gathers: ranks sub, sub + 8, ... in that order, four loads in flight
        auto fetch = [&](int j) { return ix.pts[min(max(ordered[min(j, cnt - 1)], 0), ix.n - 1)]; };
        for (int j = sub; j < cnt; j += 4 * kTeam) {
          const float4 t0 = fetch(j), t1 = fetch(j + kTeam), t2 = fetch(j + 2 * kTeam), t3 = fetch(j + 3 * kTeam);
          acc.add(t0, q.x, q.y, q.z);
          if (j + kTeam < cnt) acc.add(t1, q.x, q.y, q.z);
          if (j + 2 * kTeam < cnt) acc.add(t2, q.x, q.y, q.z);
          if (j + 3 * kTeam < cnt) acc.add(t3, q.x, q.y, q.z);
        }
        lds_fence();  // (the row is read: the next pass may write it)
        m = cnt;
      }
      acc.fold<kTeam>();
    } else {
      // RADIUS.  The shells out to the first whose reach clears the radius; beyond max_shells, the scan over the cloud.
      int ci = 0, cj = 0, ck = 0;
      float margin = 0.f;
      if (search) query_cell(ix.geom, q.x, q.y, q.z, ci, cj, ck, margin);
      int count_in = 0;  // lane
      auto consider = [&](float d, unsigned, bool ok, const float4& t) {
        if (ok && d <= P.r2) {
          acc.add(t, q.x, q.y, q.z);
          count_in++;
        }
      };
      const float far = P.radius * kClear;
      int r_need = 0;
      bool scan = false;
      if (search) {
        const float x = far - margin + ix.slack;
        r_need = x > 0.0f ? static_cast<int>(fminf(x / lim.leaf, 1.0e6f)) : 0;
        r_need = min(r_need, lim.r_lim);
        while (r_need < lim.r_lim && !(static_cast<float>(r_need) * lim.leaf + margin - ix.slack > far)) r_need++;
        scan = r_need > lim.r_max;
        if (!scan)
          for (int r = 0; r <= r_need; r++)
            team_shell<kTeam, true>(ix, ci, cj, ck, r, sub, q.x, q.y, q.z, consider, P.r2 * (kClear * kClear));
      }
      m = team_sum(count_in);
      acc.fold<kTeam>();
      unsigned long long open_teams = __ballot(scan && sub == 0);
      if (open_teams && lane == 0) atomicAdd(scanned, static_cast<unsigned>(__popcll(open_teams)));
      while (open_teams) {
        const int src_lane = __builtin_ctzll(open_teams);
        open_teams &= open_teams - 1;
        const float ox = __shfl(q.x, src_lane, kWave), oy = __shfl(q.y, src_lane, kWave), oz = __shfl(q.z, src_lane, kWave);
        Sums w;
        int c4 = 0;
        wave_scan_all_pts(ix, ox, oy, oz, [&](float d, int, bool ok, const float4& t) {
          if (ok && d <= P.r2) {
            w.add(t, ox, oy, oz);
            c4++;
          }
        });
        w.fold<kWave>();
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) c4 += __shfl_xor(c4, off, kWave);
        if (team == src_lane / kTeam) {
          acc = w;
          m = c4;
        }
      }
    }
    if (live && sub == 0) {
      float rec[4] = {qnan, qnan, qnan, qnan};
      if (search) {
        const float p[3] = {q.x, q.y, q.z};
        int line = 0;
        const bool valid = normal_from_sums(P.min_neighbors, P.viewpoint, p, m, acc.s, acc.s + 3, rec, &line);
        t_valid += valid ? 1u : 0u;
        t_line += static_cast<unsigned>(line);
        t_max = max(t_max, static_cast<unsigned>(m));
      }
      if (normals) normals[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
      if (counts) counts[i] = search ? m : 0;
      if (keys) keys[i] = !search ? dnan : normal_keep(P.filter, rec) ? 1.0 : 0.0;
    }
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    t_valid += __shfl_xor(t_valid, off, kWave);
    t_line += __shfl_xor(t_line, off, kWave);
    t_max = max(t_max, static_cast<unsigned>(__shfl_xor(t_max, off, kWave)));
  }
  if (lane == 0) {  // one set of integer atomics per wave
    if (t_valid) atomicAdd(tally + 0, t_valid);
    if (t_line) atomicAdd(tally + 1, t_line);
    if (t_max) atomicMax(tally + 2, t_max);
  }
}

// (a call of one cloud hands its member over as a kernel argument: no table to copy up first)
template <bool KNN>
__global__ __launch_bounds__(kBlock) void k_normals(NrmMember one, const NrmMember* __restrict__ members, int n_members, NormalParams P,
                                                    unsigned* __restrict__ scanned) {
  // (not ndt::block_member: one body fed by a select between the argument and a table entry costs k_outlier_values, whose
  // walk this is, 49 VGPRs and two waves per SIMD -- an NrmMember carries a whole PointIndex too; two calls keep each path's own)
  const int b = static_cast<int>(blockIdx.x);
  if (n_members == 1) {
    if (b < one.n_blocks) normals_block<KNN>(one.ix, one.mode, P, b, one.n_blocks, one.normals, one.counts, one.keys, one.tally, scanned);
    return;
  }
  const int lo = ndt::member_at(n_members, b, [&](int c) { return members[c].first_block; });
  const NrmMember m = members[lo];
  const int local = b - m.first_block;
  if (local >= m.n_blocks) return;
  normals_block<KNN>(m.ix, m.mode, P, local, m.n_blocks, m.normals, m.counts, m.keys, m.tally, scanned);
}

// RADIUS: the sort key of every position of the index's cell order -- (where its cell's segment starts, point index) -- a wave
// per leaf.  Sorted by it the segments stay where they are and every one ascends.
__global__ __launch_bounds__(kOrderBlock) void k_normal_order_keys(const unsigned* __restrict__ leaf_start, const int* __restrict__ leaf_count,
                                                                   int n_leaves, const int* __restrict__ sorted_idx, int n_sorted,
                                                                   unsigned long long* __restrict__ keys, int* __restrict__ vals) {
  constexpr int W = kOrderBlock / ndt::kWave;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & (ndt::kWave - 1);
  for (long long l = static_cast<long long>(blockIdx.x) * W + wave; l < n_leaves; l += static_cast<long long>(gridDim.x) * W) {
    const unsigned first = leaf_start[l];
    const int cnt = leaf_count[l];
    for (int j = lane; j < cnt; j += ndt::kWave) {
      const unsigned p = first + static_cast<unsigned>(j);
      if (p >= static_cast<unsigned>(n_sorted)) break;  // (never: the segments tile [0, n_sorted))
      const int idx = sorted_idx[p];
      keys[p] = (static_cast<unsigned long long>(first) << 32) | static_cast<unsigned>(idx);
      vals[p] = idx;
    }
  }
}

// development switch, read at every call: small values reach the strided regime with small clouds
int max_blocks_switch() { return env_block_cap("NDT_NORMAL_MAX_BLOCKS", ndt::kNormalMaxBlocks); }

size_t align256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

// every cell's points of g's index in ascending point index (queued on h's stream; g is this call's own grid)
ndt_status order_cells(ndt_handle h, DeviceGrid* g, DevBuf<unsigned char>& tmp) {
  hipStream_t st = h->stream;
  const int ns = static_cast<int>(g->n_sorted), nl = static_cast<int>(g->n_leaves);
  const size_t kb = align256(static_cast<size_t>(ns) * sizeof(unsigned long long)), vb = align256(static_cast<size_t>(ns) * sizeof(int));
  const size_t tb = std::max(ndt::sort_pairs_temp_bytes(ns, sizeof(unsigned long long)), size_t(256));
  HIP_TRY(tmp.reserve(2 * kb + vb + align256(tb)));
  unsigned long long* k_in = reinterpret_cast<unsigned long long*>(tmp.p);
  unsigned long long* k_out = reinterpret_cast<unsigned long long*>(tmp.p + kb);
  int* v_in = reinterpret_cast<int*>(tmp.p + 2 * kb);
  void* temp = tmp.p + 2 * kb + vb;
  const unsigned grid = static_cast<unsigned>(std::min<size_t>((static_cast<size_t>(nl) + 3) / 4, 16384));
  hipLaunchKernelGGL(k_normal_order_keys, dim3(std::max(grid, 1u)), dim3(kOrderBlock), 0, st, g->leaf_start.p, g->leaf_count.p, nl, g->sorted_idx.p, ns,
                     k_in, v_in);
  HIP_TRY(hipGetLastError());
  int bits = 1;
  while ((static_cast<unsigned long long>(ns) >> bits) != 0) bits++;  // the segment starts are < n_sorted
  HIP_TRY(ndt::sort_pairs(k_in, k_out, v_in, g->sorted_idx.p, ns, 32 + bits, temp, tb, st));
  HIP_TRY(ndt::launch_gather_points(g->target->pts.p, g->sorted_idx.p, g->counts.p, static_cast<int>(g->target->n), g->cell_pts.p, st));
  return NDT_OK;
}

// What one call works on: the clouds, where each one's outputs go, and what comes back
struct NormalRun {
  std::vector<std::shared_ptr<DeviceCloud>> clouds;
  std::vector<float4*> d_normals;  // per cloud: n records of device memory, or null
  std::vector<int*> d_counts;      // per cloud: n, or null
  std::vector<double*> d_keys;     // per cloud: n, or null
  std::vector<ndt_normal_stats> stats;  // per cloud, valid after the stream has been waited for (normal_finish)
  // kept until the wait
  std::vector<std::shared_ptr<DeviceGrid>> grids;
  std::vector<std::unique_ptr<DevBuf<unsigned char>>> order_tmp;
  MemberTable<NrmMember> mem;
  DevBuf<unsigned> d_tally, d_scanned;
  std::vector<unsigned> tally_host;
  unsigned scanned_host = 0;
  std::vector<size_t> n_finite;
};

// Indices and the normals launch, queued on h's stream; the read-backs are queued too but NOT waited for.
ndt_status normal_queue(ndt_handle h, const ndt_normal_spec& spec, const ndt_normal_filter* filter, NormalRun& R) {
  hipStream_t st = h->stream;
  const size_t nc = R.clouds.size();
  const bool knn = spec.method == NDT_NORMAL_KNN;
  h->nr_index_builds = h->nr_launches = h->nr_blocks = h->nr_scanned = 0;
  R.stats.assign(nc, ndt_normal_stats{});
  R.grids.resize(nc);
  R.n_finite.assign(nc, 0);
  R.tally_host.assign(nc * kTally, 0u);
  // ---- the indices
  for (size_t k = 0; k < nc; k++) {
    const std::shared_ptr<DeviceCloud>& c = R.clouds[k];
    if (c->n == 0) continue;
    ndt_status s;
    if (knn) {
      s = index_cloud_by_density(h, c, false, 0.f, nullptr, R.grids[k]);
    } else {
      s = build_grid(h, c, GridSpec{index_leaf_clamped(*c, spec.radius), 1, h->eig_ratio, 0, false, true}, R.grids[k]);
      if (!s) s = grid_counts(h, R.grids[k].get());
    }
    if (s) return s;
    h->nr_index_builds++;
    DeviceGrid* g = R.grids[k].get();
    if (!g->empty && g->n_sorted) {
      if ((s = ensure_cell2leaf(h, g))) return s;
      R.n_finite[k] = g->n_sorted;
      if (!knn) {
        R.order_tmp.emplace_back(new DevBuf<unsigned char>());
        if ((s = order_cells(h, g, *R.order_tmp.back()))) return s;
      }
    }
  }
  // ---- the member table
  NormalParams P{};
  for (int a = 0; a < 3; a++) P.viewpoint[a] = spec.viewpoint[a];
  if (filter) P.filter = *filter;
  P.method = spec.method;
  P.k = knn ? spec.k : 0;
  P.min_neighbors = spec.min_neighbors;
  P.radius = spec.radius;
  P.r2 = spec.radius * spec.radius;
  HIP_TRY(R.d_tally.reserve(std::max<size_t>(nc, 1) * kTally));
  long long blocks = 0;
  const int cap = max_blocks_switch();
  for (size_t k = 0; k < nc; k++) {
    const DeviceCloud* c = R.clouds[k].get();
    if (c->n == 0) continue;
    NrmMember m{};
    if (R.n_finite[k] == 0) {
      m.ix.pts = c->pts.p;
      m.ix.n = static_cast<int>(c->n);
      m.mode = 1;
    } else {
      fill_point_index(R.grids[k].get(), m.ix);
    }
    int nb = 0, qpb = 0;
    ndt::normal_plan(c->n, cap, &nb, &qpb);
    m.normals = R.d_normals[k];
    m.counts = R.d_counts[k];
    m.keys = R.d_keys[k];
    m.tally = R.d_tally.p + k * kTally;
    m.first_block = static_cast<int>(blocks);
    m.n_blocks = nb;
    blocks += nb;
    R.mem.host.push_back(m);
  }
  if (R.mem.host.empty()) return NDT_OK;
  if (blocks > std::numeric_limits<int>::max()) return fail(NDT_ERR_INVALID, "too many points");
  HIP_TRY(R.d_scanned.reserve(1));
  HIP_TRY(hipMemsetAsync(R.d_scanned.p, 0, sizeof(unsigned), st));
  HIP_TRY(hipMemsetAsync(R.d_tally.p, 0, nc * kTally * sizeof(unsigned), st));
  if (ndt_status s = R.mem.upload(st)) return s;
  const size_t lds = knn ? ndt::knn_lds_bytes<int>(spec.k, KnnNeighbours::kPositions) : 0;
  if (knn)
    hipLaunchKernelGGL(k_normals<true>, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), lds, st, R.mem.one(), R.mem.table(), R.mem.n(), P,
                       R.d_scanned.p);
  else
    hipLaunchKernelGGL(k_normals<false>, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), lds, st, R.mem.one(), R.mem.table(), R.mem.n(), P,
                       R.d_scanned.p);
  HIP_TRY(hipGetLastError());
  h->nr_launches = 1;
  h->nr_blocks = static_cast<size_t>(blocks);
  HIP_TRY(hipMemcpyAsync(&R.scanned_host, R.d_scanned.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(R.tally_host.data(), R.d_tally.p, nc * kTally * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  return NDT_OK;
}

// after the stream has been waited for: the statistics of every cloud, the diagnostics
void normal_finish(ndt_handle h, NormalRun& R) {
  for (size_t k = 0; k < R.clouds.size(); k++) {
    const unsigned* t = &R.tally_host[k * kTally];
    R.stats[k] = ndt_normal_stats{R.n_finite[k], t[0], t[1], t[2]};
  }
  h->nr_scanned = R.scanned_host;
}

// the selection that goes with a call: the keys are 1 (kept), 0 (not kept), NaN (not finite: never kept)
ndt_select_spec key_spec() {
  ndt_select_spec s{};
  s.flags = NDT_SELECT_KEY;
  s.key_lo = 1.0;
  s.key_hi = 1.0;
  return s;
}

ndt_status spec_checks(const ndt_normal_spec* spec) { return ndtc::spec_checks(spec, ndt::normal_spec_error); }
ndt_status filter_checks(const ndt_normal_filter* f) { return ndtc::spec_checks(f, ndt::normal_filter_error, "null filter"); }

// records and counts on their way out: at() is where the kernel writes -- the caller's device memory, or buffers whose copy to
// the caller's host memory fetch() queues
struct RecordsOut {
  DevBuf<float4> nb;
  DevBuf<int> cb;
  float* normals = nullptr;
  int32_t* counts = nullptr;
  size_t n = 0;
  bool on_device = false;
  ndt_status reserve(float* normals_, int32_t* counts_, size_t n_, int on_device_) {
    normals = normals_;
    counts = counts_;
    n = n_;
    on_device = on_device_ != 0;
    if (n && !on_device) {
      HIP_TRY(nb.reserve(n));
      if (counts) HIP_TRY(cb.reserve(n));
    }
    return NDT_OK;
  }
  float4* normals_at(size_t first) const { return (on_device ? reinterpret_cast<float4*>(normals) : nb.p) + first; }
  int* counts_at(size_t first) const { return counts ? (on_device ? counts : cb.p) + first : nullptr; }
  ndt_status fetch(hipStream_t st) {
    if (n && !on_device) {
      HIP_TRY(hipMemcpyAsync(normals, nb.p, n * sizeof(float4), hipMemcpyDeviceToHost, st));
      if (counts) HIP_TRY(hipMemcpyAsync(counts, cb.p, n * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    return NDT_OK;
  }
};

}  // namespace
}  // namespace ndtc

extern "C" {

ndt_status ndt_cloud_estimate_normals(ndt_handle h, ndt_cloud in, const ndt_normal_spec* spec, float* normals, int32_t* counts, int on_device,
                                      ndt_normal_stats* stats) {
  if (!h || !normals) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = cloud_entry(h, in, [&] { return spec_checks(spec); });
  if (s) return s;
  if (on_device && (reinterpret_cast<uintptr_t>(normals) & 15)) return fail(NDT_ERR_INVALID, "device records must be aligned to 16 bytes");
  NormalRun R;
  RecordsOut out;
  if ((s = out.reserve(normals, counts, in->c->n, on_device))) return s;
  R.clouds.push_back(in->c);
  R.d_normals.push_back(out.normals_at(0));
  R.d_counts.push_back(out.counts_at(0));
  R.d_keys.push_back(nullptr);
  {
    Drain drain{h->stream};
    s = normal_queue(h, *spec, nullptr, R);
    if (!s) s = out.fetch(h->stream);
    if (s) return s;
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  normal_finish(h, R);
  if (stats) *stats = R.stats[0];
  return NDT_OK;
}

ndt_status ndt_cloud_estimate_normals_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_normal_spec* spec, float* normals,
                                             int32_t* counts, int on_device, ndt_normal_stats* stats) {
  if (!h || (n_clouds && !normals)) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = clouds_begin(n_clouds, nullptr);
  if (s) return s;
  if (n_clouds && !in) return fail(NDT_ERR_INVALID, "null clouds");
  if ((s = spec_checks(spec))) return s;
  std::vector<size_t> first;
  if ((s = clouds_total(h, in, n_clouds, first))) return s;
  if (n_clouds == 0) return NDT_OK;
  if (on_device && (reinterpret_cast<uintptr_t>(normals) & 15)) return fail(NDT_ERR_INVALID, "device records must be aligned to 16 bytes");
  s = ensure_device(h);
  if (s) return s;
  NormalRun R;
  RecordsOut out;
  if ((s = out.reserve(normals, counts, first[n_clouds], on_device))) return s;
  for (size_t k = 0; k < n_clouds; k++) {
    if ((s = cloud_use_on(h, in[k]->c.get()))) return s;
    R.clouds.push_back(in[k]->c);
    R.d_normals.push_back(out.normals_at(first[k]));
    R.d_counts.push_back(out.counts_at(first[k]));
    R.d_keys.push_back(nullptr);
  }
  {
    Drain drain{h->stream};
    s = normal_queue(h, *spec, nullptr, R);
    if (!s) s = out.fetch(h->stream);
    if (s) return s;
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  normal_finish(h, R);
  if (stats)
    for (size_t k = 0; k < n_clouds; k++) stats[k] = R.stats[k];
  return NDT_OK;
}

ndt_status ndt_cloud_select_by_normals(ndt_handle h, ndt_cloud in, const ndt_normal_spec* spec, const ndt_normal_filter* filter, ndt_cloud* out,
                                       int32_t* kept_idx, size_t* n_kept, ndt_normal_stats* stats) {
  if (out) *out = nullptr;
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = cloud_entry(h, in, [&] {
    const ndt_status e = spec_checks(spec);
    return e ? e : filter_checks(filter);
  });
  if (s) return s;
  const size_t n = in->c->n;
  NormalRun R;
  DevBuf<double> d_keys;
  if (n) HIP_TRY(d_keys.reserve(n));
  R.clouds.push_back(in->c);
  R.d_normals.push_back(nullptr);
  R.d_counts.push_back(nullptr);
  R.d_keys.push_back(d_keys.p);
  std::shared_ptr<DeviceCloud> c;
  size_t kept = 0;
  {
    Drain drain{h->stream};
    SelDiagKeep keep(h);
    s = normal_queue(h, *spec, filter, R);
    if (s) return s;
    s = select_one(h, in->c->pts.p, n, key_spec(), d_keys.p, c, kept_idx, &kept);
    if (s) return s;
  }
  normal_finish(h, R);
  if (n_kept) *n_kept = kept;
  if (stats) *stats = R.stats[0];
  *out = new ndt_cloud_s{c};
  return NDT_OK;
}

ndt_status ndt_cloud_select_by_normals_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_normal_spec* spec,
                                              const ndt_normal_filter* filter, ndt_cloud* out, size_t* n_kept, ndt_normal_stats* stats) {
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = clouds_begin(n_clouds, out);
  if (s) return s;
  if (n_clouds && !in) return fail(NDT_ERR_INVALID, "null clouds");
  if ((s = spec_checks(spec))) return s;
  if ((s = filter_checks(filter))) return s;
  std::vector<size_t> first;
  if ((s = clouds_total(h, in, n_clouds, first))) return s;
  if (n_clouds == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  NormalRun R;
  DevBuf<double> d_keys;
  HIP_TRY(d_keys.reserve(std::max<size_t>(first[n_clouds], 1)));
  OutSlices outs;
  std::vector<SelJob> jobs(n_clouds);
  if ((s = outs.reserve(h, first))) return s;
  for (size_t k = 0; k < n_clouds; k++) {
    if ((s = cloud_use_on(h, in[k]->c.get()))) return s;
    R.clouds.push_back(in[k]->c);
    R.d_normals.push_back(nullptr);
    R.d_counts.push_back(nullptr);
    R.d_keys.push_back(d_keys.p + first[k]);
  }
  {
    Drain drain{h->stream};
    SelDiagKeep keep(h);
    s = normal_queue(h, *spec, filter, R);
    if (s) return s;
    for (size_t k = 0; k < n_clouds; k++) {
      DeviceCloud* c = in[k]->c.get();
      jobs[k].in = c->pts.p;
      jobs[k].n = c->n;
      jobs[k].keys = d_keys.p + first[k];
      jobs[k].out = outs.at(k);
      jobs[k].res = outs.cloud(k);
    }
    s = select_run(h, jobs, key_spec(), nullptr);
    if (s) return s;
  }
  normal_finish(h, R);
  for (size_t k = 0; k < n_clouds; k++) {
    out[k] = outs.publish(k, jobs[k].kept);
    if (n_kept) n_kept[k] = jobs[k].kept;
    if (stats) stats[k] = R.stats[k];
  }
  return NDT_OK;
}

ndt_status ndt_diag_normals(ndt_handle h, size_t* index_builds, size_t* launches, size_t* blocks, size_t* scanned_queries) {
  if (!h || !index_builds || !launches || !blocks || !scanned_queries) return fail(NDT_ERR_INVALID, "bad arguments");
  *index_builds = h->nr_index_builds;
  *launches = h->nr_launches;
  *blocks = h->nr_blocks;
  *scanned_queries = h->nr_scanned;
  return NDT_OK;
}

ndt_status ndt_host_normal_spec_check(const ndt_normal_spec* spec) { return spec_checks(spec); }

ndt_status ndt_host_normal_filter_check(const ndt_normal_filter* filter) { return filter_checks(filter); }

ndt_status ndt_host_normal_plan(size_t n_points, int* blocks, int* queries_per_block) {
  if (!blocks || !queries_per_block) return fail(NDT_ERR_INVALID, "bad arguments");
  if (n_points > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  ndt::normal_plan(n_points, ndtc::max_blocks_switch(), blocks, queries_per_block);
  return NDT_OK;
}

ndt_status ndt_host_normal_from_sums(const ndt_normal_spec* spec, const float xyz[3], int m, const double S1[3], const double S2[6], float out[4],
                                     int* collinear) {
  if (!xyz || !S1 || !S2 || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  if (ndt_status s = spec_checks(spec)) return s;
  int line = 0;
  ndt::normal_from_sums(spec->min_neighbors, spec->viewpoint, xyz, m, S1, S2, out, &line);
  if (collinear) *collinear = line;
  return NDT_OK;
}

ndt_status ndt_host_normal_keep(const ndt_normal_filter* filter, const float record[4], int* keep) {
  if (!record || !keep) return fail(NDT_ERR_INVALID, "bad arguments");
  if (ndt_status s = filter_checks(filter)) return s;
  *keep = ndt::normal_keep(*filter, record) ? 1 : 0;
  return NDT_OK;
}

}  // extern "C"
