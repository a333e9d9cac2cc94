// ndt_plane.hip -- the dominant plane of resident clouds by RANSAC (ndt_cloud_plane_counts, ndt_cloud_segment_plane,
// ndt_cloud_segment_plane_clouds, ndt_cloud_plane_distances; contract: include/ndt_mi355.h, shared host / device definitions:
// ndt_plane.hpp).  Modelled on pcl::SACSegmentation + pcl::ExtractIndices; no bit parity with PCL is claimed.
//   models : k_plane_models, one thread per (cloud, hypothesis): the sample (or the caller's triple), three records gathered,
//            the model of ndt_plane.hpp -- 4 f64 and the state.
//   counts : k_plane_counts, the hot path.  LANES ARE HYPOTHESES: a thread holds one model in registers; the block's tile of
//            points is staged in LDS once as f64 (x[], y[], z[]: the staging stores are conflict-free) and every lane walks the
//            tile reading the SAME address per step, a broadcast.  No reduction inside the loop: a lane keeps one integer.  A
//            (tile slot, hypothesis block) pair ends with one integer atomic add per lane, or (NDT_PLANE_MERGE=rows) with a
//            partial row the choice launch sums in slot order; integer counts are exact either way.  One launch whatever the
//            number of clouds (a member table; a block finds its member by bisection).
//   choice : k_plane_best, one block per cloud: arg-max over the valid hypotheses, lowest h among equals; writes the chosen
//            model, its first sample point and the state tallies where the later kernels read them (the cloud's `chosen` row).
//   sums   : k_plane_sums (refinement): per block (count, S1, S2) of the chosen plane's inliers about a, a fixed tree; the
//            rows are added in block order on the host, which solves the fit (plane_fit) and writes the refined model back.
//   keys   : k_plane_keys writes s per point from the device-resident model (NaN: not finite; +inf: no plane) and tallies the
//            inliers and the finite points with integer atomics.  The compaction of ndt_select.hip follows with the keys.
// No floating-point atomics, no inline assembly.
#include "ndt_internal.hpp"
#include "ndt_plane.hpp"
#include "ndt_select.hpp"

#include "ndt_device.hpp"

namespace ndtc {
namespace {

using ndt::PlaneParams;
constexpr int kBlock = ndt::kPlaneBlock;
constexpr int kTile = ndt::kPlaneTile;
constexpr int kChosen = 16;   // doubles of a cloud's chosen row: found, best, best_count, n_degenerate, n_rejected, coeff[4], a[3]
constexpr int kSumRow = 10;   // doubles of a block's row of the sums: count, S1[3], S2[6]

struct PlaneMember {
  const float4* pts;
  int n;
  double* models;      // [H][4]
  int* states;         // [H]
  unsigned* counts;    // [H]
  unsigned* partials;  // [tile_blocks][H] (rows form)
  double* chosen;      // [kChosen]
  unsigned* tally;     // [2]: inliers, finite points (the key launch)
  double* keys;        // [n]
  double* sum_rows;    // [sum_blocks][kSumRow]
  int first_block, n_blocks, tiles, hyp_blocks, tile_blocks;  // the count launch
  int key_first, key_blocks, key_ppb;                         // the key launch (select_plan)
  int sum_first, sum_blocks, sum_chunk;                       // the sums launch (plane_sum_plan)
};

// (a call of one cloud hands its member over as a kernel argument: no table to copy up first)
__global__ __launch_bounds__(256) void k_plane_models(PlaneMember one, const PlaneMember* __restrict__ members, int n_members, PlaneParams P,
                                                      const int* __restrict__ triples) {
  const long long g = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  const int H = P.n_hypotheses;
  if (g >= static_cast<long long>(n_members) * H) return;
  const int c = static_cast<int>(g / H), h = static_cast<int>(g % H);
  const PlaneMember m = ndt::member_of(one, members, n_members, c);
  double coeff[4] = {0.0, 0.0, 0.0, 0.0};
  int state = ndt::kPlaneDegenerateState;
  if (m.n >= 3) {
    int i0, i1, i2;
    if (triples) {
      i0 = triples[3 * h];
      i1 = triples[3 * h + 1];
      i2 = triples[3 * h + 2];
    } else {
      i0 = ndt::plane_sample(P.seed, h, 0, m.n);
      i1 = ndt::plane_sample(P.seed, h, 1, m.n);
      i2 = ndt::plane_sample(P.seed, h, 2, m.n);
    }
    const float4 a = m.pts[i0], b = m.pts[i1], cc = m.pts[i2];
    const float a3[3] = {a.x, a.y, a.z}, b3[3] = {b.x, b.y, b.z}, c3[3] = {cc.x, cc.y, cc.z};
    state = ndt::plane_model(P, a3, b3, c3, i0 == i1 || i0 == i2 || i1 == i2, coeff);
  }
  double* out = m.models + static_cast<size_t>(h) * 4;
  out[0] = coeff[0];
  out[1] = coeff[1];
  out[2] = coeff[2];
  out[3] = coeff[3];
  m.states[h] = state;
}

__global__ __launch_bounds__(kBlock) void k_plane_counts(PlaneMember one, const PlaneMember* __restrict__ members, int n_members, int H,
                                                         double T, int rows_form) {
  __shared__ double tx[kTile], ty[kTile], tz[kTile];
  const int b = static_cast<int>(blockIdx.x);
  const PlaneMember m = ndt::block_member(one, members, n_members, b, &PlaneMember::first_block);
  const int lb = b - m.first_block;
  if (lb >= m.n_blocks) return;  // (uniform over the block)
  const int hb = lb % m.hyp_blocks, slot = lb / m.hyp_blocks;
  const int h = hb * kBlock + static_cast<int>(threadIdx.x);
  const bool live = h < H;
  double nx = 0.0, ny = 0.0, nz = 0.0, d = 0.0;
  bool valid = false;
  if (live) {
    const double* mod = m.models + static_cast<size_t>(h) * 4;
    nx = mod[0];
    ny = mod[1];
    nz = mod[2];
    d = mod[3];
    valid = m.states[h] == ndt::kPlaneValid;
  }
  unsigned cnt = 0;
  for (int t = slot; t < m.tiles; t += m.tile_blocks) {
    long long start;
    const int len = ndt::block_range(t, kTile, m.n, &start);
    __syncthreads();  // the tile before this one has been walked by every wave
    for (int i = threadIdx.x; i < len; i += kBlock) {
      const float4 p = m.pts[start + i];
      tx[i] = static_cast<double>(p.x);
      ty[i] = static_cast<double>(p.y);
      tz[i] = static_cast<double>(p.z);
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < len; i++) {
      const double s = ndt::plane_distance(nx, ny, nz, d, tx[i], ty[i], tz[i]);
      cnt += ndt::plane_inlier(s, T) ? 1u : 0u;
    }
  }
  if (!live) return;
  if (!valid) cnt = 0;
  if (rows_form) m.partials[static_cast<size_t>(slot) * H + h] = cnt;
  else if (cnt) atomicAdd(&m.counts[h], cnt);
}

__global__ __launch_bounds__(kBlock) void k_plane_best(PlaneMember one, const PlaneMember* __restrict__ members, int n_members, PlaneParams P,
                                                       const int* __restrict__ triples, int rows_form) {
  __shared__ long long s_cnt[kBlock];
  __shared__ int s_h[kBlock];
  __shared__ unsigned s_deg[kBlock], s_rej[kBlock];
  const PlaneMember m = ndt::member_of(one, members, n_members, blockIdx.x);
  const int H = P.n_hypotheses, tid = threadIdx.x;
  long long bc = -1;  // the best count so far; -1: no valid hypothesis seen
  int bh = H;
  unsigned ndeg = 0, nrej = 0;
  for (int h = tid; h < H; h += kBlock) {
    unsigned c;
    if (rows_form) {
      c = 0;
      for (int s = 0; s < m.tile_blocks; s++) c += m.partials[static_cast<size_t>(s) * H + h];
      m.counts[h] = c;
    } else {
      c = m.counts[h];
    }
    const int st = m.states[h];
    if (st == ndt::kPlaneValid) {
      if (static_cast<long long>(c) > bc) {  // (h ascends: the first of equals stays)
        bc = c;
        bh = h;
      }
    } else if (st == ndt::kPlaneDegenerateState) {
      ndeg++;
    } else {
      nrej++;
    }
  }
  s_cnt[tid] = bc;
  s_h[tid] = bh;
  s_deg[tid] = ndeg;
  s_rej[tid] = nrej;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const long long oc = s_cnt[tid + s];
      const int oh = s_h[tid + s];
      if (oc > s_cnt[tid] || (oc == s_cnt[tid] && oh < s_h[tid])) {
        s_cnt[tid] = oc;
        s_h[tid] = oh;
      }
      s_deg[tid] += s_deg[tid + s];
      s_rej[tid] += s_rej[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* row = m.chosen;
    const bool found = s_cnt[0] >= 0;
    const int best = found ? s_h[0] : -1;
    row[0] = found ? 1.0 : 0.0;
    row[1] = static_cast<double>(best);
    row[2] = found ? static_cast<double>(s_cnt[0]) : 0.0;
    row[3] = static_cast<double>(s_deg[0]);
    row[4] = static_cast<double>(s_rej[0]);
    for (int k = 5; k < kChosen; k++) row[k] = 0.0;
    if (found) {
      const double* mod = m.models + static_cast<size_t>(best) * 4;
      row[5] = mod[0];
      row[6] = mod[1];
      row[7] = mod[2];
      row[8] = mod[3];
      const int i0 = triples ? triples[3 * best] : ndt::plane_sample(P.seed, best, 0, m.n);
      const float4 a = m.pts[i0];
      row[9] = static_cast<double>(a.x);
      row[10] = static_cast<double>(a.y);
      row[11] = static_cast<double>(a.z);
    }
  }
}

__global__ __launch_bounds__(ndt::kPlaneSumBlock) void k_plane_sums(PlaneMember one, const PlaneMember* __restrict__ members, int n_members,
                                                                    double T) {
#pragma clang fp contract(off)
  __shared__ double sh[ndt::kPlaneSumBlock];
  const int b = static_cast<int>(blockIdx.x);
  const PlaneMember m = ndt::block_member(one, members, n_members, b, &PlaneMember::sum_first);
  const int lb = b - m.sum_first;
  if (lb >= m.sum_blocks) return;
  const bool found = m.chosen[0] != 0.0;
  const double nx = m.chosen[5], ny = m.chosen[6], nz = m.chosen[7], d = m.chosen[8];
  const double ax = m.chosen[9], ay = m.chosen[10], az = m.chosen[11];
  long long start;
  const int len = found ? ndt::block_range(lb, m.sum_chunk, m.n, &start) : 0;
  double acc[kSumRow] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = threadIdx.x; j < len; j += ndt::kPlaneSumBlock) {
    const float4 p = m.pts[start + j];
    const double px = static_cast<double>(p.x), py = static_cast<double>(p.y), pz = static_cast<double>(p.z);
    if (!ndt::plane_inlier(ndt::plane_distance(nx, ny, nz, d, px, py, pz), T)) continue;
    const double qx = px - ax, qy = py - ay, qz = pz - az;
    acc[0] += 1.0;
    acc[1] += qx;
    acc[2] += qy;
    acc[3] += qz;
    acc[4] += qx * qx;
    acc[5] += qx * qy;
    acc[6] += qx * qz;
    acc[7] += qy * qy;
    acc[8] += qy * qz;
    acc[9] += qz * qz;
  }
  double* row = m.sum_rows + static_cast<size_t>(lb) * kSumRow;
#pragma unroll
  for (int k = 0; k < kSumRow; k++) {
    const double v = ndt::block_sum<ndt::kPlaneSumBlock>(acc[k], sh);
    if (threadIdx.x == 0) row[k] = v;
  }
}

__global__ __launch_bounds__(256) void k_plane_keys(PlaneMember one, const PlaneMember* __restrict__ members, int n_members, double T) {
  __shared__ unsigned w_in[4], w_fin[4];
  const int b = static_cast<int>(blockIdx.x);
  const PlaneMember m = ndt::block_member(one, members, n_members, b, &PlaneMember::key_first);
  const int lb = b - m.key_first;
  if (lb >= m.key_blocks) return;
  const bool found = m.chosen[0] != 0.0;
  const double nx = m.chosen[5], ny = m.chosen[6], nz = m.chosen[7], d = m.chosen[8];
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  long long start;
  const int len = ndt::block_range(lb, m.key_ppb, m.n, &start);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned n_in = 0, n_fin = 0;
  for (int r0 = 0; r0 < len; r0 += 256) {
    const int i = r0 + static_cast<int>(threadIdx.x);
    bool fin = false, in = false;
    if (i < len) {
      const float4 p = m.pts[start + i];
      fin = ndt::finite3(p);
      double s = nan;
      if (fin) {
        s = found ? ndt::plane_distance(nx, ny, nz, d, static_cast<double>(p.x), static_cast<double>(p.y), static_cast<double>(p.z)) : inf;
        in = found && ndt::plane_inlier(s, T);
      }
      m.keys[start + i] = s;
    }
    n_in += static_cast<unsigned>(__popcll(__ballot(in)));
    n_fin += static_cast<unsigned>(__popcll(__ballot(fin)));
  }
  if (!m.tally) return;
  if (lane == 0) {
    w_in[wave] = n_in;
    w_fin[wave] = n_fin;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned a = w_in[0] + w_in[1] + w_in[2] + w_in[3], f = w_fin[0] + w_fin[1] + w_fin[2] + w_fin[3];
    if (a) atomicAdd(&m.tally[0], a);
    if (f) atomicAdd(&m.tally[1], f);
  }
}

// development switches, read at every call (tools alternate the two merge forms in one process)
int max_blocks_switch() { return env_block_cap("NDT_PLANE_MAX_BLOCKS", ndt::kPlaneMaxBlocks); }
bool rows_switch() {
  const char* e = getenv("NDT_PLANE_MERGE");
  return e && std::strcmp(e, "rows") == 0;
}

// What one call works on
struct PlaneRun {
  std::vector<std::shared_ptr<DeviceCloud>> clouds;
  PlaneParams P{};
  int refine = 0;
  const int* d_triples = nullptr;
  double* keys_override = nullptr;  // the distances call: where the one cloud's keys go instead of d_keys
  bool rows = false;
  MemberTable<PlaneMember> mem;
  DevBuf<double> d_models, d_chosen, d_keys, d_sum_rows;
  DevBuf<int> d_states;
  DevBuf<unsigned> d_counts, d_partials, d_tally;
  long long count_blocks = 0, key_blocks = 0, sum_blocks = 0;
  std::vector<double> chosen_host, sums_host;
  std::vector<unsigned> tally_host;
  std::vector<size_t> key_first_pt;  // [clouds + 1]: the points before each cloud, the total
  std::vector<ndt_plane_result> results;
};

// the buffers and the member table of a call (want_keys: the key launch follows)
ndt_status plane_plan_run(ndt_handle h, PlaneRun& R, bool want_keys) {
  hipStream_t st = h->stream;
  const size_t nc = R.clouds.size();
  const size_t H = static_cast<size_t>(R.P.n_hypotheses);
  const int cap = max_blocks_switch();
  R.rows = rows_switch();
  R.mem.host.assign(nc, PlaneMember{});
  R.key_first_pt.assign(nc + 1, 0);
  size_t total_pts = 0, partial_rows = 0;
  for (size_t k = 0; k < nc; k++) {
    PlaneMember& m = R.mem.host[k];
    const size_t n = R.clouds[k]->n;
    m.pts = R.clouds[k]->pts.p;
    m.n = static_cast<int>(n);
    ndt::plane_plan(n, R.P.n_hypotheses, cap, &m.tiles, &m.hyp_blocks, &m.tile_blocks);
    m.first_block = static_cast<int>(R.count_blocks);
    m.n_blocks = m.tile_blocks * m.hyp_blocks;
    R.count_blocks += m.n_blocks;
    int kb = 0, ppb = 0;
    if (n) ndt::select_plan(n, &kb, &ppb);
    m.key_first = static_cast<int>(R.key_blocks);
    m.key_blocks = kb;
    m.key_ppb = ppb;
    R.key_blocks += kb;
    int sb = 0, chunk = 0;
    if (n) ndt::plane_sum_plan(n, &sb, &chunk);
    m.sum_first = static_cast<int>(R.sum_blocks);
    m.sum_blocks = sb;
    m.sum_chunk = chunk;
    R.sum_blocks += sb;
    R.key_first_pt[k] = total_pts;
    total_pts += n;
    partial_rows += static_cast<size_t>(m.tile_blocks);
  }
  R.key_first_pt[nc] = total_pts;
  if (R.count_blocks > std::numeric_limits<int>::max()) return fail(NDT_ERR_INVALID, "too many points");
  HIP_TRY(R.d_models.reserve(nc * H * 4));
  HIP_TRY(R.d_states.reserve(nc * H));
  HIP_TRY(R.d_counts.reserve(nc * H));
  HIP_TRY(R.d_chosen.reserve(nc * kChosen));
  HIP_TRY(R.d_tally.reserve(nc * 2));
  if (R.rows) HIP_TRY(R.d_partials.reserve(std::max<size_t>(partial_rows * H, 1)));
  if (want_keys && !R.keys_override) HIP_TRY(R.d_keys.reserve(std::max<size_t>(total_pts, 1)));
  if (R.refine) HIP_TRY(R.d_sum_rows.reserve(std::max<size_t>(static_cast<size_t>(R.sum_blocks) * kSumRow, 1)));
  size_t rows_before = 0;
  for (size_t k = 0; k < nc; k++) {
    PlaneMember& m = R.mem.host[k];
    m.models = R.d_models.p + k * H * 4;
    m.states = R.d_states.p + k * H;
    m.counts = R.d_counts.p + k * H;
    m.partials = R.rows ? R.d_partials.p + rows_before * H : nullptr;
    m.chosen = R.d_chosen.p + k * kChosen;
    m.tally = R.d_tally.p + k * 2;
    m.keys = R.keys_override ? R.keys_override : (want_keys ? R.d_keys.p + R.key_first_pt[k] : nullptr);
    m.sum_rows = R.refine ? R.d_sum_rows.p + static_cast<size_t>(m.sum_first) * kSumRow : nullptr;
    rows_before += static_cast<size_t>(m.tile_blocks);
  }
  return R.mem.upload(st);
}

// models, counts, choice: queued on h's stream, nothing waited for
ndt_status plane_front(ndt_handle h, PlaneRun& R) {
  hipStream_t st = h->stream;
  const size_t nc = R.clouds.size();
  const size_t H = static_cast<size_t>(R.P.n_hypotheses);
  const unsigned model_blocks = static_cast<unsigned>((nc * H + 255) / 256);
  hipLaunchKernelGGL(k_plane_models, dim3(model_blocks), dim3(256), 0, st, R.mem.one(), R.mem.table(), R.mem.n(), R.P, R.d_triples);
  HIP_TRY(hipGetLastError());
  h->pl_launches++;
  if (!R.rows) HIP_TRY(hipMemsetAsync(R.d_counts.p, 0, nc * H * sizeof(unsigned), st));
  if (R.count_blocks) {
    hipLaunchKernelGGL(k_plane_counts, dim3(static_cast<unsigned>(R.count_blocks)), dim3(kBlock), 0, st, R.mem.one(), R.mem.table(), R.mem.n(),
                       R.P.n_hypotheses, R.P.T, R.rows ? 1 : 0);
    HIP_TRY(hipGetLastError());
    h->pl_launches++;
  }
  h->pl_count_blocks = static_cast<size_t>(R.count_blocks);
  hipLaunchKernelGGL(k_plane_best, dim3(static_cast<unsigned>(nc)), dim3(kBlock), 0, st, R.mem.one(), R.mem.table(), R.mem.n(), R.P, R.d_triples,
                     R.rows ? 1 : 0);
  HIP_TRY(hipGetLastError());
  h->pl_launches++;
  return NDT_OK;
}

ndt_status spec_checks(const ndt_plane_spec* spec) { return ndtc::spec_checks(spec, ndt::plane_spec_error); }

void diag_reset(ndt_handle h, size_t clouds) {
  h->pl_launches = h->pl_select_launches = h->pl_count_blocks = 0;
  h->pl_clouds = clouds;
}

// the caller's triples checked against the cloud (host), then copied up
ndt_status triples_checks(const int32_t* triples, int H, size_t n) {
  if (!triples) return NDT_OK;
  for (int i = 0; i < 3 * H; i++)
    if (triples[i] < 0 || static_cast<size_t>(triples[i]) >= n) return fail(NDT_ERR_INVALID, "a triple index lies outside the cloud");
  return NDT_OK;
}

// The segmentation of R.clouds: results, and (where asked for) the two output clouds of every input.
ndt_status segment_run(ndt_handle h, PlaneRun& R, ndt_cloud* inliers, ndt_cloud* others) {
  hipStream_t st = h->stream;
  const size_t nc = R.clouds.size();
  diag_reset(h, nc);
  R.results.assign(nc, ndt_plane_result{});
  Drain drain{st};
  SelDiagKeep keep(h);
  ndt_status s = plane_plan_run(h, R, true);
  if (!s) s = plane_front(h, R);
  if (s) return s;
  R.chosen_host.assign(nc * kChosen, 0.0);
  std::vector<char> refined(nc, 0);
  const bool sums_ran = R.refine && R.sum_blocks;
  if (sums_ran) {
    hipLaunchKernelGGL(k_plane_sums, dim3(static_cast<unsigned>(R.sum_blocks)), dim3(ndt::kPlaneSumBlock), 0, st, R.mem.one(), R.mem.table(), R.mem.n(),
                       R.P.T);
    HIP_TRY(hipGetLastError());
    h->pl_launches++;
    R.sums_host.assign(static_cast<size_t>(R.sum_blocks) * kSumRow, 0.0);
    HIP_TRY(hipMemcpyAsync(R.sums_host.data(), R.d_sum_rows.p, R.sums_host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(R.chosen_host.data(), R.d_chosen.p, nc * kChosen * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t k = 0; k < nc; k++) {
      double* row = &R.chosen_host[k * kChosen];
      if (row[0] == 0.0) continue;
      double S[kSumRow] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      const PlaneMember& m = R.mem.host[k];
      for (int b = 0; b < m.sum_blocks; b++)
        for (int j = 0; j < kSumRow; j++) S[j] += R.sums_host[static_cast<size_t>(m.sum_first + b) * kSumRow + j];
      double coeff[4];
      if (!ndt::plane_fit(R.P, S[0], S + 1, S + 4, row + 9, coeff, nullptr)) continue;
      refined[k] = 1;
      for (int j = 0; j < 4; j++) row[5 + j] = coeff[j];
      HIP_TRY(hipMemcpyAsync(R.d_chosen.p + k * kChosen + 5, row + 5, 4 * sizeof(double), hipMemcpyHostToDevice, st));
    }
  }
  R.tally_host.assign(nc * 2, 0u);
  HIP_TRY(hipMemsetAsync(R.d_tally.p, 0, nc * 2 * sizeof(unsigned), st));
  if (R.key_blocks) {
    hipLaunchKernelGGL(k_plane_keys, dim3(static_cast<unsigned>(R.key_blocks)), dim3(256), 0, st, R.mem.one(), R.mem.table(), R.mem.n(), R.P.T);
    HIP_TRY(hipGetLastError());
    h->pl_launches++;
  }
  // (without a refinement nothing has come back so far: the rows are read behind the last plane kernel, in one wait)
  if (!sums_ran) HIP_TRY(hipMemcpyAsync(R.chosen_host.data(), R.d_chosen.p, nc * kChosen * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(R.tally_host.data(), R.d_tally.p, nc * 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  // ---- the selections: the outputs of one kind are slices of one block
  ndt_cloud* outs[2] = {inliers, others};
  OutSlices slices[2];
  std::vector<SelJob> jobs[2];
  for (int v = 0; v < 2; v++) {
    if (!outs[v]) continue;
    ndt_select_spec sel{};
    sel.flags = v == 0 ? NDT_SELECT_KEY : (NDT_SELECT_KEY | NDT_SELECT_KEY_NEGATE | NDT_SELECT_FINITE);
    sel.key_lo = -R.P.T;
    sel.key_hi = R.P.T;
    if ((s = slices[v].reserve(h, R.key_first_pt))) return s;
    jobs[v].resize(nc);
    for (size_t k = 0; k < nc; k++) {
      jobs[v][k].in = R.clouds[k]->pts.p;
      jobs[v][k].n = R.clouds[k]->n;
      jobs[v][k].keys = R.d_keys.p + R.key_first_pt[k];
      jobs[v][k].out = slices[v].at(k);
      jobs[v][k].res = slices[v].cloud(k);
    }
    s = select_run(h, jobs[v], sel, nullptr);
    if (s) return s;
    h->pl_select_launches += h->sel_launches;
  }
  HIP_TRY(hipStreamSynchronize(st));
  for (size_t k = 0; k < nc; k++) {
    const double* row = &R.chosen_host[k * kChosen];
    ndt_plane_result& r = R.results[k];
    r.found = row[0] != 0.0 ? 1 : 0;
    r.refined = refined[k];
    for (int j = 0; j < 4; j++) r.coeff[j] = r.found ? row[5 + j] : 0.0;
    r.best = static_cast<int>(row[1]);
    r.best_count = static_cast<size_t>(row[2]);
    r.n_degenerate = static_cast<size_t>(row[3]);
    r.n_rejected = static_cast<size_t>(row[4]);
    r.n_inliers = R.tally_host[2 * k];
    r.n_finite = R.tally_host[2 * k + 1];
  }
  for (int v = 0; v < 2; v++) {
    if (!outs[v]) continue;
    for (size_t k = 0; k < nc; k++) outs[v][k] = slices[v].publish(k, jobs[v][k].kept);
  }
  return NDT_OK;
}

}  // namespace
}  // namespace ndtc

extern "C" {

ndt_status ndt_cloud_plane_counts(ndt_handle h, ndt_cloud in, const ndt_plane_spec* spec, const int32_t* triples, double* coeffs,
                                  int32_t* states, uint32_t* counts) {
  if (!h || !counts) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = cloud_entry(h, in, [&] {
    const ndt_status e = spec_checks(spec);
    return e ? e : triples_checks(triples, spec->n_hypotheses, in->c->n);
  });
  if (s) return s;
  hipStream_t st = h->stream;
  const size_t H = static_cast<size_t>(spec->n_hypotheses);
  PlaneRun R;
  R.clouds.push_back(in->c);
  R.P = ndt::plane_params(*spec);
  diag_reset(h, 1);
  Drain drain{st};
  DevBuf<int> d_tri;
  if (triples) {
    HIP_TRY(d_tri.reserve(3 * H));
    HIP_TRY(hipMemcpyAsync(d_tri.p, triples, 3 * H * sizeof(int), hipMemcpyHostToDevice, st));
    R.d_triples = d_tri.p;
  }
  s = plane_plan_run(h, R, false);
  if (!s) s = plane_front(h, R);
  if (s) return s;
  if (coeffs) HIP_TRY(hipMemcpyAsync(coeffs, R.d_models.p, H * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (states) HIP_TRY(hipMemcpyAsync(states, R.d_states.p, H * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(counts, R.d_counts.p, H * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return NDT_OK;
}

ndt_status ndt_cloud_segment_plane(ndt_handle h, ndt_cloud in, const ndt_plane_spec* spec, const int32_t* triples, ndt_plane_result* result,
                                   ndt_cloud* inliers, ndt_cloud* others) {
  if (inliers) *inliers = nullptr;
  if (others) *others = nullptr;
  if (!h || !result) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = cloud_entry(h, in, [&] {
    const ndt_status e = spec_checks(spec);
    return e ? e : triples_checks(triples, spec->n_hypotheses, in->c->n);
  });
  if (s) return s;
  PlaneRun R;
  R.clouds.push_back(in->c);
  R.P = ndt::plane_params(*spec);
  R.refine = spec->refine;
  DevBuf<int> d_tri;
  Drain drain{h->stream};
  if (triples) {
    const size_t H = static_cast<size_t>(spec->n_hypotheses);
    HIP_TRY(d_tri.reserve(3 * H));
    HIP_TRY(hipMemcpyAsync(d_tri.p, triples, 3 * H * sizeof(int), hipMemcpyHostToDevice, h->stream));
    R.d_triples = d_tri.p;
  }
  ndt_cloud out_in = nullptr, out_ot = nullptr;
  s = segment_run(h, R, inliers ? &out_in : nullptr, others ? &out_ot : nullptr);
  if (s) return s;
  *result = R.results[0];
  if (inliers) *inliers = out_in;
  if (others) *others = out_ot;
  return NDT_OK;
}

ndt_status ndt_cloud_segment_plane_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_plane_spec* spec,
                                          ndt_plane_result* results, ndt_cloud* inliers, ndt_cloud* others) {
  if (!h) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = clouds_begin(n_clouds, inliers, others);
  if (s) return s;
  if (n_clouds && (!in || !results)) return fail(NDT_ERR_INVALID, "null clouds or results");
  if ((s = spec_checks(spec))) return s;
  std::vector<size_t> first;
  if ((s = clouds_total(h, in, n_clouds, first))) return s;
  if (n_clouds == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  PlaneRun R;
  R.P = ndt::plane_params(*spec);
  R.refine = spec->refine;
  for (size_t k = 0; k < n_clouds; k++) {
    if ((s = cloud_use_on(h, in[k]->c.get()))) return s;
    R.clouds.push_back(in[k]->c);
  }
  std::vector<ndt_cloud> out_in(n_clouds, nullptr), out_ot(n_clouds, nullptr);
  s = segment_run(h, R, inliers ? out_in.data() : nullptr, others ? out_ot.data() : nullptr);
  if (s) return s;
  for (size_t k = 0; k < n_clouds; k++) {
    results[k] = R.results[k];
    if (inliers) inliers[k] = out_in[k];
    if (others) others[k] = out_ot[k];
  }
  return NDT_OK;
}

ndt_status ndt_cloud_plane_distances(ndt_handle h, ndt_cloud in, const double coeff[4], double* values, int values_on_device) {
  if (!h || !coeff || !values) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = cloud_entry(h, in, [&]() -> ndt_status {
    for (int k = 0; k < 4; k++)
      if (!std::isfinite(coeff[k])) return fail(NDT_ERR_INVALID, "the plane must be finite");
    if (coeff[0] == 0.0 && coeff[1] == 0.0 && coeff[2] == 0.0) return fail(NDT_ERR_INVALID, "the plane's normal must not be zero");
    return NDT_OK;
  });
  if (s) return s;
  hipStream_t st = h->stream;
  const size_t n = in->c->n;
  diag_reset(h, 1);
  if (n == 0) return NDT_OK;
  DoublesOut vals;
  DevBuf<double> d_row;
  if ((s = vals.reserve(values, n, values_on_device))) return s;
  HIP_TRY(d_row.reserve(kChosen));
  double row[kChosen] = {1.0, 0.0, 0.0, 0.0, 0.0, coeff[0], coeff[1], coeff[2], coeff[3]};
  PlaneMember m{};
  m.pts = in->c->pts.p;
  m.n = static_cast<int>(n);
  m.chosen = d_row.p;
  m.keys = vals.at();
  ndt::select_plan(n, &m.key_blocks, &m.key_ppb);
  Drain drain{st};
  HIP_TRY(hipMemcpyAsync(d_row.p, row, sizeof(row), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_plane_keys, dim3(static_cast<unsigned>(m.key_blocks)), dim3(256), 0, st, m, static_cast<const PlaneMember*>(nullptr), 1,
                     0.0);
  HIP_TRY(hipGetLastError());
  h->pl_launches = 1;
  if ((s = vals.fetch(st))) return s;
  HIP_TRY(hipStreamSynchronize(st));
  return NDT_OK;
}

ndt_status ndt_diag_plane(ndt_handle h, size_t* launches, size_t* select_launches, size_t* count_blocks, size_t* clouds) {
  if (!h || !launches || !select_launches || !count_blocks || !clouds) return fail(NDT_ERR_INVALID, "bad arguments");
  *launches = h->pl_launches;
  *select_launches = h->pl_select_launches;
  *count_blocks = h->pl_count_blocks;
  *clouds = h->pl_clouds;
  return NDT_OK;
}

ndt_status ndt_host_plane_spec_check(const ndt_plane_spec* spec) { return spec_checks(spec); }

ndt_status ndt_host_plane_sample(uint64_t seed, int hyp, size_t n_points, int32_t idx[3]) {
  if (!idx || hyp < 0 || n_points == 0) return fail(NDT_ERR_INVALID, "bad arguments");
  if (n_points > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  for (int j = 0; j < 3; j++) idx[j] = ndt::plane_sample(seed, hyp, j, static_cast<int>(n_points));
  return NDT_OK;
}

ndt_status ndt_host_plane_model(const ndt_plane_spec* spec, const float a[3], const float b[3], const float c[3], int same_index,
                                double coeff[4], int* state) {
  if (!a || !b || !c || !coeff || !state) return fail(NDT_ERR_INVALID, "bad arguments");
  if (ndt_status s = spec_checks(spec)) return s;
  const ndt::PlaneParams P = ndt::plane_params(*spec);
  *state = ndt::plane_model(P, a, b, c, same_index != 0, coeff);
  return NDT_OK;
}

ndt_status ndt_host_plane_distance(const double coeff[4], const float xyz[3], double* s) {
  if (!coeff || !xyz || !s) return fail(NDT_ERR_INVALID, "bad arguments");
  *s = ndt::plane_distance(coeff[0], coeff[1], coeff[2], coeff[3], static_cast<double>(xyz[0]), static_cast<double>(xyz[1]),
                           static_cast<double>(xyz[2]));
  return NDT_OK;
}

ndt_status ndt_host_plane_fit(const ndt_plane_spec* spec, double count, const double S1[3], const double S2[6], const double a[3],
                              double coeff[4], double* lambda, int* taken) {
  if (!S1 || !S2 || !a || !coeff || !taken) return fail(NDT_ERR_INVALID, "bad arguments");
  if (ndt_status s = spec_checks(spec)) return s;
  *taken = ndt::plane_fit(ndt::plane_params(*spec), count, S1, S2, a, coeff, lambda) ? 1 : 0;
  return NDT_OK;
}

ndt_status ndt_host_plane_plan(size_t n_points, int n_hypotheses, int* tile_points, int* hyp_per_block, int* tiles, int* hyp_blocks,
                               int* tile_blocks) {
  if (!tile_points || !hyp_per_block || !tiles || !hyp_blocks || !tile_blocks) return fail(NDT_ERR_INVALID, "bad arguments");
  if (n_points > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  if (n_hypotheses < 1 || n_hypotheses > ndt::kPlaneMaxHypotheses) return fail(NDT_ERR_INVALID, "n_hypotheses must be 1 ... 65536");
  *tile_points = ndt::kPlaneTile;
  *hyp_per_block = ndt::kPlaneBlock;
  ndt::plane_plan(n_points, n_hypotheses, ndtc::max_blocks_switch(), tiles, hyp_blocks, tile_blocks);
  return NDT_OK;
}

}  // extern "C"
