// gicp_kernels.hip -- HIP kernels of the GICP row, gfx950 / wave64 only.
//
//   k_knn_covariances  computeCovariances (gicp_omp_impl.hpp:48-116): exact k nearest neighbours of
//                      every point of a cloud among the cloud itself, the f64 covariance of those k
//                      points, its eigenvectors, and the regularised covariance (1, 1, epsilon).
//   k_knn_covariances_multi  the same for many clouds in one launch (gicp_align_pairs_clouds): a table of members, each
//                      with blocks of its own; one per-block body shared with k_knn_covariances.
//   k_count_nonfinite_multi  the finite check of many resident clouds in one launch.
//   k_correspond       per outer iteration (:419-456): nearest target point of every transformed
//                      source point, distance gate, Mahalanobis matrix (R C1 R^T + C2)^-1.
//   k_functor          the BFGS objective / gradient sums (:241-368), one fused launch per evaluation.
//   k_correspond_multi / k_functor_multi  the same two for the members of a lock-step (gicp_align_pairs_lockstep,
//                      gicp_align_guesses): a table of members, per-block bodies shared with the single kernels.
//
// All three are gather kernels over point sets that sit in L2 at the reference's sizes (tens of
// thousands of points after the 0.1 m prefilter, apps/align.cpp:60-69); nothing here is
// GEMM-shaped.  Nearest-neighbour search: the target's counting-sort voxel index (K1), cubic
// shells of cells around the query until the k-th best distance cannot be beaten by any unvisited
// shell -- exact, and with (distance, index) ordering deterministic.
#include "gicp_kernels.hpp"

#include "gicp_device.hpp"
#include "ndt_device.hpp"
#include "ndt_search.hpp"

namespace gicp {

using namespace ndt;

namespace {

constexpr int kKnnBlock = 64;   // one wave = 8 query teams per block
static_assert(kKnnBlock == kTeamsPerWave * kTeam, "team_knn: one wave per block");

// computeCovariances' neighbours (ndt_search.hpp team_knn): the k nearest in (distance, point index) order, the query --
// a point of the cloud -- among them
struct KnnOrdered {
  static constexpr bool kPositions = true, kDropSelf = false, kCountScans = false;
  static constexpr float kClear = 1.0f;
};

// The work of ONE block of a kNN / covariance grid, shared by k_knn_covariances (one cloud per launch) and
// k_knn_covariances_multi (many clouds per launch): block `block` of the `n_blocks` that cut cloud `ix`, eight queries per
// pass, strided by n_blocks.  Both kernels hand it the cloud and the block's place among the cloud's own blocks and nothing
// else, so a cloud's covariances are the same bits whichever kernel computed them.
__device__ __forceinline__ void knn_covariances_block(const PointIndex& ix, int k, double gicp_epsilon, int block, int n_blocks,
                                                      double* __restrict__ cov6, int* __restrict__ nn_idx,
                                                      float* __restrict__ nn_d2) {
#pragma clang fp contract(off)
  extern __shared__ unsigned char knn_lds[];
  const int sub = threadIdx.x & (kTeam - 1), team = threadIdx.x / kTeam;
  int* ordered = knn_row<int>(knn_lds, k, KnnOrdered::kPositions, team);  // [8][k] point indices, ascending (distance, index)
  const ShellLimits lim = shell_limits(ix);
  // The loop is uniform across the wave (a team without a query idles): the scan of the isolated queries is wave-wide.
  for (int base = block * kTeamsPerWave; base < ix.n; base += n_blocks * kTeamsPerWave) {
    const int i = base + team;  // uniform within a team
    const bool live = i < ix.n;
    const float4 q = live ? ix.pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int cnt = team_knn<KnnOrdered>(ix, lim, k, knn_lds, q, live, nullptr, [&](int rank, float d, int p) {
      const int idx = ix.sorted_idx[p];
      ordered[rank] = idx;
      if (nn_idx) {
        nn_idx[static_cast<size_t>(i) * k + rank] = idx;
        nn_d2[static_cast<size_t>(i) * k + rank] = d;
      }
    });
    if (!live) continue;
    if (nn_idx)
      for (int j = cnt + sub; j < k; j += kTeam) {  // (only a cloud smaller than k, which the host refuses)
        nn_idx[static_cast<size_t>(i) * k + j] = -1;
        nn_d2[static_cast<size_t>(i) * k + j] = INFINITY;
      }
    lds_fence();
    if (sub != 0) continue;  // the 3x3 algebra of a query is one lane's work
    // :81-105  f32 products, f64 sums, neighbours in ascending distance
    double mx = 0, my = 0, mz = 0, cxx = 0, cyx = 0, cyy = 0, czx = 0, czy = 0, czz = 0;
    auto add = [&](const float4& t) {
      mx += static_cast<double>(t.x);
      my += static_cast<double>(t.y);
      mz += static_cast<double>(t.z);
      cxx += static_cast<double>(t.x * t.x);
      cyx += static_cast<double>(t.y * t.x);
      cyy += static_cast<double>(t.y * t.y);
      czx += static_cast<double>(t.z * t.x);
      czy += static_cast<double>(t.z * t.y);
      czz += static_cast<double>(t.z * t.z);
    };
    auto fetch = [&](int j) { return ix.pts[min(max(ordered[j], 0), ix.n - 1)]; };
    int j = 0;
    for (; j + 4 <= cnt; j += 4) {  // four gathers in flight, added in order
      const float4 t0 = fetch(j), t1 = fetch(j + 1), t2 = fetch(j + 2), t3 = fetch(j + 3);
      add(t0);
      add(t1);
      add(t2);
      add(t3);
    }
    for (; j < cnt; j++) add(fetch(j));
    const double kd = static_cast<double>(k);
    mx /= kd;
    my /= kd;
    mz /= kd;
    double C[3][3];
    C[0][0] = cxx / kd - mx * mx;
    C[1][0] = cyx / kd - my * mx;
    C[1][1] = cyy / kd - my * my;
    C[2][0] = czx / kd - mz * mx;
    C[2][1] = czy / kd - mz * my;
    C[2][2] = czz / kd - mz * mz;
    C[0][1] = C[1][0];
    C[0][2] = C[2][0];
    C[1][2] = C[2][1];
    // :108-120  [Eigen] JacobiSVD of a symmetric matrix: U = eigenvectors ordered by |eigenvalue| descending
    double w[3], V[3][3];
    eig3_jacobi(C, w, V);
    int o0 = 2, o1 = 1, o2 = 0;  // eig3_jacobi: ascending eigenvalues
    if (fabs(w[o1]) > fabs(w[o0])) { const int t = o0; o0 = o1; o1 = t; }
    if (fabs(w[o2]) > fabs(w[o1])) { const int t = o1; o1 = o2; o2 = t; }
    if (fabs(w[o1]) > fabs(w[o0])) { const int t = o0; o0 = o1; o1 = t; }
    double out[6];
    int e = 0;
    for (int a = 0; a < 3; a++)
      for (int b = a; b < 3; b++) {
        double s = (1.0 * V[a][o0]) * V[b][o0];
        s += (1.0 * V[a][o1]) * V[b][o1];
        s += (gicp_epsilon * V[a][o2]) * V[b][o2];
        out[e++] = s;
      }
    for (int t = 0; t < 6; t++) cov6[static_cast<size_t>(i) * 6 + t] = out[t];
  }
}

__global__ __launch_bounds__(kKnnBlock) void k_knn_covariances(PointIndex ix, int k, double gicp_epsilon,
                                                               double* __restrict__ cov6, int* __restrict__ nn_idx,
                                                               float* __restrict__ nn_d2) {
  knn_covariances_block(ix, k, gicp_epsilon, static_cast<int>(blockIdx.x), static_cast<int>(gridDim.x), cov6, nn_idx, nn_d2);
}

// The covariances of MANY clouds from one launch (gicp_align_pairs_clouds).  members[m] owns the n_blocks consecutive blocks
// from first_block on (ascending, no gaps: member m + 1 starts where m ends, the grid is their sum); a block finds its
// member by bisection over first_block.  blockIdx.x and the table are the same for the whole wave, so the search and the
// copy of the member's PointIndex are scalar loads and scalar compares: no lane searches, nothing diverges.  From there on
// the block does what a block of k_knn_covariances does for that cloud alone (knn_covariances_block).
__global__ __launch_bounds__(kKnnBlock) void k_knn_covariances_multi(const KnnMember* __restrict__ members, int n_members, int k,
                                                                     double gicp_epsilon) {
  const int b = static_cast<int>(blockIdx.x);
  const int lo = member_at(n_members, b, [&](int m) { return members[m].first_block; });
  const PointIndex ix = members[lo].ix;
  const int local = b - members[lo].first_block, n_blocks = members[lo].n_blocks;
  if (local >= n_blocks) return;  // (a grid larger than the table's blocks: nothing to do)
  knn_covariances_block(ix, k, gicp_epsilon, local, n_blocks, members[lo].cov6, nullptr, nullptr);
}

// The finite check of many clouds in one launch: counts[m] += the points of member m with a NaN or an infinity among x, y, z.
// Member m owns the blocks from first_block on, kFinitePointsPerBlock points each; found as above.  counts zeroed before.
constexpr int kFiniteBlock = 256;
__global__ __launch_bounds__(kFiniteBlock) void k_count_nonfinite_multi(const FiniteMember* __restrict__ members, int n_members,
                                                                        unsigned* __restrict__ counts) {
  const int b = static_cast<int>(blockIdx.x);
  const int lo = member_at(n_members, b, [&](int m) { return members[m].first_block; });
  const float4* __restrict__ pts = members[lo].pts;
  const int n = members[lo].n;
  const long long first = static_cast<long long>(b - members[lo].first_block) * kFinitePointsPerBlock;
  unsigned bad = 0;
  for (int j = threadIdx.x; j < kFinitePointsPerBlock; j += kFiniteBlock) {
    const long long i = first + j;
    if (i >= n) break;
    const float4 p = pts[i];
    bad += (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) ? 0u : 1u;
  }
  const unsigned long long any = __ballot(bad != 0);
  if (any == 0) return;
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) bad += __shfl_xor(bad, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) atomicAdd(&counts[lo], bad);
}

// The work of ONE block of a correspondence grid, shared by k_correspond (one registration per launch) and
// k_correspond_multi (the members of a lock-step, gicp_align_pairs_lockstep): block `block` of the `n_blocks` that cut the
// n queries, 32 queries per pass, strided by n_blocks.  Both kernels hand it the member's arrays and the block's place
// among the member's own blocks and nothing else, so corr and maha9 are the same bits whichever kernel wrote them.
__device__ __forceinline__ void correspond_block(const float4* __restrict__ output, int n, const float* __restrict__ T12,
                                                 const Rot3d& R, const PointIndex& ix, const double* __restrict__ cov_src6,
                                                 const double* __restrict__ cov_tgt6, double dist_threshold, int block,
                                                 int n_blocks, int* __restrict__ corr, float* __restrict__ maha9) {
#pragma clang fp contract(off)
  constexpr int kTeams = kBlock / kTeam;
  const int sub = threadIdx.x & (kTeam - 1);
  const ShellLimits lim = shell_limits(ix);
  // The loop is uniform across the WAVE (a team without a query idles): the fallback below is a wave-wide operation.
  const int wave_in_block = threadIdx.x / kWave, team_in_wave = (threadIdx.x & (kWave - 1)) / kTeam;
  for (int base = (block * (kBlock / kWave) + wave_in_block) * kTeamsPerWave; base < n; base += n_blocks * kTeams) {
    const int i = base + team_in_wave;
    const bool live = i < n;  // uniform within a team
    float qx = 0.f, qy = 0.f, qz = 0.f;
    bool done = !live;
    float tb = INFINITY;  // the team's best
    int tb_i = 0x7fffffff;
    if (live) {
      const float4 p = output[i];
      matvec_eigen(T12, p.x, p.y, p.z, qx, qy, qz);
      float best = INFINITY;  // this lane's share: distance and POSITION in the cell order (the index behind it is
      int best_p = -1;        // looked up on ties and at the end of a shell only)
      auto consider = [&](float d, unsigned pos, bool ok) {
        if (ok && nearer(ix.sorted_idx, d, static_cast<int>(pos), best, best_p)) {
          best = d;
          best_p = static_cast<int>(pos);
        }
      };
      int ci, cj, ck;
      float margin;
      query_cell(ix.geom, qx, qy, qz, ci, cj, ck, margin);
      for (int r = 0; r <= lim.r_max && !done; r++) {
        team_shell(ix, ci, cj, ck, r, sub, qx, qy, qz, consider);
        tb = best;
        tb_i = best_p >= 0 ? ix.sorted_idx[best_p] : 0x7fffffff;
        team_min(tb, tb_i);
        const float reach = static_cast<float>(r) * lim.leaf + margin - ix.slack;
        if ((tb_i != 0x7fffffff && reach > 0.0f && tb < reach * reach) || r >= lim.r_lim) done = true;
        // nothing closer than the gate is left once the shells reach past it: no correspondence either way
        if (reach > 0.0f && static_cast<double>(reach) * static_cast<double>(reach) >= dist_threshold &&
            !(static_cast<double>(tb) < dist_threshold))
          done = true;
      }
    }
    // sparse neighbourhoods: the wave scans everything, one unfinished query at a time
    unsigned long long open_teams = __ballot(!done && sub == 0);
    while (open_teams) {
      const int src_lane = __builtin_ctzll(open_teams);
      open_teams &= open_teams - 1;
      float wd;
      int wi;
      wave_nearest(ix, __shfl(qx, src_lane, kWave), __shfl(qy, src_lane, kWave), __shfl(qz, src_lane, kWave), wd, wi);
      if (team_in_wave == src_lane / kTeam) {
        tb = wd;
        tb_i = wi;
      }
    }
    if (!live) continue;
    if (sub != 0) continue;
    int c_out = -1;
    if (tb_i != 0x7fffffff && static_cast<double>(tb) < dist_threshold) {  // :436
      mahalanobis_store(cov_src6 + static_cast<size_t>(i) * 6, cov_tgt6 + static_cast<size_t>(tb_i) * 6, R, maha9 + static_cast<size_t>(i) * 9);
      c_out = tb_i;
    }
    corr[i] = c_out;
  }
}

__global__ __launch_bounds__(kBlock) void k_correspond(const float4* __restrict__ output, int n, EvalParams P, Rot3d R,
                                                       PointIndex ix, const double* __restrict__ cov_src6,
                                                       const double* __restrict__ cov_tgt6, double dist_threshold,
                                                       int* __restrict__ corr, float* __restrict__ maha9) {
  correspond_block(output, n, P.T, R, ix, cov_src6, cov_tgt6, dist_threshold, static_cast<int>(blockIdx.x),
                   static_cast<int>(gridDim.x), corr, maha9);
}

// The correspondence steps of MANY registrations from one launch (the lock-step of gicp_align_pairs_lockstep and
// gicp_align_guesses).  steps[s] is one member that asked for new correspondences in this step: its transformation and
// rotation, its slot in the member table, and the n_blocks consecutive blocks from first_block on it owns (ascending, no
// gaps) -- correspond_blocks(n, cap) of them, the grid k_correspond gets for it alone.  A block finds its entry by
// bisection; blockIdx.x and both tables are the same for the whole wave, so the search and the member's pointers are
// scalar.  From there on the block does what a block of k_correspond does for that member (correspond_block).
__global__ __launch_bounds__(kBlock) void k_correspond_multi(const LockstepMember* __restrict__ members,
                                                             const LockstepCorrespond* __restrict__ steps, int n_steps,
                                                             double dist_threshold) {
  const int b = static_cast<int>(blockIdx.x);
  const int lo = member_at(n_steps, b, [&](int m) { return steps[m].first_block; });
  const LockstepCorrespond* __restrict__ st = steps + lo;
  const int local = b - st->first_block, n_blocks = st->n_blocks;
  if (local >= n_blocks) return;  // (a grid larger than the table's blocks: nothing to do)
  const LockstepMember* __restrict__ m = members + st->slot;
  const PointIndex ix = m->tgt;
  const Rot3d R = st->R;
  correspond_block(m->output, m->n, st->T, R, ix, m->cov_src6, m->cov_tgt6, dist_threshold, local, n_blocks, m->corr, m->maha9);
}

// MODE 0: operator() only; 1: df / fdf (f64); 2: operator() in slot 0 AND the f64 gradient sums of df in slots 1..12 --
// the line search asks for df right after operator() at the same point, and one launch serves both
//
// The work of ONE block of a functor grid, shared by k_functor (one evaluation per launch) and k_functor_multi (one
// evaluation of every waiting member of a lock-step per launch): block `block` of the `n_blocks` that cut the n source
// points, its row into partials[block], a ticket on `counter`, and the member's last block sums the n_blocks rows in the
// fixed order and publishes them into out_row.  Both kernels hand it the member's arrays, the block's place among the
// member's own blocks and their LDS and nothing else, so a member's row is the same bits whichever kernel summed it.
constexpr int kFunctorWaves = kBlock / kWave, kFunctorParts = kBlock / kEvalStride;
struct FunctorLds {
  double lds[kFunctorWaves * 32];
  double lds2[kFunctorParts * kEvalStride];
  int last;
};
template <int MODE>
__device__ __forceinline__ void functor_block(const float4* __restrict__ output, int n, const float4* __restrict__ tgt,
                                              const int* __restrict__ corr, const float* __restrict__ maha9,
                                              const float* __restrict__ T12, int block, int n_blocks,
                                              double* __restrict__ partials, unsigned* __restrict__ counter,
                                              double* __restrict__ out_row, unsigned long long seq, FunctorLds& sh) {
#pragma clang fp contract(off)
  constexpr int kWaves = kFunctorWaves, kParts = kFunctorParts;
  double* lds = sh.lds;
  double* lds2 = sh.lds2;
  double acc[kFunctorValues];
#pragma unroll
  for (int k = 0; k < kFunctorValues; k++) acc[k] = 0.0;
  for (int i = block * kBlock + threadIdx.x; i < n; i += n_blocks * kBlock) {
    const int c = corr[i];
    if (c < 0) continue;
    const float4 ps = output[i];
    const float4 pt = tgt[c];
    const float* M = maha9 + static_cast<size_t>(i) * 9;
    float px, py, pz;
    matvec_eigen(T12, ps.x, ps.y, ps.z, px, py, pz);
    const float r0 = px - pt.x, r1 = py - pt.y, r2 = pz - pt.z;
    if (MODE != 1) {  // operator(), :241-274
      const float m0 = (M[0] * r0 + M[1] * r1) + M[2] * r2;
      const float m1 = (M[3] * r0 + M[4] * r1) + M[5] * r2;
      const float m2 = (M[6] * r0 + M[7] * r1) + M[8] * r2;
      const float ret = (r0 * m0 + r2 * m2) + r1 * m1;  // [Eigen] 4-wide dot: (p0 + p2) + (p1 + p3)
      acc[0] += static_cast<double>(ret);
    }
    if (MODE != 0) {  // df / fdf, :277-368
      const double d0 = static_cast<double>(r0), d1 = static_cast<double>(r1), d2 = static_cast<double>(r2);
      const double t0 = (static_cast<double>(M[0]) * d0 + static_cast<double>(M[1]) * d1) + static_cast<double>(M[2]) * d2;
      const double t1 = (static_cast<double>(M[3]) * d0 + static_cast<double>(M[4]) * d1) + static_cast<double>(M[5]) * d2;
      const double t2 = (static_cast<double>(M[6]) * d0 + static_cast<double>(M[7]) * d1) + static_cast<double>(M[8]) * d2;
      if (MODE == 1) acc[0] += (d0 * t0 + d1 * t1) + d2 * t2;
      acc[1] += t0;
      acc[2] += t1;
      acc[3] += t2;
      const double sx = static_cast<double>(ps.x), sy = static_cast<double>(ps.y), sz = static_cast<double>(ps.z);
      acc[4] += sx * t0;
      acc[5] += sx * t1;
      acc[6] += sx * t2;
      acc[7] += sy * t0;
      acc[8] += sy * t1;
      acc[9] += sy * t2;
      acc[10] += sz * t0;
      acc[11] += sz * t1;
      acc[12] += sz * t2;
    }
    acc[13] += 1.0;
  }
  // block row -> ticket -> fixed-order sum by the last block -> tagged publication (as k_derivatives_fused)
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const double tot = wave_fold<kFunctorValues>(acc);
  if ((lane & 1) == 0) lds[wave * 32 + fold_index(lane)] = tot;
  __syncthreads();
  if (wave == 0) {
    if (lane < kEvalStride) {
      double v = 0.0;
      if (lane < kFunctorValues) {
        v = lds[lane];
#pragma unroll
        for (int w = 1; w < kWaves; w++) v += lds[w * 32 + lane];
      }
      __hip_atomic_store(partials + static_cast<size_t>(block) * kEvalStride + lane, v, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
      const unsigned ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sh.last = (ticket == static_cast<unsigned>(n_blocks) - 1u) ? 1 : 0;
    }
  }
  __syncthreads();
  if (!sh.last) return;
  const int k = threadIdx.x % kEvalStride, part = threadIdx.x / kEvalStride;
  lds2[part * kEvalStride + k] = sum_rows_fixed<kParts>(partials, n_blocks, threadIdx.x);
  __syncthreads();
  if (threadIdx.x < kEvalStride) {
    double t = 0.0;
#pragma unroll
    for (int p = 0; p < kParts; p++) t += lds2[p * kEvalStride + threadIdx.x];
    lds[threadIdx.x] = t;
    if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  publish_row_tagged(out_row, lds, threadIdx.x, seq);
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_functor(const float4* __restrict__ output, int n, const float4* __restrict__ tgt,
                                                    const int* __restrict__ corr, const float* __restrict__ maha9,
                                                    EvalParams P, double* __restrict__ partials,
                                                    unsigned* __restrict__ counter, double* __restrict__ out_row,
                                                    unsigned long long seq) {
  __shared__ FunctorLds sh;
  functor_block<MODE>(output, n, tgt, corr, maha9, P.T, static_cast<int>(blockIdx.x), static_cast<int>(gridDim.x), partials,
                      counter, out_row, seq, sh);
}

// One evaluation of EVERY waiting member of a lock-step from one launch.  steps[s] is one member blocked in an objective
// evaluation: its pose, its mode (0 operator(), 1 / 2 df / fdf, 3 operator() with df's sums -- launch_functor's numbering),
// its slot in the member table and the n_blocks blocks from first_block on it owns: server_blocks(n, cap) of them, the
// count the objective server of a single registration sums over, so the row is the server's row.  Found by bisection as in
// k_correspond_multi; the mode is the same for the whole block, a scalar branch onto k_functor's three bodies.  Every
// member has its own partial rows, ticket counter and tagged row in pinned host memory; all rows carry the step's seq.
__global__ __launch_bounds__(kBlock) void k_functor_multi(const LockstepMember* __restrict__ members,
                                                          const LockstepFunctor* __restrict__ steps, int n_steps,
                                                          unsigned long long seq) {
  __shared__ FunctorLds sh;
  const int b = static_cast<int>(blockIdx.x);
  const int lo = member_at(n_steps, b, [&](int m) { return steps[m].first_block; });
  const LockstepFunctor* __restrict__ st = steps + lo;
  const int local = b - st->first_block, n_blocks = st->n_blocks, mode = st->mode;
  if (local >= n_blocks) return;
  const LockstepMember* __restrict__ m = members + st->slot;
  if (mode == 0)
    functor_block<0>(m->output, m->n, m->tgt_pts, m->corr, m->maha9, st->T, local, n_blocks, m->partials, m->counter, m->out_row, seq, sh);
  else if (mode == 3)
    functor_block<2>(m->output, m->n, m->tgt_pts, m->corr, m->maha9, st->T, local, n_blocks, m->partials, m->counter, m->out_row, seq, sh);
  else
    functor_block<1>(m->output, m->n, m->tgt_pts, m->corr, m->maha9, st->T, local, n_blocks, m->partials, m->counter, m->out_row, seq, sh);
}

// ---------------------------------------------------------------------------
// Persistent objective server: ONE launch per BFGS run (the ~50 objective / gradient evaluations between two
// correspondence steps) instead of one launch per evaluation -- the protocol of the NDT evaluation server
// (ndt_latency.hip) with the direct mailbox: the host writes a 256-byte command (32 self-validating words: T[12], the
// mode) through the BAR into fine-grained device memory, every block reads it there, evaluates its slice of the
// correspondences, stores its partial row, takes a ticket on one of 8 shard counters (shard = part of k_functor's
// fixed-order sum), and a shard's last arriver publishes the part sum as a tagged row into pinned host memory; the host
// adds the 8 parts in order -- the same additions in the same order as k_functor's last block.
// Liveness: every spin is bounded by s_memrealtime budgets; block 0 tells the host when the server gives up.
// gridDim.x must not exceed the number of co-resident blocks (the launcher keeps it small).
// ---------------------------------------------------------------------------
constexpr int kGicpCmdWords = 32;
constexpr int kGicpCmdExit = 0x7fffffff;
struct GicpMailbox {  // layout of ndt_latency.hip's ServerMailbox (the host fills it with ndt::server_post)
  unsigned long long cmd[kGicpCmdWords];
  unsigned long long dead;
  unsigned long long pad[15];
};

__global__ __launch_bounds__(kBlock) void k_gicp_server(const float4* __restrict__ output, int n, const float4* __restrict__ tgt,
                                                        const int* __restrict__ corr, const float* __restrict__ maha9,
                                                        GicpMailbox* mb, double* __restrict__ partials,
                                                        unsigned* __restrict__ counter, double* __restrict__ out_rows,
                                                        unsigned long long first_seq, unsigned long long idle_ticks) {
#pragma clang fp contract(off)
  constexpr int kWaves = kBlock / kWave, kParts = kBlock / kEvalStride;  // 8 parts, as in k_functor
  static_assert(kParts == kGicpServerParts, "the host adds kGicpServerParts part sums");
  __shared__ double lds[kWaves * 32];
  __shared__ float sT[12];
  __shared__ int s_mode;
  unsigned long long expect = first_seq;
  for (;;) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    if (wave == 0) {
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      const unsigned long long patience = (blockIdx.x == 0) ? idle_ticks : 4 * idle_ticks;
      unsigned long long w = 0;
      bool got = false;
      for (;;) {
        if (lane < kGicpCmdWords) w = __hip_atomic_load(&mb->cmd[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else if (lane == kGicpCmdWords) w = __hip_atomic_load(&mb->dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (__ballot(lane >= kGicpCmdWords || static_cast<unsigned>(w) == static_cast<unsigned>(expect)) == ~0ull) { got = true; break; }
        if (__ballot(lane == kGicpCmdWords && w == expect) != 0) break;  // block 0 gave up on this very command: leave with it
        if (__builtin_amdgcn_s_memrealtime() - t0 > patience) break;
        __builtin_amdgcn_s_sleep(2);
      }
      if (!got && blockIdx.x == 0 && lane == 0) __hip_atomic_store(&mb->dead, expect, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      int mode = kGicpCmdExit;
      if (got) {
        const unsigned payload = static_cast<unsigned>(w >> 32);
        mode = static_cast<int>(__shfl(payload, 12, kWave));
        if (lane < 12) sT[lane] = __int_as_float(static_cast<int>(payload));
      }
      if (lane == 0) s_mode = mode;
    }
    __syncthreads();
    const int mode = s_mode;
    if (mode < 0 || mode > 3) return;  // EXIT, time-out or garbage: the whole block leaves together (0 f, 1 df, 2 fdf, 3 f + df)
    double acc[kFunctorValues];
#pragma unroll
    for (int k = 0; k < kFunctorValues; k++) acc[k] = 0.0;
    for (int i = blockIdx.x * kBlock + tid; i < n; i += gridDim.x * kBlock) {
      const int c = corr[i];
      if (c < 0) continue;
      const float4 ps = output[i];
      const float4 pt = tgt[c];
      const float* M = maha9 + static_cast<size_t>(i) * 9;
      float px, py, pz;
      matvec_eigen(sT, ps.x, ps.y, ps.z, px, py, pz);
      const float r0 = px - pt.x, r1 = py - pt.y, r2 = pz - pt.z;
      if (mode == 0 || mode == 3) {  // operator(), :241-274
        const float m0 = (M[0] * r0 + M[1] * r1) + M[2] * r2;
        const float m1 = (M[3] * r0 + M[4] * r1) + M[5] * r2;
        const float m2 = (M[6] * r0 + M[7] * r1) + M[8] * r2;
        const float ret = (r0 * m0 + r2 * m2) + r1 * m1;
        acc[0] += static_cast<double>(ret);
      }
      if (mode != 0) {  // df / fdf, :277-368
        const double d0 = static_cast<double>(r0), d1 = static_cast<double>(r1), d2 = static_cast<double>(r2);
        const double t0 = (static_cast<double>(M[0]) * d0 + static_cast<double>(M[1]) * d1) + static_cast<double>(M[2]) * d2;
        const double t1 = (static_cast<double>(M[3]) * d0 + static_cast<double>(M[4]) * d1) + static_cast<double>(M[5]) * d2;
        const double t2 = (static_cast<double>(M[6]) * d0 + static_cast<double>(M[7]) * d1) + static_cast<double>(M[8]) * d2;
        if (mode != 3) acc[0] += (d0 * t0 + d1 * t1) + d2 * t2;
        acc[1] += t0;
        acc[2] += t1;
        acc[3] += t2;
        const double sx = static_cast<double>(ps.x), sy = static_cast<double>(ps.y), sz = static_cast<double>(ps.z);
        acc[4] += sx * t0;
        acc[5] += sx * t1;
        acc[6] += sx * t2;
        acc[7] += sy * t0;
        acc[8] += sy * t1;
        acc[9] += sy * t2;
        acc[10] += sz * t0;
        acc[11] += sz * t1;
        acc[12] += sz * t2;
      }
      acc[13] += 1.0;
    }
    const double tot = wave_fold<kFunctorValues>(acc);
    if ((lane & 1) == 0) lds[wave * 32 + fold_index(lane)] = tot;
    __syncthreads();
    if (wave == 0) {
      if (lane < kEvalStride) {
        double v = 0.0;
        if (lane < kFunctorValues) {
          v = lds[lane];
#pragma unroll
          for (int w = 1; w < kWaves; w++) v += lds[w * 32 + lane];
        }
        __hip_atomic_store(partials + static_cast<size_t>(blockIdx.x) * kEvalStride + lane, v, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // the ticket's answer, the shard's part sum and its publication stay inside this wave (as in k_eval_server): no LDS
      // stage, no block barrier -- the other waves wait at the round's last barrier
      const unsigned round = static_cast<unsigned>(expect - first_seq);
      const unsigned shard = blockIdx.x % static_cast<unsigned>(kParts);
      const unsigned in_shard = (gridDim.x + static_cast<unsigned>(kParts) - 1u - shard) / static_cast<unsigned>(kParts);
      unsigned t1 = 0u;
      if (lane == 0) t1 = __hip_atomic_fetch_add(counter + 32u * shard, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__builtin_amdgcn_readfirstlane(t1) == (round + 1u) * in_shard - 1u) {
        const double part = (lane < kEvalStride) ? sum_rows_fixed<kParts>(partials, gridDim.x, static_cast<int>(shard) * kEvalStride + lane) : 0.0;
        publish_lanes_tagged(out_rows + static_cast<size_t>(shard) * kPubWords, part, lane, expect);
      }
    }
    __syncthreads();  // s_mode / lds are rewritten by the next round
    expect++;
  }
}

}  // namespace

// The four grids.  max_blocks > 0 caps a grid below its own limit (NDT_GICP_MAX_BLOCKS, a development switch: every kernel
// strides over what its grid does not cover, so the results do not depend on it).
static int grid_of(int n, int per_block, int limit, int max_blocks) {
  if (max_blocks > 0) limit = min(limit, max_blocks);
  return max(1, min(limit, (n + per_block - 1) / per_block));
}
int knn_blocks(int n, int max_blocks) { return grid_of(n, kKnnBlock / kTeam, 65536, max_blocks); }
int correspond_blocks(int n, int max_blocks) { return grid_of(n, kBlock / kTeam, 32768, max_blocks); }
int functor_blocks(int n, int max_blocks) { return grid_of(n, kBlock, kFunctorMaxBlocks, max_blocks); }
int server_blocks(int n, int max_blocks) { return grid_of(n, kBlock, 512, max_blocks); }

hipError_t launch_knn_covariances(const PointIndex& ix, int k, double gicp_epsilon, int blocks, double* cov6, int* nn_idx,
                                  float* nn_d2, hipStream_t stream) {
  if (k < 1 || k > kMaxK || blocks < 1) return hipErrorInvalidValue;
  const size_t lds = knn_lds_bytes<int>(k, KnnOrdered::kPositions);  // + per team: k ordered indices
  hipLaunchKernelGGL(k_knn_covariances, dim3(blocks), dim3(kKnnBlock), lds, stream, ix, k, gicp_epsilon, cov6, nn_idx, nn_d2);
  return hipGetLastError();
}

hipError_t launch_knn_covariances_multi(const KnnMember* d_members, int n_members, int n_blocks, int k, double gicp_epsilon,
                                        hipStream_t stream) {
  if (k < 1 || k > kMaxK || n_members < 1 || n_blocks < 1 || !d_members) return hipErrorInvalidValue;
  const size_t lds = knn_lds_bytes<int>(k, KnnOrdered::kPositions);  // as launch_knn_covariances: the same k for every member
  hipLaunchKernelGGL(k_knn_covariances_multi, dim3(n_blocks), dim3(kKnnBlock), lds, stream, d_members, n_members, k, gicp_epsilon);
  return hipGetLastError();
}

int finite_blocks(int n) { return max(1, (n + kFinitePointsPerBlock - 1) / kFinitePointsPerBlock); }

hipError_t launch_count_nonfinite_multi(const FiniteMember* d_members, int n_members, int n_blocks, unsigned* counts,
                                        hipStream_t stream) {
  if (n_members < 1 || n_blocks < 1 || !d_members || !counts) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_count_nonfinite_multi, dim3(n_blocks), dim3(kFiniteBlock), 0, stream, d_members, n_members, counts);
  return hipGetLastError();
}

hipError_t launch_correspond(const float4* output, int n, const float* T12, const Rot3d& R, const PointIndex& tgt,
                             const double* cov_src6, const double* cov_tgt6, double dist_threshold, int blocks, int* corr,
                             float* maha9, hipStream_t stream) {
  if (blocks < 1) return hipErrorInvalidValue;
  EvalParams P{};
  for (int i = 0; i < 12; i++) P.T[i] = T12[i];
  hipLaunchKernelGGL(k_correspond, dim3(blocks), dim3(kBlock), 0, stream, output, n, P, R, tgt, cov_src6, cov_tgt6,
                     dist_threshold, corr, maha9);
  return hipGetLastError();
}

hipError_t launch_functor(int mode, const float4* output, int n, const float4* tgt, const int* corr, const float* maha9,
                          const float* T12, int n_blocks, double* partials, unsigned* counter, double* out_row,
                          unsigned long long seq, hipStream_t stream) {
  EvalParams P{};
  for (int i = 0; i < 12; i++) P.T[i] = T12[i];
  if (mode == 0)
    hipLaunchKernelGGL(k_functor<0>, dim3(n_blocks), dim3(kBlock), 0, stream, output, n, tgt, corr, maha9, P, partials, counter,
                       out_row, seq);
  else if (mode == 3)
    hipLaunchKernelGGL(k_functor<2>, dim3(n_blocks), dim3(kBlock), 0, stream, output, n, tgt, corr, maha9, P, partials, counter,
                       out_row, seq);
  else
    hipLaunchKernelGGL(k_functor<1>, dim3(n_blocks), dim3(kBlock), 0, stream, output, n, tgt, corr, maha9, P, partials, counter,
                       out_row, seq);
  return hipGetLastError();
}

hipError_t launch_correspond_multi(const LockstepMember* d_members, const LockstepCorrespond* d_steps, int n_steps, int n_blocks,
                                   double dist_threshold, hipStream_t stream) {
  if (n_steps < 1 || n_blocks < 1 || !d_members || !d_steps) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_correspond_multi, dim3(n_blocks), dim3(kBlock), 0, stream, d_members, d_steps, n_steps, dist_threshold);
  return hipGetLastError();
}

hipError_t launch_functor_multi(const LockstepMember* d_members, const LockstepFunctor* d_steps, int n_steps, int n_blocks,
                                unsigned long long seq, hipStream_t stream) {
  if (n_steps < 1 || n_blocks < 1 || !d_members || !d_steps) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_functor_multi, dim3(n_blocks), dim3(kBlock), 0, stream, d_members, d_steps, n_steps, seq);
  return hipGetLastError();
}

hipError_t launch_server(const float4* output, int n, const float4* tgt, const int* corr, const float* maha9, void* mailbox,
                         int n_blocks, double* partials, unsigned* counter, double* out_rows, unsigned long long first_seq,
                         unsigned long long idle_ticks, hipStream_t stream) {
  if (ndt::server_mailbox_bytes() != sizeof(GicpMailbox)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gicp_server, dim3(n_blocks), dim3(kBlock), 0, stream, output, n, tgt, corr, maha9,
                     static_cast<GicpMailbox*>(mailbox), partials, counter, out_rows, first_seq, idle_ticks);
  return hipGetLastError();
}

}  // namespace gicp
