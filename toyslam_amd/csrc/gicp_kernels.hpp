// gicp_kernels.hpp -- launchers of the GICP kernels (gicp_kernels.hip), gfx950 only.
// GICP = pclomp::GeneralizedIterativeClosestPoint (reference ndt_omp/include/pclomp/gicp_omp.h,
// gicp_omp_impl.hpp), SURVEY 8(f) row N4.
#pragma once
#include <hip/hip_runtime.h>

#include "ndt_kernels.hpp"

namespace gicp {

using ndt::PointIndex;  // a cloud + the voxel index K1 built over it (ndt_kernels.hpp)

using ndt::launch_gather_points;

constexpr int kMaxK = 64;           // k_correspondences_ supported by the LDS candidate lists
constexpr int kFunctorValues = 14;  // f, g_t[3], R[9] (row-major), correspondence count
constexpr int kFunctorMaxBlocks = 1024;

// Blocks each of the four kernels gets for n points (queries of the two search kernels, source points of the functor and
// the server); max_blocks > 0 caps the grid below its own limit (NDT_GICP_MAX_BLOCKS).  The callers hand the result to the
// launchers below, and gicp_diag_plan reports it.
int knn_blocks(int n, int max_blocks);
int correspond_blocks(int n, int max_blocks);
int functor_blocks(int n, int max_blocks);
int server_blocks(int n, int max_blocks);

// computeCovariances (gicp_omp_impl.hpp:48-116): cov6[i] = xx,xy,xz,yy,yz,zz of the regularised
// covariance of point i.  nn_idx / nn_d2 (optional, [n][k]): the neighbours, ascending (distance, index).
hipError_t launch_knn_covariances(const PointIndex& ix, int k, double gicp_epsilon, int blocks, double* cov6, int* nn_idx,
                                  float* nn_d2, hipStream_t stream);

// The same for many clouds in one launch (k_knn_covariances_multi): member m is cloud ix, gets knn_blocks(ix.n, cap) blocks
// of its own -- n_blocks, the grid launch_knn_covariances would be given for it -- from first_block on, and writes cov6.
// d_members: the table in device memory, first_block ascending from 0 without gaps; n_blocks of the launch = their sum.
// Every member's cov6 is bit for bit what launch_knn_covariances(ix, k, eps, n_blocks, cov6, ...) writes.
struct KnnMember {
  PointIndex ix;
  double* cov6 = nullptr;
  int first_block = 0;
  int n_blocks = 0;
};
// Blocks one k_knn_covariances_multi launch carries at most; the members beyond go to a further launch (a member is never
// split: its blocks stride by its own count).  2^20 blocks of 8 queries are 8.4 M points per pass -- every sequence the
// callers hold today is one launch -- and 16 members of knn_blocks' own limit (65536); the grid's x dimension would allow
// 2^31, the bound is there so that one launch stays a bounded piece of work on a shared device.
constexpr int kKnnMultiMaxBlocks = 1 << 20;
hipError_t launch_knn_covariances_multi(const KnnMember* d_members, int n_members, int n_blocks, int k, double gicp_epsilon,
                                        hipStream_t stream);

// The finite check of many clouds in one launch (k_count_nonfinite_multi): counts[m] (zeroed by the caller) += the number of
// points of member m with a NaN or an infinity in x, y or z.  Member m owns finite_blocks(n) blocks from first_block on.
struct FiniteMember {
  const float4* pts = nullptr;
  int n = 0;
  int first_block = 0;
};
constexpr int kFinitePointsPerBlock = 2048;
int finite_blocks(int n);
hipError_t launch_count_nonfinite_multi(const FiniteMember* d_members, int n_members, int n_blocks, unsigned* counts,
                                        hipStream_t stream);

// One outer iteration's correspondence step (:405-456): query = T * output[i]; corr[i] = nearest target
// index if its squared distance < dist_threshold else -1; maha9[i] = (R C1 R^T + C2)^-1 as f32 (row-major).
struct Rot3d {
  double m[9];
};
hipError_t launch_correspond(const float4* output, int n, const float* T12, const Rot3d& R, const PointIndex& tgt,
                             const double* cov_src6, const double* cov_tgt6, double dist_threshold, int blocks, int* corr,
                             float* maha9, hipStream_t stream);

// OptimizationFunctorWithIndices (:241-368) over the current correspondences.  mode 0 = operator()
// (f32 quadratic form), 1 / 2 = df / fdf (f64), 3 = operator() in slot 0 together with df's gradient sums.  One launch: per-block rows -> ticket -> the last block
// sums them in a fixed order and publishes kFunctorValues raw sums as a tagged row (ndt_device.hpp
// publish_row_tagged) into pinned host memory.  counter: one zero-initialised u32, reset by the kernel.
hipError_t launch_functor(int mode, const float4* output, int n, const float4* tgt, const int* corr, const float* maha9,
                          const float* T12, int n_blocks, double* partials, unsigned* counter, double* out_row,
                          unsigned long long seq, hipStream_t stream);

// The lock-step of many registrations (gicp_align_pairs_lockstep, gicp_align_guesses): one k_correspond_multi launch for the
// members that asked for new correspondences and one k_functor_multi launch for every member waiting for an evaluation.
// LockstepMember: what a member keeps while it is in flight (slot = its place in the device table), uploaded once when it
// starts.  LockstepCorrespond / LockstepFunctor: one entry per member that takes part in a step, first_block ascending
// from 0 without gaps, uploaded every step.  A member's corr / maha9 are bit for bit what launch_correspond(.., n_blocks, ..)
// writes, and its row what launch_functor(mode, .., n_blocks, ..) publishes (the per-block bodies are shared).
struct LockstepMember {
  const float4* output = nullptr;  // the source moved by the guess
  const float4* tgt_pts = nullptr;
  const double* cov_src6 = nullptr;
  const double* cov_tgt6 = nullptr;
  int* corr = nullptr;
  float* maha9 = nullptr;
  double* partials = nullptr;   // its own rows: [n_blocks of the functor][kEvalStride]
  unsigned* counter = nullptr;  // its own ticket counter (zero between launches)
  double* out_row = nullptr;    // its own tagged row, pinned host memory
  PointIndex tgt;
  int n = 0;
  int pad = 0;
};
struct LockstepCorrespond {
  float T[12];
  Rot3d R;
  int slot = 0;
  int first_block = 0;
  int n_blocks = 0;  // correspond_blocks(n, cap)
  int pad = 0;
};
struct LockstepFunctor {
  float T[12];
  int slot = 0;
  int mode = 0;  // launch_functor's
  int first_block = 0;
  int n_blocks = 0;  // server_blocks(n, cap)
};
hipError_t launch_correspond_multi(const LockstepMember* d_members, const LockstepCorrespond* d_steps, int n_steps, int n_blocks,
                                   double dist_threshold, hipStream_t stream);
hipError_t launch_functor_multi(const LockstepMember* d_members, const LockstepFunctor* d_steps, int n_steps, int n_blocks,
                                unsigned long long seq, hipStream_t stream);

// Persistent objective server (one launch per BFGS run), see gicp_kernels.hip.  mailbox: 256 + 128 bytes of fine-grained
// device memory laid out like the NDT server's (the host posts with ndt::server_post: kind = functor mode 0 / 1 / 3, or
// ndt::kServerCmdExit); counter: kGicpServerParts * 32 zeroed u32; out_rows: kGicpServerParts tagged rows of pinned host memory.
constexpr int kGicpServerParts = 8;
hipError_t launch_server(const float4* output, int n, const float4* tgt, const int* corr, const float* maha9, void* mailbox,
                         int n_blocks, double* partials, unsigned* counter, double* out_rows, unsigned long long first_seq,
                         unsigned long long idle_ticks, hipStream_t stream);

}  // namespace gicp
