// ndt_pairs_kernels.hip -- the lock-step evaluation step of ndt_align_pairs* (ndt_pairs.hip): every member of the step is
// evaluated against a voxel grid of its OWN (its pair's target), read from a per-member GridView table instead of the one
// GridView argument of k_derivatives / k_hessian64 / k_batch_step (ndt_kernels.hip, left as they are so that
// ndt_align_batch keeps its bits).  The bodies, the block layout (descs[m].pad blocks per member, one contiguous run of
// kBatchPointsPerBlock points per block, dealt to the XCDs by xcd_chunk) and the per-block rows are those of the batch
// kernels, so a member's sums are the ones ndt_align_batch would produce for that source against that target.
#define NDT_THROUGHPUT_UNIT 1  // same record-load form as ndt_kernels.hip (see derivatives_body)
#include "ndt_device.hpp"
#include "ndt_search.hpp"

namespace ndt {

namespace {

// KIND 0 / 1 / 2: every member of the launch wants that kind (the forms of k_derivatives<NNB, WANT_H, true> and
// k_hessian64<NNB, true>); KIND -1: kinds mixed, read per member (the form of k_batch_step).  NNB 27 = KDTREE.
template <int NNB, int KIND>
__global__ __launch_bounds__(kBlock) void k_pairs_step(const float4* __restrict__ src, const GridView* __restrict__ views,
                                                       const ScanDesc* __restrict__ descs, const int* __restrict__ active,
                                                       int max_blocks, double* __restrict__ partials) {
  __shared__ double lds[(kBlock / kWave) * 32];
  __shared__ EvalParams sP;
  __shared__ Hess64Params sP64;
  __shared__ PackedTables sT;
  const int member = active[blockIdx.y];
  const ScanDesc* dsc = descs + member;
  const int kind = KIND >= 0 ? KIND : dsc->kind;
  {
    const int* sp = (kind == 2) ? reinterpret_cast<const int*>(&dsc->P64) : reinterpret_cast<const int*>(&dsc->P);
    int* dp = (kind == 2) ? reinterpret_cast<int*>(&sP64) : reinterpret_cast<int*>(&sP);
    const int words = static_cast<int>(((kind == 2) ? sizeof(Hess64Params) : sizeof(EvalParams)) / 4);
    for (int t = threadIdx.x; t < words; t += kBlock) dp[t] = sp[t];
    if (kind != 2) pack_tables(dsc->P, sT, threadIdx.x, kBlock);
  }
  __syncthreads();
  // Block-uniform exit, taken by all waves together after the only barrier before block_reduce_store (whose barriers
  // the surviving blocks reach with every wave).
  if (static_cast<int>(blockIdx.x) >= dsc->pad) return;
  const GridView gv = views[member];  // (uniform: scalar loads)
  double acc[kNumAcc];
#pragma unroll
  for (int k = 0; k < kNumAcc; k++) acc[k] = 0.0;
  const int lo = xcd_chunk(blockIdx.x, dsc->pad) * kBatchPointsPerBlock;
  const int first = lo + static_cast<int>(threadIdx.x), stride = kBlock;
  const float4* pts = src + dsc->offset;
  const int n = min(dsc->count, lo + kBatchPointsPerBlock);
  if (KIND == 2) {
    hessian64_body<NNB>(pts, n, gv, sP64, first, stride, acc);
  } else if (KIND < 0 && kind == 2) {
    hessian64_body<NNB, true>(pts, n, gv, sP64, first, stride, acc);
  } else if (NNB == 27) {
    if (kind == 0) derivatives_body_kd<true>(pts, n, gv, sP, sT, first, stride, acc);
    else derivatives_body_kd<false>(pts, n, gv, sP, sT, first, stride, acc);
  } else {
    if (kind == 0) derivatives_body<NNB == 27 ? 7 : NNB, true>(pts, n, gv, sP, sT, first, stride, acc);
    else derivatives_body<NNB == 27 ? 7 : NNB, false>(pts, n, gv, sP, sT, first, stride, acc);
  }
  block_reduce_store<kNumAcc>(acc, partials + (static_cast<size_t>(member) * max_blocks + blockIdx.x) * kEvalStride, lds);
}

template <int NNB>
void launch_pairs_t(int kind, dim3 grid, const float4* src, const GridView* views, const ScanDesc* descs, const int* active,
                    int max_blocks, double* partials, hipStream_t stream) {
  const dim3 block(kBlock);
  if (kind == 0) hipLaunchKernelGGL((k_pairs_step<NNB, 0>), grid, block, 0, stream, src, views, descs, active, max_blocks, partials);
  else if (kind == 1) hipLaunchKernelGGL((k_pairs_step<NNB, 1>), grid, block, 0, stream, src, views, descs, active, max_blocks, partials);
  else if (kind == 2) hipLaunchKernelGGL((k_pairs_step<NNB, 2>), grid, block, 0, stream, src, views, descs, active, max_blocks, partials);
  else hipLaunchKernelGGL((k_pairs_step<NNB, -1>), grid, block, 0, stream, src, views, descs, active, max_blocks, partials);
}

}  // namespace

hipError_t launch_pairs_step(const float4* src, const GridView* views, int search, int kind, const ScanDesc* descs,
                             const int* active, int n_active, int max_blocks, int n_blocks, double* partials, hipStream_t stream) {
  if (n_active <= 0) return hipSuccess;
  const dim3 grid(n_blocks, n_active);
  // search: 0 = KDTREE, 1 = DIRECT26, 2 = DIRECT7 (and the reference's `default:`), 3 = DIRECT1
  if (search == 0) launch_pairs_t<27>(kind, grid, src, views, descs, active, max_blocks, partials, stream);
  else if (search == 1) launch_pairs_t<26>(kind, grid, src, views, descs, active, max_blocks, partials, stream);
  else if (search == 3) launch_pairs_t<1>(kind, grid, src, views, descs, active, max_blocks, partials, stream);
  else launch_pairs_t<7>(kind, grid, src, views, descs, active, max_blocks, partials, stream);
  return hipGetLastError();
}

}  // namespace ndt
