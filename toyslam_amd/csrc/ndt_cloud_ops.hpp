// ndt_cloud_ops.hpp -- what the operations on resident clouds share (ndt_select.hip, ndt_deskew.hip, ndt_outliers.hip,
// ndt_plane.hip; their host side is ndt_cloud_ops.hip, declared in ndt_internal.hpp): the plan that cuts a cloud into ranges,
// and, for the kernels, a block's member and range, the two bounding boxes of a block and the fixed-order block sum.
#pragma once
#include <cstddef>

namespace ndt {

// A cloud of n items cut into ranges of one size: block b owns [b * per, min(n, (b + 1) * per)).  per is `least` until that
// would take more than max_blocks blocks, then n / max_blocks rounded up: monotone in n, and the blocks tile [0, n).
// n == 0: no block.  (select_plan, deskew_plan: a pass of the block's threads at least; outlier_stat_plan, plane_sum_plan: a
// chunk of values at least -- one rule.)
inline void range_plan(size_t n, int least, int max_blocks, int* blocks, int* per) {
  const size_t cap = static_cast<size_t>(max_blocks);
  const size_t share = (n + cap - 1) / cap;
  const size_t p = share > static_cast<size_t>(least) ? share : static_cast<size_t>(least);
  *per = static_cast<int>(p);
  *blocks = static_cast<int>((n + p - 1) / p);
}

}  // namespace ndt

#if defined(__HIPCC__)
#include <cfloat>

#include "ndt_device.hpp"

namespace ndt {

// The member a block works for.  A call of one member -- the usual one -- hands it over as the kernel argument `one`: no
// table to copy up first.  Otherwise the table entry member_at finds; first: the field that holds an entry's first block in
// THIS launch (the plane's member has three block ranges).
template <class M>
__device__ __forceinline__ M block_member(const M& one, const M* __restrict__ table, int n, int b, int M::*first) {
  return n == 1 ? one : table[member_at(n, b, [&](int i) { return table[i].*first; })];
}
// ... where the launch has one block (or one thread) per member: entry i
template <class M>
__device__ __forceinline__ M member_of(const M& one, const M* __restrict__ table, int n, int i) {
  return n == 1 ? one : table[i];
}

// local block lb of a member of n items cut into ranges of `per` (range_plan): where its range starts; returns its length
__device__ __forceinline__ int block_range(int lb, int per, int n, long long* start) {
  *start = static_cast<long long>(lb) * per;
  return static_cast<int>(min(static_cast<long long>(per), n - *start));
}

// The two bounding boxes of the records a block writes: box [0] per coordinate over the values that are not NaN (fminf /
// fmaxf drop a NaN operand), box [1] over the finite points.  A thread adds its records; to_lds() folds each wave
// into its row of the kernel's wave_box; behind the kernel's __syncthreads(), threads 0 ... 11 each take one float of the
// block's row from block_value(): [0..2] min and [3..5] max of box [0], [6..11] the same of box [1].
template <int WAVES>
struct TwoBox {
  float mn0[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx0[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  float mn1[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx1[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  __device__ __forceinline__ void add(const float4& p) {
    const float v[3] = {p.x, p.y, p.z};
    const bool fin = finite3(p);
#pragma unroll
    for (int a = 0; a < 3; a++) {
      mn0[a] = fminf(mn0[a], v[a]);
      mx0[a] = fmaxf(mx0[a], v[a]);
      mn1[a] = fin ? fminf(mn1[a], v[a]) : mn1[a];  // (a select, not a guarded store: the accumulator stays in registers)
      mx1[a] = fin ? fmaxf(mx1[a], v[a]) : mx1[a];
    }
  }
  __device__ __forceinline__ void to_lds(float (&wave_box)[WAVES][12]) const {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
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
  }
  static __device__ __forceinline__ float block_value(const float (&wave_box)[WAVES][12], int t) {
    const bool is_min = (t % 6) < 3;
    float v = wave_box[0][t];
    for (int w = 1; w < WAVES; w++) v = is_min ? fminf(v, wave_box[w][t]) : fmaxf(v, wave_box[w][t]);
    return v;
  }
};

// tree sum over the BLOCK threads of a block in a fixed order (sh: BLOCK doubles of LDS); the result in every thread
template <int BLOCK>
__device__ __forceinline__ double block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

}  // namespace ndt
#endif
