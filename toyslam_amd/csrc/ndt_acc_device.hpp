// ndt_acc_device.hpp -- device building blocks the kernel units of the accumulating target share (ndt_acc_kernels.hip,
// ndt_acc_rays.hip): the key table's probe, and the fold of a keep-flag pass into a call's info block
#pragma once
#include "ndt_acc.hpp"
#include "ndt_device.hpp"

namespace ndt {

constexpr unsigned long long kAccEmptyKey = ~0ull;  // free table slot; also the key of a point that is not binned (sorts last)

__device__ __forceinline__ unsigned acc_hash(unsigned long long key, int bits) {
  return static_cast<unsigned>((key * 0x9E3779B97F4A7C15ull) >> (64 - bits));
}

__device__ __forceinline__ int acc_find(const AccView& v, unsigned long long key) {
  if (!v.keys) return -1;
  const unsigned mask = (1u << v.bits) - 1u;
  for (unsigned h = acc_hash(key, v.bits);; h = (h + 1u) & mask) {
    const unsigned long long seen = v.keys[h];
    if (seen == key) return v.vals[h];
    if (seen == kAccEmptyKey) return -1;
  }
}

// The tail of a keep-flag pass (a thread per slot): kept slots, their points and their cell box reduced in the wave, then one
// atomic per wave and word (cells are exact floats: |cell| <= 2^20).  mn / mx: the thread's cell if kept, else +-FLT_MAX;
// pts: its count if kept, else 0.  info words: kAccCropInfoWords
__device__ __forceinline__ void acc_mark_fold(bool kept, float* mn, float* mx, double pts, int* __restrict__ info) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    mn[k] = wave_min(mn[k]);
    mx[k] = wave_max(mx[k]);
  }
  pts = wave_sum(pts);  // (at most 64 x INT_MAX: exact)
  const unsigned long long mask = __ballot(kept);
  if ((threadIdx.x & (kWave - 1)) == 0 && mask != 0) {
    for (int k = 0; k < 3; k++) {
      atomicMin(info + k, static_cast<int>(mn[k]));
      atomicMax(info + 3 + k, static_cast<int>(mx[k]));
    }
    atomicAdd(info + 6, __popcll(mask));
    atomicAdd(reinterpret_cast<unsigned long long*>(info + 8), static_cast<unsigned long long>(pts));
  }
}

}  // namespace ndt
