// ndt_acc_rays.hip -- the ray pass of ndt_target_accumulate_clear_rays / _ray_counts (the definition: include/ndt_mi355.h; the
// walk of one ray: ndt_rays.hpp) and the keep flags that follow it.  What a call queues around them is told where the host
// decides: ndt_accumulate.hip.
//   k_acc_rays       a thread per point of the call, all clouds in ONE launch (a point finds its cloud -- pose, sensor origin --
//                    by bisection of the clouds' first points; a call of one cloud takes it as a kernel argument).  The point
//                    is moved by its pose (N2's f32 transform), its build cell (k_acc_keys' arithmetic) looked up in the key
//                    table and that slot's hit flag set; then the ray is walked in f64, an acc_find per visited cell that lies
//                    in the target's cell box, +1 on the miss count of an occupied one -- the lanes of a wave that found the
//                    same slot at the same step add their number in ONE atomic (ray_count).  Integer counts: the result does
//                    not depend on the order.  No barrier: lanes leave the walk at different steps; the three totals (cast,
//                    skipped, visited) are folded in the wave after the loop, one 64-bit atomic per wave and word.
//   k_acc_rays_mark  k_acc_crop_mark with the predicate miss < min_rays || hit: the same fold into the info block
#include "ndt_acc.hpp"
#include "ndt_acc_device.hpp"
#include "ndt_prims.hpp"
#include "ndt_rays.hpp"

namespace ndt {
namespace {

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// +1 on miss[s] for every active lane with s >= 0.  kMerge: lanes of the wave that hold the same slot are merged into one
// atomic of their number (the voxels around the sensor are crossed by nearly every ray: a wave's lanes then share slots); the
// lanes that reach this point together are the ones whose walks are at the same step
template <bool kMerge>
__device__ __forceinline__ void ray_count(unsigned* __restrict__ miss, int s) {
  if (!kMerge) {
    if (s >= 0) atomicAdd(miss + s, 1u);
    return;
  }
  const int lane = threadIdx.x & (kWave - 1);
  unsigned long long todo = __ballot(s >= 0);
  while (todo) {
    const int leader = __ffsll(static_cast<long long>(todo)) - 1;
    const int ls = __shfl(s, leader, kWave);
    const unsigned long long same = __ballot(s == ls);
    if (lane == leader) atomicAdd(miss + ls, static_cast<unsigned>(__popcll(same)));
    todo &= ~same;
  }
}

template <bool kMerge>
__global__ __launch_bounds__(kRayBlock) void k_acc_rays(AccRayScan one, const AccRayScan* __restrict__ scans, int n_scans, int n_points, float inv_leaf,
                                                        double L, double margin, double min_range, double max_range, AccView v, AccCropBox box,
                                                        unsigned* __restrict__ miss, unsigned* __restrict__ hit,
                                                        unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  unsigned long long cast = 0, skipped = 0, visited = 0;
  const long long step = static_cast<long long>(gridDim.x) * kRayBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kRayBlock + threadIdx.x; i < n_points; i += step) {
    int c = 0;
    if (n_scans > 1) {  // the last cloud whose first point is not behind i (clouds are never empty)
      int hi = n_scans - 1;
      while (c < hi) {
        const int mid = (c + hi + 1) >> 1;
        if (scans[mid].first <= i) c = mid;
        else hi = mid - 1;
      }
    }
    const AccRayScan& S = n_scans > 1 ? scans[c] : one;
    const float4 pt = S.src[i - S.first];
    if (!finite3(pt.x, pt.y, pt.z)) continue;
    float p[3];
    xform_point(S.T, pt.x, pt.y, pt.z, p[0], p[1], p[2]);
    if (!finite3(p[0], p[1], p[2])) continue;
    // the build cell: floor(x * inv_leaf) in f32 as k_acc_keys bins a point; outside the lattice: no hit, no ray
    const float fx = floorf(p[0] * inv_leaf), fy = floorf(p[1] * inv_leaf), fz = floorf(p[2] * inv_leaf);
    const float lim = static_cast<float>(kAccCellBias);
    if (!(fx >= -lim && fx < lim && fy >= -lim && fy < lim && fz >= -lim && fz < lim)) {
      skipped++;
      continue;
    }
    const int own = acc_find(v, acc_pack(static_cast<int>(fx), static_cast<int>(fy), static_cast<int>(fz)));
    if (own >= 0) hit[own] = 1u;
    const float o[3] = {S.o[0], S.o[1], S.o[2]};
    const long long cells = ray_walk(o, p, L, margin, min_range, max_range, nullptr, [&](int ci, int cj, int ck) {
      const bool in_box = ci >= box.lo[0] && ci <= box.hi[0] && cj >= box.lo[1] && cj <= box.hi[1] && ck >= box.lo[2] && ck <= box.hi[2];
      ray_count<kMerge>(miss, in_box ? acc_find(v, acc_pack(ci, cj, ck)) : -1);
    });
    if (cells < 0) {
      skipped++;
    } else {
      cast++;
      visited += static_cast<unsigned long long>(cells);
    }
  }
  cast = wave_sum_u64(cast);
  skipped = wave_sum_u64(skipped);
  visited = wave_sum_u64(visited);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (cast) atomicAdd(counters + 0, cast);
    if (skipped) atomicAdd(counters + 1, skipped);
    if (visited) atomicAdd(counters + 2, visited);
  }
}

__global__ __launch_bounds__(kBlock) void k_acc_rays_mark(const int4* __restrict__ cell, int n_slots, const unsigned* __restrict__ miss,
                                                          const unsigned* __restrict__ hit, unsigned min_rays, unsigned* __restrict__ keep,
                                                          int* __restrict__ info) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  bool kept = false, seen = false;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  double pts = 0.0;
  if (s < n_slots) {
    const int4 c = cell[s];
    const unsigned m = miss[s];
    seen = m >= 1u;
    kept = m < min_rays || hit[s] != 0u;
    keep[s] = kept ? 1u : 0u;
    if (kept) {
      mn[0] = mx[0] = static_cast<float>(c.x);
      mn[1] = mx[1] = static_cast<float>(c.y);
      mn[2] = mx[2] = static_cast<float>(c.z);
      pts = static_cast<double>(c.w);
    }
  }
  const unsigned long long seen_mask = __ballot(seen);
  if ((threadIdx.x & (kWave - 1)) == 0 && seen_mask != 0) atomicAdd(info + 7, __popcll(seen_mask));
  acc_mark_fold(kept, mn, mx, pts, info);
}

}  // namespace

hipError_t launch_acc_rays(const AccRayScan& one, const AccRayScan* d_scans, int n_scans, int n_points, int blocks, float resolution,
                           const ndt_ray_spec& spec, const AccView& v, const AccCropBox& box, unsigned* miss, unsigned* hit,
                           unsigned long long* counters, hipStream_t st) {
  // development switch, read per call: NDT_RAYS_MERGE=0 = an atomic per lane instead of the wave-level merge of equal slots
  // (measured: tools/time_clear_rays.py, NOTES.md; the counts do not depend on it)
  const char* e = getenv("NDT_RAYS_MERGE");
  const auto kernel = (e && atoi(e) == 0) ? k_acc_rays<false> : k_acc_rays<true>;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kRayBlock), 0, st, one, d_scans, n_scans, n_points, 1.0f / resolution,
                     static_cast<double>(resolution), static_cast<double>(spec.margin), static_cast<double>(spec.min_range),
                     static_cast<double>(spec.max_range), v, box, miss, hit, counters);
  return hipGetLastError();
}

hipError_t launch_acc_rays_mark(const AccView& v, int n_slots, const unsigned* miss, const unsigned* hit, int min_rays, unsigned* keep, int* info,
                                unsigned* number, hipStream_t st) {
  ndtc::DevBuf<unsigned char> temp;
  const size_t tb = exclusive_sum_temp_bytes(n_slots);
  HIP_PASS(temp.reserve(tb));
  const int blocks = std::max(1, (n_slots + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_acc_rays_mark, dim3(blocks), dim3(kBlock), 0, st, v.cell, n_slots, miss, hit, static_cast<unsigned>(min_rays), keep, info);
  HIP_PASS(hipGetLastError());
  HIP_PASS(exclusive_sum(keep, number, n_slots, temp.p, tb, st));
  return hipGetLastError();
}

}  // namespace ndt
