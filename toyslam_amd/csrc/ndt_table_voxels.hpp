// ndt_table_voxels.hpp -- the voxels of a target's look-up table that a predicate picks, enumerated in ASCENDING LINEAR INDEX:
// the centroid cloud (ndt_centroid_fitness.hip) and GICP's voxel set D (gicp_grid.hip) are both this pass.
//   Sel   a predicate on a table entry (a static `pick(e)`): which voxels are enumerated
//   Emit  a device functor (record, position, linear index): what one voxel writes
#pragma once
#include "ndt_internal.hpp"
#include "ndt_prims.hpp"
#include "ndt_voxel_table.hpp"

namespace ndt {

// the grid of one pass over a table (grid-stride kernels)
inline dim3 table_grid(long long entries) {
  return dim3(static_cast<unsigned>(std::max<long long>(1, std::min<long long>(4096, (entries + kBlock - 1) / kBlock))));
}

namespace {

// dense table: flag[t] = 1 where entry t is picked (flag has entries + 1 words, the last 0: its scan ends in the total)
template <class Sel>
__global__ __launch_bounds__(kBlock) void k_table_mark(GridView gv, long long entries, unsigned* __restrict__ flag) {
  for (long long t = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; t <= entries; t += static_cast<long long>(gridDim.x) * kBlock)
    flag[t] = (t < entries && Sel::pick(gv.lut[t])) ? 1u : 0u;
}
// ... and, the flags scanned in place: the voxel of entry t to position pos[t].  The padded table's order is the linear index's
// order (x fastest, then y, then z in both)
template <class Sel, class Emit>
__global__ __launch_bounds__(kBlock) void k_table_gather(GridView gv, long long entries, const unsigned* __restrict__ pos, Emit emit) {
  for (long long t = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; t < entries; t += static_cast<long long>(gridDim.x) * kBlock) {
    const int e = gv.lut[t];
    if (!Sel::pick(e)) continue;
    int x, y, z;
    table_cell(gv, t, x, y, z);
    emit(entry_record(e), pos[t],
         static_cast<long long>(x) * gv.g.mul[0] + static_cast<long long>(y) * gv.g.mul[1] + static_cast<long long>(z) * gv.g.mul[2]);
  }
}
// hash: every slot's (key, entry) for the sort -- a slot that is free, or not picked, gets the key 0xffffffff, which sorts behind
// every linear index -- and the count of the others
template <class Sel>
__global__ __launch_bounds__(kBlock) void k_table_mark_hash(GridView gv, long long entries, unsigned* __restrict__ keys, int* __restrict__ vals,
                                                            unsigned* __restrict__ count) {
  int n = 0;
  for (long long t = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; t < entries; t += static_cast<long long>(gridDim.x) * kBlock) {
    const int2 s = reinterpret_cast<const int2*>(gv.lut)[t];
    const bool picked = s.x != -1 && Sel::pick(s.y);
    keys[t] = picked ? static_cast<unsigned>(s.x) : 0xffffffffu;
    vals[t] = s.y;
    n += picked ? 1 : 0;
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) n += __shfl_xor(n, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && n) atomicAdd(count, static_cast<unsigned>(n));
}
template <class Emit>
__global__ __launch_bounds__(kBlock) void k_table_gather_sorted(const unsigned* __restrict__ keys, const int* __restrict__ vals, int n, Emit emit) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p < n) emit(entry_record(vals[p]), static_cast<unsigned>(p), static_cast<long long>(keys[p]));
}

}  // namespace
}  // namespace ndt

namespace ndtc {

// The voxels of g's table that Sel picks, *n of them, on `st`: mark, exclusive scan (dense) or sort by key (hash), the count
// read back, gather.  want == false: the count alone (the hash form does not sort, the dense form does not gather).  Otherwise
// reserve(count, emit) reserves the outputs once the count is known (and not 0) and fills the Emit object.  Nothing waits for
// the gather: the scratch goes back to the pool behind it, in stream order; a caller that reads the outputs on the host waits.
template <class Sel, class Emit, class Reserve>
ndt_status table_voxels(hipStream_t st, const DeviceGrid* g, bool want, Reserve&& reserve, size_t* n) {
  *n = 0;
  const long long entries = table_entries(g);
  const bool hash = g->geom.hash_bits != 0;
  if (hash && entries > std::numeric_limits<int>::max()) return fail(NDT_ERR_INVALID, "the voxel hash is too large to sort");
  if (!hash && entries + 1 > std::numeric_limits<int>::max()) return fail(NDT_ERR_INVALID, "the voxel table is too large to scan");
  const int words = static_cast<int>(hash ? entries : entries + 1);
  const ndt::GridView gv = g->view();
  const dim3 grid = ndt::table_grid(entries), block(ndt::kBlock);
  DevBuf<unsigned> keys_a, keys_b, count;  // (dense: keys_a holds the flags, scanned in place; its last word is the count)
  DevBuf<int> vals_a, vals_b;
  DevBuf<unsigned char> temp;
  HIP_TRY(keys_a.reserve(words));
  if (hash) {
    HIP_TRY(vals_a.reserve(words));
    HIP_TRY(count.reserve(1));
    HIP_TRY(hipMemsetAsync(count.p, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(ndt::k_table_mark_hash<Sel>, grid, block, 0, st, gv, entries, keys_a.p, vals_a.p, count.p);
    HIP_TRY(hipGetLastError());
    if (want) {
      const size_t tb = ndt::sort_pairs_temp_bytes(words, sizeof(unsigned));
      HIP_TRY(keys_b.reserve(words));
      HIP_TRY(vals_b.reserve(words));
      HIP_TRY(temp.reserve(tb));
      HIP_TRY(ndt::sort_pairs(keys_a.p, keys_b.p, vals_a.p, vals_b.p, words, 32, temp.p, tb, st));
    }
  } else {
    const size_t tb = ndt::exclusive_sum_temp_bytes(words);
    hipLaunchKernelGGL(ndt::k_table_mark<Sel>, grid, block, 0, st, gv, entries, keys_a.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(temp.reserve(tb));
    HIP_TRY(ndt::exclusive_sum(keys_a.p, keys_a.p, words, temp.p, tb, st));
  }
  unsigned cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, hash ? count.p : keys_a.p + entries, sizeof(cnt), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *n = cnt;
  if (!want || cnt == 0) return NDT_OK;
  Emit emit{};
  HIP_TRY(reserve(cnt, emit));
  if (hash)
    hipLaunchKernelGGL(ndt::k_table_gather_sorted<Emit>, dim3((cnt + ndt::kBlock - 1) / ndt::kBlock), block, 0, st, keys_b.p, vals_b.p,
                       static_cast<int>(cnt), emit);
  else
    hipLaunchKernelGGL((ndt::k_table_gather<Sel, Emit>), grid, block, 0, st, gv, entries, keys_a.p, emit);
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

}  // namespace ndtc
