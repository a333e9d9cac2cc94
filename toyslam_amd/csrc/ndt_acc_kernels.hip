// ndt_acc_kernels.hip -- HIP kernels of the accumulating target and the launch functions over them (the radix sort and
// scan of ndt_prims.hpp included).  What each call queues, and in which order, is told where the host decides: ndt_accumulate.hip, ndt_acc_persist.hip
#include "ndt_acc.hpp"
#include "ndt_acc_device.hpp"
#include "ndt_prims.hpp"
#include "ndt_voxel_finish.hpp"

namespace ndt {
namespace {

constexpr int kAccTeam = 16;

// info: [0..2] min xyz, [3..5] max xyz (encoded), [6] range flag
__global__ __launch_bounds__(kBlock) void k_acc_keys(const float4* __restrict__ pts, int n, float inv_leaf, unsigned long long* __restrict__ keys,
                                                     int* __restrict__ vals, int* __restrict__ info) {
#pragma clang fp contract(off)
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  bool bad = false, any = false;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const float4 p = pts[i];
    unsigned long long key = kAccEmptyKey;
    if (finite3(p.x, p.y, p.z)) {
      // floor(x * inv_leaf), _impl.hpp:218-223 (f32; the product rounded before floor()); exact integers up to 2^24, so
      // within +-2^20 subtracting float(min_b) is exact too: the cell does not depend on the box
      const float fx = floorf(p.x * inv_leaf), fy = floorf(p.y * inv_leaf), fz = floorf(p.z * inv_leaf);
      const float lim = static_cast<float>(kAccCellBias);
      if (fx >= -lim && fx < lim && fy >= -lim && fy < lim && fz >= -lim && fz < lim) {
        key = acc_pack(static_cast<int>(fx), static_cast<int>(fy), static_cast<int>(fz));
      } else {
        bad = true;
      }
      any = true;
      mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
      mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
    }
    keys[i] = key;
    vals[i] = i;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    mn[k] = wave_min(mn[k]);
    mx[k] = wave_max(mx[k]);
  }
  const bool wave_any = __ballot(any) != 0, wave_bad = __ballot(bad) != 0;
  if ((threadIdx.x & (kWave - 1)) == 0 && wave_any) {
    for (int k = 0; k < 3; k++) {
      atomicMin(info + k, acc_encode(mn[k]));
      atomicMax(info + 3 + k, acc_encode(mx[k]));
    }
    if (wave_bad) atomicOr(info + 6, 1);
  }
}

// head flags of the runs of equal keys (unbinned points form no run); counts[0] = points binned
__global__ __launch_bounds__(kBlock) void k_acc_heads(const unsigned long long* __restrict__ keys, int n, unsigned* __restrict__ flags,
                                                      unsigned* __restrict__ counts) {
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
    const unsigned long long k = keys[j];
    const unsigned long long prev = j ? keys[j - 1] : kAccEmptyKey;
    flags[j] = (k != kAccEmptyKey && (j == 0 || k != prev)) ? 1u : 0u;
    if (k == kAccEmptyKey && (j == 0 || prev != kAccEmptyKey)) counts[0] = static_cast<unsigned>(j);
    if (j == n - 1 && k != kAccEmptyKey) counts[0] = static_cast<unsigned>(n);
  }
}

__device__ __forceinline__ void acc_insert(const AccView& v, unsigned long long key, int slot) {
  const unsigned mask = (1u << v.bits) - 1u;
  for (unsigned h = acc_hash(key, v.bits);; h = (h + 1u) & mask) {
    if (atomicCAS(v.keys + h, kAccEmptyKey, key) == kAccEmptyKey) {  // (keys are unique: one insert per voxel)
      v.vals[h] = slot;
      return;
    }
  }
}

// per run (ordinal = exclusive scan of the head flags): where it starts, the slot of its voxel (-1: new); counts[1] = runs
__global__ __launch_bounds__(kBlock) void k_acc_runs(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ flags,
                                                     const unsigned* __restrict__ ord, int n, AccView v, unsigned* __restrict__ run_start,
                                                     int* __restrict__ run_slot, unsigned* __restrict__ is_new, unsigned* __restrict__ counts) {
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
    if (flags[j]) {
      const unsigned r = ord[j];
      const int s = acc_find(v, keys[j]);
      run_start[r] = static_cast<unsigned>(j);
      run_slot[r] = s;
      is_new[r] = s < 0 ? 1u : 0u;
    }
    if (j == n - 1) counts[1] = ord[j] + flags[j];
  }
}
// counts[2] = new voxels (new_rank: exclusive scan of is_new over the runs)
__global__ void k_acc_new_total(const unsigned* __restrict__ is_new, const unsigned* __restrict__ new_rank, unsigned* __restrict__ counts) {
  const unsigned r = counts[1];
  counts[2] = r ? new_rank[r - 1] + is_new[r - 1] : 0u;
}

// capacity growth: every slot's cell into the (larger, empty) table
__global__ __launch_bounds__(kBlock) void k_acc_rehash(AccView v, int n_slots) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n_slots) return;
  const int4 c = v.cell[s];
  acc_insert(v, acc_pack(c.x, c.y, c.z), s);
}

__device__ __forceinline__ int acc_linear(const GridGeom& g, const int4& c) {
  return (c.x - g.min_b[0]) * g.mul[0] + (c.y - g.min_b[1]) * g.mul[1] + (c.z - g.min_b[2]) * g.mul[2];
}
__device__ __forceinline__ void acc_set_entry(int* __restrict__ lut, const GridGeom& geom, int cell, int entry) {
  if (geom.hash_bits) {
    int2* tab = reinterpret_cast<int2*>(lut);
    const unsigned mask = (1u << geom.hash_bits) - 1u;
    for (unsigned hslot = hash_slot(cell, geom.hash_bits);; hslot = (hslot + 1u) & mask) {
      const int seen = atomicCAS(&tab[hslot].x, -1, cell);
      if (seen == -1 || seen == cell) {
        tab[hslot].y = entry;
        break;
      }
    }
  } else {
    const int cz = cell / geom.mul[2], cy = (cell - cz * geom.mul[2]) / geom.mul[1], cx = cell - cz * geom.mul[2] - cy * geom.mul[1];
    const long long slot = static_cast<long long>(cx + kLutBorder) + static_cast<long long>(cy + kLutBorder) * geom.pmul[1] +
                           static_cast<long long>(cz + kLutBorder) * geom.pmul[2];
    lut[slot] = entry;
  }
}
// the box (or the table's form / size) changed: every slot's entry into the cleared table under the new geometry.  A voxel
// under min_pts has none (kLutEmpty, what the table was cleared to), a rejected one lut_rejected(r), a valid one its slot
__global__ __launch_bounds__(kBlock) void k_acc_relink(AccView v, int n_slots, GridGeom geom, int* __restrict__ lut) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n_slots) return;
  const int st = v.state[s];
  if (st == 0) return;
  acc_set_entry(lut, geom, acc_linear(geom, v.cell[s]), st == 1 ? s : lut_rejected(s));
}

// One team of 16 lanes per run: lane -> accumulator as K1's crowded cells (0-2 the mean sums, 3-8 the products xx xy xz yy yz
// zz, 9-11 the f32 centroid sums): twelve independent chains of strictly ordered additions, continued from the slot's sums.
__global__ __launch_bounds__(kBlock) void k_acc_merge(const float4* __restrict__ pts, const int* __restrict__ sorted_idx,
                                                      const unsigned long long* __restrict__ keys, const unsigned* __restrict__ run_start,
                                                      const int* __restrict__ run_slot, const unsigned* __restrict__ new_rank, int n_runs,
                                                      int n_binned, int n_slots_before, AccView v, int* __restrict__ touched) {
#pragma clang fp contract(off)
  const int tl = threadIdx.x & (kAccTeam - 1);
  const int r = (blockIdx.x * kBlock + threadIdx.x) / kAccTeam;
  if (r >= n_runs) return;
  const int beg = static_cast<int>(run_start[r]);
  const int end = (r + 1 < n_runs) ? static_cast<int>(run_start[r + 1]) : n_binned;
  int slot = run_slot[r];
  const bool fresh = slot < 0;
  if (fresh) slot = n_slots_before + static_cast<int>(new_rank[r]);
  const int ia = (tl < 3) ? tl : (tl < 6) ? 0 : (tl < 8) ? 1 : (tl == 8) ? 2 : (tl < 12) ? tl - 9 : 0;
  const int ib = (tl == 3) ? 0 : (tl == 4 || tl == 6) ? 1 : (tl == 5 || tl == 7 || tl == 8) ? 2 : -1;
  double acc = (tl == 3 || tl == 6 || tl == 8) ? 1.0 : 0.0;  // cov_ starts as Identity (voxel_grid_covariance_omp.h:107)
  float acc32 = 0.f;
  if (!fresh) {
    if (tl < 9) acc = v.sums[slot].d[tl];
    else if (tl < 12) acc32 = v.sums[slot].f[tl - 9];
  }
  auto pick = [](const float4& p, int q) { return q == 0 ? p.x : q == 1 ? p.y : q == 2 ? p.z : 1.0f; };  // (x * 1.0f is exact)
  int i = beg;
  for (; i + 4 <= end; i += 4) {
    float4 p[4];
#pragma unroll
    for (int u = 0; u < 4; u++) p[u] = pts[sorted_idx[i + u]];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const float a = pick(p[u], ia), b = pick(p[u], ib);
      const double prod = static_cast<double>(a) * static_cast<double>(b);
      acc += prod;
      acc32 += a;
    }
  }
  for (; i < end; i++) {
    const float4 p = pts[sorted_idx[i]];
    const float a = pick(p, ia), b = pick(p, ib);
    const double prod = static_cast<double>(a) * static_cast<double>(b);
    acc += prod;
    acc32 += a;
  }
  if (tl < 9) v.sums[slot].d[tl] = acc;
  else if (tl < 12) v.sums[slot].f[tl - 9] = acc32;
  if (tl == 15) {
    const unsigned long long key = keys[beg];
    int4 c;
    if (fresh) {
      acc_unpack(key, c.x, c.y, c.z);
      c.w = 0;
      v.state[slot] = 0;
      acc_insert(v, key, slot);
    } else {
      c = v.cell[slot];
    }
    c.w += end - beg;
    v.cell[slot] = c;
    touched[r] = slot;
  }
}

// a thread per listed slot (list == null: slot = ordinal): second pass of applyFilter from the slot's sums.  Dump mode writes the
// per-leaf outputs at the ordinal and leaves the slot's state alone (recs / cents / lut are then scratch)
__global__ __launch_bounds__(kBlock) void k_acc_finish(const int* __restrict__ list, int n_list, AccView v, int min_pts, double eig_ratio,
                                                       VoxelRec* __restrict__ recs, VoxelSide* __restrict__ cents, int* __restrict__ lut,
                                                       GridGeom geom, FinalizeDump dump, int* __restrict__ cell_out) {
#pragma clang fp contract(off)
  const int o = blockIdx.x * kBlock + threadIdx.x;
  if (o >= n_list) return;
  const int slot = list ? list[o] : o;
  const int4 c = v.cell[slot];
  const AccSums A = v.sums[slot];
  VoxelSums S;
  S.sx = A.d[0]; S.sy = A.d[1]; S.sz = A.d[2];
  S.cxx = A.d[3]; S.cxy = A.d[4]; S.cxz = A.d[5]; S.cyy = A.d[6]; S.cyz = A.d[7]; S.czz = A.d[8];
  S.fx = A.f[0]; S.fy = A.f[1]; S.fz = A.f[2];
  const int cell = acc_linear(geom, c);
  const bool valid = finish_voxel(S, c.w, o, slot, cell, min_pts, eig_ratio, recs, cents, lut, geom, dump);
  if (cell_out) cell_out[o] = cell;
  else v.state[slot] = c.w < min_pts ? 0 : valid ? 1 : 2;
}

// a thread per slot: its keep flag; kept slots, their points and their cell box reduced in the wave, then one atomic per
// wave and word (cells are exact floats: |cell| <= 2^20).  An export also wants the pairs its sort takes (sort_keys != null):
// the packed cell of a kept slot, kAccEmptyKey (sorts last) of any other, and the slot
__global__ __launch_bounds__(kBlock) void k_acc_crop_mark(const int4* __restrict__ cell, int n_slots, AccCropBox box, unsigned* __restrict__ keep,
                                                          int* __restrict__ info, unsigned long long* __restrict__ sort_keys,
                                                          int* __restrict__ sort_vals) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  bool kept = false;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  double pts = 0.0;
  if (s < n_slots) {
    const int4 c = cell[s];
    kept = c.x >= box.lo[0] && c.x <= box.hi[0] && c.y >= box.lo[1] && c.y <= box.hi[1] && c.z >= box.lo[2] && c.z <= box.hi[2];
    keep[s] = kept ? 1u : 0u;
    if (sort_keys) {
      sort_keys[s] = kept ? acc_pack(c.x, c.y, c.z) : kAccEmptyKey;
      sort_vals[s] = s;
    }
    if (kept) {
      mn[0] = mx[0] = static_cast<float>(c.x);
      mn[1] = mx[1] = static_cast<float>(c.y);
      mn[2] = mx[2] = static_cast<float>(c.z);
      pts = static_cast<double>(c.w);
    }
  }
  acc_mark_fold(kept, mn, mx, pts, info);
}

// every kept slot to its new number (the exclusive scan of the keep flags: kept slots keep their order) in fresh arrays.
// A record and its side sector hold the voxel's mean, inverse covariance, count and centroid -- nothing of the box or of
// the slot number -- so they are copied, not finished again
__global__ __launch_bounds__(kBlock) void k_acc_crop_compact(AccView from, int n_slots, const unsigned* __restrict__ keep,
                                                             const unsigned* __restrict__ number, int n_kept, int4* __restrict__ cell,
                                                             AccSums* __restrict__ sums, int* __restrict__ state, VoxelRec* __restrict__ recs,
                                                             VoxelSide* __restrict__ cents) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n_slots || !keep[s]) return;
  const int t = static_cast<int>(number[s]);
  if (t >= n_kept) return;  // (cannot happen: the scan numbers the kept slots 0 .. n_kept - 1)
  cell[t] = from.cell[s];
  sums[t] = from.sums[s];
  const int st = from.state[s];
  state[t] = st;
  if (st != 0) {  // a voxel under min_pts has no record yet
    const float4* rs = reinterpret_cast<const float4*>(from.recs + s);
    const float4* cs = reinterpret_cast<const float4*>(from.cents + s);
    float4* rd = reinterpret_cast<float4*>(recs + t);
    float4* cd = reinterpret_cast<float4*>(cents + t);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      rd[q] = rs[q];
      cd[q] = cs[q];
    }
  }
}

// a thread per row of the export: the slots in ascending key, as the sort left them; info[6] = rows (k_acc_crop_mark)
__global__ __launch_bounds__(kBlock) void k_acc_export_gather(AccView v, const int* __restrict__ sorted_slot, const int* __restrict__ info, int n_slots,
                                                              AccRow* __restrict__ rows) {
  const int o = blockIdx.x * kBlock + threadIdx.x;
  if (o >= n_slots || o >= info[6]) return;
  const int s = sorted_slot[o];
  const int4 c = v.cell[s];
  const AccSums A = v.sums[s];
  AccRow r;
  r.i = c.x; r.j = c.y; r.k = c.z; r.count = c.w;
#pragma unroll
  for (int q = 0; q < 9; q++) r.d[q] = A.d[q];
#pragma unroll
  for (int q = 0; q < 3; q++) r.f[q] = A.f[q];
  r.pad = 0.f;
  rows[o] = r;
}

// a thread per row of an import: its flags, the rows' cell box and the sum of their counts, reduced as k_acc_crop_mark does.
// info words as a crop's: [0..2] lowest cell, [3..5] highest cell, [6] flags (or), [8..9] points (64 bit)
__global__ __launch_bounds__(kBlock) void k_acc_import_check(const AccRow* __restrict__ rows, int n, AccCropBox box, AccView v, int* __restrict__ info) {
  const int o = blockIdx.x * kBlock + threadIdx.x;
  int flags = 0;
  bool inside = false;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  double pts = 0.0;
  if (o < n) {
    const AccRow r = rows[o];
    inside = r.i >= box.lo[0] && r.i <= box.hi[0] && r.j >= box.lo[1] && r.j <= box.hi[1] && r.k >= box.lo[2] && r.k <= box.hi[2];
    if (!inside) flags |= kAccRowOutside;
    if (r.count < 1) flags |= kAccRowCount;
    else pts = static_cast<double>(r.count);
    bool fin = isfinite(r.f[0]) && isfinite(r.f[1]) && isfinite(r.f[2]);
#pragma unroll
    for (int q = 0; q < 9; q++) fin = fin && isfinite(r.d[q]);
    if (!fin) flags |= kAccRowNonFinite;
    if (inside) {  // (the header's box lies within the lattice: the cell packs)
      const unsigned long long key = acc_pack(r.i, r.j, r.k);
      if (o > 0) {
        const AccRow p = rows[o - 1];
        const bool p_inside = p.i >= box.lo[0] && p.i <= box.hi[0] && p.j >= box.lo[1] && p.j <= box.hi[1] && p.k >= box.lo[2] && p.k <= box.hi[2];
        if (p_inside && acc_pack(p.i, p.j, p.k) >= key) flags |= kAccRowOrder;
      }
      if (acc_find(v, key) >= 0) flags |= kAccRowPresent;
      mn[0] = mx[0] = static_cast<float>(r.i);
      mn[1] = mx[1] = static_cast<float>(r.j);
      mn[2] = mx[2] = static_cast<float>(r.k);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    mn[k] = wave_min(mn[k]);
    mx[k] = wave_max(mx[k]);
  }
  pts = wave_sum(pts);  // (at most 64 x INT_MAX: exact)
  const unsigned long long mask = __ballot(inside);
  if (mask != 0 && (threadIdx.x & (kWave - 1)) == 0) {
    for (int k = 0; k < 3; k++) {
      atomicMin(info + k, static_cast<int>(mn[k]));
      atomicMax(info + 3 + k, static_cast<int>(mx[k]));
    }
  }
  if ((threadIdx.x & (kWave - 1)) == 0) atomicAdd(reinterpret_cast<unsigned long long*>(info + 8), static_cast<unsigned long long>(pts));
  if (flags) atomicOr(info + 6, flags);
}

// a thread per (checked) row: the voxel into slot n_slots_before + row -- cell, sums, "not finished yet", its key
__global__ __launch_bounds__(kBlock) void k_acc_import_place(const AccRow* __restrict__ rows, int n, int n_slots_before, AccView v,
                                                             int* __restrict__ touched) {
  const int o = blockIdx.x * kBlock + threadIdx.x;
  if (o >= n) return;
  const AccRow r = rows[o];
  const int slot = n_slots_before + o;
  AccSums A;
#pragma unroll
  for (int q = 0; q < 9; q++) A.d[q] = r.d[q];
#pragma unroll
  for (int q = 0; q < 3; q++) A.f[q] = r.f[q];
  A.pad = 0.f;
  v.cell[slot] = make_int4(r.i, r.j, r.k, r.count);
  v.sums[slot] = A;
  v.state[slot] = 0;
  acc_insert(v, acc_pack(r.i, r.j, r.k), slot);
  touched[o] = slot;
}

inline int acc_grid_for(size_t n, int cap) {
  const size_t b = (n + kBlock - 1) / kBlock;
  return static_cast<int>(std::max<size_t>(1, std::min<size_t>(b, static_cast<size_t>(cap))));
}

inline dim3 acc_blocks(size_t n) { return dim3(acc_grid_for(n, 1 << 30)); }

}  // namespace

hipError_t launch_acc_bin(const float4* posed, int n, float inv_leaf, const AccView& v, int* info, AccBins& b, hipStream_t st) {
  const size_t N = static_cast<size_t>(n);
  DevBuf<unsigned long long> keys_a;
  DevBuf<int> vals_a;
  DevBuf<unsigned char> temp;
  HIP_PASS(keys_a.reserve(N));
  HIP_PASS(b.keys.reserve(N));
  HIP_PASS(vals_a.reserve(N));
  HIP_PASS(b.sorted_idx.reserve(N));
  HIP_PASS(b.run_slot.reserve(N));
  HIP_PASS(b.w.reserve(5 * N));
  HIP_PASS(b.counts.reserve(4));
  unsigned *flags = b.w.p, *ord = b.w.p + N, *is_new = b.w.p + 3 * N;
  b.run_start = b.w.p + 2 * N;
  b.new_rank = b.w.p + 4 * N;
  const size_t tb = std::max(sort_pairs_temp_bytes(n, sizeof(unsigned long long)), exclusive_sum_temp_bytes(n));
  HIP_PASS(temp.reserve(tb));
  HIP_PASS(hipMemsetAsync(b.counts.p, 0, 4 * sizeof(unsigned), st));
  HIP_PASS(hipMemsetAsync(is_new, 0, N * sizeof(unsigned), st));
  hipLaunchKernelGGL(k_acc_keys, dim3(acc_grid_for(N, 2048)), dim3(kBlock), 0, st, posed, n, inv_leaf, keys_a.p, vals_a.p, info);
  HIP_PASS(sort_pairs(keys_a.p, b.keys.p, vals_a.p, b.sorted_idx.p, n, 64, temp.p, tb, st));
  hipLaunchKernelGGL(k_acc_heads, dim3(acc_grid_for(N, 2048)), dim3(kBlock), 0, st, b.keys.p, n, flags, b.counts.p);
  HIP_PASS(exclusive_sum(flags, ord, n, temp.p, tb, st));
  hipLaunchKernelGGL(k_acc_runs, dim3(acc_grid_for(N, 2048)), dim3(kBlock), 0, st, b.keys.p, flags, ord, n, v, b.run_start, b.run_slot.p, is_new, b.counts.p);
  HIP_PASS(exclusive_sum(is_new, b.new_rank, n, temp.p, tb, st));
  hipLaunchKernelGGL(k_acc_new_total, dim3(1), dim3(1), 0, st, is_new, b.new_rank, b.counts.p);
  return hipGetLastError();
}

hipError_t launch_acc_mark(const AccView& v, int n_slots, const AccCropBox& box, unsigned* keep, int* info, unsigned* number, AccRow* rows, hipStream_t st) {
  const size_t S = static_cast<size_t>(n_slots);
  DevBuf<unsigned long long> keys_a, keys_b;  // an export's (key, slot) pairs
  DevBuf<int> vals_a, vals_b;
  DevBuf<unsigned char> temp;
  size_t tb = 0;
  if (rows) {
    HIP_PASS(keys_a.reserve(S));
    HIP_PASS(keys_b.reserve(S));
    HIP_PASS(vals_a.reserve(S));
    HIP_PASS(vals_b.reserve(S));
    tb = sort_pairs_temp_bytes(n_slots, sizeof(unsigned long long));
  } else if (number) {
    tb = exclusive_sum_temp_bytes(n_slots);
  }
  if (rows || number) HIP_PASS(temp.reserve(tb));
  hipLaunchKernelGGL(k_acc_crop_mark, acc_blocks(S), dim3(kBlock), 0, st, v.cell, n_slots, box, keep, info, keys_a.p, vals_a.p);
  HIP_PASS(hipGetLastError());
  if (rows) {
    HIP_PASS(sort_pairs(keys_a.p, keys_b.p, vals_a.p, vals_b.p, n_slots, 64, temp.p, tb, st));
    hipLaunchKernelGGL(k_acc_export_gather, acc_blocks(S), dim3(kBlock), 0, st, v, vals_b.p, info, n_slots, rows);
  } else if (number) {
    HIP_PASS(exclusive_sum(keep, number, n_slots, temp.p, tb, st));
  }
  return hipGetLastError();
}

hipError_t launch_acc_rehash(const AccView& v, int n_slots, hipStream_t st) {
  hipLaunchKernelGGL(k_acc_rehash, acc_blocks(n_slots), dim3(kBlock), 0, st, v, n_slots);
  return hipGetLastError();
}
hipError_t launch_acc_relink(const AccView& v, int n_slots, const GridGeom& geo, int* lut, hipStream_t st) {
  hipLaunchKernelGGL(k_acc_relink, acc_blocks(n_slots), dim3(kBlock), 0, st, v, n_slots, geo, lut);
  return hipGetLastError();
}
hipError_t launch_acc_compact(const AccView& from, int n_slots, const unsigned* keep, const unsigned* number, int n_kept, const AccView& to, hipStream_t st) {
  hipLaunchKernelGGL(k_acc_crop_compact, acc_blocks(n_slots), dim3(kBlock), 0, st, from, n_slots, keep, number, n_kept, to.cell, to.sums, to.state, to.recs,
                     to.cents);
  return hipGetLastError();
}
hipError_t launch_acc_import_check(const AccRow* rows, int n, const AccCropBox& box, const AccView& v, int* info, hipStream_t st) {
  hipLaunchKernelGGL(k_acc_import_check, acc_blocks(n), dim3(kBlock), 0, st, rows, n, box, v, info);
  return hipGetLastError();
}

hipError_t launch_acc_extend(const AccPlan& p, int n_slots_before, ndtc::AccTarget* a, const GridGeom& geo, hipStream_t st) {
  const int n = p.n_touched;
  DevBuf<int> touched;  // the slot of every run / row: what the finish pass walks
  HIP_PASS(touched.reserve(static_cast<size_t>(n)));
  if (p.rows)
    hipLaunchKernelGGL(k_acc_import_place, acc_blocks(n), dim3(kBlock), 0, st, p.rows, n, n_slots_before, a->view(), touched.p);
  else
    hipLaunchKernelGGL(k_acc_merge, acc_blocks(static_cast<size_t>(n) * kAccTeam), dim3(kBlock), 0, st, p.posed, p.bins->sorted_idx.p, p.bins->keys.p,
                       p.bins->run_start, p.bins->run_slot.p, p.bins->new_rank, n, p.n_binned, n_slots_before, a->view(), touched.p);
  return launch_acc_finish(touched.p, n, a, a->grid->recs.p, a->grid->centroids.p, a->grid->lut.p, geo, FinalizeDump{}, nullptr, st);
}
// the listed slots finished into recs / cents / lut: the target's own, or the scratch of a dump (cell_out != null)
hipError_t launch_acc_finish(const int* order, int n, ndtc::AccTarget* a, VoxelRec* recs, VoxelSide* cents, int* lut, const GridGeom& geo, FinalizeDump dump,
                             int* cell_out, hipStream_t st) {
  hipLaunchKernelGGL(k_acc_finish, acc_blocks(n), dim3(kBlock), 0, st, order, n, a->view(), a->min_pts, a->eig_ratio, recs, cents, lut, geo, dump, cell_out);
  return hipGetLastError();
}

}  // namespace ndt
