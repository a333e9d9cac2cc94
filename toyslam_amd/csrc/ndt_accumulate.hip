// ndt_accumulate.hip -- the ACCUMULATING target (ndt_target_accumulate*): posed scans merged into the voxel grid, the
// registration target of a mapping run, in memory O(voxels) instead of O(points of the run).
//
// applyFilter's first pass is a set of running sums per voxel (VoxelSums: f64 sums seeded with the identity, f32 centroid
// sums, points added in index order) and its second pass (finish_voxel) reads nothing but those sums and the count.  The
// reference's cell of a point is floor(x * inv_leaf) on an ABSOLUTE lattice; the bounding box only shifts the linear index.
// So a voxel's sums can be kept and continued -- scan 1's points added after scan 0's round exactly like one pass over
// [scan 0 | scan 1] -- and a grown box changes keys, not contents: the accumulated grid is, leaf for leaf and bit for bit,
// the grid K1 builds from the concatenation of the posed scans.
//
// State per voxel SLOT (record ordinal = slot): absolute cell (i, j, k) and count, the running sums, the finished VoxelRec /
// VoxelSide, and what the look-up table says about it (under min_pts / valid / rejected).  An open-addressing table keyed by
// the packed absolute cell (3 x 21 bits) maps a cell to its slot.  One update:
//   k_transform_multi   the clouds moved by their poses (N2's device code), one launch
//   k_acc_keys          packed cell of every posed point, the range test, the bounding box of the finite ones
//   radix sort          stable sort of (key, point index) -- hipCUB, as ndt_sparse.hip
//   k_acc_heads / scan / k_acc_runs   run heads, one run per voxel; its slot if the voxel exists; new voxels numbered by
//                       a scan over the runs (slot = slots so far + rank among the new runs: the same numbering every time)
//   ---- one read-back: runs, new voxels, box, range flag; the host decides refusals, growth, geometry, dense / sparse ----
//   k_acc_rehash / copies   capacity growth (table doubled and re-inserted, slot arrays doubled and copied)
//   k_acc_relink        only when the box (or the table form / size) changed: every slot's entry rewritten
//   k_acc_merge         a team of 16 lanes per run, a lane per accumulator (K1's form for crowded cells): insert the voxel if
//                       new, continue its sums over the run in ascending point index
//   k_acc_finish        a thread per touched voxel: finish_voxel -> record, centroid, table entry
// The evaluation kernels see an ordinary GridView: the padded dense table or the hash keyed by the reference's linear index.
//
// One crop to a box of cells (ndt_target_accumulate_crop) -- over the slots, never over points:
//   k_acc_crop_mark     a thread per slot: keep flag from its cell; kept slots, their points and their cell box
//   scan                new slot numbers (kept slots keep their order)
//   ---- one read-back: kept slots, kept points, cell box; nothing removed -> return; the host derives geometry, form, capacities ----
//   k_acc_crop_compact  kept slots into FRESH arrays (cell, sums, state, record, side sector: none depends on box or slot)
//   k_acc_rehash / k_acc_relink   the cleared key table and the cleared look-up table from the kept slots
#include <hipcub/hipcub.hpp>
#include <unistd.h>

#include <cerrno>

#include "ndt_acc_blob.hpp"
#include "ndt_internal.hpp"
#include "ndt_voxel_finish.hpp"

namespace ndt {
namespace {

constexpr unsigned long long kAccEmptyKey = ~0ull;  // free table slot; also the key of a point that is not binned (sorts last)
constexpr int kAccCellBias = 1 << 20;               // cells of [-2^20, 2^20) on every axis
constexpr int kAccTeam = 16;

struct AccSums {  // VoxelSums as an array: d = sx sy sz cxx cxy cxz cyy cyz czz, f = the f32 centroid sums
  double d[9];
  float f[3];
  float pad;
};

struct AccView {
  unsigned long long* keys;  // [2^bits] packed absolute cell, kAccEmptyKey = free
  int* vals;                 // [2^bits] slot
  int bits;
  int4* cell;      // per slot: absolute cell i, j, k; count
  AccSums* sums;   // per slot
  int* state;      // per slot: 0 under min_pts, 1 valid, 2 rejected
  VoxelRec* recs;  // per slot
  VoxelSide* cents;
};

__host__ __device__ inline unsigned long long acc_pack(int i, int j, int k) {
  return (static_cast<unsigned long long>(k + kAccCellBias) << 42) | (static_cast<unsigned long long>(j + kAccCellBias) << 21) |
         static_cast<unsigned long long>(i + kAccCellBias);
}
__host__ __device__ inline void acc_unpack(unsigned long long key, int& i, int& j, int& k) {
  i = static_cast<int>(key & 0x1fffffull) - kAccCellBias;
  j = static_cast<int>((key >> 21) & 0x1fffffull) - kAccCellBias;
  k = static_cast<int>((key >> 42) & 0x1fffffull) - kAccCellBias;
}
__device__ __forceinline__ unsigned acc_hash(unsigned long long key, int bits) {
  return static_cast<unsigned>((key * 0x9E3779B97F4A7C15ull) >> (64 - bits));
}
// order-preserving int code of a float (atomicMin / atomicMax over floats of either sign)
__host__ __device__ inline int acc_encode(float v) {
  int b;
#if defined(__HIP_DEVICE_COMPILE__)
  b = __float_as_int(v);
#else
  std::memcpy(&b, &v, sizeof(b));
#endif
  return b ^ ((b >> 31) & 0x7fffffff);
}
inline float acc_decode(int c) {
  const int b = c ^ ((c >> 31) & 0x7fffffff);
  float v;
  std::memcpy(&v, &b, sizeof(v));
  return v;
}

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

__device__ __forceinline__ int acc_find(const AccView& v, unsigned long long key) {
  if (!v.keys) return -1;
  const unsigned mask = (1u << v.bits) - 1u;
  for (unsigned h = acc_hash(key, v.bits);; h = (h + 1u) & mask) {
    const unsigned long long seen = v.keys[h];
    if (seen == key) return v.vals[h];
    if (seen == kAccEmptyKey) return -1;
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

// ---- crop to a box of cells (ndt_target_accumulate_crop): over the slots, never over points
struct AccCropBox {
  int lo[3], hi[3];  // kept: lo <= cell <= hi on every axis
};
// info words of a crop: [0..2] lowest kept cell, [3..5] highest kept cell, [6] kept slots, [8..9] kept points (64 bit)
constexpr int kAccCropInfoWords = 10;

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

// ---- export / import (ndt_target_accumulate_export / _import): a voxel leaves or enters as its cell, count and sums
struct AccRow {  // a row of the blob (include/ndt_mi355.h)
  int i, j, k, count;
  double d[9];
  float f[3];
  float pad;
};
static_assert(sizeof(AccRow) == ndtc::kAccBlobRowBytes, "a blob row is 104 bytes");

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

// what is wrong with a row (info[6] of an import check)
constexpr int kAccRowOutside = 1, kAccRowCount = 2, kAccRowNonFinite = 4, kAccRowOrder = 8, kAccRowPresent = 16;

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

}  // namespace
}  // namespace ndt

namespace ndtc {

// the accumulated target of a handle (h->acc): alive while h->grid is its grid -- any call that gives the handle another
// grid (ndt_set_input_target*, ndt_share_input_target, ndt_promote_source_to_target) thereby replaces it
struct AccTarget {
  std::shared_ptr<DeviceGrid> grid;  // what the evaluation paths see: lut, recs, centroids, geometry
  float resolution = 0;
  int min_pts = 6;
  double eig_ratio = 0.01;
  size_t n_points = 0, n_updates = 0;
  int n_slots = 0, slot_cap = 0, bits = 0;
  int first_bits = 0, first_cap = 0;  // the capacities a target starts with: what a crop shrinks back towards
  DevBuf<unsigned long long> keys;
  DevBuf<int> vals;
  DevBuf<int4> cell;
  DevBuf<ndt::AccSums> sums;
  DevBuf<int> state;
  bool have_box = false;
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
  bool sparse = false;
  ndt::AccView view() {
    return ndt::AccView{keys.p, vals.p, bits, cell.p, sums.p, state.p, grid->recs.p, grid->centroids.p};
  }
};

namespace {

int env_int(const char* name, int dflt, int lo, int hi) {
  const char* v = getenv(name);
  return v ? std::max(lo, std::min(hi, atoi(v))) : dflt;
}

AccTarget* acc_live(ndt_context* h) { return (h->acc && h->grid && h->acc->grid == h->grid) ? h->acc.get() : nullptr; }

struct AccScan {
  std::shared_ptr<DeviceCloud> c;
  const float* pose = nullptr;
};

// the lattice of the accumulated box (lattice_geometry: what a cloud's grid gets) and its padded table
ndt_status acc_geometry(float resolution, const float* min_p, const float* max_p, ndt::GridGeom& geo) {
  const ndt::LatticeStatus ls = ndt::lattice_geometry(resolution, min_p, max_p, geo);
  if (ls == ndt::kLatticeIndexOverflow)
    return fail(NDT_ERR_GRID_OVERFLOW, "leaf size is too small for the accumulated target: integer indices would overflow");
  if (ls != ndt::kLatticeOk) return fail(NDT_ERR_GRID_OVERFLOW, "voxel grid too large");
  ndt::set_padded_lut(geo);
  return NDT_OK;
}

// slot arrays at least `want` slots, the key table at most half full with `want` voxels: doubled, copied / re-inserted
ndt_status acc_grow(ndt_context* h, AccTarget* a, int want, bool* grown) {
  hipStream_t st = h->stream;
  DeviceGrid* g = a->grid.get();
  if (want > a->slot_cap) {
    int cap = std::max(a->slot_cap, 1);
    while (cap < want) cap *= 2;
    DevBuf<int4> cell;
    DevBuf<ndt::AccSums> sums;
    DevBuf<int> state;
    DevBuf<ndt::VoxelRec> recs;
    DevBuf<ndt::VoxelSide> cents;
    HIP_TRY(cell.reserve(cap));
    HIP_TRY(sums.reserve(cap));
    HIP_TRY(state.reserve(cap));
    HIP_TRY(recs.reserve(cap));
    HIP_TRY(cents.reserve(cap));
    if (a->n_slots) {
      const size_t m = static_cast<size_t>(a->n_slots);
      HIP_TRY(hipMemcpyAsync(cell.p, a->cell.p, m * sizeof(int4), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(sums.p, a->sums.p, m * sizeof(ndt::AccSums), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(state.p, a->state.p, m * sizeof(int), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(recs.p, g->recs.p, m * sizeof(ndt::VoxelRec), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(cents.p, g->centroids.p, m * sizeof(ndt::VoxelSide), hipMemcpyDeviceToDevice, st));
      *grown = true;
    }
    a->cell.swap(cell);  // (the old arrays go back to the pool at scope exit: reused only behind these copies, stream order)
    a->sums.swap(sums);
    a->state.swap(state);
    g->recs.swap(recs);
    g->centroids.swap(cents);
    a->slot_cap = cap;
  }
  if (!a->keys.p || 2 * static_cast<size_t>(want) > (static_cast<size_t>(1) << a->bits)) {
    int bits = std::max(a->bits, 2);
    while (2 * static_cast<size_t>(want) > (static_cast<size_t>(1) << bits)) bits++;
    DevBuf<unsigned long long> keys;
    DevBuf<int> vals;
    const size_t cap = static_cast<size_t>(1) << bits;
    HIP_TRY(keys.reserve(cap));
    HIP_TRY(vals.reserve(cap));
    HIP_TRY(hipMemsetAsync(keys.p, 0xFF, cap * sizeof(unsigned long long), st));
    a->keys.swap(keys);
    a->vals.swap(vals);
    a->bits = bits;
    if (a->n_slots) {
      hipLaunchKernelGGL(ndt::k_acc_rehash, dim3(ndt::acc_grid_for(a->n_slots, 1 << 30)), dim3(ndt::kBlock), 0, st, a->view(), a->n_slots);
      h->acc_launches++;
      *grown = true;
    }
  }
  return NDT_OK;
}

// a target starts: the handle's parameters captured, nothing of its previous target continued.  It becomes the handle's
// (acc_adopt) only once the call that starts it can no longer be refused
std::shared_ptr<AccTarget> acc_start(ndt_context* h) {
  auto started = std::make_shared<AccTarget>();
  AccTarget* a = started.get();
  a->resolution = h->resolution;
  a->min_pts = h->min_pts;
  a->eig_ratio = h->eig_ratio;
  a->bits = a->first_bits = env_int("NDT_ACC_HASH_BITS", 16, 2, 30);
  a->first_cap = env_int("NDT_ACC_SLOTS", 1 << 15, 1, 1 << 30);
  a->slot_cap = 0;
  a->grid = std::make_shared<DeviceGrid>();
  a->grid->accumulated = true;
  a->grid->resolution = a->resolution;
  a->grid->min_pts = a->min_pts;
  a->grid->eig_ratio = a->eig_ratio;
  for (int k = 0; k < 3; k++) {
    a->grid->geom.leaf[k] = a->resolution;
    a->grid->geom.inv_leaf[k] = 1.0f / a->resolution;
  }
  return started;
}
void acc_adopt(ndt_context* h, const std::shared_ptr<AccTarget>& started) {
  h->acc = started;
  h->grid = started->grid;
  auto holder = std::make_shared<DeviceCloud>();  // the handle "has a target"; its points are not kept
  h->target = holder;
  h->target_dense = 0;
}

// the table the evaluation kernels read, under the geometry `geo` of the box [mn, mx]: relinked only when the box, its form
// or its size changed.  The slots before this call are entered again; the call's own voxels follow through k_acc_finish
ndt_status acc_settle_table(ndt_context* h, AccTarget* a, ndt::GridGeom& geo, bool sparse, const float* mn, const float* mx, int n_slots_before) {
  hipStream_t st = h->stream;
  DeviceGrid* g = a->grid.get();
  bool relink = !a->have_box || sparse != a->sparse || std::memcmp(geo.min_b, g->geom.min_b, sizeof(geo.min_b)) != 0 ||
                std::memcmp(geo.max_b, g->geom.max_b, sizeof(geo.max_b)) != 0;
  int hash_bits = 0;
  if (sparse) {
    hash_bits = 10;
    while ((static_cast<size_t>(1) << hash_bits) < 2 * static_cast<size_t>(a->slot_cap)) hash_bits++;
    if (hash_bits != g->geom.hash_bits) relink = true;
  }
  geo.hash_bits = hash_bits;
  if (relink) {
    const size_t words = sparse ? (static_cast<size_t>(2) << hash_bits) : static_cast<size_t>(geo.lut_cells);
    DevBuf<int> lut;
    HIP_TRY(lut.reserve(words));
    HIP_TRY(hipMemsetAsync(lut.p, 0xFF, words * sizeof(int), st));  // kLutEmpty / free hash slots
    g->lut.swap(lut);
    if (n_slots_before) {
      hipLaunchKernelGGL(ndt::k_acc_relink, dim3(ndt::acc_grid_for(n_slots_before, 1 << 30)), dim3(ndt::kBlock), 0, st, a->view(), n_slots_before, geo, g->lut.p);
      h->acc_launches++;
      h->acc_relinked = a->have_box ? 1 : 0;
    }
  }
  g->geom = geo;
  a->sparse = sparse;
  a->have_box = true;
  for (int k = 0; k < 3; k++) {
    a->mn[k] = mn[k];
    a->mx[k] = mx[k];
  }
  return NDT_OK;
}

ndt_status acc_update(ndt_context* h, const std::vector<AccScan>& scans, size_t total) {
  static const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  hipStream_t st = h->stream;
  const int n = static_cast<int>(total);
  h->acc_touched = h->acc_new = h->acc_launches = 0;
  h->acc_relinked = h->acc_grown = 0;
  AccTarget* a = acc_live(h);
  std::shared_ptr<AccTarget> started;
  if (!a) {  // a target starts: parameters captured, nothing of the handle's previous target is continued
    started = acc_start(h);
    a = started.get();
  }
  DeviceGrid* g = a->grid.get();
  const float inv_leaf = 1.0f / a->resolution;

  // ---- the posed points (N2's transform, one launch for all clouds) and their keys
  DevBuf<float4> posed;
  DevBuf<unsigned long long> keys_a, keys_b;
  DevBuf<int> vals_a, sorted_idx, run_slot, touched, info;
  DevBuf<unsigned> w;  // flags, ord, run_start, is_new, new_rank
  DevBuf<unsigned> counts;
  DevBuf<unsigned char> temp, d_desc;
  const size_t N = static_cast<size_t>(n);
  HIP_TRY(posed.reserve(N));
  {
    std::vector<ndt::TransformScan> d;
    std::vector<int> starts;
    size_t first = 0;
    long long blocks = 0;
    for (const AccScan& sc : scans) {
      const size_t m = sc.c->n;
      if (!m) continue;
      ndt::TransformScan t{};
      t.src = sc.c->pts.p;
      t.n = static_cast<int>(m);
      t.first = static_cast<int>(first);
      t.dense = 0;  // transformPointCloud of a cloud that is not dense: a non-finite row stays as it is (and is not binned)
      colmajor_to_T12(sc.pose ? sc.pose : I, t.T);
      d.push_back(t);
      starts.push_back(static_cast<int>(blocks));
      blocks += ndt::transform_multi_blocks(m);
      first += m;
    }
    starts.push_back(static_cast<int>(blocks));
    const size_t desc_bytes = d.size() * sizeof(ndt::TransformScan), bytes = desc_bytes + starts.size() * sizeof(int);
    std::vector<unsigned char> stage(bytes);
    std::memcpy(stage.data(), d.data(), desc_bytes);
    std::memcpy(stage.data() + desc_bytes, starts.data(), starts.size() * sizeof(int));
    HIP_TRY(d_desc.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(d_desc.p, stage.data(), bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (`stage` is pageable: the copy has read it)
    HIP_TRY(ndt::launch_transform_multi(reinterpret_cast<const ndt::TransformScan*>(d_desc.p), reinterpret_cast<const int*>(d_desc.p + desc_bytes),
                                        static_cast<int>(d.size()), static_cast<int>(blocks), posed.p, st));
    h->acc_launches++;
  }
  HIP_TRY(keys_a.reserve(N));
  HIP_TRY(keys_b.reserve(N));
  HIP_TRY(vals_a.reserve(N));
  HIP_TRY(sorted_idx.reserve(N));
  HIP_TRY(run_slot.reserve(N));
  HIP_TRY(touched.reserve(N));
  HIP_TRY(w.reserve(5 * N));
  HIP_TRY(info.reserve(8));
  HIP_TRY(counts.reserve(4));
  unsigned *flags = w.p, *ord = w.p + N, *run_start = w.p + 2 * N, *is_new = w.p + 3 * N, *new_rank = w.p + 4 * N;
  size_t tb_sort = 0, tb_scan = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, keys_a.p, keys_b.p, vals_a.p, sorted_idx.p, n, 0, 64, st));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, flags, ord, n, st));
  const size_t tb = std::max(tb_sort, tb_scan) + 256;
  HIP_TRY(temp.reserve(tb));
  const int info0[8] = {std::numeric_limits<int>::max(), std::numeric_limits<int>::max(), std::numeric_limits<int>::max(),
                        std::numeric_limits<int>::min(), std::numeric_limits<int>::min(), std::numeric_limits<int>::min(), 0, 0};
  HIP_TRY(hipMemcpyAsync(info.p, info0, sizeof(info0), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(counts.p, 0, 4 * sizeof(unsigned), st));
  HIP_TRY(hipMemsetAsync(is_new, 0, N * sizeof(unsigned), st));
  hipLaunchKernelGGL(ndt::k_acc_keys, dim3(ndt::acc_grid_for(N, 2048)), dim3(ndt::kBlock), 0, st, posed.p, n, inv_leaf, keys_a.p, vals_a.p, info.p);
  size_t t2 = tb;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(temp.p, t2, keys_a.p, keys_b.p, vals_a.p, sorted_idx.p, n, 0, 64, st));
  hipLaunchKernelGGL(ndt::k_acc_heads, dim3(ndt::acc_grid_for(N, 2048)), dim3(ndt::kBlock), 0, st, keys_b.p, n, flags, counts.p);
  t2 = tb;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(temp.p, t2, flags, ord, n, st));
  hipLaunchKernelGGL(ndt::k_acc_runs, dim3(ndt::acc_grid_for(N, 2048)), dim3(ndt::kBlock), 0, st, keys_b.p, flags, ord, n, a->view(), run_start, run_slot.p,
                     is_new, counts.p);
  t2 = tb;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(temp.p, t2, is_new, new_rank, n, st));
  hipLaunchKernelGGL(ndt::k_acc_new_total, dim3(1), dim3(1), 0, st, is_new, new_rank, counts.p);
  HIP_TRY(hipGetLastError());
  h->acc_launches += 7;  // keys, sort, heads, scan, runs, scan, total
  // ---- the one read-back
  int hinfo[8];
  unsigned hcounts[4];
  HIP_TRY(hipMemcpyAsync(hinfo, info.p, sizeof(hinfo), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hcounts, counts.p, sizeof(hcounts), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // ---- refusals: nothing of the target has been written so far
  if (hinfo[6])
    return fail(NDT_ERR_INVALID, "a point lies outside the accumulating target's lattice: cell indices must be within [-2^20, 2^20) on every axis");
  const int n_binned = static_cast<int>(hcounts[0]), n_runs = static_cast<int>(hcounts[1]), n_new = static_cast<int>(hcounts[2]);
  float mn[3], mx[3];
  bool have_box = a->have_box;
  for (int k = 0; k < 3; k++) {
    mn[k] = a->mn[k];
    mx[k] = a->mx[k];
  }
  if (n_binned > 0) {
    for (int k = 0; k < 3; k++) {
      const float lo = ndt::acc_decode(hinfo[k]), hi = ndt::acc_decode(hinfo[3 + k]);
      mn[k] = have_box ? std::min(mn[k], lo) : lo;
      mx[k] = have_box ? std::max(mx[k], hi) : hi;
    }
    have_box = true;
  }
  ndt::GridGeom geo = g->geom;
  bool sparse = a->sparse;
  const size_t n_points = a->n_points + N;
  if (have_box) {
    const ndt_status gs = acc_geometry(a->resolution, mn, mx, geo);
    if (gs) return gs;
    // dense or sparse, by the rule for a cloud of the points accumulated so far
    const long long np = static_cast<long long>(std::min<size_t>(n_points, static_cast<size_t>(std::numeric_limits<int>::max())));
    sparse = ndt::wants_sparse_index(h->voxel_index, geo.n_cells, np);
  }
  if (static_cast<long long>(a->n_slots) + n_new > (1ll << 30)) return fail(NDT_ERR_INVALID, "too many voxels in the accumulated target");
  // ---- from here on the target changes
  if (started) acc_adopt(h, started);
  a->n_points = n_points;
  a->n_updates++;
  h->target->n = a->n_points;
  if (!have_box) return NDT_OK;  // no finite point so far: the empty grid
  const int n_slots_before = a->n_slots;
  if (a->slot_cap == 0 && !a->cell.p) {
    bool ignore = false;
    ndt_status s0 = acc_grow(h, a, a->first_cap, &ignore);
    if (s0) return s0;
  }
  bool grown = false;
  ndt_status s = acc_grow(h, a, n_slots_before + n_new, &grown);
  if (s) return s;
  s = acc_settle_table(h, a, geo, sparse, mn, mx, n_slots_before);
  if (s) return s;
  // ---- merge and finish the touched voxels
  if (n_runs > 0) {
    const ndt::FinalizeDump nodump{nullptr, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(ndt::k_acc_merge, dim3(ndt::acc_grid_for(static_cast<size_t>(n_runs) * ndt::kAccTeam, 1 << 30)), dim3(ndt::kBlock), 0, st, posed.p,
                       sorted_idx.p, keys_b.p, run_start, run_slot.p, new_rank, n_runs, n_binned, n_slots_before, a->view(), touched.p);
    hipLaunchKernelGGL(ndt::k_acc_finish, dim3(ndt::acc_grid_for(n_runs, 1 << 30)), dim3(ndt::kBlock), 0, st, touched.p, n_runs, a->view(), a->min_pts,
                       a->eig_ratio, g->recs.p, g->centroids.p, g->lut.p, geo, nodump, static_cast<int*>(nullptr));
    HIP_TRY(hipGetLastError());
    h->acc_launches += 2;
  }
  a->n_slots = n_slots_before + n_new;
  g->empty = a->n_slots == 0;
  g->n_leaves = static_cast<size_t>(a->n_slots);
  g->counts_known = false;
  h->acc_touched = static_cast<size_t>(n_runs);
  h->acc_new = static_cast<size_t>(n_new);
  h->acc_grown = grown ? 1 : 0;
  return NDT_OK;
}

ndt_status acc_checks(ndt_handle h, size_t total) {
  if (total > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "more than INT_MAX points in one accumulate call");
  (void)h;
  return NDT_OK;
}

ndt_status acc_buffer(ndt_handle h, const void* pts, size_t n, size_t stride, bool on_device, const float* pose) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (n && !pts) return fail(NDT_ERR_INVALID, "null point buffer");
  ndt_status s = acc_checks(h, n);
  if (s) return s;
  if (n == 0) return NDT_OK;
  if (stride < 12 || stride % 4) return fail(NDT_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  std::vector<AccScan> one(1);
  s = upload_cloud(h, pts, n, stride, on_device, one[0].c);
  if (s) return s;
  one[0].pose = pose;
  return acc_update(h, one, n);
}

// floor(bound * inv_leaf) as k_acc_keys bins a point (the f32 product rounded before the floor), saturated to the lattice
int acc_crop_cell(float bound, float inv_leaf) {
  const float p = bound * inv_leaf, lim = static_cast<float>(ndt::kAccCellBias);
  if (!(p >= -lim)) return -ndt::kAccCellBias;
  if (p >= lim) return ndt::kAccCellBias - 1;
  return static_cast<int>(std::floor(p));
}

// the target as after accumulating only non-finite points: no box, no voxel, no arrays; the captured parameters stay
void acc_make_empty(AccTarget* a) {
  DeviceGrid* g = a->grid.get();
  a->keys.release();  // (to the stream's pool: reused only behind what is queued)
  a->vals.release();
  a->cell.release();
  a->sums.release();
  a->state.release();
  g->recs.release();
  g->centroids.release();
  g->lut.release();
  a->n_slots = a->slot_cap = 0;
  a->bits = a->first_bits;
  a->have_box = false;
  a->sparse = false;
  for (int k = 0; k < 3; k++) a->mn[k] = a->mx[k] = 0;
  g->geom = ndt::GridGeom{};
  for (int k = 0; k < 3; k++) {
    g->geom.leaf[k] = a->resolution;
    g->geom.inv_leaf[k] = 1.0f / a->resolution;
  }
  g->empty = true;
  g->n_leaves = g->n_cand = g->n_valid = 0;
  g->counts_known = true;
}

// ndt_target_accumulate_crop once the bounds are cells: mark + scan, ONE read-back, then (if anything goes) the kept slots
// compacted into fresh arrays in their order, the key table and the look-up table rebuilt from them
ndt_status acc_crop(ndt_context* h, AccTarget* a, const ndt::AccCropBox& box) {
  hipStream_t st = h->stream;
  DeviceGrid* g = a->grid.get();
  h->crop_kept = static_cast<size_t>(a->n_slots);
  h->crop_points = a->n_points;
  h->crop_removed = h->crop_launches = 0;
  h->crop_relinked = 0;
  if (a->n_slots == 0) {  // no voxel: only the non-finite rows are forgotten
    h->crop_points = a->n_points = 0;
    h->target->n = 0;
    return NDT_OK;
  }
  const int n_slots = a->n_slots;
  const size_t S = static_cast<size_t>(n_slots);
  DevBuf<unsigned> w;  // keep flags, new numbers
  DevBuf<int> info;
  DevBuf<unsigned char> temp;
  HIP_TRY(w.reserve(2 * S));
  HIP_TRY(info.reserve(ndt::kAccCropInfoWords));
  unsigned *keep = w.p, *number = w.p + S;
  size_t tb = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, keep, number, n_slots, st));
  tb += 256;
  HIP_TRY(temp.reserve(tb));
  const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
  const int info0[ndt::kAccCropInfoWords] = {imax, imax, imax, imin, imin, imin, 0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(info.p, info0, sizeof(info0), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(ndt::k_acc_crop_mark, dim3(ndt::acc_grid_for(S, 1 << 30)), dim3(ndt::kBlock), 0, st, a->cell.p, n_slots, box, keep, info.p,
                     static_cast<unsigned long long*>(nullptr), static_cast<int*>(nullptr));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(temp.p, tb, keep, number, n_slots, st));
  h->crop_launches += 2;
  // ---- the one read-back
  int hinfo[ndt::kAccCropInfoWords];
  HIP_TRY(hipMemcpyAsync(hinfo, info.p, sizeof(hinfo), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int kept = hinfo[6];
  unsigned long long kept_points = 0;
  std::memcpy(&kept_points, hinfo + 8, sizeof(kept_points));
  if (kept < 0 || kept > n_slots) return fail(NDT_ERR_HIP, "crop: the kept count is out of range");
  if (kept == n_slots) {  // nothing removed: nothing written, no table rewritten (only the non-finite rows are forgotten)
    h->crop_points = a->n_points = static_cast<size_t>(kept_points);
    h->target->n = a->n_points;
    return NDT_OK;
  }
  h->crop_kept = static_cast<size_t>(kept);
  h->crop_removed = S - static_cast<size_t>(kept);
  h->crop_points = static_cast<size_t>(kept_points);
  if (kept == 0) {
    acc_make_empty(a);
    a->n_points = 0;
    h->target->n = 0;
    return NDT_OK;
  }
  // ---- the box of the kept cells, carried as the centres of its corner cells: (cell + 0.5f) * leaf floors back to the cell
  // for |cell| < 2^20 (the two roundings stay under 0.2 of a cell), so a later update unions its points' box with it as ever
  float mn[3], mx[3];
  for (int k = 0; k < 3; k++) {
    mn[k] = (static_cast<float>(hinfo[k]) + 0.5f) * a->resolution;
    mx[k] = (static_cast<float>(hinfo[3 + k]) + 0.5f) * a->resolution;
  }
  ndt::GridGeom geo = g->geom;
  const ndt_status gs = acc_geometry(a->resolution, mn, mx, geo);
  if (gs) return gs;
  for (int k = 0; k < 3; k++)
    if (geo.min_b[k] != hinfo[k] || geo.max_b[k] != hinfo[3 + k]) return fail(NDT_ERR_HIP, "crop: the kept cells' box does not round-trip");
  const long long np = static_cast<long long>(std::min<unsigned long long>(kept_points, static_cast<unsigned long long>(std::numeric_limits<int>::max())));
  const bool sparse = ndt::wants_sparse_index(h->voxel_index, geo.n_cells, np);
  // ---- capacities: the smallest the kept slots fit (power-of-two multiples of what the target started with)
  int cap = std::max(a->first_cap, 1);
  while (cap < kept) cap *= 2;
  int bits = std::max(a->first_bits, 2);
  while (2 * static_cast<size_t>(kept) > (static_cast<size_t>(1) << bits)) bits++;
  int hash_bits = 0;
  if (sparse) {
    hash_bits = 10;
    while ((static_cast<size_t>(1) << hash_bits) < 2 * static_cast<size_t>(cap)) hash_bits++;
  }
  geo.hash_bits = hash_bits;
  const size_t key_cap = static_cast<size_t>(1) << bits;
  const size_t words = sparse ? (static_cast<size_t>(2) << hash_bits) : static_cast<size_t>(geo.lut_cells);
  DevBuf<int4> cell;
  DevBuf<ndt::AccSums> sums;
  DevBuf<int> state, vals, lut;
  DevBuf<ndt::VoxelRec> recs;
  DevBuf<ndt::VoxelSide> cents;
  DevBuf<unsigned long long> keys;
  HIP_TRY(cell.reserve(cap));
  HIP_TRY(sums.reserve(cap));
  HIP_TRY(state.reserve(cap));
  HIP_TRY(recs.reserve(cap));
  HIP_TRY(cents.reserve(cap));
  HIP_TRY(keys.reserve(key_cap));
  HIP_TRY(vals.reserve(key_cap));
  HIP_TRY(lut.reserve(words));
  // ---- from here on the target changes
  HIP_TRY(hipMemsetAsync(keys.p, 0xFF, key_cap * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(lut.p, 0xFF, words * sizeof(int), st));  // kLutEmpty / free hash slots
  hipLaunchKernelGGL(ndt::k_acc_crop_compact, dim3(ndt::acc_grid_for(S, 1 << 30)), dim3(ndt::kBlock), 0, st, a->view(), n_slots, keep, number, kept, cell.p,
                     sums.p, state.p, recs.p, cents.p);
  a->cell.swap(cell);  // (the old arrays go back to the pool at scope exit: reused only behind the compaction, stream order)
  a->sums.swap(sums);
  a->state.swap(state);
  g->recs.swap(recs);
  g->centroids.swap(cents);
  a->keys.swap(keys);
  a->vals.swap(vals);
  g->lut.swap(lut);
  a->slot_cap = cap;
  a->bits = bits;
  a->n_slots = kept;
  hipLaunchKernelGGL(ndt::k_acc_rehash, dim3(ndt::acc_grid_for(kept, 1 << 30)), dim3(ndt::kBlock), 0, st, a->view(), kept);
  hipLaunchKernelGGL(ndt::k_acc_relink, dim3(ndt::acc_grid_for(kept, 1 << 30)), dim3(ndt::kBlock), 0, st, a->view(), kept, geo, g->lut.p);
  h->crop_launches += 3;
  h->crop_relinked = 1;
  g->geom = geo;
  a->sparse = sparse;
  for (int k = 0; k < 3; k++) {
    a->mn[k] = mn[k];
    a->mx[k] = mx[k];
  }
  a->n_points = static_cast<size_t>(kept_points);
  h->target->n = a->n_points;
  g->empty = false;
  g->n_leaves = static_cast<size_t>(kept);
  g->counts_known = false;
  HIP_TRY(hipGetLastError());
  return NDT_OK;
}

// ndt_target_accumulate_export once the bounds are cells.  buf == null: only the size (the mark alone).  Else mark, sort of
// the (key, slot) pairs, gather -- queued together -- then ONE read-back (rows, their points, their cell box) and the copy of
// the rows; the host writes the header and the checksum.  Nothing of the target is written
ndt_status acc_export(ndt_context* h, AccTarget* a, const ndt::AccCropBox& box, void* buf, size_t capacity, size_t* bytes) {
  hipStream_t st = h->stream;
  h->exp_voxels = h->exp_points = h->exp_launches = 0;
  const int zero[3] = {0, 0, 0};
  if (a->n_slots == 0) {  // no voxel: the header alone
    if (buf && capacity < ndtc::kAccBlobHeaderBytes) return fail(NDT_ERR_INVALID, "the export buffer is too small for the blob");
    if (buf) acc_blob_write_header(buf, a->resolution, 0, zero, zero, nullptr);
    *bytes = ndtc::kAccBlobHeaderBytes;
    return NDT_OK;
  }
  const int n_slots = a->n_slots;
  const size_t S = static_cast<size_t>(n_slots);
  DevBuf<unsigned> keep;
  DevBuf<int> info, vals_a, vals_b;
  DevBuf<unsigned long long> keys_a, keys_b;
  DevBuf<ndt::AccRow> rows;
  DevBuf<unsigned char> temp;
  HIP_TRY(keep.reserve(S));
  HIP_TRY(info.reserve(ndt::kAccCropInfoWords));
  size_t tb = 0;
  if (buf) {
    HIP_TRY(keys_a.reserve(S));
    HIP_TRY(keys_b.reserve(S));
    HIP_TRY(vals_a.reserve(S));
    HIP_TRY(vals_b.reserve(S));
    HIP_TRY(rows.reserve(S));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys_a.p, keys_b.p, vals_a.p, vals_b.p, n_slots, 0, 64, st));
    tb += 256;
    HIP_TRY(temp.reserve(tb));
  }
  const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
  const int info0[ndt::kAccCropInfoWords] = {imax, imax, imax, imin, imin, imin, 0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(info.p, info0, sizeof(info0), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(ndt::k_acc_crop_mark, dim3(ndt::acc_grid_for(S, 1 << 30)), dim3(ndt::kBlock), 0, st, a->cell.p, n_slots, box, keep.p, info.p,
                     buf ? keys_a.p : nullptr, buf ? vals_a.p : nullptr);
  HIP_TRY(hipGetLastError());
  h->exp_launches = 1;
  if (buf) {
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(temp.p, tb, keys_a.p, keys_b.p, vals_a.p, vals_b.p, n_slots, 0, 64, st));
    hipLaunchKernelGGL(ndt::k_acc_export_gather, dim3(ndt::acc_grid_for(S, 1 << 30)), dim3(ndt::kBlock), 0, st, a->view(), vals_b.p, info.p, n_slots, rows.p);
    HIP_TRY(hipGetLastError());
    h->exp_launches = 3;
  }
  // ---- the one read-back
  int hinfo[ndt::kAccCropInfoWords];
  HIP_TRY(hipMemcpyAsync(hinfo, info.p, sizeof(hinfo), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int n = hinfo[6];
  unsigned long long points = 0;
  std::memcpy(&points, hinfo + 8, sizeof(points));
  if (n < 0 || n > n_slots) return fail(NDT_ERR_HIP, "export: the row count is out of range");
  const size_t payload = static_cast<size_t>(n) * ndtc::kAccBlobRowBytes, need = ndtc::kAccBlobHeaderBytes + payload;
  if (buf) {
    if (capacity < need) return fail(NDT_ERR_INVALID, "the export buffer is too small for the blob");
    unsigned char* out = static_cast<unsigned char*>(buf);
    if (n) {
      HIP_TRY(hipMemcpyAsync(out + ndtc::kAccBlobHeaderBytes, rows.p, payload, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    acc_blob_write_header(out, a->resolution, static_cast<uint64_t>(n), hinfo, hinfo + 3, out + ndtc::kAccBlobHeaderBytes);
  }
  *bytes = need;
  h->exp_voxels = static_cast<size_t>(n);
  h->exp_points = static_cast<size_t>(points);
  return NDT_OK;
}

ndt_status acc_export_entry(ndt_handle h, const float* min_xyz, const float* max_xyz, void* buf, size_t capacity, size_t* bytes) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!bytes) return fail(NDT_ERR_INVALID, "null bytes");
  if ((min_xyz == nullptr) != (max_xyz == nullptr)) return fail(NDT_ERR_INVALID, "one bound of the export box is null: give both, or neither for every voxel");
  ndt::AccCropBox box;
  for (int k = 0; k < 3; k++) {
    box.lo[k] = -ndt::kAccCellBias;
    box.hi[k] = ndt::kAccCellBias - 1;
  }
  if (min_xyz) {
    for (int k = 0; k < 3; k++) {
      if (std::isnan(min_xyz[k]) || std::isnan(max_xyz[k])) return fail(NDT_ERR_INVALID, "a bound of the crop box is NaN");
      if (min_xyz[k] > max_xyz[k]) return fail(NDT_ERR_INVALID, "the crop box has min > max on an axis");
    }
  }
  AccTarget* a = acc_live(h);
  if (!a) return fail(NDT_ERR_NO_INPUT, "no accumulated target to export");
  if (min_xyz) {
    const float inv_leaf = 1.0f / a->resolution;
    for (int k = 0; k < 3; k++) {
      box.lo[k] = acc_crop_cell(min_xyz[k], inv_leaf);
      box.hi[k] = acc_crop_cell(max_xyz[k], inv_leaf);
    }
  }
  if (a->n_slots) {
    ndt_status s = ensure_device(h);
    if (s) return s;
  }
  return acc_export(h, a, box, buf, capacity, bytes);
}

// ndt_target_accumulate_import: an accumulate call whose input is voxels.  Upload, ONE check launch over the rows, ONE
// read-back, the refusals; then growth and relink as an update, the rows placed behind the existing slots and finished
ndt_status acc_import(ndt_handle h, const void* blob, size_t bytes) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  ndtc::AccBlobHeader hd;
  if (const char* why = acc_blob_parse(blob, bytes, &hd)) return fail(NDT_ERR_INVALID, why);
  AccTarget* a = acc_live(h);
  const float resolution = a ? a->resolution : h->resolution;
  if (std::memcmp(&hd.resolution, &resolution, sizeof(float)) != 0)
    return fail(NDT_ERR_INVALID, "the blob's resolution is not the resolution of the target it is imported into");
  if (static_cast<unsigned long long>(a ? a->n_slots : 0) + hd.n_voxels > (1ull << 30)) return fail(NDT_ERR_INVALID, "too many voxels in the accumulated target");
  if (hd.n_voxels == 0) return NDT_OK;
  ndt_status s = ensure_device(h);
  if (s) return s;
  hipStream_t st = h->stream;
  h->acc_touched = h->acc_new = h->acc_launches = 0;
  h->acc_relinked = h->acc_grown = 0;
  std::shared_ptr<AccTarget> started;
  if (!a) {
    started = acc_start(h);
    a = started.get();
  }
  DeviceGrid* g = a->grid.get();
  const int n = static_cast<int>(hd.n_voxels);
  const size_t N = static_cast<size_t>(n);
  DevBuf<ndt::AccRow> rows;
  DevBuf<int> info, touched;
  HIP_TRY(rows.reserve(N));
  HIP_TRY(info.reserve(ndt::kAccCropInfoWords));
  HIP_TRY(touched.reserve(N));
  const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
  const int info0[ndt::kAccCropInfoWords] = {imax, imax, imax, imin, imin, imin, 0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(info.p, info0, sizeof(info0), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(rows.p, static_cast<const unsigned char*>(blob) + ndtc::kAccBlobHeaderBytes, N * sizeof(ndt::AccRow), hipMemcpyHostToDevice, st));
  ndt::AccCropBox box;
  for (int k = 0; k < 3; k++) {
    box.lo[k] = hd.lo[k];
    box.hi[k] = hd.hi[k];
  }
  hipLaunchKernelGGL(ndt::k_acc_import_check, dim3(ndt::acc_grid_for(N, 1 << 30)), dim3(ndt::kBlock), 0, st, rows.p, n, box, a->view(), info.p);
  HIP_TRY(hipGetLastError());
  h->acc_launches++;
  // ---- the one read-back (the blob is the caller's pageable memory: the copy has read it by then)
  int hinfo[ndt::kAccCropInfoWords];
  HIP_TRY(hipMemcpyAsync(hinfo, info.p, sizeof(hinfo), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // ---- refusals: nothing of the target has been written so far
  const int flags = hinfo[6];
  if (flags & ndt::kAccRowOutside) return fail(NDT_ERR_INVALID, "a row of the blob lies outside the cell box of its header");
  if (flags & ndt::kAccRowCount) return fail(NDT_ERR_INVALID, "a row of the blob has a count below 1");
  if (flags & ndt::kAccRowNonFinite) return fail(NDT_ERR_INVALID, "a row of the blob holds a non-finite sum");
  if (flags & ndt::kAccRowOrder) return fail(NDT_ERR_INVALID, "the rows of the blob are not in strictly ascending key order");
  for (int k = 0; k < 3; k++)
    if (hinfo[k] != hd.lo[k] || hinfo[3 + k] != hd.hi[k]) return fail(NDT_ERR_INVALID, "the header's cell box is not the tight box of the blob's rows");
  if (flags & ndt::kAccRowPresent) return fail(NDT_ERR_INVALID, "cell already in the target: a blob's cells must be absent from the target it is imported into");
  unsigned long long points = 0;
  std::memcpy(&points, hinfo + 8, sizeof(points));
  // ---- the box: the union with the centres of the blob's corner cells, the float a cropped target carries
  float mn[3], mx[3];
  for (int k = 0; k < 3; k++) {
    const float lo = (static_cast<float>(hd.lo[k]) + 0.5f) * a->resolution, hi = (static_cast<float>(hd.hi[k]) + 0.5f) * a->resolution;
    mn[k] = a->have_box ? std::min(a->mn[k], lo) : lo;
    mx[k] = a->have_box ? std::max(a->mx[k], hi) : hi;
  }
  ndt::GridGeom geo = g->geom;
  s = acc_geometry(a->resolution, mn, mx, geo);
  if (s) return s;
  const size_t n_points = a->n_points + static_cast<size_t>(points);
  const long long np = static_cast<long long>(std::min<size_t>(n_points, static_cast<size_t>(std::numeric_limits<int>::max())));
  const bool sparse = ndt::wants_sparse_index(h->voxel_index, geo.n_cells, np);
  // ---- from here on the target changes
  if (started) acc_adopt(h, started);
  a->n_points = n_points;
  a->n_updates++;
  h->target->n = a->n_points;
  const int n_slots_before = a->n_slots;
  if (a->slot_cap == 0 && !a->cell.p) {
    bool ignore = false;
    s = acc_grow(h, a, a->first_cap, &ignore);
    if (s) return s;
  }
  bool grown = false;
  s = acc_grow(h, a, n_slots_before + n, &grown);
  if (s) return s;
  s = acc_settle_table(h, a, geo, sparse, mn, mx, n_slots_before);
  if (s) return s;
  const ndt::FinalizeDump nodump{nullptr, nullptr, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(ndt::k_acc_import_place, dim3(ndt::acc_grid_for(N, 1 << 30)), dim3(ndt::kBlock), 0, st, rows.p, n, n_slots_before, a->view(), touched.p);
  hipLaunchKernelGGL(ndt::k_acc_finish, dim3(ndt::acc_grid_for(N, 1 << 30)), dim3(ndt::kBlock), 0, st, touched.p, n, a->view(), a->min_pts, a->eig_ratio,
                     g->recs.p, g->centroids.p, g->lut.p, geo, nodump, static_cast<int*>(nullptr));
  HIP_TRY(hipGetLastError());
  h->acc_launches += 2;
  a->n_slots = n_slots_before + n;
  g->empty = false;
  g->n_leaves = static_cast<size_t>(a->n_slots);
  g->counts_known = false;
  h->acc_touched = h->acc_new = N;
  h->acc_grown = grown ? 1 : 0;
  return NDT_OK;
}

// a whole file into memory / a buffer to a file through a temporary one beside it; "" = done, else the failure
std::string acc_read_file(const char* path, std::vector<unsigned char>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return std::string("cannot open ") + path + ": " + std::strerror(errno);
  unsigned char chunk[1 << 16];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) out.insert(out.end(), chunk, chunk + got);
  const bool bad = std::ferror(f) != 0;
  const int err = errno;
  std::fclose(f);
  return bad ? std::string("cannot read ") + path + ": " + std::strerror(err) : std::string();
}
std::string acc_write_file(const char* path, const unsigned char* data, size_t bytes) {
  const std::string tmp = std::string(path) + ".tmp" + std::to_string(static_cast<long long>(getpid()));
  FILE* f = std::fopen(tmp.c_str(), "wb");
  if (!f) return std::string("cannot write ") + path + ": " + std::strerror(errno);
  const bool wrote = std::fwrite(data, 1, bytes, f) == bytes;
  int err = errno;
  const bool closed = std::fclose(f) == 0;
  if (wrote && !closed) err = errno;
  if (wrote && closed && std::rename(tmp.c_str(), path) == 0) return std::string();
  if (wrote && closed) err = errno;
  std::remove(tmp.c_str());
  return std::string("cannot write ") + path + ": " + std::strerror(err);
}

}  // namespace

bool acc_is_live(const ndt_context* h) { return acc_live(const_cast<ndt_context*>(h)) != nullptr; }

void acc_drop(ndt_context* h) {
  if (acc_live(h)) {
    h->grid.reset();
    h->target.reset();
  }
  h->acc.reset();
}

// occupied / candidate / valid voxels of an accumulated grid, from the slots' states
ndt_status acc_grid_counts(ndt_context* h, DeviceGrid* g) {
  AccTarget* a = acc_live(h);
  if (!a || a->grid.get() != g) return fail(NDT_ERR_INVALID, "not this handle's accumulated target");
  std::vector<int> st(static_cast<size_t>(a->n_slots));
  if (a->n_slots) {
    HIP_TRY(hipMemcpyAsync(st.data(), a->state.p, st.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  g->n_leaves = st.size();
  g->n_cand = g->n_valid = 0;
  for (int v : st) {
    g->n_cand += v != 0;
    g->n_valid += v == 1;
  }
  g->n_sorted = 0;
  g->counts_known = true;
  return NDT_OK;
}

// ndt_grid_dump of an accumulated target: every voxel finished from its sums in dump mode, in ascending linear index
ndt_status acc_grid_dump(ndt_context* h, int64_t* idx, int* nr_points, double* mean, double* cov, double* icov, double* evals) {
  AccTarget* a = acc_live(h);
  if (!a) return fail(NDT_ERR_NO_INPUT, "no grid");
  const size_t V = static_cast<size_t>(a->n_slots);
  if (V == 0) return NDT_OK;
  ndt_status s = ensure_device(h);
  if (s) return s;
  hipStream_t st = h->stream;
  const ndt::GridGeom& geo = a->grid->geom;
  std::vector<int4> cells(V);
  HIP_TRY(hipMemcpyAsync(cells.data(), a->cell.p, V * sizeof(int4), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  std::vector<long long> lin(V);
  std::vector<int> perm(V);
  for (size_t i = 0; i < V; i++) {
    lin[i] = static_cast<long long>(cells[i].x - geo.min_b[0]) * geo.mul[0] + static_cast<long long>(cells[i].y - geo.min_b[1]) * geo.mul[1] +
             static_cast<long long>(cells[i].z - geo.min_b[2]) * geo.mul[2];
    perm[i] = static_cast<int>(i);
  }
  std::sort(perm.begin(), perm.end(), [&](int x, int y) { return lin[x] < lin[y]; });
  DevBuf<int> d_perm, d_n, d_lut;
  DevBuf<double> d_mean, d_cov, d_icov, d_evals;
  DevBuf<ndt::VoxelRec> d_recs;  // dump mode takes the full eigen path for every voxel: its records go to scratch
  DevBuf<ndt::VoxelSide> d_cents;
  HIP_TRY(d_perm.reserve(V));
  HIP_TRY(d_n.reserve(V));
  HIP_TRY(d_mean.reserve(V * 3));
  HIP_TRY(d_cov.reserve(V * 9));
  HIP_TRY(d_icov.reserve(V * 9));
  HIP_TRY(d_evals.reserve(V * 3));
  HIP_TRY(d_recs.reserve(V));
  HIP_TRY(d_cents.reserve(V));
  ndt::GridGeom scratch_geo = geo;
  int hb = 4;
  while ((static_cast<size_t>(1) << hb) < 2 * V) hb++;
  scratch_geo.hash_bits = hb;
  HIP_TRY(d_lut.reserve(static_cast<size_t>(2) << hb));
  HIP_TRY(hipMemsetAsync(d_lut.p, 0xFF, (static_cast<size_t>(2) << hb) * sizeof(int), st));
  HIP_TRY(hipMemcpyAsync(d_perm.p, perm.data(), V * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  const ndt::FinalizeDump dump{d_n.p, d_mean.p, d_cov.p, d_icov.p, d_evals.p};
  DevBuf<int> d_cell;
  HIP_TRY(d_cell.reserve(V));
  hipLaunchKernelGGL(ndt::k_acc_finish, dim3(ndt::acc_grid_for(V, 1 << 30)), dim3(ndt::kBlock), 0, st, d_perm.p, static_cast<int>(V), a->view(), a->min_pts,
                     a->eig_ratio, d_recs.p, d_cents.p, d_lut.p, scratch_geo, dump, d_cell.p);
  HIP_TRY(hipGetLastError());
  if (nr_points) HIP_TRY(hipMemcpyAsync(nr_points, d_n.p, V * sizeof(int), hipMemcpyDeviceToHost, st));
  if (mean) HIP_TRY(hipMemcpyAsync(mean, d_mean.p, V * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (cov) HIP_TRY(hipMemcpyAsync(cov, d_cov.p, V * 9 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (icov) HIP_TRY(hipMemcpyAsync(icov, d_icov.p, V * 9 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (evals) HIP_TRY(hipMemcpyAsync(evals, d_evals.p, V * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (idx)
    for (size_t i = 0; i < V; i++) idx[i] = lin[static_cast<size_t>(perm[i])];
  return NDT_OK;
}

}  // namespace ndtc

extern "C" {

ndt_status ndt_target_accumulate(ndt_handle h, const void* pts, size_t n, size_t stride_bytes, int /*is_dense*/, const float* pose) {
  return acc_buffer(h, pts, n, stride_bytes, false, pose);
}
ndt_status ndt_target_accumulate_device(ndt_handle h, const void* d_pts, size_t n, size_t stride_bytes, int /*is_dense*/, const float* pose) {
  return acc_buffer(h, d_pts, n, stride_bytes, true, pose);
}
ndt_status ndt_target_accumulate_clouds(ndt_handle h, const ndt_cloud* clouds, size_t n_clouds, int /*is_dense*/, const float* poses) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (n_clouds && !clouds) return fail(NDT_ERR_INVALID, "null clouds");
  size_t total = 0;
  for (size_t k = 0; k < n_clouds; k++) {
    if (!clouds[k] || !clouds[k]->c) return fail(NDT_ERR_INVALID, "null cloud");
    total += clouds[k]->c->n;
    if (total > static_cast<size_t>(std::numeric_limits<int>::max())) break;
  }
  ndt_status s = acc_checks(h, total);
  if (s) return s;
  if (total == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  std::vector<AccScan> list(n_clouds);
  for (size_t k = 0; k < n_clouds; k++) {
    s = cloud_use_on(h, clouds[k]->c.get());
    if (s) return s;
    list[k].c = clouds[k]->c;
    list[k].pose = poses ? poses + 16 * k : nullptr;
  }
  return acc_update(h, list, total);
}
ndt_status ndt_target_accumulate_cloud(ndt_handle h, ndt_cloud c, int is_dense, const float* pose) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!c) return fail(NDT_ERR_INVALID, "null cloud");
  return ndt_target_accumulate_clouds(h, &c, 1, is_dense, pose);
}
ndt_status ndt_target_accumulate_reset(ndt_handle h) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (h->device_ready && h->acc) {  // nothing queued may still read what goes back to the pool
    ndt_status s = ensure_device(h);
    if (s) return s;
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  acc_drop(h);
  return NDT_OK;
}
ndt_status ndt_target_accumulated(ndt_handle h, size_t* n_points, size_t* n_voxels, size_t* n_updates) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  const AccTarget* a = acc_live(h);
  if (n_points) *n_points = a ? a->n_points : 0;
  if (n_voxels) *n_voxels = a ? static_cast<size_t>(a->n_slots) : 0;
  if (n_updates) *n_updates = a ? a->n_updates : 0;
  return NDT_OK;
}
ndt_status ndt_diag_target_accumulate(ndt_handle h, size_t* touched_voxels, size_t* new_voxels, int* relinked, int* table_grown,
                                      size_t* launches) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (touched_voxels) *touched_voxels = h->acc_touched;
  if (new_voxels) *new_voxels = h->acc_new;
  if (relinked) *relinked = h->acc_relinked;
  if (table_grown) *table_grown = h->acc_grown;
  if (launches) *launches = h->acc_launches;
  return NDT_OK;
}

ndt_status ndt_target_accumulate_crop(ndt_handle h, const float* min_xyz, const float* max_xyz) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!min_xyz || !max_xyz) return fail(NDT_ERR_INVALID, "null bounds");
  for (int k = 0; k < 3; k++) {
    if (std::isnan(min_xyz[k]) || std::isnan(max_xyz[k])) return fail(NDT_ERR_INVALID, "a bound of the crop box is NaN");
    if (min_xyz[k] > max_xyz[k]) return fail(NDT_ERR_INVALID, "the crop box has min > max on an axis");
  }
  AccTarget* a = acc_live(h);
  if (!a) return fail(NDT_ERR_NO_INPUT, "no accumulated target to crop");
  ndt::AccCropBox box;
  const float inv_leaf = 1.0f / a->resolution;
  for (int k = 0; k < 3; k++) {
    box.lo[k] = acc_crop_cell(min_xyz[k], inv_leaf);
    box.hi[k] = acc_crop_cell(max_xyz[k], inv_leaf);
  }
  ndt_status s = ensure_device(h);
  if (s) return s;
  return acc_crop(h, a, box);
}
ndt_status ndt_diag_target_crop(ndt_handle h, size_t* kept_voxels, size_t* removed_voxels, size_t* kept_points, int* relinked, size_t* launches) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (kept_voxels) *kept_voxels = h->crop_kept;
  if (removed_voxels) *removed_voxels = h->crop_removed;
  if (kept_points) *kept_points = h->crop_points;
  if (relinked) *relinked = h->crop_relinked;
  if (launches) *launches = h->crop_launches;
  return NDT_OK;
}

ndt_status ndt_target_accumulate_export(ndt_handle h, const float* min_xyz, const float* max_xyz, void* buf, size_t capacity, size_t* bytes) {
  return acc_export_entry(h, min_xyz, max_xyz, buf, capacity, bytes);
}
ndt_status ndt_target_accumulate_import(ndt_handle h, const void* blob, size_t bytes) { return acc_import(h, blob, bytes); }
ndt_status ndt_target_accumulate_save(ndt_handle h, const float* min_xyz, const float* max_xyz, const char* path) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!path) return fail(NDT_ERR_INVALID, "null path");
  const AccTarget* a = acc_live(h);
  // room for every voxel: one export, whatever the box selects
  std::vector<unsigned char> blob(ndtc::kAccBlobHeaderBytes + (a ? static_cast<size_t>(a->n_slots) : 0) * ndtc::kAccBlobRowBytes);
  size_t bytes = 0;
  ndt_status s = acc_export_entry(h, min_xyz, max_xyz, blob.data(), blob.size(), &bytes);
  if (s) return s;
  const std::string err = acc_write_file(path, blob.data(), bytes);
  if (!err.empty()) return fail(NDT_ERR_INVALID, err);
  return NDT_OK;
}
ndt_status ndt_target_accumulate_load(ndt_handle h, const char* path) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!path) return fail(NDT_ERR_INVALID, "null path");
  std::vector<unsigned char> blob;
  const std::string err = acc_read_file(path, blob);
  if (!err.empty()) return fail(NDT_ERR_INVALID, err);
  return acc_import(h, blob.data(), blob.size());
}
ndt_status ndt_diag_target_export(ndt_handle h, size_t* voxels, size_t* points, size_t* launches) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (voxels) *voxels = h->exp_voxels;
  if (points) *points = h->exp_points;
  if (launches) *launches = h->exp_launches;
  return NDT_OK;
}
ndt_status ndt_host_acc_blob_info(const void* blob, size_t bytes, float* resolution, size_t* n_voxels, int* lo, int* hi) {
  ndtc::AccBlobHeader hd;
  if (const char* why = acc_blob_parse(blob, bytes, &hd)) return fail(NDT_ERR_INVALID, why);
  if (resolution) *resolution = hd.resolution;
  if (n_voxels) *n_voxels = static_cast<size_t>(hd.n_voxels);
  for (int k = 0; k < 3; k++) {
    if (lo) lo[k] = hd.lo[k];
    if (hi) hi[k] = hd.hi[k];
  }
  return NDT_OK;
}
ndt_status ndt_host_acc_blob_checksum(const void* data, size_t bytes, uint64_t* out) {
  if (!out) return fail(NDT_ERR_INVALID, "null out");
  if (bytes && !data) return fail(NDT_ERR_INVALID, "null data");
  if (bytes % 8) return fail(NDT_ERR_INVALID, "the checksum runs over 8-byte words: bytes must be a multiple of 8");
  *out = acc_blob_hash(ndtc::kAccBlobHashSeed, data, bytes);
  return NDT_OK;
}

ndt_status ndt_host_acc_pack_cell(int i, int j, int k, uint64_t* key) {
  const int lim = ndt::kAccCellBias;
  if (!key) return fail(NDT_ERR_INVALID, "null key");
  if (i < -lim || i >= lim || j < -lim || j >= lim || k < -lim || k >= lim)
    return fail(NDT_ERR_INVALID, "cell indices must be within [-2^20, 2^20) on every axis");
  *key = ndt::acc_pack(i, j, k);
  return NDT_OK;
}
void ndt_host_acc_unpack_cell(uint64_t key, int* i, int* j, int* k) { ndt::acc_unpack(key, *i, *j, *k); }

}  // extern "C"
