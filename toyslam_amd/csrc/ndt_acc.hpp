// ndt_acc.hpp -- private to the units of the accumulating target: ndt_acc_kernels.hip (kernels and their launches),
// ndt_acc_rays.hip (the ray pass of a clearing and its launches), ndt_accumulate.hip (the target's state and what changes
// slots), ndt_acc_persist.hip (export / import / files)
#pragma once
#include "ndt_acc_blob.hpp"
#include "ndt_internal.hpp"

namespace ndt {

constexpr int kAccCellBias = 1 << 20;               // cells of [-2^20, 2^20) on every axis

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

// ---- crop to a box of cells (ndt_target_accumulate_crop): over the slots, never over points
struct AccCropBox {
  int lo[3], hi[3];  // kept: lo <= cell <= hi on every axis
};
// info words of a crop: [0..2] lowest kept cell, [3..5] highest kept cell, [6] kept slots, [8..9] kept points (64 bit)
constexpr int kAccCropInfoWords = 10;

// ---- export / import (ndt_target_accumulate_export / _import): a voxel leaves or enters as its cell, count and sums
struct AccRow {  // a row of the blob (include/ndt_mi355.h)
  int i, j, k, count;
  double d[9];
  float f[3];
  float pad;
};
static_assert(sizeof(AccRow) == ndtc::kAccBlobRowBytes, "a blob row is 104 bytes");

// what is wrong with a row (info[6] of an import check)
constexpr int kAccRowOutside = 1, kAccRowCount = 2, kAccRowNonFinite = 4, kAccRowOrder = 8, kAccRowPresent = 16;

// ---- launches (ndt_acc_kernels.hip): each queues everything between two host decisions.  Scratch of one stage comes from the
// pool of the calling thread's stream (DevBuf) and goes back at return: reused only behind what is queued
struct AccBins {  // what the binning of an update's points leaves for its merge
  ndtc::DevBuf<unsigned long long> keys;  // sorted: a run of equal keys is a voxel's points
  ndtc::DevBuf<int> sorted_idx, run_slot;
  ndtc::DevBuf<unsigned> w, counts;  // w: flags, ord, run_start, is_new, new_rank; counts: points binned, runs, new voxels
  unsigned *run_start = nullptr, *new_rank = nullptr;
};
// keys, sort, heads, scan, runs, scan, total (7 launches); info as acc_info_reset left it
hipError_t launch_acc_bin(const float4* posed, int n, float inv_leaf, const AccView& v, int* info, AccBins& b, hipStream_t st);
// the keep flags of a box; number != null: and their exclusive scan; rows != null: and the kept slots sorted by key, gathered
hipError_t launch_acc_mark(const AccView& v, int n_slots, const AccCropBox& box, unsigned* keep, int* info, unsigned* number, AccRow* rows, hipStream_t st);
hipError_t launch_acc_rehash(const AccView& v, int n_slots, hipStream_t st);
hipError_t launch_acc_relink(const AccView& v, int n_slots, const GridGeom& geo, int* lut, hipStream_t st);
struct AccPlan {  // what an update or an import has decided while the target is still untouched, and the voxels it brings
  float mn[3], mx[3];    // the target's box after the call
  bool have_box = true;  // false: no finite point so far -- the call only counts its points
  size_t n_points = 0;   // the target's points after the call
  int n_touched = 0, n_new = 0;  // voxels the call adds to (an update's runs, an import's rows); of those, the ones it starts
  const float4* posed = nullptr;  // an update: the posed points, n_binned of them in the runs of their bins ...
  const AccBins* bins = nullptr;
  int n_binned = 0;
  const AccRow* rows = nullptr;  // ... or an import: the checked rows
};
// the plan's voxels into the slots of `a` from n_slots_before on (merge, or place), then finished: 2 launches
hipError_t launch_acc_extend(const AccPlan& p, int n_slots_before, ndtc::AccTarget* a, const GridGeom& geo, hipStream_t st);
hipError_t launch_acc_compact(const AccView& from, int n_slots, const unsigned* keep, const unsigned* number, int n_kept, const AccView& to, hipStream_t st);
hipError_t launch_acc_import_check(const AccRow* rows, int n, const AccCropBox& box, const AccView& v, int* info, hipStream_t st);
hipError_t launch_acc_finish(const int* order, int n, ndtc::AccTarget* a, VoxelRec* recs, VoxelSide* cents, int* lut, const GridGeom& geo, FinalizeDump dump,
                             int* cell_out, hipStream_t st);

// ---- clearing by rays (ndt_target_accumulate_clear_rays, ndt_acc_rays.hip): a walk per point through the key table
struct AccRayScan {  // a cloud of a call: n > 0 records, the call's points [first, first + n); its pose and its sensor origin
  const float4* src;
  int n, first;
  float T[12];
  float o[3];
};
constexpr int kAccRayCounters = 3;  // u64 words a ray pass adds to: rays cast, rays skipped, cells visited by cast rays
// ONE launch over all clouds: per point the hit flag of its build cell's slot, and +1 on the miss count of every occupied cell
// its ray visits.  box: the target's cell box (no voxel lies outside it).  miss / hit: n_slots words each, zeroed
hipError_t launch_acc_rays(const AccRayScan& one, const AccRayScan* d_scans, int n_scans, int n_points, int blocks, float resolution,
                           const ndt_ray_spec& spec, const AccView& v, const AccCropBox& box, unsigned* miss, unsigned* hit,
                           unsigned long long* counters, hipStream_t st);
// the keep flags of a clearing (miss < min_rays || hit) and their exclusive scan: launch_acc_mark's two launches and its info
// block; info[7] = voxels with miss >= 1
hipError_t launch_acc_rays_mark(const AccView& v, int n_slots, const unsigned* miss, const unsigned* hit, int min_rays, unsigned* keep, int* info,
                                unsigned* number, hipStream_t st);

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

// the info block every call's kernels reduce into, as its kAccCropInfoWords words lie: a box (of encoded floats from k_acc_keys:
// ndt::acc_decode; else of cells), [6] the range flag of an update / kept slots / rows / the flags of an import's rows, [7] a clearing's voxels with a miss, [8..9] points
struct AccInfo {
  int lo[3], hi[3], word6, word7;
  unsigned long long points;
};
static_assert(sizeof(AccInfo) == ndt::kAccCropInfoWords * sizeof(int), "AccInfo is the info block");
hipError_t acc_info_reset(DevBuf<int>& info, hipStream_t st);                     // reserved; the empty box and zeros queued
hipError_t acc_info_read(const DevBuf<int>& info, hipStream_t st, AccInfo* out);  // THE read-back of a call: waits for the stream

AccTarget* acc_live(ndt_context* h);
AccTarget* acc_begin(ndt_context* h, std::shared_ptr<AccTarget>& started);  // the live target or one started for this call; acc_* diagnostics cleared
ndt_status acc_commit(ndt_context* h, AccTarget* a, const std::shared_ptr<AccTarget>& started, const ndt::AccPlan& p);
// bounds (both null: every cell) checked, the handle's live target (else NDT_ERR_NO_INPUT with `no_target`), the bounds as its cells
ndt_status acc_box_of_bounds(ndt_context* h, const float* min_xyz, const float* max_xyz, const char* no_target, AccTarget** a, ndt::AccCropBox* box);
void acc_box_of_cells(const AccTarget* a, const int* lo, const int* hi, bool unite, float* mn, float* mx);

}  // namespace ndtc
