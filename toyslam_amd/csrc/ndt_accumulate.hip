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
//
// One clearing by rays (ndt_target_accumulate_clear_rays*) -- one launch over the call's points, then over the slots:
//   k_acc_rays          a thread per point of all clouds: pose, hit flag of its build cell's slot, the ray walked through the key
//                       table, +1 on the miss count of every occupied cell it visits (ndt_acc_rays.hip, ndt_rays.hpp)
//   k_acc_rays_mark / scan   the crop's mark with the predicate miss < min_rays || hit
//   ---- one read-back; then the crop's tail (acc_remove_unkept): compact, rehash, relink if anything goes and anything stays
#include "ndt_acc.hpp"
#include "ndt_rays.hpp"

namespace ndtc {

namespace {

int env_int(const char* name, int dflt, int lo, int hi) {
  const char* v = getenv(name);
  return v ? std::max(lo, std::min(hi, atoi(v))) : dflt;
}

struct AccScan {
  std::shared_ptr<DeviceCloud> c;
  const float* pose = nullptr;
};
constexpr const char* kAccTooManyPoints = "more than INT_MAX points in one accumulate call";

// the lattice of the accumulated box (lattice_geometry: what a cloud's grid gets) and its padded table
ndt_status acc_geometry(float resolution, const float* min_p, const float* max_p, ndt::GridGeom& geo) {
  const ndt::LatticeStatus ls = ndt::lattice_geometry(resolution, min_p, max_p, geo);
  if (ls == ndt::kLatticeIndexOverflow)
    return fail(NDT_ERR_GRID_OVERFLOW, "leaf size is too small for the accumulated target: integer indices would overflow");
  if (ls != ndt::kLatticeOk) return fail(NDT_ERR_GRID_OVERFLOW, "voxel grid too large");
  ndt::set_padded_lut(geo);
  return NDT_OK;
}

// dense or sparse, by the rule for a cloud of as many points
bool acc_wants_sparse(const ndt_context* h, const ndt::GridGeom& geo, unsigned long long n_points) {
  const long long np = static_cast<long long>(std::min<unsigned long long>(n_points, static_cast<unsigned long long>(std::numeric_limits<int>::max())));
  return ndt::wants_sparse_index(h->voxel_index, geo.n_cells, np);
}
// fresh slot arrays, reserved while the target is still untouched and then installed / a fresh, cleared key table: the smallest
// power-of-two multiple of `from` that holds `want` slots, the table at most half full with them
struct AccSlots {
  DevBuf<int4> cell;
  DevBuf<ndt::AccSums> sums;
  DevBuf<int> state;
  DevBuf<ndt::VoxelRec> recs;
  DevBuf<ndt::VoxelSide> cents;
  int cap = 0;
  hipError_t reserve(int from, int want) {
    cap = std::max(from, 1);
    while (cap < want) cap *= 2;
    HIP_PASS(cell.reserve(cap));
    HIP_PASS(sums.reserve(cap));
    HIP_PASS(state.reserve(cap));
    HIP_PASS(recs.reserve(cap));
    return cents.reserve(cap);
  }
  ndt::AccView view() { return ndt::AccView{nullptr, nullptr, 0, cell.p, sums.p, state.p, recs.p, cents.p}; }
  void install(AccTarget* a) {  // (the old arrays go back to the pool at scope exit: reused only behind what is queued, stream order)
    a->cell.swap(cell);
    a->sums.swap(sums);
    a->state.swap(state);
    a->grid->recs.swap(recs);
    a->grid->centroids.swap(cents);
    a->slot_cap = cap;
  }
};
bool acc_keys_hold(int bits, int want) { return 2 * static_cast<size_t>(want) <= (static_cast<size_t>(1) << bits); }
hipError_t acc_fresh_keys(AccTarget* a, int from, int want, hipStream_t st) {  // (nothing of `a` changes unless both are reserved)
  int bits = std::max(from, 2);
  while (!acc_keys_hold(bits, want)) bits++;
  DevBuf<unsigned long long> keys;
  DevBuf<int> vals;
  HIP_PASS(keys.reserve(static_cast<size_t>(1) << bits));
  HIP_PASS(vals.reserve(static_cast<size_t>(1) << bits));
  a->keys.swap(keys);
  a->vals.swap(vals);
  a->bits = bits;
  return hipMemsetAsync(a->keys.p, 0xFF, sizeof(unsigned long long) << bits, st);
}

// slot arrays at least `want` slots, the key table at most half full with `want` voxels: doubled, copied / re-inserted
ndt_status acc_grow(ndt_context* h, AccTarget* a, int want, bool* grown) {
  hipStream_t st = h->stream;
  if (want > a->slot_cap) {
    AccSlots fresh;
    HIP_TRY(fresh.reserve(a->slot_cap, want));
    if (a->n_slots) {
      const size_t m = static_cast<size_t>(a->n_slots);
      HIP_TRY(hipMemcpyAsync(fresh.cell.p, a->cell.p, m * sizeof(int4), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(fresh.sums.p, a->sums.p, m * sizeof(ndt::AccSums), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(fresh.state.p, a->state.p, m * sizeof(int), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(fresh.recs.p, a->grid->recs.p, m * sizeof(ndt::VoxelRec), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(fresh.cents.p, a->grid->centroids.p, m * sizeof(ndt::VoxelSide), hipMemcpyDeviceToDevice, st));
      *grown = true;
    }
    fresh.install(a);
  }
  if (!a->keys.p || !acc_keys_hold(a->bits, want)) {
    HIP_TRY(acc_fresh_keys(a, a->bits, want, st));
    if (a->n_slots) {
      HIP_TRY(ndt::launch_acc_rehash(a->view(), a->n_slots, st));
      h->acc_launches++;
      *grown = true;
    }
  }
  return NDT_OK;
}

void acc_adopt(ndt_context* h, const std::shared_ptr<AccTarget>& started) {
  h->acc = started;
  h->grid = started->grid;
  auto holder = std::make_shared<DeviceCloud>();  // the handle "has a target"; its points are not kept
  h->target = holder;
  h->target_dense = 0;
}

// the look-up table of a geometry and form: a hash of at least twice the slots (geo.hash_bits) or the padded dense table (0), cleared
int acc_lut_hash_bits(bool sparse, int slot_cap, int floor = 10) {
  int hash_bits = sparse ? floor : 0;
  while (sparse && (static_cast<size_t>(1) << hash_bits) < 2 * static_cast<size_t>(slot_cap)) hash_bits++;
  return hash_bits;
}
hipError_t acc_fresh_lut(const ndt::GridGeom& geo, DevBuf<int>& lut, hipStream_t st) {
  const size_t words = geo.hash_bits ? (static_cast<size_t>(2) << geo.hash_bits) : static_cast<size_t>(geo.lut_cells);
  HIP_PASS(lut.reserve(words));
  return hipMemsetAsync(lut.p, 0xFF, words * sizeof(int), st);  // kLutEmpty / free hash slots
}
// the target's table is `lut`, built under `geo` for the box [mn, mx]
void acc_install_table(AccTarget* a, DevBuf<int>& lut, const ndt::GridGeom& geo, bool sparse, const float* mn, const float* mx) {
  if (lut.p) a->grid->lut.swap(lut);
  a->grid->geom = geo;
  a->sparse = sparse;
  a->have_box = true;
  std::memcpy(a->mn, mn, sizeof(a->mn));
  std::memcpy(a->mx, mx, sizeof(a->mx));
}

// the table the evaluation kernels read, under the geometry `geo` of the box [mn, mx]: relinked only when the box, its form
// or its size changed.  The slots before this call are entered again; the call's own voxels follow through k_acc_finish
ndt_status acc_settle_table(ndt_context* h, AccTarget* a, ndt::GridGeom& geo, bool sparse, const float* mn, const float* mx, int n_slots_before) {
  const ndt::GridGeom& old = a->grid->geom;
  geo.hash_bits = acc_lut_hash_bits(sparse, a->slot_cap);
  const bool relink = !a->have_box || sparse != a->sparse || std::memcmp(geo.min_b, old.min_b, sizeof(geo.min_b)) != 0 ||
                      std::memcmp(geo.max_b, old.max_b, sizeof(geo.max_b)) != 0 || geo.hash_bits != old.hash_bits;
  const bool had_box = a->have_box;
  DevBuf<int> lut;
  if (relink) HIP_TRY(acc_fresh_lut(geo, lut, h->stream));
  acc_install_table(a, lut, geo, sparse, mn, mx);
  if (relink && n_slots_before) {
    HIP_TRY(ndt::launch_acc_relink(a->view(), n_slots_before, geo, a->grid->lut.p, h->stream));
    h->acc_launches++;
    h->acc_relinked = had_box ? 1 : 0;
  }
  return NDT_OK;
}

ndt_status acc_update(ndt_context* h, const std::vector<AccScan>& scans, size_t total) {
  static const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  hipStream_t st = h->stream;
  const int n = static_cast<int>(total);
  std::shared_ptr<AccTarget> started;
  AccTarget* a = acc_begin(h, started);

  // ---- the posed points (N2's transform, one launch for all clouds) and their keys
  DevBuf<float4> posed;
  DevBuf<int> info;
  DevBuf<unsigned char> d_desc;
  ndt::AccBins bins;
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
  HIP_TRY(acc_info_reset(info, st));
  HIP_TRY(ndt::launch_acc_bin(posed.p, n, 1.0f / a->resolution, a->view(), info.p, bins, st));
  h->acc_launches += 7;  // keys, sort, heads, scan, runs, scan, total
  // ---- the one read-back
  AccInfo seen;
  unsigned hcounts[4];
  HIP_TRY(hipMemcpyAsync(hcounts, bins.counts.p, sizeof(hcounts), hipMemcpyDeviceToHost, st));
  HIP_TRY(acc_info_read(info, st, &seen));
  // ---- refusals: nothing of the target has been written so far
  if (seen.word6)
    return fail(NDT_ERR_INVALID, "a point lies outside the accumulating target's lattice: cell indices must be within [-2^20, 2^20) on every axis");
  ndt::AccPlan plan;
  plan.posed = posed.p;
  plan.bins = &bins;
  const int n_binned = plan.n_binned = static_cast<int>(hcounts[0]);
  plan.n_touched = static_cast<int>(hcounts[1]);  // runs
  plan.n_new = static_cast<int>(hcounts[2]);
  plan.n_points = a->n_points + N;
  plan.have_box = a->have_box || n_binned > 0;
  for (int k = 0; k < 3; k++) {  // the box so far and the box of the call's finite points
    const float lo = ndt::acc_decode(seen.lo[k]), hi = ndt::acc_decode(seen.hi[k]);
    plan.mn[k] = n_binned <= 0 ? a->mn[k] : a->have_box ? std::min(a->mn[k], lo) : lo;
    plan.mx[k] = n_binned <= 0 ? a->mx[k] : a->have_box ? std::max(a->mx[k], hi) : hi;
  }
  return acc_commit(h, a, started, plan);
}

ndt_status acc_buffer(ndt_handle h, const void* pts, size_t n, size_t stride, bool on_device, const float* pose) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (n && !pts) return fail(NDT_ERR_INVALID, "null point buffer");
  if (n > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, kAccTooManyPoints);
  if (n == 0) return NDT_OK;
  if (stride < 12 || stride % 4) return fail(NDT_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  std::vector<AccScan> one(1);
  const ndt_status s = upload_cloud(h, pts, n, stride, on_device, one[0].c);
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
  g->touched();
}

// What a removal of whole voxels did (a crop's and a clearing's diagnostics)
struct AccRemoval {
  size_t kept = 0, removed = 0, points = 0, launches = 0;
  int relinked = 0;
};

// The shared tail of a crop and a clearing, after THE read-back of the mark pass (`seen`: kept slots, their points, their cell
// box; keep / number: the flags and their exclusive scan): nothing removed -> nothing written; else the kept slots compacted
// into fresh arrays in their order, the key table and the look-up table rebuilt from them (three launches)
ndt_status acc_remove_unkept(ndt_context* h, AccTarget* a, const AccInfo& seen, const unsigned* keep, const unsigned* number, AccRemoval* r) {
  hipStream_t st = h->stream;
  DeviceGrid* g = a->grid.get();
  const int n_slots = a->n_slots;
  const size_t S = static_cast<size_t>(n_slots);
  auto done = [&](size_t points) {  // the points the target still holds: the non-finite rows are forgotten in any case
    r->points = a->n_points = points;
    h->target->n = points;
    return NDT_OK;
  };
  const int kept = seen.word6;
  if (kept < 0 || kept > n_slots) return fail(NDT_ERR_HIP, "crop: the kept count is out of range");
  if (kept == n_slots) return done(seen.points);  // nothing removed: nothing written, no table rewritten
  r->kept = static_cast<size_t>(kept);
  r->removed = S - static_cast<size_t>(kept);
  r->points = static_cast<size_t>(seen.points);
  if (kept == 0) {
    acc_make_empty(a);
    return done(0);
  }
  float mn[3], mx[3];
  acc_box_of_cells(a, seen.lo, seen.hi, false, mn, mx);
  ndt::GridGeom geo = g->geom;
  const ndt_status gs = acc_geometry(a->resolution, mn, mx, geo);
  if (gs) return gs;
  for (int k = 0; k < 3; k++)
    if (geo.min_b[k] != seen.lo[k] || geo.max_b[k] != seen.hi[k]) return fail(NDT_ERR_HIP, "crop: the kept cells' box does not round-trip");
  const bool sparse = acc_wants_sparse(h, geo, seen.points);
  // ---- capacities: the smallest the kept slots fit (power-of-two multiples of what the target started with)
  AccSlots slots;
  DevBuf<int> lut;
  HIP_TRY(slots.reserve(a->first_cap, kept));
  geo.hash_bits = acc_lut_hash_bits(sparse, slots.cap);
  HIP_TRY(acc_fresh_lut(geo, lut, st));
  // ---- from here on the target changes: a fresh key table, compact into the fresh slots, install them, rehash, relink
  HIP_TRY(acc_fresh_keys(a, a->first_bits, kept, st));
  HIP_TRY(ndt::launch_acc_compact(a->view(), n_slots, keep, number, kept, slots.view(), st));
  slots.install(a);
  acc_install_table(a, lut, geo, sparse, mn, mx);
  a->n_slots = kept;
  g->touched();  // (the centroid fitness and readers' caches: voxels left, the box changed)
  HIP_TRY(ndt::launch_acc_rehash(a->view(), kept, st));
  HIP_TRY(ndt::launch_acc_relink(a->view(), kept, geo, g->lut.p, st));
  r->launches += 3;
  r->relinked = 1;
  g->empty = false;
  g->n_leaves = static_cast<size_t>(kept);
  g->counts_known = false;
  return done(seen.points);
}

// ndt_target_accumulate_crop once the bounds are cells: mark + scan, ONE read-back, then (if anything goes) acc_remove_unkept
ndt_status acc_crop_run(ndt_context* h, AccTarget* a, const ndt::AccCropBox& box, AccRemoval* r) {
  hipStream_t st = h->stream;
  const int n_slots = a->n_slots;
  const size_t S = static_cast<size_t>(n_slots);
  r->kept = S;
  r->points = a->n_points;
  if (n_slots == 0) {  // no voxel: the non-finite rows are forgotten
    r->points = a->n_points = 0;
    h->target->n = 0;
    return NDT_OK;
  }
  DevBuf<unsigned> w;  // keep flags, new numbers
  DevBuf<int> info;
  HIP_TRY(w.reserve(2 * S));
  HIP_TRY(acc_info_reset(info, st));
  unsigned *keep = w.p, *number = w.p + S;
  HIP_TRY(ndt::launch_acc_mark(a->view(), n_slots, box, keep, info.p, number, nullptr, st));
  r->launches += 2;
  // ---- the one read-back
  AccInfo seen;
  HIP_TRY(acc_info_read(info, st, &seen));
  return acc_remove_unkept(h, a, seen, keep, number, r);
}
ndt_status acc_crop(ndt_context* h, AccTarget* a, const ndt::AccCropBox& box) {
  AccRemoval r;
  const ndt_status s = acc_crop_run(h, a, box, &r);
  h->crop_kept = r.kept;
  h->crop_removed = r.removed;
  h->crop_points = r.points;
  h->crop_launches = r.launches;
  h->crop_relinked = r.relinked;
  return s;
}

// ---- clearing by rays (ndt_target_accumulate_clear_rays*, _ray_counts): the ray pass over the call's points, then a removal
int rays_max_blocks() {  // development switch, read per call: small values reach the strided regime with small clouds
  const char* e = getenv("NDT_RAYS_MAX_BLOCKS");
  const int x = e ? atoi(e) : 0;
  return x > 0 ? std::min(x, ndt::kRayMaxBlocks) : ndt::kRayMaxBlocks;
}

struct RayCall {  // a checked call: its live target, its non-empty clouds as the kernel takes them, its points
  AccTarget* a = nullptr;
  std::vector<std::shared_ptr<DeviceCloud>> clouds;
  std::vector<ndt::AccRayScan> scans;
  size_t total = 0;
};
struct RayPass {  // what the ray pass leaves on the device: miss and hit per slot, the three totals
  DevBuf<unsigned> w;
  DevBuf<unsigned long long> counters;
  DevBuf<unsigned char> d_scans;
  unsigned *miss = nullptr, *hit = nullptr;
};

// every refusal of the three entries, in the header's order; nothing needs a device
ndt_status rays_checks(ndt_handle h, const ndt_cloud* clouds, size_t n_clouds, const float* poses, const float* origins, const ndt_ray_spec* spec,
                       RayCall* call) {
  static const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!spec) return fail(NDT_ERR_INVALID, "null ray spec");
  if (n_clouds && !clouds) return fail(NDT_ERR_INVALID, "null clouds");
  for (size_t k = 0; k < n_clouds; k++) {
    for (int q = 0; poses && q < 16; q++)
      if (!std::isfinite(poses[16 * k + q])) return fail(NDT_ERR_INVALID, "a pose of a ray call is not finite");
    for (int q = 0; origins && q < 3; q++)
      if (!std::isfinite(origins[3 * k + q])) return fail(NDT_ERR_INVALID, "a sensor origin of a ray call is not finite");
  }
  for (size_t k = 0; k < n_clouds; k++)
    if (!clouds[k] || !clouds[k]->c) return fail(NDT_ERR_INVALID, "null cloud");
  call->a = acc_live(h);
  if (!call->a) return fail(NDT_ERR_NO_INPUT, "no accumulated target to cast rays through");
  if (const char* why = ndt::ray_spec_error(*spec, call->a->resolution)) return fail(NDT_ERR_INVALID, why);
  for (size_t k = 0; k < n_clouds; k++) {
    const size_t m = clouds[k]->c->n;
    if (!m) continue;
    if (call->total + m > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "more than INT_MAX points in one ray call");
    ndt::AccRayScan sc{};
    const float* pose = poses ? poses + 16 * k : I;
    sc.n = static_cast<int>(m);
    sc.first = static_cast<int>(call->total);
    colmajor_to_T12(pose, sc.T);
    for (int q = 0; q < 3; q++) sc.o[q] = origins ? origins[3 * k + q] : pose[12 + q];
    call->scans.push_back(sc);
    call->clouds.push_back(clouds[k]->c);
    call->total += m;
  }
  return NDT_OK;
}

// the ONE launch over the call's points, queued; miss / hit / the totals are read behind the caller's wait
ndt_status rays_pass(ndt_context* h, RayCall& call, const ndt_ray_spec& spec, RayPass& p) {
  hipStream_t st = h->stream;
  AccTarget* a = call.a;
  h->ray_cast = h->ray_skipped = h->ray_touched = h->ray_removed = h->ray_points = h->ray_launches = 0;
  h->ray_visited = 0;
  h->ray_relinked = 0;
  h->ray_kept = static_cast<size_t>(a->n_slots);
  const size_t S = static_cast<size_t>(std::max(a->n_slots, 1));
  for (size_t k = 0; k < call.scans.size(); k++) {
    const ndt_status s = cloud_use_on(h, call.clouds[k].get());
    if (s) return s;
    call.scans[k].src = call.clouds[k]->pts.p;
  }
  HIP_TRY(p.w.reserve(2 * S));
  HIP_TRY(p.counters.reserve(ndt::kAccRayCounters));
  p.miss = p.w.p;
  p.hit = p.w.p + S;
  const int n_scans = static_cast<int>(call.scans.size());
  if (n_scans > 1) {
    const size_t bytes = call.scans.size() * sizeof(ndt::AccRayScan);
    HIP_TRY(p.d_scans.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(p.d_scans.p, call.scans.data(), bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the table is pageable: the copy has read it)
  }
  HIP_TRY(hipMemsetAsync(p.w.p, 0, 2 * S * sizeof(unsigned), st));
  HIP_TRY(hipMemsetAsync(p.counters.p, 0, ndt::kAccRayCounters * sizeof(unsigned long long), st));
  ndt::AccCropBox box;
  for (int k = 0; k < 3; k++) {  // the target's cell box: no voxel lies outside it (no voxel: the empty box)
    box.lo[k] = a->n_slots ? a->grid->geom.min_b[k] : 1;
    box.hi[k] = a->n_slots ? a->grid->geom.max_b[k] : 0;
  }
  int blocks = 0, passes = 0;
  ndt::ray_plan(call.total, rays_max_blocks(), &blocks, &passes);
  HIP_TRY(ndt::launch_acc_rays(call.scans[0], reinterpret_cast<const ndt::AccRayScan*>(p.d_scans.p), n_scans, static_cast<int>(call.total), blocks,
                               a->resolution, spec, a->view(), box, p.miss, p.hit, p.counters.p, st));
  h->ray_launches = 1;
  return NDT_OK;
}
void rays_totals(ndt_context* h, const unsigned long long* c) {
  h->ray_cast = static_cast<size_t>(c[0]);
  h->ray_skipped = static_cast<size_t>(c[1]);
  h->ray_visited = c[2];
}

ndt_status rays_clear(ndt_context* h, RayCall& call, const ndt_ray_spec& spec) {
  hipStream_t st = h->stream;
  AccTarget* a = call.a;
  RayPass p;
  ndt_status s = rays_pass(h, call, spec, p);
  if (s) return s;
  const int n_slots = a->n_slots;
  unsigned long long totals[ndt::kAccRayCounters];
  if (n_slots == 0) {  // no voxel: the rays are counted, nothing can go
    HIP_TRY(hipMemcpyAsync(totals, p.counters.p, sizeof(totals), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    rays_totals(h, totals);
    return NDT_OK;
  }
  const size_t S = static_cast<size_t>(n_slots);
  DevBuf<unsigned> w;  // keep flags, new numbers
  DevBuf<int> info;
  HIP_TRY(w.reserve(2 * S));
  HIP_TRY(acc_info_reset(info, st));
  unsigned *keep = w.p, *number = w.p + S;
  HIP_TRY(ndt::launch_acc_rays_mark(a->view(), n_slots, p.miss, p.hit, spec.min_rays, keep, info.p, number, st));
  h->ray_launches += 2;
  // ---- the one read-back
  AccInfo seen;
  HIP_TRY(hipMemcpyAsync(totals, p.counters.p, sizeof(totals), hipMemcpyDeviceToHost, st));
  HIP_TRY(acc_info_read(info, st, &seen));
  rays_totals(h, totals);
  h->ray_touched = static_cast<size_t>(seen.word7);
  AccRemoval r;
  r.kept = S;
  r.points = a->n_points;
  s = acc_remove_unkept(h, a, seen, keep, number, &r);
  h->ray_kept = r.kept;
  h->ray_removed = r.removed;
  h->ray_points = r.points;
  h->ray_relinked = r.relinked;
  h->ray_launches += r.launches;
  return s;
}

}  // namespace

AccTarget* acc_live(ndt_context* h) { return (h->acc && h->grid && h->acc->grid == h->grid) ? h->acc.get() : nullptr; }

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

AccTarget* acc_begin(ndt_context* h, std::shared_ptr<AccTarget>& started) {
  h->acc_touched = h->acc_new = h->acc_launches = 0;
  h->acc_relinked = h->acc_grown = 0;
  if (AccTarget* a = acc_live(h)) return a;
  started = acc_start(h);  // a target starts: parameters captured, nothing of the handle's previous target is continued
  return started.get();
}

hipError_t acc_info_reset(DevBuf<int>& info, hipStream_t st) {
  static const AccInfo none = {{std::numeric_limits<int>::max(), std::numeric_limits<int>::max(), std::numeric_limits<int>::max()},
                               {std::numeric_limits<int>::min(), std::numeric_limits<int>::min(), std::numeric_limits<int>::min()}, 0, 0, 0};
  HIP_PASS(info.reserve(ndt::kAccCropInfoWords));
  return hipMemcpyAsync(info.p, &none, sizeof(none), hipMemcpyHostToDevice, st);
}
hipError_t acc_info_read(const DevBuf<int>& info, hipStream_t st, AccInfo* out) {
  HIP_PASS(hipMemcpyAsync(out, info.p, sizeof(*out), hipMemcpyDeviceToHost, st));
  return hipStreamSynchronize(st);
}

// the shared tail of an update and an import: the table planned (the last refusals); adoption, totals, growth, table, voxels
ndt_status acc_commit(ndt_context* h, AccTarget* a, const std::shared_ptr<AccTarget>& started, const ndt::AccPlan& p) {
  ndt::GridGeom geo = a->grid->geom;
  bool sparse = a->sparse;
  if (p.have_box) {  // dense or sparse, by the rule for a cloud of the points accumulated so far
    const ndt_status gs = acc_geometry(a->resolution, p.mn, p.mx, geo);
    if (gs) return gs;
    sparse = acc_wants_sparse(h, geo, p.n_points);
  }
  if (static_cast<long long>(a->n_slots) + p.n_new > (1ll << 30)) return fail(NDT_ERR_INVALID, "too many voxels in the accumulated target");
  // ---- from here on the target changes
  if (started) acc_adopt(h, started);
  DeviceGrid* g = a->grid.get();
  g->touched();  // (the centroid fitness and readers' caches: centroids move, voxels arrive, the box may grow)
  a->n_points = p.n_points;
  a->n_updates++;
  h->target->n = a->n_points;
  if (!p.have_box) return NDT_OK;  // no finite point so far: the empty grid
  const int n_slots_before = a->n_slots;
  bool ignore = false, grown = false;
  ndt_status s = (a->slot_cap == 0 && !a->cell.p) ? acc_grow(h, a, a->first_cap, &ignore) : NDT_OK;
  if (!s) s = acc_grow(h, a, n_slots_before + p.n_new, &grown);
  if (!s) s = acc_settle_table(h, a, geo, sparse, p.mn, p.mx, n_slots_before);
  if (s) return s;
  if (p.n_touched > 0) {  // merge or place, and finish the touched voxels
    HIP_TRY(ndt::launch_acc_extend(p, n_slots_before, a, geo, h->stream));
    h->acc_launches += 2;
  }
  a->n_slots = n_slots_before + p.n_new;
  g->empty = a->n_slots == 0;
  g->n_leaves = static_cast<size_t>(a->n_slots);
  g->counts_known = false;
  h->acc_touched = static_cast<size_t>(p.n_touched);
  h->acc_new = static_cast<size_t>(p.n_new);
  h->acc_grown = grown ? 1 : 0;
  return NDT_OK;
}

ndt_status acc_box_of_bounds(ndt_context* h, const float* min_xyz, const float* max_xyz, const char* no_target, AccTarget** a, ndt::AccCropBox* box) {
  for (int k = 0; min_xyz && k < 3; k++) {
    if (std::isnan(min_xyz[k]) || std::isnan(max_xyz[k])) return fail(NDT_ERR_INVALID, "a bound of the crop box is NaN");
    if (min_xyz[k] > max_xyz[k]) return fail(NDT_ERR_INVALID, "the crop box has min > max on an axis");
  }
  *a = acc_live(h);
  if (!*a) return fail(NDT_ERR_NO_INPUT, no_target);
  const float inv_leaf = 1.0f / (*a)->resolution;
  for (int k = 0; k < 3; k++) {
    box->lo[k] = min_xyz ? acc_crop_cell(min_xyz[k], inv_leaf) : -ndt::kAccCellBias;
    box->hi[k] = min_xyz ? acc_crop_cell(max_xyz[k], inv_leaf) : ndt::kAccCellBias - 1;
  }
  return NDT_OK;
}
// a box of cells as the float box a target carries: the centres of its corner cells.  (cell + 0.5f) * leaf floors back to the
// cell for |cell| < 2^20 (the two roundings stay under 0.2 of a cell), so a later update unions its points' box with it as ever
void acc_box_of_cells(const AccTarget* a, const int* lo, const int* hi, bool unite, float* mn, float* mx) {
  for (int k = 0; k < 3; k++) {
    const float l = (static_cast<float>(lo[k]) + 0.5f) * a->resolution, u = (static_cast<float>(hi[k]) + 0.5f) * a->resolution;
    mn[k] = unite && a->have_box ? std::min(a->mn[k], l) : l;
    mx[k] = unite && a->have_box ? std::max(a->mx[k], u) : u;
  }
}

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
  scratch_geo.hash_bits = acc_lut_hash_bits(true, static_cast<int>(V), 4);
  HIP_TRY(acc_fresh_lut(scratch_geo, d_lut, st));
  HIP_TRY(hipMemcpyAsync(d_perm.p, perm.data(), V * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  const ndt::FinalizeDump dump{d_n.p, d_mean.p, d_cov.p, d_icov.p, d_evals.p};
  DevBuf<int> d_cell;
  HIP_TRY(d_cell.reserve(V));
  HIP_TRY(ndt::launch_acc_finish(d_perm.p, static_cast<int>(V), a, d_recs.p, d_cents.p, d_lut.p, scratch_geo, dump, d_cell.p, st));
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
  if (total > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, kAccTooManyPoints);
  if (total == 0) return NDT_OK;
  ndt_status s = ensure_device(h);
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
  AccTarget* a = nullptr;
  ndt::AccCropBox box;
  ndt_status s = acc_box_of_bounds(h, min_xyz, max_xyz, "no accumulated target to crop", &a, &box);
  if (!s) s = ensure_device(h);
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

ndt_status ndt_target_accumulate_clear_rays_clouds(ndt_handle h, const ndt_cloud* clouds, size_t n_clouds, const float* poses, const float* origins,
                                                   const ndt_ray_spec* spec) {
  RayCall call;
  ndt_status s = rays_checks(h, clouds, n_clouds, poses, origins, spec, &call);
  if (s || call.total == 0) return s;
  s = ensure_device(h);
  if (s) return s;
  return rays_clear(h, call, *spec);
}
ndt_status ndt_target_accumulate_clear_rays(ndt_handle h, ndt_cloud cloud, const float* pose, const float* origin, const ndt_ray_spec* spec) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!cloud) return fail(NDT_ERR_INVALID, "null cloud");
  return ndt_target_accumulate_clear_rays_clouds(h, &cloud, 1, pose, origin, spec);
}
ndt_status ndt_target_accumulate_ray_counts(ndt_handle h, const ndt_cloud* clouds, size_t n_clouds, const float* poses, const float* origins,
                                            const ndt_ray_spec* spec, int* cells, unsigned* misses, unsigned char* hit, size_t capacity,
                                            size_t* n_voxels) {
  RayCall call;
  ndt_status s = rays_checks(h, clouds, n_clouds, poses, origins, spec, &call);
  if (s) return s;
  AccTarget* a = call.a;
  const size_t V = static_cast<size_t>(a->n_slots);
  if (n_voxels) *n_voxels = V;
  if (!cells) return NDT_OK;
  if (!misses || !hit) return fail(NDT_ERR_INVALID, "null output of the ray counts");
  if (capacity < V) return fail(NDT_ERR_INVALID, "the ray counts need room for every voxel of the target");
  if (V == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  hipStream_t st = h->stream;
  std::vector<int4> cell(V);
  std::vector<unsigned> mh(2 * V, 0u);
  if (call.total) {
    RayPass p;
    s = rays_pass(h, call, *spec, p);
    if (s) return s;
    unsigned long long totals[ndt::kAccRayCounters];
    HIP_TRY(hipMemcpyAsync(mh.data(), p.w.p, 2 * V * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(totals, p.counters.p, sizeof(totals), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cell.data(), a->cell.p, V * sizeof(int4), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    rays_totals(h, totals);
  } else {
    HIP_TRY(hipMemcpyAsync(cell.data(), a->cell.p, V * sizeof(int4), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  std::vector<size_t> perm(V);
  for (size_t i = 0; i < V; i++) perm[i] = i;
  std::sort(perm.begin(), perm.end(), [&](size_t x, size_t y) {
    return ndt::acc_pack(cell[x].x, cell[x].y, cell[x].z) < ndt::acc_pack(cell[y].x, cell[y].y, cell[y].z);
  });
  size_t touched = 0, removed = 0, points = 0;
  for (size_t o = 0; o < V; o++) {
    const size_t q = perm[o];
    cells[3 * o] = cell[q].x;
    cells[3 * o + 1] = cell[q].y;
    cells[3 * o + 2] = cell[q].z;
    misses[o] = mh[q];
    hit[o] = mh[V + q] ? 1 : 0;
    touched += mh[q] >= 1u;
    const bool goes = mh[q] >= static_cast<unsigned>(spec->min_rays) && !mh[V + q];
    removed += goes;
    if (!goes) points += static_cast<size_t>(cell[q].w);
  }
  if (call.total) {  // what a clearing would do
    h->ray_touched = touched;
    h->ray_removed = removed;
    h->ray_kept = V - removed;
    h->ray_points = points;
  }
  return NDT_OK;
}
ndt_status ndt_diag_target_clear_rays(ndt_handle h, size_t* rays_cast, size_t* rays_skipped, uint64_t* cells_visited, size_t* touched_voxels,
                                      size_t* removed_voxels, size_t* kept_voxels, size_t* kept_points, int* relinked, size_t* launches) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (rays_cast) *rays_cast = h->ray_cast;
  if (rays_skipped) *rays_skipped = h->ray_skipped;
  if (cells_visited) *cells_visited = h->ray_visited;
  if (touched_voxels) *touched_voxels = h->ray_touched;
  if (removed_voxels) *removed_voxels = h->ray_removed;
  if (kept_voxels) *kept_voxels = h->ray_kept;
  if (kept_points) *kept_points = h->ray_points;
  if (relinked) *relinked = h->ray_relinked;
  if (launches) *launches = h->ray_launches;
  return NDT_OK;
}
ndt_status ndt_host_ray_spec_check(const ndt_ray_spec* spec, float resolution) {
  if (!spec) return fail(NDT_ERR_INVALID, "null ray spec");
  if (const char* why = ndt::ray_spec_error(*spec, resolution)) return fail(NDT_ERR_INVALID, why);
  return NDT_OK;
}
ndt_status ndt_host_ray_cells(const float* origin, const float* point, float resolution, float margin, int* cells, size_t capacity, size_t* n) {
  if (!origin || !point || !n) return fail(NDT_ERR_INVALID, "bad arguments");
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(origin[k]) || !std::isfinite(point[k])) return fail(NDT_ERR_INVALID, "the origin and the point of a ray must be finite");
  if (!(std::isfinite(resolution) && resolution > 0.f)) return fail(NDT_ERR_INVALID, "the resolution must be finite and positive");
  if (!(std::isfinite(margin) && margin >= 0.f)) return fail(NDT_ERR_INVALID, "a ray's margin must be finite and >= 0");
  size_t seen = 0;
  const long long c = ndt::ray_walk(origin, point, static_cast<double>(resolution), static_cast<double>(margin), 0.0,
                                    std::numeric_limits<double>::infinity(), nullptr, [&](int i, int j, int k) {
                                      if (cells && seen < capacity) {
                                        cells[3 * seen] = i;
                                        cells[3 * seen + 1] = j;
                                        cells[3 * seen + 2] = k;
                                      }
                                      seen++;
                                    });
  *n = c < 0 ? 0 : static_cast<size_t>(c);
  if (cells && seen > capacity) return fail(NDT_ERR_INVALID, "the ray visits more cells than the buffer holds");
  return NDT_OK;
}
ndt_status ndt_host_ray_plan(size_t n_points, int* blocks, int* passes) {
  if (!blocks || !passes) return fail(NDT_ERR_INVALID, "bad arguments");
  if (n_points > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "more than INT_MAX points in one ray call");
  ndt::ray_plan(n_points, rays_max_blocks(), blocks, passes);
  return NDT_OK;
}

}  // extern "C"
