// ndt_grid.hip -- voxel grids: the pieces every cell-sorting caller shares (the scan-and-scatter half of the cell chain, the
// sort-built sparse index), the K1 target grid build (VoxelGridCovariance::filter) in its forms, record compaction, the counts
// and the search index of a built grid, the target setters and the grid inspection entry points.
#include "ndt_internal.hpp"

#include <type_traits>

namespace ndtc {

// (block_sums goes back to the caching pool at scope exit; the pool hands memory out again only to work queued on the same stream)
ndt_status chain_scan(hipStream_t st, unsigned* counters, long long n_cells, int min_pts, const ChainOut& o, unsigned* totals) {
  const int n_tiles = ndt::scan_tiles(n_cells);
  DevBuf<unsigned> block_sums;
  HIP_TRY(block_sums.reserve(static_cast<size_t>(n_tiles) * 3));
  HIP_TRY(ndt::launch_scan_reduce(counters, n_cells, min_pts, block_sums.p, n_tiles, st));
  HIP_TRY(ndt::launch_scan_blocks(block_sums.p, n_tiles, totals, st));
  HIP_TRY(ndt::launch_scan_apply(counters, n_cells, min_pts, block_sums.p, n_tiles, o.leaf_cell, o.leaf_start, o.leaf_count, o.leaf_rec, st));
  return NDT_OK;
}
ndt_status chain_scan_scatter(hipStream_t st, unsigned* counters, long long n_cells, int min_pts, const int* key, const unsigned* rank,
                              int n, const ChainOut& o, unsigned* totals) {
  if (ndt_status s = chain_scan(st, counters, n_cells, min_pts, o, totals)) return s;
  HIP_TRY(ndt::launch_scatter(key, rank, n, counters, o.sorted_idx, st));
  return NDT_OK;
}

ndt_status sparse_index(hipStream_t st, const float4* pts, int n, int dense, const ndt::GridGeom& geo, int min_pts, const ChainOut& o,
                        unsigned* counts) {
  const size_t tb = ndt::sparse_index_temp_bytes(n), m = static_cast<size_t>(n);
  DevBuf<unsigned char> temp;
  DevBuf<unsigned> w;  // keys_a, keys_b, flags, ord
  DevBuf<int> vals;
  HIP_TRY(temp.reserve(tb));
  HIP_TRY(w.reserve(4 * m));
  HIP_TRY(vals.reserve(m));
  HIP_TRY(ndt::launch_sparse_index(pts, n, dense, geo, min_pts, temp.p, tb, w.p, w.p + m, vals.p, w.p + 2 * m, w.p + 3 * m, o.leaf_cell,
                                   o.leaf_start, o.leaf_count, o.leaf_rec, o.sorted_idx, counts, st));
  return NDT_OK;  // (the temporaries go back to the stream's pool: reused only behind this launch)
}

static ndt_status compact_records_now(ndt_context* h, DeviceGrid* g);

// The first half of build_grid: the geometry of the cloud's grid hd.g and what its build needs.  hd.done: nothing to build
// (no point, no finite point, or the reference's overflow) -- hd.g is the finished (empty) grid.  A failure other than that
// overflow leaves hd.g null.
struct GridHead {
  std::shared_ptr<DeviceGrid> g;  // geometry set
  int n = 0;
  size_t max_leaves = 0, max_cand = 0;
  bool sparse = false, done = true;
};
static ndt_status grid_head(const std::shared_ptr<DeviceCloud>& cloud, const GridSpec& spec, GridHead& hd) {
  hd.done = true;
  if (!cloud) return fail(NDT_ERR_NO_INPUT, "no target");
  auto g = std::make_shared<DeviceGrid>();
  hd.g = g;
  g->target = cloud;
  g->resolution = spec.resolution;
  g->min_pts = spec.min_pts;
  g->eig_ratio = spec.eig_ratio;
  const int n = static_cast<int>(cloud->n);
  ndt::GridGeom& geo = g->geom;
  for (int k = 0; k < 3; k++) {
    geo.leaf[k] = spec.resolution;
    geo.inv_leaf[k] = 1.0f / spec.resolution;  // [PCL] VoxelGrid::setLeafSize
  }
  if (n == 0) return NDT_OK;
  const BBox bb = bbox_of(*cloud, spec.dense);  // computed during the upload: no kernel, no wait
  if (!(bb.mn[0] <= bb.mx[0])) return NDT_OK;  // no finite point at all
  const ndt::LatticeStatus ls = ndt::lattice_geometry(spec.resolution, bb.mn, bb.mx, geo);
  if (ls == ndt::kLatticeIndexOverflow)  // the reference warns and leaves an empty grid (:79-84)
    return fail(NDT_ERR_GRID_OVERFLOW, "leaf size is too small for the input dataset: integer indices would overflow");
  if (ls != ndt::kLatticeOk) {
    hd.g.reset();
    return fail(NDT_ERR_GRID_OVERFLOW, "voxel grid too large");
  }
  ndt::set_padded_lut(geo);
  hd.n = n;
  hd.max_leaves = std::min<size_t>(static_cast<size_t>(n), static_cast<size_t>(geo.n_cells));
  hd.max_cand = std::min<size_t>(hd.max_leaves, static_cast<size_t>(n) / static_cast<size_t>(std::max(1, spec.min_pts)) + 1);
  hd.sparse = !spec.index_only && ndt::wants_sparse_index(spec.voxel_index, geo.n_cells, n);
  hd.done = false;
  return NDT_OK;
}

// The form build_grid builds hd's dense table in (plan: the bucket plan).  The bucket form, its cells dealt to the buckets in
// short runs (k1_bucket), is the faster one for every cloud shape measured, uniform to heavily clustered (tools/time_k1_forms.py);
// NDT_K1=old: the general chain, kept for index-only builds -- GICP's search index -- and as the cross-check of tools/fuzz_grid.py.
enum K1Form { K1_CHAIN, K1_BUCKETS, K1_SMALL };
static K1Form k1_form(const GridSpec& spec, const GridHead& hd, ndt::GridBuildPlan& plan) {
  static const bool chain_only = [] { const char* v = getenv("NDT_K1"); return v && std::strcmp(v, "old") == 0; }();
  static const bool small_on = [] { const char* v = getenv("NDT_K1_SMALL"); return !v || atoi(v) != 0; }();
  if (hd.sparse || chain_only || spec.index_only || !ndt::grid_build_plan(hd.g->geom.n_cells, hd.n, plan)) return K1_CHAIN;
  return small_on && ndt::grid_build_small_applies(hd.n, plan) ? K1_SMALL : K1_BUCKETS;
}
// NDT_K1_STAMPS=1: the bucket form's phase clocks on stderr (development aid)
static bool k1_stamps_on() { static const bool on = [] { const char* v = getenv("NDT_K1_STAMPS"); return v && atoi(v) != 0; }(); return on; }

// What every form of the build writes into: the grid's counts -- [points binned, occupied voxels, candidate voxels (>= min_pts),
// valid voxels, points in crowded cells] -- and its leaf arrays, sized for the worst case.
static hipError_t reserve_leaves(const GridHead& hd) {
  DeviceGrid* g = hd.g.get();
  for (hipError_t e : {g->counts.reserve(8), g->leaf_cell.reserve(hd.max_leaves), g->leaf_start.reserve(hd.max_leaves), g->leaf_count.reserve(hd.max_leaves),
                       g->leaf_rec.reserve(hd.max_leaves), g->sorted_idx.reserve(static_cast<size_t>(hd.n))})
    if (e != hipSuccess) return e;
  return hipSuccess;
}
static ChainOut chain_out(const DeviceGrid* g) { return ChainOut{g->leaf_cell.p, g->leaf_start.p, g->leaf_count.p, g->leaf_rec.p, g->sorted_idx.p}; }

// A bucket-form build of hd's cloud with the bucket plan `plan`: the grid's buffers (scratch: the finish's [5 n] words) and
// state as the build leaves it, and for the one-launch form (k1_small; many targets: k1_small_multi) the launch in *D (*lds: its
// dynamic LDS; multi: k1_small_multi's lists).
static ndt_status setup_bucket_form(const GridSpec& spec, const GridHead& hd, const ndt::GridBuildPlan& plan, DevBuf<unsigned>& scratch,
                                    ndt::SmallBuildDesc* D, size_t* lds, bool multi) {
  DeviceGrid* g = hd.g.get();
  const size_t n = static_cast<size_t>(hd.n), K = static_cast<size_t>(plan.n_buckets);
  const size_t rec_slots = n / static_cast<size_t>(std::max(1, spec.min_pts)) + 1;  // slot = segment start / min_pts
  HIP_TRY(reserve_leaves(hd));
  HIP_TRY(g->lut.reserve(static_cast<size_t>(g->geom.lut_cells)));
  HIP_TRY(g->recs.reserve(rec_slots));
  HIP_TRY(g->centroids.reserve(rec_slots));
  HIP_TRY(g->bucket_base.reserve(2 * K + 1));  // [K + 1] bucket bases, [K] valid voxels per bucket
  HIP_TRY(g->bpts.reserve(n));
  HIP_TRY(scratch.reserve(5 * n));
  g->plan = plan;
  g->build_form = D ? 3 : 2;
  g->leaves_pending = true;  // leaf arrays and the occupied / candidate counts: on demand (grid_counts)
  g->counts_known = false;
  g->empty = false;
  if (!D) return NDT_OK;
  if (!ndt::small_build_desc(hd.n, plan, multi, *D, lds)) return fail(NDT_ERR_HIP, "one-launch grid build: the finish's LDS does not fit");
  D->pts = g->target->pts.p;
  D->dense = spec.dense;
  D->g = g->geom;
  D->min_pts = spec.min_pts;
  D->eig_ratio = spec.eig_ratio;
  D->bucket_base = g->bucket_base.p;
  D->bpts = g->bpts.p;
  D->sorted_idx = g->sorted_idx.p;
  D->recs = g->recs.p;
  D->centroids = g->centroids.p;
  D->lut = g->lut.p;
  D->scratch = scratch.p;
  D->counts = g->counts.p;
  return NDT_OK;
}

// NDT_K1_STAMPS: the bucket form's phase clocks, per phase the median and the maximum over the buckets / blocks (shader cycles)
static ndt_status print_k1_stamps(ndt_context* h, const unsigned long long* stamps, const ndt::GridBuildPlan& plan, bool small_form) {
  const size_t K = static_cast<size_t>(plan.n_buckets);
  std::vector<unsigned long long> hst(8 * K);
  HIP_TRY(hipMemcpyAsync(hst.data(), stamps, 8 * K * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  static const char* names[8] = {"load+rank", "scans+select", "place", "teams", "sums+finish", "passes", "points", "total"};
  std::fprintf(stderr, "[k1_finalize clocks, %zu buckets] ", K);
  for (int q = 0; q < 8; q++) {
    std::vector<unsigned long long> d;
    for (size_t b = 0; b < K; b++)
      if (hst[8 * b + 7]) d.push_back(hst[8 * b + q]);
    if (d.empty()) continue;
    std::sort(d.begin(), d.end());
    std::fprintf(stderr, "%s %llu/%llu  ", names[q], d[d.size() / 2], d.back());
  }
  std::fprintf(stderr, "\n");
  if (small_form) {  // k1_small: cycles from the block's start to the end of the scan / the publication / the end
    std::vector<unsigned long long> hk(4 * K);
    HIP_TRY(hipMemcpy(hk.data(), stamps + 8 * K, 4 * K * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[k1_small clocks, %zu blocks, cycles since the block's start: scan / published / end] ", K);
    for (int q = 1; q < 4; q++) {
      std::vector<unsigned long long> d;
      for (size_t b = 0; b < K; b++) d.push_back(hk[4 * b + q] - hk[4 * b]);
      std::sort(d.begin(), d.end());
      std::fprintf(stderr, "%llu/%llu  ", d[d.size() / 2], d.back());
    }
    unsigned long long t_lo = ~0ull, t_hi = 0;
    for (size_t b = 0; b < K; b++) { t_lo = std::min(t_lo, hk[4 * b]); t_hi = std::max(t_hi, hk[4 * b + 3]); }
    std::fprintf(stderr, " first start -> last end %llu\n", t_hi - t_lo);
  }
  const size_t B = small_form ? 0 : static_cast<size_t>(plan.n_blocks);
  std::vector<unsigned long long> hs(8 * B + 1);
  HIP_TRY(hipMemcpy(hs.data(), stamps + 8 * K, 8 * B * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (B) std::fprintf(stderr, "[k1_scatter clocks, %zu blocks, cycles since the block's start: tables / ranks / column scan / stores] ", B);
  for (int q = 1; q < 5; q++) {
    std::vector<unsigned long long> d;
    for (size_t bq = 0; bq < B; bq++)
      if (hs[8 * bq] && hs[8 * bq + q]) d.push_back(hs[8 * bq + q] - hs[8 * bq]);
    if (d.empty()) continue;
    std::sort(d.begin(), d.end());
    std::fprintf(stderr, "%llu/%llu  ", d[d.size() / 2], d.back());
  }
  std::fprintf(stderr, "\n");
  return NDT_OK;
}

// VoxelGridCovariance::filter(true) on the GPU.
ndt_status build_grid(ndt_context* h, const std::shared_ptr<DeviceCloud>& cloud, const GridSpec& spec, std::shared_ptr<DeviceGrid>& out) {
  GridHead hd;
  ndt_status hs = grid_head(cloud, spec, hd);
  if (hs || hd.done) {
    if (hd.g) out = hd.g;  // the empty grid (no point, no finite point, the reference's overflow)
    return hs;
  }
  const std::shared_ptr<DeviceGrid> g = hd.g;
  const int n = hd.n;
  const float4* pts = cloud->pts.p;
  ndt::GridGeom& geo = g->geom;
  const size_t max_leaves = hd.max_leaves, max_cand = hd.max_cand;
  hipStream_t st = h->stream;
  if (hd.sparse) {
    const size_t rec_slots = static_cast<size_t>(n) / static_cast<size_t>(std::max(1, spec.min_pts)) + 1;  // slot = segment start / min_pts
    HIP_TRY(reserve_leaves(hd));
    HIP_TRY(g->recs.reserve(rec_slots));
    HIP_TRY(g->centroids.reserve(rec_slots));
    int bits = 10;
    while ((static_cast<size_t>(1) << bits) < 2 * rec_slots) bits++;
    geo.hash_bits = bits;
    HIP_TRY(g->lut.reserve(static_cast<size_t>(2) << bits));  // int2 slots
    HIP_TRY(hipMemsetAsync(g->lut.p, 0xFF, (static_cast<size_t>(2) << bits) * sizeof(int), st));
    if ((hs = sparse_index(st, pts, n, spec.dense, geo, spec.min_pts, chain_out(g.get()), g->counts.p))) return hs;
    ndt::FinalizeDump nodump{nullptr, nullptr, nullptr, nullptr, nullptr};
    DevBuf<float4> big_pts;
    HIP_TRY(big_pts.reserve(n));
    HIP_TRY(ndt::launch_finalize(pts, g->leaf_cell.p, g->leaf_start.p, g->leaf_count.p, g->leaf_rec.p, static_cast<int>(max_leaves),
                                 g->sorted_idx.p, spec.min_pts, spec.eig_ratio, g->recs.p, g->centroids.p, g->lut.p, geo, g->counts.p + 3, nodump, st,
                                 g->counts.p, big_pts.p));
    g->counts_known = false;
    g->empty = false;
    g->build_form = 4;
    out = g;
    return NDT_OK;
  }
  ndt::GridBuildPlan plan{};
  const K1Form form = k1_form(spec, hd, plan);
  if (form != K1_CHAIN) {
    // ---- bucket form (ndt_kernels.hip "K1, bucket form"): no per-point global atomic, per-voxel work staged through LDS
    const size_t K = static_cast<size_t>(plan.n_buckets);
    DevBuf<unsigned> cntmat, order;
    DevBuf<unsigned long long> stamps;
    if (k1_stamps_on()) {
      HIP_TRY(stamps.reserve(8 * (K + std::max(K, static_cast<size_t>(plan.n_blocks)))));
      HIP_TRY(hipMemsetAsync(stamps.p, 0, 8 * (K + std::max(K, static_cast<size_t>(plan.n_blocks))) * sizeof(unsigned long long), st));
    }
    ndt::SmallBuildDesc D{};
    size_t lds = 0;
    hs = setup_bucket_form(spec, hd, plan, order, form == K1_SMALL ? &D : nullptr, &lds, false);
    if (hs) return hs;
    if (form == K1_SMALL) {
      HIP_TRY(ndt::launch_grid_build_small(D, lds, stamps.p, st));
    } else {
      HIP_TRY(cntmat.reserve((static_cast<size_t>(plan.n_blocks) + 1) * K));
      static const bool index_form_env = [] { const char* v = getenv("NDT_K1_INDEX"); return v && atoi(v) != 0; }();
      const ndt::GridBuildScratch S{cntmat.p, g->bucket_base.p, g->bpts.p, order.p, stamps.p, index_form_env};
      HIP_TRY(ndt::launch_grid_build_buckets(pts, n, spec.dense, geo, plan, spec.min_pts, spec.eig_ratio, S, g->sorted_idx.p,
                                             g->recs.p, g->centroids.p, g->lut.p, g->counts.p, st));
      g->index_form = S.index_form;
    }
    // Records dense and in ascending cell order (maybe_compact_records: two small launches, ~13 us) pay for themselves as
    // soon as a few scans are registered against the grid: +8 % on lock-step batches, +1-5 % on a single 100k-point scan.
    // A mapping node registers ONE scan against every target it builds (ndt_omp_mapping_node.cpp:151-169), so the build
    // itself leaves k1_finalize's numbering and the compaction runs when the grid is seen to be reused: before the second
    // registration against it, or before the first lock-step batch (NDT_K1_COMPACT=eager: at once, as round 2 did; off: never).
    // The mapping nodes' 16 k-point clouds (records that fit L2 many times over) never compact.
    static const int compact_mode = [] { const char* v = getenv("NDT_K1_COMPACT"); return !v ? 1 : std::strcmp(v, "eager") == 0 ? 2 : std::strcmp(v, "off") == 0 ? 0 : 1; }();
    g->compact_pending = n > 65536 && compact_mode != 0;
    if (k1_stamps_on() && (hs = print_k1_stamps(h, stamps.p, plan, form == K1_SMALL))) return hs;
    if (compact_mode == 2 && g->compact_pending) {
      ndt_status cs = compact_records_now(h, g.get());
      if (cs) return cs;
    }
  } else {
  // every cell of the padded table starts out empty (kLutEmpty = -1 = all bits set); the finalize pass fills in the
  // voxels that reached min_points_per_voxel
  g->build_form = 1;
  HIP_TRY(reserve_leaves(hd));
  HIP_TRY(g->lut.reserve(static_cast<size_t>(geo.lut_cells)));
  HIP_TRY(hipMemsetAsync(g->lut.p, 0xFF, static_cast<size_t>(geo.lut_cells) * sizeof(int), st));
  HIP_TRY(g->recs.reserve(max_cand));
  HIP_TRY(g->centroids.reserve(max_cand));
  // ---- count
  DevBuf<unsigned> cell_count, rank;
  DevBuf<int> key;
  HIP_TRY(cell_count.reserve(static_cast<size_t>(geo.n_cells)));
  HIP_TRY(key.reserve(n));
  HIP_TRY(rank.reserve(n));
  HIP_TRY(hipMemsetAsync(cell_count.p, 0, static_cast<size_t>(geo.n_cells) * sizeof(unsigned), st));
  HIP_TRY(ndt::launch_count(pts, n, spec.dense, geo, key.p, rank.p, cell_count.p, st));
  // ---- scan + scatter.  The counts stay on the device: the host fetches the four numbers only if somebody asks
  // (grid_counts()).  Two host round trips (~30 us each) less per target; nothing below waits for the GPU.
  if ((hs = chain_scan_scatter(st, cell_count.p, geo.n_cells, spec.min_pts, key.p, rank.p, n, chain_out(g.get()), g->counts.p))) return hs;
  // ---- finalize
  HIP_TRY(hipMemsetAsync(g->counts.p + 3, 0, 2 * sizeof(unsigned), st));
  ndt::FinalizeDump nodump{nullptr, nullptr, nullptr, nullptr, nullptr};
  DevBuf<float4> big_pts;  // scratch of the crowded-leaf path (k_presort_large)
  if (!spec.index_only) {
    HIP_TRY(big_pts.reserve(n));
    HIP_TRY(ndt::launch_finalize(pts, g->leaf_cell.p, g->leaf_start.p, g->leaf_count.p, g->leaf_rec.p,
                                 static_cast<int>(max_leaves), g->sorted_idx.p, spec.min_pts, spec.eig_ratio, g->recs.p, g->centroids.p,
                                 g->lut.p, geo, g->counts.p + 3, nodump, st, g->counts.p, big_pts.p));
  }
  }
  // the temporaries (cell_count, key, rank) go back to the caching pool at scope exit; the
  // pool hands memory out again only to work queued on the same stream, i.e. after these kernels
  g->counts_known = false;
  g->empty = false;
  out = g;
  return NDT_OK;
}

ndt_status build_grids(ndt_context* h, const std::vector<std::shared_ptr<DeviceCloud>>& targets, int is_dense,
                       std::vector<std::shared_ptr<DeviceGrid>>& out, size_t* n_small) {
  const GridSpec spec = grid_spec_of(h, is_dense);
  out.assign(targets.size(), nullptr);
  std::vector<ndt::SmallBuildDesc> descs;
  std::vector<std::unique_ptr<DevBuf<unsigned>>> scratch;  // per small target: [5 n] (back to the pool behind the launch)
  int max_K = 0;
  size_t lds = 0;
  ndt_status s = NDT_OK;
  for (size_t i = 0; i < targets.size(); i++) {
    GridHead hd;
    s = grid_head(targets[i], spec, hd);
    if (s) return s;
    out[i] = hd.g;
    if (hd.done) continue;
    // the one-launch form where build_grid takes it; stamped builds (development aid) through build_grid
    ndt::GridBuildPlan plan{};
    if (k1_stamps_on() || k1_form(spec, hd, plan) != K1_SMALL) {
      s = build_grid(h, targets[i], spec, out[i]);
      if (s) return s;
      continue;
    }
    size_t lds_i = 0;
    s = setup_bucket_form(spec, hd, plan, *scratch.emplace_back(new DevBuf<unsigned>()), &descs.emplace_back(), &lds_i, true);
    if (s) return s;
    max_K = std::max(max_K, plan.n_buckets);
    lds = std::max(lds, lds_i);
  }
  *n_small = descs.size();
  if (descs.empty()) return NDT_OK;
  DevBuf<ndt::SmallBuildDesc> d_descs;
  HIP_TRY(d_descs.reserve(descs.size()));
  HIP_TRY(hipMemcpyAsync(d_descs.p, descs.data(), descs.size() * sizeof(ndt::SmallBuildDesc), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(ndt::launch_grid_build_small_multi(d_descs.p, static_cast<int>(descs.size()), max_K, lds, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));  // (`descs` is pageable: the copy has read it)
  return NDT_OK;
}

// Records of a bucket-form build -> dense, ascending cell order (launch_compact_records), in place: only while this handle is
// the grid's single holder (a clone may be evaluating on it) and before anybody has asked for the leaf arrays (they quote
// record numbers).  eager: now; otherwise from the second registration against the grid on.
static ndt_status compact_records_now(ndt_context* h, DeviceGrid* g) {
  g->compact_pending = false;
  if (!g->leaves_pending || g->empty) return NDT_OK;
  const size_t rec_slots = g->recs.cap;
  DevBuf<ndt::VoxelRec> recs_new;
  DevBuf<ndt::VoxelSide> cent_new;
  DevBuf<unsigned> tile_sums;
  HIP_TRY(recs_new.reserve(rec_slots));
  HIP_TRY(cent_new.reserve(rec_slots));
  HIP_TRY(tile_sums.reserve(ndt::record_compaction_tiles(g->geom.lut_cells) + 1));
  HIP_TRY(ndt::launch_compact_records(g->lut.p, g->geom.lut_cells, g->recs.p, g->centroids.p, recs_new.p, cent_new.p, tile_sums.p, h->stream));
  g->recs.swap(recs_new);  // (the old arrays go back to the pool at scope exit: reused only behind these launches, stream order)
  g->centroids.swap(cent_new);
  g->generation++;  // (the records are renumbered: whoever cached record numbers reads the table again)
  return NDT_OK;
}
ndt_status maybe_compact_records(ndt_context* h, bool eager) {
  DeviceGrid* g = h->grid.get();
  if (!g || !g->compact_pending) return NDT_OK;
  if (!eager && g->n_registrations++ == 0) return NDT_OK;
  if (h->grid.use_count() != 1) {  // shared with a clone: leave it alone for good
    g->compact_pending = false;
    return NDT_OK;
  }
  return compact_records_now(h, g);
}

// The counts and the search index of a built grid in three pieces (the caller holds g->fit_mu and does the waiting).
// A bucket-form build numbers its leaves only now that somebody wants them: the numbering queued; `scratch` lives until the
// stream has been waited for.
static ndt_status queue_grid_leaves(ndt_context* h, DeviceGrid* g, DevBuf<unsigned>& scratch) {
  HIP_TRY(scratch.reserve(4 * static_cast<size_t>(g->plan.n_buckets) + 4));
  HIP_TRY(ndt::launch_grid_leaves(g->geom, g->plan, g->min_pts, g->bpts.p, g->bucket_base.p, scratch.p, g->leaf_cell.p, g->leaf_start.p,
                                  g->leaf_count.p, g->leaf_rec.p, g->counts.p, g->lut.p, h->stream, g->index_form ? g->target->pts.p : nullptr));
  return NDT_OK;
}
// the four counts fetched behind a wait (and so behind the numbering, whose inputs go back to the pool)
static void adopt_counts(DeviceGrid* g, const unsigned* c) {
  if (g->leaves_pending) {
    g->leaves_pending = false;
    g->bpts.release();
    g->bucket_base.release();
  }
  g->n_sorted = c[0];
  g->n_leaves = c[1];
  g->n_cand = c[2];
  g->n_valid = c[3];
  g->counts_known = true;
}
// cell -> segment of the points in cell order, occupied x-rows (the nearest-neighbour searches walk them), queued
static ndt_status queue_cell_index(ndt_context* h, DeviceGrid* g) {
  HIP_TRY(g->cell_range.reserve(static_cast<size_t>(g->geom.n_cells)));
  HIP_TRY(hipMemsetAsync(g->cell_range.p, 0, static_cast<size_t>(g->geom.n_cells) * sizeof(uint2), h->stream));
  const size_t n_rows = static_cast<size_t>(g->geom.div_b[1]) * static_cast<size_t>(g->geom.div_b[2]);
  HIP_TRY(g->row_any.reserve(n_rows));
  HIP_TRY(hipMemsetAsync(g->row_any.p, 0, n_rows * sizeof(int), h->stream));
  HIP_TRY(ndt::launch_cell_ranges(g->leaf_cell.p, g->leaf_start.p, g->leaf_count.p, static_cast<int>(g->n_leaves), g->cell_range.p,
                                  g->geom.div_b[0], g->row_any.p, h->stream));
  HIP_TRY(g->cell_pts.reserve(g->target->n));
  HIP_TRY(ndt::launch_gather_points(g->target->pts.p, g->sorted_idx.p, g->counts.p, static_cast<int>(g->target->n), g->cell_pts.p,
                                    h->stream));
  return NDT_OK;
}

// occupied / candidate / valid voxel counts of a built grid (fetched from the device on first use)
ndt_status grid_counts(ndt_context* h, DeviceGrid* g) {
  if (g->counts_known || g->empty) return NDT_OK;
  if (g->accumulated) return acc_grid_counts(h, g);
  std::lock_guard<std::mutex> lock(g->fit_mu);
  if (g->counts_known) return NDT_OK;
  DevBuf<unsigned> scratch;
  if (g->leaves_pending) {
    if (ndt_status s = queue_grid_leaves(h, g, scratch)) return s;
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  unsigned c[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(c, g->counts.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  adopt_counts(g, c);
  return NDT_OK;
}

// the search index of a built grid, built on first use
ndt_status ensure_cell2leaf(ndt_context* h, DeviceGrid* g) {
  std::lock_guard<std::mutex> lock(g->fit_mu);
  if (!g->have_cell2leaf) {
    if (ndt_status s = queue_cell_index(h, g)) return s;
    HIP_TRY(hipStreamSynchronize(h->stream));
    g->have_cell2leaf = true;
  }
  return NDT_OK;
}
// grid_counts + ensure_cell2leaf of many grids (getFitnessScore of many members): every counts read-back (with the leaf
// numbering of a bucket-form build) queued, one wait; then every missing index queued, one wait -- two synchronisations
// in all instead of up to two per grid.  The tables and flags are those of the single-grid calls, which find the work done.
// The grids are locked in address order (fit_mu), so two callers that share grids cannot deadlock.
ndt_status ensure_indices(ndt_context* h, const std::vector<DeviceGrid*>& grids) {
  std::vector<DeviceGrid*> gs;
  for (DeviceGrid* g : grids)
    if (g && !g->empty) gs.push_back(g);
  std::sort(gs.begin(), gs.end());
  gs.erase(std::unique(gs.begin(), gs.end()), gs.end());
  std::vector<std::unique_lock<std::mutex>> locks;
  locks.reserve(gs.size());
  for (DeviceGrid* g : gs) locks.emplace_back(g->fit_mu);
  std::vector<DeviceGrid*> need;
  for (DeviceGrid* g : gs)
    if (!g->counts_known) need.push_back(g);
  if (!need.empty()) {
    ndt_status s = ensure_host_rows(h, (4 * need.size() * sizeof(unsigned) + sizeof(double) * ndt::kEvalStride - 1) /
                                           (sizeof(double) * ndt::kEvalStride));
    if (s) return s;
    unsigned* c = reinterpret_cast<unsigned*>(h->host_result);
    std::vector<std::unique_ptr<DevBuf<unsigned>>> scratch;  // (kept until the wait)
    for (size_t i = 0; i < need.size(); i++) {
      DeviceGrid* g = need[i];
      if (g->leaves_pending && (s = queue_grid_leaves(h, g, *scratch.emplace_back(new DevBuf<unsigned>())))) return s;
      HIP_TRY(hipMemcpyAsync(c + 4 * i, g->counts.p, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < need.size(); i++) adopt_counts(need[i], c + 4 * i);
  }
  bool queued = false;
  for (DeviceGrid* g : gs) {
    if (g->have_cell2leaf || g->n_sorted == 0) continue;  // (nothing to search: fitness_impl builds no index either)
    if (ndt_status s = queue_cell_index(h, g)) return s;
    queued = true;
  }
  if (queued) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (DeviceGrid* g : gs)
      if (g->n_sorted) g->have_cell2leaf = true;
  }
  return NDT_OK;
}

// slack of the shell bound: the build-time and search-time cell indices of a coordinate can differ
// at cell borders by rounding (SURVEY 8a trap 2) -- a few ulps of the largest coordinate
float index_slack(const DeviceGrid* g) {
  float max_abs = 0.f;
  for (int k = 0; k < 3; k++)
    max_abs = std::max(max_abs, std::max(std::fabs(g->geom.min_b[k] * g->geom.leaf[k]), std::fabs((g->geom.max_b[k] + 1) * g->geom.leaf[k])));
  return 1e-3f * g->resolution + 4e-6f * max_abs;
}
// the search structure over a built grid's target (after ensure_cell2leaf + grid_counts)
void fill_point_index(const DeviceGrid* g, ndt::PointIndex& ix) {
  ix.pts = g->target->pts.p;
  ix.n = static_cast<int>(g->target->n);
  ix.geom = g->geom;
  ix.cell_range = g->cell_range.p;
  ix.row_any = g->row_any.p;
  ix.sorted_idx = g->sorted_idx.p;
  ix.sorted_pts = g->cell_pts.p;
  ix.n_sorted = static_cast<int>(g->n_sorted);
  ix.slack = index_slack(g);
}

ndt_status grid_size(ndt_context* h, DeviceGrid* g, size_t* n_leaves, size_t* n_valid) {
  if (!g->empty) {
    ndt_status s = ensure_device(h);
    if (!s) s = grid_counts(h, g);
    if (s) return s;
  }
  if (n_leaves) *n_leaves = g->n_leaves;
  if (n_valid) *n_valid = g->n_valid;
  return NDT_OK;
}

void grid_info(const DeviceGrid* g, int* min_b, int* max_b, int* div_b) {
  for (int k = 0; k < 3; k++) {
    if (min_b) min_b[k] = g->geom.min_b[k];
    if (max_b) max_b[k] = g->geom.max_b[k];
    if (div_b) div_b[k] = g->geom.div_b[k];
  }
}

// Re-runs the finalize pass in dump mode (the records and LUT it rewrites are
// bit-identical, so sharing handles stay valid).
ndt_status grid_dump(ndt_context* h, DeviceGrid* g, int64_t* idx, int* nr_points, double* mean, double* cov, double* icov,
                     double* evals) {
  if (g->accumulated) return acc_grid_dump(h, idx, nr_points, mean, cov, icov, evals);
  if (!g->empty) {
    ndt_status sc = ensure_device(h);
    if (!sc) sc = grid_counts(h, g);
    if (sc) return sc;
  }
  const size_t V = g->n_leaves;
  if (V == 0) return NDT_OK;
  ndt_status s = ensure_device(h);
  if (s) return s;
  DevBuf<int> d_n;
  DevBuf<double> d_mean, d_cov, d_icov, d_evals;
  DevBuf<unsigned> d_cnt;
  HIP_TRY(d_n.reserve(V));
  HIP_TRY(d_mean.reserve(V * 3));
  HIP_TRY(d_cov.reserve(V * 9));
  HIP_TRY(d_icov.reserve(V * 9));
  HIP_TRY(d_evals.reserve(V * 3));
  HIP_TRY(d_cnt.reserve(1));
  HIP_TRY(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned), h->stream));
  ndt::FinalizeDump dump{d_n.p, d_mean.p, d_cov.p, d_icov.p, d_evals.p};
  HIP_TRY(ndt::launch_finalize(g->target->pts.p, g->leaf_cell.p, g->leaf_start.p, g->leaf_count.p, g->leaf_rec.p,
                               static_cast<int>(V), g->sorted_idx.p, g->min_pts, g->eig_ratio, g->recs.p, g->centroids.p, g->lut.p,
                               g->geom, d_cnt.p, dump, h->stream));
  std::vector<int> cell(V);
  HIP_TRY(hipMemcpyAsync(cell.data(), g->leaf_cell.p, V * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (nr_points) HIP_TRY(hipMemcpyAsync(nr_points, d_n.p, V * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (mean) HIP_TRY(hipMemcpyAsync(mean, d_mean.p, V * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (cov) HIP_TRY(hipMemcpyAsync(cov, d_cov.p, V * 9 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (icov) HIP_TRY(hipMemcpyAsync(icov, d_icov.p, V * 9 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (evals) HIP_TRY(hipMemcpyAsync(evals, d_evals.p, V * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  // ascending voxel index, the order of the reference's std::map (a bucket-form build numbers its leaves bucket by bucket)
  bool ascending = true;
  for (size_t i = 1; i < V && ascending; i++) ascending = cell[i - 1] < cell[i];
  if (!ascending) {
    std::vector<size_t> perm(V);
    for (size_t i = 0; i < V; i++) perm[i] = i;
    std::sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return cell[a] < cell[b]; });
    auto apply = [&](auto* arr, size_t width) {
      if (!arr) return;
      using T = std::remove_pointer_t<decltype(arr)>;
      std::vector<T> tmp(arr, arr + V * width);
      for (size_t i = 0; i < V; i++) std::copy(tmp.begin() + perm[i] * width, tmp.begin() + (perm[i] + 1) * width, arr + i * width);
    };
    apply(nr_points, 1);
    apply(mean, 3);
    apply(cov, 9);
    apply(icov, 9);
    apply(evals, 3);
    std::vector<int> sorted_cell(V);
    for (size_t i = 0; i < V; i++) sorted_cell[i] = cell[perm[i]];
    cell.swap(sorted_cell);
  }
  if (idx)
    for (size_t i = 0; i < V; i++) idx[i] = cell[i];
  return NDT_OK;
}

}  // namespace ndtc

extern "C" {

static ndt_status set_target_impl(ndt_handle h, const void* pts, size_t n, size_t stride, int is_dense, bool on_device, bool by_ref = false) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  std::shared_ptr<DeviceCloud> c;
  ndt_status s = upload_cloud(h, pts, n, stride, on_device, c, by_ref);
  if (s) return s;
  h->target = c;
  h->target_dense = is_dense ? 1 : 0;
  return build_grid(h, c, grid_spec_of(h, is_dense), h->grid);  // init(), ndt_omp.h:276-283
}
ndt_status ndt_set_input_target(ndt_handle h, const void* pts, size_t n, size_t stride, int is_dense) {
  return set_target_impl(h, pts, n, stride, is_dense, false);
}
ndt_status ndt_set_input_target_device(ndt_handle h, const void* pts, size_t n, size_t stride, int is_dense) {
  return set_target_impl(h, pts, n, stride, is_dense, true);
}
ndt_status ndt_set_input_target_device_ref(ndt_handle h, const void* d_pts, size_t n, int is_dense) {
  return set_target_impl(h, d_pts, n, sizeof(float4), is_dense, true, true);
}

ndt_status ndt_set_voxel_index(ndt_handle h, int mode) {
  if (!h || mode < 0 || mode > 2) return fail(NDT_ERR_INVALID, "bad arguments");
  h->voxel_index = mode;
  return NDT_OK;
}

// the target cloud and its built grid, shared like the source above: a prep handle (side partition) builds the next target
// while the registration handle works; no copy, no rebuild
ndt_status ndt_share_input_target(ndt_handle dst, ndt_handle src) {
  if (!dst || !src) return fail(NDT_ERR_INVALID, "null handle");
  if (!src->target || !src->grid) return fail(NDT_ERR_NO_INPUT, "the donor handle has no input target");
  if (dst == src) return NDT_OK;
  if (src->grid->accumulated)
    return fail(NDT_ERR_INVALID, "an accumulated target cannot be shared: its grid changes in place and belongs to one handle");
  if (dst->device != src->device) return fail(NDT_ERR_INVALID, "handles on different devices");
  HIP_TRY(hipSetDevice(src->device));
  if (src->device_ready) HIP_TRY(hipStreamSynchronize(src->stream));  // the grid may still be under construction there
  ndt_status s = ensure_device(dst);
  if (s) return s;
  HIP_TRY(hipStreamSynchronize(dst->stream));
  dst->target = src->target;
  dst->target_dense = src->target_dense;
  dst->grid = src->grid;
  dst->resolution = src->grid->resolution;  // the grid's parameters come with it (the Gauss constants follow the resolution)
  dst->min_pts = src->grid->min_pts;
  dst->eig_ratio = src->grid->eig_ratio;
  return NDT_OK;
}

ndt_status ndt_set_input_target_cloud(ndt_handle h, ndt_cloud c, int is_dense) {
  if (!h || !c) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = ensure_device(h);
  if (!s) s = cloud_use_on(h, c->c.get());
  if (s) return s;
  h->target = c->c;
  h->target_dense = is_dense ? 1 : 0;
  return build_grid(h, h->target, grid_spec_of(h, is_dense), h->grid);
}
ndt_status ndt_promote_source_to_target(ndt_handle h, int is_dense) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!h->source) return fail(NDT_ERR_NO_INPUT, "no input source to promote");
  ndt_status s = ensure_device(h);
  if (s) return s;
  // the resident points and their boxes: no upload, no repack, no bounding-box pass (a view made for ordering: its parent)
  h->target = h->source->parent ? h->source->parent : h->source;
  h->target_dense = is_dense ? 1 : 0;
  return build_grid(h, h->target, grid_spec_of(h, is_dense), h->grid);
}

ndt_status ndt_host_lattice(float leaf, const float* mn, const float* mx, int* min_b, int* max_b, int* div_b, long long* n_cells,
                            int voxel_index, long long n_points, int* sparse) {
  if (!mn || !mx || !(leaf > 0)) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt::GridGeom geo{};
  if (ndt::lattice_geometry(leaf, mn, mx, geo) != ndt::kLatticeOk)
    return fail(NDT_ERR_GRID_OVERFLOW, "leaf size is too small for the box: integer indices would overflow");
  for (int k = 0; k < 3; k++) {
    if (min_b) min_b[k] = geo.min_b[k];
    if (max_b) max_b[k] = geo.max_b[k];
    if (div_b) div_b[k] = geo.div_b[k];
  }
  if (n_cells) *n_cells = geo.n_cells;
  if (sparse) *sparse = ndt::wants_sparse_index(voxel_index, geo.n_cells, n_points) ? 1 : 0;
  return NDT_OK;
}

// the host side of a build's plan: what build_grid, the bucket launches and the record compaction would decide
ndt_status ndt_host_grid_plan(long long n_cells, long long n_points, const int* div_b, int* bucket_form, int* n_buckets, int* cells_per_bucket,
                              int* pts_per_block, int* n_blocks, int* one_launch, int* wmax, int* lds_cap, long long* lut_cells,
                              int* compact_items, long long* compact_tiles, int* compact_prefix, int* filter_buckets, int* filter_chunks) {
  if (n_cells < 0 || n_points < 0 || n_points > 0x7fffffffll) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt::GridBuildPlan plan{};
  const bool ok = ndt::grid_build_plan(n_cells, static_cast<int>(n_points), plan);
  const ndt::K1FinishLds F = ok ? ndt::grid_build_finish_lds(plan.cells_per_bucket) : ndt::K1FinishLds{};
  if (bucket_form) *bucket_form = ok ? 1 : 0;
  if (n_buckets) *n_buckets = ok ? plan.n_buckets : 0;
  if (cells_per_bucket) *cells_per_bucket = ok ? plan.cells_per_bucket : 0;
  if (pts_per_block) *pts_per_block = ok ? plan.pts_per_block : 0;
  if (n_blocks) *n_blocks = ok ? plan.n_blocks : 0;
  if (one_launch) *one_launch = ok && ndt::grid_build_small_applies(static_cast<int>(n_points), plan) ? 1 : 0;
  if (wmax) *wmax = F.wmax;
  if (lds_cap) *lds_cap = F.lds_cap;
  long long lc = 0;
  if (div_b) {
    if (div_b[0] <= 0 || div_b[1] <= 0 || div_b[2] <= 0) return fail(NDT_ERR_INVALID, "bad arguments");
    ndt::GridGeom geo{};
    for (int k = 0; k < 3; k++) {
      geo.div_b[k] = div_b[k];
      geo.leaf[k] = 1.0f;
    }
    ndt::set_padded_lut(geo);
    lc = geo.lut_cells;
  }
  if (lut_cells) *lut_cells = lc;
  if (compact_items) *compact_items = lc ? ndt::record_compaction_items(lc) : 0;
  if (compact_tiles) *compact_tiles = lc ? static_cast<long long>(ndt::record_compaction_tiles(lc)) : 0;
  if (compact_prefix) *compact_prefix = lc && ndt::record_compaction_prefix(lc) ? 1 : 0;
  ndt::GridBuildPlan fplan{};
  const bool fb = n_cells > 0 && filter_takes_buckets(n_cells, n_points, fplan);
  if (filter_buckets) *filter_buckets = fb ? 1 : 0;
  if (filter_chunks) *filter_chunks = fb ? ndt::filter_buckets_chunks(n_cells) : 0;
  return NDT_OK;
}

ndt_status ndt_diag_grid_build(ndt_handle h, int* form, size_t* n_points, long long* n_cells, int* n_buckets, int* cells_per_bucket,
                               int* pts_per_block, int* n_blocks, int* wmax, int* lds_cap, long long* lut_cells, int* compact_items,
                               long long* compact_tiles, int* compact_prefix, int* compact_pending) {
  if (!h || !h->grid) return fail(NDT_ERR_NO_INPUT, "no grid");
  const DeviceGrid* g = h->grid.get();
  const int f = g->empty ? 0 : g->build_form;
  const bool bucketed = f == 2 || f == 3, table = f == 1 || bucketed;
  ndt::K1FinishLds F{};
  if (f == 2) F = ndt::grid_build_finish_lds(g->plan.cells_per_bucket);
  if (f == 3) {  // the one-launch form shares the finish's LDS with its point lists: a cap of its own
    ndt::SmallBuildDesc D{};
    size_t lds = 0;
    if (ndt::small_build_desc(static_cast<int>(g->target ? g->target->n : 0), g->plan, false, D, &lds)) {
      F.wmax = D.wmax;
      F.lds_cap = D.lds_cap;
    }
  }
  const long long lc = table ? g->geom.lut_cells : 0;
  if (form) *form = f;
  if (n_points) *n_points = g->target ? g->target->n : 0;
  if (n_cells) *n_cells = f ? g->geom.n_cells : 0;
  if (n_buckets) *n_buckets = bucketed ? g->plan.n_buckets : 0;
  if (cells_per_bucket) *cells_per_bucket = bucketed ? g->plan.cells_per_bucket : 0;
  if (pts_per_block) *pts_per_block = f == 2 ? g->plan.pts_per_block : 0;
  if (n_blocks) *n_blocks = f == 2 ? g->plan.n_blocks : 0;
  if (wmax) *wmax = F.wmax;
  if (lds_cap) *lds_cap = F.lds_cap;
  if (lut_cells) *lut_cells = lc;
  if (compact_items) *compact_items = lc ? ndt::record_compaction_items(lc) : 0;
  if (compact_tiles) *compact_tiles = lc ? static_cast<long long>(ndt::record_compaction_tiles(lc)) : 0;
  if (compact_prefix) *compact_prefix = lc && ndt::record_compaction_prefix(lc) ? 1 : 0;
  if (compact_pending) *compact_pending = g->compact_pending ? 1 : 0;
  return NDT_OK;
}

ndt_status ndt_grid_size(ndt_handle h, size_t* n_leaves, size_t* n_valid) {
  if (!h || !h->grid) return fail(NDT_ERR_NO_INPUT, "no grid");
  return grid_size(h, h->grid.get(), n_leaves, n_valid);
}
ndt_status ndt_grid_info(ndt_handle h, int* min_b, int* max_b, int* div_b) {
  if (!h || !h->grid) return fail(NDT_ERR_NO_INPUT, "no grid");
  grid_info(h->grid.get(), min_b, max_b, div_b);
  return NDT_OK;
}
ndt_status ndt_grid_dump(ndt_handle h, int64_t* idx, int* nr_points, double* mean, double* cov, double* icov,
                         double* evals) {
  if (!h || !h->grid) return fail(NDT_ERR_NO_INPUT, "no grid");
  return grid_dump(h, h->grid.get(), idx, nr_points, mean, cov, icov, evals);
}

}  // extern "C"
