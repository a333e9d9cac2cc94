// ndt_filter.hip -- N1, the voxel-grid centroid down-sample (pcl::VoxelGrid::applyFilter) of one cloud: the route decision, the
// queued and the synchronous form, and the entry points over host buffers, device buffers and ndt_clouds (whole, or in two
// halves on the filter stream).  Many clouds in one call: ndt_filter_batch.hip; the map's filter: ndt_map_batch.hip.
#include "ndt_internal.hpp"

namespace ndtc {

// ---- N1: voxel-grid centroid down-sample -----------------------------------
// [PCL] VoxelGrid::applyFilter on a dense float4 device cloud: d_out (capacity n) receives one centroid per occupied voxel
// in ascending voxel-index order.  Two halves: voxel_filter_enqueue queues the whole chain on a stream and returns -- the
// count and the per-block rows of the result's bounding boxes travel to page-locked memory behind the last kernel --
// voxel_filter_finish reads them once that stream has been waited for.  voxel_filter_device is the two with a
// synchronisation in between (N1); the map update (N2) leaves the wait to whoever next needs the map.

FilterRoute filter_route(const ndt_context* h, size_t n, const BBox& bb, float leaf) {
  FilterRoute r;
  const float* min_p = bb.mn;
  const float* max_p = bb.mx;
  if (n == 0 || !(min_p[0] <= max_p[0])) return r;  // no finite point: empty output
  ndt::GridGeom& geo = r.geo;
  if (ndt::lattice_geometry(leaf, min_p, max_p, geo) == ndt::kLatticeIndexOverflow) {
    r.kind = FilterRoute::kOverflow;
    return r;
  }
  // a fine leaf over a wide box (apps/align.cpp: 0.1 m over a whole scan): per-point work only (ndt_sparse.hip)
  const bool sparse = h->voxel_index == 2 || (h->voxel_index == 0 && geo.n_cells > 16ll * static_cast<long long>(n) + (1ll << 22));
  r.kind = sparse ? FilterRoute::kSparse : FilterRoute::kDense;
  return r;
}

bool filter_takes_buckets(long long n_cells, long long n, ndt::GridBuildPlan& plan) {
  static const bool vf_buckets = [] { const char* v = getenv("NDT_VF"); return !(v && std::strcmp(v, "chain") == 0); }();
  // (from 128 k points and for boxes with at most four cells per point: below / beyond, a bucket's share of the cell space --
  // thousands of cells for a hundred points -- makes vf_finalize cost what the chain's scans cost: 60 k points 81 against 76 us,
  // a 250 k-point map 29 us for that kernel alone; 300 k-point scan 81 against 111, 1 M 106 against 228.  NDT_VF_FROM=0: always.)
  static const long long vf_from = [] { const char* v = getenv("NDT_VF_FROM"); return v ? static_cast<long long>(std::max(0, atoi(v))) : 131072ll; }();
  const bool vf_dense = vf_from == 0 || (n >= vf_from && n_cells <= 4ll * n);
  return vf_buckets && vf_dense && n <= 0x7fffffffll && ndt::filter_buckets_plan(n_cells, static_cast<int>(n), plan);
}

ndt_status voxel_filter_enqueue(ndt_handle h, hipStream_t st, const float4* d_in, size_t n, int is_dense, float leaf, float4* d_out,
                                const BBox& bb, FilterPending& P) {
  P.n_max = n;
  P.fixed_n = 0;
  P.from_device = false;
  P.overflow = false;
  if (n == 0) return NDT_OK;
  const PoolStreamGuard guard(st);
  const int ni = static_cast<int>(n);
  const FilterRoute route = filter_route(h, n, bb, leaf);
  if (route.kind == FilterRoute::kEmpty) {  // no finite point: empty output
    for (int i = 0; i < kOutBoxBlocks * 12; i++) P.rows[i] = (i % 6) < 3 ? FLT_MAX : -FLT_MAX;
    return NDT_OK;
  }
  const int nb_rows = static_cast<int>(std::min<size_t>(kOutBoxBlocks, (n + 255) / 256));
  if (route.kind == FilterRoute::kOverflow) {
    HIP_TRY(hipMemcpyAsync(d_out, d_in, n * sizeof(float4), hipMemcpyDeviceToDevice, st));  // output = *input_
    HIP_TRY(ndt::launch_repack_bbox(d_out, n, sizeof(float4), nullptr, P.rows, nb_rows, st, 0, nullptr));
    P.fixed_n = n;
    P.overflow = true;
    return NDT_OK;
  }
  const ndt::GridGeom geo = route.geo;
  DevBuf<unsigned> cell_count, totals, rank;
  DevBuf<int> key;
  ChainBufs lv;
  const size_t n_leaves = std::min<size_t>(n, static_cast<size_t>(geo.n_cells));  // upper bound; the count stays on the device
  P.from_device = true;
  if (route.kind == FilterRoute::kSparse) {
    // a fine leaf over a wide box (apps/align.cpp: 0.1 m over a whole scan): per-point work only (ndt_sparse.hip)
    DevBuf<float4> big2;
    HIP_TRY(totals.reserve(8));
    HIP_TRY(lv.reserve(n_leaves, n));
    HIP_TRY(big2.reserve(n));
    if (ndt_status s = sparse_index(st, d_in, ni, is_dense, geo, 1, lv.out(), totals.p)) return s;
    HIP_TRY(ndt::launch_voxel_centroids(d_in, lv.leaf_start.p, lv.leaf_count.p, static_cast<int>(n_leaves), lv.sorted_idx.p, d_out, st, totals.p, big2.p));
    HIP_TRY(hipMemcpyAsync(P.tot, totals.p, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(ndt::launch_repack_bbox(d_out, n, sizeof(float4), nullptr, P.rows, nb_rows, st, 0, totals.p + 1));
    return NDT_OK;  // (the temporaries go back to the stream's pool: reused only behind these launches)
  }
  // Dense grids within the bucket plan's range: the order-preserving bucket front end of K1 + vf_finalize / vf_bitmap_prefix /
  // vf_place (ndt_grid_kernels.hip): the cell space is never walked, no point is gathered through an index.
  // NDT_VF=chain: the general chain below for every grid (the cross-check).
  ndt::GridBuildPlan plan{};
  if (filter_takes_buckets(geo.n_cells, static_cast<long long>(n), plan)) {
    const size_t K = static_cast<size_t>(plan.n_buckets);
    const size_t bw = ndt::filter_buckets_bitmap_words(geo.n_cells);
    DevBuf<unsigned> cntmat, order, bucket_base, bitmap, wprefix;
    DevBuf<float4> bpts, st_cent;
    DevBuf<int> st_cell;
    HIP_TRY(cntmat.reserve((static_cast<size_t>(plan.n_blocks) + 1) * K));
    HIP_TRY(order.reserve(5 * n));
    HIP_TRY(bucket_base.reserve(2 * K + 1));
    HIP_TRY(bpts.reserve(n));
    HIP_TRY(st_cell.reserve(n));
    HIP_TRY(st_cent.reserve(n));
    HIP_TRY(bitmap.reserve(bw));
    HIP_TRY(wprefix.reserve(bw));
    HIP_TRY(totals.reserve(4));
    ndt::GridBuildScratch S{};
    S.cntmat = cntmat.p;
    S.bucket_base = bucket_base.p;
    S.bpts = bpts.p;
    S.order = order.p;
    HIP_TRY(ndt::launch_filter_buckets(d_in, ni, is_dense, geo, plan, S, st_cell.p, st_cent.p, bitmap.p, wprefix.p, totals.p, d_out, st));
    HIP_TRY(hipMemcpyAsync(P.tot, totals.p, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(ndt::launch_repack_bbox(d_out, n, sizeof(float4), nullptr, P.rows, nb_rows, st, 0, totals.p + 1));
    return NDT_OK;  // (the temporaries go back to the stream's pool: reused only behind these launches)
  }
  HIP_TRY(cell_count.reserve(static_cast<size_t>(geo.n_cells)));
  HIP_TRY(key.reserve(n));
  HIP_TRY(rank.reserve(n));
  HIP_TRY(hipMemsetAsync(cell_count.p, 0, static_cast<size_t>(geo.n_cells) * sizeof(unsigned), st));
  HIP_TRY(ndt::launch_count(d_in, ni, is_dense, geo, key.p, rank.p, cell_count.p, st));
  HIP_TRY(totals.reserve(4));
  HIP_TRY(lv.reserve(n_leaves, n));
  if (ndt_status s = chain_scan_scatter(st, cell_count.p, geo.n_cells, 1, key.p, rank.p, ni, lv.out(), totals.p)) return s;
  DevBuf<float4> big_pts;  // scratch of the crowded-voxel path (k_presort_large)
  HIP_TRY(big_pts.reserve(n));
  HIP_TRY(ndt::launch_voxel_centroids(d_in, lv.leaf_start.p, lv.leaf_count.p, static_cast<int>(n_leaves), lv.sorted_idx.p, d_out, st, totals.p, big_pts.p));
  HIP_TRY(hipMemcpyAsync(P.tot, totals.p, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(ndt::launch_repack_bbox(d_out, n, sizeof(float4), nullptr, P.rows, nb_rows, st, 0, totals.p + 1));
  return NDT_OK;
}

// after the stream of voxel_filter_enqueue has been waited for: the count, and the boxes of the result
void voxel_filter_finish(const FilterPending& P, size_t* n_out, DeviceCloud* boxes) {
  *n_out = P.from_device ? P.tot[1] : P.fixed_n;
  if (!boxes) return;
  boxes->box_route = NDT_BOX_ROUTE_FILTER_ROWS;
  for (int v = 0; v < 2; v++)
    for (int k = 0; k < 3; k++) {
      boxes->bb_min[v][k] = FLT_MAX;
      boxes->bb_max[v][k] = -FLT_MAX;
    }
  if (*n_out == 0) return;
  const int nb = static_cast<int>(std::min<size_t>(kOutBoxBlocks, (P.n_max + 255) / 256));
  for (int b = 0; b < nb; b++)
    for (int v = 0; v < 2; v++)
      for (int k = 0; k < 3; k++) {
        boxes->bb_min[v][k] = std::min(boxes->bb_min[v][k], P.rows[b * 12 + v * 6 + k]);
        boxes->bb_max[v][k] = std::max(boxes->bb_max[v][k], P.rows[b * 12 + v * 6 + 3 + k]);
      }
}

ndt_status filter_slots(ndt_handle h, int which, FilterPending& P) {
  if (!h->filter_slots) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->filter_slots), 3 * (kOutBoxBlocks * 12 + 4) * sizeof(float), hipHostMallocDefault));
  }
  float* base = h->filter_slots + which * (kOutBoxBlocks * 12 + 4);
  P.rows = base;
  P.tot = reinterpret_cast<unsigned*>(base + kOutBoxBlocks * 12);
  return NDT_OK;
}

// the synchronous form (N1): *overflow = the leaf is too small for the bounding box and, as PCL does, the input was copied
// through.  Synchronises h->stream.
ndt_status voxel_filter_device(ndt_handle h, const float4* d_in, size_t n, int is_dense, float leaf, float4* d_out,
                                      size_t* n_out, bool* overflow, const BBox* known_bbox, DeviceCloud* out_boxes) {
  *n_out = 0;
  *overflow = false;
  if (n == 0) return NDT_OK;
  BBox bb;
  if (known_bbox) bb = *known_bbox;
  else { ndt_status sb = bbox_compute(h, d_in, static_cast<int>(n), is_dense, bb); if (sb) return sb; }
  FilterPending P;
  ndt_status s = filter_slots(h, 0, P);
  if (!s) s = voxel_filter_enqueue(h, h->stream, d_in, n, is_dense, leaf, d_out, bb, P);
  if (s) return s;
  HIP_TRY(hipStreamSynchronize(h->stream));
  voxel_filter_finish(P, n_out, out_boxes);
  *overflow = P.overflow;
  return NDT_OK;
}

}  // namespace ndtc

extern "C" {

static ndt_status voxel_filter_impl(ndt_handle h, const void* pts, size_t n, size_t stride, int is_dense, float leaf,
                                    bool on_device, void* out, size_t out_stride, size_t* n_out) {
  if (!h || !n_out || (n && !out) || !(leaf > 0)) return fail(NDT_ERR_INVALID, "bad arguments");
  *n_out = 0;
  std::shared_ptr<DeviceCloud> c;
  ndt_status s = upload_cloud(h, pts, n, stride, on_device, c);
  if (s) return s;
  if (n == 0) return NDT_OK;
  float4* d_out = on_device ? static_cast<float4*>(out) : nullptr;
  if (!on_device) {
    // Host buffer out: the centroid kernel writes straight into the handle's page-locked block (posted writes over the link,
    // inside the kernel's own time) instead of into HBM followed by a copy and a second synchronisation; the CPU then
    // spreads the records into the caller's buffer.  (60 k-point scan from a C++ caller, tools/probes/time_filter.cpp: 178-216 -> 158-182 us.)
    if (out_stride < 16) return fail(NDT_ERR_INVALID, "out_stride_bytes must be >= 16");
    if ((s = out_block_at_least(h, n * sizeof(float4)))) return s;
    d_out = static_cast<float4*>(h->out_pinned);
  }
  size_t n_written = 0;
  bool overflow = false;
  const BBox bb = bbox_of(*c, is_dense);
  s = voxel_filter_device(h, c->pts.p, n, is_dense, leaf, d_out, &n_written, &overflow, &bb);  // (synchronises the stream)
  if (s) return s;
  if (!on_device && n_written) spread_records(h->out_pinned, n_written, out, out_stride);
  *n_out = n_written;
  if (overflow) return fail(NDT_ERR_GRID_OVERFLOW, "leaf size is too small for the input dataset: integer indices would overflow");
  return NDT_OK;
}

ndt_status ndt_voxel_grid_filter(ndt_handle h, const void* pts, size_t n, size_t stride, int is_dense, float leaf, void* out,
                                 size_t out_stride, size_t* n_out) {
  return voxel_filter_impl(h, pts, n, stride, is_dense, leaf, false, out, out_stride, n_out);
}
ndt_status ndt_voxel_grid_filter_device(ndt_handle h, const void* d_pts, size_t n, size_t stride, int is_dense, float leaf,
                                        void* d_out, size_t* n_out) {
  return voxel_filter_impl(h, d_pts, n, stride, is_dense, leaf, true, d_out, 16, n_out);
}

ndt_status ndt_cloud_voxel_filter(ndt_handle h, const void* pts, size_t n, size_t stride, int is_dense, float leaf, int on_device,
                                  ndt_cloud* out, int* overflowed) {
  if (!h || !out || !(leaf > 0)) return fail(NDT_ERR_INVALID, "bad arguments");
  *out = nullptr;
  if (overflowed) *overflowed = 0;
  std::shared_ptr<DeviceCloud> in;
  // (a device cloud of 16-byte records is read where it lies; everything it is needed for is over when this returns)
  const bool ref_ok = on_device && n > 0 && stride == sizeof(float4) && (reinterpret_cast<uintptr_t>(pts) & 15) == 0;
  ndt_status s = upload_cloud(h, pts, n, stride, on_device != 0, in, ref_ok);
  if (s) return s;
  auto c = std::make_shared<DeviceCloud>();
  c->device = h->device;
  c->made_on = h->stream;
  HIP_TRY(c->pts.reserve(std::max<size_t>(n, 1)));
  size_t n_written = 0;
  bool overflow = false;
  if (n) {
    const BBox bb = bbox_of(*in, is_dense);
    s = voxel_filter_device(h, in->pts.p, n, is_dense, leaf, c->pts.p, &n_written, &overflow, &bb, c.get());
    if (s) return s;
  }
  c->n = n_written;
  if (overflowed) *overflowed = overflow ? 1 : 0;
  *out = new ndt_cloud_s{c};
  return NDT_OK;
}

// N1 of an ndt_cloud, in two halves: begin queues the whole chain on the handle's FILTER stream and returns (the input's boxes
// are known: nothing has to come back from the device before the chain can be queued); end waits for it.  Between the two the
// caller registers the previous scan on the handle's own stream.
ndt_status ndt_cloud_voxel_filter_begin(ndt_handle h, ndt_cloud in, int is_dense, float leaf) {
  if (!h || !in || !(leaf > 0)) return fail(NDT_ERR_INVALID, "bad arguments");
  if (h->n1_pending) return fail(NDT_ERR_INVALID, "a prefilter has been begun and not ended");
  ndt_status s = ensure_device(h);
  if (s) return s;
  if (!h->filter_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&h->filter_stream, hipStreamNonBlocking));
    DevPool::instance().adopt_stream(h->filter_stream);
  }
  DeviceCloud* ic = in->c.get();
  if (ic->made_on && ic->made_on != h->filter_stream) {  // made elsewhere: complete before the filter stream reads it
    if (ic->device != h->device) return fail(NDT_ERR_INVALID, "the cloud lives on another device");
    HIP_TRY(hipStreamSynchronize(ic->made_on));
    if (std::find(ic->used_on.begin(), ic->used_on.end(), h->filter_stream) == ic->used_on.end()) ic->used_on.push_back(h->filter_stream);
  }
  auto c = std::make_shared<DeviceCloud>();
  c->device = h->device;
  c->made_on = h->filter_stream;
  {
    const PoolStreamGuard guard(h->filter_stream);
    HIP_TRY(c->pts.reserve(std::max<size_t>(ic->n, 1)));
  }
  s = filter_slots(h, 2, h->n1_filter);
  if (!s) s = voxel_filter_enqueue(h, h->filter_stream, ic->pts.p, ic->n, is_dense, leaf, c->pts.p, bbox_of(*ic, is_dense), h->n1_filter);
  if (s) return s;
  h->n1_in = in->c;
  h->n1_out = c;
  h->n1_pending = true;
  return NDT_OK;
}
ndt_status ndt_cloud_voxel_filter_end(ndt_handle h, ndt_cloud* out, int* overflowed) {
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  *out = nullptr;
  if (!h->n1_pending) return fail(NDT_ERR_INVALID, "no prefilter has been begun");
  ndt_status s = ensure_device(h);
  if (s) return s;
  h->n1_pending = false;
  HIP_TRY(hipStreamSynchronize(h->filter_stream));
  size_t n_written = 0;
  voxel_filter_finish(h->n1_filter, &n_written, h->n1_out.get());
  h->n1_out->n = n_written;
  if (overflowed) *overflowed = h->n1_filter.overflow ? 1 : 0;
  *out = new ndt_cloud_s{h->n1_out};
  h->n1_in.reset();
  h->n1_out.reset();
  return NDT_OK;
}

}  // extern "C"
