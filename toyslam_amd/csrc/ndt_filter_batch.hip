// ndt_filter_batch.hip -- N1 of many clouds in one call (ndt_cloud_voxel_filter_batch / _clouds): pcl::VoxelGrid::filter
// of every cloud at one leaf size, each cloud's result what ndt_cloud_voxel_filter returns for it alone, bit for bit.
//
// A call is a box pass over every input (k_repack_bbox_multi, one launch whatever the number of clouds; the clouds form
// knows its boxes and only gathers its inputs into one block), a host plan (filter_route: the single filter's own
// decision), then one or a few COMPOSITE PASSES: the clouds whose dense cell space fits a counter budget share one
// count / scan / scatter / centroid chain.  k_count_multi puts cloud k's points on ITS lattice (build_cell, range-tested
// against its own cell count) and moves the cell to counters of its own (base_k + cell), so the leaves of cloud k are a
// contiguous run in its own voxel order, each summed in ascending point index -- the cloud's own order -- as the single
// chain sums it.  k_leaf_ranges finds every run, k_repack_bbox_multi boxes it, and one read-back brings counts and boxes.
// The other clouds (overflow copy-through, the sparse index, a cell space larger than one pass) take voxel_filter_enqueue
// on the same stream, each with page-locked result rows of its own, and are read behind the same waits.
#include "ndt_internal.hpp"

namespace ndtc {
namespace {

// counters per composite pass (NDT_VF_BATCH_CELLS, a development switch read once; default order_batch's kMaxCounters)
long long batch_cell_budget() {
  static const long long v = [] {
    const char* e = getenv("NDT_VF_BATCH_CELLS");
    const long long x = e ? atoll(e) : 0;
    return x > 0 ? std::min(x, 1ll << 30) : 32000000ll;
  }();
  return v;
}

struct BatchIn {
  size_t first = 0, n = 0;  // its records in the staged block
  int dense = 0;
  BBox bb{};                // the box of its NaN rule
};

void decode_boxes(const unsigned* w, DeviceCloud* c) {
  for (int v = 0; v < 2; v++)
    for (int k = 0; k < 3; k++) {
      c->bb_min[v][k] = ndt::box_word_decode(w[6 * v + k], true);
      c->bb_max[v][k] = ndt::box_word_decode(w[6 * v + 3 + k], false);
    }
  c->box_route = NDT_BOX_ROUTE_MULTI_WORDS;
}

// One composite pass over clouds [s0, s1] of `in`: the members (is_member) are filtered, the others in that span only get
// keys of -1.  Every member's result is a slice of the pass's output block.  Waits for the stream.
ndt_status composite_pass(ndt_handle h, const float4* block, const std::vector<BatchIn>& in, const std::vector<FilterRoute>& route,
                          const std::vector<char>& is_member, size_t s0, size_t s1, std::vector<std::shared_ptr<DeviceCloud>>& out) {
  hipStream_t st = h->stream;
  const size_t nd = s1 - s0 + 1;
  const size_t span = in[s1].first + in[s1].n - in[s0].first;
  std::vector<ndt::FilterBatchCloud> cl(nd);
  long long total_cells = 0;
  size_t members_pts = 0, max_n = 1;
  for (size_t j = 0; j < nd; j++) {
    const BatchIn& b = in[s0 + j];
    ndt::FilterBatchCloud& d = cl[j];
    d = ndt::FilterBatchCloud{};
    d.first = static_cast<int>(b.first - in[s0].first);
    d.n = static_cast<int>(b.n);
    d.dense = b.dense;
    d.base = static_cast<int>(total_cells);
    if (is_member[s0 + j]) {
      d.g = route[s0 + j].geo;
      total_cells += d.g.n_cells;
      members_pts += b.n;
      max_n = std::max(max_n, b.n);
    }
  }
  auto blk = new_cloud(h);  // the pass's output block
  HIP_TRY(blk->pts.reserve(std::max<size_t>(members_pts, 1)));
  blk->n = members_pts;
  // device words: [cell counters][12 box words per cloud][2 leaf bounds per cloud][4 totals]
  const size_t w_boxes = static_cast<size_t>(total_cells), w_ranges = w_boxes + 12 * nd, w_totals = w_ranges + 2 * nd, n_words = w_totals + 4;
  const size_t desc_bytes = nd * sizeof(ndt::FilterBatchCloud), seg_bytes = nd * sizeof(ndt::SegDesc);
  const size_t back_bytes = (n_words - w_boxes) * sizeof(unsigned);
  DevBuf<unsigned> work, rank;
  DevBuf<int> key;
  ChainBufs lv;
  DevBuf<float4> big_pts;
  DevBuf<unsigned char> d_desc;
  HIP_TRY(d_desc.reserve(desc_bytes + seg_bytes));
  HIP_TRY(work.reserve(n_words));
  ndt_status s = pinned_at_least(h->fb_pinned, h->fb_pinned_bytes, std::max(desc_bytes + seg_bytes, back_bytes), st);
  if (s) return s;
  std::memcpy(h->fb_pinned, cl.data(), desc_bytes);
  // the result's boxes: segment j = the leaves [lo, hi) of the block that k_leaf_ranges finds (a device-side range)
  ndt::SegDesc* segs = reinterpret_cast<ndt::SegDesc*>(static_cast<unsigned char*>(h->fb_pinned) + desc_bytes);
  for (size_t j = 0; j < nd; j++) {
    segs[j] = ndt::SegDesc{};
    segs[j].src = reinterpret_cast<const unsigned char*>(blk->pts.p);
    segs[j].range = work.p + w_ranges + 2 * j;
    segs[j].n = in[s0 + j].n;
    segs[j].stride = sizeof(float4);
  }
  const ndt::FilterBatchCloud* d_cl = reinterpret_cast<const ndt::FilterBatchCloud*>(d_desc.p);
  const ndt::SegDesc* d_seg = reinterpret_cast<const ndt::SegDesc*>(d_desc.p + desc_bytes);
  const size_t n_leaves = std::min<size_t>(members_pts, static_cast<size_t>(total_cells));  // upper bound; the count stays on the device
  HIP_TRY(key.reserve(span));
  HIP_TRY(rank.reserve(span));
  HIP_TRY(lv.reserve(n_leaves, members_pts));
  HIP_TRY(big_pts.reserve(members_pts));  // scratch of the crowded-voxel path (k_presort_large)
  const float4* pts = block + in[s0].first;
  unsigned* totals = work.p + w_totals;
  HIP_TRY(hipMemcpyAsync(d_desc.p, h->fb_pinned, desc_bytes + seg_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(work.p, 0, w_ranges * sizeof(unsigned), st));  // the counters and the box words
  HIP_TRY(ndt::launch_count_multi(pts, d_cl, static_cast<int>(nd), static_cast<int>(max_n), key.p, rank.p, work.p, st));
  if ((s = chain_scan_scatter(st, work.p, total_cells, 1, key.p, rank.p, static_cast<int>(span), lv.out(), totals))) return s;
  HIP_TRY(ndt::launch_voxel_centroids(pts, lv.leaf_start.p, lv.leaf_count.p, static_cast<int>(n_leaves), lv.sorted_idx.p, blk->pts.p, st, totals, big_pts.p));
  HIP_TRY(ndt::launch_leaf_ranges(lv.leaf_cell.p, totals, d_cl, static_cast<int>(nd), work.p + w_ranges, st));
  HIP_TRY(ndt::launch_repack_bbox_multi(d_seg, static_cast<int>(nd), max_n, work.p + w_boxes, st));
  HIP_TRY(hipMemcpyAsync(h->fb_pinned, work.p + w_boxes, back_bytes, hipMemcpyDeviceToHost, st));
  h->fb_launches += 12;
  h->fb_passes++;
  HIP_TRY(hipStreamSynchronize(st));
  const unsigned* r = static_cast<const unsigned*>(h->fb_pinned);
  const unsigned* ranges = r + 12 * nd;
  for (size_t j = 0; j < nd; j++) {
    if (!is_member[s0 + j]) continue;
    const unsigned lo = ranges[2 * j], hi = ranges[2 * j + 1];
    auto c = new_cloud(h);
    c->pts.borrow(blk->pts.p + lo, hi - lo);
    c->n = hi - lo;
    if (c->n) decode_boxes(r + 12 * j, c.get());
    c->owner = blk;
    out[s0 + j] = c;
  }
  return NDT_OK;
}

// the plan and the passes over a staged block of dense records (in[k]: cloud k's records, NaN rule and box)
ndt_status filter_batch_run(ndt_handle h, const float4* block, const std::vector<BatchIn>& in, float leaf,
                            std::vector<std::shared_ptr<DeviceCloud>>& out, std::vector<int>& ovf) {
  const size_t N = in.size();
  const long long budget = batch_cell_budget();
  std::vector<FilterRoute> route(N);
  std::vector<char> member(N, 0);
  std::vector<size_t> single;
  for (size_t k = 0; k < N; k++) {
    route[k] = filter_route(h, in[k].n, in[k].bb, leaf);
    if (route[k].kind == FilterRoute::kDense && route[k].geo.n_cells <= budget) member[k] = 1;
    else if (route[k].kind == FilterRoute::kEmpty) out[k] = new_cloud(h);  // (no point, no finite point: an empty cloud)
    else single.push_back(k);
  }
  // the single-cloud route first, queued and not waited for: page-locked result rows of its own per cloud
  h->fb_single = single.size();
  std::vector<FilterPending> pend(single.size());
  if (!single.empty()) {
    const size_t per = kOutBoxBlocks * 12 + 4;
    ndt_status s = pinned_at_least(h->fb_rows, h->fb_rows_bytes, single.size() * per * sizeof(float), h->stream);
    if (s) return s;
    for (size_t i = 0; i < single.size(); i++) {
      const size_t k = single[i];
      pend[i].rows = static_cast<float*>(h->fb_rows) + i * per;
      pend[i].tot = reinterpret_cast<unsigned*>(pend[i].rows + kOutBoxBlocks * 12);
      auto c = new_cloud(h);
      HIP_TRY(c->pts.reserve(std::max<size_t>(in[k].n, 1)));
      s = voxel_filter_enqueue(h, h->stream, block + in[k].first, in[k].n, in[k].dense, leaf, c->pts.p, in[k].bb, pend[i]);
      if (s) return s;
      out[k] = c;
    }
  }
  // composite passes: consecutive clouds while the members' counters fit the budget and the span's points an int
  bool waited = false;
  for (size_t k = 0; k < N;) {
    if (!member[k]) {
      k++;
      continue;
    }
    const size_t s0 = k;
    size_t last = k;
    long long cells = route[k].geo.n_cells;
    for (size_t j = k + 1; j < N; j++) {
      if (!member[j]) continue;
      if (cells + route[j].geo.n_cells > budget || in[j].first + in[j].n - in[s0].first > static_cast<size_t>(std::numeric_limits<int>::max()))
        break;
      cells += route[j].geo.n_cells;
      last = j;
    }
    ndt_status s = composite_pass(h, block, in, route, member, s0, last, out);
    if (s) return s;
    waited = true;
    k = last + 1;
  }
  if (!single.empty()) {
    if (!waited) HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < single.size(); i++) {
      DeviceCloud* c = out[single[i]].get();
      size_t n_written = 0;
      voxel_filter_finish(pend[i], &n_written, c);
      c->n = n_written;
      ovf[single[i]] = pend[i].overflow ? 1 : 0;
    }
  }
  return NDT_OK;
}

// the buffer form: cloud k = records [offsets[k], offsets[k+1]) of pts, staged into one block of dense records (or used where
// they lie: 16-byte device records), boxed by one launch, the boxes read back behind one wait
ndt_status filter_batch_buffer(ndt_handle h, const void* pts, const size_t* offsets, size_t N, size_t stride, const int* is_dense,
                               float leaf, bool on_device, std::vector<std::shared_ptr<DeviceCloud>>& out, std::vector<int>& ovf) {
  hipStream_t st = h->stream;
  const size_t total = offsets[N] - offsets[0];
  std::vector<BatchIn> in(N);
  size_t max_n = 1;
  for (size_t k = 0; k < N; k++) {
    in[k].first = offsets[k] - offsets[0];
    in[k].n = offsets[k + 1] - offsets[k];
    in[k].dense = (is_dense && is_dense[k]) ? 1 : 0;
    max_n = std::max(max_n, in[k].n);
  }
  const unsigned char* src = static_cast<const unsigned char*>(pts) + offsets[0] * stride;
  DevBuf<float4> staged;
  const float4* block = nullptr;
  if (total) {
    if (!on_device) {
      HIP_TRY(h->staging.reserve(total * stride));
      HIP_TRY(hipMemcpyAsync(h->staging.p, src, total * stride, hipMemcpyHostToDevice, st));
      src = h->staging.p;
      h->fb_launches++;
    }
    const bool in_place = on_device && stride == sizeof(float4) && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    if (in_place) {
      block = reinterpret_cast<const float4*>(src);
    } else {
      HIP_TRY(staged.reserve(total));
      block = staged.p;
    }
    const size_t seg_bytes = N * sizeof(ndt::SegDesc), box_bytes = 12 * N * sizeof(unsigned);
    ndt_status s = pinned_at_least(h->fb_pinned, h->fb_pinned_bytes, seg_bytes + box_bytes, st);
    if (s) return s;
    ndt::SegDesc* segs = static_cast<ndt::SegDesc*>(h->fb_pinned);
    for (size_t k = 0; k < N; k++) {
      segs[k] = ndt::SegDesc{};
      segs[k].src = src + in[k].first * stride;
      segs[k].dst = in_place ? nullptr : staged.p + in[k].first;
      segs[k].n = in[k].n;
      segs[k].stride = static_cast<int>(stride);
    }
    unsigned char* w_host = static_cast<unsigned char*>(h->fb_pinned) + seg_bytes;
    std::memset(w_host, 0, box_bytes);  // (the box words start at zero: copied up with the descriptors)
    DevBuf<unsigned char> d_desc;
    HIP_TRY(d_desc.reserve(seg_bytes + box_bytes));
    unsigned* d_boxes = reinterpret_cast<unsigned*>(d_desc.p + seg_bytes);
    HIP_TRY(hipMemcpyAsync(d_desc.p, h->fb_pinned, seg_bytes + box_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ndt::launch_repack_bbox_multi(reinterpret_cast<const ndt::SegDesc*>(d_desc.p), static_cast<int>(N), max_n, d_boxes, st));
    HIP_TRY(hipMemcpyAsync(w_host, d_boxes, box_bytes, hipMemcpyDeviceToHost, st));
    h->fb_launches += 3;
    HIP_TRY(hipStreamSynchronize(st));
    const unsigned* w = reinterpret_cast<const unsigned*>(w_host);
    for (size_t k = 0; k < N; k++) {
      DeviceCloud boxes;
      decode_boxes(w + 12 * k, &boxes);
      in[k].bb = bbox_of(boxes, in[k].dense);
    }
  }
  return filter_batch_run(h, block, in, leaf, out, ovf);
}

// the clouds form: the boxes are known; the inputs are gathered into one block by the same kernel (no box words)
ndt_status filter_batch_clouds(ndt_handle h, const ndt_cloud* cl, size_t N, const int* is_dense, float leaf,
                               std::vector<std::shared_ptr<DeviceCloud>>& out, std::vector<int>& ovf) {
  hipStream_t st = h->stream;
  std::vector<BatchIn> in(N);
  size_t total = 0, max_n = 1;
  for (size_t k = 0; k < N; k++) {
    DeviceCloud* c = cl[k]->c.get();
    ndt_status s = cloud_use_on(h, c);
    if (s) return s;
    in[k].first = total;
    in[k].n = c->n;
    in[k].dense = (is_dense && is_dense[k]) ? 1 : 0;
    in[k].bb = bbox_of(*c, in[k].dense);
    total += c->n;
    max_n = std::max(max_n, c->n);
  }
  DevBuf<float4> staged;
  if (total) {
    HIP_TRY(staged.reserve(total));
    const size_t seg_bytes = N * sizeof(ndt::SegDesc);
    ndt_status s = pinned_at_least(h->fb_pinned, h->fb_pinned_bytes, seg_bytes, st);
    if (s) return s;
    ndt::SegDesc* segs = static_cast<ndt::SegDesc*>(h->fb_pinned);
    for (size_t k = 0; k < N; k++) {
      segs[k] = ndt::SegDesc{};
      segs[k].src = reinterpret_cast<const unsigned char*>(cl[k]->c->pts.p);
      segs[k].dst = staged.p + in[k].first;
      segs[k].n = in[k].n;
      segs[k].stride = sizeof(float4);
    }
    DevBuf<unsigned char> d_desc;
    HIP_TRY(d_desc.reserve(seg_bytes));
    HIP_TRY(hipMemcpyAsync(d_desc.p, h->fb_pinned, seg_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ndt::launch_repack_bbox_multi(reinterpret_cast<const ndt::SegDesc*>(d_desc.p), static_cast<int>(N), max_n, nullptr, st));
    h->fb_launches += 2;
    // the first pass rewrites the page-locked descriptors before it queues anything: this copy must have read them
    HIP_TRY(hipStreamSynchronize(st));
  }
  return filter_batch_run(h, staged.p, in, leaf, out, ovf);
}

ndt_status batch_checks(ndt_handle h, ndt_cloud* out, size_t n_clouds, int* overflowed, float leaf) {
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  for (size_t k = 0; k < n_clouds; k++) out[k] = nullptr;
  if (overflowed)
    for (size_t k = 0; k < n_clouds; k++) overflowed[k] = 0;
  if (!(leaf > 0)) return fail(NDT_ERR_INVALID, "leaf size must be > 0");
  if (n_clouds > 65535) return fail(NDT_ERR_INVALID, "at most 65535 clouds per call");
  return NDT_OK;
}

// all results handed out, or none
ndt_status batch_finish(ndt_handle h, ndt_status s, const std::vector<std::shared_ptr<DeviceCloud>>& res, const std::vector<int>& ovf,
                        ndt_cloud* out, int* overflowed) {
  if (s) {
    (void)hipStreamSynchronize(h->stream);  // (nothing queued may still write into what goes back to the pool)
    return s;
  }
  for (size_t k = 0; k < res.size(); k++) {
    out[k] = new ndt_cloud_s{res[k]};
    if (overflowed) overflowed[k] = ovf[k];
  }
  return NDT_OK;
}

}  // namespace
}  // namespace ndtc

extern "C" {

ndt_status ndt_cloud_voxel_filter_batch(ndt_handle h, const void* pts, const size_t* offsets, size_t n_clouds, size_t stride_bytes,
                                        const int* is_dense, float leaf_size, int on_device, ndt_cloud* out, int* overflowed) {
  ndt_status s = batch_checks(h, out, n_clouds, overflowed, leaf_size);
  if (s) return s;
  if (n_clouds && !offsets) return fail(NDT_ERR_INVALID, "null offsets");
  if (n_clouds && (stride_bytes < 12 || stride_bytes % 4)) return fail(NDT_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  for (size_t k = 0; k < n_clouds; k++) {
    if (offsets[k + 1] < offsets[k]) return fail(NDT_ERR_INVALID, "offsets must not decrease");
    if (offsets[k + 1] - offsets[k] > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points in a cloud");
  }
  if (n_clouds && offsets[n_clouds] > offsets[0] && !pts) return fail(NDT_ERR_INVALID, "null point buffer");
  h->fb_passes = h->fb_single = h->fb_launches = 0;
  if (n_clouds == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  std::vector<std::shared_ptr<DeviceCloud>> res(n_clouds);
  std::vector<int> ovf(n_clouds, 0);
  s = filter_batch_buffer(h, pts, offsets, n_clouds, stride_bytes, is_dense, leaf_size, on_device != 0, res, ovf);
  return batch_finish(h, s, res, ovf, out, overflowed);
}

ndt_status ndt_cloud_voxel_filter_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const int* is_dense, float leaf_size,
                                         ndt_cloud* out, int* overflowed) {
  ndt_status s = batch_checks(h, out, n_clouds, overflowed, leaf_size);
  if (s) return s;
  if (n_clouds && !in) return fail(NDT_ERR_INVALID, "null clouds");
  for (size_t k = 0; k < n_clouds; k++)
    if (!in[k] || !in[k]->c) return fail(NDT_ERR_INVALID, "null cloud");
  h->fb_passes = h->fb_single = h->fb_launches = 0;
  if (n_clouds == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  std::vector<std::shared_ptr<DeviceCloud>> res(n_clouds);
  std::vector<int> ovf(n_clouds, 0);
  s = filter_batch_clouds(h, in, n_clouds, is_dense, leaf_size, res, ovf);
  return batch_finish(h, s, res, ovf, out, overflowed);
}

ndt_status ndt_diag_filter_batch(ndt_handle h, size_t* passes, size_t* single_route, size_t* launches) {
  if (!h || !passes || !single_route || !launches) return fail(NDT_ERR_INVALID, "bad arguments");
  *passes = h->fb_passes;
  *single_route = h->fb_single;
  *launches = h->fb_launches;
  return NDT_OK;
}

}  // extern "C"
