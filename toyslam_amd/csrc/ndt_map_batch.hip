// ndt_map_batch.hip -- N2, the global map: map_update_scans (a list of posed resident scans into the map in one pass), the
// map's stream and its settling, the single-scan entry points (ndt_map_update*: the list of one), the map's read-out, and
// N2 of many posed scans in one call (ndt_map_update_clouds / _batch): transformPointCloud of every scan by its pose, one +=
// of all of them behind the map, ONE pcl::VoxelGrid::filter of the concatenation.
//
// A many-scan call is one transform launch for all scans (k_transform_multi, straight into the room behind the map) and one
// filter (map_update_scans: the single ndt_map_update* calls are its list of one).  The clouds form reads resident
// ndt_clouds where they lie and knows their boxes.  The buffer form sends the whole buffer up with one copy and makes
// dense records and both boxes of every scan with one k_repack_bbox_multi launch -- the batched prefilter's front end --
// so no host pass over the points is needed; the caller's buffer is free when the call returns.
#include "ndt_internal.hpp"

// ---- N2: global map accumulation --------------------------------------------
// update_global_map of the mapping nodes (ndt_omp_mapping_node.cpp:195-211,
// ndt_rosbag_mapping_node.cpp:146-161): transformPointCloud(scan, pose); global_map += it;
// global_map = VoxelGrid(leaf).filter(global_map).  The map stays in HBM.
namespace ndtc {
// the map's stream (created on first use) and the completion of a queued update
static ndt_status map_stream_of(ndt_handle h) {
  if (!h->map_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&h->map_stream, hipStreamNonBlocking));
    DevPool::instance().adopt_stream(h->map_stream);
    HIP_TRY(hipEventCreateWithFlags(&h->map_ready, hipEventDisableTiming));
  }
  return NDT_OK;
}
// waits for a queued map update: the map's size and boxes are current afterwards
ndt_status map_complete(ndt_handle h) {
  if (!h->map_pending) return NDT_OK;
  h->map_pending = false;
  HIP_TRY(hipStreamSynchronize(h->map_stream));
  h->map_scans.clear();
  size_t n_new = 0;
  voxel_filter_finish(h->map_filter, &n_new, &h->map_boxes);
  h->map_boxes_known = true;
  h->map_n = n_new;
  return NDT_OK;
}

// the box of `sb` under the column-major pose P, padded for the f32 rounding of the transform, joined into `guess`;
// false: the padded box is not finite
static bool join_moved_box(const BBox& sb, const float* P, BBox& guess) {
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, mag = 0;
  for (int corner = 0; corner < 8; corner++) {
    const double q[3] = {(corner & 1) ? sb.mx[0] : sb.mn[0], (corner & 2) ? sb.mx[1] : sb.mn[1], (corner & 4) ? sb.mx[2] : sb.mn[2]};
    for (int r = 0; r < 3; r++) {
      double a = P[12 + r], m = std::fabs(a);
      for (int k = 0; k < 3; k++) {
        a += static_cast<double>(P[4 * k + r]) * q[k];
        m += std::fabs(static_cast<double>(P[4 * k + r]) * q[k]);
      }
      lo[r] = std::min(lo[r], a);
      hi[r] = std::max(hi[r], a);
      mag = std::max(mag, m);
    }
  }
  const double pad = 1e-5 * mag + 1e-6;  // (a transformed coordinate is three f32 multiply-adds: a few ulps of the terms)
  bool finite = true;
  for (int r = 0; r < 3; r++) {
    guess.mn[r] = std::min(guess.mn[r], static_cast<float>(lo[r] - pad));
    guess.mx[r] = std::max(guess.mx[r], static_cast<float>(hi[r] + pad));
    finite = finite && std::isfinite(guess.mn[r]) && std::isfinite(guess.mx[r]);
  }
  return finite;
}

ndt_status map_settle(ndt_handle h) {
  ndt_status s = map_stream_of(h);
  if (!s) s = map_complete(h);
  return s;
}

// N2 of a list of resident scans: every scan moved by its pose into the room behind the map, in the list's order, then ONE
// filter of [map | scan 0 | scan 1 | ...].  The single entry points are the list of one.
ndt_status map_update_scans(ndt_handle h, const std::vector<MapScan>& scans, float leaf, int* overflowed, MapBatchDiag* diag) {
  static const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  size_t n = 0, n_moved = 0;  // the scans' points; the scans that have any
  for (const MapScan& sc : scans) {
    n += sc.c->n;
    if (sc.c->n) n_moved++;
  }
  ndt_status s = map_stream_of(h);
  if (!s) s = map_complete(h);  // the map as the previous update left it: its size and its boxes
  if (s) return s;
  const size_t total = h->map_n + n;
  if (total > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "map too large");
  if (total == 0) return NDT_OK;
  hipStream_t ms = h->map_stream;
  // the scans were made on the handle's stream (an upload, a filter): the map's stream starts behind it; a resident cloud is
  // read by the map's stream from now on (its memory is not recycled before that stream has been waited for)
  HIP_TRY(hipEventRecord(h->map_ready, h->stream));
  HIP_TRY(hipStreamWaitEvent(ms, h->map_ready, 0));
  for (const MapScan& sc : scans) {
    DeviceCloud* c = sc.c.get();
    if (c->made_on && c->made_on != ms && std::find(c->used_on.begin(), c->used_on.end(), ms) == c->used_on.end()) c->used_on.push_back(ms);
  }
  const PoolStreamGuard guard(ms);  // the map's buffers come from (and go back to) the map stream's pool
  // concatenation [map | transformed scans] (operator+= keeps the map's points first): the scans are transformed straight
  // into the room behind the map -- the map is not copied
  if (h->map_pts.cap < total) {
    DevBuf<float4> bigger;
    HIP_TRY(bigger.reserve(total + total / 2 + n));
    if (h->map_n) HIP_TRY(hipMemcpyAsync(bigger.p, h->map_pts.p, h->map_n * sizeof(float4), hipMemcpyDeviceToDevice, ms));
    h->map_pts.swap(bigger);  // (the old block goes back to the pool behind the copy, stream order)
  }
  if (n_moved == 1) {
    for (const MapScan& sc : scans) {
      if (!sc.c->n) continue;
      float T12[12];
      colmajor_to_T12(sc.pose ? sc.pose : I, T12);
      HIP_TRY(ndt::launch_transform(sc.c->pts.p, static_cast<int>(sc.c->n), T12, h->map_pts.p + h->map_n, ms, sc.dense));
    }
  } else if (n_moved > 1) {
    // one launch for all of them: a descriptor per scan and the table of its blocks, sent up with one copy.  The copy is
    // queued on the map's stream and reads the page-locked block after this returns: whoever writes h->mb_pinned does so
    // behind map_complete (above; ndt_map_update_batch settles the map before it stages its buffer through the same block)
    const size_t desc_bytes = n_moved * sizeof(ndt::TransformScan), bytes = desc_bytes + (n_moved + 1) * sizeof(int);
    s = pinned_at_least(h->mb_pinned, h->mb_pinned_bytes, bytes, ms);
    if (s) return s;
    ndt::TransformScan* d = static_cast<ndt::TransformScan*>(h->mb_pinned);
    int* starts = reinterpret_cast<int*>(static_cast<unsigned char*>(h->mb_pinned) + desc_bytes);
    size_t first = 0, j = 0;
    long long blocks = 0;
    for (const MapScan& sc : scans) {
      const size_t m = sc.c->n;
      if (!m) continue;
      d[j] = ndt::TransformScan{};
      d[j].src = sc.c->pts.p;
      d[j].n = static_cast<int>(m);
      d[j].first = static_cast<int>(first);
      d[j].dense = sc.dense ? 1 : 0;
      colmajor_to_T12(sc.pose ? sc.pose : I, d[j].T);
      starts[j] = static_cast<int>(blocks);
      blocks += ndt::transform_multi_blocks(m);
      first += m;
      j++;
    }
    starts[n_moved] = static_cast<int>(blocks);  // (at most 65 535 scans of at most 2 048 blocks)
    DevBuf<unsigned char> d_desc;
    HIP_TRY(d_desc.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(d_desc.p, h->mb_pinned, bytes, hipMemcpyHostToDevice, ms));
    HIP_TRY(ndt::launch_transform_multi(reinterpret_cast<const ndt::TransformScan*>(d_desc.p), reinterpret_cast<const int*>(d_desc.p + desc_bytes),
                                        static_cast<int>(n_moved), static_cast<int>(blocks), h->map_pts.p + h->map_n, ms));
  }
  if (diag && n_moved) diag->transform_launches++;
  HIP_TRY(h->map_alt.reserve(total + total / 2 + n));
  // the accumulated map is dense only if every scan was; PCL carries is_dense through operator+=
  int dense = h->map_n == 0 ? 1 : h->map_dense;
  for (const MapScan& sc : scans) dense = dense && sc.dense;
  // A box for the filter without a pass over the points: the map's own box (the last pass left it) joined with the box of
  // every scan's box under its pose, padded for the f32 rounding of the transform.  ANY box that holds the points gives the
  // same voxels in the same order -- a voxel is floor(x / leaf) whatever min_b is, and the linear index orders the voxels by
  // (z, y, x) for every box -- so the result is PCL's bit for bit; only the index-overflow test wants the exact box, and it
  // is computed (one pass, one wait) when the padded one comes near overflowing.
  BBox guess{};
  bool have_guess = (h->map_n == 0 || h->map_boxes_known);
  const int v = dense ? 0 : 1;
  if (have_guess) {
    for (int k = 0; k < 3; k++) {
      guess.mn[k] = h->map_n ? h->map_boxes.bb_min[v][k] : FLT_MAX;
      guess.mx[k] = h->map_n ? h->map_boxes.bb_max[v][k] : -FLT_MAX;
    }
    for (const MapScan& sc : scans) {
      if (!sc.c->n) continue;
      const BBox sb = bbox_of(*sc.c, sc.dense);
      if (sb.mn[0] <= sb.mx[0]) have_guess = join_moved_box(sb, sc.pose ? sc.pose : I, guess) && have_guess;
    }
    if (have_guess && guess.mn[0] <= guess.mx[0]) {  // would the padded box overflow the index space?  then the exact one decides
      long long d[3];
      for (int k = 0; k < 3; k++) d[k] = static_cast<long long>((guess.mx[k] - guess.mn[k]) * (1.0f / leaf)) + 1;
      if (d[0] * d[1] * d[2] > static_cast<long long>(std::numeric_limits<int32_t>::max()) / 2) have_guess = false;
    } else {
      have_guess = false;
    }
  }
  if (!have_guess) {  // the exact box: one pass over [map | scans] and a wait for it
    BBox exact;
    HIP_TRY(hipStreamSynchronize(ms));
    const hipStream_t keep_stream = h->stream;
    h->stream = ms;  // (bbox_compute launches on and waits for the handle's stream)
    s = bbox_compute(h, h->map_pts.p, static_cast<int>(total), dense, exact);
    h->stream = keep_stream;
    if (s) return s;
    guess = exact;
    if (diag) diag->box_passes++;
  }
  s = filter_slots(h, 1, h->map_filter);
  if (!s) s = voxel_filter_enqueue(h, ms, h->map_pts.p, total, dense, leaf, h->map_alt.p, guess, h->map_filter);
  if (s) return s;
  if (diag) diag->filters++;
  h->map_dense = dense;
  h->map_pts.swap(h->map_alt);
  for (const MapScan& sc : scans) h->map_scans.push_back(sc.c);
  h->map_pending = true;  // (its size and boxes: map_complete, when somebody needs them)
  if (overflowed) *overflowed = h->map_filter.overflow ? 1 : 0;
  return NDT_OK;
}

namespace {

ndt_status map_batch_checks(ndt_handle h, size_t n_scans, float leaf, int* overflowed) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (overflowed) *overflowed = 0;
  if (!(leaf > 0)) return fail(NDT_ERR_INVALID, "leaf size must be > 0");
  if (n_scans > 65535) return fail(NDT_ERR_INVALID, "at most 65535 scans per call");
  return NDT_OK;
}

// the size test: before a device is asked for with what is known (a queued update leaves the map's size open), then exactly,
// behind map_settle -- and before anything of this call is queued or copied
ndt_status map_batch_total(ndt_handle h, size_t scan_points) {
  const size_t lim = static_cast<size_t>(std::numeric_limits<int>::max());
  if (scan_points > lim || (!h->map_pending && h->map_n + scan_points > lim)) return fail(NDT_ERR_INVALID, "map too large");
  return NDT_OK;
}

// the device, the map as the previous update left it (its size, its boxes; h->mb_pinned no longer read by a queued copy),
// and the size test on the settled map
ndt_status map_batch_begin(ndt_handle h, size_t scan_points) {
  h->mb_transform_launches = h->mb_filters = h->mb_box_passes = 0;
  ndt_status s = ensure_device(h);
  if (!s) s = map_settle(h);
  if (!s) s = map_batch_total(h, scan_points);
  return s;
}

ndt_status map_batch_run(ndt_handle h, std::vector<MapScan>& scans, const int* is_dense, const float* poses, float leaf, int* overflowed) {
  for (size_t k = 0; k < scans.size(); k++) {
    scans[k].dense = (is_dense && is_dense[k]) ? 1 : 0;
    scans[k].pose = poses ? poses + 16 * k : nullptr;
  }
  MapBatchDiag diag;
  const ndt_status s = map_update_scans(h, scans, leaf, overflowed, &diag);
  // an error behind the transform: the map's stream may still read the scans (the buffer form's block goes with the list)
  if (s && h->map_stream) (void)hipStreamSynchronize(h->map_stream);
  h->mb_transform_launches = diag.transform_launches;
  h->mb_filters = diag.filters;
  h->mb_box_passes = diag.box_passes;
  return s;
}

// the buffer form: scan k = records [offsets[k], offsets[k+1]) of pts -> slices of one block of dense records with their boxes
ndt_status map_batch_stage(ndt_handle h, const void* pts, const size_t* offsets, size_t N, size_t stride, bool on_device,
                           std::vector<MapScan>& scans) {
  hipStream_t st = h->stream;
  const size_t total = offsets[N] - offsets[0];
  auto block = std::make_shared<DeviceCloud>();
  for (size_t k = 0; k < N; k++) scans[k].c = std::make_shared<DeviceCloud>();
  if (!total) return NDT_OK;
  const unsigned char* src = static_cast<const unsigned char*>(pts) + offsets[0] * stride;
  if (!on_device) {
    HIP_TRY(h->staging.reserve(total * stride));
    HIP_TRY(hipMemcpyAsync(h->staging.p, src, total * stride, hipMemcpyHostToDevice, st));
    src = h->staging.p;
  }
  HIP_TRY(block->pts.reserve(total));
  block->n = total;
  const size_t seg_bytes = N * sizeof(ndt::SegDesc), box_bytes = 12 * N * sizeof(unsigned);
  ndt_status s = pinned_at_least(h->mb_pinned, h->mb_pinned_bytes, seg_bytes + box_bytes, h->map_stream);  // (settled: nothing reads it)
  if (s) return s;
  ndt::SegDesc* segs = static_cast<ndt::SegDesc*>(h->mb_pinned);
  size_t max_n = 1;
  for (size_t k = 0; k < N; k++) {
    const size_t first = offsets[k] - offsets[0], n = offsets[k + 1] - offsets[k];
    segs[k] = ndt::SegDesc{};
    segs[k].src = src + first * stride;
    segs[k].dst = block->pts.p + first;
    segs[k].n = n;
    segs[k].stride = static_cast<int>(stride);
    max_n = std::max(max_n, n);
  }
  unsigned char* w_host = static_cast<unsigned char*>(h->mb_pinned) + seg_bytes;
  std::memset(w_host, 0, box_bytes);  // (the box words start at zero: copied up with the descriptors)
  DevBuf<unsigned char> d_desc;
  HIP_TRY(d_desc.reserve(seg_bytes + box_bytes));
  unsigned* d_boxes = reinterpret_cast<unsigned*>(d_desc.p + seg_bytes);
  HIP_TRY(hipMemcpyAsync(d_desc.p, h->mb_pinned, seg_bytes + box_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ndt::launch_repack_bbox_multi(reinterpret_cast<const ndt::SegDesc*>(d_desc.p), static_cast<int>(N), max_n, d_boxes, st));
  HIP_TRY(hipMemcpyAsync(w_host, d_boxes, box_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (the boxes are in, and the caller's buffer has been read)
  const unsigned* w = reinterpret_cast<const unsigned*>(w_host);
  for (size_t k = 0; k < N; k++) {
    DeviceCloud* c = scans[k].c.get();
    c->n = offsets[k + 1] - offsets[k];
    if (!c->n) continue;
    c->pts.borrow(block->pts.p + (offsets[k] - offsets[0]), c->n);
    c->owner = block;
    for (int v = 0; v < 2; v++)
      for (int i = 0; i < 3; i++) {
        c->bb_min[v][i] = ndt::box_word_decode(w[12 * k + 6 * v + i], true);
        c->bb_max[v][i] = ndt::box_word_decode(w[12 * k + 6 * v + 3 + i], false);
      }
    c->box_route = NDT_BOX_ROUTE_MULTI_WORDS;
  }
  return NDT_OK;
}

}  // namespace
}  // namespace ndtc

extern "C" {

static ndt_status map_update_impl(ndt_handle h, const void* scan, size_t n, size_t stride, int is_dense, bool on_device,
                                  const float* pose, float leaf, int* overflowed, const std::shared_ptr<DeviceCloud>* resident = nullptr) {
  if (!h || !(leaf > 0)) return fail(NDT_ERR_INVALID, "bad arguments");
  if (overflowed) *overflowed = 0;
  std::vector<MapScan> one(1);
  ndt_status s = NDT_OK;
  if (resident) one[0].c = *resident;  // an ndt_cloud: read where it lies
  else s = upload_cloud(h, scan, n, stride, on_device, one[0].c);
  if (s) return s;
  one[0].dense = is_dense;
  one[0].pose = pose;
  return map_update_scans(h, one, leaf, overflowed, nullptr);
}

ndt_status ndt_map_clear(ndt_handle h) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (h->map_pending) {
    ndt_status s = ensure_device(h);
    if (!s) s = map_complete(h);
    if (s) return s;
  }
  h->map_n = 0;
  h->map_dense = 1;
  h->map_boxes_known = false;
  return NDT_OK;
}

ndt_status ndt_map_update_cloud(ndt_handle h, ndt_cloud scan, int is_dense, const float* pose, float leaf, int* overflowed) {
  if (!h || !scan) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = ensure_device(h);
  if (!s) s = cloud_use_on(h, scan->c.get());
  if (s) return s;
  return map_update_impl(h, nullptr, scan->c->n, sizeof(float4), is_dense, true, pose, leaf, overflowed, &scan->c);
}

ndt_status ndt_map_update(ndt_handle h, const void* scan, size_t n, size_t stride, int is_dense, const float* pose, float leaf,
                          int* overflowed) {
  return map_update_impl(h, scan, n, stride, is_dense, false, pose, leaf, overflowed);
}
ndt_status ndt_map_update_device(ndt_handle h, const void* d_scan, size_t n, size_t stride, int is_dense, const float* pose,
                                 float leaf, int* overflowed) {
  return map_update_impl(h, d_scan, n, stride, is_dense, true, pose, leaf, overflowed);
}
ndt_status ndt_map_size(ndt_handle h, size_t* n) {
  if (!h || !n) return fail(NDT_ERR_INVALID, "bad arguments");
  if (h->map_pending) {
    ndt_status s = ensure_device(h);
    if (!s) s = map_complete(h);
    if (s) return s;
  }
  *n = h->map_n;
  return NDT_OK;
}
ndt_status ndt_map_get(ndt_handle h, void* out, size_t out_stride) {
  if (!h) return fail(NDT_ERR_INVALID, "bad arguments");
  if (out_stride < 16) return fail(NDT_ERR_INVALID, "out_stride_bytes must be >= 16");
  if (h->map_pending || h->map_stream) {
    ndt_status s = ensure_device(h);
    if (!s) s = map_complete(h);
    if (s) return s;
    HIP_TRY(hipStreamSynchronize(h->map_stream));  // (the download runs on the handle's stream)
  }
  if (h->map_n && !out) return fail(NDT_ERR_INVALID, "bad arguments");
  if (h->map_n == 0) return NDT_OK;
  return download_records(h, h->map_pts.p, h->map_n, out, out_stride);
}
ndt_status ndt_map_get_device(ndt_handle h, const void** d_pts, size_t* n) {
  if (!h || !d_pts || !n) return fail(NDT_ERR_INVALID, "bad arguments");
  if (h->device_ready) HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->map_stream) {
    ndt_status s = ensure_device(h);
    if (!s) s = map_complete(h);
    if (s) return s;
    HIP_TRY(hipStreamSynchronize(h->map_stream));
  }
  *d_pts = h->map_pts.p;
  *n = h->map_n;
  return NDT_OK;
}
void ndt_host_chain_pose(const float* pose, const float* transform, float* out) { ndt::chain_pose(pose, transform, out); }

ndt_status ndt_map_update_clouds(ndt_handle h, const ndt_cloud* scans, size_t n_scans, const int* is_dense, const float* poses,
                                 float leaf_size, int* overflowed) {
  ndt_status s = map_batch_checks(h, n_scans, leaf_size, overflowed);
  if (s) return s;
  if (n_scans && !scans) return fail(NDT_ERR_INVALID, "null scans");
  size_t points = 0;
  for (size_t k = 0; k < n_scans; k++) {
    if (!scans[k] || !scans[k]->c) return fail(NDT_ERR_INVALID, "null scan");
    points += scans[k]->c->n;  // (each at most INT_MAX, at most 65 535 of them: no wrap)
  }
  s = map_batch_total(h, points);
  if (s) return s;
  if (n_scans == 0) return NDT_OK;
  s = map_batch_begin(h, points);
  if (s) return s;
  std::vector<MapScan> list(n_scans);
  for (size_t k = 0; k < n_scans; k++) {
    s = cloud_use_on(h, scans[k]->c.get());
    if (s) return s;
    list[k].c = scans[k]->c;
  }
  return map_batch_run(h, list, is_dense, poses, leaf_size, overflowed);
}

ndt_status ndt_map_update_batch(ndt_handle h, const void* pts, const size_t* offsets, size_t n_scans, size_t stride_bytes,
                                const int* is_dense, const float* poses, float leaf_size, int on_device, int* overflowed) {
  ndt_status s = map_batch_checks(h, n_scans, leaf_size, overflowed);
  if (s) return s;
  if (n_scans && !offsets) return fail(NDT_ERR_INVALID, "null offsets");
  if (n_scans && (stride_bytes < 12 || stride_bytes % 4)) return fail(NDT_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  for (size_t k = 0; k < n_scans; k++)
    if (offsets[k + 1] < offsets[k]) return fail(NDT_ERR_INVALID, "offsets must not decrease");
  if (n_scans && offsets[n_scans] > offsets[0] && !pts) return fail(NDT_ERR_INVALID, "null point buffer");
  const size_t points = n_scans ? offsets[n_scans] - offsets[0] : 0;
  s = map_batch_total(h, points);
  if (s) return s;
  if (n_scans == 0) return NDT_OK;
  s = map_batch_begin(h, points);  // (before the buffer is staged: the staging writes the page-locked block a queued update reads)
  if (s) return s;
  std::vector<MapScan> list(n_scans);
  s = map_batch_stage(h, pts, offsets, n_scans, stride_bytes, on_device != 0, list);
  if (s) {
    (void)hipStreamSynchronize(h->stream);  // (nothing queued may still write into what goes back to the pool)
    return s;
  }
  return map_batch_run(h, list, is_dense, poses, leaf_size, overflowed);
}

ndt_status ndt_diag_map_batch(ndt_handle h, size_t* transform_launches, size_t* filters, size_t* box_passes) {
  if (!h || !transform_launches || !filters || !box_passes) return fail(NDT_ERR_INVALID, "bad arguments");
  *transform_launches = h->mb_transform_launches;
  *filters = h->mb_filters;
  *box_passes = h->mb_box_passes;
  return NDT_OK;
}

}  // extern "C"
