// ndt_map_batch.hip -- N2 of many posed scans in one call (ndt_map_update_clouds / _batch): transformPointCloud of every scan
// by its pose, one += of all of them behind the map, ONE pcl::VoxelGrid::filter of the concatenation.
//
// A call is one transform launch for all scans (k_transform_multi, straight into the room behind the map) and one filter
// (map_update_scans, ndt_grid.hip: the single ndt_map_update* calls are its list of one).  The clouds form reads resident
// ndt_clouds where they lie and knows their boxes.  The buffer form sends the whole buffer up with one copy and makes
// dense records and both boxes of every scan with one k_repack_bbox_multi launch -- the batched prefilter's front end --
// so no host pass over the points is needed; the caller's buffer is free when the call returns.
#include "ndt_internal.hpp"

namespace ndtc {
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
  }
  return NDT_OK;
}

}  // namespace
}  // namespace ndtc

extern "C" {

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
