// ndt_clouds.hip -- clouds on their way in and out: upload (repack, bounding boxes), download into the caller's records, the
// spatial ordering of sources (one scan, the scans of a batch), the ndt_cloud handles and the source setters.  What builds
// something FROM a cloud -- a grid, a filtered cloud, the map -- is in the unit of that task.
#include "ndt_internal.hpp"

#include <immintrin.h>

namespace ndtc {

// Host counterpart of k_repack_bbox for small clouds: records of `stride` bytes (x y z first) -> dense (x, y, z, 1) in dst,
// and the two bounding boxes of the cloud -- [0]: NaN coordinates dropped (what min / max do with them), [1]: finite
// points only (pcl::getMinMax3D for a cloud that is not dense).  min / max are exact and order-free, so the boxes are the
// ones the kernel's per-block rows reduce to.
static void host_repack_bbox(const unsigned char* src, size_t n, size_t stride, float* dst, float bb_min[2][3], float bb_max[2][3]) {
  __m128 mn0 = _mm_set1_ps(FLT_MAX), mx0 = _mm_set1_ps(-FLT_MAX), mn1 = mn0, mx1 = mx0;
  const __m128 keep_xyz = _mm_castsi128_ps(_mm_set_epi32(0, -1, -1, -1)), one_w = _mm_set_ps(1.0f, 0.0f, 0.0f, 0.0f);
  const __m128 abs_mask = _mm_castsi128_ps(_mm_set1_epi32(0x7fffffff)), inf = _mm_set1_ps(INFINITY);
  auto take = [&](__m128 v, float* out) {
    v = _mm_or_ps(_mm_and_ps(v, keep_xyz), one_w);
    _mm_store_ps(out, v);
    mn0 = _mm_min_ps(v, mn0);  // (min / max hand back their SECOND operand when the first is NaN)
    mx0 = _mm_max_ps(v, mx0);
    if ((_mm_movemask_ps(_mm_cmplt_ps(_mm_and_ps(v, abs_mask), inf)) & 7) == 7) {
      mn1 = _mm_min_ps(v, mn1);
      mx1 = _mm_max_ps(v, mx1);
    }
  };
  const size_t n_wide = (stride >= 16) ? n : (n ? n - 1 : 0);  // 12-B records: a 16-B load of the last one would leave the buffer
  for (size_t i = 0; i < n_wide; i++) take(_mm_loadu_ps(reinterpret_cast<const float*>(src + i * stride)), dst + 4 * i);
  for (size_t i = n_wide; i < n; i++) {
    const float* p = reinterpret_cast<const float*>(src + i * stride);
    take(_mm_set_ps(0.0f, p[2], p[1], p[0]), dst + 4 * i);
  }
  alignas(16) float a[4], b[4], c[4], d[4];
  _mm_store_ps(a, mn0); _mm_store_ps(b, mx0); _mm_store_ps(c, mn1); _mm_store_ps(d, mx1);
  for (int k = 0; k < 3; k++) {
    bb_min[0][k] = a[k]; bb_max[0][k] = b[k];
    bb_min[1][k] = c[k]; bb_max[1][k] = d[k];
  }
}

// The same, two points per instruction (AVX2; chosen at run time): 16 k points 16 -> ~9 us.  min / max are exact and order-free,
// so the boxes are the ones the one-point loop gives.
__attribute__((target("avx2"))) static void host_repack_bbox_avx2(const unsigned char* src, size_t n, size_t stride, float* dst,
                                                                  float bb_min[2][3], float bb_max[2][3]) {
  const __m256 big = _mm256_set1_ps(FLT_MAX), small = _mm256_set1_ps(-FLT_MAX);
  __m256 mn0 = big, mx0 = small, mn1 = big, mx1 = small;
  const __m256 keep_xyz = _mm256_castsi256_ps(_mm256_set_epi32(0, -1, -1, -1, 0, -1, -1, -1));
  const __m256 one_w = _mm256_set_ps(1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f);
  const __m256 abs_mask = _mm256_castsi256_ps(_mm256_set1_epi32(0x7fffffff)), inf = _mm256_set1_ps(INFINITY);
  const size_t n_wide = (stride >= 16) ? n : (n ? n - 1 : 0);  // 12-B records: a 16-B load of the last one would leave the buffer
  size_t i = 0;
  for (; i + 2 <= n_wide; i += 2) {
    __m256 v = _mm256_castps128_ps256(_mm_loadu_ps(reinterpret_cast<const float*>(src + i * stride)));
    v = _mm256_insertf128_ps(v, _mm_loadu_ps(reinterpret_cast<const float*>(src + (i + 1) * stride)), 1);
    v = _mm256_or_ps(_mm256_and_ps(v, keep_xyz), one_w);
    _mm256_storeu_ps(dst + 4 * i, v);
    mn0 = _mm256_min_ps(v, mn0);  // (min / max hand back their SECOND operand when the first is NaN)
    mx0 = _mm256_max_ps(v, mx0);
    const int fin = _mm256_movemask_ps(_mm256_cmp_ps(_mm256_and_ps(v, abs_mask), inf, _CMP_LT_OQ));
    if ((fin & 0x77) == 0x77) {  // both points finite (the usual case)
      mn1 = _mm256_min_ps(v, mn1);
      mx1 = _mm256_max_ps(v, mx1);
    } else {
      // one of the two (or neither): the other half is replaced by the neutral values
      const __m256 lo_ok = _mm256_castsi256_ps(_mm256_set_epi32(0, 0, 0, 0, -1, -1, -1, -1)), hi_ok = _mm256_castsi256_ps(_mm256_set_epi32(-1, -1, -1, -1, 0, 0, 0, 0));
      __m256 ok = _mm256_setzero_ps();
      if ((fin & 0x07) == 0x07) ok = _mm256_or_ps(ok, lo_ok);
      if ((fin & 0x70) == 0x70) ok = _mm256_or_ps(ok, hi_ok);
      mn1 = _mm256_min_ps(_mm256_or_ps(_mm256_and_ps(ok, v), _mm256_andnot_ps(ok, big)), mn1);
      mx1 = _mm256_max_ps(_mm256_or_ps(_mm256_and_ps(ok, v), _mm256_andnot_ps(ok, small)), mx1);
    }
  }
  float rest_min[2][3], rest_max[2][3];
  host_repack_bbox(src + i * stride, n - i, stride, dst + 4 * i, rest_min, rest_max);  // the odd point, the last 12-byte record
  alignas(32) float a[8], b[8], c[8], d[8];
  _mm256_store_ps(a, mn0); _mm256_store_ps(b, mx0); _mm256_store_ps(c, mn1); _mm256_store_ps(d, mx1);
  for (int k = 0; k < 3; k++) {
    bb_min[0][k] = std::min(std::min(a[k], a[4 + k]), rest_min[0][k]);
    bb_max[0][k] = std::max(std::max(b[k], b[4 + k]), rest_max[0][k]);
    bb_min[1][k] = std::min(std::min(c[k], c[4 + k]), rest_min[1][k]);
    bb_max[1][k] = std::max(std::max(d[k], d[4 + k]), rest_max[1][k]);
  }
}

// n dense float4 records from HBM into the caller's records of out_stride bytes: device -> the handle's page-locked
// staging (one contiguous DMA) -> the caller's buffer by the CPU.  A strided copy straight into pageable memory goes
// through the runtime's own staging in small pieces (measured 74 us for 256 KB; ~0.4 ms for the 1 MB of a filtered
// 70 k-point scan, most of the N1 call).  Synchronises the handle's stream.
ndt_status download_records(ndt_context* h, const float4* d_src, size_t n, void* out, size_t out_stride) {
  if (n == 0) return NDT_OK;
  if (ndt_status s = out_block_at_least(h, n * sizeof(float4))) return s;
  HIP_TRY(hipMemcpyAsync(h->out_pinned, d_src, n * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  spread_records(h->out_pinned, n, out, out_stride);
  return NDT_OK;
}
ndt_status out_block_at_least(ndt_context* h, size_t bytes) {
  if (h->out_pinned_bytes >= bytes) return NDT_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));  // (an earlier download may still be reading the old block)
  if (h->out_pinned) (void)hipHostFree(h->out_pinned);
  h->out_pinned = nullptr;
  h->out_pinned_bytes = 0;
  HIP_TRY(hipHostMalloc(&h->out_pinned, bytes + bytes / 4, hipHostMallocDefault));
  h->out_pinned_bytes = bytes + bytes / 4;
  return NDT_OK;
}
void spread_records(const void* src, size_t n, void* out, size_t out_stride) {
  const unsigned char* s = static_cast<const unsigned char*>(src);
  unsigned char* dst = static_cast<unsigned char*>(out);
  if (out_stride == sizeof(float4)) std::memcpy(out, src, n * sizeof(float4));
  else for (size_t i = 0; i < n; i++) std::memcpy(dst + i * out_stride, s + i * sizeof(float4), sizeof(float4));
}

// upload + repack to dense float4
ndt_status upload_cloud(ndt_context* h, const void* pts, size_t n, size_t stride, bool on_device,
                        std::shared_ptr<DeviceCloud>& out, bool by_reference) {
  if (n > 0 && !pts) return fail(NDT_ERR_INVALID, "null point buffer");
  if (stride < 12 || stride % 4) return fail(NDT_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  if (n > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  ndt_status s = ensure_device(h);
  if (s) return s;
  auto c = std::make_shared<DeviceCloud>();
  // by reference: dense 16-byte records already in HBM are used where they lie -- the caller keeps them alive and unchanged
  // while they are an input of this handle (what pcl::Registration's ConstPtr inputs promise); only the boxes are computed
  const bool borrowed = by_reference && on_device && n > 0 && stride == sizeof(float4) && (reinterpret_cast<uintptr_t>(pts) & 15) == 0;
  if (by_reference && !borrowed && n > 0) return fail(NDT_ERR_INVALID, "a cloud by reference must be device memory of 16-byte records on a 16-byte boundary");
  if (borrowed) c->pts.borrow(const_cast<float4*>(static_cast<const float4*>(pts)), n);
  else HIP_TRY(c->pts.reserve(n));
  c->n = n;
  // clouds of at most this many points take the host route (NDT_HOST_STAGE_MAX, 0 = never): the repack + bounding box pass
  // costs the host ~1 ns per point, the device route a blocking pageable copy, a kernel and a wait (~35 us whatever the size)
  static const size_t host_stage_max = [] {
    const char* v = getenv("NDT_HOST_STAGE_MAX");
    return std::min<size_t>(ndt_context::kStageSlotPoints, v ? static_cast<size_t>(std::max(0, atoi(v))) : 20480);
  }();
  if (n && !on_device && n <= host_stage_max) {
    const int slot = h->stage_next;
    h->stage_next = (slot + 1) % ndt_context::kStageSlots;
    if (!h->stage_host[slot]) {
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->stage_host[slot]), ndt_context::kStageSlotPoints * sizeof(float4), hipHostMallocDefault));
      HIP_TRY(hipEventCreateWithFlags(&h->stage_done[slot], hipEventDisableTiming));
    } else {
      HIP_TRY(hipEventSynchronize(h->stage_done[slot]));  // (four uploads ago: long done)
    }
    static const bool avx2 = [] { const char* v = getenv("NDT_HOST_AVX2"); return (!v || atoi(v) != 0) && __builtin_cpu_supports("avx2"); }();
    if (avx2) host_repack_bbox_avx2(static_cast<const unsigned char*>(pts), n, stride, h->stage_host[slot], c->bb_min, c->bb_max);
    else host_repack_bbox(static_cast<const unsigned char*>(pts), n, stride, h->stage_host[slot], c->bb_min, c->bb_max);
    c->box_route = avx2 ? NDT_BOX_ROUTE_HOST_AVX2 : NDT_BOX_ROUTE_HOST_SCALAR;
    HIP_TRY(ndt::launch_copy_records(reinterpret_cast<const float4*>(h->stage_host[slot]), c->pts.p, static_cast<int>(n), h->stream));
    HIP_TRY(hipEventRecord(h->stage_done[slot], h->stream));
  } else if (n) {
    const void* d_src = pts;
    // NDT_ZERO_COPY=1 (measured and left off): page-locked host memory of 16-byte records read by the repack kernel itself,
    // over the link -- one kernel and a poll of its rows instead of a copy into the staging buffer, the kernel and a stream
    // synchronisation.  The kernel's reads over PCIe run at 37 GB/s (26.5 us per 1 MB scan) against the copy engine's
    // ~50 GB/s plus a 5.6 us kernel: the node loop's prefilter 0.155 against 0.13-0.145 ms per scan on one box.
    static const bool zero_copy = [] { const char* v = getenv("NDT_ZERO_COPY"); return v && atoi(v) != 0; }();
    if (!on_device && zero_copy && stride == sizeof(float4) && (reinterpret_cast<uintptr_t>(pts) & 15) == 0) {
      hipPointerAttribute_t attr{};
      if (hipPointerGetAttributes(&attr, pts) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer) {
        d_src = attr.devicePointer;
        on_device = true;  // (for what follows: a source the device reads where it lies, copied by the kernel)
      } else {
        (void)hipGetLastError();  // pageable memory: not an error, the staging copy takes it
      }
    }
    if (!on_device) {
      HIP_TRY(h->staging.reserve(n * stride));
      HIP_TRY(hipMemcpyAsync(h->staging.p, pts, n * stride, hipMemcpyHostToDevice, h->stream));
      d_src = h->staging.p;
    }
    // repack and bounding boxes in one pass; the per-block rows come back behind the synchronisation
    // the upload needs anyway (the caller's buffer must be free to go when this returns)
    // (16-byte records: a block per CU and eight 16-byte loads in flight per thread; the rows travel over PCIe one by one,
    // so fewer, fatter blocks also mean fewer of those writes at the end of the kernel)
    const bool rec16 = stride == sizeof(float4) && (reinterpret_cast<uintptr_t>(d_src) & 15) == 0;
    const int nb = static_cast<int>(std::min<size_t>(rec16 ? 256 : 1024, (n + 255) / 256));
    if (!h->bbox_rows) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->bbox_rows), 1024 * 12 * sizeof(float), hipHostMallocDefault));
    // the kernel stores its per-block rows straight into pinned host memory (no D2H copy to queue)
    static const bool poll_rows = [] { const char* v = getenv("NDT_BBOX_POLL"); return !v || atoi(v) != 0; }();
    bool polled = false;
    if (on_device && rec16 && poll_rows) {
      // A cloud used where it lies: nothing is copied, so nothing has to be waited for but the rows themselves -- tagged
      // word by word and polled here (a stream synchronisation costs several microseconds beyond the kernel's end).
      // A device cloud the library copies: a block writes its row after its last read of the caller's records, so all rows
      // in = the caller's buffer is free; the copy's own stores are ordered before whatever this stream runs next.
      if (!h->bbox_tagged) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->bbox_tagged), 256 * 12 * sizeof(unsigned long long), hipHostMallocDefault));
        std::memset(h->bbox_tagged, 0, 256 * 12 * sizeof(unsigned long long));
      }
      if (++h->bbox_tag == 0) h->bbox_tag = 1;
      const unsigned tag = h->bbox_tag;
      HIP_TRY(ndt::launch_repack_bbox(d_src, n, stride, borrowed ? nullptr : c->pts.p, reinterpret_cast<float*>(h->bbox_tagged), nb, h->stream, tag));
      const volatile unsigned long long* w = h->bbox_tagged;
      const auto t0 = std::chrono::steady_clock::now();
      unsigned spins = 0;
      polled = true;
      for (int i = nb * 12 - 1; i >= 0 && polled; i--)
        while (static_cast<unsigned>(w[i]) != tag) {
          __builtin_ia32_pause();
          if ((++spins & 0xFFFF) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) { polled = false; break; }
        }
      if (!polled) {
        // two seconds without the rows: a stream that is merely slow (a profiler serialising it, long work queued ahead)
        // or a launch that failed / a device that hung.  Let the runtime say which: after a successful synchronisation the
        // kernel HAS run and its rows are valid.
        HIP_TRY(hipStreamSynchronize(h->stream));
        polled = true;
        for (int i = 0; i < nb * 12 && polled; i++) polled = static_cast<unsigned>(w[i]) == tag;
        if (!polled) return fail(NDT_ERR_HIP, "bounding-box rows did not arrive");
      }
      std::atomic_thread_fence(std::memory_order_acquire);
      for (int i = 0; i < nb * 12; i++) {
        const unsigned bits = static_cast<unsigned>(w[i] >> 32);
        std::memcpy(&h->bbox_rows[i], &bits, sizeof(float));
      }
    }
    if (!polled) {
      HIP_TRY(ndt::launch_repack_bbox(d_src, n, stride, borrowed ? nullptr : c->pts.p, h->bbox_rows, nb, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
    }
    const float* mm = h->bbox_rows;
    for (int b = 0; b < nb; b++)
      for (int v = 0; v < 2; v++)
        for (int k = 0; k < 3; k++) {
          c->bb_min[v][k] = std::min(c->bb_min[v][k], mm[b * 12 + v * 6 + k]);
          c->bb_max[v][k] = std::max(c->bb_max[v][k], mm[b * 12 + v * 6 + 3 + k]);
        }
    c->box_route = !rec16 ? NDT_BOX_ROUTE_REPACK : borrowed ? NDT_BOX_ROUTE_REC16_POLLED : NDT_BOX_ROUTE_REC16_COPY;
  }
  out = c;
  return NDT_OK;
}

// bounding box of a dense float4 device cloud: taken from the upload when the cloud came through
// upload_cloud (no kernel, no wait), else computed here (one kernel + one host round trip)

BBox bbox_of(const DeviceCloud& c, int dense) {
  BBox b;
  const int v = dense ? 0 : 1;
  for (int k = 0; k < 3; k++) {
    b.mn[k] = c.bb_min[v][k];
    b.mx[k] = c.bb_max[v][k];
  }
  return b;
}
ndt_status bbox_compute(ndt_context* h, const float4* d_pts, int n, int dense, BBox& out) {
  const int nb = std::min(1024, (n + 255) / 256);
  DevBuf<float> d_mm;
  HIP_TRY(d_mm.reserve(static_cast<size_t>(nb) * 6));
  HIP_TRY(ndt::launch_bbox(d_pts, n, dense, d_mm.p, nb, h->stream));
  std::vector<float> mm(static_cast<size_t>(nb) * 6);
  HIP_TRY(hipMemcpyAsync(mm.data(), d_mm.p, mm.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int k = 0; k < 3; k++) {
    out.mn[k] = FLT_MAX;
    out.mx[k] = -FLT_MAX;
  }
  for (int b = 0; b < nb; b++)
    for (int k = 0; k < 3; k++) {
      out.mn[k] = std::min(out.mn[k], mm[b * 6 + k]);
      out.mx[k] = std::max(out.mx[k], mm[b * 6 + 3 + k]);
    }
  return NDT_OK;
}

// Spatial ordering of a source range: counting sort by the cell of a lattice of pitch ~resolution
// laid over the range's own bounding box (x fastest), stable inside a cell.  Rigid transforms
// preserve locality, so whatever the pose, consecutive lanes of the derivative kernels land in
// the same or adjacent target voxels.  Only the order of the f64 summation changes.
ndt_status order_range(ndt_context* h, const float4* d_pts, size_t n, float pitch, float4* d_out, size_t* n_out,
                       const BBox* known_bbox) {
  *n_out = 0;
  if (n == 0) return NDT_OK;
  hipStream_t st = h->stream;
  const int ni = static_cast<int>(n);
  BBox bb;
  if (known_bbox) bb = *known_bbox;
  else { ndt_status sb = bbox_compute(h, d_pts, ni, 0, bb); if (sb) return sb; }
  const float* min_p = bb.mn;
  const float* max_p = bb.mx;
  if (!(min_p[0] <= max_p[0])) return NDT_OK;  // no finite point
  ndt::GridGeom geo{};
  // the pitch doubled until the lattice has at most 4e6 cells (either overflow status means far more: an extent of d cells
  // spans at least d / 2 of them, so over INT32_MAX by the reference's test is over 2^28 cells -- the same pitch is chosen)
  while (ndt::lattice_geometry(pitch, min_p, max_p, geo) != ndt::kLatticeOk || geo.n_cells > 4000000) pitch *= 2.0f;
  // Big clouds: stable radix passes of K1's order-preserving scatter (launch_order_radix) -- the same order, point for point,
  // as the counting sort below (NDT_ORDER=chain: that one always).
  static const bool radix_on = [] { const char* v = getenv("NDT_ORDER"); return !v || std::strcmp(v, "chain") != 0; }();
  static const size_t radix_from = [] { const char* v = getenv("NDT_ORDER_RADIX_FROM"); return v ? static_cast<size_t>(std::max(0, atoi(v))) : static_cast<size_t>(65536); }();
  if (radix_on && n >= radix_from && ndt::order_radix_passes(geo.n_cells) <= 3) {
    int digit_bits = 0;
    const size_t words = ndt::order_radix_cntmat_words(geo.n_cells, ni, nullptr, nullptr, &digit_bits);
    const int passes = ndt::order_radix_passes(geo.n_cells);
    DevBuf<unsigned> cntmat, bucket_base, counts;
    DevBuf<float4> tmp;
    HIP_TRY(cntmat.reserve(words));
    HIP_TRY(bucket_base.reserve((static_cast<size_t>(1) << digit_bits) + 1));
    HIP_TRY(counts.reserve(4));
    if (passes > 1) HIP_TRY(tmp.reserve(n));
    HIP_TRY(ndt::launch_order_radix(d_pts, ni, geo, cntmat.p, bucket_base.p, tmp.p, d_out, counts.p, st));
    unsigned kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, counts.p + (passes - 1), sizeof(kept), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_out = kept;
    return NDT_OK;
  }
  DevBuf<unsigned> cell_count, totals, rank;
  DevBuf<int> key;
  ChainBufs lv;
  HIP_TRY(cell_count.reserve(static_cast<size_t>(geo.n_cells)));
  HIP_TRY(key.reserve(n));
  HIP_TRY(rank.reserve(n));
  HIP_TRY(hipMemsetAsync(cell_count.p, 0, static_cast<size_t>(geo.n_cells) * sizeof(unsigned), st));
  HIP_TRY(ndt::launch_count(d_pts, ni, 0, geo, key.p, rank.p, cell_count.p, st));
  // the leaf count stays on the device (the kernels read it there): leaf arrays are sized for the
  // worst case and the host learns the totals once, at the end, instead of in the middle
  const size_t n_leaves = std::min<size_t>(n, static_cast<size_t>(geo.n_cells));
  HIP_TRY(totals.reserve(4));
  HIP_TRY(lv.reserve(n_leaves, n));
  if (ndt_status s = chain_scan_scatter(st, cell_count.p, geo.n_cells, 1, key.p, rank.p, ni, lv.out(), totals.p)) return s;
  HIP_TRY(ndt::launch_sort_gather(d_pts, lv.leaf_start.p, lv.leaf_count.p, static_cast<int>(n_leaves), lv.sorted_idx.p, d_out, st, totals.p));
  unsigned tot[3];
  HIP_TRY(hipMemcpyAsync(tot, totals.p, sizeof(tot), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *n_out = tot[0];
  return NDT_OK;
}

// The scans of a batch in count / scan / scatter passes (composite key: the scan's first counter + its cell); the ordered
// points of scan k end up contiguous at scan_starts[k] (non-finite points are dropped, so the segments are compacted).
// A scan's order must not depend on the batch around it -- a member of a lock-step batch gets the same sums, bit for bit,
// whichever group or rank it is registered in (tools/fuzz_batch.py) -- so every scan is ordered on a lattice of its own:
// pitch `resolution` (doubled only while that ONE scan's box has more than kMaxCounters cells), box from its own points.
// Scans go through in passes of at most kMaxCounters counters.
ndt_status order_batch(ndt_context* h, DeviceCloud* c, const size_t* offsets, size_t n_scans) {
  hipStream_t st = h->stream;
  c->scan_counts.assign(n_scans, 0);
  c->scan_starts.assign(n_scans + 1, 0);
  c->n_sorted = 0;
  if (n_scans == 0 || c->n == 0) return NDT_OK;
  constexpr double kMaxCounters = 32.0e6;
  // ---- per-scan bounding boxes (one kernel, one small copy back)
  std::vector<int> off(n_scans + 1);
  size_t max_scan = 0;
  for (size_t k = 0; k <= n_scans; k++) off[k] = static_cast<int>(offsets[k] - offsets[0]);
  for (size_t k = 0; k < n_scans; k++) max_scan = std::max(max_scan, offsets[k + 1] - offsets[k]);
  DevBuf<int> d_off, d_box;
  HIP_TRY(d_off.reserve(n_scans + 1));
  HIP_TRY(d_box.reserve(6 * n_scans));
  std::vector<int> box(6 * n_scans);
  for (size_t k = 0; k < n_scans; k++)
    for (int j = 0; j < 6; j++) box[6 * k + j] = j < 3 ? std::numeric_limits<int>::max() : std::numeric_limits<int>::min();
  HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), (n_scans + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_box.p, box.data(), box.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(ndt::launch_scan_bboxes(c->pts.p, d_off.p, static_cast<int>(n_scans), static_cast<int>(max_scan), d_box.p, st));
  HIP_TRY(hipMemcpyAsync(box.data(), d_box.p, box.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // ---- every scan's own lattice
  std::vector<ndt::ScanLattice> lat(n_scans);
  for (size_t k = 0; k < n_scans; k++) {
    ndt::ScanLattice& L = lat[k];
    L = ndt::ScanLattice{};
    if (box[6 * k] > box[6 * k + 3]) continue;  // no finite point: n_cells 0
    float mn[3], mx[3];
    for (int j = 0; j < 3; j++) { mn[j] = ndt::scan_bbox_decode(box[6 * k + j]); mx[j] = ndt::scan_bbox_decode(box[6 * k + 3 + j]); }
    for (float pitch = h->resolution;; pitch *= 2.0f) {
      const float inv = 1.0f / pitch;
      double cells = 1;
      int div[3];
      for (int j = 0; j < 3; j++) {
        L.min_b[j] = static_cast<int>(std::floor(mn[j] * inv));
        div[j] = static_cast<int>(std::floor(mx[j] * inv)) - L.min_b[j] + 1;
        cells *= div[j];
      }
      if (cells <= kMaxCounters) {
        L.inv_leaf = inv;
        L.mul1 = div[0];
        L.mul2 = div[0] * div[1];
        L.n_cells = static_cast<int>(cells);
        break;
      }
    }
  }
  DevBuf<unsigned> cell_count, totals, rank, d_starts;
  DevBuf<int> key;
  ChainBufs lv;
  DevBuf<ndt::ScanLattice> d_lat;
  DevBuf<long long> d_bases;
  size_t out_base = 0;
  for (size_t s0 = 0; s0 < n_scans;) {
    // this pass: scans [s0, s0 + ns) while their counters fit
    size_t ns = 0;
    long long total_cells = 0;
    while (s0 + ns < n_scans && (ns == 0 || static_cast<double>(total_cells + lat[s0 + ns].n_cells) <= kMaxCounters)) {
      lat[s0 + ns].base = total_cells;
      total_cells += lat[s0 + ns].n_cells;
      ns++;
    }
    const size_t first_pt = offsets[s0] - offsets[0], n_pts = offsets[s0 + ns] - offsets[s0];
    if (n_pts == 0 || total_cells == 0) {
      for (size_t k = 0; k < ns; k++) c->scan_starts[s0 + k] = out_base;
      s0 += ns;
      continue;
    }
    const int ni = static_cast<int>(n_pts);
    const float4* in = c->pts.p + first_pt;
    std::vector<int> poff(ns + 1);
    std::vector<long long> bases(ns + 1);
    size_t pass_max = 0;
    for (size_t k = 0; k <= ns; k++) poff[k] = static_cast<int>(offsets[s0 + k] - offsets[s0]);
    for (size_t k = 0; k < ns; k++) {
      pass_max = std::max(pass_max, offsets[s0 + k + 1] - offsets[s0 + k]);
      bases[k] = lat[s0 + k].base;
    }
    bases[ns] = total_cells;  // the sentinel cell: the pass's total
    HIP_TRY(d_off.reserve(ns + 1));
    HIP_TRY(d_lat.reserve(ns));
    HIP_TRY(d_bases.reserve(ns + 1));
    HIP_TRY(d_starts.reserve(ns + 1));
    HIP_TRY(hipMemcpyAsync(d_off.p, poff.data(), (ns + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_lat.p, lat.data() + s0, ns * sizeof(ndt::ScanLattice), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_bases.p, bases.data(), (ns + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    HIP_TRY(cell_count.reserve(static_cast<size_t>(total_cells) + 1));
    HIP_TRY(key.reserve(n_pts));
    HIP_TRY(rank.reserve(n_pts));
    HIP_TRY(hipMemsetAsync(cell_count.p, 0, (static_cast<size_t>(total_cells) + 1) * sizeof(unsigned), st));
    HIP_TRY(ndt::launch_count_batch(in, d_off.p, static_cast<int>(ns), static_cast<int>(pass_max), d_lat.p, key.p, rank.p, cell_count.p, st));
    // one extra (always empty) cell at the end so that its start offset is the pass's total
    const long long scan_cells = total_cells + 1;
    const size_t n_leaves = std::min<size_t>(n_pts, static_cast<size_t>(scan_cells));  // upper bound; the count stays on the device
    HIP_TRY(totals.reserve(4));
    HIP_TRY(lv.reserve(n_leaves, n_pts));
    if (ndt_status s = chain_scan(st, cell_count.p, scan_cells, 1, lv.out(), totals.p)) return s;
    unsigned tot[3];
    HIP_TRY(hipMemcpyAsync(tot, totals.p, sizeof(tot), hipMemcpyDeviceToHost, st));  // read after the pass's synchronise
    // start offset of every scan's first cell (+ the sentinel cell)
    std::vector<unsigned> starts(ns + 1);
    HIP_TRY(ndt::launch_pick(cell_count.p, d_bases.p, d_starts.p, static_cast<int>(ns + 1), st));
    HIP_TRY(hipMemcpyAsync(starts.data(), d_starts.p, (ns + 1) * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(ndt::launch_scatter(key.p, rank.p, ni, cell_count.p, lv.sorted_idx.p, st));
    HIP_TRY(ndt::launch_sort_gather(in, lv.leaf_start.p, lv.leaf_count.p, static_cast<int>(n_leaves), lv.sorted_idx.p, c->sorted.p + out_base, st, totals.p));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t k = 0; k < ns; k++) {
      c->scan_starts[s0 + k] = out_base + starts[k];
      c->scan_counts[s0 + k] = starts[k + 1] - starts[k];
    }
    out_base += starts[ns];
    c->n_sorted += tot[0];
    s0 += ns;
  }
  c->scan_starts[n_scans] = out_base;
  return NDT_OK;
}

ndt_status order_cloud(ndt_context* h, DeviceCloud* c, const size_t* offsets, size_t n_scans) {
  // Spatial ordering pays for itself only on big scans (measured: 5-6 us per evaluation at 100k points
  // against a 1M-point target, nothing at <= 60k points where the voxel records stay in L2 anyway,
  // for 85-170 us of ordering work).  NDT_SORT_SOURCE=0 / 1 forces it off / on; a lock-step batch is
  // always ordered (its points are concatenated scan by scan).
  static const int mode = [] { const char* v = getenv("NDT_SORT_SOURCE"); return v ? (atoi(v) != 0 ? 1 : 0) : -1; }();
  constexpr size_t kOrderFrom = 65536;
  c->n_sorted = 0;
  const bool enabled = mode < 0 ? (offsets != nullptr || c->n >= kOrderFrom) : mode != 0;
  if (!enabled || c->n == 0) return NDT_OK;
  HIP_TRY(c->sorted.reserve(c->n));
  if (!offsets) {
    size_t got = 0;
    const BBox bb = bbox_of(*c, 0);
    ndt_status s = order_range(h, c->pts.p, c->n, h->resolution, c->sorted.p, &got, &bb);
    if (s) return s;
    c->n_sorted = got;
  } else {
    ndt_status s = order_batch(h, c, offsets, n_scans);
    if (s) return s;
  }
  return NDT_OK;
}

// ---- ndt_cloud: clouds that stay in HBM between the steps of a node's loop ----------------------------------------------
// the cloud is about to be read by work on h's stream: order that stream behind the cloud's making, remember it for the
// cloud's release
ndt_status cloud_use_on(ndt_handle h, DeviceCloud* c) {
  if (c->made_on && c->made_on != h->stream) {
    if (c->device != h->device) return fail(NDT_ERR_INVALID, "the cloud lives on another device");
    if (!DevPool::instance().retired(c->made_on)) HIP_TRY(hipStreamSynchronize(c->made_on));  // (a destroyed stream's work is over)
    if (std::find(c->used_on.begin(), c->used_on.end(), h->stream) == c->used_on.end()) c->used_on.push_back(h->stream);
  }
  return NDT_OK;
}

}  // namespace ndtc

extern "C" {

static ndt_status set_source_impl(ndt_handle h, const void* pts, size_t n, size_t stride, bool on_device, bool by_ref = false) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  std::shared_ptr<DeviceCloud> c;
  ndt_status s = upload_cloud(h, pts, n, stride, on_device, c, by_ref);
  if (s) return s;
  s = order_cloud(h, c.get(), nullptr, 0);
  if (s) return s;
  h->source = c;
  return NDT_OK;
}
ndt_status ndt_set_input_source(ndt_handle h, const void* pts, size_t n, size_t stride) {
  return set_source_impl(h, pts, n, stride, false);
}
ndt_status ndt_set_input_source_device(ndt_handle h, const void* pts, size_t n, size_t stride) {
  return set_source_impl(h, pts, n, stride, true);
}
ndt_status ndt_set_input_source_device_ref(ndt_handle h, const void* d_pts, size_t n) {
  return set_source_impl(h, d_pts, n, sizeof(float4), true, true);
}

ndt_status ndt_share_input_source(ndt_handle dst, ndt_handle src) {
  if (!dst || !src) return fail(NDT_ERR_INVALID, "null handle");
  if (!src->source) return fail(NDT_ERR_NO_INPUT, "the donor handle has no input source");
  if (dst == src) return NDT_OK;
  if (dst->device != src->device) return fail(NDT_ERR_INVALID, "handles on different devices");
  // the cloud was uploaded and ordered on the donor's stream; what `dst` still runs on its old source must be over
  // before that cloud can go back to the pool
  HIP_TRY(hipSetDevice(src->device));
  if (src->device_ready) HIP_TRY(hipStreamSynchronize(src->stream));
  ndt_status s = ensure_device(dst);
  if (s) return s;
  HIP_TRY(hipStreamSynchronize(dst->stream));
  dst->source = src->source;
  return NDT_OK;
}

ndt_status ndt_cloud_upload(ndt_handle h, const void* pts, size_t n, size_t stride, ndt_cloud* out) {
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  *out = nullptr;
  std::shared_ptr<DeviceCloud> c;
  ndt_status s = upload_cloud(h, pts, n, stride, false, c);
  if (s) return s;
  c->device = h->device;
  c->made_on = h->stream;
  *out = new ndt_cloud_s{c};
  return NDT_OK;
}

ndt_status ndt_cloud_size(ndt_cloud c, size_t* n) {
  if (!c || !n) return fail(NDT_ERR_INVALID, "bad arguments");
  *n = c->c->n;
  return NDT_OK;
}
ndt_status ndt_cloud_data(ndt_cloud c, const void** d_pts, size_t* n) {
  if (!c || !d_pts || !n) return fail(NDT_ERR_INVALID, "bad arguments");
  *d_pts = c->c->pts.p;
  *n = c->c->n;
  return NDT_OK;
}
ndt_status ndt_cloud_download(ndt_handle h, ndt_cloud c, void* out, size_t out_stride) {
  if (!h || !c || (c->c->n && !out)) return fail(NDT_ERR_INVALID, "bad arguments");
  if (out_stride < 16) return fail(NDT_ERR_INVALID, "out_stride_bytes must be >= 16");
  ndt_status s = ensure_device(h);
  if (!s) s = cloud_use_on(h, c->c.get());
  if (s) return s;
  return download_records(h, c->c->pts.p, c->c->n, out, out_stride);
}
void ndt_cloud_release(ndt_cloud c) { delete c; }

static void write_bounds(const float bb_min[2][3], const float bb_max[2][3], float out[12]) {
  for (int v = 0; v < 2; v++)
    for (int k = 0; k < 3; k++) {
      out[6 * v + k] = bb_min[v][k];
      out[6 * v + 3 + k] = bb_max[v][k];
    }
}
static void write_bounds(const DeviceCloud& c, float out[12], int* route) {
  write_bounds(c.bb_min, c.bb_max, out);
  if (route) *route = c.box_route;
}
ndt_status ndt_cloud_bounds(ndt_cloud c, float out[12], int* route) {
  if (!c || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  write_bounds(*c->c, out, route);
  return NDT_OK;
}
ndt_status ndt_diag_input_bounds(ndt_handle h, int which, float out[12], int* route) {
  if (!h || !out || which < 0 || which > 2) return fail(NDT_ERR_INVALID, "bad arguments");
  if (which == 2) {
    if (h->map_pending) {
      ndt_status s = ensure_device(h);
      if (!s) s = map_settle(h);
      if (s) return s;
    }
    if (!h->map_boxes_known) return fail(NDT_ERR_NO_INPUT, "the map's boxes are not known");
    write_bounds(h->map_boxes, out, route);
    return NDT_OK;
  }
  const std::shared_ptr<DeviceCloud>& c = which == 0 ? h->source : h->target;
  if (!c) return fail(NDT_ERR_NO_INPUT, which == 0 ? "no input source" : "no input target");
  write_bounds(*c, out, route);
  return NDT_OK;
}
ndt_status ndt_host_repack_bbox(const void* pts, size_t n, size_t stride, int avx2, float* out_records, float out_bounds[12]) {
  if ((n && (!pts || !out_records)) || !out_bounds) return fail(NDT_ERR_INVALID, "bad arguments");
  if (stride < 12 || stride % 4) return fail(NDT_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  if (reinterpret_cast<uintptr_t>(out_records) & 15) return fail(NDT_ERR_INVALID, "out_records must be on a 16-byte boundary");
  if (avx2 && !__builtin_cpu_supports("avx2")) return fail(NDT_ERR_INVALID, "this CPU has no AVX2");
  float bb_min[2][3], bb_max[2][3];
  if (avx2) ndtc::host_repack_bbox_avx2(static_cast<const unsigned char*>(pts), n, stride, out_records, bb_min, bb_max);
  else ndtc::host_repack_bbox(static_cast<const unsigned char*>(pts), n, stride, out_records, bb_min, bb_max);
  write_bounds(bb_min, bb_max, out_bounds);
  return NDT_OK;
}

ndt_status ndt_set_input_source_cloud(ndt_handle h, ndt_cloud c) {
  if (!h || !c) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = ensure_device(h);
  if (!s) s = cloud_use_on(h, c->c.get());
  if (s) return s;
  // Big scans are registered from a copy in lattice order whose pitch is this handle's resolution (order_cloud): that copy
  // belongs to the handle, not to the shared cloud -- a view of the cloud's points with an ordered copy of its own.
  auto view = std::make_shared<DeviceCloud>();
  view->pts.borrow(c->c->pts.p, c->c->n);
  view->n = c->c->n;
  std::memcpy(view->bb_min, c->c->bb_min, sizeof(view->bb_min));
  std::memcpy(view->bb_max, c->c->bb_max, sizeof(view->bb_max));
  view->box_route = c->c->box_route;
  s = order_cloud(h, view.get(), nullptr, 0);
  if (s) return s;
  if (view->n_sorted == 0) {  // (the usual case at the nodes' size: nothing to order, the cloud itself is the source)
    h->source = c->c;
    return NDT_OK;
  }
  view->parent = c->c;
  h->source = view;
  return NDT_OK;
}

}  // extern "C"
