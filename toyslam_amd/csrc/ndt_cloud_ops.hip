// ndt_cloud_ops.hip -- the host side of what the operations on resident clouds share (ndt_select.hip, ndt_deskew.hip,
// ndt_outliers.hip, ndt_plane.hip; declared in ndt_internal.hpp, the kernels' share is ndt_cloud_ops.hpp): the checks of an
// input cloud, the output slices of a call over a list, the fold of per-block box rows, the staging of per-point doubles.
#include "ndt_internal.hpp"

namespace ndtc {

std::shared_ptr<DeviceCloud> new_cloud(ndt_handle h) {
  auto c = std::make_shared<DeviceCloud>();
  c->device = h->device;
  c->made_on = h->stream;
  return c;
}

ndt_status cloud_checks(ndt_handle h, ndt_cloud c) {
  if (!c || !c->c) return fail(NDT_ERR_INVALID, "null cloud");
  if (c->c->device >= 0 && c->c->device != h->device) return fail(NDT_ERR_INVALID, "the cloud lives on another device");
  if (c->c->n > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  return NDT_OK;
}

ndt_status clouds_begin(size_t n_clouds, ndt_cloud* out_a, ndt_cloud* out_b) {
  if (n_clouds > 65535) return fail(NDT_ERR_INVALID, "at most 65535 clouds per call");
  for (size_t k = 0; k < n_clouds; k++) {
    if (out_a) out_a[k] = nullptr;
    if (out_b) out_b[k] = nullptr;
  }
  return NDT_OK;
}

void fold_box_rows(DeviceCloud* c, const float* rows, size_t stride, int b0, int nb, int route) {
  for (int b = b0; b < b0 + nb; b++) {
    const float* row = rows + static_cast<size_t>(b) * stride;
    for (int v = 0; v < 2; v++)
      for (int a = 0; a < 3; a++) {
        c->bb_min[v][a] = std::min(c->bb_min[v][a], row[v * 6 + a]);
        c->bb_max[v][a] = std::max(c->bb_max[v][a], row[v * 6 + 3 + a]);
      }
  }
  c->box_route = route;
}

ndt_status OutSlices::reserve(ndt_handle h, const std::vector<size_t>& first_points) {
  first = first_points;
  const size_t nc = first.size() - 1;
  blk = new_cloud(h);
  res.resize(nc);
  for (size_t k = 0; k < nc; k++) res[k] = new_cloud(h);
  HIP_TRY(blk->pts.reserve(std::max<size_t>(first[nc], 1)));
  blk->n = first[nc];
  return NDT_OK;
}

ndt_cloud OutSlices::publish(size_t k, size_t count) {
  res[k]->pts.borrow(at(k), count);
  res[k]->owner = blk;
  return new ndt_cloud_s{res[k]};
}

ndt_status doubles_in(hipStream_t st, const double* src, size_t n, int on_device, DevBuf<double>& buf, const double** d) {
  *d = src;
  if (n && !on_device) {
    HIP_TRY(buf.reserve(n));
    HIP_TRY(hipMemcpyAsync(buf.p, src, n * sizeof(double), hipMemcpyHostToDevice, st));
    *d = buf.p;
  }
  return NDT_OK;
}

ndt_status DoublesOut::reserve(double* dst_, size_t n_, int on_device_) {
  dst = dst_;
  n = n_;
  on_device = on_device_ != 0;
  if (n && !on_device) HIP_TRY(buf.reserve(n));
  return NDT_OK;
}

ndt_status DoublesOut::fetch(hipStream_t st) {
  if (n && !on_device) HIP_TRY(hipMemcpyAsync(dst, buf.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
  return NDT_OK;
}

int env_block_cap(const char* name, int cap) {
  const char* e = getenv(name);
  const int x = e ? atoi(e) : 0;
  return x > 0 ? std::min(x, cap) : cap;
}

}  // namespace ndtc
