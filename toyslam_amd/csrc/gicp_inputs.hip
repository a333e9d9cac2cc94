// gicp_inputs.hip -- what makes a cloud an input of a GICP registration (a GicpInput, gicp_internal.hpp): its search index,
// the finite check, the covariance passes; and the entry points that set or inspect the handle's two inputs.
#include "gicp_internal.hpp"

namespace {
// The index of a host cloud: finite check on the host, upload (which computes the box), gicp_index_cloud.
ndt_status gicp_build_index(ndt_context* c, const void* pts, size_t n, size_t stride, LeafHint& hint, GicpInput& in) {
  if (!pts || n == 0) return fail(NDT_ERR_INVALID, "invalid or empty point cloud dataset given");
  if (stride < 12 || stride % 4) return fail(NDT_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  const unsigned char* base = static_cast<const unsigned char*>(pts);
  for (size_t i = 0; i < n; i++) {
    float p[3];
    std::memcpy(p, base + i * stride, sizeof(p));
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2])))
      return fail(NDT_ERR_INVALID, "GICP needs finite points (point " + std::to_string(i) + " is not)");
  }
  ndt_status s = ensure_device(c);
  if (s) return s;
  std::shared_ptr<DeviceCloud> cloud;
  s = upload_cloud(c, pts, n, stride, false, cloud);
  if (s) return s;
  return gicp_index_cloud(c, cloud, hint, in);
}

// packed covariances [n][6] (the upper triangle, row by row) <-> [n][9] row-major 3x3
void cov9_from_cov6(const double* c6, size_t n, double* c9) {
  for (size_t i = 0; i < n; i++) {
    const double* s6 = c6 + i * 6;
    double* o = c9 + i * 9;
    o[0] = s6[0]; o[1] = s6[1]; o[2] = s6[2];
    o[3] = s6[1]; o[4] = s6[3]; o[5] = s6[4];
    o[6] = s6[2]; o[7] = s6[4]; o[8] = s6[5];
  }
}
void cov6_from_cov9(const double* c9, size_t n, double* c6) {
  for (size_t i = 0; i < n; i++) {
    const double* m = c9 + i * 9;
    double* o = c6 + i * 6;
    o[0] = m[0]; o[1] = m[1]; o[2] = m[2]; o[3] = m[4]; o[4] = m[5]; o[5] = m[8];
  }
}

// what every input setter starts with: the input is not set (and stays so if the setter fails), its covariances are gone
// (target_covariances_.reset() / input_covariances_.reset())
GicpInput& gicp_unset(gicp_context* h, int which) {
  GicpInput& in = h->in[which];
  in.set = in.have_cov = in.user_cov = false;
  if (which == 0 && in.vox) {  // a voxel target (gicp_set_input_target_grid): the binding is dropped
    in.vox = nullptr;
    h->grid_target.map = nullptr;
    h->grid_target.valid = false;
  }
  h->step_ready = false;
  return in;
}

// computeCovariances of one cloud (lazily, gicp_omp_impl.hpp:385-397).  on_src_stream: the handle's source, whose pass runs
// on the stream its index was built on, next to the target's (two independent kernels of a few thousand waves each);
// everything that follows on the main stream waits for it through an event (gicp_join_source)
ndt_status gicp_cloud_covariances(gicp_context* h, GicpInput& in, bool on_src_stream, bool want_neighbors) {
  if (in.have_cov && !want_neighbors) return NDT_OK;
  const size_t n = in.n();
  const int k = h->prm.k_correspondences;
  if (k > static_cast<int>(n))  // :53-57: PCL_ERROR and return, the covariances stay empty
    return fail(NDT_ERR_INVALID, "number of points in cloud (" + std::to_string(n) + ") is less than k_correspondences_ (" +
                                     std::to_string(k) + ")");
  HIP_TRY(in.cov.reserve(n * 6));
  if (want_neighbors) {
    HIP_TRY(h->nn_idx.reserve(n * static_cast<size_t>(k)));
    HIP_TRY(h->nn_d2.reserve(n * static_cast<size_t>(k)));
  }
  hipStream_t st = on_src_stream ? h->src.stream : h->tgt.stream;
  HIP_TRY(gicp::launch_knn_covariances(gicp_index_of(in), k, h->prm.gicp_epsilon, gicp::knn_blocks(static_cast<int>(n), kGicpMaxBlocks),
                                       in.cov.p, want_neighbors ? h->nn_idx.p : nullptr, want_neighbors ? h->nn_d2.p : nullptr, st));
  if (on_src_stream) {
    if (!h->ev_src) HIP_TRY(hipEventCreateWithFlags(&h->ev_src, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->ev_src, h->src.stream));
    h->src_cov_pending = true;  // gicp_join_source makes the main stream wait -- after the target's pass has been queued
  }
  in.have_cov = true;
  return NDT_OK;
}

ndt_status gicp_join_source(gicp_context* h) {
  if (h->src_cov_pending) {
    HIP_TRY(hipStreamWaitEvent(h->tgt.stream, h->ev_src, 0));
    h->src_cov_pending = false;
  }
  return NDT_OK;
}

// What the two kinds of input setter share.  Head: the input is unset, then the main stream is waited for before the old index
// goes -- kernels of an earlier align may still read it.  Tail: the source's own stream is waited for -- the index is read from the
// main stream from here on -- and the input is set.  A resident cloud that is none (!usable) is refused before any device call, and
// its main stream is made where there is none; a host cloud's own refusals come with its upload (middle), behind the wait.
template <class Middle>
ndt_status gicp_set_input(gicp_context* h, int which, bool resident, bool usable, Middle middle) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  GicpInput& in = gicp_unset(h, which);
  if (resident) {
    if (!usable) return fail(NDT_ERR_INVALID, "invalid or empty point cloud dataset given");
    const ndt_status s = ensure_device(&h->tgt);
    if (s) return s;
  } else if (h->tgt.device_ready) {
    HIP_TRY(hipSetDevice(h->tgt.device));
  }
  if (h->tgt.device_ready) HIP_TRY(hipStreamSynchronize(h->tgt.stream));
  ndt_context* c = h->builder(which);
  const ndt_status s = middle(c, in);
  if (s) return s;
  if (which == 1) HIP_TRY(hipStreamSynchronize(c->stream));
  in.set = true;
  return NDT_OK;
}
}  // namespace

namespace ndtc {
// The extents of a cloud's finite box and the clamp that keeps a dense cell table over it within budget
namespace {
struct LeafClamp {
  double ext[3], vol = 1.0;
  explicit LeafClamp(const DeviceCloud& cloud) {
    for (int k = 0; k < 3; k++) {
      ext[k] = std::max(static_cast<double>(cloud.bb_max[1][k]) - static_cast<double>(cloud.bb_min[1][k]), 1e-3);
      vol *= ext[k];
    }
  }
  float operator()(double leaf) const {
    leaf = std::max(leaf, 1e-4);
    for (int it = 0; it < 64; it++) {  // keep the dense cell table within budget
      const double cells = (ext[0] / leaf + 2) * (ext[1] / leaf + 2) * (ext[2] / leaf + 2);
      if (cells <= static_cast<double>(kGicpMaxCells)) break;
      leaf *= 1.26;
    }
    return static_cast<float>(leaf);
  }
};
}  // namespace

float index_leaf_clamped(const DeviceCloud& cloud, double want) { return LeafClamp(cloud)(want); }

// Leaf size from the cloud's own density (volume guess first, then corrected once from the measured points per occupied cell
// -- scans are surfaces, so occupancy grows with the square of the leaf).  What GICP's index and the statistical outlier
// filter's share.
ndt_status index_cloud_by_density(ndt_context* c, const std::shared_ptr<DeviceCloud>& cloud, bool dense, float leaf0, float* leaf_out,
                                  std::shared_ptr<DeviceGrid>& grid) {
  const size_t n = cloud->n;
  ndt_status s = NDT_OK;
  const LeafClamp clamp_leaf(*cloud);
  float leaf = leaf0 > 0 ? clamp_leaf(leaf0) : clamp_leaf(std::cbrt(clamp_leaf.vol * kGicpPointsPerCell / static_cast<double>(std::max<size_t>(n, 1))));
  for (int pass = 0; pass < 4; pass++) {
    s = build_grid(c, cloud, GridSpec{leaf, 1, c->eig_ratio, 0, dense, true}, grid);  // cells and their point lists only
    if (s) return s;
    s = grid_counts(c, grid.get());
    if (s) return s;
    if (grid->empty) break;  // (no finite point: nothing to index)
    const double per_cell = static_cast<double>(n) / static_cast<double>(std::max<size_t>(grid->n_leaves, 1));
    if (per_cell <= 2.0 * kGicpPointsPerCell && (per_cell >= 0.4 * kGicpPointsPerCell || grid->n_leaves <= 8)) break;
    // too coarse (dense surfaces) or too fine (flat / thin clouds, where the volume guess means little)
    const float next = clamp_leaf(static_cast<double>(leaf) * std::sqrt(kGicpPointsPerCell / per_cell));
    if (next < 0.9f * leaf || next > 1.1f * leaf) leaf = next;
    else break;
  }
  if (leaf_out) *leaf_out = leaf;
  return NDT_OK;
}

// The voxel index of `cloud` (on the device, every point finite -- so the box the cloud carries over its finite points is
// the box of all of them) into in.grid: leaf size from the cloud's own density (index_cloud_by_density).
// Built with `c`: its stream, its scratch, its pool (the caller has made `c` current); `c` holds neither the cloud nor the grid.
ndt_status gicp_index_cloud(ndt_context* c, const std::shared_ptr<DeviceCloud>& cloud, LeafHint& hint, GicpInput& in) {
  in.grid.reset();  // (before the new one is allocated: an input never holds two)
  std::shared_ptr<DeviceGrid> grid;
  const size_t n = cloud->n;
  // start from the leaf the previous cloud of about this size ended up with (usually right at once; the search results do
  // not depend on the leaf, only the time does)
  const float leaf0 = hint.leaf > 0 && n >= hint.n - hint.n / 4 && n <= hint.n + hint.n / 4 ? hint.leaf : 0.f;
  float leaf = 0.f;
  ndt_status s = index_cloud_by_density(c, cloud, true, leaf0, &leaf, grid);
  if (s) return s;
  if (std::getenv("NDT_GICP_DEBUG"))
    std::fprintf(stderr, "[gicp index] n=%zu leaf=%.4f cells=%lld (%d x %d x %d) occupied=%zu\n", n, static_cast<double>(leaf),
                 grid->geom.n_cells, grid->geom.div_b[0], grid->geom.div_b[1], grid->geom.div_b[2], grid->n_leaves);
  hint.leaf = leaf;
  hint.n = n;
  s = ensure_cell2leaf(c, grid.get());
  if (!s) in.grid = std::move(grid);
  return s;
}

// One device pass, one launch, over all of `clouds` (on h->tgt's stream): bad[m] = points of clouds[m] that are not finite.
// One small read-back; the points stay where they are.
ndt_status gicp_finite_check(gicp_context* h, const std::vector<const DeviceCloud*>& clouds, std::vector<unsigned>& bad) {
  const size_t m = clouds.size();
  bad.assign(m, 0);
  if (m == 0) return NDT_OK;
  std::vector<gicp::FiniteMember> tab(m);
  long long blocks = 0;
  for (size_t i = 0; i < m; i++) {
    tab[i].pts = clouds[i]->pts.p;
    tab[i].n = static_cast<int>(clouds[i]->n);
    tab[i].first_block = static_cast<int>(blocks);
    blocks += gicp::finite_blocks(tab[i].n);
  }
  if (blocks > static_cast<long long>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points in the named clouds");
  hipStream_t st = h->tgt.stream;
  HIP_TRY(h->member_table.reserve(m * sizeof(gicp::FiniteMember)));
  HIP_TRY(h->finite_counts.reserve(m));
  StreamDrain drain{st};  // `tab` is pageable: whatever path leaves, its copy has run before it dies
  HIP_TRY(hipMemcpyAsync(h->member_table.p, tab.data(), m * sizeof(gicp::FiniteMember), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(h->finite_counts.p, 0, m * sizeof(unsigned), st));
  HIP_TRY(gicp::launch_count_nonfinite_multi(reinterpret_cast<const gicp::FiniteMember*>(h->member_table.p), static_cast<int>(m),
                                             static_cast<int>(blocks), h->finite_counts.p, st));
  HIP_TRY(hipMemcpyAsync(bad.data(), h->finite_counts.p, m * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  drain.done = true;
  return NDT_OK;
}

// the covariances of `in` to the host as [n][9], behind everything queued on the main stream, which is waited for
ndt_status gicp_read_covariances(gicp_context* h, const GicpInput& in, double* cov9) {
  const size_t n = in.n();
  std::vector<double> c6(n * 6);
  HIP_TRY(hipMemcpyAsync(c6.data(), in.covariances(), n * 6 * sizeof(double), hipMemcpyDeviceToHost, h->tgt.stream));
  HIP_TRY(hipStreamSynchronize(h->tgt.stream));
  cov9_from_cov6(c6.data(), n, cov9);
  return NDT_OK;
}

// covariances of both clouds + the guess-moved source (:385-403); guess_rm: the guess, row-major.  An input that has its
// covariances (every record of a pairs call) launches nothing here: only the handle's own source ever uses src's stream.
ndt_status gicp_prepare_covariances(gicp_context* h, GicpInput& tgt, GicpInput& src) {
  ndt_status s = gicp_scratch(h);
  if (s) return s;
  s = gicp_cloud_covariances(h, src, true, false);  // (source first: it runs on its own stream while the target's is queued here)
  if (s) return s;
  s = gicp_cloud_covariances(h, tgt, false, false);
  if (s) return s;
  return gicp_join_source(h);
}
}  // namespace ndtc

extern "C" {
// setInputTarget (which = 0) / setInputSource (1) from host memory: finite check on the host, upload, index
static ndt_status gicp_set_input_host(gicp_handle h, int which, const void* pts, size_t n, size_t stride_bytes) {
  return gicp_set_input(h, which, false, true,
                        [&](ndt_context* c, GicpInput& in) { return gicp_build_index(c, pts, n, stride_bytes, in.hint, in); });
}
ndt_status gicp_set_input_target(gicp_handle h, const void* pts, size_t n, size_t stride_bytes) { return gicp_set_input_host(h, 0, pts, n, stride_bytes); }
ndt_status gicp_set_input_source(gicp_handle h, const void* pts, size_t n, size_t stride_bytes) { return gicp_set_input_host(h, 1, pts, n, stride_bytes); }

// the same from a resident cloud: finite check on the device, the index built over the cloud where it lies
static ndt_status gicp_set_input_cloud(gicp_handle h, int which, ndt_cloud cl) {
  return gicp_set_input(h, which, true, cl && cl->c && cl->c->n != 0, [&](ndt_context* c, GicpInput& in) {
    ndt_status s = cloud_use_on(&h->tgt, cl->c.get());  // (the source's points are read on the main stream too)
    if (s) return s;
    std::vector<unsigned> bad;
    s = gicp_finite_check(h, {cl->c.get()}, bad);
    if (s) return s;
    if (bad[0]) return fail(NDT_ERR_INVALID, "GICP needs finite points (" + std::to_string(bad[0]) + " of the cloud's are not)");
    if (which == 1) {
      s = ensure_device(c);
      if (!s) s = cloud_use_on(c, cl->c.get());
      if (s) return s;
    }
    return gicp_index_cloud(c, cl->c, in.hint, in);
  });
}
ndt_status gicp_set_input_target_cloud(gicp_handle h, ndt_cloud c) { return gicp_set_input_cloud(h, 0, c); }
ndt_status gicp_set_input_source_cloud(gicp_handle h, ndt_cloud c) { return gicp_set_input_cloud(h, 1, c); }

// setTargetCovariances / setSourceCovariances (gicp_omp.h:165-168,186-189): caller-supplied covariances take the place of
// the k-NN ones until the cloud is set again.  cov: [n][9] row-major 3x3 (symmetric: the upper triangle is kept).
static ndt_status gicp_set_covariances(gicp_handle h, int which, const double* cov, size_t n) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  GicpInput& in = h->in[which];
  if (!in.set) return fail(NDT_ERR_NO_INPUT, "set the cloud before its covariances");
  if (in.vox) return fail(NDT_ERR_INVALID, "a grid target has its voxels' covariances: none can be set");
  if (!cov || n == 0) {  // an empty vector: computed again by the next align (:386,392)
    in.have_cov = in.user_cov = false;
    return NDT_OK;
  }
  if (n != in.n()) return fail(NDT_ERR_INVALID, "one covariance per point of the cloud is required");
  ndt_status s = ensure_device(&h->tgt);
  if (s) return s;
  std::vector<double> c6(n * 6);
  cov6_from_cov9(cov, n, c6.data());
  HIP_TRY(in.cov.reserve(n * 6));
  HIP_TRY(hipStreamSynchronize(h->tgt.stream));  // kernels of an earlier align may still read the old covariances
  HIP_TRY(hipMemcpy(in.cov.p, c6.data(), n * 6 * sizeof(double), hipMemcpyHostToDevice));
  in.have_cov = in.user_cov = true;
  h->step_ready = false;
  return NDT_OK;
}
ndt_status gicp_set_target_covariances(gicp_handle h, const double* cov, size_t n) { return gicp_set_covariances(h, 0, cov, n); }
ndt_status gicp_set_source_covariances(gicp_handle h, const double* cov, size_t n) { return gicp_set_covariances(h, 1, cov, n); }

ndt_status gicp_covariances(gicp_handle h, int which, double* cov, int* nn_idx, float* nn_d2) {
  if (!h || !cov || which < 0 || which > 1) return fail(NDT_ERR_INVALID, "bad arguments");
  GicpInput& in = h->in[which];
  if (!in.set) return fail(NDT_ERR_NO_INPUT, "cloud not set");
  if (in.vox) {  // a voxel target: D's covariances as the next registration would use them
    if (nn_idx || nn_d2) return fail(NDT_ERR_INVALID, "a grid target's covariances have no neighbour lists");
    const ndt_status sg = gicp_grid_ready(h);
    return sg ? sg : gicp_read_covariances(h, in, cov);
  }
  ndt_status s = ensure_device(&h->tgt);
  if (s) return s;
  // inspection: the k-NN covariances for the CURRENT k (caller-supplied ones are returned as they are; neighbours cannot
  // be asked for then)
  if (in.user_cov) {
    if (nn_idx || nn_d2) return fail(NDT_ERR_INVALID, "caller-supplied covariances have no neighbour lists");
  } else {
    in.have_cov = false;
  }
  const bool want_nn = nn_idx && nn_d2;
  s = gicp_cloud_covariances(h, in, which == 1, want_nn);
  if (s) return s;
  s = gicp_join_source(h);
  if (s) return s;
  if (want_nn) {
    const size_t nk = in.n() * static_cast<size_t>(h->prm.k_correspondences);
    HIP_TRY(hipMemcpyAsync(nn_idx, h->nn_idx.p, nk * sizeof(int), hipMemcpyDeviceToHost, h->tgt.stream));
    HIP_TRY(hipMemcpyAsync(nn_d2, h->nn_d2.p, nk * sizeof(float), hipMemcpyDeviceToHost, h->tgt.stream));
  }
  return gicp_read_covariances(h, in, cov);  // (waits for the main stream: the neighbour lists have arrived too)
}
}  // extern "C"
