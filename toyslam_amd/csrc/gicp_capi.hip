// gicp_capi.hip -- C-ABI glue of the GICP row (include/gicp_mi355.h).  It reuses the NDT units' device pool,
// cloud upload and K1 grid build (ndt_internal.hpp) -- the
// voxel index K1 produces over a cloud is the search structure of GICP's nearest-neighbour queries.
//
// One input of a registration is a GicpInput: a cloud's search index (which holds the cloud), its packed covariances and
// where they came from.  The handle's own target and source are two of them (in[0], in[1]), the clouds a pairs call
// prepares are more of them, and a registration (gicp_register, gicp_prepare, GicpDevice) is a function of two of them --
// its parameters, streams and scratch are the handle's.  The two ndt_contexts a gicp_context owns are tools, not state:
// `tgt` is the main stream (all GICP kernels run on it) and the builder of every index but the handle's source's, `src`
// builds that one and runs its k-NN covariances next to the target's.  Neither keeps a cloud or a grid between calls.
#include "ndt_internal.hpp"

#include "gicp_lockstep.hpp"

struct LeafHint {  // consecutive clouds have about the same density: the index leaf the previous one ended up with, and its size
  float leaf = 0.f;
  size_t n = 0;
};

struct GicpInput {
  std::shared_ptr<DeviceGrid> grid;  // the search index; grid->target is the cloud
  DevBuf<double> cov;                // [n][6]
  bool have_cov = false;
  bool user_cov = false;  // supplied through gicp_set_*_covariances
  // the setters' side: the input has been set (a pairs call's record: the cloud was named), the leaf chain of this slot
  bool set = false;
  LeafHint hint;
  const DeviceCloud& cloud() const { return *grid->target; }
  size_t n() const { return grid->target->n; }
};

struct gicp_context {
  ndt_context tgt, src;  // first: every device buffer below goes back to the pool before these two destroy their streams
  gicp::Params prm;
  GicpInput in[2];                  // target, source
  DevBuf<float4> output;            // the source moved by the guess
  DevBuf<int> corr;
  DevBuf<float> maha;
  DevBuf<double> partials;
  DevBuf<unsigned> counter;
  DevBuf<float4> out_cloud;
  DevBuf<int> nn_idx;
  DevBuf<float> nn_d2;
  double* host_pub = nullptr;  // pinned tagged publication row
  void* out_pinned = nullptr;  // page-locked staging of the aligned cloud
  // persistent objective server (one launch per BFGS run): two alternating command mailboxes in host-visible device
  // memory, shard counters, the pinned part rows
  void* srv_mbs = nullptr;
  int srv_flip = 0;
  bool srv_tried = false;
  double* srv_rows = nullptr;
  DevBuf<unsigned> srv_counter;
  int srv_blocks = 0;
  bool src_cov_pending = false;
  hipEvent_t ev_src = nullptr;  // the source's covariance pass (on src's stream) -> the main stream
  size_t out_pinned_bytes = 0;
  unsigned long long seq = 0;
  bool step_ready = false;
  // gicp_align_pairs_clouds: what the last successful call prepared for every cloud (`set`: a pair named it), and what it
  // launched (gicp_pairs_covariances, gicp_diag_pairs)
  std::vector<GicpInput> pairs_prepared;
  bool pairs_valid = false;
  size_t pairs_index_builds = 0, pairs_knn_launches = 0, pairs_knn_blocks = 0;
  double pairs_prepare_ms = 0, pairs_register_ms = 0;  // host wall clock of the call's two halves (tools/time_gicp_pairs.py)
  DevBuf<unsigned char> member_table;  // the member tables of the finite check and of k_knn_covariances_multi
  // the lock-step (gicp_align_pairs_lockstep, gicp_align_guesses): the slots' tagged rows and the tables' staging in pinned
  // host memory, the tables, partial rows and ticket counters on the device (grow-only, sized by the window); what the
  // last successful call did (gicp_diag_lockstep)
  void* ls_host = nullptr;
  int ls_slots = 0;
  DevBuf<unsigned char> ls_tables;
  DevBuf<double> ls_partials;
  DevBuf<unsigned> ls_counters;
  bool ls_valid = false;
  gicp::LockstepStats ls_stats;
  DevBuf<unsigned> finite_counts;
  // the last gicp_align's result
  gicp::Result result;
  float final_T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // column-major

  ndt_context* builder(int which) { return which == 0 ? &tgt : &src; }

  // Nothing may still run when the buffers go: both streams are waited for.  The inputs, the pairs records and the scratch
  // are members, released after this body in reverse order of declaration -- into the main stream's pool, which tgt's
  // destructor then empties -- so nothing is listed here but what is not a DevBuf.
  ~gicp_context() {
    for (ndt_context* c : {&src, &tgt})
      if (c->device_ready) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        tls_pool_stream = c->stream;
      }
    if (host_pub) (void)hipHostFree(host_pub);
    if (out_pinned) (void)hipHostFree(out_pinned);
    if (ev_src) (void)hipEventDestroy(ev_src);
    if (srv_mbs) (void)hipFree(srv_mbs);
    if (srv_rows) (void)hipHostFree(srv_rows);
    if (ls_host) (void)hipHostFree(ls_host);
  }
};

namespace {

// what the index leaf size aims for (points per occupied cell; NDT_GICP_PPC overrides it for tuning runs): with the
// margin bound most queries finish inside their own cell, so fuller cells cost little and far queries need fewer shells
static const double kGicpPointsPerCell = std::getenv("NDT_GICP_PPC") ? std::atof(std::getenv("NDT_GICP_PPC")) : 12.0;
// development switch: caps the grids of all four GICP kernels (0 = each kernel's own limit), so that their grid-strided
// regime is reached at a few thousand points -- as NDT_K2_MAX_BLOCKS does for the NDT kernels
static const int kGicpMaxBlocks = std::getenv("NDT_GICP_MAX_BLOCKS") ? std::max(0, std::atoi(std::getenv("NDT_GICP_MAX_BLOCKS"))) : 0;
// development switch: the blocks one k_knn_covariances_multi launch carries (default gicp::kKnnMultiMaxBlocks), so that the
// split of a pairs call's covariance pass into several launches is reached with a few thousand points
static const int kGicpMultiMaxBlocks = std::getenv("NDT_GICP_MULTI_MAX_BLOCKS") ? std::max(1, std::atoi(std::getenv("NDT_GICP_MULTI_MAX_BLOCKS")))
                                                                                : gicp::kKnnMultiMaxBlocks;
constexpr long long kGicpMaxCells = 1ll << 26;       // dense cell table budget (256 MB of int)

// The voxel index of `cloud` (on the device, every point finite -- so the box the cloud carries over its finite points is
// the box of all of them) into in.grid: leaf size from the cloud's own density (volume guess first, then corrected once
// from the measured points per occupied cell -- scans are surfaces, so occupancy grows with the square of the leaf).
// Built with `c`: its stream, its scratch, its pool (the caller has made `c` current); `c` holds neither the cloud nor the grid.
ndt_status gicp_index_cloud(ndt_context* c, const std::shared_ptr<DeviceCloud>& cloud, LeafHint& hint, GicpInput& in) {
  in.grid.reset();  // (before the new one is allocated: an input never holds two)
  std::shared_ptr<DeviceGrid> grid;
  const size_t n = cloud->n;
  ndt_status s = NDT_OK;
  double ext[3], vol = 1.0;
  for (int k = 0; k < 3; k++) {
    ext[k] = std::max(static_cast<double>(cloud->bb_max[1][k]) - static_cast<double>(cloud->bb_min[1][k]), 1e-3);
    vol *= ext[k];
  }
  auto clamp_leaf = [&](double leaf) {
    leaf = std::max(leaf, 1e-4);
    for (int it = 0; it < 64; it++) {  // keep the dense cell table within budget
      const double cells = (ext[0] / leaf + 2) * (ext[1] / leaf + 2) * (ext[2] / leaf + 2);
      if (cells <= static_cast<double>(kGicpMaxCells)) break;
      leaf *= 1.26;
    }
    return static_cast<float>(leaf);
  };
  float leaf = clamp_leaf(std::cbrt(vol * kGicpPointsPerCell / static_cast<double>(n)));
  // start from the leaf the previous cloud of about this size ended up with (usually right at once; the search results do
  // not depend on the leaf, only the time does)
  if (hint.leaf > 0 && n >= hint.n - hint.n / 4 && n <= hint.n + hint.n / 4) leaf = clamp_leaf(hint.leaf);
  for (int pass = 0; pass < 4; pass++) {
    s = build_grid(c, cloud, GridSpec{leaf, 1, c->eig_ratio, 0, true, true}, grid);  // cells and their point lists only
    if (s) return s;
    s = grid_counts(c, grid.get());
    if (s) return s;
    const double per_cell = static_cast<double>(n) / static_cast<double>(std::max<size_t>(grid->n_leaves, 1));
    if (per_cell <= 2.0 * kGicpPointsPerCell && (per_cell >= 0.4 * kGicpPointsPerCell || grid->n_leaves <= 8)) break;
    // too coarse (dense surfaces) or too fine (flat / thin clouds, where the volume guess means little)
    const float next = clamp_leaf(static_cast<double>(leaf) * std::sqrt(kGicpPointsPerCell / per_cell));
    if (next < 0.9f * leaf || next > 1.1f * leaf) leaf = next;
    else break;
  }
  if (std::getenv("NDT_GICP_DEBUG"))
    std::fprintf(stderr, "[gicp index] n=%zu leaf=%.4f cells=%lld (%d x %d x %d) occupied=%zu\n", n, static_cast<double>(leaf),
                 grid->geom.n_cells, grid->geom.div_b[0], grid->geom.div_b[1], grid->geom.div_b[2], grid->n_leaves);
  hint.leaf = leaf;
  hint.n = n;
  s = ensure_cell2leaf(c, grid.get());
  if (!s) in.grid = std::move(grid);
  return s;
}

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

// An asynchronous copy from pageable host memory is queued on `s`: unless the success path has synchronised already
// (done), leaving the scope waits for the stream, so an error return between the copy and that synchronise cannot free
// the host memory under a copy still queued.
struct StreamDrain {
  hipStream_t s;
  bool done = false;
  ~StreamDrain() { if (!done) (void)hipStreamSynchronize(s); }
};

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

gicp::PointIndex gicp_index_of(const GicpInput& in) {
  gicp::PointIndex ix;
  fill_point_index(in.grid.get(), ix);
  return ix;
}

void rowmajor_from_colmajor(const float* cm, float* rm) {
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) rm[r * 4 + c] = cm ? cm[c * 4 + r] : (r == c ? 1.0f : 0.0f);
}
void colmajor_from_rowmajor(const float* rm, float* cm) {
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) cm[c * 4 + r] = rm[r * 4 + c];
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
  h->step_ready = false;
  return in;
}

ndt_status gicp_inputs_set(const gicp_context* h) {
  if (!h->in[0].set) return fail(NDT_ERR_NO_INPUT, "no target cloud set");
  if (!h->in[1].set) return fail(NDT_ERR_NO_INPUT, "no source cloud set");
  return NDT_OK;
}

// the main stream current (device, this thread's pool stream) and the scratch every evaluation needs
ndt_status gicp_scratch(gicp_context* h) {
  ndt_status s = ensure_device(&h->tgt);
  if (s) return s;
  if (!h->host_pub) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->host_pub), ndt::kPublishSlots * sizeof(double), hipHostMallocDefault));
    std::memset(h->host_pub, 0, ndt::kPublishSlots * sizeof(double));
  }
  if (!h->counter.p) {
    HIP_TRY(h->counter.reserve(1));
    HIP_TRY(hipMemsetAsync(h->counter.p, 0, sizeof(unsigned), h->tgt.stream));
  }
  return NDT_OK;
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

// the covariances of `in` to the host as [n][9], behind everything queued on the main stream, which is waited for
ndt_status gicp_read_covariances(gicp_context* h, const GicpInput& in, double* cov9) {
  const size_t n = in.n();
  std::vector<double> c6(n * 6);
  HIP_TRY(hipMemcpyAsync(c6.data(), in.cov.p, n * 6 * sizeof(double), hipMemcpyDeviceToHost, h->tgt.stream));
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

ndt_status gicp_prepare(gicp_context* h, GicpInput& tgt, GicpInput& src, const float* guess_cm, float guess_rm[16]) {
  ndt_status s = gicp_prepare_covariances(h, tgt, src);
  if (s) return s;
  const size_t n = src.n();
  rowmajor_from_colmajor(guess_cm, guess_rm);
  HIP_TRY(h->output.reserve(n));
  HIP_TRY(h->corr.reserve(n));
  HIP_TRY(h->maha.reserve(n * 9));
  HIP_TRY(h->partials.reserve(static_cast<size_t>(gicp::kFunctorMaxBlocks) * ndt::kEvalStride));
  // pcl::transformPointCloud(output, output, guess), :403
  HIP_TRY(ndt::launch_transform(src.cloud().pts.p, static_cast<int>(n), guess_rm, h->output.p, h->tgt.stream));
  return NDT_OK;
}

// The device side of one registration of `src` onto `tgt`, with h's parameters, main stream and scratch.
struct GicpDevice : gicp::Backend {
  gicp_context* h;
  const GicpInput& tgt;
  const GicpInput& src;
  std::string error;
  // The line search evaluates operator() and then, if the step passes Fletcher's rho test, df at the very same
  // point (gicp_driver.cpp line_search): the operator() launch also accumulates df's sums, and the df request that
  // follows is answered from here without a launch.
  // (gicp::SumsPlan: the mapping the lock-step's members use too)
  gicp::SumsPlan plan{gicp::fuse_enabled()};
  int evals_served = 0;
  GicpDevice(gicp_context* ctx, const GicpInput& target, const GicpInput& source) : h(ctx), tgt(target), src(source) {}

  bool correspond(const float transformation[16], const double R[9]) override {
    gicp::Rot3d rot;
    for (int i = 0; i < 9; i++) rot.m[i] = R[i];
    plan.invalidate();
    server_stop();  // the correspondences change: the next BFGS run gets a fresh server behind this kernel
    const double thr = h->prm.corr_dist_threshold * h->prm.corr_dist_threshold;  // :401
    const int n = static_cast<int>(src.n());
    const hipError_t e = gicp::launch_correspond(h->output.p, n, transformation, rot, gicp_index_of(tgt), src.cov.p, tgt.cov.p, thr,
                                                 gicp::correspond_blocks(n, kGicpMaxBlocks), h->corr.p, h->maha.p, h->tgt.stream);
    if (e != hipSuccess) {
      error = std::string("correspondence kernel: ") + hipGetErrorString(e);
      return false;
    }
    return true;
  }

  // ---- persistent objective server -------------------------------------------------------------------------
  void* mailbox() const { return static_cast<unsigned char*>(h->srv_mbs) + static_cast<size_t>(h->srv_flip) * ndt::server_mailbox_bytes(); }
  bool server_available() {
    if (h->srv_tried) return h->srv_mbs != nullptr;
    h->srv_tried = true;
    const char* v = std::getenv("NDT_GICP_SERVER");
    if (v && std::atoi(v) == 0) return false;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->tgt.device) != hipSuccess || prop.isLargeBar == 0) return false;  // the direct mailbox needs the BAR
    const size_t mb = ndt::server_mailbox_bytes();
    if (hipExtMallocWithFlags(&h->srv_mbs, 2 * mb, hipDeviceMallocFinegrained) != hipSuccess) {
      h->srv_mbs = nullptr;
      (void)hipGetLastError();
      return false;
    }
    if (hipMemset(h->srv_mbs, 0, 2 * mb) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&h->srv_rows), gicp::kGicpServerParts * ndt::kPublishSlots * sizeof(double), hipHostMallocDefault) != hipSuccess ||
        h->srv_counter.reserve(32 * gicp::kGicpServerParts) != hipSuccess) {
      (void)hipFree(h->srv_mbs);
      h->srv_mbs = nullptr;
      (void)hipGetLastError();
      return false;
    }
    std::memset(h->srv_rows, 0, gicp::kGicpServerParts * ndt::kPublishSlots * sizeof(double));
    return true;
  }
  bool server_start() {
    server_mark(&h->tgt, true);  // this device's turn among the persistent kernels of the process
    h->srv_flip ^= 1;
    ndt::server_reset_mailbox(mailbox());
    const int n = static_cast<int>(src.n());
    h->srv_blocks = gicp::server_blocks(n, kGicpMaxBlocks);
    hipError_t e = hipMemsetAsync(h->srv_counter.p, 0, 32 * gicp::kGicpServerParts * sizeof(unsigned), h->tgt.stream);
    if (e == hipSuccess) e = h->partials.reserve(static_cast<size_t>(std::max(h->srv_blocks, gicp::kFunctorMaxBlocks)) * ndt::kEvalStride);
    if (e == hipSuccess)
      e = gicp::launch_server(h->output.p, n, tgt.cloud().pts.p, h->corr.p, h->maha.p, mailbox(), h->srv_blocks, h->partials.p,
                              h->srv_counter.p, h->srv_rows, h->seq + 1, 2000000ull /* 20 ms */, h->tgt.stream);
    if (e != hipSuccess) {
      server_mark(&h->tgt, false);
      error = std::string("objective server: ") + hipGetErrorString(e);
      return false;
    }
    return true;
  }
  void server_stop() {  // the last command: everything queued later on the stream runs behind the exiting kernel
    if (!h->tgt.server_running) return;
    ndt::server_post(mailbox(), ++h->seq, ndt::kServerCmdExit, nullptr, nullptr);
    server_mark(&h->tgt, false);
  }
  // one evaluation through the server; false = it has left (idle time-out): the caller uses the launch path
  bool server_sums(int launch_mode, const float T[16], double row[ndt::kEvalStride]) {
    const unsigned long long seq = ++h->seq;
    ndt::server_post(mailbox(), seq, launch_mode, T, nullptr);
    const int n_parts = std::min(gicp::kGicpServerParts, h->srv_blocks);
    unsigned arrived = 0;
    const unsigned all = (1u << n_parts) - 1u;
    unsigned spins = 0;
    for (;;) {
      for (int p = 0; p < n_parts; p++)
        if (!(arrived & (1u << p)) && pub_ready(h->srv_rows + static_cast<size_t>(p) * ndt::kPublishSlots, seq)) arrived |= 1u << p;
      if (arrived == all) break;
      __builtin_ia32_pause();
      if ((++spins & 0x3FFF) == 0 && (ndt::server_dead_word(mailbox()) != 0 || hipStreamQuery(h->tgt.stream) != hipErrorNotReady)) {
        server_mark(&h->tgt, false);
        (void)hipStreamSynchronize(h->tgt.stream);
        return false;
      }
    }
    double part[ndt::kEvalStride];
    for (int k = 0; k < ndt::kEvalStride; k++) row[k] = 0.0;
    for (int p = 0; p < gicp::kGicpServerParts; p++) {  // second stage of k_functor's fixed-order sum
      if (p < n_parts) pub_gather(h->srv_rows + static_cast<size_t>(p) * ndt::kPublishSlots, part);
      for (int k = 0; k < ndt::kEvalStride; k++) row[k] += (p < n_parts) ? part[k] : 0.0;
    }
    return true;
  }

  bool sums(int mode, const float T[16], gicp::FunctorSums& out) override {
    if (plan.answered(mode, T, out)) return true;
    const int n = static_cast<int>(src.n());
    const int launch_mode = plan.launch_mode(mode);
    double row[ndt::kEvalStride];
    bool have_row = false;
    if (server_available()) {
      if (!h->tgt.server_running && !server_start()) return false;
      // liveness test hook: a host that goes quiet in the middle of a BFGS run (the server's patience is 20 ms)
      static const int stall_ms = std::getenv("NDT_GICP_TEST_STALL_MS") ? std::atoi(std::getenv("NDT_GICP_TEST_STALL_MS")) : 0;
      if (stall_ms > 0 && ++evals_served == 5) std::this_thread::sleep_for(std::chrono::milliseconds(stall_ms));
      have_row = server_sums(launch_mode, T, row);
    }
    if (!have_row) {
      const unsigned long long seq = ++h->seq;
      const hipError_t e = gicp::launch_functor(launch_mode, h->output.p, n, tgt.cloud().pts.p, h->corr.p, h->maha.p, T,
                                                gicp::functor_blocks(n, kGicpMaxBlocks), h->partials.p, h->counter.p, h->host_pub, seq, h->tgt.stream);
      if (e != hipSuccess) {
        error = std::string("functor kernel: ") + hipGetErrorString(e);
        return false;
      }
      // the row arrives as 64 self-validating words; poll, and look at the stream now and then so that a
      // failed launch cannot hang the caller
      for (unsigned long long spins = 1; !pub_ready(h->host_pub, seq); spins++) {
        if ((spins & 0xfffff) == 0) {
          const hipError_t q = hipStreamQuery(h->tgt.stream);
          if (q == hipSuccess) {
            if (pub_ready(h->host_pub, seq)) break;
            error = "functor kernel finished without publishing its result";
            return false;
          }
          if (q != hipErrorNotReady) {
            error = std::string("functor kernel: ") + hipGetErrorString(q);
            return false;
          }
        }
      }
      pub_gather(h->host_pub, row);
    }
    gicp::sums_from_row(row, out);
    plan.keep(launch_mode, T, out);
    return true;
  }
  ~GicpDevice() override { server_stop(); }
};

// One registration of `src` onto `tgt` from the guess (column-major, NULL = identity): what gicp_align and every pair of
// gicp_align_pairs_clouds run.  *status != NDT_OK: the result means nothing.
gicp::Result gicp_register(gicp_context* h, GicpInput& tgt, GicpInput& src, const float* guess_cm, ndt_status* status) {
  gicp::Result r{};
  float guess_rm[16];
  *status = gicp_prepare(h, tgt, src, guess_cm, guess_rm);
  if (*status) return r;
  h->step_ready = false;  // the scratch of gicp_step_correspond is overwritten from here on
  GicpDevice dev(h, tgt, src);
  r = gicp::run(h->prm, guess_rm, dev);
  dev.server_stop();  // before anything else is queued on the stream or waited for: the server would sit out its patience
  if (r.backend_failed || !dev.error.empty()) *status = fail(NDT_ERR_HIP, dev.error.empty() ? "device failure" : dev.error);
  return r;
}

// ---- the lock-step: the device side of gicp::run_lockstep ----------------------------------------------------------
// One registration of the lock-step: two inputs and a guess.
struct LockstepJob {
  const GicpInput* tgt;
  const GicpInput* src;
  float guess_rm[16];
};

size_t ls_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

// The slots' memory for a window of `slots` members (grow-only; the counters are zeroed at every call: a failed step may
// have left tickets behind).  Pinned: [slots] tagged rows, then the staging of the three tables; device: the three tables.
struct LockstepLayout {
  size_t rows = 0, members = 0, corr = 0, functor = 0, host_bytes = 0, dev_members = 0, dev_corr = 0, dev_functor = 0, dev_bytes = 0;
  explicit LockstepLayout(size_t w) {
    members = rows + ls_align(w * ndt::kPublishSlots * sizeof(double));
    corr = members + ls_align(w * sizeof(gicp::LockstepMember));
    functor = corr + ls_align(w * sizeof(gicp::LockstepCorrespond));
    host_bytes = functor + ls_align(w * sizeof(gicp::LockstepFunctor));
    dev_corr = dev_members + ls_align(w * sizeof(gicp::LockstepMember));
    dev_functor = dev_corr + ls_align(w * sizeof(gicp::LockstepCorrespond));
    dev_bytes = dev_functor + ls_align(w * sizeof(gicp::LockstepFunctor));
  }
};

ndt_status gicp_lockstep_scratch(gicp_context* h, int slots) {
  const int rows_per_slot = gicp::server_blocks(1 << 30, kGicpMaxBlocks);
  if (h->ls_slots < slots) {
    HIP_TRY(hipStreamSynchronize(h->tgt.stream));
    if (h->ls_host) (void)hipHostFree(h->ls_host);
    h->ls_host = nullptr;
    h->ls_slots = 0;
    const LockstepLayout L(static_cast<size_t>(slots));
    HIP_TRY(hipHostMalloc(&h->ls_host, L.host_bytes, hipHostMallocDefault));
    std::memset(h->ls_host, 0, L.host_bytes);
    HIP_TRY(h->ls_tables.reserve(L.dev_bytes));
    HIP_TRY(h->ls_partials.reserve(static_cast<size_t>(slots) * rows_per_slot * ndt::kEvalStride));
    HIP_TRY(h->ls_counters.reserve(static_cast<size_t>(slots)));
    h->ls_slots = slots;
  }
  HIP_TRY(hipMemsetAsync(h->ls_counters.p, 0, static_cast<size_t>(h->ls_slots) * sizeof(unsigned), h->tgt.stream));
  return NDT_OK;
}

// gicp::StepExecutor on the device: per step one table upload, one k_correspond_multi launch for the members that asked for
// correspondences, one k_functor_multi launch for all of them, and the poll of their tagged rows.  Called by the
// coordinator (the API's calling thread) only.  A member in flight owns a slot: a row of the tables, of the partial rows,
// a counter and a pinned row; and its own scratch from the main stream's pool -- the guess-moved source, corr, maha9 --
// which goes back when the member ends (stream order makes the next user safe).
struct LockstepDevice : gicp::StepExecutor {
  gicp_context* h;
  const std::vector<LockstepJob>& jobs;
  LockstepLayout L;
  struct Scratch {
    DevBuf<float4> output;
    DevBuf<int> corr;
    DevBuf<float> maha;
  };
  std::vector<std::unique_ptr<Scratch>> scratch;  // per slot
  std::vector<int> slot_of;                       // per member, -1 = not in flight
  std::vector<int> free_slots;
  int rows_per_slot;
  std::string error;

  LockstepDevice(gicp_context* ctx, const std::vector<LockstepJob>& j)
      : h(ctx), jobs(j), L(static_cast<size_t>(ctx->ls_slots)), scratch(static_cast<size_t>(ctx->ls_slots)), slot_of(j.size(), -1),
        rows_per_slot(gicp::server_blocks(1 << 30, kGicpMaxBlocks)) {
    for (int s = h->ls_slots - 1; s >= 0; s--) free_slots.push_back(s);
  }
  template <class T>
  T* host_at(size_t off) const { return reinterpret_cast<T*>(static_cast<unsigned char*>(h->ls_host) + off); }
  template <class T>
  T* dev_at(size_t off) const { return reinterpret_cast<T*>(h->ls_tables.p + off); }
  double* row_of(int slot) const { return host_at<double>(L.rows) + static_cast<size_t>(slot) * ndt::kPublishSlots; }
  bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    error = std::string(what) + ": " + hipGetErrorString(e);
    return false;
  }

  bool start(int member) override {
    if (free_slots.empty()) {
      error = "lock-step: no free slot";
      return false;
    }
    const LockstepJob& job = jobs[static_cast<size_t>(member)];
    const size_t n = job.src->n();
    std::unique_ptr<Scratch> sc(new Scratch());
    if (!hip_ok(sc->output.reserve(n), "lock-step scratch") || !hip_ok(sc->corr.reserve(n), "lock-step scratch") ||
        !hip_ok(sc->maha.reserve(n * 9), "lock-step scratch"))
      return false;
    hipStream_t st = h->tgt.stream;
    // pcl::transformPointCloud(output, output, guess), :403
    if (!hip_ok(ndt::launch_transform(job.src->cloud().pts.p, static_cast<int>(n), job.guess_rm, sc->output.p, st), "transform kernel")) return false;
    const int slot = free_slots.back();
    gicp::LockstepMember& m = host_at<gicp::LockstepMember>(L.members)[slot];
    m = gicp::LockstepMember();
    m.output = sc->output.p;
    m.tgt_pts = job.tgt->cloud().pts.p;
    m.cov_src6 = job.src->cov.p;
    m.cov_tgt6 = job.tgt->cov.p;
    m.corr = sc->corr.p;
    m.maha9 = sc->maha.p;
    m.partials = h->ls_partials.p + static_cast<size_t>(slot) * rows_per_slot * ndt::kEvalStride;
    m.counter = h->ls_counters.p + slot;
    m.out_row = row_of(slot);
    m.tgt = gicp_index_of(*job.tgt);
    m.n = static_cast<int>(n);
    // (the staging row is rewritten only when the slot has a new owner: its last owner's final step, queued behind this
    // copy's predecessors, has been waited for)
    if (!hip_ok(hipMemcpyAsync(dev_at<gicp::LockstepMember>(L.dev_members) + slot, &m, sizeof(m), hipMemcpyHostToDevice, st), "lock-step member table"))
      return false;
    free_slots.pop_back();
    scratch[static_cast<size_t>(slot)] = std::move(sc);
    slot_of[static_cast<size_t>(member)] = slot;
    return true;
  }

  void finish(int member) override {
    const int slot = slot_of[static_cast<size_t>(member)];
    if (slot < 0) return;
    scratch[static_cast<size_t>(slot)].reset();
    slot_of[static_cast<size_t>(member)] = -1;
    free_slots.push_back(slot);
  }

  bool step(const std::vector<gicp::StepRequest>& requests, std::vector<gicp::FunctorSums>& out) override {
    hipStream_t st = h->tgt.stream;
    gicp::LockstepCorrespond* ct = host_at<gicp::LockstepCorrespond>(L.corr);
    gicp::LockstepFunctor* ft = host_at<gicp::LockstepFunctor>(L.functor);
    int n_corr = 0, corr_blocks = 0, n_fun = 0, fun_blocks = 0;
    for (const gicp::StepRequest& r : requests) {
      const int slot = slot_of[static_cast<size_t>(r.member)];
      const int n = static_cast<int>(jobs[static_cast<size_t>(r.member)].src->n());
      if (r.correspond) {
        gicp::LockstepCorrespond& c = ct[n_corr++];
        for (int i = 0; i < 12; i++) c.T[i] = r.corr_T[i];
        for (int i = 0; i < 9; i++) c.R.m[i] = r.corr_R[i];
        c.slot = slot;
        c.first_block = corr_blocks;
        c.n_blocks = gicp::correspond_blocks(n, kGicpMaxBlocks);
        c.pad = 0;
        corr_blocks += c.n_blocks;
      }
      gicp::LockstepFunctor& f = ft[n_fun++];
      for (int i = 0; i < 12; i++) f.T[i] = r.T[i];
      f.slot = slot;
      f.mode = r.mode;
      f.first_block = fun_blocks;
      f.n_blocks = gicp::server_blocks(n, kGicpMaxBlocks);
      fun_blocks += f.n_blocks;
    }
    const unsigned long long seq = ++h->seq;
    // (the staging is free: the previous step's kernels, queued behind its copies, have published)
    if (n_corr) {
      if (!hip_ok(hipMemcpyAsync(dev_at<gicp::LockstepCorrespond>(L.dev_corr), ct, static_cast<size_t>(n_corr) * sizeof(*ct), hipMemcpyHostToDevice, st),
                  "lock-step step table"))
        return false;
      const double thr = h->prm.corr_dist_threshold * h->prm.corr_dist_threshold;  // :401
      if (!hip_ok(gicp::launch_correspond_multi(dev_at<gicp::LockstepMember>(L.dev_members), dev_at<gicp::LockstepCorrespond>(L.dev_corr), n_corr,
                                                corr_blocks, thr, st),
                  "correspondence kernel"))
        return false;
    }
    if (!hip_ok(hipMemcpyAsync(dev_at<gicp::LockstepFunctor>(L.dev_functor), ft, static_cast<size_t>(n_fun) * sizeof(*ft), hipMemcpyHostToDevice, st),
                "lock-step step table") ||
        !hip_ok(gicp::launch_functor_multi(dev_at<gicp::LockstepMember>(L.dev_members), dev_at<gicp::LockstepFunctor>(L.dev_functor), n_fun, fun_blocks,
                                           seq, st),
                "functor kernel"))
      return false;
    // every member's row arrives as 64 self-validating words; poll them as GicpDevice::sums polls its one, and look at the
    // stream now and then so that a failed launch cannot hang the caller
    int arrived = 0;
    std::vector<char> have(static_cast<size_t>(n_fun), 0);
    for (unsigned long long spins = 1; arrived < n_fun; spins++) {
      for (int i = 0; i < n_fun; i++)
        if (!have[static_cast<size_t>(i)] && pub_ready(row_of(ft[i].slot), seq)) {
          have[static_cast<size_t>(i)] = 1;
          arrived++;
        }
      if (arrived < n_fun && (spins & 0xffff) == 0) {
        const hipError_t q = hipStreamQuery(st);
        if (q == hipSuccess) {
          bool all = true;
          for (int i = 0; i < n_fun; i++) all = all && pub_ready(row_of(ft[i].slot), seq);
          if (all) break;
          error = "functor kernel finished without publishing its result";
          return false;
        }
        if (q != hipErrorNotReady) return hip_ok(q, "functor kernel");
      }
    }
    double row[ndt::kEvalStride];
    for (int i = 0; i < n_fun; i++) {
      pub_gather(row_of(ft[i].slot), row);
      gicp::sums_from_row(row, out[static_cast<size_t>(i)]);
    }
    return true;
  }
};

// The registrations of `jobs` advanced together, with h's parameters.  results[j] is gicp_register's for job j.
ndt_status gicp_register_lockstep(gicp_context* h, const std::vector<LockstepJob>& jobs, std::vector<gicp::Result>& results,
                                  gicp::LockstepStats& stats) {
  const int window = std::min<int>(gicp::lockstep_window(), static_cast<int>(std::max<size_t>(jobs.size(), 1)));
  ndt_status s = gicp_scratch(h);
  if (!s) s = gicp_lockstep_scratch(h, window);
  if (s) return s;
  std::vector<gicp::LockstepInput> in(jobs.size());
  for (size_t j = 0; j < jobs.size(); j++) {
    in[j].prm = h->prm;
    std::memcpy(in[j].guess, jobs[j].guess_rm, sizeof(in[j].guess));
  }
  LockstepDevice dev(h, jobs);
  const bool ok = gicp::run_lockstep(in, window, gicp::fuse_enabled(), dev, results, stats);
  if (!ok) {
    (void)hipStreamSynchronize(h->tgt.stream);  // before the members' scratch goes back to the pool
    return fail(NDT_ERR_HIP, dev.error.empty() ? "device failure" : dev.error);
  }
  return NDT_OK;
}

}  // namespace

extern "C" {

ndt_status gicp_create(int device, gicp_handle* out) {
  if (!out || device < 0) return fail(NDT_ERR_INVALID, "bad arguments");
  gicp_context* h = new gicp_context();
  h->tgt.device = device;
  h->src.device = device;
  *out = h;
  return NDT_OK;
}

void gicp_destroy(gicp_handle h) { delete h; }

ndt_status gicp_set_correspondence_randomness(gicp_handle h, int k) {
  if (!h || k < 1 || k > gicp::kMaxK) return fail(NDT_ERR_INVALID, "k_correspondences must be in [1, 64]");
  // (covariances already computed stay, as in the reference: computeTransformation only computes them while they are
  // empty, gicp_omp_impl.hpp:386-397, and only setInputSource / setInputTarget reset them)
  h->prm.k_correspondences = k;
  return NDT_OK;
}
ndt_status gicp_set_rotation_epsilon(gicp_handle h, double eps) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  h->prm.rotation_epsilon = eps;
  return NDT_OK;
}
ndt_status gicp_set_maximum_optimizer_iterations(gicp_handle h, int n) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  h->prm.max_inner_iterations = n;
  return NDT_OK;
}
ndt_status gicp_set_transformation_epsilon(gicp_handle h, double eps) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  h->prm.transformation_epsilon = eps;
  return NDT_OK;
}
ndt_status gicp_set_maximum_iterations(gicp_handle h, int n) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  h->prm.max_iterations = n;
  return NDT_OK;
}
ndt_status gicp_set_max_correspondence_distance(gicp_handle h, double d) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  h->prm.corr_dist_threshold = d;
  return NDT_OK;
}

// setInputTarget (which = 0) / setInputSource (1) from host memory
static ndt_status gicp_set_input(gicp_handle h, int which, const void* pts, size_t n, size_t stride_bytes) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  GicpInput& in = gicp_unset(h, which);
  if (h->tgt.device_ready) {  // kernels of an earlier align may still read the old index
    HIP_TRY(hipSetDevice(h->tgt.device));
    HIP_TRY(hipStreamSynchronize(h->tgt.stream));
  }
  ndt_context* c = h->builder(which);
  const ndt_status s = gicp_build_index(c, pts, n, stride_bytes, in.hint, in);
  if (s) return s;
  if (which == 1) HIP_TRY(hipStreamSynchronize(c->stream));  // the index is read from the main stream from here on
  in.set = true;
  return NDT_OK;
}
ndt_status gicp_set_input_target(gicp_handle h, const void* pts, size_t n, size_t stride_bytes) { return gicp_set_input(h, 0, pts, n, stride_bytes); }
ndt_status gicp_set_input_source(gicp_handle h, const void* pts, size_t n, size_t stride_bytes) { return gicp_set_input(h, 1, pts, n, stride_bytes); }

// the same from a resident cloud: finite check on the device, the index built over the cloud where it lies
static ndt_status gicp_set_input_cloud(gicp_handle h, int which, ndt_cloud cl) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  GicpInput& in = gicp_unset(h, which);
  if (!cl || !cl->c || cl->c->n == 0) return fail(NDT_ERR_INVALID, "invalid or empty point cloud dataset given");
  ndt_status s = ensure_device(&h->tgt);
  if (s) return s;
  HIP_TRY(hipStreamSynchronize(h->tgt.stream));  // kernels of an earlier align may still read the old index
  s = cloud_use_on(&h->tgt, cl->c.get());  // (the source's points are read on the main stream too)
  if (s) return s;
  std::vector<unsigned> bad;
  s = gicp_finite_check(h, {cl->c.get()}, bad);
  if (s) return s;
  if (bad[0]) return fail(NDT_ERR_INVALID, "GICP needs finite points (" + std::to_string(bad[0]) + " of the cloud's are not)");
  ndt_context* c = h->builder(which);
  if (which == 1) {
    s = ensure_device(c);
    if (!s) s = cloud_use_on(c, cl->c.get());
    if (s) return s;
  }
  s = gicp_index_cloud(c, cl->c, in.hint, in);
  if (s) return s;
  if (which == 1) HIP_TRY(hipStreamSynchronize(c->stream));  // the index is read from the main stream from here on
  in.set = true;
  return NDT_OK;
}
ndt_status gicp_set_input_target_cloud(gicp_handle h, ndt_cloud c) { return gicp_set_input_cloud(h, 0, c); }
ndt_status gicp_set_input_source_cloud(gicp_handle h, ndt_cloud c) { return gicp_set_input_cloud(h, 1, c); }

// drops what the last pairs call kept (the buffers go back to the main stream's pool)
static void gicp_pairs_drop(gicp_handle h) {
  h->pairs_valid = false;
  h->pairs_index_builds = h->pairs_knn_launches = h->pairs_knn_blocks = 0;
  h->pairs_prepare_ms = h->pairs_register_ms = 0;
  if (h->pairs_prepared.empty()) return;
  if (h->tgt.device_ready) (void)ensure_device(&h->tgt);
  h->pairs_prepared.clear();
}

// What both pairs calls do before the first registration: the argument checks, the named clouds made readable on the main
// stream, the finite check of all of them in one launch, one index per named cloud (a leaf chain of the call's own) and
// the covariances of all of them from one k_knn_covariances_multi launch (a further launch per kGicpMultiMaxBlocks),
// waited for.  empty: n_pairs == 0, nothing was needed.
struct PairsPrep {
  std::vector<GicpInput> prep;  // one record per cloud; set: a pair named it
  size_t index_builds = 0, knn_launches = 0, knn_blocks = 0;
  std::chrono::steady_clock::time_point t_begin, t_prepared;
  bool empty = false;
};

static ndt_status gicp_pairs_prepare(gicp_handle h, const ndt_cloud* clouds, size_t n_clouds, const int* pairs, size_t n_pairs, PairsPrep& out) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  gicp_pairs_drop(h);
  if (n_clouds && !clouds) return fail(NDT_ERR_INVALID, "null clouds");
  if (n_pairs && !pairs) return fail(NDT_ERR_INVALID, "null pairs");
  if (n_pairs > 65535) return fail(NDT_ERR_INVALID, "at most 65535 pairs per call");
  for (size_t c = 0; c < n_clouds; c++)
    if (!clouds[c] || !clouds[c]->c) return fail(NDT_ERR_INVALID, "null cloud (entry " + std::to_string(c) + ")");
  for (size_t i = 0; i < 2 * n_pairs; i++)
    if (pairs[i] < 0 || static_cast<size_t>(pairs[i]) >= n_clouds) return fail(NDT_ERR_INVALID, "pair names a cloud that does not exist");
  const int k = h->prm.k_correspondences;
  std::vector<int> named;  // in order of first use
  {
    std::vector<char> seen(n_clouds, 0);
    for (size_t i = 0; i < 2 * n_pairs; i++)
      if (!seen[pairs[i]]) {
        seen[pairs[i]] = 1;
        named.push_back(pairs[i]);
      }
  }
  for (int c : named)
    if (clouds[c]->c->n < static_cast<size_t>(k))  // gicp_omp_impl.hpp:53-57
      return fail(NDT_ERR_INVALID, "number of points in cloud " + std::to_string(c) + " (" + std::to_string(clouds[c]->c->n) +
                                       ") is less than k_correspondences_ (" + std::to_string(k) + ")");
  if (n_pairs == 0) {
    h->pairs_valid = true;
    out.empty = true;
    return NDT_OK;
  }
  ndt_status s = ensure_device(&h->tgt);
  if (s) return s;
  hipStream_t st = h->tgt.stream;
  HIP_TRY(hipStreamSynchronize(st));
  out.t_begin = std::chrono::steady_clock::now();
  // ---- every named cloud: stream order, then the finite check of all of them in one launch
  std::vector<const DeviceCloud*> nc;
  for (int c : named) {
    s = cloud_use_on(&h->tgt, clouds[c]->c.get());
    if (s) return s;
    nc.push_back(clouds[c]->c.get());
  }
  std::vector<unsigned> bad;
  s = gicp_finite_check(h, nc, bad);
  if (s) return s;
  for (size_t j = 0; j < named.size(); j++)
    if (bad[j]) return fail(NDT_ERR_INVALID, "GICP needs finite points (" + std::to_string(bad[j]) + " of cloud " + std::to_string(named[j]) + " are not)");

  // ---- one record per named cloud: its index, the leaf of the previous one as the hint for the next (a chain of this
  // call's own; the builds are the handle's own path, one after the other, on the main stream)
  std::vector<GicpInput>& prep = out.prep;
  prep = std::vector<GicpInput>(n_clouds);
  LeafHint hint;
  for (int c : named) {
    GicpInput& P = prep[c];
    s = gicp_index_cloud(&h->tgt, clouds[c]->c, hint, P);
    if (s) return s;
    HIP_TRY(P.cov.reserve(P.n() * 6));
    P.set = P.have_cov = true;  // (the covariances: the launch below, waited for before the first pair)
  }
  // ---- the covariances of all of them: one launch (members in order while their blocks stay within kGicpMultiMaxBlocks,
  // then a further launch)
  std::vector<gicp::KnnMember> tab(named.size());
  std::vector<std::pair<size_t, size_t>> launches;  // [first member, end member)
  size_t knn_launches = 0, knn_blocks = 0;
  {
    size_t first = 0;
    long long blocks = 0;
    for (size_t j = 0; j < named.size(); j++) {
      const GicpInput& P = prep[named[j]];
      const int nb = gicp::knn_blocks(static_cast<int>(P.n()), kGicpMaxBlocks);
      if (blocks > 0 && blocks + nb > kGicpMultiMaxBlocks) {  // (a member is never split: alone it may exceed the limit)
        launches.emplace_back(first, j);
        first = j;
        blocks = 0;
      }
      tab[j].ix = gicp_index_of(P);
      tab[j].cov6 = P.cov.p;
      tab[j].first_block = static_cast<int>(blocks);
      tab[j].n_blocks = nb;
      blocks += nb;
      knn_blocks += static_cast<size_t>(nb);
    }
    launches.emplace_back(first, named.size());
  }
  HIP_TRY(h->member_table.reserve(tab.size() * sizeof(gicp::KnnMember)));
  StreamDrain drain{st};  // (a launch that fails returns with the table's copy waited for)
  HIP_TRY(hipMemcpyAsync(h->member_table.p, tab.data(), tab.size() * sizeof(gicp::KnnMember), hipMemcpyHostToDevice, st));
  for (const auto& l : launches) {
    const gicp::KnnMember* d = reinterpret_cast<const gicp::KnnMember*>(h->member_table.p) + l.first;
    const int nb = tab[l.second - 1].first_block + tab[l.second - 1].n_blocks;
    HIP_TRY(gicp::launch_knn_covariances_multi(d, static_cast<int>(l.second - l.first), nb, k, h->prm.gicp_epsilon, st));
    knn_launches++;
  }
  HIP_TRY(hipStreamSynchronize(st));  // (the table's host copy may go; a failed launch shows here, not in the first pair)
  drain.done = true;
  out.t_prepared = std::chrono::steady_clock::now();
  out.index_builds = named.size();
  out.knn_launches = knn_launches;
  out.knn_blocks = knn_blocks;
  return NDT_OK;
}

// The pairs' results to the caller and the call's records to the handle (both pairs calls, after the last registration).
struct PairsResults {
  std::vector<float> T;
  std::vector<int> conv, it, corr;
  std::vector<double> fit;
  explicit PairsResults(size_t n) : T(16 * n), conv(n), it(n), corr(n), fit(n) {}
  void set(size_t p, const gicp::Result& r) {
    colmajor_from_rowmajor(r.final_T, &T[16 * p]);
    conv[p] = r.converged ? 1 : 0;
    it[p] = r.nr_iterations;
    corr[p] = r.correspondences;
  }
};
static void gicp_pairs_finish(gicp_handle h, PairsPrep& pp, const PairsResults& R, size_t n_pairs, float* final_T, int* converged,
                              int* n_iterations, int* correspondences, double* fitness) {
  if (final_T) std::memcpy(final_T, R.T.data(), R.T.size() * sizeof(float));
  if (converged) std::memcpy(converged, R.conv.data(), n_pairs * sizeof(int));
  if (n_iterations) std::memcpy(n_iterations, R.it.data(), n_pairs * sizeof(int));
  if (correspondences) std::memcpy(correspondences, R.corr.data(), n_pairs * sizeof(int));
  if (fitness) std::memcpy(fitness, R.fit.data(), n_pairs * sizeof(double));
  h->pairs_prepared.swap(pp.prep);
  h->pairs_index_builds = pp.index_builds;
  h->pairs_knn_launches = pp.knn_launches;
  h->pairs_knn_blocks = pp.knn_blocks;
  h->pairs_prepare_ms = std::chrono::duration<double, std::milli>(pp.t_prepared - pp.t_begin).count();
  h->pairs_register_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pp.t_prepared).count();
  h->pairs_valid = true;
}

ndt_status gicp_align_pairs_clouds(gicp_handle h, const ndt_cloud* clouds, size_t n_clouds, const int* pairs, size_t n_pairs,
                                   const float* guesses, double max_range, float* final_T, int* converged, int* n_iterations,
                                   int* correspondences, double* fitness) {
  PairsPrep pp;
  ndt_status s = gicp_pairs_prepare(h, clouds, n_clouds, pairs, n_pairs, pp);
  if (s || pp.empty) return s;
  std::vector<GicpInput>& prep = pp.prep;
  // ---- the pairs, one after the other: gicp_align's registration and gicp_get_fitness_score's score of two records.  The
  // handle's own inputs, covariances, result and statistics are not touched (its step scratch is: gicp_register)
  PairsResults R(n_pairs);
  for (size_t p = 0; p < n_pairs; p++) {
    GicpInput& Pt = prep[pairs[2 * p]];
    GicpInput& Ps = prep[pairs[2 * p + 1]];
    const gicp::Result r = gicp_register(h, Pt, Ps, guesses ? guesses + 16 * p : nullptr, &s);
    if (s) return s;
    R.set(p, r);
    if (fitness) {
      s = fitness_against(&h->tgt, Pt.grid.get(), Ps.cloud().pts.p, static_cast<int>(Ps.n()), &R.T[16 * p], max_range, &R.fit[p]);
      if (s) return s;
    }
  }
  HIP_TRY(hipStreamSynchronize(h->tgt.stream));
  gicp_pairs_finish(h, pp, R, n_pairs, final_T, converged, n_iterations, correspondences, fitness);
  return NDT_OK;
}

ndt_status gicp_align_pairs_lockstep(gicp_handle h, const ndt_cloud* clouds, size_t n_clouds, const int* pairs, size_t n_pairs,
                                     const float* guesses, double max_range, float* final_T, int* converged, int* n_iterations,
                                     int* correspondences, double* fitness) {
  PairsPrep pp;
  ndt_status s = gicp_pairs_prepare(h, clouds, n_clouds, pairs, n_pairs, pp);
  if (s) return s;
  if (pp.empty) {
    h->ls_stats = gicp::LockstepStats();
    h->ls_valid = true;
    return NDT_OK;
  }
  // ---- the pairs, advanced together (gicp::run_lockstep over LockstepDevice), then gicp_get_fitness_score's score of
  // each.  The handle's own inputs, covariances, result, statistics and step scratch are not touched.
  std::vector<LockstepJob> jobs(n_pairs);
  for (size_t p = 0; p < n_pairs; p++) {
    jobs[p].tgt = &pp.prep[pairs[2 * p]];
    jobs[p].src = &pp.prep[pairs[2 * p + 1]];
    rowmajor_from_colmajor(guesses ? guesses + 16 * p : nullptr, jobs[p].guess_rm);
  }
  std::vector<gicp::Result> res;
  gicp::LockstepStats stats;
  s = gicp_register_lockstep(h, jobs, res, stats);
  if (s) return s;
  PairsResults R(n_pairs);
  for (size_t p = 0; p < n_pairs; p++) {
    R.set(p, res[p]);
    if (fitness) {
      s = fitness_against(&h->tgt, jobs[p].tgt->grid.get(), jobs[p].src->cloud().pts.p, static_cast<int>(jobs[p].src->n()), &R.T[16 * p],
                          max_range, &R.fit[p]);
      if (s) return s;
    }
  }
  HIP_TRY(hipStreamSynchronize(h->tgt.stream));
  gicp_pairs_finish(h, pp, R, n_pairs, final_T, converged, n_iterations, correspondences, fitness);
  h->ls_stats = stats;
  h->ls_valid = true;
  return NDT_OK;
}

ndt_status gicp_align_guesses(gicp_handle h, const float* guesses, size_t n_guesses, double max_range, float* final_T, int* converged,
                              int* n_iterations, int* correspondences, double* fitness) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (n_guesses > 65535) return fail(NDT_ERR_INVALID, "at most 65535 guesses per call");
  if (n_guesses == 0) {  // (nothing to register: no device, and no inputs, needed)
    h->ls_stats = gicp::LockstepStats();
    h->ls_valid = true;
    return NDT_OK;
  }
  ndt_status s = gicp_inputs_set(h);
  if (s) return s;
  if (!guesses) return fail(NDT_ERR_INVALID, "null guesses");
  GicpInput& tgt = h->in[0];
  GicpInput& src = h->in[1];
  // the covariances gicp_align would use: the caller's, or the k-NN ones, computed once for all guesses -- and, where this
  // call computed them, not kept: the handle's covariances stay as they were
  struct Restore {
    GicpInput &a, &b;
    bool ha, hb;
    ~Restore() { a.have_cov = ha; b.have_cov = hb; }
  } restore{tgt, src, tgt.have_cov, src.have_cov};
  s = gicp_prepare_covariances(h, tgt, src);
  if (s) return s;
  std::vector<LockstepJob> jobs(n_guesses);
  for (size_t g = 0; g < n_guesses; g++) {
    jobs[g].tgt = &tgt;
    jobs[g].src = &src;
    rowmajor_from_colmajor(guesses + 16 * g, jobs[g].guess_rm);
  }
  std::vector<gicp::Result> res;
  gicp::LockstepStats stats;
  s = gicp_register_lockstep(h, jobs, res, stats);
  if (s) return s;
  PairsResults R(n_guesses);
  for (size_t g = 0; g < n_guesses; g++) {
    R.set(g, res[g]);
    if (fitness) {
      s = fitness_against(&h->tgt, tgt.grid.get(), src.cloud().pts.p, static_cast<int>(src.n()), &R.T[16 * g], max_range, &R.fit[g]);
      if (s) return s;
    }
  }
  HIP_TRY(hipStreamSynchronize(h->tgt.stream));
  if (final_T) std::memcpy(final_T, R.T.data(), R.T.size() * sizeof(float));
  if (converged) std::memcpy(converged, R.conv.data(), n_guesses * sizeof(int));
  if (n_iterations) std::memcpy(n_iterations, R.it.data(), n_guesses * sizeof(int));
  if (correspondences) std::memcpy(correspondences, R.corr.data(), n_guesses * sizeof(int));
  if (fitness) std::memcpy(fitness, R.fit.data(), n_guesses * sizeof(double));
  h->ls_stats = stats;
  h->ls_valid = true;
  return NDT_OK;
}

ndt_status gicp_diag_lockstep(gicp_handle h, size_t* steps, size_t* correspond_launches, size_t* functor_launches,
                              size_t* max_members_in_step) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  if (!h->ls_valid) return fail(NDT_ERR_NO_INPUT, "no successful lock-step call on this handle");
  if (steps) *steps = h->ls_stats.steps;
  if (correspond_launches) *correspond_launches = h->ls_stats.correspond_launches;
  if (functor_launches) *functor_launches = h->ls_stats.functor_launches;
  if (max_members_in_step) *max_members_in_step = h->ls_stats.max_members_in_step;
  return NDT_OK;
}

ndt_status gicp_pairs_covariances(gicp_handle h, size_t cloud, double* cov) {
  if (!h || !cov) return fail(NDT_ERR_INVALID, "bad arguments");
  if (!h->pairs_valid || cloud >= h->pairs_prepared.size() || !h->pairs_prepared[cloud].set)
    return fail(NDT_ERR_NO_INPUT, "the last pairs call computed no covariances for this cloud");
  ndt_status s = ensure_device(&h->tgt);
  if (s) return s;
  return gicp_read_covariances(h, h->pairs_prepared[cloud], cov);
}

ndt_status gicp_diag_pairs(gicp_handle h, size_t* index_builds, size_t* knn_launches, size_t* knn_blocks) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  if (!h->pairs_valid) return fail(NDT_ERR_NO_INPUT, "no successful pairs call on this handle");
  if (index_builds) *index_builds = h->pairs_index_builds;
  if (knn_launches) *knn_launches = h->pairs_knn_launches;
  if (knn_blocks) *knn_blocks = h->pairs_knn_blocks;
  return NDT_OK;
}

ndt_status gicp_diag_pairs_time(gicp_handle h, double* prepare_ms, double* register_ms) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  if (!h->pairs_valid) return fail(NDT_ERR_NO_INPUT, "no successful pairs call on this handle");
  if (prepare_ms) *prepare_ms = h->pairs_prepare_ms;
  if (register_ms) *register_ms = h->pairs_register_ms;
  return NDT_OK;
}

ndt_status gicp_align(gicp_handle h, const float* guess, float* final_T, int* converged, int* n_iterations, void* out_cloud) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  ndt_status s = gicp_inputs_set(h);
  if (s) return s;
  const GicpInput& src = h->in[1];
  const gicp::Result r = gicp_register(h, h->in[0], h->in[1], guess, &s);
  if (s) return s;
  h->result = r;
  colmajor_from_rowmajor(r.final_T, h->final_T);
  (void)gicp_get_result(h, final_T, converged, n_iterations);
  if (out_cloud) {  // pcl::transformPointCloud(*input_, output, final_transformation_), :513-516
    const size_t n = src.n();
    HIP_TRY(h->out_cloud.reserve(n));
    HIP_TRY(ndt::launch_transform(src.cloud().pts.p, static_cast<int>(n), r.final_T, h->out_cloud.p, h->tgt.stream));
    // through page-locked staging: a D2H copy into the caller's pageable buffer is staged by the runtime in small pieces
    const size_t bytes = n * sizeof(float4);
    if (h->out_pinned_bytes < bytes) {
      if (h->out_pinned) (void)hipHostFree(h->out_pinned);
      h->out_pinned = nullptr;
      h->out_pinned_bytes = 0;
      HIP_TRY(hipHostMalloc(&h->out_pinned, bytes + bytes / 4, hipHostMallocDefault));
      h->out_pinned_bytes = bytes + bytes / 4;
    }
    HIP_TRY(hipMemcpyAsync(h->out_pinned, h->out_cloud.p, bytes, hipMemcpyDeviceToHost, h->tgt.stream));
    HIP_TRY(hipStreamSynchronize(h->tgt.stream));
    std::memcpy(out_cloud, h->out_pinned, bytes);
  }
  return NDT_OK;
}

ndt_status gicp_get_result(gicp_handle h, float* final_T, int* converged, int* n_iterations) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  if (final_T) std::memcpy(final_T, h->final_T, sizeof(h->final_T));
  if (converged) *converged = h->result.converged ? 1 : 0;
  if (n_iterations) *n_iterations = h->result.nr_iterations;
  return NDT_OK;
}

ndt_status gicp_get_fitness_score(gicp_handle h, double max_range, double* fitness) {
  if (!h || !fitness) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = gicp_inputs_set(h);
  if (!s) s = gicp_scratch(h);
  if (s) return s;
  const GicpInput& src = h->in[1];
  return fitness_against(&h->tgt, h->in[0].grid.get(), src.cloud().pts.p, static_cast<int>(src.n()), h->final_T, max_range, fitness);
}

ndt_status gicp_get_stats(gicp_handle h, int* n_f, int* n_df, int* n_fdf, int* correspondences) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  if (n_f) *n_f = h->result.n_f;
  if (n_df) *n_df = h->result.n_df;
  if (n_fdf) *n_fdf = h->result.n_fdf;
  if (correspondences) *correspondences = h->result.correspondences;
  return NDT_OK;
}

// setTargetCovariances / setSourceCovariances (gicp_omp.h:165-168,186-189): caller-supplied covariances take the place of
// the k-NN ones until the cloud is set again.  cov: [n][9] row-major 3x3 (symmetric: the upper triangle is kept).
static ndt_status gicp_set_covariances(gicp_handle h, int which, const double* cov, size_t n) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  GicpInput& in = h->in[which];
  if (!in.set) return fail(NDT_ERR_NO_INPUT, "set the cloud before its covariances");
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

ndt_status gicp_step_correspond(gicp_handle h, const float* guess, const float* transformation, int* corr, float* maha,
                                int* n_correspondences) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  ndt_status s = gicp_inputs_set(h);
  if (s) return s;
  GicpInput& tgt = h->in[0];
  GicpInput& src = h->in[1];
  float guess_rm[16];
  s = gicp_prepare(h, tgt, src, guess, guess_rm);
  if (s) return s;
  float T[16];
  rowmajor_from_colmajor(transformation, T);
  double R[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double acc = 0.0;
      for (int k = 0; k < 4; k++) acc += static_cast<double>(T[i * 4 + k]) * static_cast<double>(guess_rm[k * 4 + j]);
      R[i * 3 + j] = acc;
    }
  GicpDevice dev(h, tgt, src);
  if (!dev.correspond(T, R)) return fail(NDT_ERR_HIP, dev.error);
  const size_t n = src.n();
  std::vector<int> c(n);
  HIP_TRY(hipMemcpyAsync(c.data(), h->corr.p, n * sizeof(int), hipMemcpyDeviceToHost, h->tgt.stream));
  if (maha) HIP_TRY(hipMemcpyAsync(maha, h->maha.p, n * 9 * sizeof(float), hipMemcpyDeviceToHost, h->tgt.stream));
  HIP_TRY(hipStreamSynchronize(h->tgt.stream));
  int m = 0;
  for (size_t i = 0; i < n; i++) m += c[i] >= 0;
  if (corr) std::memcpy(corr, c.data(), n * sizeof(int));
  if (n_correspondences) *n_correspondences = m;
  h->step_ready = true;
  return NDT_OK;
}

ndt_status gicp_step_functor(gicp_handle h, int mode, const double* x, double* f, double* g) {
  if (!h || !x || mode < 0 || mode > 2) return fail(NDT_ERR_INVALID, "bad arguments");
  if (!h->step_ready) return fail(NDT_ERR_NO_INPUT, "gicp_step_correspond has not run");
  ndt_status s = gicp_inputs_set(h);
  if (!s) s = gicp_scratch(h);
  if (s) return s;
  GicpDevice dev(h, h->in[0], h->in[1]);
  float T[16];
  gicp::apply_state(x, T);
  gicp::FunctorSums sums;
  if (!dev.sums(mode, T, sums)) return fail(NDT_ERR_HIP, dev.error);
  const int m = static_cast<int>(sums.m);
  if (mode != 1 && f) *f = sums.f / static_cast<double>(m);
  if (mode != 0 && g) {
    for (int i = 0; i < 3; i++) g[i] = sums.g[i] * (2.0 / m);
    double R[9];
    for (int i = 0; i < 9; i++) R[i] = sums.R[i] * (2.0 / m);
    gicp::rotation_gradient(x, R, g);
  }
  return NDT_OK;
}

ndt_status gicp_diag_plan(gicp_handle h, size_t n, int out[4]) {
  if (!h || !out || n > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "bad arguments");
  const int ni = static_cast<int>(n);
  out[0] = gicp::knn_blocks(ni, kGicpMaxBlocks);
  out[1] = gicp::correspond_blocks(ni, kGicpMaxBlocks);
  out[2] = gicp::functor_blocks(ni, kGicpMaxBlocks);
  out[3] = gicp::server_blocks(ni, kGicpMaxBlocks);
  return NDT_OK;
}

void gicp_host_apply_state(const double* x, float* T) {
  float rm[16];
  gicp::apply_state(x, rm);
  colmajor_from_rowmajor(rm, T);
}

}  // extern "C"
