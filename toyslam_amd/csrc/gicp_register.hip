// gicp_register.hip -- one GICP registration of a source input onto a target input (gicp_internal.hpp): its preparation, GicpDevice,
// the persistent objective server, the wait for published rows; gicp_align, the fitness score and the two step calls.
#include "gicp_internal.hpp"

// ---- persistent objective server (ObjectiveServer, gicp_internal.hpp) ------------------------------------------------
bool ObjectiveServer::available(int device) {
  if (tried) return mbs != nullptr;
  tried = true;
  const char* v = std::getenv("NDT_GICP_SERVER");
  if (v && std::atoi(v) == 0) return false;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || prop.isLargeBar == 0) return false;  // the direct mailbox needs the BAR
  const size_t mb = ndt::server_mailbox_bytes();
  if (hipExtMallocWithFlags(&mbs, 2 * mb, hipDeviceMallocFinegrained) != hipSuccess) {
    mbs = nullptr;
    (void)hipGetLastError();
    return false;
  }
  if (hipMemset(mbs, 0, 2 * mb) != hipSuccess || rows.reserve(gicp::kGicpServerParts * ndt::kPublishSlots * sizeof(double)) != hipSuccess ||
      counter.reserve(32 * gicp::kGicpServerParts) != hipSuccess) {
    (void)hipFree(mbs);
    mbs = nullptr;
    (void)hipGetLastError();
    return false;
  }
  rows.zero();
  return true;
}
bool ObjectiveServer::start(gicp_context* h, const GicpInput& tgt, const GicpInput& src, std::string& error) {
  server_mark(&h->tgt, true);  // this device's turn among the persistent kernels of the process
  flip ^= 1;
  ndt::server_reset_mailbox(mailbox());
  const int n = static_cast<int>(src.n());
  blocks = gicp::server_blocks(n, kGicpMaxBlocks);
  hipError_t e = hipMemsetAsync(counter.p, 0, 32 * gicp::kGicpServerParts * sizeof(unsigned), h->tgt.stream);
  if (e == hipSuccess) e = h->partials.reserve(static_cast<size_t>(std::max(blocks, gicp::kFunctorMaxBlocks)) * ndt::kEvalStride);
  if (e == hipSuccess)
    e = gicp::launch_server(h->output.p, n, tgt.points(), h->corr.p, h->maha.p, mailbox(), blocks, h->partials.p,
                            counter.p, rows.rows(), h->seq + 1, 2000000ull /* 20 ms */, h->tgt.stream);
  if (e != hipSuccess) {
    server_mark(&h->tgt, false);
    error = std::string("objective server: ") + hipGetErrorString(e);
    return false;
  }
  return true;
}
void ObjectiveServer::stop(gicp_context* h) {
  if (!h->tgt.server_running) return;
  ndt::server_post(mailbox(), ++h->seq, ndt::kServerCmdExit, nullptr, nullptr);
  server_mark(&h->tgt, false);
}
bool ObjectiveServer::sums(gicp_context* h, int launch_mode, const float T[16], double row[ndt::kEvalStride]) {
  const unsigned long long seq = ++h->seq;
  ndt::server_post(mailbox(), seq, launch_mode, T, nullptr);
  const int n_parts = std::min(gicp::kGicpServerParts, blocks);
  unsigned arrived = 0;
  const unsigned all = (1u << n_parts) - 1u;
  unsigned spins = 0;
  for (;;) {
    for (int p = 0; p < n_parts; p++)
      if (!(arrived & (1u << p)) && pub_ready(rows.rows() + static_cast<size_t>(p) * ndt::kPublishSlots, seq)) arrived |= 1u << p;
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
    if (p < n_parts) pub_gather(rows.rows() + static_cast<size_t>(p) * ndt::kPublishSlots, part);
    for (int k = 0; k < ndt::kEvalStride; k++) row[k] += (p < n_parts) ? part[k] : 0.0;
  }
  return true;
}

namespace {
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
    h->srv.stop(h);  // the correspondences change: the next BFGS run gets a fresh server behind this kernel
    const double thr = h->prm.corr_dist_threshold * h->prm.corr_dist_threshold;  // :401
    const int n = static_cast<int>(src.n());
    const hipError_t e = tgt.vox ? gicp_grid_correspond(h, n, transformation, rot, src.cov.p, thr)  // a voxel target: through the map's table
                                 : gicp::launch_correspond(h->output.p, n, transformation, rot, gicp_index_of(tgt), src.cov.p, tgt.cov.p, thr,
                                                           gicp::correspond_blocks(n, kGicpMaxBlocks), h->corr.p, h->maha.p, h->tgt.stream);
    if (e != hipSuccess) {
      error = std::string("correspondence kernel: ") + hipGetErrorString(e);
      return false;
    }
    return true;
  }

  bool sums(int mode, const float T[16], gicp::FunctorSums& out) override {
    if (plan.answered(mode, T, out)) return true;
    const int n = static_cast<int>(src.n());
    const int launch_mode = plan.launch_mode(mode);
    double row[ndt::kEvalStride];
    bool have_row = false;
    if (h->srv.available(h->tgt.device)) {
      if (!h->tgt.server_running && !h->srv.start(h, tgt, src, error)) return false;
      // liveness test hook: a host that goes quiet in the middle of a BFGS run (the server's patience is 20 ms)
      static const int stall_ms = std::getenv("NDT_GICP_TEST_STALL_MS") ? std::atoi(std::getenv("NDT_GICP_TEST_STALL_MS")) : 0;
      if (stall_ms > 0 && ++evals_served == 5) std::this_thread::sleep_for(std::chrono::milliseconds(stall_ms));
      have_row = h->srv.sums(h, launch_mode, T, row);
    }
    if (!have_row) {
      const unsigned long long seq = ++h->seq;
      const double* pub = h->host_pub.rows();
      const hipError_t e = gicp::launch_functor(launch_mode, h->output.p, n, tgt.points(), h->corr.p, h->maha.p, T,
                                                gicp::functor_blocks(n, kGicpMaxBlocks), h->partials.p, h->counter.p, h->host_pub.rows(), seq, h->tgt.stream);
      if (e != hipSuccess) {
        error = std::string("functor kernel: ") + hipGetErrorString(e);
        return false;
      }
      if (!gicp_wait_rows(h->tgt.stream, seq, &pub, 1, 0xfffff, error)) return false;
      pub_gather(pub, row);
    }
    gicp::sums_from_row(row, out);
    plan.keep(launch_mode, T, out);
    return true;
  }
  ~GicpDevice() override { h->srv.stop(h); }
};
}  // namespace

namespace ndtc {
// the main stream current (device, this thread's pool stream) and the scratch every evaluation needs
ndt_status gicp_scratch(gicp_context* h) {
  ndt_status s = ensure_device(&h->tgt);
  if (s) return s;
  if (!h->host_pub.p) {
    HIP_TRY(h->host_pub.reserve(ndt::kPublishSlots * sizeof(double)));
    h->host_pub.zero();
  }
  if (!h->counter.p) {
    HIP_TRY(h->counter.reserve(1));
    HIP_TRY(hipMemsetAsync(h->counter.p, 0, sizeof(unsigned), h->tgt.stream));
  }
  return NDT_OK;
}

bool gicp_wait_rows(hipStream_t st, unsigned long long seq, const double* const* rows, int n, unsigned long long look_every, std::string& error) {
  int arrived = 0;
  std::vector<char> have(static_cast<size_t>(n), 0);
  for (unsigned long long spins = 1; arrived < n; spins++) {
    for (int i = 0; i < n; i++)
      if (!have[static_cast<size_t>(i)] && pub_ready(rows[i], seq)) {
        have[static_cast<size_t>(i)] = 1;
        arrived++;
      }
    if (arrived < n && (spins & look_every) == 0) {
      const hipError_t q = hipStreamQuery(st);
      if (q == hipSuccess) {
        bool all = true;
        for (int i = 0; i < n; i++) all = all && pub_ready(rows[i], seq);
        if (all) break;
        error = "functor kernel finished without publishing its result";
        return false;
      }
      if (q != hipErrorNotReady) {
        error = std::string("functor kernel: ") + hipGetErrorString(q);
        return false;
      }
    }
  }
  return true;
}

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
  h->srv.stop(h);  // before anything else is queued on the stream or waited for: the server would sit out its patience
  if (r.backend_failed || !dev.error.empty()) *status = fail(NDT_ERR_HIP, dev.error.empty() ? "device failure" : dev.error);
  return r;
}
}  // namespace ndtc

extern "C" {
ndt_status gicp_align(gicp_handle h, const float* guess, float* final_T, int* converged, int* n_iterations, void* out_cloud) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  ndt_status s = gicp_inputs_set(h);
  if (!s) s = gicp_grid_ready(h);
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
    HIP_TRY(h->out_pinned.reserve(bytes, bytes / 4));
    HIP_TRY(hipMemcpyAsync(h->out_pinned.p, h->out_cloud.p, bytes, hipMemcpyDeviceToHost, h->tgt.stream));
    HIP_TRY(hipStreamSynchronize(h->tgt.stream));
    std::memcpy(out_cloud, h->out_pinned.p, bytes);
  }
  return NDT_OK;
}

ndt_status gicp_get_fitness_score(gicp_handle h, double max_range, double* fitness) {
  if (!h || !fitness) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = gicp_inputs_set(h);
  if (!s) s = gicp_scratch(h);
  if (!s) s = gicp_grid_ready(h);
  if (s) return s;
  const GicpInput& src = h->in[1];
  if (h->in[0].vox) return gicp_grid_fitness(h, src.cloud().pts.p, static_cast<int>(src.n()), h->final_T, max_range, fitness);
  return fitness_against(&h->tgt, h->in[0].grid.get(), src.cloud().pts.p, static_cast<int>(src.n()), h->final_T, max_range, fitness);
}

ndt_status gicp_step_correspond(gicp_handle h, const float* guess, const float* transformation, int* corr, float* maha,
                                int* n_correspondences) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  ndt_status s = gicp_inputs_set(h);
  if (!s) s = gicp_grid_ready(h);
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
  if (!s) s = gicp_grid_ready(h);  // (a voxel target that has changed since the step: its ordinals are gone)
  if (s) return s;
  if (!h->step_ready) return fail(NDT_ERR_NO_INPUT, "the grid target has changed: gicp_step_correspond has to run again");
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
}  // extern "C"
