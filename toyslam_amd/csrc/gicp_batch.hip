// gicp_batch.hip -- many GICP registrations in one call (gicp_internal.hpp): the lock-step's slots and its executor on the
// device, what a pairs call prepares and records, and the three batch calls with their one tail.
#include "gicp_internal.hpp"

ndt_status LockstepSlots::reserve(int want, hipStream_t st) {
  rows_per_slot = gicp::server_blocks(1 << 30, kGicpMaxBlocks);
  if (slots < want) {
    HIP_TRY(hipStreamSynchronize(st));
    host.release();
    slots = 0;
    const LockstepLayout L(static_cast<size_t>(want));
    HIP_TRY(host.reserve(L.host_bytes));
    host.zero();
    HIP_TRY(tables.reserve(L.dev_bytes));
    HIP_TRY(partials.reserve(static_cast<size_t>(want) * rows_per_slot * ndt::kEvalStride));
    HIP_TRY(counters.reserve(static_cast<size_t>(want)));
    slots = want;
  }
  HIP_TRY(hipMemsetAsync(counters.p, 0, static_cast<size_t>(slots) * sizeof(unsigned), st));
  return NDT_OK;
}

namespace {
// ---- the lock-step: the device side of gicp::run_lockstep ----------------------------------------------------------
// One registration of the lock-step: two inputs and a guess (column-major, NULL = identity).
struct LockstepJob {
  const GicpInput* tgt;
  const GicpInput* src;
  float guess_rm[16];
  LockstepJob(const GicpInput* t, const GicpInput* s, const float* guess_cm) : tgt(t), src(s) { rowmajor_from_colmajor(guess_cm, guess_rm); }
};

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
  std::string error;

  LockstepDevice(gicp_context* ctx, const std::vector<LockstepJob>& j)
      : h(ctx), jobs(j), L(static_cast<size_t>(ctx->ls.slots)), scratch(static_cast<size_t>(ctx->ls.slots)), slot_of(j.size(), -1) {
    for (int s = h->ls.slots - 1; s >= 0; s--) free_slots.push_back(s);
  }
  template <class T>
  T* host_at(size_t off) const { return reinterpret_cast<T*>(static_cast<unsigned char*>(h->ls.host.p) + off); }
  template <class T>
  T* dev_at(size_t off) const { return reinterpret_cast<T*>(h->ls.tables.p + off); }
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
    m.partials = h->ls.partials.p + static_cast<size_t>(slot) * h->ls.rows_per_slot * ndt::kEvalStride;
    m.counter = h->ls.counters.p + slot;
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
    std::vector<const double*> rows(static_cast<size_t>(n_fun));
    for (int i = 0; i < n_fun; i++) rows[static_cast<size_t>(i)] = row_of(ft[i].slot);
    if (!gicp_wait_rows(st, seq, rows.data(), n_fun, 0xffff, error)) return false;
    double row[ndt::kEvalStride];
    for (int i = 0; i < n_fun; i++) {
      pub_gather(rows[static_cast<size_t>(i)], row);
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
  if (!s) s = h->ls.reserve(window, h->tgt.stream);
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
// What both pairs calls do before the first registration: the argument checks, the named clouds made readable on the main
// stream, the finite check of all of them in one launch, one index per named cloud (a leaf chain of the call's own) and
// the covariances of all of them from one k_knn_covariances_multi launch (a further launch per kGicpMultiMaxBlocks),
// waited for.  n_pairs == 0: nothing is needed, the handle's record is valid and empty, `out` stays as it is.
struct PairsPrep { PairsRecord rec; std::chrono::steady_clock::time_point t_begin, t_prepared; };
static ndt_status gicp_pairs_prepare(gicp_handle h, const ndt_cloud* clouds, size_t n_clouds, const int* pairs, size_t n_pairs, PairsPrep& out) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  // what the last pairs call kept is dropped (the buffers go back to the main stream's pool)
  if (!h->pairs.prepared.empty() && h->tgt.device_ready) (void)ensure_device(&h->tgt);
  h->pairs = PairsRecord();
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
    h->pairs.valid = true;
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
  std::vector<GicpInput>& prep = out.rec.prepared;
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
      out.rec.knn_blocks += static_cast<size_t>(nb);
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
    out.rec.knn_launches++;
  }
  HIP_TRY(hipStreamSynchronize(st));  // (the table's host copy may go; a failed launch shows here, not in the first pair)
  drain.done = true;
  out.t_prepared = std::chrono::steady_clock::now();
  out.rec.index_builds = named.size();
  return NDT_OK;
}

// The tail all three batch calls end in.  Per member: its result from result_of(p, m) -- the lock-step's finished registration,
// or (gicp_align_pairs_clouds) the registration itself, so that a pair's score is queued behind its own registration -- and
// gicp_get_fitness_score's score of its two inputs where the caller asked for it; then the wait for the main stream, the copies.
struct BatchOut { float* final_T; int *converged, *n_iterations, *correspondences; double* fitness; };
struct BatchMember { const GicpInput *tgt, *src; gicp::Result r; };
static ndt_status gicp_batch_tail(gicp_handle h, size_t n, const std::function<ndt_status(size_t, BatchMember&)>& result_of, double max_range,
                                  const BatchOut& out) {
  std::vector<float> T(16 * n);  // (the caller's arrays are written only when every member has succeeded)
  std::vector<int> conv(n), it(n), corr(n);
  std::vector<double> fit(n);
  for (size_t p = 0; p < n; p++) {
    BatchMember m{};
    ndt_status s = result_of(p, m);
    if (s) return s;
    colmajor_from_rowmajor(m.r.final_T, &T[16 * p]);
    conv[p] = m.r.converged ? 1 : 0;
    it[p] = m.r.nr_iterations;
    corr[p] = m.r.correspondences;
    if (out.fitness) {
      s = fitness_against(&h->tgt, m.tgt->grid.get(), m.src->cloud().pts.p, static_cast<int>(m.src->n()), &T[16 * p], max_range, &fit[p]);
      if (s) return s;
    }
  }
  HIP_TRY(hipStreamSynchronize(h->tgt.stream));
  if (out.final_T) std::memcpy(out.final_T, T.data(), T.size() * sizeof(float));
  if (out.converged) std::memcpy(out.converged, conv.data(), n * sizeof(int));
  if (out.n_iterations) std::memcpy(out.n_iterations, it.data(), n * sizeof(int));
  if (out.correspondences) std::memcpy(out.correspondences, corr.data(), n * sizeof(int));
  if (out.fitness) std::memcpy(out.fitness, fit.data(), n * sizeof(double));
  return NDT_OK;
}
static void gicp_pairs_finish(gicp_handle h, PairsPrep& pp) {  // the call's record to the handle (both pairs calls, after the tail)
  pp.rec.prepare_ms = std::chrono::duration<double, std::milli>(pp.t_prepared - pp.t_begin).count();
  pp.rec.register_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pp.t_prepared).count();
  pp.rec.valid = true;
  h->pairs = std::move(pp.rec);
}
// what a lock-step call leaves for gicp_diag_lockstep (one that had nothing to do: fresh statistics, and no device needed)
static ndt_status gicp_lockstep_done(gicp_handle h, const gicp::LockstepStats& stats) {
  h->ls_stats = stats;
  h->ls_valid = true;
  return NDT_OK;
}
// the lock-step's two calls: the jobs advanced together (gicp::run_lockstep over LockstepDevice), the tail, the records (pp: a pairs call's)
static ndt_status gicp_lockstep_batch(gicp_handle h, const std::vector<LockstepJob>& jobs, double max_range, const BatchOut& out, PairsPrep* pp) {
  std::vector<gicp::Result> res;
  gicp::LockstepStats stats;
  ndt_status s = gicp_register_lockstep(h, jobs, res, stats);
  if (!s)
    s = gicp_batch_tail(h, jobs.size(), [&](size_t p, BatchMember& m) { m = BatchMember{jobs[p].tgt, jobs[p].src, res[p]}; return NDT_OK; },
                        max_range, out);
  if (s) return s;
  if (pp) gicp_pairs_finish(h, *pp);
  return gicp_lockstep_done(h, stats);
}

ndt_status gicp_align_pairs_clouds(gicp_handle h, const ndt_cloud* clouds, size_t n_clouds, const int* pairs, size_t n_pairs,
                                   const float* guesses, double max_range, float* final_T, int* converged, int* n_iterations,
                                   int* correspondences, double* fitness) {
  PairsPrep pp;
  ndt_status s = gicp_pairs_prepare(h, clouds, n_clouds, pairs, n_pairs, pp);
  if (s || n_pairs == 0) return s;
  std::vector<GicpInput>& prep = pp.rec.prepared;
  // ---- the pairs, one after the other: gicp_align's registration and gicp_get_fitness_score's score of two records.  The
  // handle's own inputs, covariances, result and statistics are not touched (its step scratch is: gicp_register)
  s = gicp_batch_tail(h, n_pairs, [&](size_t p, BatchMember& m) {
    GicpInput& Pt = prep[pairs[2 * p]];
    GicpInput& Ps = prep[pairs[2 * p + 1]];
    ndt_status rs = NDT_OK;
    m = BatchMember{&Pt, &Ps, gicp_register(h, Pt, Ps, guesses ? guesses + 16 * p : nullptr, &rs)};
    return rs;
  }, max_range, BatchOut{final_T, converged, n_iterations, correspondences, fitness});
  if (!s) gicp_pairs_finish(h, pp);
  return s;
}

ndt_status gicp_align_pairs_lockstep(gicp_handle h, const ndt_cloud* clouds, size_t n_clouds, const int* pairs, size_t n_pairs,
                                     const float* guesses, double max_range, float* final_T, int* converged, int* n_iterations,
                                     int* correspondences, double* fitness) {
  PairsPrep pp;
  ndt_status s = gicp_pairs_prepare(h, clouds, n_clouds, pairs, n_pairs, pp);
  if (s) return s;
  if (n_pairs == 0) return gicp_lockstep_done(h, gicp::LockstepStats());
  // ---- the pairs, advanced together.  The handle's own inputs, covariances, result, statistics and step scratch are not touched.
  std::vector<LockstepJob> jobs;
  for (size_t p = 0; p < n_pairs; p++)
    jobs.emplace_back(&pp.rec.prepared[pairs[2 * p]], &pp.rec.prepared[pairs[2 * p + 1]], guesses ? guesses + 16 * p : nullptr);
  return gicp_lockstep_batch(h, jobs, max_range, BatchOut{final_T, converged, n_iterations, correspondences, fitness}, &pp);
}

ndt_status gicp_align_guesses(gicp_handle h, const float* guesses, size_t n_guesses, double max_range, float* final_T, int* converged,
                              int* n_iterations, int* correspondences, double* fitness) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (n_guesses > 65535) return fail(NDT_ERR_INVALID, "at most 65535 guesses per call");
  if (n_guesses == 0) return gicp_lockstep_done(h, gicp::LockstepStats());  // (nothing to register: no inputs needed either)
  if (h->in[0].vox) return fail(NDT_ERR_INVALID, "the batch forms take cloud targets: the handle's target is a grid target");
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
  std::vector<LockstepJob> jobs;
  for (size_t g = 0; g < n_guesses; g++) jobs.emplace_back(&tgt, &src, guesses + 16 * g);
  return gicp_lockstep_batch(h, jobs, max_range, BatchOut{final_T, converged, n_iterations, correspondences, fitness}, nullptr);
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
  if (!h->pairs.valid || cloud >= h->pairs.prepared.size() || !h->pairs.prepared[cloud].set)
    return fail(NDT_ERR_NO_INPUT, "the last pairs call computed no covariances for this cloud");
  ndt_status s = ensure_device(&h->tgt);
  if (s) return s;
  return gicp_read_covariances(h, h->pairs.prepared[cloud], cov);
}

ndt_status gicp_diag_pairs(gicp_handle h, size_t* index_builds, size_t* knn_launches, size_t* knn_blocks) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  if (!h->pairs.valid) return fail(NDT_ERR_NO_INPUT, "no successful pairs call on this handle");
  if (index_builds) *index_builds = h->pairs.index_builds;
  if (knn_launches) *knn_launches = h->pairs.knn_launches;
  if (knn_blocks) *knn_blocks = h->pairs.knn_blocks;
  return NDT_OK;
}

ndt_status gicp_diag_pairs_time(gicp_handle h, double* prepare_ms, double* register_ms) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  if (!h->pairs.valid) return fail(NDT_ERR_NO_INPUT, "no successful pairs call on this handle");
  if (prepare_ms) *prepare_ms = h->pairs.prepare_ms;
  if (register_ms) *register_ms = h->pairs.register_ms;
  return NDT_OK;
}
}  // extern "C"
