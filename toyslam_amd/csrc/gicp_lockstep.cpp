// gicp_lockstep.cpp -- see gicp_lockstep.hpp.  Build: g++ -O2 -ffp-contract=off, no HIP headers.
#include "gicp_lockstep.hpp"

#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

namespace gicp {

bool SumsPlan::answered(int mode, const float T[16], FunctorSums& out) const {
  if (mode == 1 && have_grad_ && std::memcmp(T, grad_T_, sizeof(grad_T_)) == 0) {
    out = grad_sums_;
    return true;
  }
  return false;
}

void SumsPlan::keep(int launch_mode, const float T[16], const FunctorSums& sums) {
  if (launch_mode != 3) return;  // slot 0 is operator()'s value; the gradient sums serve the df that follows
  have_grad_ = true;
  std::memcpy(grad_T_, T, sizeof(grad_T_));
  grad_sums_ = sums;
}

bool fuse_enabled() { return std::getenv("NDT_GICP_NO_FUSE") == nullptr; }

void sums_from_row(const double* row, FunctorSums& out) {
  out.f = row[0];
  for (int i = 0; i < 3; i++) out.g[i] = row[1 + i];
  for (int i = 0; i < 9; i++) out.R[i] = row[4 + i];
  out.m = row[13];
}

int lockstep_window() {
  static const int w = [] {
    const char* v = std::getenv("NDT_GICP_LOCKSTEP_MEMBERS");
    return v ? std::min(256, std::max(1, std::atoi(v))) : 32;
  }();
  return w;
}

namespace {

enum State { kRunning, kWaiting, kDone };

struct Shared {
  std::mutex mu;
  std::condition_variable coordinator;  // the last running member began to wait or ended
  int running = 0;                      // members in flight that neither wait nor have ended
};

// One member in flight.  Everything the coordinator and the member's thread both touch is guarded by Shared::mu.
struct Member : Backend {
  Shared& sh;
  const int index;
  SumsPlan plan;
  std::condition_variable wake;
  State state = kRunning;
  bool reply_ok = false;
  bool corr_pending = false;  // (the member's thread alone until it waits)
  StepRequest req;
  FunctorSums reply;
  Result result;
  std::thread thread;

  Member(Shared& s, int idx, bool fuse) : sh(s), index(idx), plan(fuse) { req.member = idx; }

  bool correspond(const float transformation[16], const double R[9]) override {  // recorded; it goes out with the next sums()
    plan.invalidate();
    corr_pending = true;
    std::memcpy(req.corr_T, transformation, sizeof(req.corr_T));
    std::memcpy(req.corr_R, R, sizeof(req.corr_R));
    return true;
  }

  bool sums(int mode, const float T[16], FunctorSums& out) override {
    if (plan.answered(mode, T, out)) return true;
    const int lm = plan.launch_mode(mode);
    std::unique_lock<std::mutex> lk(sh.mu);
    req.correspond = corr_pending;
    req.mode = lm;
    std::memcpy(req.T, T, sizeof(req.T));
    state = kWaiting;
    if (--sh.running == 0) sh.coordinator.notify_one();
    wake.wait(lk, [&] { return state != kWaiting; });
    if (!reply_ok) return false;
    corr_pending = false;
    out = reply;
    lk.unlock();
    plan.keep(lm, T, out);
    return true;
  }
};

}  // namespace

bool run_lockstep(const std::vector<LockstepInput>& members, int window, bool fuse, StepExecutor& exec,
                  std::vector<Result>& results, LockstepStats& stats) {
  const std::size_t n = members.size();
  window = std::max(1, window);
  results.assign(n, Result());
  stats = LockstepStats();
  Shared sh;
  std::vector<std::unique_ptr<Member>> live;  // in order of their start = ascending member index
  std::size_t next = 0;
  bool failed = false;
  std::vector<StepRequest> requests;
  std::vector<FunctorSums> sums;

  auto all_quiet = [&] { return sh.running == 0; };
  // joins the members that have ended, keeps their results, gives their scratch back; true = there was one
  auto reap = [&] {
    bool any = false;
    for (std::size_t i = 0; i < live.size();) {
      bool done;
      {
        std::lock_guard<std::mutex> lk(sh.mu);
        done = live[i]->state == kDone;
      }
      if (!done) {
        i++;
        continue;
      }
      live[i]->thread.join();
      results[live[i]->index] = live[i]->result;
      exec.finish(live[i]->index);
      live.erase(live.begin() + static_cast<std::ptrdiff_t>(i));
      any = true;
    }
    return any;
  };
  // every waiting member is sent back with a failure; they end (backend_failed) and are joined
  auto abandon = [&] {
    failed = true;
    {
      std::unique_lock<std::mutex> lk(sh.mu);
      for (;;) {
        sh.coordinator.wait(lk, all_quiet);
        bool all_done = true;
        for (auto& m : live)
          if (m->state == kWaiting) {
            m->reply_ok = false;
            m->state = kRunning;
            sh.running++;
            m->wake.notify_one();
            all_done = false;
          }
        if (all_done) break;
      }
    }
    reap();
  };

  while (!failed) {
    // the window slides: the places of the members that have ended are taken before the next step
    while (next < n && live.size() < static_cast<std::size_t>(window)) {
      const int idx = static_cast<int>(next);
      if (!exec.start(idx)) {
        failed = true;
        break;
      }
      next++;
      live.emplace_back(new Member(sh, idx, fuse));
      Member* m = live.back().get();
      const LockstepInput* in = &members[idx];
      {
        std::lock_guard<std::mutex> lk(sh.mu);
        sh.running++;
      }
      m->thread = std::thread([m, in] {
        const Result r = run(in->prm, in->guess, *m);
        std::lock_guard<std::mutex> lk(m->sh.mu);
        m->result = r;
        m->state = kDone;
        if (--m->sh.running == 0) m->sh.coordinator.notify_one();
      });
    }
    if (failed) break;
    if (live.empty()) break;
    {
      std::unique_lock<std::mutex> lk(sh.mu);
      sh.coordinator.wait(lk, all_quiet);
    }
    if (reap()) continue;  // (a new member may start, and joins this very step)
    requests.clear();
    bool any_corr = false;
    {
      std::lock_guard<std::mutex> lk(sh.mu);
      for (const auto& m : live) {
        requests.push_back(m->req);
        any_corr = any_corr || m->req.correspond;
      }
    }
    sums.assign(requests.size(), FunctorSums());
    stats.steps++;
    stats.functor_launches++;
    if (any_corr) stats.correspond_launches++;
    stats.max_members_in_step = std::max(stats.max_members_in_step, requests.size());
    if (!exec.step(requests, sums)) {
      failed = true;
      break;
    }
    {
      std::lock_guard<std::mutex> lk(sh.mu);
      for (std::size_t i = 0; i < live.size(); i++) {
        live[i]->reply = sums[i];
        live[i]->reply_ok = true;
        live[i]->state = kRunning;
      }
      sh.running += static_cast<int>(live.size());
    }
    for (auto& m : live) m->wake.notify_one();  // (after the unlock: a woken member takes the mutex at once)
  }
  if (failed) {
    abandon();
    for (Result& r : results) r.backend_failed = true;
  }
  return !failed;
}

}  // namespace gicp
