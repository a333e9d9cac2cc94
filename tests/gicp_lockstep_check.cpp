// tests/gicp_lockstep_check.cpp -- the lock-step of many GICP registrations (toyslam_amd/csrc/gicp_lockstep.cpp) on the CPU.
// A StepExecutor that computes every member's correspondences and functor sums from the oracle's functions
// (oracle/gicp_oracle.cpp) stands in for the device; every member's Result must equal, bit for bit, gicp::run with the
// equivalent single-member backend over the same oracle functions -- whatever the other members, the window and the order
// in which the threads happen to run.  Also: the step counts (copies of one member, window 1) and an executor that fails.
// Built and run by tests/test_gicp_lockstep_host.py (plain, -fsanitize=thread, -fsanitize=address,undefined).
//   usage: gicp_lockstep_check [few]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "gicp_driver.hpp"
#include "gicp_lockstep.hpp"
#include "gicp_oracle.hpp"

using oracle::Pt;

namespace {

// one member: its own clouds, parameters and guess, and the oracle object that holds its correspondences
struct Case {
  std::unique_ptr<oracle::GICP> g;
  gicp::Params prm;
  float guess[4][4];
  std::vector<Pt> output;  // the source moved by the guess
  void reset() {
    output = g->source;
    for (Pt& p : output) p.w = 1.0f;
    oracle::transform_cloud(output, output, guess);
    g->opt_src = &output;
    g->mahalanobis.clear();
    g->corr_src.clear();
    g->corr_tgt.clear();
  }
};

void oracle_correspond(Case& c, const float T[16]) {
  float t[4][4];
  std::memcpy(t, T, sizeof(t));
  c.g->correspond(c.output, t, c.guess);
}

// launch_functor's modes: 0 operator(), 1 / 2 df / fdf, 3 operator() in slot 0 with df's sums
void oracle_sums(const Case& c, int launch_mode, const float T[16], gicp::FunctorSums& out) {
  float t[4][4];
  std::memcpy(t, T, sizeof(t));
  double raw[14];
  if (launch_mode == 3) {
    double f0[14];
    c.g->functor_raw(0, t, f0);
    c.g->functor_raw(1, t, raw);
    raw[0] = f0[0];
  } else {
    c.g->functor_raw(launch_mode, t, raw);
  }
  gicp::sums_from_row(raw, out);
}

// the single registration: what GicpDevice does, over the oracle's functions
struct SingleBackend : gicp::Backend {
  Case& c;
  gicp::SumsPlan plan;
  int requests = 0;  // evaluations that went to the "device"
  SingleBackend(Case& cs, bool fuse) : c(cs), plan(fuse) { c.reset(); }
  bool correspond(const float T[16], const double*) override {
    plan.invalidate();
    oracle_correspond(c, T);
    return true;
  }
  bool sums(int mode, const float T[16], gicp::FunctorSums& out) override {
    if (plan.answered(mode, T, out)) return true;
    const int lm = plan.launch_mode(mode);
    requests++;
    oracle_sums(c, lm, T, out);
    plan.keep(lm, T, out);
    return true;
  }
};

struct OracleExecutor : gicp::StepExecutor {
  std::vector<Case>& cases;
  int fail_at_step = 0;  // 1-based; 0 = never
  int steps = 0, in_flight = 0, max_in_flight = 0;
  std::vector<int> started_before_step;  // per member: the step it first takes part in
  explicit OracleExecutor(std::vector<Case>& cs) : cases(cs), started_before_step(cs.size(), 0) {}
  bool start(int m) override {
    cases[static_cast<size_t>(m)].reset();
    started_before_step[static_cast<size_t>(m)] = steps + 1;
    in_flight++;
    if (in_flight > max_in_flight) max_in_flight = in_flight;
    return true;
  }
  void finish(int) override { in_flight--; }
  bool step(const std::vector<gicp::StepRequest>& rq, std::vector<gicp::FunctorSums>& out) override {
    steps++;
    if (steps == fail_at_step) return false;
    for (size_t i = 0; i < rq.size(); i++) {
      Case& c = cases[static_cast<size_t>(rq[i].member)];
      if (rq[i].correspond) oracle_correspond(c, rq[i].corr_T);
      oracle_sums(c, rq[i].mode, rq[i].T, out[i]);
    }
    return true;
  }
};

std::vector<Pt> scene(std::mt19937_64& rng, int n) {  // a floor, two walls, a little clutter
  std::uniform_real_distribution<float> u(0.f, 1.f);
  std::normal_distribution<float> nz(0.f, 0.01f);
  std::vector<Pt> c(static_cast<size_t>(n));
  for (int i = 0; i < n; i++) {
    const float s = u(rng);
    Pt p{0, 0, 0, 1};
    if (s < 0.5f) p = Pt{20 * u(rng) - 10, 20 * u(rng) - 10, nz(rng), 1};
    else if (s < 0.75f) p = Pt{-10 + nz(rng), 20 * u(rng) - 10, 4 * u(rng), 1};
    else if (s < 0.95f) p = Pt{20 * u(rng) - 10, 10 + nz(rng), 4 * u(rng), 1};
    else p = Pt{20 * u(rng) - 10, 20 * u(rng) - 10, 4 * u(rng), 1};
    c[static_cast<size_t>(i)] = p;
  }
  return c;
}

void small_T(std::mt19937_64& rng, float max_t, float max_deg, float T[4][4]) {
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  const double p[6] = {max_t * u(rng), max_t * u(rng), max_t * u(rng), max_deg * u(rng) * M_PI / 180, max_deg * u(rng) * M_PI / 180,
                       max_deg * u(rng) * M_PI / 180};
  oracle::pose_to_matrix(p, T);
}

Case make_case(std::mt19937_64& rng, int variant) {
  Case c;
  const int nt = 300 + static_cast<int>(rng() % 500), ns = 40 + static_cast<int>(rng() % 300);
  std::vector<Pt> tgt = scene(rng, nt);
  float Tgt[4][4];
  small_T(rng, 0.3f, 2.0f, Tgt);
  std::vector<Pt> pick(static_cast<size_t>(ns)), src(static_cast<size_t>(ns));
  for (int i = 0; i < ns; i++) pick[static_cast<size_t>(i)] = tgt[rng() % static_cast<unsigned>(nt)];
  oracle::transform_cloud(pick, src, Tgt);
  std::normal_distribution<float> nz(0.f, 0.01f);
  for (Pt& p : src) { p.x += nz(rng); p.y += nz(rng); p.z += nz(rng); }
  small_T(rng, 0.2f, 1.5f, c.guess);
  c.g.reset(new oracle::GICP());
  c.g->prm.k_correspondences = 10;
  c.g->set_target(tgt);
  c.g->set_source(src);
  oracle::GICP::covariances(c.g->target, c.g->prm.k_correspondences, c.g->prm.gicp_epsilon, c.g->target_cov);
  oracle::GICP::covariances(c.g->source, c.g->prm.k_correspondences, c.g->prm.gicp_epsilon, c.g->source_cov);
  c.prm.k_correspondences = 10;
  if (variant == 1) c.prm.corr_dist_threshold = 1e-4;  // fewer than 4 correspondences: ends at once
  if (variant == 2) c.prm.max_iterations = 1;
  if (variant == 4) c.prm.max_inner_iterations = 5;
  c.g->prm.corr_dist_threshold = c.prm.corr_dist_threshold;
  if (variant == 3) {  // starts at the answer
    SingleBackend be(c, true);
    float g16[16];
    std::memcpy(g16, c.guess, sizeof(g16));
    const gicp::Result r = gicp::run(c.prm, g16, be);
    std::memcpy(c.guess, r.final_T, sizeof(c.guess));
  }
  return c;
}

Case copy_case(const Case& o) {
  Case c;
  c.g.reset(new oracle::GICP(*o.g));
  c.prm = o.prm;
  std::memcpy(c.guess, o.guess, sizeof(c.guess));
  return c;
}

bool same(const gicp::Result& a, const gicp::Result& b) {
  return std::memcmp(a.final_T, b.final_T, sizeof(a.final_T)) == 0 && a.converged == b.converged && a.backend_failed == b.backend_failed &&
         a.nr_iterations == b.nr_iterations && a.n_f == b.n_f && a.n_df == b.n_df && a.n_fdf == b.n_fdf &&
         a.correspondences == b.correspondences;
}

std::vector<gicp::LockstepInput> inputs_of(const std::vector<Case>& cases) {
  std::vector<gicp::LockstepInput> in(cases.size());
  for (size_t i = 0; i < cases.size(); i++) {
    in[i].prm = cases[i].prm;
    std::memcpy(in[i].guess, cases[i].guess, sizeof(in[i].guess));
  }
  return in;
}

int bad = 0;
void expect(bool ok, const std::string& what) {
  if (!ok) {
    bad++;
    std::printf("FAILED: %s\n", what.c_str());
  }
}

}  // namespace

int main(int argc, char** argv) {
  const bool few = argc > 1 && std::strcmp(argv[1], "few") == 0;
  const std::vector<int> scenes = few ? std::vector<int>{1, 3, 9} : std::vector<int>{1, 2, 3, 9, 40};
  const int windows[3] = {1, 2, 32};
  std::mt19937_64 rng(20251018);
  int at_once = 0, one_iter = 0, at_answer = 0, members_checked = 0;
  std::vector<Case> last;
  for (int M : scenes) {
    for (int fuse = 1; fuse >= (few ? 1 : 0); fuse--) {
      std::vector<Case> cases;
      for (int i = 0; i < M; i++) cases.push_back(make_case(rng, M == 1 ? 0 : i % 5));
      // every member alone
      std::vector<gicp::Result> want(cases.size());
      long long own_steps = 0;
      for (size_t i = 0; i < cases.size(); i++) {
        SingleBackend be(cases[i], fuse != 0);
        float g16[16];
        std::memcpy(g16, cases[i].guess, sizeof(g16));
        want[i] = gicp::run(cases[i].prm, g16, be);
        own_steps += be.requests;
        at_once += want[i].nr_iterations == 0 && want[i].correspondences < 4;
        one_iter += cases[i].prm.max_iterations == 1 && want[i].nr_iterations == 1;
        at_answer += (i % 5 == 3) && want[i].converged && want[i].nr_iterations == 1;
      }
      for (int w : windows) {
        OracleExecutor ex(cases);
        std::vector<gicp::Result> got;
        gicp::LockstepStats st;
        const bool ok = gicp::run_lockstep(inputs_of(cases), w, fuse != 0, ex, got, st);
        const std::string ctx = "members " + std::to_string(M) + " window " + std::to_string(w) + " fuse " + std::to_string(fuse);
        expect(ok && got.size() == cases.size(), ctx + ": run");
        for (size_t i = 0; ok && i < cases.size(); i++) {
          expect(same(got[i], want[i]), ctx + ": member " + std::to_string(i));
          members_checked++;
        }
        expect(ex.in_flight == 0 && ex.max_in_flight == std::min(w, M), ctx + ": members in flight");
        expect(st.steps == static_cast<size_t>(ex.steps) && st.functor_launches == st.steps && st.correspond_launches <= st.steps &&
                   st.max_members_in_step <= static_cast<size_t>(std::min(w, M)) && st.max_members_in_step >= 1,
               ctx + ": statistics");
        if (w == 1) expect(static_cast<long long>(st.steps) == own_steps, ctx + ": with window 1 the steps are the sum of the members' own");
      }
      last.swap(cases);
    }
  }
  expect(few || (at_once > 0 && one_iter > 0 && at_answer > 0), "the scenes hold members that end at once, after one iteration, at the answer");

  // M copies of one member within the window take exactly the steps of one copy
  {
    Case one = make_case(rng, 0);
    size_t one_steps = 0, one_corr = 0;
    for (int M : {1, 2, 9}) {
      std::vector<Case> copies;
      for (int i = 0; i < M; i++) copies.push_back(copy_case(one));
      OracleExecutor ex(copies);
      std::vector<gicp::Result> got;
      gicp::LockstepStats st;
      const bool ok = gicp::run_lockstep(inputs_of(copies), 32, true, ex, got, st);
      if (M == 1) {
        one_steps = st.steps;
        one_corr = st.correspond_launches;
      }
      expect(ok && st.steps == one_steps && st.correspond_launches == one_corr && st.max_members_in_step == static_cast<size_t>(M) && one_steps > 2,
             "copies " + std::to_string(M) + ": the steps of one copy");
      for (int i = 1; ok && i < M; i++) expect(same(got[static_cast<size_t>(i)], got[0]), "copies " + std::to_string(M) + ": equal results");
    }
  }

  // an executor that fails: at step 1, at step 7, and at the step in which a new member starts (window 2)
  {
    std::vector<Case>& cases = last;  // the last scene: 9 or 40 members
    int start_step = 0;
    {
      OracleExecutor ex(cases);
      std::vector<gicp::Result> got;
      gicp::LockstepStats st;
      gicp::run_lockstep(inputs_of(cases), 2, true, ex, got, st);
      for (size_t i = 2; i < cases.size() && !start_step; i++)
        if (ex.started_before_step[i] > 1) start_step = ex.started_before_step[i];
    }
    expect(start_step > 1, "a member starts at a later step");
    for (int at : {1, 7, start_step})
      for (int w : {2, 32}) {
        OracleExecutor ex(cases);
        ex.fail_at_step = at;
        std::vector<gicp::Result> got;
        gicp::LockstepStats st;
        const bool ok = gicp::run_lockstep(inputs_of(cases), w, true, ex, got, st);
        const std::string ctx = "failure at step " + std::to_string(at) + " window " + std::to_string(w);
        expect(!ok && got.size() == cases.size() && ex.steps == at && ex.in_flight == 0, ctx + ": the run returns");
        for (size_t i = 0; i < got.size(); i++) expect(got[i].backend_failed, ctx + ": member " + std::to_string(i) + " has backend_failed");
      }
  }
  std::printf("members checked %d (at once %d, one iteration %d, at the answer %d) failures %d\n", members_checked, at_once, one_iter,
              at_answer, bad);
  return bad ? 1 : 0;
}
