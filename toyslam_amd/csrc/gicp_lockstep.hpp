// gicp_lockstep.hpp -- the lock-step of many GICP registrations (gicp_align_pairs_lockstep, gicp_align_guesses), host side.
// Every member in flight runs gicp::run (gicp_driver.cpp, unchanged: the host arithmetic of a member is the arithmetic of a
// single registration) on a thread of its own, with a backend that only posts what it wants from the device and sleeps.
// The calling thread is the coordinator: when every live member sleeps in sums() or has ended, it hands the step's
// requests to a StepExecutor -- one correspondence launch and one functor launch for all of them on the device
// (gicp_capi.hip), the oracle's functions in the CPU check (tests/gicp_lockstep_check.cpp) -- and wakes the members with
// their sums.  Host-only, no HIP headers; built like gicp_driver.cpp.
#pragma once
#include <cstddef>
#include <vector>

#include "gicp_driver.hpp"

namespace gicp {

// How a Backend::sums request becomes a device request -- ONE piece of code for the single registration (GicpDevice) and
// the lock-step's members.  operator() (mode 0) is asked as mode 3, which also accumulates df's sums, unless fusing is
// off (NDT_GICP_NO_FUSE); the df the line search asks for next at the very same T is then answered from the kept sums
// without a device request; new correspondences invalidate what is kept.
class SumsPlan {
 public:
  explicit SumsPlan(bool fuse) : fuse_(fuse) {}
  void invalidate() { have_grad_ = false; }
  // true: `out` is the answer, nothing to ask
  bool answered(int mode, const float T[16], FunctorSums& out) const;
  int launch_mode(int mode) const { return (mode == 0 && fuse_) ? 3 : mode; }
  // the device's answer to launch_mode at T
  void keep(int launch_mode, const float T[16], const FunctorSums& sums);

 private:
  bool fuse_;
  bool have_grad_ = false;
  float grad_T_[16];
  FunctorSums grad_sums_;
};
bool fuse_enabled();  // NDT_GICP_NO_FUSE unset
// the 14 raw sums of a functor row (f, g[3], R[9], count) as FunctorSums
void sums_from_row(const double* row, FunctorSums& out);

// What one member wants from a step: always one evaluation (mode: launch_functor's numbering, at T), and before it new
// correspondences if the member's outer loop has just asked for them.
struct StepRequest {
  int member = 0;  // index into run_lockstep's members
  bool correspond = false;
  float corr_T[16];  // transformation_, row-major
  double corr_R[9];  // rotation of transformation_ * guess
  int mode = 0;
  float T[16];
};

// All three are called by the coordinator thread only, never by a member's.
class StepExecutor {
 public:
  virtual ~StepExecutor() {}
  // the member joins at the next step: whatever it needs for as long as it is in flight.  false = failure.
  virtual bool start(int member) = 0;
  // the member has ended (its last step is over): its scratch may go
  virtual void finish(int member) = 0;
  // one step: correspondences of the requests that ask for them, then every request's sums into out[i].  false = failure.
  virtual bool step(const std::vector<StepRequest>& requests, std::vector<FunctorSums>& out) = 0;
};

struct LockstepInput {
  Params prm;
  float guess[16];  // row-major
};

struct LockstepStats {
  std::size_t steps = 0;                // executor steps = functor launches
  std::size_t correspond_launches = 0;  // steps in which a member asked for correspondences
  std::size_t functor_launches = 0;
  std::size_t max_members_in_step = 0;
};

// Members in flight at most (NDT_GICP_LOCKSTEP_MEMBERS, a development switch read once: 1 ... 256, default 32).
int lockstep_window();

// Registers every member; at most `window` are in flight, the next one starts at the step after a member has ended.
// results[m] is gicp::run's for member m.  false: the executor failed -- every member that had not ended has
// backend_failed set, the ones never started too.  Every thread it started has been joined when it returns.
bool run_lockstep(const std::vector<LockstepInput>& members, int window, bool fuse, StepExecutor& exec,
                  std::vector<Result>& results, LockstepStats& stats);

}  // namespace gicp
