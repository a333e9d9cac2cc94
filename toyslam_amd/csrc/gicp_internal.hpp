// gicp_internal.hpp -- private to the units of the GICP row (include/gicp_mi355.h): gicp_capi.hip, gicp_inputs.hip,
// gicp_register.hip, gicp_batch.hip, gicp_grid.hip (what each holds: ndt_internal.hpp's list).  They reuse the NDT units' device pool, cloud upload and
// K1 grid build -- the voxel index K1 produces over a cloud is the search structure of GICP's nearest-neighbour queries.
//
// One input of a registration is a GicpInput: a cloud's search index (which holds the cloud), its packed covariances and
// where they came from.  The handle's own target and source are two of them (in[0], in[1]), the clouds a pairs call
// prepares are more of them, and a registration (gicp_register, gicp_prepare, GicpDevice) is a function of two of them --
// its parameters, streams and scratch are the handle's.  The two ndt_contexts a gicp_context owns are tools, not state:
// `tgt` is the main stream (all GICP kernels run on it) and the builder of every index but the handle's source's, `src`
// builds that one and runs its k-NN covariances next to the target's.  Neither keeps a cloud or a grid between calls.
#pragma once
#include "ndt_internal.hpp"
#include "gicp_lockstep.hpp"

struct LeafHint {  // consecutive clouds have about the same density: the index leaf the previous one ended up with, and its size
  float leaf = 0.f;
  size_t n = 0;
};

// A VOXEL target (gicp_set_input_target_grid, gicp_grid.hip): the NDT handle whose current target grid is the target -- borrowed,
// the caller keeps it alive -- and what is materialised from that grid's table and records in one mark / scan (or sort) /
// gather pass: the set D of its valid voxels in ascending linear voxel index.  Refreshed when the grid's generation has moved,
// when the handle holds another grid, or when gicp_epsilon (PLANE covariances) has changed.
struct GridTarget {
  ndt_context* map = nullptr;
  int cov_mode = 0;
  std::weak_ptr<DeviceGrid> seen;  // the grid the arrays were made from (expired: that grid is gone, whatever lies at its address)
  unsigned long long seen_generation = 0;
  double seen_epsilon = 0;
  bool valid = false;
  DevBuf<float4> pts;      // [n] the voxels' f32 centroids (x, y, z, 1)
  DevBuf<double> cov;      // [n][6]
  DevBuf<long long> idx;   // [n] linear voxel indices, ascending
  DevBuf<int> ord;         // per record of the grid: its ordinal in D (read only through table entries that are records)
  size_t n = 0;
  size_t refreshes = 0, correspond_blocks = 0;  // gicp_diag_target_grid
  hipEvent_t ev = nullptr;                      // the map's stream -> the main stream
  ~GridTarget() { if (ev) (void)hipEventDestroy(ev); }
};

struct GicpInput {
  std::shared_ptr<DeviceGrid> grid;  // the search index; grid->target is the cloud
  const GridTarget* vox = nullptr;   // the handle's target only: a voxel target instead (no index, no cloud; covariances in vox)
  DevBuf<double> cov;                // [n][6]
  bool have_cov = false;
  bool user_cov = false;  // supplied through gicp_set_*_covariances
  // the setters' side: the input has been set (a pairs call's record: the cloud was named), the leaf chain of this slot
  bool set = false;
  LeafHint hint;
  const DeviceCloud& cloud() const { return *grid->target; }
  size_t n() const { return vox ? vox->n : grid->target->n; }
  // what the objective kernels read of a target: its points and packed covariances
  const float4* points() const { return vox ? vox->pts.p : grid->target->pts.p; }
  const double* covariances() const { return vox ? vox->cov.p : cov.p; }
};

struct gicp_context;
// A grow-only block of page-locked host memory that frees itself.  A block that grows is freed first: the caller has waited
// for whatever read or wrote the old one.  slack: what a new block gets beyond `want`.
struct PinnedBlock {
  void* p = nullptr;
  size_t bytes = 0;
  PinnedBlock() = default;
  PinnedBlock(const PinnedBlock&) = delete;
  ~PinnedBlock() { release(); }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
  hipError_t reserve(size_t want, size_t slack = 0) {
    if (bytes >= want) return hipSuccess;
    release();
    const hipError_t e = hipHostMalloc(&p, want + slack, hipHostMallocDefault);
    if (e != hipSuccess) p = nullptr;
    else bytes = want + slack;
    return e;
  }
  void zero() { std::memset(p, 0, bytes); }
  double* rows() const { return static_cast<double*>(p); }
};

// what a pairs call leaves behind (gicp_pairs_covariances, gicp_diag_pairs, gicp_diag_pairs_time): what it prepared for
// every cloud (`set`: a pair named it), what it launched, the host wall clock of its two halves (tools/time_gicp_pairs.py)
struct PairsRecord {
  std::vector<GicpInput> prepared;
  size_t index_builds = 0, knn_launches = 0, knn_blocks = 0;
  double prepare_ms = 0, register_ms = 0;
  bool valid = false;
};

// persistent objective server (one launch per BFGS run): two alternating command mailboxes in host-visible device
// memory, shard counters, the pinned part rows.  It lives with the handle; a registration's GicpDevice drives it.
struct ObjectiveServer {
  void* mbs = nullptr;
  int flip = 0, blocks = 0;
  bool tried = false;
  PinnedBlock rows;  // (it and the counters keep the server from being copied)
  DevBuf<unsigned> counter;
  ~ObjectiveServer() { if (mbs) (void)hipFree(mbs); }
  void* mailbox() const { return static_cast<unsigned char*>(mbs) + static_cast<size_t>(flip) * ndt::server_mailbox_bytes(); }
  bool available(int device);
  bool start(gicp_context* h, const GicpInput& tgt, const GicpInput& src, std::string& error);
  void stop(gicp_context* h);  // the last command: everything queued later on the stream runs behind the exiting kernel
  // one evaluation through the server; false = it has left (idle time-out): the caller uses the launch path
  bool sums(gicp_context* h, int launch_mode, const float T[16], double row[ndt::kEvalStride]);
};
inline size_t ls_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

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

// the lock-step (gicp_align_pairs_lockstep, gicp_align_guesses): the slots' tagged rows and the tables' staging in pinned
// host memory, the tables, partial rows and ticket counters on the device (grow-only, sized by the window)
struct LockstepSlots {
  PinnedBlock host;
  int slots = 0, rows_per_slot = 0;  // (partial rows a slot may need: the largest grid of k_functor_multi's members)
  DevBuf<unsigned char> tables;
  DevBuf<double> partials;
  DevBuf<unsigned> counters;
  ndt_status reserve(int want, hipStream_t st);  // at least `want` slots, behind a wait for `st` where they grow; counters zeroed on `st`
};

// Release order: `tgt` and `src` are the first members, so they are destroyed last.  The destructor body waits for both
// streams and makes the main stream's pool current; then every member below goes, in reverse order of declaration -- the
// DevBufs into that pool, the pinned blocks and the server's mailboxes back to the runtime -- and only then do tgt and
// src empty their pools and destroy the two streams.
struct gicp_context {
  ndt_context tgt, src;
  gicp::Params prm;
  GicpInput in[2];                  // target, source
  GridTarget grid_target;           // in[0].vox points here while the target is a voxel target
  DevBuf<float4> output;            // the source moved by the guess
  DevBuf<int> corr;
  DevBuf<float> maha;
  DevBuf<double> partials;
  DevBuf<unsigned> counter;
  DevBuf<float4> out_cloud;
  DevBuf<int> nn_idx;
  DevBuf<float> nn_d2;
  PinnedBlock host_pub;    // tagged publication row
  PinnedBlock out_pinned;  // page-locked staging of the aligned cloud
  ObjectiveServer srv;
  bool src_cov_pending = false;
  hipEvent_t ev_src = nullptr;  // the source's covariance pass (on src's stream) -> the main stream
  unsigned long long seq = 0;
  bool step_ready = false;
  PairsRecord pairs;                   // of the last successful pairs call
  DevBuf<unsigned char> member_table;  // the member tables of the finite check and of k_knn_covariances_multi
  LockstepSlots ls;
  bool ls_valid = false;  // what the last successful lock-step call did (gicp_diag_lockstep)
  gicp::LockstepStats ls_stats;
  DevBuf<unsigned> finite_counts;
  // the last gicp_align's result
  gicp::Result result;
  float final_T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // column-major
  ndt_context* builder(int which) { return which == 0 ? &tgt : &src; }
  ~gicp_context() {
    for (ndt_context* c : {&src, &tgt})
      if (c->device_ready) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        tls_pool_stream = c->stream;
      }
    if (ev_src) (void)hipEventDestroy(ev_src);
  }
};

namespace ndtc {
// development switches, read from the environment once per process (gicp_capi.hip)
extern const double kGicpPointsPerCell;
extern const int kGicpMaxBlocks, kGicpMultiMaxBlocks;
constexpr long long kGicpMaxCells = 1ll << 26;       // dense cell table budget (256 MB of int)

// An asynchronous copy from pageable host memory is queued on `s`: unless the success path has synchronised already
// (done), leaving the scope waits for the stream, so an error return between the copy and that synchronise cannot free
// the host memory under a copy still queued.
struct StreamDrain {
  hipStream_t s;
  bool done = false;
  ~StreamDrain() { if (!done) (void)hipStreamSynchronize(s); }
};

inline gicp::PointIndex gicp_index_of(const GicpInput& in) {
  gicp::PointIndex ix;
  fill_point_index(in.grid.get(), ix);
  return ix;
}

inline void rowmajor_from_colmajor(const float* cm, float* rm) {
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) rm[r * 4 + c] = cm ? cm[c * 4 + r] : (r == c ? 1.0f : 0.0f);
}
inline void colmajor_from_rowmajor(const float* rm, float* cm) {
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) cm[c * 4 + r] = rm[r * 4 + c];
}

inline ndt_status gicp_inputs_set(const gicp_context* h) {
  if (!h->in[0].set) return fail(NDT_ERR_NO_INPUT, "no target cloud set");
  if (!h->in[1].set) return fail(NDT_ERR_NO_INPUT, "no source cloud set");
  return NDT_OK;
}

// ---- gicp_inputs.hip
ndt_status gicp_index_cloud(ndt_context* c, const std::shared_ptr<DeviceCloud>& cloud, LeafHint& hint, GicpInput& in);
ndt_status gicp_finite_check(gicp_context* h, const std::vector<const DeviceCloud*>& clouds, std::vector<unsigned>& bad);
ndt_status gicp_read_covariances(gicp_context* h, const GicpInput& in, double* cov9);
ndt_status gicp_prepare_covariances(gicp_context* h, GicpInput& tgt, GicpInput& src);
// ---- gicp_grid.hip
// What every call that needs a voxel target starts with (after gicp_inputs_set; a cloud target: nothing to do): the map has a
// target, the main stream is ordered behind the map's by an event, D is materialised if stale (then step_ready is dropped) and
// not empty.  NDT_ERR_NO_INPUT otherwise.
ndt_status gicp_grid_ready(gicp_context* h);
// the correspondence step against the voxel target (k_correspond_voxel), the arguments of gicp::launch_correspond otherwise
hipError_t gicp_grid_correspond(gicp_context* h, int n, const float* T12, const gicp::Rot3d& R, const double* cov_src6, double dist_threshold);
// getFitnessScore against D: k_fitness's shape with the voxel search -- the bits of the fitness against a cloud of D's centroids
ndt_status gicp_grid_fitness(gicp_context* h, const float4* d_src, int n, const float* T_colmajor, double max_range, double* fitness);
// ---- gicp_register.hip
ndt_status gicp_scratch(gicp_context* h);
// Waits for the n tagged rows of sequence number `seq` that a kernel queued on `st` publishes (each arrives as 64 self-validating
// words), looking at the stream every look_every + 1 spins so that a failed launch cannot hang the caller.  false: `error` says why
bool gicp_wait_rows(hipStream_t st, unsigned long long seq, const double* const* rows, int n, unsigned long long look_every, std::string& error);
gicp::Result gicp_register(gicp_context* h, GicpInput& tgt, GicpInput& src, const float* guess_cm, ndt_status* status);
}  // namespace ndtc
