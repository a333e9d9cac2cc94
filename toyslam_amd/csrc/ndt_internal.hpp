// ndt_internal.hpp -- state shared by the translation units behind the C-ABI (include/ndt_mi355.h,
// include/gicp_mi355.h): error reporting, the caching device allocator, device clouds / grids, the handle
// itself, and the helpers one unit offers the others.  Not installed; nothing here crosses the C-ABI.
//   ndt_handle.hip : handle lifetime, parameters, results, profiling switches, host-only scalar exports, ndt_warm_up
//   ndt_clouds.hip : cloud upload and download, bounding boxes, spatial ordering, the ndt_cloud handles, the source setters
//   ndt_grid.hip   : the cell chain and the sparse index every cell-sorting caller shares, K1 target grid build, counts and
//                    search index of a built grid, the target setters, grid inspection
//   ndt_filter.hip : N1 voxel filter of one cloud (ndt_filter_batch.hip: of many)      ndt_map_batch.hip : N2 map accumulation
//   ndt_fitness.hip : getFitnessScore      ndt_centroid_fitness.hip : the same against the voxel centroids, the centroid cloud
//   ndt_score.hip : calculateScore (of a cloud, of the source under many poses)
//   ndt_nvtl.hip  : nearest-voxel transformation likelihood (of a cloud, of the source under one or many poses, per point)
//   ndt_select.hip : selection of the points of resident clouds (finite, box, range, per-point value): kernels and C-ABI
//   ndt_deskew.hip : motion compensation of resident scans by the time of every point: kernel and C-ABI
//   ndt_normals.hip: surface normals and curvature of resident clouds (k-nearest / radius neighbourhoods): kernels and C-ABI
//   ndt_cloud_ops.hip : what ndt_select / _deskew / _outliers / _plane.hip share on the host: the checks of an input cloud and
//                    the parts of the entry preambles, the member table, output slices, the box-row fold, per-point doubles
//   ndt_pose_cov.hip: 6x6 pose covariance (Laplace / sandwich) of the handle's pair and of the pairs of a pairs call
//   ndt_eval.hip   : one evaluation (launch path), the persistent evaluation server's host side (mailbox protocol),
//                    ndt_align, ndt_eval*, diagnostics and self-tests
//   ndt_batch.hip  : lock-step batches (ndt_align_batch*, ndt_align_guesses, ndt_align_multistart), the RCCL communicator
//                    (ndt_comm_*), ndt_set_allreduce
//   ndt_accumulate.hip : the accumulating target (ndt_target_accumulate*): kernels and C-ABI
//   ndt_io.hip     : PCD files, numbered scan sequences, PointCloud2-style repacking (host)
//   gicp_capi.hip, gicp_inputs.hip, gicp_register.hip, gicp_batch.hip, gicp_grid.hip (gicp_internal.hpp, private to them) : the GICP
//                    row -- handle, parameters, results / inputs and covariances / one registration / many in one call / a voxel
//                    target (an NDT handle's grid: its refresh pass, the correspondence kernel, the fitness)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>
#include <cfloat>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <set>
#include <mutex>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "gicp_driver.hpp"
#include "gicp_kernels.hpp"
#include "gicp_mi355.h"
#include "ndt_driver.hpp"
#include "ndt_kernels.hpp"
#include "ndt_pcd.hpp"
#include "ndt_sequence.hpp"
#include "ndt_mi355.h"

namespace ndtc {

extern thread_local std::string g_last_error;

inline ndt_status fail(ndt_status s, const std::string& msg) {
  g_last_error = msg;
  return s;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return fail(NDT_ERR_HIP, std::string(#expr) + " failed: " + hipGetErrorString(_e));          \
  } while (0)
#define HIP_PASS(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)  // where hipError_t is returned

// Caching device allocator: setInputTarget / setInputSource run once per scan in the nodes, and a
// dozen hipMalloc/hipFree pairs per call (~100 us each) would dominate the GPU time of the grid
// build.  Freed blocks go to a free list keyed by (device, STREAM, rounded size class) and are reused
// only by work queued on the same stream: a block may be released while the kernels that use it are
// still in flight (the grid build does not wait for the GPU), and stream order is what makes the
// next user safe.  The calling thread's current stream is set by every API entry (ensure_device).
// The cache is trimmed (hipFree, which synchronises) when it exceeds kPoolTrimBytes.
extern thread_local hipStream_t tls_pool_stream;

class DevPool {
 public:
  static DevPool& instance() {
    static DevPool p;
    return p;
  }
  static size_t size_class(size_t bytes) {
    if (bytes < 512) return 512;
    size_t p2 = 512;
    while (p2 * 2 <= bytes) p2 *= 2;
    const size_t step = p2 / 8;
    return (bytes + step - 1) / step * step;
  }
  using Key = std::tuple<int, hipStream_t, size_t>;
  hipError_t alloc(size_t bytes, void** out, size_t* got) {
    const size_t cls = size_class(bytes);
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
      std::lock_guard<std::mutex> g(m_);
      auto it = free_.find(Key(dev, tls_pool_stream, cls));
      if (it != free_.end()) {
        *out = it->second;
        *got = cls;
        cached_ -= cls;
        free_.erase(it);
        return hipSuccess;
      }
    }
    hipError_t e = hipMalloc(out, cls);
    if (e != hipSuccess) {  // retry once with an empty cache
      trim(0);
      e = hipMalloc(out, cls);
    }
    *got = cls;
    return e;
  }
  void release(void* p, size_t cls) {
    if (!p) return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    bool over = false;
    {
      std::lock_guard<std::mutex> g(m_);
      free_.insert(std::make_pair(Key(dev, tls_pool_stream, cls), p));
      cached_ += cls;
      over = cached_ > kPoolTrimBytes;
    }
    if (over) trim(kPoolTrimBytes / 2);
  }
  // Streams that have been destroyed (forget_stream) and not created again since (adopt_stream: a new stream may get an old
  // one's handle value): an ndt_cloud that outlives a handle it was made or read on must neither wait for such a stream nor
  // give its memory to that stream's pool.
  void adopt_stream(hipStream_t st) {
    std::lock_guard<std::mutex> g(m_);
    retired_.erase(st);
  }
  bool retired(hipStream_t st) {
    std::lock_guard<std::mutex> g(m_);
    return retired_.count(st) != 0;
  }
  // blocks cached for a stream that is about to be destroyed: give them back
  void forget_stream(hipStream_t st) {
    std::lock_guard<std::mutex> g(m_);
    retired_.insert(st);
    for (auto it = free_.begin(); it != free_.end();) {
      if (std::get<1>(it->first) == st) {
        (void)hipFree(it->second);
        cached_ -= std::get<2>(it->first);
        it = free_.erase(it);
      } else {
        ++it;
      }
    }
  }
  void trim(size_t keep) {
    std::lock_guard<std::mutex> g(m_);
    for (auto it = free_.begin(); it != free_.end() && cached_ > keep;) {
      (void)hipFree(it->second);
      cached_ -= std::get<2>(it->first);
      it = free_.erase(it);
    }
  }

 private:
  static constexpr size_t kPoolTrimBytes = size_t(16) << 30;
  std::mutex m_;
  std::multimap<Key, void*> free_;
  std::set<hipStream_t> retired_;
  size_t cached_ = 0;
};

// grow-only device buffer on top of the pool
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;        // elements the caller may use
  size_t cls_bytes = 0;  // pool size class actually held
  ~DevBuf() { release(); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  void release() {
    if (p && cls_bytes) DevPool::instance().release(p, cls_bytes);  // (cls_bytes == 0: borrowed memory, not ours to free)
    p = nullptr;
    cap = 0;
    cls_bytes = 0;
  }
  // refer to n elements of memory somebody else owns and keeps alive (clouds handed over by reference)
  void borrow(T* ptr, size_t n) {
    release();
    p = ptr;
    cap = n;
    cls_bytes = 0;
  }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    std::swap(cls_bytes, o.cls_bytes);
  }
  hipError_t reserve(size_t n) {
    if (n <= cap && p && cls_bytes) return hipSuccess;
    release();
    void* q = nullptr;
    size_t got = 0;
    hipError_t e = DevPool::instance().alloc(std::max<size_t>(n, 1) * sizeof(T), &q, &got);
    if (e == hipSuccess) {
      p = static_cast<T*>(q);
      cls_bytes = got;
      cap = got / sizeof(T);
    }
    return e;
  }
};

struct DeviceCloud {
  DevBuf<float4> pts;     // caller's order (align's output cloud keeps it)
  DevBuf<float4> sorted;  // lattice-cell order, what the derivative kernels read
  size_t n = 0;
  // bounding boxes computed during the upload (k_repack_bbox): [0] over the non-NaN points (the
  // is_dense rule of getMinMax3D), [1] over the finite points (!is_dense); min > max = no such point
  float bb_min[2][3] = {{FLT_MAX, FLT_MAX, FLT_MAX}, {FLT_MAX, FLT_MAX, FLT_MAX}};
  float bb_max[2][3] = {{-FLT_MAX, -FLT_MAX, -FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}};
  int box_route = NDT_BOX_ROUTE_NONE;  // which producer wrote the boxes (ndt_box_route; set where the boxes are set)
  size_t n_sorted = 0;    // finite points only
  std::vector<size_t> scan_counts;  // batch uploads: finite points of each scan ...
  std::vector<size_t> scan_starts;  // ... and where its ordered segment starts in `sorted`
  const float4* k2_pts() const { return n_sorted ? sorted.p : pts.p; }
  int k2_n() const { return static_cast<int>(n_sorted ? n_sorted : n); }
  // An ndt_cloud (a cloud the caller holds as an object and hands to several consumers): the stream it was made on -- its
  // memory goes back to THAT stream's pool, whichever thread or handle drops the last reference -- and the other streams
  // it has been read on (waited for before the memory is given back).  Null for the handles' own uploads.
  int device = -1;
  hipStream_t made_on = nullptr;
  std::vector<hipStream_t> used_on;
  std::shared_ptr<DeviceCloud> parent;  // a view of another cloud's points (pts borrowed) with an ordered copy of its own
  // A slice of a batched filter's output block (ndt_filter_batch.hip; pts borrowed): keeps the block alive.  Not `parent`:
  // the slice is a cloud of its own (ndt_promote_source_to_target promotes it, not the block).  The streams that read a
  // slice are waited for when the slice goes, so the block's memory goes back only after every reader of every slice.
  std::shared_ptr<DeviceCloud> owner;
  ~DeviceCloud() {
    if (!made_on) return;
    (void)hipSetDevice(device);
    DevPool& pool = DevPool::instance();
    for (hipStream_t s : used_on)
      if (s != made_on && !pool.retired(s)) (void)hipStreamSynchronize(s);  // (a destroyed stream's work is over: its handle waited)
    const hipStream_t keep = tls_pool_stream;
    if (pool.retired(made_on)) {  // the handle that made it is gone: to the default pool, behind a device-wide wait
      (void)hipDeviceSynchronize();
      tls_pool_stream = nullptr;
    } else {
      tls_pool_stream = made_on;
    }
    pts.release();
    sorted.release();
    tls_pool_stream = keep;
  }
};


// An enqueued voxel filter: where its count and the rows of its result's boxes arrive (page-locked), what the host decided
static constexpr int kOutBoxBlocks = 64;
struct FilterPending {
  float* rows = nullptr;     // [64][12] per-block rows of the result's bounding boxes
  unsigned* tot = nullptr;   // [3]: points binned, voxels, -
  size_t n_max = 0, fixed_n = 0;
  bool from_device = false;  // the count is tot[1] (else fixed_n: empty input, or the input copied through)
  bool overflow = false;
};

// Immutable once built (shared between cloned handles).
struct DeviceGrid {
  ndt::GridGeom geom{};
  float resolution = 0;
  int min_pts = 6;
  double eig_ratio = 0.01;
  bool empty = true;
  size_t n_leaves = 0, n_cand = 0, n_valid = 0;
  std::shared_ptr<DeviceCloud> target;  // kept for the dump pass
  DevBuf<int> lut;
  DevBuf<ndt::VoxelRec> recs;
  DevBuf<ndt::VoxelSide> centroids;  // per record: voxel centroid (KDTREE search) + f64 inverse covariance
  DevBuf<int> leaf_cell, leaf_count, leaf_rec, sorted_idx;
  DevBuf<unsigned> leaf_start;
  size_t n_sorted = 0;  // target points that landed in a voxel (finite ones)
  DevBuf<unsigned> counts;      // device copy of {n_sorted, n_leaves, n_cand, n_valid}
  bool counts_known = true;     // host copies above are current (grid_counts() fetches them lazily)
  // getFitnessScore's nearest-neighbour search: cell -> leaf ordinal (or -1), built on first use
  std::mutex fit_mu;
  DevBuf<uint2> cell_range;  // per cell: its segment of cell_pts (count 0 = empty)
  DevBuf<float4> cell_pts;  // the target points in cell order (ndt_search.hpp scans them)
  DevBuf<int> row_any;      // per x-row of cells: occupied or not
  bool have_cell2leaf = false;
  // bucket-form build: records still numbered the way k1_finalize numbers them (slot = segment start / min_pts: gaps,
  // bucket by bucket); maybe_compact_records makes them dense and cell-ordered once the grid is seen to be reused
  bool compact_pending = false;
  int n_registrations = 0;
  int build_form = 0;  // what built it (ndt_diag_grid_build): 0 nothing (empty, accumulated), 1 dense chain, 2 buckets, 3 one launch, 4 sparse
  // bucket-form build (ndt_kernels.hip): kept until the leaf arrays have been written (grid_counts)
  bool leaves_pending = false;
  ndt::GridBuildPlan plan{};
  DevBuf<float4> bpts;
  bool index_form = false;  // (NDT_K1_INDEX=1: bpts holds point indices)
  // the grid of an accumulating target (ndt_accumulate.hip): lut / recs / centroids / geom only, mutated in place by its one
  // handle; no points, no leaf arrays -- what needs either (getFitnessScore, sharing) refuses it
  bool accumulated = false;
  DevBuf<unsigned> bucket_base;
  // the centroid fitness (ndt_centroid_fitness.hip): how far any centroid of the grid lies outside its own cell's box, computed
  // on first use (under fit_mu); an accumulated target marks it stale wherever its voxels change (commit, crop)
  bool excursion_known = false;
  float excursion = 0.f;
  size_t n_centroids = 0;  // voxels of the centroid cloud, counted by the same pass
  // what a reader that caches arrays derived from the table and the records (GICP's voxel target, gicp_grid.hip) compares:
  // moved wherever the voxels change (touched() -- every place the excursion goes stale) or the records are renumbered
  unsigned long long generation = 0;
  void touched() {
    excursion_known = false;
    generation++;
  }
  ndt::GridView view() const {
    ndt::GridView v;
    v.lut = lut.p;
    v.recs = recs.p;
    v.centroids = centroids.p;
    v.g = geom;
    return v;
  }
};


}  // namespace ndtc
using namespace ndtc;

// the C-ABI's ndt_cloud
struct ndt_cloud_s {
  std::shared_ptr<DeviceCloud> c;
};

struct ndt_context;
namespace ndtc {
void comm_release(ndt_context* h);  // ndt_batch.hip
struct AccTarget;                   // ndt_accumulate.hip
}

struct ndt_context {
  int device = 0;
  bool device_ready = false;
  hipStream_t stream = nullptr;
  bool stream_masked[3] = {false, false, false};
  hipStream_t partition_stream[3] = {nullptr, nullptr, nullptr};  // the streams this handle has had, by CU partition (ndt_set_cu_partition switches, nothing is destroyed before the handle is)
  // parameters (ctor defaults ndt_omp_impl.hpp:47-76, voxel_grid_covariance_omp.h:208-223)
  float resolution = 1.0f;
  double step_size = 0.1, outlier_ratio = 0.55, trans_eps = 0.1;
  int max_iter = 35, search = NDT_DIRECT7, num_threads = 1, min_pts = 6;
  double eig_ratio = 0.01;
  // inputs
  std::shared_ptr<DeviceCloud> target, source;
  int target_dense = 1;
  std::shared_ptr<DeviceGrid> grid;
  // scratch
  DevBuf<double> partials;
  DevBuf<unsigned> ticket;  // zero between launches (reset by the last block of the fused kernel)
  DevBuf<double> batch_out;
  DevBuf<ndt::ScanDesc> descs;
  void* batch_pinned = nullptr;  // pinned staging: [n_scans] ScanDesc + [3 n_scans] int
  size_t batch_pinned_bytes = 0;
  DevBuf<float4> out_cloud;
  void* out_pinned = nullptr;  // page-locked staging of the aligned cloud on its way to the caller
  float4* server_out_host = nullptr;  // set by ndt_align before the server starts: the server writes the cloud there too
  bool server_wrote_host = false;
  size_t out_pinned_bytes = 0;
  DevBuf<unsigned char> staging;
  double* host_result = nullptr;  // pinned, kEvalStride doubles (+ batch rows)
  float* bbox_rows = nullptr;     // pinned, per-block bounding-box rows of the last upload (k_repack_bbox)
  unsigned long long* bbox_tagged = nullptr;  // pinned: the same rows as self-validating words, polled (clouds by reference)
  unsigned bbox_tag = 0;
  // small host clouds (the mapping nodes' 16 k-point scans): repacked to float4 and bounded ON THE HOST into one of these
  // page-locked slots and DMA'd from there -- no repack kernel, no wait for the device (upload_cloud)
  static constexpr int kStageSlots = 4;
  static constexpr size_t kStageSlotPoints = 65536;
  float* stage_host[kStageSlots] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t stage_done[kStageSlots] = {nullptr, nullptr, nullptr, nullptr};  // the slot's last DMA has been read
  int stage_next = 0;
  double* host_pub = nullptr;     // pinned, tagged publication row of the single-scan paths (ndt_kernels.hip publish_row_tagged)
  size_t host_result_rows = 0;
  unsigned long long eval_seq = 0;
  double t_launch = 0, t_wait = 0, t_solver = 0, t_fill = 0, t_gap = 0;  // NDT_TIMING=1 accounting (seconds; t_gap: NDT_TIMING=2)
  // results
  float final_T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  int converged = 0, nr_iterations = 0;
  double trans_probability = 0;
  int n_evals = 0, n_hess = 0;
  double mean_neighbors = 0;
  size_t out_n = 0;
  // persistent evaluation server (single-scan align)
  bool server_running = false;
  int server_blocks = 0;  // grid of the running server: min(16, blocks) part rows come back per evaluation
  // N2: accumulated global map (dense float4, HBM resident)
  DevBuf<float4> map_pts;   // the map, with room behind it: the next scan is transformed straight into its tail
  DevBuf<float4> map_alt;   // where the next filter pass writes (the two swap roles)
  size_t map_n = 0;
  int map_dense = 1;
  DeviceCloud map_boxes;    // bounding boxes of the map as the last filter pass left it (bb_min / bb_max only)
  bool map_boxes_known = false;
  // The map lives on a stream of its own: an update is queued there and NOT waited for -- the next registration does not
  // read the map -- until somebody needs the map or its size (map_complete): the next update, ndt_map_size / _get.
  hipStream_t map_stream = nullptr;
  hipEvent_t map_ready = nullptr;       // recorded on the handle's stream: the scan the update reads is complete
  bool map_pending = false;
  FilterPending map_filter;
  std::vector<std::shared_ptr<DeviceCloud>> map_scans;  // the scans a queued update reads (kept until the update has been waited for)
  float* filter_slots = nullptr;        // page-locked: [3] x (64 x 12 rows + count words): slot 0 N1, slot 1 the map, slot 2 a begun N1
  // ndt_cloud_voxel_filter_begin / _end: one prefilter queued on a stream of its own (beside a registration on the handle's)
  hipStream_t filter_stream = nullptr;
  bool n1_pending = false;
  FilterPending n1_filter;
  std::shared_ptr<DeviceCloud> n1_in, n1_out;
  int voxel_index = 0;              // ndt_set_voxel_index: 0 automatic, 1 dense table, 2 sparse (sorted build + hash look-up)
  int persistent = -1;  // -1 = default (NDT_PERSISTENT / on), 0 = launch per evaluation, 1 = server
  // ndt_set_evaluation_reuse: -1 = default (NDT_EVAL_REUSE / on), 0 = every evaluation is asked of the device, 1 = a solver
  // answers a repeated request itself (ScanSolver, SolverParams::reuse_evaluations); and, for ndt_diag_eval_reuse, the
  // evaluations the last align / batch call was served by the device and the steps its solvers fed themselves
  int eval_reuse = -1;
  long long reuse_served = 0, reuse_reused = 0;
  // Two command mailboxes, used by alternate server instances: a server told to finish (transform +
  // exit) is not waited for, and the next instance's first command must not overwrite the line the
  // old one may still be reading.
  void* server_host_mbs = nullptr;  // 2 command mailboxes the host writes: host-visible device memory (large BAR) or pinned host memory
  bool server_mbs_on_device = false;
  void* server_host_mb = nullptr;   // the running (or next) instance's mailbox
  int server_flip = 0;
  DevBuf<unsigned char> server_dev_mb;
  DevBuf<unsigned> server_counter;  // two sets of kServerCounterWords, used alternately (server_start)
  int server_counter_set = 0;
  DevBuf<unsigned long long> server_dbg;  // diagnostics only (ndt_diag_server_roundtrip)
  bool server_want_dbg = false;
  int cu_count = 0;      // CUs this handle's stream may use (its partition's)
  int cu_total = 0;      // CUs of the device
  int cu_partition = 0;  // ndt_set_cu_partition: 0 whole device, 1 registration partition, 2 side partition
  // live kernel timing (HIP events on `stream`)
  bool profiling = false;       // mode 1: one launch per evaluation, an event pair around each
  bool profile_server = false;  // mode 2: the persistent kernel of each registration between one event pair
  bool server_timed = false;
  hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr, ev_d = nullptr;
  static constexpr int kProfSlots = 7;  // 0-2 evaluation kinds / lock-step kernels, 3 server launch, 4-6 exchange step (ndt_mi355.h)
  long long prof_n[kProfSlots] = {0, 0, 0, 0, 0, 0, 0};
  double prof_ms[kProfSlots] = {0, 0, 0, 0, 0, 0, 0};
  // collective hook
  ndt_allreduce_fn allreduce = nullptr;
  void* allreduce_user = nullptr;
  int allreduce_on_device = 0;
  // native RCCL communicator (ndt_comm_*, ndt_batch.hip): sharded lock-step batches, point-sharded scans
  void* comm = nullptr;  // ncclComm_t
  int comm_rank = 0, comm_world = 1;
  long long comm_collectives = 0;
  int batch_lock_steps = 0;  // lock-steps of the last ndt_align_batch*
  int batch_groups = 1;      // independent lock-step groups the last batch ran as
  bool is_batch_worker = false;
  int batch_groups_wanted = 0;  // ndt_set_batch_groups: 0 = automatic
  std::vector<ndt_context*> batch_workers;  // worker handles of those groups (own stream and staging each; grid shared)
  // ndt_align_pairs*: the grid of every cloud the last pairs call used as a target (null for the others), and the per-member
  // GridView table its lock-step kernels read (ndt_pairs.hip)
  std::vector<std::shared_ptr<DeviceGrid>> pairs_grids;
  // ... and, for ndt_pairs_fitness_scores, every pair's source (caller's point order), its target's grid and its final
  // transformation (column-major, 16 per pair); empty after a failed or empty pairs call
  std::vector<std::shared_ptr<DeviceCloud>> pairs_sources;
  std::vector<std::shared_ptr<DeviceGrid>> pairs_targets;
  std::vector<float> pairs_T;
  // the last many-member getFitnessScore (fitness_many): its launches and the blocks of the largest one (partial rows
  // held at once), for ndt_diag_fitness_launches
  size_t fit_launches = 0, fit_max_blocks = 0;
  DevBuf<ndt::GridView> pair_views;
  // ndt_cloud_voxel_filter_batch / _clouds (ndt_filter_batch.hip): page-locked descriptors and read-backs, the result rows
  // of the clouds that take the single-cloud route, and what the last call did (ndt_diag_filter_batch)
  void* fb_pinned = nullptr;
  size_t fb_pinned_bytes = 0;
  void* fb_rows = nullptr;
  size_t fb_rows_bytes = 0;
  size_t fb_passes = 0, fb_single = 0, fb_launches = 0;
  // ndt_map_update_clouds / _batch (ndt_map_batch.hip): the page-locked scan descriptors of the one transform launch, and what
  // the last call did (ndt_diag_map_batch)
  void* mb_pinned = nullptr;
  size_t mb_pinned_bytes = 0;
  size_t mb_transform_launches = 0, mb_filters = 0, mb_box_passes = 0;
  // ndt_score_poses (ndt_score.hip): the pose table of one chunk (12 row-major floats per pose) in page-locked memory and in
  // HBM, and what the last call did (ndt_diag_score_poses)
  void* sp_pinned = nullptr;
  size_t sp_pinned_bytes = 0;
  DevBuf<float> sp_poses;
  size_t sp_launches = 0, sp_blocks = 0;
  // the nearest-voxel likelihood calls (ndt_nvtl.hip): the pose table of one chunk as above, L of every source point of the
  // last ndt_source_point_nvtl (what its d_out names), and what the last call that reached the device did (ndt_diag_nvtl)
  void* nv_pinned = nullptr;
  size_t nv_pinned_bytes = 0;
  DevBuf<float> nv_poses;
  DevBuf<double> nv_points;
  size_t nv_launches = 0, nv_blocks = 0;
  // the pose covariance calls (ndt_pose_cov.hip): k_grad_outer / k_grad_outer_multi launches and blocks of the last one
  // that reached the device (ndt_diag_pose_covariance)
  size_t pc_launches = 0, pc_blocks = 0;
  // ndt_target_accumulate* (ndt_accumulate.hip): the accumulated target -- alive while `grid` is its grid -- and what the last
  // call did (ndt_diag_target_accumulate)
  std::shared_ptr<ndtc::AccTarget> acc;
  size_t acc_touched = 0, acc_new = 0, acc_launches = 0;
  int acc_relinked = 0, acc_grown = 0;
  // ... and the last ndt_target_accumulate_crop (ndt_diag_target_crop)
  size_t crop_kept = 0, crop_removed = 0, crop_points = 0, crop_launches = 0;
  int crop_relinked = 0;
  // ... and the last ndt_target_accumulate_clear_rays* / _ray_counts that reached the device (ndt_diag_target_clear_rays)
  size_t ray_cast = 0, ray_skipped = 0, ray_touched = 0, ray_removed = 0, ray_kept = 0, ray_points = 0, ray_launches = 0;
  unsigned long long ray_visited = 0;
  int ray_relinked = 0;
  // ... and the last ndt_target_accumulate_export / _save (ndt_diag_target_export)
  size_t exp_voxels = 0, exp_points = 0, exp_launches = 0;
  // the last centroid fitness call (ndt_diag_centroid_fitness): launches queued, excursion passes among them, the excursion it
  // searched with, the blocks of its largest launch
  size_t cf_launches = 0, cf_passes = 0, cf_max_blocks = 0;
  float cf_excursion = 0.f;
  // the selections (ndt_select.hip): the page-locked block of a call -- its segment table on the way up, its totals and box
  // rows on the way back -- and what the last call that reached the device did (ndt_diag_select)
  void* sel_pinned = nullptr;
  size_t sel_pinned_bytes = 0;
  size_t sel_launches = 0, sel_blocks = 0, sel_clouds = 0;
  // the outlier filters (ndt_outliers.hip): what the last call that reached the device did (ndt_diag_outliers)
  size_t ol_index_builds = 0, ol_value_launches = 0, ol_value_blocks = 0, ol_scanned = 0;
  // the plane of a cloud (ndt_plane.hip): what the last call that reached the device did (ndt_diag_plane)
  size_t pl_launches = 0, pl_select_launches = 0, pl_count_blocks = 0, pl_clouds = 0;
  // the cluster extraction (ndt_clusters.hip): what the last call that reached the device did (ndt_diag_clusters)
  size_t cl_index_builds = 0, cl_launches = 0, cl_link_blocks = 0, cl_scanned = 0, cl_cas_retries = 0;
  // the normals (ndt_normals.hip): what the last call that reached the device did (ndt_diag_normals)
  size_t nr_index_builds = 0, nr_launches = 0, nr_blocks = 0, nr_scanned = 0;
  // the motion compensation (ndt_deskew.hip): the page-locked block of a call -- its segment table on the way up, its per-block
  // rows (boxes, untimed count) on the way back -- and what the last call that reached the device did (ndt_diag_deskew)
  void* dsk_pinned = nullptr;
  size_t dsk_pinned_bytes = 0;
  size_t dsk_launches = 0, dsk_blocks = 0, dsk_clouds = 0;

  ~ndt_context() {
    for (ndt_context* w : batch_workers) delete w;
    batch_workers.clear();
    ndtc::comm_release(this);
    if (stream) {  // nothing of this handle may still be running when its buffers go back to the pool
      (void)hipSetDevice(device);
      (void)hipStreamSynchronize(stream);
      tls_pool_stream = stream;
    }
    if (map_stream) {  // the map's buffers belong to the map stream's pool
      (void)hipStreamSynchronize(map_stream);
      const hipStream_t keep = tls_pool_stream;
      tls_pool_stream = map_stream;
      map_pts.release();
      map_alt.release();
      tls_pool_stream = keep;
      DevPool::instance().forget_stream(map_stream);
      (void)hipStreamDestroy(map_stream);
      if (map_ready) (void)hipEventDestroy(map_ready);
    }
    if (filter_stream) {
      (void)hipStreamSynchronize(filter_stream);
      n1_in.reset();
      n1_out.reset();
      DevPool::instance().forget_stream(filter_stream);
      (void)hipStreamDestroy(filter_stream);
    }
    if (filter_slots) (void)hipHostFree(filter_slots);
    if (fb_pinned) (void)hipHostFree(fb_pinned);
    if (fb_rows) (void)hipHostFree(fb_rows);
    if (mb_pinned) (void)hipHostFree(mb_pinned);
    if (sp_pinned) (void)hipHostFree(sp_pinned);
    if (nv_pinned) (void)hipHostFree(nv_pinned);
    if (sel_pinned) (void)hipHostFree(sel_pinned);
    if (dsk_pinned) (void)hipHostFree(dsk_pinned);
    acc.reset();
    release_buffers();
    if (host_result) (void)hipHostFree(host_result);
    if (host_pub) (void)hipHostFree(host_pub);
    if (out_pinned) (void)hipHostFree(out_pinned);
    if (bbox_rows) (void)hipHostFree(bbox_rows);
    if (bbox_tagged) (void)hipHostFree(bbox_tagged);
    for (int k = 0; k < kStageSlots; k++) {
      if (stage_host[k]) (void)hipHostFree(stage_host[k]);
      if (stage_done[k]) (void)hipEventDestroy(stage_done[k]);
    }
    if (server_host_mbs) (void)(server_mbs_on_device ? hipFree(server_host_mbs) : hipHostFree(server_host_mbs));
    if (batch_pinned) (void)hipHostFree(batch_pinned);
    if (ev_a) (void)hipEventDestroy(ev_a);
    if (ev_b) (void)hipEventDestroy(ev_b);
    if (ev_c) (void)hipEventDestroy(ev_c);
    if (ev_d) (void)hipEventDestroy(ev_d);
    for (hipStream_t& ps : partition_stream) {
      if (ps && ps != stream) {
        DevPool::instance().forget_stream(ps);
        (void)hipStreamDestroy(ps);
      }
      ps = nullptr;
    }
    if (stream) {
      DevPool::instance().forget_stream(stream);
      (void)hipStreamDestroy(stream);
    }
    tls_pool_stream = nullptr;
  }
  void release_buffers();
};

namespace ndt { struct CentroidIndex; }  // ndt_voxel_table.hpp

namespace ndtc {
// ---- ndt_handle.hip
int usable_devices();
int side_cus();
ndt_status ensure_device(ndt_context* h);
ndt_status ensure_host_rows(ndt_context* h, size_t rows);
ndt::SolverParams solver_params(const ndt_context* h);
// may this handle's solvers reuse evaluations now?  Off where the number of evaluations is itself observed: event pairs per
// evaluation (ndt_profile_enable(h, 1)) and the exchange modes, whose legs count a collective per evaluation.
bool eval_reuse_now(const ndt_context* h);
// page-locked scratch of a handle, grown on demand; `reader`: the stream whose queued copies may still read the old block
// (waited for before it is freed).  Rewriting the block is the caller's to order: only behind a wait for what reads it
ndt_status pinned_at_least(void*& p, size_t& have, size_t bytes, hipStream_t reader);
struct PoolStreamGuard {  // temporaries allocated (and given back) inside the scope belong to `s`'s pool
  hipStream_t keep;
  explicit PoolStreamGuard(hipStream_t s) : keep(tls_pool_stream) { tls_pool_stream = s; }
  ~PoolStreamGuard() { tls_pool_stream = keep; }
};
// ---- ndt_clouds.hip
ndt_status upload_cloud(ndt_context* h, const void* pts, size_t n, size_t stride, bool on_device,
                        std::shared_ptr<DeviceCloud>& out, bool by_reference = false);
struct BBox {
  float mn[3], mx[3];
};
BBox bbox_of(const DeviceCloud& c, int dense);
ndt_status bbox_compute(ndt_context* h, const float4* d_pts, int n, int dense, BBox& out);
ndt_status order_range(ndt_context* h, const float4* d_pts, size_t n, float pitch, float4* d_out, size_t* n_out,
                       const BBox* known_bbox = nullptr);
ndt_status order_batch(ndt_context* h, DeviceCloud* c, const size_t* offsets, size_t n_scans);
ndt_status order_cloud(ndt_context* h, DeviceCloud* c, const size_t* offsets, size_t n_scans);
ndt_status download_records(ndt_context* h, const float4* d_src, size_t n, void* out, size_t out_stride);
ndt_status out_block_at_least(ndt_context* h, size_t bytes);  // h->out_pinned, page-locked: grown behind a wait for h->stream
void spread_records(const void* src, size_t n, void* out, size_t out_stride);  // n float4 records into records of out_stride bytes
ndt_status cloud_use_on(ndt_handle h, DeviceCloud* c);  // an ndt_cloud made on another stream: wait for it, remember the reader
// ---- ndt_grid.hip
// The general cell chain sorts points by cell.  The caller counts into per-cell counters (launch_count, _count_batch or
// _count_multi: key and rank per point); chain_scan (scan_reduce, scan_blocks, scan_apply) turns them into start offsets and
// numbers the occupied cells (the leaves; leaf_rec: the record of those with min_pts), the totals {points, leaves,
// candidates} staying on the device at `totals`; chain_scan_scatter also writes the points' indices in cell order.
struct ChainOut { int* leaf_cell; unsigned* leaf_start; int *leaf_count, *leaf_rec, *sorted_idx; };
struct ChainBufs {  // the five arrays, owned: sized for the worst case, since the leaf count stays on the device
  DevBuf<int> leaf_cell, leaf_count, leaf_rec, sorted_idx;
  DevBuf<unsigned> leaf_start;
  hipError_t reserve(size_t max_leaves, size_t n_points) {
    for (hipError_t e : {leaf_cell.reserve(max_leaves), leaf_start.reserve(max_leaves), leaf_count.reserve(max_leaves), leaf_rec.reserve(max_leaves), sorted_idx.reserve(n_points)})
      if (e != hipSuccess) return e;
    return hipSuccess;
  }
  ChainOut out() const { return ChainOut{leaf_cell.p, leaf_start.p, leaf_count.p, leaf_rec.p, sorted_idx.p}; }
};
ndt_status chain_scan(hipStream_t st, unsigned* counters, long long n_cells, int min_pts, const ChainOut& o, unsigned* totals);
ndt_status chain_scan_scatter(hipStream_t st, unsigned* counters, long long n_cells, int min_pts, const int* key, const unsigned* rank,
                              int n, const ChainOut& o, unsigned* totals);
// the same five arrays by sorting (cell, point) pairs (ndt_sparse.hip): per-point work only, the cell space is never walked
ndt_status sparse_index(hipStream_t st, const float4* pts, int n, int dense, const ndt::GridGeom& geo, int min_pts, const ChainOut& o,
                        unsigned* counts);
// What a voxel grid is built with, apart from the cloud: a handle's settings (grid_spec_of) or a caller's own (GICP's point
// index: index_only -- cells and their point lists, no per-voxel statistics)
struct GridSpec {
  float resolution;
  int min_pts;
  double eig_ratio;
  int voxel_index;  // ndt_set_voxel_index
  bool dense;       // the cloud holds no NaN / inf
  bool index_only;
};
inline GridSpec grid_spec_of(const ndt_context* h, int is_dense) {
  return GridSpec{h->resolution, h->min_pts, h->eig_ratio, h->voxel_index, is_dense != 0, false};
}
// VoxelGridCovariance::filter(true) of `cloud` on the GPU, into `out`; h: the stream, the pool, the scratch.  `out` is
// assigned when the build has queued its last launch, and with the empty grid of a cloud without a finite point or of the
// reference's index overflow (NDT_ERR_GRID_OVERFLOW); any other failure leaves it alone.
ndt_status build_grid(ndt_context* h, const std::shared_ptr<DeviceCloud>& cloud, const GridSpec& spec, std::shared_ptr<DeviceGrid>& out);
// grids of many targets (ndt_align_pairs): every one the small form takes from ONE k1_small_multi launch, the others through
// build_grid; out[i] = the grid of targets[i], bit for bit what build_grid makes of it.  *n_small: how many took the launch
ndt_status build_grids(ndt_context* h, const std::vector<std::shared_ptr<DeviceCloud>>& targets, int is_dense,
                       std::vector<std::shared_ptr<DeviceGrid>>& out, size_t* n_small);
// the inspection of a built grid g (ndt_grid_size / _info / _dump of the handle's, ndt_pairs_grid_* of a pairs call's)
ndt_status grid_size(ndt_context* h, DeviceGrid* g, size_t* n_leaves, size_t* n_valid);
void grid_info(const DeviceGrid* g, int* min_b, int* max_b, int* div_b);
ndt_status grid_dump(ndt_context* h, DeviceGrid* g, int64_t* idx, int* nr_points, double* mean, double* cov, double* icov, double* evals);
ndt_status maybe_compact_records(ndt_context* h, bool eager);
ndt_status grid_counts(ndt_context* h, DeviceGrid* g);
ndt_status ensure_cell2leaf(ndt_context* h, DeviceGrid* g);
ndt_status ensure_indices(ndt_context* h, const std::vector<DeviceGrid*>& grids);  // both of the above for many grids, two waits in all
float index_slack(const DeviceGrid* g);
void fill_point_index(const DeviceGrid* g, ndt::PointIndex& ix);
// ---- ndt_fitness.hip
ndt_status fitness_impl(ndt_context* h, const float4* d_src, int n, const float* T_colmajor, double max_range, double* fitness);
// the same against a grid the caller names instead of h->grid (GICP: the target input's index)
ndt_status fitness_against(ndt_context* h, DeviceGrid* g, const float4* d_src, int n, const float* T_colmajor, double max_range,
                           double* fitness);
// getFitnessScore of many (source, target grid, transform) members: the source's n points at src, moved by the column-major T,
// against g's point index.  out[k] is what fitness_impl returns for member k on a handle holding that grid (ndt_fitness.hip)
struct FitnessJob {
  const DeviceGrid* g = nullptr;
  const float4* src = nullptr;
  size_t n = 0;
  const float* T = nullptr;  // column-major 4x4
};
ndt_status fitness_many(ndt_context* h, const std::vector<FitnessJob>& jobs, double max_range, double* out);
// blocks of getFitnessScore over n source points (k_fitness's grid, a member's blocks of k_fitness_multi): 32 query teams per
// block, at most 2048 blocks (the teams then stride over the queries)
inline int fitness_blocks(int n) { return std::max(1, std::min(2048, (n + 31) / 32)); }
// ---- ndt_centroid_fitness.hip
long long table_entries(const DeviceGrid* g);    // entries one pass over g's look-up table reads (dense cells, or hash slots)
int centroid_shell_limit(const DeviceGrid* g);   // shells a centroid search walks before the one pass over the table
// g's centroid excursion, computed on h's stream when unknown or stale (one launch, one read-back, waited for)
ndt_status ensure_excursion(ndt_context* h, DeviceGrid* g);
// g's table as the centroid searches walk it: view, table_entries, index_slack + excursion (ensure_excursion first), shell limit
ndt::CentroidIndex centroid_index(const DeviceGrid* g);
// ---- ndt_score.hip
// poses per launch of ndt_score_poses and ndt_nvtl_poses: one rule, one switch (NDT_SCORE_POSES_CHUNK)
size_t poses_chunk(size_t n_poses, size_t row_bytes);
// ---- ndt_nvtl.hip
// the readiness every NVTL call shares, after its own argument checks: a device, then a target (and a source)
ndt_status nvtl_ready(ndt_context* h, bool need_source);
// NVTL of the n device points at d_pts, moved by the column-major T first (null: used as given).  d_out (may be null): n
// doubles of device memory that receive L per point, -1.0 where the point has no neighbour.  Waits for the stream.
ndt_status nvtl_launch(ndt_context* h, const float4* d_pts, size_t n, const float* T_colmajor, double* d_out, double* nvtl,
                       size_t* n_found);
// ---- ndt_select.hip
// One cloud of a selection: n records at `in` (keys: n device doubles, or null), kept records to `out` (room for n), their
// indices to `idx` (device, room for n; or null).  key_range (device, two doubles, or null): this cloud's own key_lo / key_hi
// in place of the spec's.  Results: kept, and the boxes / route of the kept points in `res`.
struct SelJob {
  const float4* in = nullptr;
  size_t n = 0;
  const double* keys = nullptr;
  const double* key_range = nullptr;
  float4* out = nullptr;
  int* idx = nullptr;
  size_t kept = 0;
  DeviceCloud* res = nullptr;  // n, bb_min / bb_max, box_route are set
};
// the two launches over all jobs and the call's one wait (idx_host: page-locked or null, the indices of jobs[0])
ndt_status select_run(ndt_handle h, std::vector<SelJob>& jobs, const ndt_select_spec& spec, int* idx_host);
// one cloud's records into a new cloud
ndt_status select_one(ndt_handle h, const float4* d_in, size_t n, const ndt_select_spec& spec, const double* d_keys,
                      std::shared_ptr<DeviceCloud>& out, int32_t* kept_idx, size_t* n_kept, const double* d_key_range = nullptr);
// ---- ndt_cloud_ops.hip: what the operations on resident clouds share (ndt_select / _deskew / _outliers / _plane.hip)
std::shared_ptr<DeviceCloud> new_cloud(ndt_handle h);  // an ndt_cloud's DeviceCloud made on h's stream
ndt_status cloud_checks(ndt_handle h, ndt_cloud c);    // what every operation refuses of an input cloud
// a spec (a motion) the caller hands over: there, and valid by its own rule (error_of: null = valid, else what is wrong)
template <class Spec>
ndt_status spec_checks(const Spec* spec, const char* (*error_of)(const Spec&), const char* if_null = "null spec") {
  if (!spec) return fail(NDT_ERR_INVALID, if_null);
  if (const char* why = error_of(*spec)) return fail(NDT_ERR_INVALID, why);
  return NDT_OK;
}
// The preamble of an entry over ONE cloud, behind the entry's own argument checks: the cloud; own() -- the entry's checks of
// its spec and what goes with it, run only for a cloud that passed; the device; the cloud's stream.
template <class Own>
ndt_status cloud_entry(ndt_handle h, ndt_cloud in, Own&& own) {
  ndt_status s = cloud_checks(h, in);
  if (!s) s = own();
  if (!s) s = ensure_device(h);
  if (!s) s = cloud_use_on(h, in->c.get());
  return s;
}
// The preamble of an entry over a LIST of clouds, in two steps with the entry's own refusals (a missing list, the spec)
// between them.  clouds_begin: at most 65535 clouds, then every output nulled (out_b: the plane's second kind).
// clouds_total: per cloud k cloud_checks and each(k); first[k] = the points before cloud k, first[n_clouds] = the total,
// refused beyond INT_MAX.
ndt_status clouds_begin(size_t n_clouds, ndt_cloud* out_a, ndt_cloud* out_b = nullptr);
template <class Each>
ndt_status clouds_total(ndt_handle h, const ndt_cloud* in, size_t n_clouds, std::vector<size_t>& first, Each&& each) {
  first.assign(n_clouds + 1, 0);
  for (size_t k = 0; k < n_clouds; k++) {
    ndt_status s = cloud_checks(h, in[k]);
    if (!s) s = each(k);
    if (s) return s;
    first[k + 1] = first[k] + in[k]->c->n;
  }
  if (first[n_clouds] > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  return NDT_OK;
}
inline ndt_status clouds_total(ndt_handle h, const ndt_cloud* in, size_t n_clouds, std::vector<size_t>& first) {
  return clouds_total(h, in, n_clouds, first, [](size_t) { return NDT_OK; });
}
// whatever path leaves the scope: nothing queued may still read or write what the scope's buffers give back to the pool, and
// the queued copies have read (written) the call's host memory before it dies.  done: set by a path that has waited itself
struct Drain {
  hipStream_t s;
  bool done = false;
  ~Drain() {
    if (!done) (void)hipStreamSynchronize(s);
  }
};
// ndt_diag_select reports on the selections alone: what the compaction inside an outlier or a plane call did is taken back
struct SelDiagKeep {
  ndt_handle h;
  size_t a, b, c;
  explicit SelDiagKeep(ndt_handle hh) : h(hh), a(hh->sel_launches), b(hh->sel_blocks), c(hh->sel_clouds) {}
  ~SelDiagKeep() {
    h->sel_launches = a;
    h->sel_blocks = b;
    h->sel_clouds = c;
  }
};
// The member table of a launch: the host's entries and a device copy made only when there are several -- a call of one
// member hands entry 0 over as a kernel argument.  upload(st, src): src = a page-locked copy of the entries, else theirs.
template <class M>
struct MemberTable {
  std::vector<M> host;
  DevBuf<unsigned char> dev;
  int n() const { return static_cast<int>(host.size()); }
  size_t bytes() const { return host.size() * sizeof(M); }
  const M& one() const { return host[0]; }
  const M* table() const { return reinterpret_cast<const M*>(dev.p); }
  ndt_status upload(hipStream_t st, const void* src = nullptr) {
    if (host.size() < 2) return NDT_OK;
    HIP_TRY(dev.reserve(bytes()));
    HIP_TRY(hipMemcpyAsync(dev.p, src ? src : host.data(), bytes(), hipMemcpyHostToDevice, st));
    return NDT_OK;
  }
};
// per-block box rows (12 floats at the head of every `stride` floats) of blocks [b0, b0 + nb) folded into c's boxes; the route set
void fold_box_rows(DeviceCloud* c, const float* rows, size_t stride, int b0, int nb, int route);
// The outputs of a call over a list of clouds: slices of ONE block with room for every input point, kept alive by the slices'
// `owner`.  reserve (first: clouds_total's) before anything is queued; publish(k, count) once nothing can fail any more.
struct OutSlices {
  std::shared_ptr<DeviceCloud> blk;
  std::vector<std::shared_ptr<DeviceCloud>> res;
  std::vector<size_t> first;
  ndt_status reserve(ndt_handle h, const std::vector<size_t>& first_points);
  float4* at(size_t k) const { return blk->pts.p + first[k]; }
  DeviceCloud* cloud(size_t k) const { return res[k].get(); }  // what the job of cloud k writes n, the boxes and the route to
  ndt_cloud publish(size_t k, size_t count);
};
// n per-point doubles on their way in (keys, times): *d = the caller's device pointer as it is, or a copy of the host's
// queued on st and held by buf
ndt_status doubles_in(hipStream_t st, const double* src, size_t n, int on_device, DevBuf<double>& buf, const double** d);
// ... and on their way out (neighbour values, plane distances): at() is where the kernels write -- the caller's device
// memory, or a buffer reserve() made that fetch() queues the copy of to the caller's host memory
struct DoublesOut {
  DevBuf<double> buf;
  double* dst = nullptr;
  size_t n = 0;
  bool on_device = false;
  ndt_status reserve(double* dst_, size_t n_, int on_device_);
  double* at() const { return on_device ? dst : buf.p; }
  ndt_status fetch(hipStream_t st);
};
// a development switch that lowers a plan's block cap: the environment variable's value where it is > 0, at most cap
int env_block_cap(const char* name, int cap);
// ---- gicp_inputs.hip
// A point index (index_only grid) over `cloud` whose leaf follows the cloud's own density: leaf0 > 0 is tried first, else a
// volume guess, then corrected from the measured points per occupied cell.  dense: the cloud holds no NaN / inf.  *leaf_out:
// the leaf it ended with.  Search results never depend on the leaf, only the time does.
ndt_status index_cloud_by_density(ndt_context* c, const std::shared_ptr<DeviceCloud>& cloud, bool dense, float leaf0, float* leaf_out,
                                  std::shared_ptr<DeviceGrid>& grid);
// ... with a leaf of about `want` (the outlier filter's radius), clamped into the same cell budget; one build
float index_leaf_clamped(const DeviceCloud& cloud, double want);
// ---- ndt_filter.hip
ndt_status filter_slots(ndt_handle h, int which, FilterPending& P);
// The geometry and route of one N1 filter, from the cloud's box alone -- the one decision voxel_filter_enqueue and the
// batched filter (ndt_filter_batch.hip) both take: no finite point, PCL's index overflow (copy-through), the sparse index
// (ndt_set_voxel_index, or a box far larger than the points), or a dense cell space over the box (geo)
struct FilterRoute {
  enum Kind { kEmpty, kOverflow, kSparse, kDense } kind = kEmpty;
  ndt::GridGeom geo{};
};
FilterRoute filter_route(const ndt_context* h, size_t n, const BBox& bb, float leaf);
// a dense filter of n points over n_cells cells: on the bucket front end of the grid build (plan filled in), or the general chain
bool filter_takes_buckets(long long n_cells, long long n, ndt::GridBuildPlan& plan);
ndt_status voxel_filter_enqueue(ndt_handle h, hipStream_t st, const float4* d_in, size_t n, int is_dense, float leaf, float4* d_out,
                                const BBox& bb, FilterPending& P);
void voxel_filter_finish(const FilterPending& P, size_t* n_out, DeviceCloud* boxes);
// out_boxes: the result's bounding boxes as DeviceCloud keeps them ([2][3] min, [2][3] max), or null
ndt_status voxel_filter_device(ndt_handle h, const float4* d_in, size_t n, int is_dense, float leaf, float4* d_out,
                               size_t* n_out, bool* overflow, const BBox* known_bbox = nullptr, DeviceCloud* out_boxes = nullptr);
// ---- ndt_map_batch.hip
// N2 of a list of resident scans in one pass (the single ndt_map_update* are the list of one): scan k moved by its pose
// (16 column-major floats, null = identity) behind the map, in the list's order, then one filter of the concatenation
struct MapScan {
  std::shared_ptr<DeviceCloud> c;
  int dense = 1;
  const float* pose = nullptr;
};
struct MapBatchDiag {
  size_t transform_launches = 0, filters = 0, box_passes = 0;
};
ndt_status map_update_scans(ndt_handle h, const std::vector<MapScan>& scans, float leaf, int* overflowed, MapBatchDiag* diag);
// the map's stream exists and a queued update has been waited for: map_n, the boxes and h->mb_pinned are the handle's again
ndt_status map_settle(ndt_handle h);
ndt_status map_complete(ndt_handle h);  // ... the wait alone (ndt_warm_up: no stream is made for a handle that has no map)
// ---- ndt_accumulate.hip
bool acc_is_live(const ndt_context* h);  // the handle's target is an accumulated one
void acc_drop(ndt_context* h);           // forget it (the handle is left without a target if it was live)
ndt_status acc_grid_counts(ndt_context* h, DeviceGrid* g);
ndt_status acc_grid_dump(ndt_context* h, int64_t* idx, int* nr_points, double* mean, double* cov, double* icov, double* evals);
// ---- ndt_eval.hip
void colmajor_to_T12(const float* m, float* T12);
float kd_radius2(float resolution);
void fill_eval_params(const ndt::EvalRequest& rq, const ndt::Gauss& gs, float kd_r2, ndt::EvalParams& P);
void fill_h64_params(const ndt::EvalRequest& rq, const ndt::Gauss& gs, float kd_r2, ndt::Hess64Params& P);
void unpack_row(const double* row, bool have_h, ndt::EvalResult& r, double* nn);
ndt_status check_ready(ndt_context* h);
ndt_status evaluate_single(ndt_context* h, const ndt::EvalRequest& rq, ndt::EvalResult& res, double* nn_total);
ndt_status server_stop(ndt_context* h);
ndt_status server_start(ndt_context* h);
void server_finish(ndt_context* h, const float* T_colmajor);
ndt_status server_evaluate(ndt_context* h, const ndt::EvalRequest& rq, const ndt::Gauss& gs, ndt::EvalResult& res,
                           double* nn_total, bool* served);
bool server_enabled();
// ---- ndt_batch.hip
// The members of one lock-step loop: where each local member's source points lie and, for ndt_align_pairs*, which grid it is
// evaluated against (views == null: the handle's grid for every member, the map-build batch)
struct LockStepMembers {
  const float4* pts = nullptr;     // the ordered (or raw) concatenated sources
  std::vector<int> offset, count;  // per local member: its segment of pts
  std::vector<size_t> n_raw;       // per local member: its points as the caller gave them (transformation_probability's N)
  const ndt::GridView* views = nullptr;  // per local member (host copy; uploaded by lock_step)
  const char* empty = nullptr;           // per local member: its grid has no voxel (its rows are zero, nothing is launched)
};
ndt_status lock_step(ndt_context* h, const LockStepMembers& m, size_t n_local, const float* guesses, float* final_T, int* conv,
                     int* iters, double* tprob, size_t first = 0, size_t total = 0);
// what ndt_score_poses, ndt_align_guesses and ndt_align_multistart refuse before any device work: a null handle, a null
// table with entries, a handle with a communicator or an all-reduce hook
ndt_status many_poses_checks(const ndt_context* h, const void* table, size_t n, const void* out, const char* what);
size_t batch_group_count(const ndt_context* h, size_t n_members);
// runs run(worker, lo, hi) for member ranges [lo, hi) of n_members, one worker handle and host thread per group (grid and
// parameters of h copied), and gathers the workers' statistics into h; pts_of(lo, hi): the points of those members
ndt_status run_groups(ndt_context* h, size_t n_members, size_t groups, const std::function<double(size_t, size_t)>& pts_of,
                      const std::function<ndt_status(ndt_context*, size_t, size_t)>& run);
ndt_status comm_allreduce(ndt_context* h, double* d_buf, size_t n_doubles);
void server_mark(ndt_context* h, bool running);

// tagged publication row (ndt_kernels.hip publish_row_tagged): 64 words, each (half of a value << 32) |
// low 32 bits of the sequence number; complete when every word carries the tag
inline bool pub_ready(const double* pub, unsigned long long seq) {
  const volatile unsigned long long* w = reinterpret_cast<const volatile unsigned long long*>(pub);
  const unsigned tag = static_cast<unsigned>(seq);
  for (int i = ndt::kPublishSlots - 1; i >= 0; i--)
    if (static_cast<unsigned>(w[i]) != tag) return false;
  return true;
}
inline void pub_gather(const double* pub, double* row) {
  std::atomic_thread_fence(std::memory_order_acquire);
  const unsigned long long* w = reinterpret_cast<const unsigned long long*>(pub);
  for (int k = 0; k < ndt::kEvalStride; k++) {
    const unsigned long long bits = (w[2 * k] >> 32) | ((w[2 * k + 1] >> 32) << 32);
    std::memcpy(&row[k], &bits, sizeof(double));
  }
}
}  // namespace ndtc
