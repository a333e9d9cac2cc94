// gicp_grid.hip -- GICP against a VOXEL target: the source's per-point covariances matched to the voxel distributions of an NDT
// handle's current target grid (cloud-built in any form, accumulated, cropped, imported), found through that grid's own look-up
// table.  Scan-to-map GICP: nothing is built over the points of the map, nothing is rebuilt when the map grows.
//
// The target set D (include/gicp_mi355.h has the contract): the voxels whose table entry is a record -- what the DIRECT searches
// see; a lut_rejected entry and a voxel under min_points_per_voxel are not in it -- in ascending linear voxel index; voxel v gives
// its f32 centroid (the bits of ndt_grid_centroids) and a 3x3 f64 covariance (RAW: the inverse of the record's f64 icov; PLANE:
// I - (1 - gicp_epsilon) n n^T, n the eigenvector of icov's largest eigenvalue).
//   refresh  : table_voxels (ndt_table_voxels.hpp) over the entries that are records with VoxelEmit -- one mark + scan (dense
//              table, whose order IS the linear index order) or mark + sort by key (hash) + gather pass, the centroid cloud's --
//              writes D's centroids, covariances, linear indices and the record -> ordinal map; cached in the handle's GridTarget,
//              redone when the grid's generation has moved or the map handle holds another grid (gicp_grid_ready)
//   search   : k_correspond_voxel -- k_correspond's job and outputs.  Per query (a team of 8 lanes, wave-uniform loop) cubic
//              shells of cells through the map's table, the centroid fitness's walk (ndt_voxel_table.hpp: table_shell and
//              wave_scan_table under the policy NearestVoxel; axis_gap widened by give = index slack + the grid's excursion),
//              the best PAIR (d2, ordinal) carried, equal d2 to the lower ordinal = the lower linear index, rejected entries
//              passed over.  The driver (voxel_nearest) is this file's own.  Stops: the exact-search rule (the
//              best lies strictly inside reach - give), k_correspond's gate rule (the shells reach past the gate and nothing
//              under it has been found: -1), and after r_max shells one pass over the table by the whole wave.
//   cost rule: shell r probes up to (2r+1)^3 - (2r-1)^3 table entries; a query with nothing near walks shells until
//              r * leaf + margin - give >= gate, that is at most ceil((gate + give) / leaf) + 1 shells, (2 ceil((gate + give) / leaf) + 3)^3
//              probes -- the gate in leaves, cubed.  Scan-to-map GICP wants a gate of a few leaves.
//   algebra  : mahalanobis_store (gicp_device.hpp), shared with k_correspond; the objective kernels, the server and gicp::run
//              are used as they are, their `tgt` is D's centroid array.
//   fitness  : k_voxel_fitness -- k_fitness's loop, rows and reduction with the voxel search in it
#include "gicp_internal.hpp"

#include "gicp_device.hpp"
#include "ndt_table_voxels.hpp"

namespace gicp {

using namespace ndt;

// the voxel target as the kernels see it
struct VoxelTarget {
  CentroidIndex ci;
  const int* ord = nullptr;      // record -> ordinal in D
  const double* cov6 = nullptr;  // [|D|][6]
};

namespace {

constexpr int kNoVoxel = 0x7fffffff;

// The search policy of the voxel target (ndt_voxel_table.hpp): the entries that are records -- neither empty nor rejected --
// are candidates, the ordinal is loaded beside the centroid, and the best PAIR (distance, ordinal) is carried: the nearer, at
// equal distance the lower ordinal
struct NearestVoxel {
  struct Best {
    float d;
    int o;
  };
  using Side = int;
  const int* ord;  // record -> ordinal in D
  __device__ static Best none() { return Best{INFINITY, kNoVoxel}; }
  __device__ static bool candidate(int e) { return e >= 0; }
  __device__ static int record(int e) { return e; }
  __device__ Side side(int rec) const { return ord[rec]; }
  __device__ static void take(float d, int o, Best& best) {
    if (d < best.d || (d == best.d && o < best.o)) {
      best.d = d;
      best.o = o;
    }
  }
  __device__ static void fold(Best& best, int off) {
    const float od = __shfl_xor(best.d, off, kWave);
    const int oo = __shfl_xor(best.o, off, kWave);
    take(od, oo, best);
  }
};

// The nearest voxel of D to the query of every team of the wave: (tb, tb_o), uniform within the team; tb_o == kNoVoxel: none
// (only with a gate: nothing lies under it).  Every lane of the WAVE must call this together (a team without a query: live =
// false) -- the pass over the table is a wave-wide operation.  gate: a squared distance (f64, +inf: none).  What comes back is
// exact for every query whose nearest voxel lies under the gate; a query with nothing under the gate may come back with kNoVoxel
// or with a voxel at or beyond the gate -- the caller's own gate test sees no difference.
__device__ __forceinline__ void voxel_nearest(const VoxelTarget& vt, bool live, float qx, float qy, float qz, double gate, float& tb,
                                              int& tb_o) {
  const GridGeom& g = vt.ci.gv.g;
  const int sub = threadIdx.x & (kTeam - 1);
  const float leaf = fminf(g.leaf[0], fminf(g.leaf[1], g.leaf[2]));
  const int r_lim = max(g.div_b[0], max(g.div_b[1], g.div_b[2]));
  const int r_max = vt.ci.r_max;
  const NearestVoxel nearest{vt.ord};
  tb = INFINITY;
  tb_o = kNoVoxel;
  bool done = !live;
  if (live) {
    NearestVoxel::Best best = NearestVoxel::none();  // this lane's share of the candidates
    int cx, cy, cz;
    float margin;
    query_cell(g, qx, qy, qz, cx, cy, cz, margin);
    for (int r = 0; r <= r_max && !done; r++) {
      table_shell<kTeam>(vt.ci, nearest, cx, cy, cz, r, sub, qx, qy, qz, tb, best);  // (tb: the team's best after the previous shell)
      tb = best.d;
      tb_o = best.o;
      team_min(tb, tb_o);
      // every unvisited CELL is at least r cells away; its centroid may lie ci.give outside it.  Strictly inside the reach: a
      // voxel AT the reach could tie with a lower index
      const float reach = static_cast<float>(r) * leaf + margin - vt.ci.give;
      if ((tb_o != kNoVoxel && reach > 0.0f && tb < reach * reach) || r >= r_lim) done = true;
      // nothing closer than the gate is left once the shells reach past it: no correspondence either way
      if (reach > 0.0f && static_cast<double>(reach) * static_cast<double>(reach) >= gate && !(static_cast<double>(tb) < gate)) done = true;
    }
  }
  // the shells got dearer than the table itself: one pass over it by the wave, one unfinished query at a time
  unsigned long long open_teams = __ballot(!done && sub == 0);
  const int lane = threadIdx.x & (kWave - 1);
  while (open_teams) {
    const int src_lane = __builtin_ctzll(open_teams);
    open_teams &= open_teams - 1;
    const NearestVoxel::Best wb =
        wave_scan_table(vt.ci, nearest, __shfl(qx, src_lane, kWave), __shfl(qy, src_lane, kWave), __shfl(qz, src_lane, kWave));
    if (lane / kTeam == src_lane / kTeam) {
      tb = wb.d;
      tb_o = wb.o;
    }
  }
}

// k_correspond against a voxel target: corr[i] = the ordinal in D of the voxel nearest to T * output[i] if its squared distance
// is < dist_threshold, else -1; maha9[i] = (R C1 R^T + C2)^-1 with C2 = D's covariance of that voxel.  correspond_block's layout:
// 32 queries per pass and block, strided by the grid.
__global__ __launch_bounds__(kBlock) void k_correspond_voxel(const float4* __restrict__ output, int n, EvalParams P, Rot3d R, VoxelTarget vt,
                                                             const double* __restrict__ cov_src6, double dist_threshold,
                                                             int* __restrict__ corr, float* __restrict__ maha9) {
#pragma clang fp contract(off)
  constexpr int kTeams = kBlock / kTeam, kTeamsPerWave = kWave / kTeam;
  const int sub = threadIdx.x & (kTeam - 1);
  const int wave_in_block = threadIdx.x / kWave, team_in_wave = (threadIdx.x & (kWave - 1)) / kTeam;
  const int n_blocks = static_cast<int>(gridDim.x);
  // The loop is uniform across the WAVE (a team without a query idles): the pass over the table is a wave-wide operation.
  for (int base = (static_cast<int>(blockIdx.x) * (kBlock / kWave) + wave_in_block) * kTeamsPerWave; base < n; base += n_blocks * kTeams) {
    const int i = base + team_in_wave;
    const bool live = i < n;  // uniform within a team
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) {
      const float4 p = output[i];
      matvec_eigen(P.T, p.x, p.y, p.z, qx, qy, qz);
    }
    float tb;
    int tb_o;
    voxel_nearest(vt, live, qx, qy, qz, dist_threshold, tb, tb_o);
    if (!live || sub != 0) continue;
    int c_out = -1;
    if (tb_o != kNoVoxel && static_cast<double>(tb) < dist_threshold) {  // :436
      mahalanobis_store(cov_src6 + static_cast<size_t>(i) * 6, vt.cov6 + static_cast<size_t>(tb_o) * 6, R, maha9 + static_cast<size_t>(i) * 9);
      c_out = tb_o;
    }
    corr[i] = c_out;
  }
}

// getFitnessScore against D: fitness_body's loop (ndt_kernels.hip) -- the same dealing of the queries, the same per-lane sums,
// the same row -- with the voxel search in place of the point search.  The nearest squared distance is exact in both, so the
// row is the one k_fitness writes for a cloud of D's centroids.
__global__ __launch_bounds__(kBlock) void k_voxel_fitness(const float4* __restrict__ src, int n, EvalParams P, VoxelTarget vt, double max_range,
                                                          double* __restrict__ partials) {
  __shared__ double lds[(kBlock / kWave) * 32];
  constexpr int kTeams = kBlock / kTeam, kTeamsPerWave = kWave / kTeam;
  double acc[kNumAcc];
#pragma unroll
  for (int k = 0; k < kNumAcc; k++) acc[k] = 0.0;
  const int sub = threadIdx.x & (kTeam - 1);
  const int wave_in_block = threadIdx.x / kWave, team_in_wave = (threadIdx.x & (kWave - 1)) / kTeam;
  const int blk = static_cast<int>(blockIdx.x), nblk = static_cast<int>(gridDim.x);
  const int log_slots = 32 - __clz(max(n, 2) - 1), n_slots = 1 << log_slots;
  for (int base = (blk * (kBlock / kWave) + wave_in_block) * kTeamsPerWave; base < n_slots; base += nblk * kTeams) {
    const int i = static_cast<int>(__brev(static_cast<unsigned>(base + team_in_wave)) >> (32 - log_slots));
    float tx = 0.f, ty = 0.f, tz = 0.f;
    bool live = i < n;  // uniform within a team
    if (live) {
      const float4 pt = src[i];
      live = finite3(pt.x, pt.y, pt.z);
      if (live) {
        xform_point(P.T, pt.x, pt.y, pt.z, tx, ty, tz);
        live = finite3(tx, ty, tz);
      }
    }
    float tb;
    int tb_o;
    voxel_nearest(vt, live, tx, ty, tz, static_cast<double>(INFINITY), tb, tb_o);
    if (live && sub == 0 && static_cast<double>(tb) <= max_range) {  // the squared distance against max_range, as PCL does
      acc[0] += static_cast<double>(tb);
      acc[1] += 1.0;
    }
  }
  block_reduce_store<kNumAcc>(acc, partials + static_cast<size_t>(blockIdx.x) * kEvalStride, lds);
}

// ---- the refresh pass
// D's enumeration (ndt_table_voxels.hpp): the entries that are records ...
struct IsRecord {
  __device__ static bool pick(int e) { return e >= 0; }
};
// ... and one voxel of D to position p: centroid, linear index, covariance, and the record's ordinal.  One thread's work.
struct VoxelEmit {
  const VoxelSide* sides;
  double epsilon;
  int cov_mode;
  float4* pts;
  double* cov6;
  long long* idx;
  int* ord;
  __device__ void operator()(int rec, unsigned p, long long linear) const;
};
__device__ __forceinline__ void VoxelEmit::operator()(int rec, unsigned p, long long linear) const {
#pragma clang fp contract(off)
  const VoxelSide s = sides[rec];
  pts[p] = make_float4(s.cx, s.cy, s.cz, 1.0f);
  idx[p] = linear;
  ord[rec] = static_cast<int>(p);
  double A[3][3];  // icov: c00 c01 c02 c11 c12 c22
  A[0][0] = s.icov[0]; A[0][1] = s.icov[1]; A[0][2] = s.icov[2];
  A[1][0] = s.icov[1]; A[1][1] = s.icov[3]; A[1][2] = s.icov[4];
  A[2][0] = s.icov[2]; A[2][1] = s.icov[4]; A[2][2] = s.icov[5];
  double out[6];
  if (cov_mode == GICP_VOXEL_COV_RAW) {
    double inv[3][3];
    inv3_cofactor(A, inv);
    out[0] = inv[0][0]; out[1] = inv[0][1]; out[2] = inv[0][2]; out[3] = inv[1][1]; out[4] = inv[1][2]; out[5] = inv[2][2];
  } else {  // GICP's (1, 1, epsilon) along the voxel's normal: the eigenvector of icov's largest eigenvalue
    double w[3], V[3][3];
    eig3_jacobi(A, w, V);  // ascending eigenvalues
    const double k = 1.0 - epsilon;
    int e = 0;
    for (int a = 0; a < 3; a++)
      for (int b = a; b < 3; b++) out[e++] = (a == b ? 1.0 : 0.0) - (k * V[a][2]) * V[b][2];
  }
  for (int t = 0; t < 6; t++) cov6[static_cast<size_t>(p) * 6 + t] = out[t];
}

}  // namespace
}  // namespace gicp

namespace {

gicp::VoxelTarget voxel_view(const gicp_context* h) {
  const GridTarget& gt = h->grid_target;
  const DeviceGrid* g = gt.map->grid.get();
  gicp::VoxelTarget vt;
  vt.ci = centroid_index(g);
  vt.ord = gt.ord.p;
  vt.cov6 = gt.cov.p;
  return vt;
}

// D of `grid` into gt's arrays, on the main stream: one enumeration of the table's records (table_voxels).  Nothing waits for
// the gather: what reads D next is queued on the same stream.
ndt_status voxel_refresh(gicp_context* h, const std::shared_ptr<DeviceGrid>& grid) {
  GridTarget& gt = h->grid_target;
  DeviceGrid* g = grid.get();
  gt.valid = false;
  gt.n = 0;
  h->step_ready = false;  // (the ordinals a correspondence step wrote mean nothing in the new D)
  const double eps = h->prm.gicp_epsilon;
  HIP_TRY(gt.ord.reserve(std::max<size_t>(g->centroids.cap, 1)));
  size_t cnt = 0;
  const ndt_status s = table_voxels<gicp::IsRecord, gicp::VoxelEmit>(
      h->tgt.stream, g, true,
      [&](unsigned n, gicp::VoxelEmit& emit) -> hipError_t {
        HIP_PASS(gt.pts.reserve(n));
        HIP_PASS(gt.cov.reserve(static_cast<size_t>(n) * 6));
        HIP_PASS(gt.idx.reserve(n));
        emit = {g->view().centroids, eps, gt.cov_mode, gt.pts.p, gt.cov.p, gt.idx.p, gt.ord.p};
        return hipSuccess;
      },
      &cnt);
  if (s) return s;
  gt.n = cnt;
  gt.seen = grid;
  gt.seen_generation = g->generation;
  gt.seen_epsilon = eps;
  gt.valid = true;
  gt.refreshes++;
  return NDT_OK;
}

}  // namespace

namespace ndtc {

ndt_status gicp_grid_ready(gicp_context* h) {
  if (!h->in[0].vox) return NDT_OK;
  GridTarget& gt = h->grid_target;
  ndt_context* map = gt.map;
  if (!map->grid || !map->target) return fail(NDT_ERR_NO_INPUT, "the map handle of the grid target has no input target");
  ndt_status s = gicp_scratch(h);
  if (s) return s;
  if (map->stream) {  // behind whatever the map handle has queued (a build, an update, a crop): an event, no wait on the host
    if (!gt.ev) HIP_TRY(hipEventCreateWithFlags(&gt.ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(gt.ev, map->stream));
    HIP_TRY(hipStreamWaitEvent(h->tgt.stream, gt.ev, 0));
  }
  const std::shared_ptr<DeviceGrid> grid = map->grid;
  DeviceGrid* g = grid.get();
  const std::shared_ptr<DeviceGrid> seen = gt.seen.lock();
  const bool fresh = gt.valid && seen.get() == g && gt.seen_generation == g->generation && gt.seen_epsilon == h->prm.gicp_epsilon;
  if (!fresh) {
    if (g->empty) {  // no voxel at all: D is empty, nothing to read
      gt.valid = false;
      gt.n = 0;
      h->step_ready = false;
    } else {
      s = voxel_refresh(h, grid);
      if (s) return s;
    }
  }
  if (g->empty || gt.n == 0) return fail(NDT_ERR_NO_INPUT, "the target grid has no valid voxel");
  return ensure_excursion(&h->tgt, g);  // (cached in the grid: a launch only after the voxels have changed)
}

hipError_t gicp_grid_correspond(gicp_context* h, int n, const float* T12, const gicp::Rot3d& R, const double* cov_src6, double dist_threshold) {
  const int blocks = gicp::correspond_blocks(n, kGicpMaxBlocks);
  ndt::EvalParams P{};
  for (int i = 0; i < 12; i++) P.T[i] = T12[i];
  h->grid_target.correspond_blocks = static_cast<size_t>(blocks);
  hipLaunchKernelGGL(gicp::k_correspond_voxel, dim3(blocks), dim3(ndt::kBlock), 0, h->tgt.stream, h->output.p, n, P, R, voxel_view(h), cov_src6,
                     dist_threshold, h->corr.p, h->maha.p);
  return hipGetLastError();
}

ndt_status gicp_grid_fitness(gicp_context* h, const float4* d_src, int n, const float* T_colmajor, double max_range, double* fitness) {
  *fitness = std::numeric_limits<double>::max();  // nr == 0 in the reference
  if (n == 0) return NDT_OK;
  ndt_context* c = &h->tgt;
  ndt_status s = ensure_host_rows(c, 1);
  if (s) return s;
  ndt::EvalParams P{};
  colmajor_to_T12(T_colmajor, P.T);
  const int nblk = fitness_blocks(n);  // k_fitness's grid
  HIP_TRY(c->partials.reserve(static_cast<size_t>(nblk) * ndt::kEvalStride));
  hipLaunchKernelGGL(gicp::k_voxel_fitness, dim3(nblk), dim3(ndt::kBlock), 0, c->stream, d_src, n, P, voxel_view(h), max_range, c->partials.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(ndt::launch_reduce(c->partials.p, nblk, 1, nullptr, c->host_result, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->host_result[1] > 0) *fitness = c->host_result[0] / c->host_result[1];
  return NDT_OK;
}

}  // namespace ndtc

extern "C" {

ndt_status gicp_set_input_target_grid(gicp_handle h, ndt_handle map, int cov_mode) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  if (map) {
    if (cov_mode != GICP_VOXEL_COV_PLANE && cov_mode != GICP_VOXEL_COV_RAW) return fail(NDT_ERR_INVALID, "unknown cov_mode");
    if (map->device != h->tgt.device) return fail(NDT_ERR_INVALID, "the GICP handle and the map handle are on different devices");
  }
  // as every target setter: the target is unset, and the main stream is waited for before the old index goes
  GicpInput& in = h->in[0];
  in.set = in.have_cov = in.user_cov = false;
  in.vox = nullptr;
  h->step_ready = false;
  GridTarget& gt = h->grid_target;
  gt.map = nullptr;
  gt.valid = false;
  gt.n = 0;
  gt.seen.reset();
  if (h->tgt.device_ready) {
    HIP_TRY(hipSetDevice(h->tgt.device));
    HIP_TRY(hipStreamSynchronize(h->tgt.stream));
    tls_pool_stream = h->tgt.stream;
    in.grid.reset();
  }
  if (!map) return NDT_OK;  // the binding is dropped: the handle has no target
  gt.map = map;
  gt.cov_mode = cov_mode;
  in.vox = &gt;
  in.have_cov = true;  // (D's own: no k-NN pass ever runs over a voxel target)
  in.set = true;
  return NDT_OK;
}

ndt_status gicp_target_grid_voxels(gicp_handle h, float* xyz1, double* cov9, int64_t* idx, size_t capacity, size_t* n) {
  if (!h || !n) return fail(NDT_ERR_INVALID, "bad arguments");
  if (!h->in[0].vox) return fail(NDT_ERR_NO_INPUT, "the target is not a grid target");
  *n = 0;
  ndt_status s = gicp_grid_ready(h);
  if (s) return s;
  const GridTarget& gt = h->grid_target;
  const size_t count = gt.n;
  *n = count;
  if (!xyz1 && !cov9 && !idx) return NDT_OK;
  if (capacity < count) return fail(NDT_ERR_INVALID, "capacity is smaller than the target's voxel set (*n holds its size)");
  hipStream_t st = h->tgt.stream;
  std::vector<double> c6(cov9 ? count * 6 : 0);
  static_assert(sizeof(long long) == sizeof(int64_t), "linear indices are 64-bit");
  StreamDrain drain{st};
  if (xyz1) HIP_TRY(hipMemcpyAsync(xyz1, gt.pts.p, count * sizeof(float4), hipMemcpyDeviceToHost, st));
  if (cov9) HIP_TRY(hipMemcpyAsync(c6.data(), gt.cov.p, count * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (idx) HIP_TRY(hipMemcpyAsync(idx, gt.idx.p, count * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  drain.done = true;
  for (size_t i = 0; cov9 && i < count; i++) {
    const double* s6 = c6.data() + i * 6;
    double* o = cov9 + i * 9;
    o[0] = s6[0]; o[1] = s6[1]; o[2] = s6[2];
    o[3] = s6[1]; o[4] = s6[3]; o[5] = s6[4];
    o[6] = s6[2]; o[7] = s6[4]; o[8] = s6[5];
  }
  return NDT_OK;
}

ndt_status gicp_diag_target_grid(gicp_handle h, size_t* refreshes, size_t* voxels, float* excursion, size_t* correspond_blocks) {
  if (!h) return fail(NDT_ERR_INVALID, "null");
  const GridTarget& gt = h->grid_target;
  if (refreshes) *refreshes = gt.refreshes;
  if (voxels) *voxels = gt.n;
  if (excursion) {
    const DeviceGrid* g = (gt.map && gt.valid) ? gt.map->grid.get() : nullptr;
    *excursion = (g && g->excursion_known) ? g->excursion : 0.f;
  }
  if (correspond_blocks) *correspond_blocks = gt.correspond_blocks;
  return NDT_OK;
}

}  // extern "C"
