// ndt_centroid_fitness.hip -- getFitnessScore against the target's CENTROID cloud, and that cloud as an output.
//
// The centroid cloud C of a target: one point per voxel that reached min_points_per_voxel (a voxel rejected afterwards is in
// it, trap 7), the voxel's VoxelSide centroid, in ascending linear voxel index -- the reference's voxel_centroids_.  An
// accumulated target keeps no points but keeps C, so this is the fitness a scan-to-map loop can ask for.
//
// Everything here goes by the target's LOOK-UP TABLE (the padded dense table, or the open-addressing hash keyed by the linear
// index): it holds an entry -- record r, or lut_rejected(r) -- for exactly the voxels of C, in a cloud target and in an
// accumulated one alike.  So neither record-numbering trap is met: a slot of an accumulated target that is still under min_pts
// has no entry (its VoxelSide is not valid), and the gaps a bucket-form build leaves between its records until they are
// compacted have none either.  No per-map index is built; nothing is rebuilt when the map changes.
//   search   : k_centroid_fitness_multi -- per query cubic shells of cells through the table, a candidate per occupied entry
//              (centroids[r]); a team of 8 lanes for shells 0..2, the whole wave for the far queries, queries dealt in
//              bit-reversed order, a row per block (block_reduce_store), then k_fitness_reduce: k_fitness's shape.  The walk
//              of a shell and the pass over the table are ndt_voxel_table.hpp's (table_shell, wave_scan_table) under the policy
//              NearestCentroid; which shells the team walks, when the wave takes over and the stopping rule are this kernel's
//   excursion: the table is keyed by the cell the POINTS fell into; the centroid is an f32 running sum over the count and, far
//              from the origin, drifts out of that cell (by cells, not ulps).  The stopping rule and the pruning of rows and
//              cells give way by the grid's excursion -- the largest per-axis distance by which a centroid lies outside its
//              cell's box (k_centroid_excursion: one pass over the table, atomicMax of an order-preserving code), cached per
//              grid, stale after every change of an accumulated target
//   cost rule: shells 0..r probe up to (2r+1)^3 entries one scattered load each; one pass over the table reads `entries`
//              words coalesced.  Shells are walked while (2r+1)^3 <= entries / 4 (but at least kKnnMinRing shells, at most
//              the grid's extent); a query still open then takes ONE scan of the table by its whole wave (centroid_shell_limit)
//   gather   : ndt_grid_centroids* -- table_voxels (ndt_table_voxels.hpp) over the occupied entries with CentroidEmit; dense:
//              mark + exclusive scan + gather over the padded table, whose order IS the linear index order; sparse: the
//              occupied hash slots sorted by key, then gathered; one read-back of the count
// None of these calls touches the handle's target, source, grid, last result or statistics.
#include "ndt_acc.hpp"
#include "ndt_table_voxels.hpp"

namespace ndt {

struct CentroidMember {
  const float4* src = nullptr;  // caller's order
  int n = 0;
  float T[12];  // row-major 3x4 f32
};

namespace {

// The search policy of the centroid fitness (ndt_voxel_table.hpp): every occupied entry is a candidate -- a rejected voxel's
// centroid is in C -- and the squared distance alone is carried, by fminf (a NaN centroid never wins)
struct NearestCentroid {
  using Best = float;
  struct Side {};
  __device__ static Best none() { return INFINITY; }
  __device__ static bool candidate(int e) { return e != kLutEmpty; }
  __device__ static int record(int e) { return entry_record(e); }
  __device__ Side side(int) const { return Side{}; }
  __device__ static void take(float d, Side, Best& best) { best = fminf(best, d); }
  __device__ static void fold(Best& best, int off) { best = fminf(best, __shfl_xor(best, off, kWave)); }
};

// Many members against ONE centroid index in one launch: member m owns blocks [starts[m], starts[m + 1]) and block b's row is
// partials[b] (k_fitness_multi's layout: k_fitness_reduce sums it).  acc[0] = sum of the accepted squared distances, acc[1] =
// their count.  The loop is uniform across the wave (a team without a query idles): the far stage is a wave-wide operation.
__global__ __launch_bounds__(kBlock) void k_centroid_fitness_multi(const CentroidMember* __restrict__ members, const int* __restrict__ starts,
                                                                   int n_members, CentroidIndex ci, double max_range,
                                                                   double* __restrict__ partials) {
  __shared__ double lds[(kBlock / kWave) * 32];
  const int b = blockIdx.x;
  const int lo = member_at(n_members, b, [&](int m) { return starts[m]; });
  const int first = starts[lo], nblk = starts[lo + 1] - first, blk = b - first;
  const CentroidMember& M = members[lo];
  const float4* __restrict__ src = M.src;
  const int n = M.n;
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = M.T[k];

  constexpr int kTeams = kBlock / kTeam;
  constexpr int kTeamsPerWave = kWave / kTeam;
  constexpr int kTeamShells = 2;  // shells 0 .. 2 by the query's team, the rest by the wave (k_fitness's hand-off)
  double acc[2] = {0.0, 0.0};
  const GridGeom& g = ci.gv.g;
  const int sub = threadIdx.x & (kTeam - 1);
  const float leaf = fminf(g.leaf[0], fminf(g.leaf[1], g.leaf[2]));
  const int r_lim = max(g.div_b[0], max(g.div_b[1], g.div_b[2]));
  const int r_max = ci.r_max;
  const NearestCentroid nearest;
  const int wave_in_block = threadIdx.x / kWave, team_in_wave = (threadIdx.x & (kWave - 1)) / kTeam;
  const int lane = threadIdx.x & (kWave - 1);
  // queries dealt to the teams in BIT-REVERSED order: the far queries of a scan come in runs (see k_fitness)
  const int log_slots = 32 - __clz(max(n, 2) - 1), n_slots = 1 << log_slots;
  for (int base = (blk * (kBlock / kWave) + wave_in_block) * kTeamsPerWave; base < n_slots; base += nblk * kTeams) {
    const int i = static_cast<int>(__brev(static_cast<unsigned>(base + team_in_wave)) >> (32 - log_slots));
    float tx = 0.f, ty = 0.f, tz = 0.f;
    bool live = i < n;  // uniform within a team
    if (live) {
      const float4 pt = src[i];
      live = finite3(pt.x, pt.y, pt.z);
      if (live) {
        xform_point(T, pt.x, pt.y, pt.z, tx, ty, tz);
        live = finite3(tx, ty, tz);
      }
    }
    float tb = INFINITY;
    bool done = !live;
    int cx = 0, cy = 0, cz = 0;
    float margin = 0.0f;
    if (live) {
      float best = INFINITY;  // this lane's share of the candidates
      query_cell(g, tx, ty, tz, cx, cy, cz, margin);
      for (int r = 0; r <= min(r_max, kTeamShells) && !done; r++) {
        table_shell<kTeam>(ci, nearest, cx, cy, cz, r, sub, tx, ty, tz, tb, best);  // (tb: the team's best after the previous shell)
        tb = best;
#pragma unroll
        for (int off = 1; off < kTeam; off <<= 1) tb = fminf(tb, __shfl_xor(tb, off, kWave));
        // every unvisited CELL is at least r cells away; its centroid may lie ci.give outside it
        const float reach = static_cast<float>(r) * leaf + margin - ci.give;
        if ((reach > 0.0f && tb <= reach * reach) || r >= r_lim) done = true;
      }
    }
    unsigned long long open_teams = __ballot(!done && sub == 0);
    while (open_teams) {  // the far queries by the WHOLE wave, one at a time
      const int src_lane = __builtin_ctzll(open_teams);
      open_teams &= open_teams - 1;
      const float qx = __shfl(tx, src_lane, kWave), qy = __shfl(ty, src_lane, kWave), qz = __shfl(tz, src_lane, kWave);
      const int qi = __shfl(cx, src_lane, kWave), qj = __shfl(cy, src_lane, kWave), qk = __shfl(cz, src_lane, kWave);
      const float q_margin = __shfl(margin, src_lane, kWave);
      float wb = __shfl(tb, src_lane, kWave);  // what the team has found so far bounds the search
      float wbest = INFINITY;
      bool wdone = false;
      for (int r = kTeamShells + 1; r <= r_max && !wdone; r++) {
        table_shell<kWave>(ci, nearest, qi, qj, qk, r, lane, qx, qy, qz, wb, wbest);
        float m = wbest;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) m = fminf(m, __shfl_xor(m, off, kWave));
        wb = fminf(wb, m);
        const float reach = static_cast<float>(r) * leaf + q_margin - ci.give;
        if ((reach > 0.0f && wb <= reach * reach) || r >= r_lim) wdone = true;
      }
      if (!wdone) wb = wave_scan_table(ci, nearest, qx, qy, qz);  // the shells got dearer than the table itself: one pass over it
      if (lane / kTeam == src_lane / kTeam) tb = wb;
    }
    if (live && sub == 0 && static_cast<double>(tb) <= max_range) {  // the squared distance against max_range, as PCL does
      acc[0] += static_cast<double>(tb);
      acc[1] += 1.0;
    }
  }
  block_reduce_store<2>(acc, partials + static_cast<size_t>(b) * kEvalStride, lds);
}

// how far a centroid lies outside the box of the cell its entry stands for, per axis (axis_gap's box: float(cell) * leaf, + leaf)
__device__ __forceinline__ float centroid_outside(const GridView& gv, long long t, int e) {
  int x, y, z;
  table_cell(gv, t, x, y, z);
  const float4 c = *reinterpret_cast<const float4*>(gv.centroids + entry_record(e));
  const GridGeom& g = gv.g;
  return fmaxf(fmaxf(axis_gap(c.x, x + g.min_b[0], g.leaf[0], 0.0f), axis_gap(c.y, y + g.min_b[1], g.leaf[1], 0.0f)),
               axis_gap(c.z, z + g.min_b[2], g.leaf[2], 0.0f));
}
// out[0]: atomicMax of the order-preserving code of the excursion (pre-set to acc_encode(0)); out[1]: the voxels of C
__global__ __launch_bounds__(kBlock) void k_centroid_excursion(GridView gv, long long entries, int* __restrict__ out) {
  float worst = 0.0f;
  int n = 0;
  for (long long t = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; t < entries; t += static_cast<long long>(gridDim.x) * kBlock) {
    const int e = table_entry(gv, t);
    if (e == kLutEmpty) continue;
    n++;
    const float v = centroid_outside(gv, t, e);
    worst = v > worst ? v : worst;  // (a NaN centroid never raises it; INFINITY does)
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    worst = fmaxf(worst, __shfl_xor(worst, off, kWave));
    n += __shfl_xor(n, off, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && n) {
    atomicMax(out, acc_encode(worst));
    atomicAdd(out + 1, n);
  }
}

// ---- the centroid cloud (ndt_table_voxels.hpp): every occupied entry, its centroid and / or linear index to its position
struct Occupied {
  __device__ static bool pick(int e) { return e != kLutEmpty; }
};
struct CentroidEmit {
  const VoxelSide* centroids;
  float4* out;     // or null
  long long* idx;  // or null
  __device__ void operator()(int rec, unsigned p, long long linear) const {
    const float4 c = *reinterpret_cast<const float4*>(centroids + rec);
    if (out) out[p] = make_float4(c.x, c.y, c.z, 1.0f);
    if (idx) idx[p] = linear;
  }
};


}  // namespace
}  // namespace ndt

namespace ndtc {

long long table_entries(const DeviceGrid* g) { return g->geom.hash_bits ? (1ll << g->geom.hash_bits) : g->geom.lut_cells; }

// Shells walked before a query takes the one pass over the table: while (2r+1)^3 <= entries / 4, at least kKnnMinRing, at most
// the grid's extent (beyond which a shell holds no cell)
int centroid_shell_limit(const DeviceGrid* g) {
  const int r_lim = std::max(g->geom.div_b[0], std::max(g->geom.div_b[1], g->geom.div_b[2]));
  const long long budget = table_entries(g) / 4;
  int r = 0;
  while (r < r_lim && static_cast<long long>(2 * r + 3) * (2 * r + 3) * (2 * r + 3) <= budget) r++;
  return std::min(r_lim, std::max(ndt::kKnnMinRing, r));
}

// g's table as the centroid searches walk it (its excursion known: ensure_excursion)
ndt::CentroidIndex centroid_index(const DeviceGrid* g) {
  ndt::CentroidIndex ci;
  ci.gv = g->view();
  ci.entries = table_entries(g);
  ci.give = index_slack(g) + g->excursion;
  ci.r_max = centroid_shell_limit(g);
  return ci;
}

// the grid's excursion, computed when unknown or stale: one launch and one read-back
ndt_status ensure_excursion(ndt_context* h, DeviceGrid* g) {
  std::lock_guard<std::mutex> lock(g->fit_mu);
  if (g->excursion_known) return NDT_OK;
  DevBuf<int> d_out;
  HIP_TRY(d_out.reserve(2));
  HIP_TRY(hipMemsetAsync(d_out.p, 0, 2 * sizeof(int), h->stream));  // (acc_encode(0.0f) == 0)
  const long long entries = table_entries(g);
  hipLaunchKernelGGL(ndt::k_centroid_excursion, ndt::table_grid(entries), dim3(ndt::kBlock), 0, h->stream, g->view(), entries, d_out.p);
  HIP_TRY(hipGetLastError());
  int out[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(out, d_out.p, sizeof(out), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  g->excursion = ndt::acc_decode(out[0]);
  g->n_centroids = static_cast<size_t>(out[1]);
  g->excursion_known = true;
  h->cf_launches++;
  h->cf_passes++;
  return NDT_OK;
}

namespace {

struct CentroidJob {
  const float4* src = nullptr;
  size_t n = 0;
  const float* T = nullptr;  // column-major 4x4
};

// the centroid fitness of every job against g: out[k] = mean of the accepted squared distances, DBL_MAX where there is none
ndt_status centroid_fitness_many(ndt_context* h, DeviceGrid* g, const std::vector<CentroidJob>& jobs, double max_range, double* out) {
  for (size_t k = 0; k < jobs.size(); k++) out[k] = std::numeric_limits<double>::max();  // nr == 0 in the reference
  h->cf_launches = h->cf_passes = h->cf_max_blocks = 0;
  h->cf_excursion = 0.f;
  if (g->empty) return NDT_OK;  // no voxel: C is empty
  std::vector<ndt::CentroidMember> mem;
  std::vector<size_t> of;  // member -> job
  std::vector<int> starts;
  long long blocks = 0;
  for (size_t k = 0; k < jobs.size(); k++) {
    if (jobs[k].n == 0) continue;
    ndt::CentroidMember m;
    m.src = jobs[k].src;
    m.n = static_cast<int>(jobs[k].n);
    colmajor_to_T12(jobs[k].T, m.T);
    mem.push_back(m);
    of.push_back(k);
    starts.push_back(static_cast<int>(blocks));
    blocks += fitness_blocks(m.n);  // k_fitness's plan: 32 query teams per block, at most 2048 blocks a member
    if (blocks > std::numeric_limits<int>::max()) return fail(NDT_ERR_INVALID, "too many points in one centroid fitness call");
  }
  if (mem.empty()) return NDT_OK;
  starts.push_back(static_cast<int>(blocks));
  ndt_status s = ensure_excursion(h, g);
  if (s) return s;
  h->cf_excursion = g->excursion;
  if (g->n_centroids == 0) return NDT_OK;  // every voxel under min_pts: C is empty, whatever max_range is
  const size_t n_mem = mem.size();
  s = ensure_host_rows(h, (2 * n_mem + ndt::kEvalStride - 1) / ndt::kEvalStride);
  if (s) return s;
  const ndt::CentroidIndex ci = centroid_index(g);
  DevBuf<ndt::CentroidMember> d_mem;
  DevBuf<int> d_starts;
  HIP_TRY(d_mem.reserve(n_mem));
  HIP_TRY(d_starts.reserve(starts.size()));
  HIP_TRY(hipMemcpyAsync(d_mem.p, mem.data(), n_mem * sizeof(ndt::CentroidMember), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(d_starts.p, starts.data(), starts.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h->partials.reserve(static_cast<size_t>(blocks) * ndt::kEvalStride));
  hipLaunchKernelGGL(ndt::k_centroid_fitness_multi, dim3(static_cast<unsigned>(blocks)), dim3(ndt::kBlock), 0, h->stream, d_mem.p, d_starts.p,
                     static_cast<int>(n_mem), ci, max_range, h->partials.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(ndt::launch_fitness_reduce(h->partials.p, d_starts.p, static_cast<int>(n_mem), h->host_result, h->stream));
  h->cf_launches += 2;
  h->cf_max_blocks = static_cast<size_t>(blocks);
  HIP_TRY(hipStreamSynchronize(h->stream));  // (also: `mem` and `starts` are pageable, the copies have read them)
  for (size_t i = 0; i < n_mem; i++)
    if (h->host_result[2 * i + 1] > 0) out[of[i]] = h->host_result[2 * i] / h->host_result[2 * i + 1];
  return NDT_OK;
}

ndt_status batch_centroid_fitness_impl(ndt_handle h, const void* pts, const size_t* offsets, size_t n_scans, size_t stride, bool on_device,
                                       const float* transforms, double max_range, double* fitness) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!offsets) return fail(NDT_ERR_INVALID, "null offsets");
  if (n_scans && !fitness) return fail(NDT_ERR_INVALID, "null fitness");
  if (n_scans && !transforms) return fail(NDT_ERR_INVALID, "null transforms");
  if (n_scans > 65535) return fail(NDT_ERR_INVALID, "at most 65535 scans per call");
  for (size_t k = 0; k < n_scans; k++)
    if (offsets[k + 1] < offsets[k]) return fail(NDT_ERR_INVALID, "offsets must be non-decreasing");
  if (stride < 12 || stride % 4) return fail(NDT_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
  const size_t n_pts = offsets[n_scans] - offsets[0];
  if (n_pts && !pts) return fail(NDT_ERR_INVALID, "null point buffer");
  if (n_pts > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points in one centroid fitness call");
  if (!h->grid || !h->target) return fail(NDT_ERR_NO_INPUT, "no input target");
  if (n_scans == 0) return NDT_OK;
  ndt_status s = ensure_device(h);
  if (s) return s;
  std::shared_ptr<DeviceCloud> cloud;  // the scans in the caller's order, one upload
  s = upload_cloud(h, n_pts ? static_cast<const unsigned char*>(pts) + offsets[0] * stride : nullptr, n_pts, stride, on_device, cloud);
  if (s) return s;
  std::vector<CentroidJob> jobs(n_scans);
  for (size_t k = 0; k < n_scans; k++) {
    jobs[k].src = cloud->pts.p + (offsets[k] - offsets[0]);
    jobs[k].n = offsets[k + 1] - offsets[k];
    jobs[k].T = transforms + 16 * k;
  }
  return centroid_fitness_many(h, h->grid.get(), jobs, max_range, fitness);
}

// C on the device: its points (x, y, z, 1) and / or linear indices, *n of them.  want == false: the count alone.
// One enumeration of the occupied entries (table_voxels), then the wait for the gather: the caller copies next.
ndt_status centroids_device(ndt_context* h, DeviceGrid* g, bool want, DevBuf<float4>& xyz1, DevBuf<long long>* idx, size_t* n) {
  *n = 0;
  if (g->empty) return NDT_OK;
  const ndt_status s = table_voxels<ndt::Occupied, ndt::CentroidEmit>(
      h->stream, g, want,
      [&](unsigned cnt, ndt::CentroidEmit& emit) -> hipError_t {
        HIP_PASS(xyz1.reserve(cnt));
        if (idx) HIP_PASS(idx->reserve(cnt));
        emit = {g->view().centroids, xyz1.p, idx ? idx->p : nullptr};
        return hipSuccess;
      },
      n);
  if (s) return s;
  if (want && *n) HIP_TRY(hipStreamSynchronize(h->stream));
  return NDT_OK;
}

}  // namespace

}  // namespace ndtc

extern "C" {

ndt_status ndt_grid_centroids(ndt_handle h, float* xyz1, int64_t* idx, size_t capacity, size_t* n) {
  if (!h || !n) return fail(NDT_ERR_INVALID, "bad arguments");
  if (!h->grid || !h->target) return fail(NDT_ERR_NO_INPUT, "no input target");
  *n = 0;
  if (h->grid->empty) return NDT_OK;
  ndt_status s = ensure_device(h);
  if (s) return s;
  DevBuf<float4> d_xyz1;
  DevBuf<long long> d_idx;
  size_t count = 0;
  s = centroids_device(h, h->grid.get(), xyz1 != nullptr, d_xyz1, idx ? &d_idx : nullptr, &count);
  if (s) return s;
  *n = count;
  if (!xyz1 || count == 0) return NDT_OK;
  if (capacity < count) return fail(NDT_ERR_INVALID, "capacity is smaller than the centroid cloud (*n holds its size)");
  s = download_records(h, d_xyz1.p, count, xyz1, 16);
  if (s) return s;
  if (idx) {
    static_assert(sizeof(long long) == sizeof(int64_t), "linear indices are 64-bit");
    HIP_TRY(hipMemcpyAsync(idx, d_idx.p, count * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return NDT_OK;
}

ndt_status ndt_grid_centroids_cloud(ndt_handle h, ndt_cloud* out) {
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  *out = nullptr;
  if (!h->grid || !h->target) return fail(NDT_ERR_NO_INPUT, "no input target");
  ndt_status s = ensure_device(h);
  if (s) return s;
  DevBuf<float4> d_xyz1;
  size_t count = 0;
  s = centroids_device(h, h->grid.get(), true, d_xyz1, nullptr, &count);
  if (s) return s;
  std::shared_ptr<DeviceCloud> c;  // a cloud like any uploaded one (its boxes come with the copy)
  s = upload_cloud(h, count ? d_xyz1.p : nullptr, count, sizeof(float4), true, c);
  if (s) return s;
  HIP_TRY(hipStreamSynchronize(h->stream));  // d_xyz1 goes back to the pool: the copy has read it
  c->device = h->device;
  c->made_on = h->stream;
  *out = new ndt_cloud_s{c};
  return NDT_OK;
}

ndt_status ndt_get_centroid_fitness_score(ndt_handle h, double max_range, double* fitness) {
  if (!h || !fitness) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = check_ready(h);
  if (s) return s;
  std::vector<CentroidJob> job(1);
  job[0].src = h->source->pts.p;
  job[0].n = h->source->n;
  job[0].T = h->final_T;
  return centroid_fitness_many(h, h->grid.get(), job, max_range, fitness);
}

ndt_status ndt_batch_centroid_fitness_scores(ndt_handle h, const void* pts, const size_t* offsets, size_t n_scans, size_t stride_bytes,
                                             const float* transforms, double max_range, double* fitness) {
  return batch_centroid_fitness_impl(h, pts, offsets, n_scans, stride_bytes, false, transforms, max_range, fitness);
}

ndt_status ndt_batch_centroid_fitness_scores_device(ndt_handle h, const void* d_pts, const size_t* offsets, size_t n_scans,
                                                    size_t stride_bytes, const float* transforms, double max_range, double* fitness) {
  return batch_centroid_fitness_impl(h, d_pts, offsets, n_scans, stride_bytes, true, transforms, max_range, fitness);
}

ndt_status ndt_diag_centroid_fitness(ndt_handle h, size_t* launches, size_t* excursion_passes, float* excursion, size_t* max_blocks) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (launches) *launches = h->cf_launches;
  if (excursion_passes) *excursion_passes = h->cf_passes;
  if (excursion) *excursion = h->cf_excursion;
  if (max_blocks) *max_blocks = h->cf_max_blocks;
  return NDT_OK;
}

}  // extern "C"
