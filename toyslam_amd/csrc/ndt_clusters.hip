// ndt_clusters.hip -- Euclidean cluster extraction of resident clouds (ndt_cloud_cluster, ndt_cloud_extract_clusters,
// ndt_cloud_extract_clusters_clouds; contract: include/ndt_mi355.h, shared host / device definitions: ndt_clusters.hpp).
// Modelled on pcl::EuclideanClusterExtraction; no bit parity with PCL is claimed.
//   index   : one PointIndex per input cloud (build_grid, index_only, not dense: rows that are not finite are simply not in
//             it); the leaf follows the tolerance, as the RADIUS outlier filter's follows its radius.  Time only: no result
//             depends on the leaf.
//   parents : k_cluster_init, parent[i] = i for a finite point, -1 for the others; sizes 0.
//   link    : k_cluster_link, the hot path.  The walk of the RADIUS filter (one wave per block, a team of eight lanes per
//             query, shells pruned by the tolerance, the whole-cloud scan beyond max_shells) -- and every neighbour j < i
//             found within the tolerance is united with i in a LOCK-FREE union-find over parent[]: the larger root is hooked
//             under the smaller with one compare-and-swap, retried from what the swap returned.  No wave waits for another.
//   flatten : k_cluster_flatten, a launch of its own (every hook is visible): parent[i] = its root, size[root] += 1 (integer
//             atomics: exact).  A root is the smallest index of its component.
//   keys    : k_cluster_keys, per point the selection's key (1: its component's size is in range, 0: it is not, NaN: the point
//             is not finite), the flags of the clusters' roots for the table path, and the summary's tallies (integer atomics).
//   extract : the compaction of ndt_select.hip with those keys, device-resident.
//   table   : (ndt_cloud_cluster, one cloud) the flagged roots compacted in ascending order by an exclusive sum, numbered by a
//             stable sort on ~size, a label pass, the point indices sorted by label (stable: ascending inside a cluster), and
//             k_cluster_info: one block per cluster row, the exact f32 box and the f64 centroid by a plan of the size alone.
// No floating-point atomics, no inline assembly.
#include "ndt_internal.hpp"
#include "ndt_clusters.hpp"

#include "ndt_device.hpp"
#include "ndt_prims.hpp"
#include "ndt_search.hpp"

namespace ndtc {
namespace {

using ndt::PointIndex;
constexpr int kTeams = ndt::kClusterTeams;
constexpr int kBlock = 64;  // one wave
constexpr int kPtBlock = ndt::kClusterPointBlock;
static_assert(kTeams == ndt::kTeamsPerWave && kTeams * ndt::kTeam == kBlock, "a block is one wave of eight teams");

// rounding: an unvisited point at true distance D may compute a d2 a few 1e-7 (relative) below D*D.  The bounds that decide
// what is NOT looked at keep 1e-5 clear of the tolerance, so what is looked at decides alone (the RADIUS filter's bound).
constexpr float kClear = 1.00001f;
constexpr int kTally = 5;  // per cloud: finite points, components, clusters, clustered points, the largest component

struct ClMember {
  PointIndex ix;      // a cloud without a finite point: pts and n only, and no link block
  int* parent;        // n
  unsigned* size;     // n: at a root, the points of its component (after the flatten)
  double* keys;       // n, or null
  unsigned* flags;    // n, or null (the table path): 1 at the root of a cluster
  unsigned* tally;    // [kTally]
  int first_block, n_blocks;        // the link launch
  int pt_first, pt_blocks, pt_ppb;  // the per-point launches (cluster_point_plan)
};

// ---- the union-find.  parent[x] == x: x is a root; else parent[x] < x is an ancestor of x, and x never becomes a root again.
// THE COMPARE-AND-SWAP IS THE ONLY AUTHORITY.  Every read of parent[] while hooks are under way is an agent-scope relaxed
// ATOMIC load: the eight XCDs have private L2s and a plain load may be served a stale line.  A stale value is benign HERE --
// parents only ever move to smaller indices, so a stale "root" is a node whose swap fails and is retried from the value the
// swap returned -- but nothing may rely on that by accident: do not turn these into plain loads.
__device__ __forceinline__ int parent_of(const int* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// x's root as far as this lane can see; halves the path on the way (parent[x] of a non-root moves to an ancestor further up:
// an atomic minimum, so it never moves back)
__device__ __forceinline__ int find_root(int* parent, int x) {
  int p = parent_of(parent, x);
  while (p != x) {
    const int gp = parent_of(parent, p);
    if (gp != p) atomicMin(parent + x, gp);
    x = p;
    p = gp;
  }
  return x;
}
// a and b into one component; returns a node of it to go on from (its root as last seen).  a: what an earlier call returned
// for this query (or the query itself).  Lock-free: a failed swap returns a smaller index than the one it was tried on, so
// the loop ends, whatever the other waves do -- it never waits for them.
__device__ __forceinline__ int unite(int* parent, int a, int b, unsigned& retries) {
  b = find_root(parent, b);
  if (b == a) return a;  // b's tree hangs under a: one component already, whether or not a is still a root (the usual case)
  a = find_root(parent, a);
  while (a != b) {
    const int hi = max(a, b), lo = min(a, b);
    const int seen = atomicCAS(parent + hi, hi, lo);
    if (seen == hi) return lo;
    retries++;
    a = find_root(parent, seen);  // hi was no root any more
    b = find_root(parent, lo);
  }
  return a;
}

// Block `block` of the `n_blocks` that cut cloud `ix`: eight queries per pass, strided by n_blocks.
__device__ __forceinline__ void link_block(const PointIndex& ix, int* __restrict__ parent, float tol, float tol2, int block, int n_blocks,
                                           unsigned* __restrict__ diag) {
#pragma clang fp contract(off)
  using namespace ndt;
  const int lane = threadIdx.x, sub = lane & (kTeam - 1), team = lane / kTeam;
  const ShellLimits lim = shell_limits(ix);
  unsigned retries = 0;  // lane
  // The loop is uniform across the wave (a team without a query idles): the whole-cloud scan is wave-wide.
  for (int base = block * kTeams; base < ix.n; base += n_blocks * kTeams) {
    const int i = base + team;  // uniform within a team
    const bool live = i < ix.n;
    const float4 q = live ? ix.pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool search = live && finite3(q);
    int ci = 0, cj = 0, ck = 0;
    float margin = 0.f;
    if (search) query_cell(ix.geom, q.x, q.y, q.z, ci, cj, ck, margin);
    int root = i;  // lane: a node of i's component, its root as this lane last saw it
    // j < i suffices: d2(i, j) == d2(j, i) bit for bit, so the edge is found from its larger end
    auto consider = [&](float d, unsigned pos, bool ok) {
      if (ok && d <= tol2) {
        const int j = ix.sorted_idx[pos];
        if (j < i) root = unite(parent, root, j, retries);
      }
    };
    // The shells out to the first whose reach clears the tolerance; beyond max_shells, the scan over the cloud.
    const float far = tol * kClear;
    int r_need = 0;
    bool scan = false;
    if (search) {
      const float x = far - margin + ix.slack;
      r_need = x > 0.0f ? static_cast<int>(fminf(x / lim.leaf, 1.0e6f)) : 0;
      r_need = min(r_need, lim.r_lim);
      while (r_need < lim.r_lim && !(static_cast<float>(r_need) * lim.leaf + margin - ix.slack > far)) r_need++;
      scan = r_need > lim.r_max;
      if (!scan)
        for (int r = 0; r <= r_need; r++) team_shell(ix, ci, cj, ck, r, sub, q.x, q.y, q.z, consider, tol2 * (kClear * kClear));
    }
    unsigned long long open_teams = __ballot(scan && sub == 0);
    if (open_teams && lane == 0) atomicAdd(diag, static_cast<unsigned>(__popcll(open_teams)));
    while (open_teams) {
      const int src_lane = __builtin_ctzll(open_teams);
      open_teams &= open_teams - 1;
      const float ox = __shfl(q.x, src_lane, kWave), oy = __shfl(q.y, src_lane, kWave), oz = __shfl(q.z, src_lane, kWave);
      const int oi = __shfl(i, src_lane, kWave);
      int oroot = oi;
      wave_scan_all(ix, ox, oy, oz, [&](float d, int pos, bool ok) {
        if (ok && d <= tol2) {
          const int j = ix.sorted_idx[pos];
          if (j < oi) oroot = unite(parent, oroot, j, retries);
        }
      });
    }
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) retries += __shfl_xor(retries, off, kWave);
  if (lane == 0 && retries) atomicAdd(diag + 1, retries);  // one add per wave
}

// (a call of one cloud hands its member over as a kernel argument: no table to copy up first)
__global__ __launch_bounds__(kBlock) void k_cluster_link(ClMember one, const ClMember* __restrict__ members, int n_members, float tol, float tol2,
                                                         unsigned* __restrict__ diag) {
  // (not ndt::block_member: one body fed by a select between the argument and a table entry costs k_outlier_values, whose
  // walk this is, 49 VGPRs and two waves per SIMD -- a ClMember carries a whole PointIndex too; two calls keep each path's own)
  const int b = static_cast<int>(blockIdx.x);
  if (n_members == 1) {
    if (b < one.n_blocks) link_block(one.ix, one.parent, tol, tol2, b, one.n_blocks, diag);
    return;
  }
  const int lo = ndt::member_at(n_members, b, [&](int c) { return members[c].first_block; });
  const ClMember m = members[lo];
  const int local = b - m.first_block;
  if (local >= m.n_blocks) return;
  link_block(m.ix, m.parent, tol, tol2, local, m.n_blocks, diag);
}

// what the per-point launches start with: the block's member and its range of points
struct PointRange {
  long long start;
  int len;
};
__device__ __forceinline__ bool point_range(const ClMember& m, int b, PointRange& r) {
  const int lb = b - m.pt_first;
  if (lb >= m.pt_blocks) return false;
  r.len = ndt::block_range(lb, m.pt_ppb, m.ix.n, &r.start);
  return true;
}

__global__ __launch_bounds__(kPtBlock) void k_cluster_init(ClMember one, const ClMember* __restrict__ members, int n_members) {
  const int b = static_cast<int>(blockIdx.x);
  const ClMember m = ndt::block_member(one, members, n_members, b, &ClMember::pt_first);
  PointRange r;
  if (!point_range(m, b, r)) return;
  for (int j = threadIdx.x; j < r.len; j += kPtBlock) {
    const long long i = r.start + j;
    m.parent[i] = ndt::finite3(m.ix.pts[i]) ? static_cast<int>(i) : -1;
    m.size[i] = 0u;
  }
}

__global__ __launch_bounds__(kPtBlock) void k_cluster_flatten(ClMember one, const ClMember* __restrict__ members, int n_members) {
  const int b = static_cast<int>(blockIdx.x);
  const ClMember m = ndt::block_member(one, members, n_members, b, &ClMember::pt_first);
  PointRange r;
  if (!point_range(m, b, r)) return;
  for (int j = threadIdx.x; j < r.len; j += kPtBlock) {
    const int i = static_cast<int>(r.start + j);
    // (other threads of this launch shorten paths meanwhile: atomic loads and stores, and every value is an ancestor)
    int x = parent_of(m.parent, i);
    if (x < 0) continue;
    for (int p = parent_of(m.parent, x); p != x; p = parent_of(m.parent, x)) x = p;  // the roots are final: no hook is under way
    __hip_atomic_store(m.parent + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(m.size + x, 1u);
  }
}

__device__ __forceinline__ bool size_in_range(unsigned s, int min_size, int max_size) {
  return s >= static_cast<unsigned>(min_size) && s <= static_cast<unsigned>(max_size);
}

__global__ __launch_bounds__(kPtBlock) void k_cluster_keys(ClMember one, const ClMember* __restrict__ members, int n_members, int min_size,
                                                           int max_size) {
  const int b = static_cast<int>(blockIdx.x);
  const ClMember m = ndt::block_member(one, members, n_members, b, &ClMember::pt_first);
  PointRange r;
  if (!point_range(m, b, r)) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  unsigned t[kTally] = {0u, 0u, 0u, 0u, 0u};
  for (int j = threadIdx.x; j < r.len; j += kPtBlock) {
    const long long i = r.start + j;
    const int root = m.parent[i];
    double key = nan;
    unsigned flag = 0u;
    if (root >= 0) {
      const unsigned s = m.size[root];
      const bool in = size_in_range(s, min_size, max_size);
      key = in ? 1.0 : 0.0;
      t[0]++;
      if (root == i) {
        t[1]++;
        t[4] = max(t[4], s);
        if (in) {
          flag = 1u;
          t[2]++;
          t[3] += s;
        }
      }
    }
    if (m.keys) m.keys[i] = key;
    if (m.flags) m.flags[i] = flag;
  }
#pragma unroll
  for (int off = 1; off < ndt::kWave; off <<= 1) {
#pragma unroll
    for (int k = 0; k < 4; k++) t[k] += __shfl_xor(t[k], off, ndt::kWave);
    t[4] = max(t[4], static_cast<unsigned>(__shfl_xor(t[4], off, ndt::kWave)));
  }
  if ((threadIdx.x & (ndt::kWave - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (t[k]) atomicAdd(m.tally + k, t[k]);
    if (t[4]) atomicMax(m.tally + 4, t[4]);
  }
}

// ---- the table path (one cloud)
// the flagged roots, ascending: root and the sort key ~size (descending size; the stable sort keeps ascending roots on ties)
__global__ __launch_bounds__(kPtBlock) void k_cluster_compact(const unsigned* __restrict__ flags, const unsigned* __restrict__ pos,
                                                              const unsigned* __restrict__ size, int n, unsigned* __restrict__ c_key,
                                                              int* __restrict__ c_root) {
  for (long long i = static_cast<long long>(blockIdx.x) * kPtBlock + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * kPtBlock)
    if (flags[i]) {
      c_key[pos[i]] = ~size[i];
      c_root[pos[i]] = static_cast<int>(i);
    }
}
// cluster c's root gets its number; its size goes where the exclusive sum reads it
__global__ __launch_bounds__(kPtBlock) void k_cluster_number(const unsigned* __restrict__ s_key, const int* __restrict__ s_root, int n_clusters,
                                                             int* __restrict__ number, unsigned* __restrict__ sizes) {
  for (long long c = static_cast<long long>(blockIdx.x) * kPtBlock + threadIdx.x; c < n_clusters; c += static_cast<long long>(gridDim.x) * kPtBlock) {
    number[s_root[c]] = static_cast<int>(c);
    sizes[c] = ~s_key[c];
  }
}
// label_i, and the pair (label, or n_clusters for the points of no cluster; i) of the grouping sort
__global__ __launch_bounds__(kPtBlock) void k_cluster_labels(const int* __restrict__ parent, const unsigned* __restrict__ size,
                                                             const int* __restrict__ number, int n, int n_clusters, int min_size, int max_size,
                                                             int* __restrict__ labels, unsigned* __restrict__ l_key, int* __restrict__ l_val) {
  for (long long i = static_cast<long long>(blockIdx.x) * kPtBlock + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * kPtBlock) {
    const int root = parent[i];
    int label = -1;
    if (root >= 0 && size_in_range(size[root], min_size, max_size)) label = number[root];
    labels[i] = label;
    if (l_key) {
      l_key[i] = label < 0 ? static_cast<unsigned>(n_clusters) : static_cast<unsigned>(label);
      l_val[i] = static_cast<int>(i);
    }
  }
}
// Row c of the table, one block per row: the run of cluster c in the grouped indices.  Thread t takes the run's entries
// t, t + 256, ... in that order and block_sum adds the threads in its fixed tree: a shape that depends on the size alone.
__global__ __launch_bounds__(ndt::kClusterInfoBlock) void k_cluster_info(const float4* __restrict__ pts, const int* __restrict__ grouped,
                                                                         const unsigned* __restrict__ first, const unsigned* __restrict__ sizes,
                                                                         ndt_cluster_info* __restrict__ rows) {
#pragma clang fp contract(off)
  constexpr int B = ndt::kClusterInfoBlock, W = B / ndt::kWave;
  __shared__ double sh[B];
  __shared__ float box[W][6];
  const int c = static_cast<int>(blockIdx.x);
  const unsigned f = first[c], s = sizes[c];
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  double sum[3] = {0.0, 0.0, 0.0};
  for (unsigned j = threadIdx.x; j < s; j += B) {
    const float4 p = pts[grouped[f + j]];
    const float v[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int a = 0; a < 3; a++) {
      mn[a] = fminf(mn[a], v[a]);
      mx[a] = fmaxf(mx[a], v[a]);
      sum[a] += static_cast<double>(v[a]);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float lo = ndt::wave_min(mn[a]), hi = ndt::wave_max(mx[a]);
    if (lane == 0) {
      box[wave][a] = lo;
      box[wave][3 + a] = hi;
    }
    sum[a] = ndt::block_sum<B>(sum[a], sh);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ndt_cluster_info row{};
    row.root = grouped[f];  // the run ascends: its first index is the component's smallest
    row.size = static_cast<int32_t>(s);
    row.first = f;
    for (int a = 0; a < 3; a++) {
      float lo = box[0][a], hi = box[0][3 + a];
      for (int w = 1; w < W; w++) {
        lo = fminf(lo, box[w][a]);
        hi = fmaxf(hi, box[w][3 + a]);
      }
      row.box_min[a] = lo;
      row.box_max[a] = hi;
      row.centroid[a] = sum[a] / static_cast<double>(s);
    }
    rows[c] = row;
  }
}

// development switch, read at every call: small values reach the strided regime with small clouds
int max_blocks_switch() { return env_block_cap("NDT_CLUSTER_MAX_BLOCKS", ndt::kClusterMaxBlocks); }

// What one call works on
struct ClusterRun {
  std::vector<std::shared_ptr<DeviceCloud>> clouds;
  bool want_keys = false, want_flags = false;
  std::vector<size_t> first_pt;  // [clouds + 1]: the points before each cloud, the total
  // kept until the wait
  std::vector<std::shared_ptr<DeviceGrid>> grids;
  MemberTable<ClMember> mem;
  std::vector<int> member_of_cloud;  // -1: a cloud without a point has no member
  DevBuf<int> d_parent;
  DevBuf<unsigned> d_size, d_flags, d_tally, d_diag;
  DevBuf<double> d_keys;
  long long link_blocks = 0, pt_blocks = 0;
  std::vector<unsigned> tally_host;
  unsigned diag_host[2] = {0u, 0u};
  std::vector<ndt_cluster_summary> summaries;
};

// Indices, parents, link, flatten, keys: queued on h's stream; the read-backs are queued too but NOT waited for.
ndt_status cluster_queue(ndt_handle h, const ndt_cluster_spec& spec, ClusterRun& R) {
  hipStream_t st = h->stream;
  const size_t nc = R.clouds.size();
  h->cl_index_builds = h->cl_launches = h->cl_link_blocks = h->cl_scanned = h->cl_cas_retries = 0;
  R.summaries.assign(nc, ndt_cluster_summary{});
  R.grids.resize(nc);
  R.member_of_cloud.assign(nc, -1);
  R.first_pt.assign(nc + 1, 0);
  for (size_t k = 0; k < nc; k++) R.first_pt[k + 1] = R.first_pt[k] + R.clouds[k]->n;
  const size_t total = R.first_pt[nc];
  R.tally_host.assign(nc * kTally, 0u);
  if (total == 0) return NDT_OK;
  // ---- the indices
  for (size_t k = 0; k < nc; k++) {
    const std::shared_ptr<DeviceCloud>& c = R.clouds[k];
    if (c->n == 0) continue;
    ndt_status s = build_grid(h, c, GridSpec{index_leaf_clamped(*c, spec.tolerance), 1, h->eig_ratio, 0, false, true}, R.grids[k]);
    if (!s) s = grid_counts(h, R.grids[k].get());
    if (s) return s;
    h->cl_index_builds++;
    DeviceGrid* g = R.grids[k].get();
    if (!g->empty && g->n_sorted)
      if ((s = ensure_cell2leaf(h, g))) return s;
  }
  // ---- the buffers and the member table
  HIP_TRY(R.d_parent.reserve(total));
  HIP_TRY(R.d_size.reserve(total));
  if (R.want_keys) HIP_TRY(R.d_keys.reserve(total));
  if (R.want_flags) HIP_TRY(R.d_flags.reserve(total));
  HIP_TRY(R.d_tally.reserve(nc * kTally));
  HIP_TRY(R.d_diag.reserve(2));
  const int cap = max_blocks_switch();
  for (size_t k = 0; k < nc; k++) {
    const DeviceCloud* c = R.clouds[k].get();
    if (c->n == 0) continue;
    ClMember m{};
    const DeviceGrid* g = R.grids[k].get();
    const bool indexed = !g->empty && g->n_sorted;
    if (indexed) {
      fill_point_index(g, m.ix);
    } else {
      m.ix.pts = c->pts.p;
      m.ix.n = static_cast<int>(c->n);
    }
    m.parent = R.d_parent.p + R.first_pt[k];
    m.size = R.d_size.p + R.first_pt[k];
    m.keys = R.want_keys ? R.d_keys.p + R.first_pt[k] : nullptr;
    m.flags = R.want_flags ? R.d_flags.p + R.first_pt[k] : nullptr;
    m.tally = R.d_tally.p + k * kTally;
    int nb = 0, qpb = 0;
    if (indexed) ndt::cluster_plan(c->n, cap, &nb, &qpb);
    m.first_block = static_cast<int>(R.link_blocks);
    m.n_blocks = nb;
    R.link_blocks += nb;
    ndt::cluster_point_plan(c->n, &m.pt_blocks, &m.pt_ppb);
    m.pt_first = static_cast<int>(R.pt_blocks);
    R.pt_blocks += m.pt_blocks;
    R.member_of_cloud[k] = R.mem.n();
    R.mem.host.push_back(m);
  }
  if (R.link_blocks > std::numeric_limits<int>::max()) return fail(NDT_ERR_INVALID, "too many points");
  HIP_TRY(hipMemsetAsync(R.d_tally.p, 0, nc * kTally * sizeof(unsigned), st));
  HIP_TRY(hipMemsetAsync(R.d_diag.p, 0, 2 * sizeof(unsigned), st));
  if (ndt_status s = R.mem.upload(st)) return s;
  // ---- the launches
  const dim3 pt_grid(static_cast<unsigned>(R.pt_blocks));
  hipLaunchKernelGGL(k_cluster_init, pt_grid, dim3(kPtBlock), 0, st, R.mem.one(), R.mem.table(), R.mem.n());
  HIP_TRY(hipGetLastError());
  h->cl_launches++;
  if (R.link_blocks) {
    hipLaunchKernelGGL(k_cluster_link, dim3(static_cast<unsigned>(R.link_blocks)), dim3(kBlock), 0, st, R.mem.one(), R.mem.table(), R.mem.n(),
                       spec.tolerance, spec.tolerance * spec.tolerance, R.d_diag.p);
    HIP_TRY(hipGetLastError());
    h->cl_launches++;
  }
  h->cl_link_blocks = static_cast<size_t>(R.link_blocks);
  hipLaunchKernelGGL(k_cluster_flatten, pt_grid, dim3(kPtBlock), 0, st, R.mem.one(), R.mem.table(), R.mem.n());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_cluster_keys, pt_grid, dim3(kPtBlock), 0, st, R.mem.one(), R.mem.table(), R.mem.n(), spec.min_size, spec.max_size);
  HIP_TRY(hipGetLastError());
  h->cl_launches += 2;
  HIP_TRY(hipMemcpyAsync(R.tally_host.data(), R.d_tally.p, nc * kTally * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(R.diag_host, R.d_diag.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  return NDT_OK;
}

// after the stream has been waited for: the summary of every cloud, the diagnostics
void cluster_finish(ndt_handle h, ClusterRun& R) {
  for (size_t k = 0; k < R.clouds.size(); k++) {
    const unsigned* t = &R.tally_host[k * kTally];
    R.summaries[k] = ndt_cluster_summary{t[0], t[1], t[2], t[3], t[4]};
  }
  h->cl_scanned = R.diag_host[0];
  h->cl_cas_retries = R.diag_host[1];
}

// the selection that goes with a call: the keys are 1 (in a cluster), 0 (finite, in none), NaN (not finite: never kept)
ndt_select_spec key_spec(int negate) {
  ndt_select_spec s{};
  s.flags = NDT_SELECT_KEY | (negate ? NDT_SELECT_KEY_NEGATE : 0);
  s.key_lo = 1.0;
  s.key_hi = 1.0;
  return s;
}

ndt_status spec_checks(const ndt_cluster_spec* spec) { return ndtc::spec_checks(spec, ndt::cluster_spec_error); }

size_t align256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

}  // namespace
}  // namespace ndtc

extern "C" {

ndt_status ndt_cloud_cluster(ndt_handle h, ndt_cloud in, const ndt_cluster_spec* spec, int32_t* labels, int labels_on_device, int32_t* roots,
                             ndt_cluster_info* clusters, size_t cluster_capacity, int32_t* indices, ndt_cluster_summary* summary) {
  if (!h || !labels || (cluster_capacity && !clusters)) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = cloud_entry(h, in, [&] { return spec_checks(spec); });
  if (s) return s;
  hipStream_t st = h->stream;
  const size_t n = in->c->n;
  const int ni = static_cast<int>(n);
  ClusterRun R;
  R.clouds.push_back(in->c);
  R.want_flags = true;
  DevBuf<unsigned char> tmp, d_rows;
  Drain drain{st};
  if ((s = cluster_queue(h, *spec, R))) return s;
  if (n == 0) {
    cluster_finish(h, R);
    if (summary) *summary = R.summaries[0];
    return NDT_OK;
  }
  // ---- every temporary of the table path from one reservation: six arrays of n words, the labels on their way to the host,
  // the rows, and what the sorts and the scan ask for (they run one after another in stream order and share it)
  const size_t words = align256(n * sizeof(unsigned));
  const size_t tb = std::max({ndt::sort_pairs_temp_bytes(ni, sizeof(unsigned)), ndt::exclusive_sum_temp_bytes(ni), size_t(256)});
  HIP_TRY(tmp.reserve(7 * words + align256(tb)));
  auto arr = [&](int k) { return reinterpret_cast<unsigned*>(tmp.p + static_cast<size_t>(k) * words); };
  unsigned *pos = arr(0), *c_key = arr(1), *s_key = arr(2);
  int *c_root = reinterpret_cast<int*>(arr(3)), *s_root = reinterpret_cast<int*>(arr(4)), *l_val = reinterpret_cast<int*>(arr(5));
  int* d_labels = labels_on_device ? labels : reinterpret_cast<int*>(arr(6));
  void* temp = tmp.p + 7 * words;
  const ClMember& m = R.mem.one();
  HIP_TRY(ndt::exclusive_sum(m.flags, pos, ni, temp, tb, st));
  HIP_TRY(hipStreamSynchronize(st));  // the number of clusters sizes what follows
  cluster_finish(h, R);
  const ndt_cluster_summary& sum = R.summaries[0];
  const int C = static_cast<int>(sum.n_clusters);
  const size_t rows = std::min(static_cast<size_t>(C), cluster_capacity);
  const unsigned grid_n = static_cast<unsigned>(std::min<size_t>((n + kPtBlock - 1) / kPtBlock, 1024));
  // (arrays reused in stream order: number = the flags, sizes = pos, l_key = c_key, first = c_key again behind the grouping
  // sort, whose outputs go where the numbering sort's went)
  int* number = reinterpret_cast<int*>(m.flags);
  unsigned *sizes = pos, *l_key = c_key, *g_key = s_key, *first = c_key;
  int* grouped = s_root;
  if (C) {
    hipLaunchKernelGGL(k_cluster_compact, dim3(grid_n), dim3(kPtBlock), 0, st, m.flags, pos, m.size, ni, c_key, c_root);
    HIP_TRY(hipGetLastError());
    HIP_TRY(ndt::sort_pairs(c_key, s_key, c_root, s_root, C, 32, temp, tb, st));
    const unsigned grid_c = static_cast<unsigned>(std::min<size_t>((static_cast<size_t>(C) + kPtBlock - 1) / kPtBlock, 1024));
    hipLaunchKernelGGL(k_cluster_number, dim3(grid_c), dim3(kPtBlock), 0, st, s_key, s_root, C, number, sizes);
    HIP_TRY(hipGetLastError());
    h->cl_launches += 2;
  }
  const bool group = C && (indices || rows);
  hipLaunchKernelGGL(k_cluster_labels, dim3(grid_n), dim3(kPtBlock), 0, st, m.parent, m.size, number, ni, C, spec->min_size, spec->max_size, d_labels,
                     group ? l_key : nullptr, l_val);
  HIP_TRY(hipGetLastError());
  h->cl_launches++;
  if (group) {
    int bits = 1;
    while ((static_cast<unsigned long long>(C) >> bits) != 0) bits++;  // the keys are 0 ... C
    HIP_TRY(ndt::sort_pairs(l_key, g_key, l_val, grouped, ni, bits, temp, tb, st));
    if (indices) HIP_TRY(hipMemcpyAsync(indices, grouped, sum.n_clustered * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  if (rows) {
    HIP_TRY(ndt::exclusive_sum(sizes, first, C, temp, tb, st));
    HIP_TRY(d_rows.reserve(rows * sizeof(ndt_cluster_info)));
    HIP_TRY(hipMemsetAsync(d_rows.p, 0, rows * sizeof(ndt_cluster_info), st));  // (the padding of a row too: the same bytes in every call)
    hipLaunchKernelGGL(k_cluster_info, dim3(static_cast<unsigned>(rows)), dim3(ndt::kClusterInfoBlock), 0, st, m.ix.pts, grouped, first, sizes,
                       reinterpret_cast<ndt_cluster_info*>(d_rows.p));
    HIP_TRY(hipGetLastError());
    h->cl_launches++;
    HIP_TRY(hipMemcpyAsync(clusters, d_rows.p, rows * sizeof(ndt_cluster_info), hipMemcpyDeviceToHost, st));
  }
  if (!labels_on_device) HIP_TRY(hipMemcpyAsync(labels, d_labels, n * sizeof(int), hipMemcpyDeviceToHost, st));
  if (roots) HIP_TRY(hipMemcpyAsync(roots, m.parent, n * sizeof(int), labels_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (summary) *summary = sum;
  return NDT_OK;
}

ndt_status ndt_cloud_extract_clusters(ndt_handle h, ndt_cloud in, const ndt_cluster_spec* spec, int negate, ndt_cloud* out, int32_t* kept_idx,
                                      size_t* n_kept, ndt_cluster_summary* summary) {
  if (out) *out = nullptr;
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = cloud_entry(h, in, [&] { return spec_checks(spec); });
  if (s) return s;
  const size_t n = in->c->n;
  ClusterRun R;
  R.clouds.push_back(in->c);
  R.want_keys = true;
  std::shared_ptr<DeviceCloud> c;
  size_t kept = 0;
  {
    Drain drain{h->stream};
    SelDiagKeep keep(h);
    s = cluster_queue(h, *spec, R);
    if (s) return s;
    s = select_one(h, in->c->pts.p, n, key_spec(negate), R.d_keys.p, c, kept_idx, &kept);
    if (s) return s;
  }
  cluster_finish(h, R);
  if (n_kept) *n_kept = kept;
  if (summary) *summary = R.summaries[0];
  *out = new ndt_cloud_s{c};
  return NDT_OK;
}

ndt_status ndt_cloud_extract_clusters_clouds(ndt_handle h, const ndt_cloud* in, size_t n_clouds, const ndt_cluster_spec* spec, int negate,
                                             ndt_cloud* out, size_t* n_kept, ndt_cluster_summary* summaries) {
  if (!h || !out) return fail(NDT_ERR_INVALID, "bad arguments");
  ndt_status s = clouds_begin(n_clouds, out);
  if (s) return s;
  if (n_clouds && !in) return fail(NDT_ERR_INVALID, "null clouds");
  if ((s = spec_checks(spec))) return s;
  std::vector<size_t> first;
  if ((s = clouds_total(h, in, n_clouds, first))) return s;
  if (n_clouds == 0) return NDT_OK;
  s = ensure_device(h);
  if (s) return s;
  ClusterRun R;
  R.want_keys = true;
  OutSlices outs;
  std::vector<SelJob> jobs(n_clouds);
  if ((s = outs.reserve(h, first))) return s;
  for (size_t k = 0; k < n_clouds; k++) {
    if ((s = cloud_use_on(h, in[k]->c.get()))) return s;
    R.clouds.push_back(in[k]->c);
  }
  {
    Drain drain{h->stream};
    SelDiagKeep keep(h);
    s = cluster_queue(h, *spec, R);
    if (s) return s;
    for (size_t k = 0; k < n_clouds; k++) {
      DeviceCloud* c = in[k]->c.get();
      jobs[k].in = c->pts.p;
      jobs[k].n = c->n;
      jobs[k].keys = R.d_keys.p + first[k];
      jobs[k].out = outs.at(k);
      jobs[k].res = outs.cloud(k);
    }
    s = select_run(h, jobs, key_spec(negate), nullptr);
    if (s) return s;
  }
  cluster_finish(h, R);
  for (size_t k = 0; k < n_clouds; k++) {
    out[k] = outs.publish(k, jobs[k].kept);
    if (n_kept) n_kept[k] = jobs[k].kept;
    if (summaries) summaries[k] = R.summaries[k];
  }
  return NDT_OK;
}

ndt_status ndt_diag_clusters(ndt_handle h, size_t* index_builds, size_t* launches, size_t* link_blocks, size_t* scanned_queries,
                             size_t* cas_retries) {
  if (!h || !index_builds || !launches || !link_blocks || !scanned_queries || !cas_retries) return fail(NDT_ERR_INVALID, "bad arguments");
  *index_builds = h->cl_index_builds;
  *launches = h->cl_launches;
  *link_blocks = h->cl_link_blocks;
  *scanned_queries = h->cl_scanned;
  *cas_retries = h->cl_cas_retries;
  return NDT_OK;
}

ndt_status ndt_host_cluster_spec_check(const ndt_cluster_spec* spec) { return spec_checks(spec); }

ndt_status ndt_host_cluster_plan(size_t n_points, int* blocks, int* queries_per_block) {
  if (!blocks || !queries_per_block) return fail(NDT_ERR_INVALID, "bad arguments");
  if (n_points > static_cast<size_t>(std::numeric_limits<int>::max())) return fail(NDT_ERR_INVALID, "too many points");
  ndt::cluster_plan(n_points, ndtc::max_blocks_switch(), blocks, queries_per_block);
  return NDT_OK;
}

}  // extern "C"
