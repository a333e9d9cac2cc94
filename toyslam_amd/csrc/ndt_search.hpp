// ndt_search.hpp -- exact nearest-neighbour search over a PointIndex (a cloud + the counting-sort voxel
// index K1 builds over it).  Device code in an anonymous namespace, like ndt_device.hpp.
//
// Search: the query's cell, then cubic shells of cells around it, until no unvisited shell can hold a
// better point -- exact; what the shells cannot finish within max_shells goes to one scan over all points by the wave.
//
//   query_cell, team_shell, scan_run, shell_limits  the shell walk of a team of eight lanes (or of a whole wave)
//   wave_scan_all, Lowest8, wave_pop_smallest       the scan over all points by the wave, and what selects from it
//   nearer, wave_nearest, team_min                  one nearest neighbour, ties on the lower point index
//   team_knn (knn_lds_bytes, knn_row)               the k nearest neighbours of a team's query, in LDS
//
// Users: getFitnessScore (ndt_kernels.hip fitness_body: shells, wave_nearest); GICP (gicp_kernels.hip: team_knn for the
// covariances, shells + nearer + wave_nearest for the correspondences); the outlier filters (ndt_outliers.hip: team_knn for
// STATISTICAL, shells + wave_scan_all for RADIUS); the normals (ndt_normals.hip: team_knn, and the shells and the scan in
// the forms that hand the visitor the record); the searches over voxel centroids (ndt_centroid_fitness.hip,
// gicp_grid.hip: query_cell, axis_gap, team_min over their own tables).
#pragma once
#include "ndt_device.hpp"

namespace ndt {
namespace {

constexpr int kKnnMinRing = 3;  // shells every query may try (see max_shells) before one scan over all points

// The query's cell (clamped into the grid) and its MARGIN: how far the query is from the nearest face of that cell
// (0 for a query outside the grid).  After shell r every unvisited point is at least r * leaf + margin away -- with
// the margin a query in a crowded cell can stop after its own cell (r = 0) instead of always walking 27.
__device__ __forceinline__ void query_cell(const GridGeom& g, float x, float y, float z, int& ci, int& cj, int& ck, float& margin) {
  int ri, rj, rk;
  search_ijk(g, x, y, z, ri, rj, rk);
  ci = max(g.min_b[0], min(g.max_b[0], ri));
  cj = max(g.min_b[1], min(g.max_b[1], rj));
  ck = max(g.min_b[2], min(g.max_b[2], rk));
  margin = 0.0f;
  if (ci == ri && cj == rj && ck == rk) {
    const float fx = x - static_cast<float>(ri) * g.leaf[0], fy = y - static_cast<float>(rj) * g.leaf[1], fz = z - static_cast<float>(rk) * g.leaf[2];
    margin = fminf(fminf(fminf(fx, g.leaf[0] - fx), fminf(fy, g.leaf[1] - fy)), fminf(fz, g.leaf[2] - fz));
    margin = fmaxf(margin, 0.0f);
  }
  ci -= g.min_b[0];  // nearest grid cell when outside the bounding box
  cj -= g.min_b[1];
  ck -= g.min_b[2];
}

// ---------------------------------------------------------------------------
// Team search.  A query is worked on by kTeam = 8 adjacent lanes: they look up the same cell and
// stride over its points, each lane keeping its own best / its own sorted candidate list, and the
// team combines them with three xor-shuffles.  With a thread per query the few 10^4 queries of a
// down-sampled scan leave the chip almost empty and every query is one long chain of load
// latencies (measured on the reference pair: 2 ms per correspondence step, 4 ms per covariance
// pass); teams cut the chain eightfold and give the machine eight times the waves.
// ---------------------------------------------------------------------------
constexpr int kTeam = 8;

// squared distances from (qx,qy,qz) to this lane's share of the `count` cell-ordered points starting at
// `first` (positions sub, sub + 8, ...), two loads in flight.  visit(d, position in the cell order, valid) is
// called the same number of times by every lane of the team (valid = false past the end), so that a visitor may
// use team-wide operations.
template <int TEAM = kTeam, class F>
__device__ __forceinline__ void scan_run(const float4* __restrict__ sp, unsigned first, int count, int sub, float qx, float qy,
                                         float qz, F&& visit) {
  for (int base = 0; base < count; base += 2 * TEAM) {
    const int p0 = base + sub, p1 = p0 + TEAM;
    const bool v0 = p0 < count, v1 = p1 < count;
    // clamped, not predicated: both loads issue together (count >= 1 here)
    const float4 a = sp[first + min(p0, count - 1)], b = sp[first + min(p1, count - 1)];
    const float da = dist2_f32(qx, qy, qz, a.x, a.y, a.z), db = dist2_f32(qx, qy, qz, b.x, b.y, b.z);
    visit(da, first + p0, v0);
    visit(db, first + p1, v1);
  }
}
// the sibling whose visitor is also handed the record just loaded: visit(d, position, valid, record) -- for a visitor that
// sums over the neighbours themselves (ndt_normals.hip); same loads, same order
template <int TEAM = kTeam, class F>
__device__ __forceinline__ void scan_run_pts(const float4* __restrict__ sp, unsigned first, int count, int sub, float qx, float qy,
                                             float qz, F&& visit) {
  for (int base = 0; base < count; base += 2 * TEAM) {
    const int p0 = base + sub, p1 = p0 + TEAM;
    const bool v0 = p0 < count, v1 = p1 < count;
    const float4 a = sp[first + min(p0, count - 1)], b = sp[first + min(p1, count - 1)];
    const float da = dist2_f32(qx, qy, qz, a.x, a.y, a.z), db = dist2_f32(qx, qy, qz, b.x, b.y, b.z);
    visit(da, first + p0, v0, a);
    visit(db, first + p1, v1, b);
  }
}

// lexicographic minimum of (d, idx) over the 8 lanes of a team
__device__ __forceinline__ void team_min(float& d, int& idx) {
#pragma unroll
  for (int off = 1; off < kTeam; off <<= 1) {
    const float od = __shfl_xor(d, off, kWave);
    const int oi = __shfl_xor(idx, off, kWave);
    if (od < d || (od == d && oi < idx)) {
      d = od;
      idx = oi;
    }
  }
}
__device__ __forceinline__ int team_sum(int v) {
#pragma unroll
  for (int off = 1; off < kTeam; off <<= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// Shell r of cells around (ci, cj, ck), worked on by a team: the (2r+1)^2 rows of the shell are dealt out
// to the eight lanes, each lane probes one cell of its row per step (face rows: every x; interior rows:
// only x = -r and x = +r), and every occupied cell any lane finds is then scanned by the whole team.
// consider(d, position) as in scan_run.  All control flow is uniform within the team.
// bound2 (optional): a squared distance the caller can no longer use -- rows and cells that cannot hold a point
// nearer than that are not even looked up.  The distance from the query to a cell's box, less the index-rounding slack
// (a point may sit that far outside the cell it was binned into), bounds every point of the cell from below; after the
// query's own cell has given a neighbour at ~ the point spacing, that leaves one to three of a shell's 26 cells.
__device__ __forceinline__ float axis_gap(float q, int cell_abs, float leaf, float slack) {
  const float lo = static_cast<float>(cell_abs) * leaf, hi = lo + leaf;
  return fmaxf(fmaxf(lo - q, q - hi) - slack, 0.0f);
}
// PTS: consider(d, position, valid, record) -- scan_run_pts instead of scan_run
template <int TEAM = kTeam, bool PTS = false, class F>
__device__ __forceinline__ void team_shell(const PointIndex& ix, int ci, int cj, int ck, int r, int sub, float qx, float qy,
                                           float qz, F&& consider, float bound2 = INFINITY) {
  // (TEAM = 8: the team search; TEAM = 64: a whole wave on one query -- the far queries of getFitnessScore, whose shells
  // have hundreds of rows)
  constexpr unsigned long long kTeamMask = TEAM >= 64 ? ~0ull : ((1ull << (TEAM & 63)) - 1ull);
  const GridGeom& g = ix.geom;
  const int w = 2 * r + 1, rows = w * w;
  const int team_base = (threadIdx.x & (kWave - 1)) & ~(TEAM - 1);
  const bool prune = bound2 < INFINITY;
  for (int row0 = 0; row0 < rows; row0 += TEAM) {
    const int row = row0 + sub;
    const int dz = row / w - r, dy = row % w - r;
    const int z = ck + dz, y = cj + dy;
    bool row_ok = row < rows && z >= 0 && z < g.div_b[2] && y >= 0 && y < g.div_b[1];
    float row_d2 = 0.0f;
    if (prune && row_ok) {
      const float gy = axis_gap(qy, y + g.min_b[1], g.leaf[1], ix.slack), gz = axis_gap(qz, z + g.min_b[2], g.leaf[2], ix.slack);
      row_d2 = gy * gy + gz * gz;
      row_ok = row_d2 <= bound2;
    }
    if (row_ok) row_ok = ix.row_any[y + z * g.div_b[1]] != 0;  // rows without a single occupied cell cost one load
    if (((__ballot(row_ok) >> team_base) & kTeamMask) == 0) continue;
    const bool face = (dz == -r || dz == r || dy == -r || dy == r);  // r == 0: the single row is a face row
    const int nx = face ? w : 2;
    int steps = row_ok ? nx : 0;  // the longest occupied row of this batch sets the number of steps (interior rows: 2 cells)
#pragma unroll
    for (int off = 1; off < TEAM; off <<= 1) steps = max(steps, __shfl_xor(steps, off, kWave));
    for (int t = 0; t < steps; t += 2) {  // two cells of the row per step: both table loads are in flight together
      uint2 range[2] = {make_uint2(0u, 0u), make_uint2(0u, 0u)};
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int tt = t + u;
        if (row_ok && tt < nx) {
          const int x = ci + (face ? tt - r : (tt == 0 ? -r : r));
          bool cell_ok = x >= 0 && x < g.div_b[0];
          if (prune && cell_ok) {
            const float gx = axis_gap(qx, x + g.min_b[0], g.leaf[0], ix.slack);
            cell_ok = row_d2 + gx * gx <= bound2;
          }
          if (cell_ok) range[u] = ix.cell_range[x * g.mul[0] + y * g.mul[1] + z * g.mul[2]];
        }
      }
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const unsigned first = range[u].x;
        const int count = static_cast<int>(range[u].y);
        unsigned long long found = (__ballot(count > 0) >> team_base) & kTeamMask;
        while (found) {
          const int owner = __builtin_ctzll(found);
          found &= found - 1;
          const unsigned fs = __shfl(first, team_base + owner, kWave);
          const int fc = __shfl(count, team_base + owner, kWave);
          if constexpr (PTS) scan_run_pts<TEAM>(ix.sorted_pts, fs, fc, sub, qx, qy, qz, consider);
          else scan_run<TEAM>(ix.sorted_pts, fs, fc, sub, qx, qy, qz, consider);
        }
      }
    }
  }
}

// Shells tried before a query falls back to one scan over all points.  Shell r costs the team up to
// (2r+1)^3 / 8 probe steps, the shells up to r about (2r+1)^4 / 64 together; the scan costs n / 32 steps
// (8 lanes, four loads in flight): stop walking shells where the two meet.
__device__ __forceinline__ int max_shells(const PointIndex& ix, int r_lim) {
  const int by_cost = (static_cast<int>(sqrtf(sqrtf(2.0f * static_cast<float>(ix.n_sorted)))) - 1) / 2;
  return min(r_lim, max(kKnnMinRing, by_cost));
}

// What every shell loop over an index starts from: after shell r every unvisited point is at least r * leaf (+ the query's
// margin, - ix.slack) away; shell r_lim covers the whole grid; shells beyond r_max cost more than the scan over all points.
struct ShellLimits {
  float leaf;
  int r_lim, r_max;
};
__device__ __forceinline__ ShellLimits shell_limits(const PointIndex& ix) {
  const int r_lim = max(ix.geom.div_b[0], max(ix.geom.div_b[1], ix.geom.div_b[2]));
  return {fminf(ix.geom.leaf[0], fminf(ix.geom.leaf[1], ix.geom.leaf[2])), r_lim, max_shells(ix, r_lim)};
}

// ---------------------------------------------------------------------------
// The scan over all points, by the WHOLE wave: the few isolated queries that need it set a search kernel's time when one
// team of 8 lanes walks the cloud alone.  Every lane of the wave must call these with the same query.
// ---------------------------------------------------------------------------
// squared distances from the query to this lane's share of the cell-ordered points, four clamped loads in flight;
// visit(d, position, valid) is called the same number of times by every lane, so that a visitor may use wave-wide operations
template <class F>
__device__ __forceinline__ void wave_scan_all(const PointIndex& ix, float qx, float qy, float qz, F&& visit) {
  const int lane = threadIdx.x & (kWave - 1), count = ix.n_sorted;
  for (int base = 0; base < count; base += 4 * kWave) {
    const int p0 = base + lane, p1 = p0 + kWave, p2 = p1 + kWave, p3 = p2 + kWave;
    const float4 a = ix.sorted_pts[min(p0, count - 1)], b = ix.sorted_pts[min(p1, count - 1)];
    const float4 c = ix.sorted_pts[min(p2, count - 1)], d = ix.sorted_pts[min(p3, count - 1)];
    visit(dist2_f32(qx, qy, qz, a.x, a.y, a.z), p0, p0 < count);
    visit(dist2_f32(qx, qy, qz, b.x, b.y, b.z), p1, p1 < count);
    visit(dist2_f32(qx, qy, qz, c.x, c.y, c.z), p2, p2 < count);
    visit(dist2_f32(qx, qy, qz, d.x, d.y, d.z), p3, p3 < count);
  }
}
// the sibling whose visitor is also handed the record just loaded (see scan_run_pts)
template <class F>
__device__ __forceinline__ void wave_scan_all_pts(const PointIndex& ix, float qx, float qy, float qz, F&& visit) {
  const int lane = threadIdx.x & (kWave - 1), count = ix.n_sorted;
  for (int base = 0; base < count; base += 4 * kWave) {
    const int p0 = base + lane, p1 = p0 + kWave, p2 = p1 + kWave, p3 = p2 + kWave;
    const float4 a = ix.sorted_pts[min(p0, count - 1)], b = ix.sorted_pts[min(p1, count - 1)];
    const float4 c = ix.sorted_pts[min(p2, count - 1)], d = ix.sorted_pts[min(p3, count - 1)];
    visit(dist2_f32(qx, qy, qz, a.x, a.y, a.z), p0, p0 < count, a);
    visit(dist2_f32(qx, qy, qz, b.x, b.y, b.z), p1, p1 < count, b);
    visit(dist2_f32(qx, qy, qz, c.x, c.y, c.z), p2, p2 < count, c);
    visit(dist2_f32(qx, qy, qz, d.x, d.y, d.z), p3, p3 < count, d);
  }
}

// a lane's eight smallest values, ascending, in registers
struct Lowest8 {
  float m0 = INFINITY, m1 = INFINITY, m2 = INFINITY, m3 = INFINITY, m4 = INFINITY, m5 = INFINITY, m6 = INFINITY, m7 = INFINITY;
  __device__ __forceinline__ void keep(float d, bool ok) {
    if (!ok || !(d < m7)) return;
    m7 = d;  // bubble the newcomer down the sorted registers
    float t;
    if (m7 < m6) { t = m6; m6 = m7; m7 = t; }
    if (m6 < m5) { t = m5; m5 = m6; m6 = t; }
    if (m5 < m4) { t = m4; m4 = m5; m5 = t; }
    if (m4 < m3) { t = m3; m3 = m4; m4 = t; }
    if (m3 < m2) { t = m2; m2 = m3; m3 = t; }
    if (m2 < m1) { t = m1; m1 = m2; m2 = t; }
    if (m1 < m0) { t = m0; m0 = m1; m1 = t; }
  }
  __device__ __forceinline__ void pop() { m0 = m1; m1 = m2; m2 = m3; m3 = m4; m4 = m5; m5 = m6; m6 = m7; m7 = INFINITY; }
};
// Pops the wave's smallest head n times and returns the last: the n-th smallest of what the lanes kept (a lane that runs dry
// offers +inf), which bounds the n-th smallest of everything they were shown from above.
__device__ __forceinline__ float wave_pop_smallest(Lowest8& mine, int n) {
  const int lane = threadIdx.x & (kWave - 1);
  float bound = INFINITY;
  for (int j = 0; j < n; j++) {
    float h = mine.m0;
    int who = lane;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const float oh = __shfl_xor(h, off, kWave);
      const int ow = __shfl_xor(who, off, kWave);
      if (oh < h || (oh == h && ow < who)) {
        h = oh;
        who = ow;
      }
    }
    bound = h;
    if (who == lane) mine.pop();
  }
  return bound;
}

// The 1-NN rule on a lane's share of the candidates: nearer, or as near and the lower point index.  best_p is the POSITION
// of the best so far in the cell order (the index behind it is looked up on ties only), < 0: nothing taken yet -- then
// d == best == +inf is a distance that overflowed f32: not a neighbour, and there is no index to compare with
// (sorted_idx[-1] is four bytes in front of the array).
__device__ __forceinline__ bool nearer(const int* __restrict__ sorted_idx, float d, int pos, float best, int best_p) {
  if (d > best) return false;
  return d < best || (best_p >= 0 && sorted_idx[pos] < sorted_idx[best_p]);
}

// one nearest neighbour from the scan over all points: the smallest (distance, point index) in all lanes
__device__ __forceinline__ void wave_nearest(const PointIndex& ix, float qx, float qy, float qz, float& out_d, int& out_idx) {
  float best = INFINITY;
  int best_p = -1;
  wave_scan_all(ix, qx, qy, qz, [&](float d, int pos, bool ok) {
    if (ok && nearer(ix.sorted_idx, d, pos, best, best_p)) {
      best = d;
      best_p = pos;
    }
  });
  float d = best;
  int idx = best_p >= 0 ? ix.sorted_idx[best_p] : 0x7fffffff;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const float od = __shfl_xor(d, off, kWave);
    const int oi = __shfl_xor(idx, off, kWave);
    if (od < d || (od == d && oi < idx)) {
      d = od;
      idx = oi;
    }
  }
  out_d = d;
  out_idx = idx;
}

// ---------------------------------------------------------------------------
// The k nearest neighbours of a team's query.  One wave per block, eight teams, one candidate list PER TEAM in dynamic LDS
// (k entries, unordered, its worst entry tracked), not one per lane: an eighth of the LDS (per-lane lists capped the GICP
// kernel at 3.5 waves per SIMD) and a bound every lane prunes with.  A candidate that beats the worst entry replaces it and
// the team finds the new worst together; order is established once, at the end, by a rank sort.
//
// What differs between the users is a policy P, compile-time throughout:
//   kPositions  true: an entry is (distance, POSITION in the cell order) and the order is (distance, point index) -- the
//               index behind a position is looked up only when two distances are equal.  false: distances alone (the
//               caller's value depends on their multiset only); equal distances are ordered by slot.
//   kDropSelf   the query is a point of the cloud and no neighbour of itself: the first candidate at distance exactly 0
//               (the query, or a duplicate in its place) is dropped, and the scan's bound is the (k + 1)-th smallest.
//   kClear      the factor the k-th best keeps clear of the shells' reach in the stop test (1: the bare comparison).
//   kCountScans add the number of queries that went to the scan over all points to *scanned.
// ---------------------------------------------------------------------------
constexpr int kTeamsPerWave = kWave / kTeam;

// The dynamic LDS of such a block: [8][k] distances, [8][k] positions where the list carries them, then the caller's own
// [8][k] row of Row entries -- what it makes of the neighbours, in ascending order (team_knn's emit fills it).
__host__ __device__ constexpr size_t knn_list_bytes(int k, bool positions) {
  return static_cast<size_t>(kTeamsPerWave) * static_cast<size_t>(k) * (positions ? sizeof(float) + sizeof(int) : sizeof(float));
}
template <class Row>
__host__ __device__ constexpr size_t knn_lds_bytes(int k, bool positions) {
  static_assert(sizeof(Row) <= 8, "the list's end is aligned to 8 bytes");
  return knn_list_bytes(k, positions) + static_cast<size_t>(kTeamsPerWave) * static_cast<size_t>(k) * sizeof(Row);
}
template <class Row>
__device__ __forceinline__ Row* knn_row(unsigned char* lds, int k, bool positions, int team) {
  return reinterpret_cast<Row*>(lds + knn_list_bytes(k, positions)) + team * k;
}

__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }  // one wave per block: program order is enough

// Every lane of the wave calls this once per pass (a team without a query: search = false, it idles -- the scan of the
// isolated queries is wave-wide).  The team of a searching query then calls emit(rank, distance, position) for each of
// the entries found (lane `sub` for entries sub, sub + 8, ...; position 0 without kPositions); returns their number: k
// unless the cloud has fewer points.  The caller fences LDS before it reads what emit wrote there.
template <class P, class Emit>
__device__ __forceinline__ int team_knn(const PointIndex& ix, const ShellLimits& lim, int k, unsigned char* lds, const float4& q,
                                        bool search, unsigned* __restrict__ scanned, Emit&& emit) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (kWave - 1), sub = lane & (kTeam - 1), team = lane / kTeam, team_base = lane & ~(kTeam - 1);
  float* ld = reinterpret_cast<float*>(lds) + team * k;                      // [8][k] squared distances
  int* lp = reinterpret_cast<int*>(lds) + kTeamsPerWave * k + team * k;      // [8][k] positions (kPositions)
  int cnt = 0;  // entries in the list (team-uniform, like everything below that is not marked "lane")
  float worst = INFINITY;
  int worst_p = 0, worst_slot = 0;
  bool self_dropped = false;
  auto before = [&](float da, int pa, float db, int pb) {  // the order of the neighbours
    if constexpr (P::kPositions) return da < db || (da == db && ix.sorted_idx[pa] < ix.sorted_idx[pb]);
    else return da < db;
  };
  auto find_worst = [&] {  // the list's last entry in that order
    float bd = -1.0f;  // lane: worst so far over my slots
    int bp = 0, bs = -1;
    for (int j = sub; j < cnt; j += kTeam) {
      const float d = ld[j];
      const int p = P::kPositions ? lp[j] : 0;
      if (bs < 0 || before(bd, bp, d, p)) {
        bd = d;
        bp = p;
        bs = j;
      }
    }
#pragma unroll
    for (int off = 1; off < kTeam; off <<= 1) {
      const float od = __shfl_xor(bd, off, kWave);
      const int op = P::kPositions ? __shfl_xor(bp, off, kWave) : 0, os = __shfl_xor(bs, off, kWave);
      // (without positions equal distances are no tie of the order: the lower slot, so that the team agrees on one)
      if (os >= 0 && (bs < 0 || before(bd, bp, od, op) || (!P::kPositions && od == bd && os < bs))) {
        bd = od;
        bp = op;
        bs = os;
      }
    }
    worst = bd;
    worst_p = bp;
    worst_slot = bs;
  };
  auto insert_one = [&](float cd, int cp) {  // team-collective: a candidate known to all eight lanes
    if constexpr (P::kDropSelf) {
      if (cd == 0.0f && !self_dropped) {  // d2(i, i) is exactly 0: the query itself, or a duplicate in its place
        self_dropped = true;
        return;
      }
    }
    const bool fill = cnt < k;
    if (!fill && !before(cd, cp, worst, worst_p)) return;
    if (sub == 0) {
      ld[fill ? cnt : worst_slot] = cd;
      if constexpr (P::kPositions) lp[fill ? cnt : worst_slot] = cp;
    }
    lds_fence();
    if (fill) cnt++;
    if (cnt == k) find_worst();
  };
  auto from_lane = [&](int pos, int src) { return P::kPositions ? __shfl(pos, src, kWave) : 0; };
  // every lane brings one candidate (or none); the ones that can enter the list are taken one at a time
  auto offer = [&](float d, unsigned upos, bool ok) {
    const int pos = static_cast<int>(upos);
    const bool want = ok && (cnt < k || before(d, pos, worst, worst_p) || (P::kDropSelf && d == 0.0f && !self_dropped));
    unsigned pending = static_cast<unsigned>((__ballot(want) >> team_base) & 0xffull);
    while (pending) {
      const int owner = __builtin_ctz(pending);
      pending &= pending - 1;
      insert_one(__shfl(d, team_base + owner, kWave), from_lane(pos, team_base + owner));
    }
  };
  int ci = 0, cj = 0, ck = 0;
  float margin = 0.0f;
  if (search) query_cell(ix.geom, q.x, q.y, q.z, ci, cj, ck, margin);
  bool done = !search;
  for (int r = 0; r <= lim.r_max && !done; r++) {
    team_shell(ix, ci, cj, ck, r, sub, q.x, q.y, q.z, offer);
    // Every unvisited point is at least r cells plus the query's margin (less the index-rounding slack) away: once the
    // k-th best lies strictly inside that reach no unvisited point can enter the k nearest.
    const float reach = static_cast<float>(r) * lim.leaf + margin - ix.slack;
    if ((cnt == k && reach > 0.0f && worst * P::kClear < reach * reach) || r >= lim.r_lim) done = true;
  }
  // Sparse neighbourhoods: the WAVE looks at every point, twice, for one unfinished query at a time.  Pass 1 only keeps
  // each lane's eight smallest distances, in registers; the k-th smallest of the wave's 512 values (the (k + 1)-th where the
  // query itself is among them) bounds the k-th neighbour's distance from above.  Pass 2 hands the points inside that bound
  // -- about k of them -- to the query's team, which fills its list afresh.  (The few isolated queries set a kernel's time
  // when a team walks the cloud alone, and a single pass with the list spends its time updating it: points arrive in
  // arbitrary order.)
  unsigned long long open_teams = __ballot(!done && sub == 0);
  if constexpr (P::kCountScans)
    if (open_teams && lane == 0) atomicAdd(scanned, static_cast<unsigned>(__popcll(open_teams)));
  while (open_teams) {
    const int src_lane = __builtin_ctzll(open_teams);
    open_teams &= open_teams - 1;
    const bool mine = (team == src_lane / kTeam);
    const float ox = __shfl(q.x, src_lane, kWave), oy = __shfl(q.y, src_lane, kWave), oz = __shfl(q.z, src_lane, kWave);
    Lowest8 low;
    wave_scan_all(ix, ox, oy, oz, [&](float d, int, bool ok) { low.keep(d, ok); });
    const float bound = wave_pop_smallest(low, k + (P::kDropSelf ? 1 : 0));  // (the cloud has that many points)
    if (mine) {
      cnt = 0;
      worst = INFINITY;
      self_dropped = false;
    }
    wave_scan_all(ix, ox, oy, oz, [&](float d, int pos, bool ok) {  // the hits go to the owning team one by one
      unsigned long long hits = __ballot(ok && !(d > bound));
      while (hits) {
        const int from = __builtin_ctzll(hits);
        hits &= hits - 1;
        const float cd = __shfl(d, from, kWave);
        const int cp = from_lane(pos, from);
        if (mine) insert_one(cd, cp);
      }
    });
  }
  if (!search) return 0;
  // rank sort: entry j goes to the place given by the number of entries before it
  for (int j = sub; j < cnt; j += kTeam) {
    const float d = ld[j];
    const int p = P::kPositions ? lp[j] : 0;
    int rank = 0;
    for (int t = 0; t < cnt; t++) {
      const float o = ld[t];
      if constexpr (P::kPositions) rank += (t != j && before(o, lp[t], d, p)) ? 1 : 0;
      else rank += (o < d || (o == d && t < j)) ? 1 : 0;  // (equal distances: by slot)
    }
    emit(rank, d, p);
  }
  return cnt;
}

}  // namespace
}  // namespace ndt
