// ndt_voxel_table.hpp -- a target's voxel LOOK-UP TABLE read cell by cell or entry by entry, and the nearest-centroid search
// through it (device code in an anonymous namespace, like ndt_search.hpp): what the centroid fitness (ndt_centroid_fitness.hip)
// and GICP's correspondence step against a voxel target (gicp_grid.hip) share.  The table is the padded dense one, or the
// open-addressing hash keyed by the linear voxel index; an entry is a record r, lut_rejected(r), or kLutEmpty (ndt_kernels.hpp).
// table_shell<TEAM, P> and wave_scan_table<P> take a compile-time policy as team_knn<P> does; the DRIVERS -- which shells a
// team walks, when the wave takes over, the stopping rule -- stay with the two users and differ on purpose.
// (The enumeration of a table's voxels in ascending linear index: ndt_table_voxels.hpp.)
#pragma once
#include "ndt_search.hpp"

namespace ndt {

// A target's table as the centroid searches walk it (ndtc::centroid_index builds it)
struct CentroidIndex {
  GridView gv;
  long long entries;  // table entries one pass reads: lut_cells, or the hash's 2^hash_bits slots
  float give;         // index-rounding slack + excursion: how far a centroid may lie outside the box of its table cell
  int r_max;          // shells walked before the one scan of the table (centroid_shell_limit)
};

namespace {

constexpr int kProbes = 4;  // table probes (and then centroid loads) a lane keeps in flight

__device__ __forceinline__ int entry_record(int e) { return e >= 0 ? e : -(e + 2); }

// table entry of cell (x, y, z), box-relative and inside the box
__device__ __forceinline__ int cell_entry(const GridView& gv, int x, int y, int z) {
  const GridGeom& g = gv.g;
  if (g.hash_bits) {  // uniform
    const int key = x * g.mul[0] + y * g.mul[1] + z * g.mul[2];
    const int2* tab = reinterpret_cast<const int2*>(gv.lut);
    const unsigned mask = (1u << g.hash_bits) - 1u;
    for (unsigned h = hash_slot(key, g.hash_bits);; h = (h + 1u) & mask) {
      const int2 e = tab[h];
      if (e.x == key) return e.y;
      if (e.x == -1) return kLutEmpty;
    }
  }
  return gv.lut[static_cast<size_t>(x + kLutBorder) + static_cast<size_t>(y + kLutBorder) * static_cast<size_t>(g.pmul[1]) +
                static_cast<size_t>(z + kLutBorder) * static_cast<size_t>(g.pmul[2])];
}
// entry t of one pass over the table and, where occupied, its box-relative cell
__device__ __forceinline__ int table_entry(const GridView& gv, long long t) {
  if (gv.g.hash_bits) {
    const int2 e = reinterpret_cast<const int2*>(gv.lut)[t];
    return e.x == -1 ? kLutEmpty : e.y;
  }
  return gv.lut[t];
}
__device__ __forceinline__ void table_cell(const GridView& gv, long long t, int& x, int& y, int& z) {
  const GridGeom& g = gv.g;
  if (g.hash_bits) {
    const int key = reinterpret_cast<const int2*>(gv.lut)[t].x;
    z = key / g.mul[2];
    y = (key - z * g.mul[2]) / g.mul[1];
    x = key - z * g.mul[2] - y * g.mul[1];
  } else {
    const long long pz = t / g.pmul[2], rest = t - pz * g.pmul[2];
    z = static_cast<int>(pz) - kLutBorder;
    y = static_cast<int>(rest / g.pmul[1]) - kLutBorder;
    x = static_cast<int>(rest % g.pmul[1]) - kLutBorder;
  }
}

// ---- the search.  A policy P (an object: it may carry arrays) says what a walk looks for and what it carries:
//   P::Best, P::none()             a lane's best so far, and its start
//   P::candidate(e), P::record(e)  whether table entry e is a candidate, and the record it names
//   P::Side, p.side(rec)           what is loaded beside centroids[rec] (an empty struct: nothing)
//   P::take(d, side, best)         a candidate at squared distance d into the lane's best
//   P::fold(best, off)             the best of lane ^ off into this lane's
// kProbes cells go in three phases: the table entries together (the caller), the records of the candidates together, the arithmetic
template <class P>
__device__ __forceinline__ void probe_batch(const CentroidIndex& ci, const P& p, const int (&e)[kProbes], float qx, float qy, float qz,
                                            typename P::Best& best) {
  float4 c[kProbes];
  typename P::Side s[kProbes];
#pragma unroll
  for (int u = 0; u < kProbes; u++)
    if (P::candidate(e[u])) {
      const int rec = P::record(e[u]);
      c[u] = *reinterpret_cast<const float4*>(ci.gv.centroids + rec);  // (cx, cy, cz, -)
      s[u] = p.side(rec);
    }
#pragma unroll
  for (int u = 0; u < kProbes; u++)
    if (P::candidate(e[u])) P::take(dist2_f32(qx, qy, qz, c[u].x, c[u].y, c[u].z), s[u], best);
}

// Shell r of cells around (cx, cy, cz): its (2r+1)^2 rows dealt to the TEAM lanes; a lane walks its row (a face row: every x;
// an interior row: x = -r and +r) kProbes cells at a time and keeps its own best.  No lane needs another inside the walk: the
// team combines after it.  Rows and cells whose box, widened by ci.give, lies farther than bound2 are not looked up (at bound2
// exactly they are: a tie may hide there).
template <int TEAM, class P>
__device__ __forceinline__ void table_shell(const CentroidIndex& ci, const P& p, int cx, int cy, int cz, int r, int sub, float qx, float qy,
                                            float qz, float bound2, typename P::Best& best) {
  const GridGeom& g = ci.gv.g;
  const int w = 2 * r + 1, rows = w * w;
  for (int row = sub; row < rows; row += TEAM) {
    const int dz = row / w - r, dy = row % w - r;
    const int z = cz + dz, y = cy + dy;
    if (z < 0 || z >= g.div_b[2] || y < 0 || y >= g.div_b[1]) continue;
    const float gy = axis_gap(qy, y + g.min_b[1], g.leaf[1], ci.give), gz = axis_gap(qz, z + g.min_b[2], g.leaf[2], ci.give);
    const float row_d2 = gy * gy + gz * gz;
    if (row_d2 > bound2) continue;
    const bool face = (dz == -r || dz == r || dy == -r || dy == r);  // r == 0: the single row is a face row
    const int nx = face ? w : 2;
    for (int t = 0; t < nx; t += kProbes) {
      int e[kProbes];
#pragma unroll
      for (int u = 0; u < kProbes; u++) {
        e[u] = kLutEmpty;
        const int tt = t + u;
        const int x = cx + (face ? tt - r : (tt == 0 ? -r : r));
        if (tt < nx && x >= 0 && x < g.div_b[0]) {
          const float gx = axis_gap(qx, x + g.min_b[0], g.leaf[0], ci.give);
          if (row_d2 + gx * gx <= bound2) e[u] = cell_entry(ci.gv, x, y, z);
        }
      }
      probe_batch(ci, p, e, qx, qy, qz, best);
    }
  }
}

// ONE pass over the table by the whole wave (every lane with the same query): the best over all of it, in all lanes
template <class P>
__device__ __forceinline__ typename P::Best wave_scan_table(const CentroidIndex& ci, const P& p, float qx, float qy, float qz) {
  const int lane = threadIdx.x & (kWave - 1);
  typename P::Best best = P::none();
  for (long long base = 0; base < ci.entries; base += kProbes * kWave) {
    int e[kProbes];
#pragma unroll
    for (int u = 0; u < kProbes; u++) {
      const long long t = base + lane + u * kWave;
      e[u] = t < ci.entries ? table_entry(ci.gv, t) : kLutEmpty;
    }
    probe_batch(ci, p, e, qx, qy, qz, best);
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) P::fold(best, off);
  return best;
}

}  // namespace
}  // namespace ndt
