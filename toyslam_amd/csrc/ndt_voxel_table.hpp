// ndt_voxel_table.hpp -- reading a target's voxel LOOK-UP TABLE cell by cell or entry by entry (device code in an anonymous
// namespace, like ndt_search.hpp): what the centroid searches share -- the centroid fitness (ndt_centroid_fitness.hip) and GICP's
// correspondence step against a voxel target (gicp_grid.hip).  The table is the padded dense one, or the open-addressing hash
// keyed by the linear voxel index; an entry is a record r, lut_rejected(r), or kLutEmpty (ndt_kernels.hpp).
#pragma once
#include "ndt_device.hpp"

namespace ndt {

// A target's table as the centroid searches walk it
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

}  // namespace
}  // namespace ndt
