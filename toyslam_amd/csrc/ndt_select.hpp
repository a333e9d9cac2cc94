// ndt_select.hpp -- the selection predicate of ndt_cloud_select (include/ndt_mi355.h), ONE definition for the host entry
// (ndt_host_select_point) and the kernels (ndt_select.hip), the validity of a spec, and the launch plan both sides use.
// Every f32 operation of the range test is rounded on its own: select_dist2 is compiled with contraction off for host and
// device alike (the pragma below; g++ units have -ffp-contract=off).  HIP's __fmul_rn / __fadd_rn do NOT do that here: they
// are plain operators of a header compiled under the default -ffp-contract=fast, and once inlined the pair is fused again
// (seen in the ISA: v_fma_f32) -- tests/select_cases.py's FUSED_ROWS are the points on which a fused sum differs.
#pragma once
#include <cmath>
#include <cstddef>

#include "ndt_cloud_ops.hpp"
#include "ndt_mi355.h"

#if defined(__HIPCC__)
#define NDT_SELECT_HD __host__ __device__
#else
#define NDT_SELECT_HD
#endif

namespace ndt {

constexpr int kSelectBlock = 256;        // threads of a block (four waves)
constexpr int kSelectMaxBlocks = 1024;   // blocks of one cloud at most: beyond it points_per_block grows
constexpr unsigned kSelectKnownFlags = NDT_SELECT_FINITE | NDT_SELECT_BOX | NDT_SELECT_BOX_NEGATE | NDT_SELECT_RANGE |
                                       NDT_SELECT_RANGE_NEGATE | NDT_SELECT_KEY | NDT_SELECT_KEY_NEGATE;

// squared distance of (x, y, z) from the centre: (dx*dx + dy*dy) + dz*dz, five roundings
NDT_SELECT_HD inline float select_dist2(float x, float y, float z, const float c[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float dx = x - c[0], dy = y - c[1], dz = z - c[2];
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float xy = xx + yy;
  return xy + zz;
}

// is the point (with key k) kept?  Every enabled test must pass.
NDT_SELECT_HD inline bool select_keep(const ndt_select_spec& s, float x, float y, float z, double k) {
  const unsigned f = s.flags;
  if (f & NDT_SELECT_FINITE) {
    if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))) return false;
  }
  if (f & NDT_SELECT_BOX) {
    const bool inside = s.box_min[0] <= x && x <= s.box_max[0] && s.box_min[1] <= y && y <= s.box_max[1] && s.box_min[2] <= z &&
                        z <= s.box_max[2];
    if (inside == ((f & NDT_SELECT_BOX_NEGATE) != 0)) return false;
  }
  if (f & NDT_SELECT_RANGE) {
    const float d2 = select_dist2(x, y, z, s.centre);
    const float lo = s.r_min * s.r_min, hi = s.r_max * s.r_max;
    const bool inside = lo <= d2 && d2 <= hi;
    if (inside == ((f & NDT_SELECT_RANGE_NEGATE) != 0)) return false;
  }
  if (f & NDT_SELECT_KEY) {
    if (k != k) return false;  // a NaN key fails in both senses
    const bool inside = s.key_lo <= k && k <= s.key_hi;
    if (inside == ((f & NDT_SELECT_KEY_NEGATE) != 0)) return false;
  }
  return true;
}

// null = a valid spec, else what is wrong with it
inline const char* select_spec_error(const ndt_select_spec& s) {
  const unsigned f = s.flags;
  if (f & ~kSelectKnownFlags) return "unknown selection flags";
  if ((f & NDT_SELECT_BOX_NEGATE) && !(f & NDT_SELECT_BOX)) return "BOX_NEGATE without BOX";
  if ((f & NDT_SELECT_RANGE_NEGATE) && !(f & NDT_SELECT_RANGE)) return "RANGE_NEGATE without RANGE";
  if ((f & NDT_SELECT_KEY_NEGATE) && !(f & NDT_SELECT_KEY)) return "KEY_NEGATE without KEY";
  if (f & NDT_SELECT_BOX)
    for (int a = 0; a < 3; a++)
      if (!(s.box_min[a] <= s.box_max[a])) return "the box needs box_min <= box_max on every axis (no NaN)";
  if (f & NDT_SELECT_RANGE) {
    for (int a = 0; a < 3; a++)
      if (s.centre[a] != s.centre[a]) return "the range centre must not be NaN";
    if (!(s.r_min >= 0.0f) || !(s.r_min <= s.r_max)) return "the range needs 0 <= r_min <= r_max (no NaN)";
  }
  if ((f & NDT_SELECT_KEY) && !(s.key_lo <= s.key_hi)) return "the key range needs key_lo <= key_hi (no NaN)";
  return nullptr;
}

// The launch plan of one cloud (range_plan): blocks of kSelectBlock threads, block b owns points [b * ppb, min(n, (b + 1) * ppb));
// ppb is one pass of the block's threads until that would take more than kSelectMaxBlocks blocks.
inline void select_plan(size_t n, int* blocks, int* ppb) { range_plan(n, kSelectBlock, kSelectMaxBlocks, blocks, ppb); }

}  // namespace ndt
