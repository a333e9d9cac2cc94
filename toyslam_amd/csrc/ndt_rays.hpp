// ndt_rays.hpp -- the ray of ndt_target_accumulate_clear_rays (include/ndt_mi355.h), ONE definition for the host entry
// (ndt_host_ray_cells) and the kernel (k_acc_rays, ndt_acc_rays.hip), the validity of a spec, and the launch plan.
// Every f64 operation of the body is rounded on its own: ray_walk is compiled with contraction off for host and device alike
// (the pragma below, as ndt_deskew.hpp's body), so the two sides differ only where their f64 division or square root would.
#pragma once
#include <cmath>
#include <cstddef>

#include "ndt_mi355.h"

#if defined(__HIPCC__)
#define NDT_RAYS_HD __host__ __device__
#else
#define NDT_RAYS_HD
#endif

namespace ndt {

constexpr int kRayBlock = 256;        // threads of a block (four waves)
constexpr int kRayMaxBlocks = 1024;   // blocks of one call at most: beyond it the threads stride over the points
constexpr int kRayLattice = 1 << 20;  // cells of [-2^20, 2^20) on every axis (kAccCellBias)
constexpr double kRayMaxCells = 65536.0;  // max_range / resolution at most: a walk is at most 3 x 65537 steps

// One ray from the sensor origin o to the posed point p (both f32 values, widened), on the lattice of leaf L: visit(i, j, k)
// for the start cell and for every cell entered while t <= t_end = 1 - margin / len.  Returns the cells visited, or -1 when
// the ray is not cast (len == 0, len outside [min_range, max_range], t_end <= 0).  A walk ends where it leaves the lattice; a
// start outside it visits nothing.
template <class Visit>
NDT_RAYS_HD inline long long ray_walk(const float o32[3], const float p32[3], double L, double margin, double min_range, double max_range,
                                      double* len_out, Visit&& visit) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double o[3] = {static_cast<double>(o32[0]), static_cast<double>(o32[1]), static_cast<double>(o32[2])};
  const double d[3] = {static_cast<double>(p32[0]) - o[0], static_cast<double>(p32[1]) - o[1], static_cast<double>(p32[2]) - o[2]};
  const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  if (len_out) *len_out = len;
  if (!(len > 0.0) || !(len >= min_range) || !(len <= max_range)) return -1;
  const double t_end = 1.0 - margin / len;
  if (!(t_end > 0.0)) return -1;
  const double inf = __builtin_huge_val(), lim = static_cast<double>(kRayLattice);
  int m[3], f[3], s[3];
  double t[3];
  for (int k = 0; k < 3; k++) {
    const double q = floor(o[k] / L);
    if (!(q >= -lim - 1.0 && q <= lim)) return 0;
    int c = static_cast<int>(q);
    while (static_cast<double>(c) * L > o[k]) c--;         // (the quotient is rounded, the products are exact)
    while (static_cast<double>(c + 1) * L <= o[k]) c++;
    if (c < -kRayLattice || c >= kRayLattice) return 0;
    m[k] = c;
    s[k] = d[k] > 0.0 ? 1 : d[k] < 0.0 ? -1 : 0;
    f[k] = c + (s[k] > 0 ? 1 : 0);
    t[k] = s[k] ? (static_cast<double>(f[k]) * L - o[k]) / d[k] : inf;
  }
  long long n = 1;
  visit(m[0], m[1], m[2]);
  for (;;) {
    int a = 0;
    if (t[1] < t[a]) a = 1;
    if (t[2] < t[a]) a = 2;
    if (!(t[a] <= t_end)) break;
    m[a] += s[a];
    f[a] += s[a];
    if (m[a] < -kRayLattice || m[a] >= kRayLattice) break;
    t[a] = (static_cast<double>(f[a]) * L - o[a]) / d[a];
    n++;
    visit(m[0], m[1], m[2]);
  }
  return n;
}

// null = a valid spec for a target of this resolution, else what is wrong with it
inline const char* ray_spec_error(const ndt_ray_spec& s, float resolution) {
  if (!std::isfinite(s.min_range) || !std::isfinite(s.max_range) || !std::isfinite(s.margin)) return "every length of a ray spec must be finite";
  if (!(s.min_range >= 0.f)) return "a ray spec needs min_range >= 0";
  if (!(s.min_range <= s.max_range)) return "a ray spec needs min_range <= max_range";
  if (!(s.max_range > 0.f)) return "a ray spec needs max_range > 0";
  if (!(s.margin >= 0.f)) return "a ray spec needs margin >= 0";
  if (s.min_rays < 1) return "a ray spec needs min_rays >= 1";
  if (!(std::isfinite(resolution) && resolution > 0.f)) return "the resolution must be finite and positive";
  if (!(static_cast<double>(s.max_range) / static_cast<double>(resolution) <= kRayMaxCells)) return "a ray spec needs max_range / resolution <= 65536";
  return nullptr;
}

// The grid of k_acc_rays over the n points of a call (all its clouds together): one thread per point up to max_blocks
// blocks, beyond which thread g takes the points g, g + blocks * 256, ...; *passes is the most points one thread takes.
inline void ray_plan(size_t n, int max_blocks, int* blocks, int* passes) {
  const size_t b = (n + kRayBlock - 1) / kRayBlock;
  const size_t g = b < static_cast<size_t>(max_blocks) ? b : static_cast<size_t>(max_blocks);
  *blocks = static_cast<int>(g);
  *passes = g ? static_cast<int>((n + g * kRayBlock - 1) / (g * kRayBlock)) : 0;
}

}  // namespace ndt
