// ndt_deskew.hpp -- the motion compensation of ndt_cloud_deskew (include/ndt_mi355.h), ONE definition for the host entry
// (ndt_host_deskew_point) and the kernel (ndt_deskew.hip), the validity of a motion, and the launch plan both sides use.
// Every f64 operation of the body is rounded on its own: deskew_point is compiled with contraction off for host and device
// alike (the pragma below, as ndt_select.hpp's range test), so the two sides differ only by their libraries' sin / cos.
#pragma once
#include <cmath>
#include <cstddef>

#include "ndt_cloud_ops.hpp"
#include "ndt_mi355.h"

#if defined(__HIPCC__)
#define NDT_DESKEW_HD __host__ __device__
#else
#define NDT_DESKEW_HD
#endif

namespace ndt {

constexpr int kDeskewBlock = 256;       // threads of a block (four waves)
constexpr int kDeskewMaxBlocks = 1024;  // blocks of one cloud at most: beyond it points_per_block grows

// One record: (x, y, z) as stored and its time t -> q.  dt = t_end - t_begin, computed once by the caller.
// Returns 0: moved, 1: a coordinate is not finite, q = the input as it is (the caller copies the record's own bits),
// 2: a finite point without a finite time, q = NaN.
NDT_DESKEW_HD inline int deskew_point(const ndt_deskew_motion& m, double dt, float x, float y, float z, double t, float q[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))) {
    q[0] = x;
    q[1] = y;
    q[2] = z;
    return 1;
  }
  if (!__builtin_isfinite(t)) {
    q[0] = q[1] = q[2] = __builtin_nanf("");
    return 2;
  }
  const double s = (t - m.t_ref) / dt;
  const double theta = s * m.angle;
#if defined(__HIP_DEVICE_COMPILE__)
  double sn, cs;
  sincos(theta, &sn, &cs);
#else
  const double sn = std::sin(theta), cs = std::cos(theta);
#endif
  const double p[3] = {static_cast<double>(x), static_cast<double>(y), static_cast<double>(z)};
  const double* k = m.axis;
  const double kxp[3] = {k[1] * p[2] - k[2] * p[1], k[2] * p[0] - k[0] * p[2], k[0] * p[1] - k[1] * p[0]};
  const double kp = (k[0] * p[0] + k[1] * p[1]) + k[2] * p[2];
  const double omc = 1.0 - cs;
#if defined(__clang__)
#pragma unroll
#endif
  for (int a = 0; a < 3; a++) {
    const double v = ((p[a] * cs + kxp[a] * sn) + (k[a] * kp) * omc) + s * m.tau_ref[a];
    q[a] = static_cast<float>(v);
  }
  return 0;
}

// null = a valid motion, else what is wrong with it
inline const char* deskew_motion_error(const ndt_deskew_motion& m) {
  const double v[11] = {m.t_begin, m.t_end, m.t_ref, m.axis[0], m.axis[1], m.axis[2], m.angle, m.tau_ref[0], m.tau_ref[1], m.tau_ref[2], 0.0};
  for (double x : v)
    if (!std::isfinite(x)) return "every field of a motion must be finite";
  if (!(m.t_end > m.t_begin)) return "a motion needs t_end > t_begin";
  if (!(m.angle >= 0.0 && m.angle <= 3.14159265358979323846)) return "a motion's angle must lie in [0, pi]";
  const double len = std::sqrt((m.axis[0] * m.axis[0] + m.axis[1] * m.axis[1]) + m.axis[2] * m.axis[2]);
  if (!(std::fabs(len - 1.0) <= 1e-12)) return "a motion's axis must have length 1";
  return nullptr;
}

// The launch plan of one cloud (range_plan): blocks of kDeskewBlock threads, block b owns points [b * ppb, min(n, (b + 1) * ppb));
// ppb is one pass of the block's threads until that would take more than max_blocks blocks.
inline void deskew_plan(size_t n, int max_blocks, int* blocks, int* ppb) { range_plan(n, kDeskewBlock, max_blocks, blocks, ppb); }

}  // namespace ndt
