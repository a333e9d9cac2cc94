// ndt_normals.hpp -- surface normals and curvature of resident clouds (ndt_cloud_estimate_normals, include/ndt_mi355.h): ONE
// definition, for the host entries (ndt_host_normal_from_sums / _keep) and the kernel (ndt_normals.hip), of the step from a
// neighbourhood's sums to the record and of the filter's predicate; the validity of a spec and of a filter, the launch plan.
// Modelled on pcl::NormalEstimation; the class is not in the reference and PCL was not at hand, so no bit parity with PCL is
// claimed: the definitions in include/ndt_mi355.h are the contract.
// Every f64 operation of the bodies is rounded on its own: they are compiled with contraction off for host and device alike
// (the pragmas below, as ndt_plane.hpp's bodies), so the two sides differ only where their f64 division or square root would.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "ndt_cloud_ops.hpp"
#include "ndt_mi355.h"

#if defined(__HIPCC__)
#define NDT_NORMAL_HD __host__ __device__
#else
#define NDT_NORMAL_HD
#endif

namespace ndt {

constexpr int kNormalTeams = 8;           // queries of one pass of a block: one wave, eight lanes per query
constexpr int kNormalMaxBlocks = 4096;    // blocks of one cloud at most: beyond it the blocks stride over the queries
constexpr int kNormalMinK = 3;
constexpr int kNormalMaxK = 256;          // k at most (the per-team list lives in LDS)
constexpr double kNormalCollinear = 1e-12;  // l1 <= this * l2: the neighbourhood is a line
constexpr double kNormalUnitAxis = 1e-12;   // a filter's axis is a unit vector to this (the deskew rule)

// null = a valid spec, else what is wrong with it
inline const char* normal_spec_error(const ndt_normal_spec& s) {
  if (s.method == NDT_NORMAL_KNN) {
    if (s.k < kNormalMinK || s.k > kNormalMaxK) return "k must be 3 ... 256";
  } else if (s.method == NDT_NORMAL_RADIUS) {
    if (!std::isfinite(s.radius) || !(s.radius > 0.0f)) return "the radius must be finite and > 0";
  } else {
    return "unknown normal method";
  }
  if (s.min_neighbors < 3) return "min_neighbors must be at least 3";
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(s.viewpoint[a])) return "the viewpoint must be finite";
  return nullptr;
}

// null = a valid filter, else what is wrong with it
inline const char* normal_filter_error(const ndt_normal_filter& f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (f.flags & ~static_cast<unsigned>(NDT_NORMAL_KEEP_CURVATURE | NDT_NORMAL_KEEP_ANGLE | NDT_NORMAL_KEEP_NEGATE)) return "unknown filter flags";
  if (f.flags & NDT_NORMAL_KEEP_CURVATURE) {
    if (f.curvature_lo != f.curvature_lo || f.curvature_hi != f.curvature_hi) return "the curvature bounds must not be NaN";
    if (f.curvature_lo > f.curvature_hi) return "curvature_lo must not exceed curvature_hi";
  }
  if (f.flags & NDT_NORMAL_KEEP_ANGLE) {
    if (f.cos_lo != f.cos_lo || f.cos_hi != f.cos_hi) return "the cosine bounds must not be NaN";
    if (f.cos_lo > f.cos_hi) return "cos_lo must not exceed cos_hi";
    if (f.cos_lo < 0.0 || f.cos_hi > 1.0) return "the cosine bounds must lie in [0, 1]";
    const double len = std::sqrt((f.axis[0] * f.axis[0] + f.axis[1] * f.axis[1]) + f.axis[2] * f.axis[2]);
    if (!(std::fabs(len - 1.0) <= kNormalUnitAxis)) return "the axis must be a unit vector";
  }
  return nullptr;
}

// The kernel's grid over a cloud of n points: one wave per block, kNormalTeams queries per pass; a block per pass until that
// would take more than max_blocks, then block b takes the passes b, b + blocks, ...
// *qpb: the queries a block works on at most.  n == 0: no block.
inline void normal_plan(size_t n, int max_blocks, int* blocks, int* qpb) {
  const size_t passes = (n + kNormalTeams - 1) / kNormalTeams;
  const size_t b = passes < static_cast<size_t>(max_blocks) ? passes : static_cast<size_t>(max_blocks);
  *blocks = static_cast<int>(b);
  *qpb = b ? static_cast<int>((passes + b - 1) / b) * kNormalTeams : 0;
}

// 3x3 symmetric eigen-decomposition, cyclic Jacobi in f64: eigenvalues ascending in w, eigenvectors in the columns of V.
// (ndt_device.hpp's eig3_jacobi is device-only and its users' bits are pinned; this one serves host and device.)
NDT_NORMAL_HD inline void normal_eig3(const double C[6], double w[3], double V[3][3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 50; sweep++) {
    const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
    const double dia = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
    if (off <= 1e-300 || off <= dia * 1e-16) break;
    for (int pq = 0; pq < 3; pq++) {
      const int p = (pq == 2) ? 1 : 0, q = (pq == 0) ? 1 : 2;
      const double apq = A[p][q];
      if (apq == 0.0) continue;
      // tan of the rotation angle: the root of t^2 + 2 theta t - 1 = 0 that is smaller in magnitude, without forming theta
      const double d = A[q][q] - A[p][p], b2 = 2.0 * apq;
      const double t = b2 / (d + copysign(sqrt(d * d + b2 * b2), d));
      const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
      for (int k = 0; k < 3; k++) {
        const double akp = A[k][p], akq = A[k][q];
        A[k][p] = c * akp - s * akq;
        A[k][q] = s * akp + c * akq;
      }
      for (int k = 0; k < 3; k++) {
        const double apk = A[p][k], aqk = A[q][k];
        A[p][k] = c * apk - s * aqk;
        A[q][k] = s * apk + c * aqk;
      }
      for (int k = 0; k < 3; k++) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
      }
    }
  }
  const double d[3] = {A[0][0], A[1][1], A[2][2]};
  int o[3] = {0, 1, 2};
  if (d[o[0]] > d[o[1]]) { const int t = o[0]; o[0] = o[1]; o[1] = t; }
  if (d[o[1]] > d[o[2]]) { const int t = o[1]; o[1] = o[2]; o[2] = t; }
  if (d[o[0]] > d[o[1]]) { const int t = o[0]; o[0] = o[1]; o[1] = t; }
  double Vs[3][3];
  for (int j = 0; j < 3; j++) {
    w[j] = d[o[j]];
    for (int i = 0; i < 3; i++) Vs[i][j] = V[i][o[j]];
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) V[i][j] = Vs[i][j];
}

// four quiet NaNs
NDT_NORMAL_HD inline void normal_nan_record(float out[4]) {
  const uint32_t q = 0x7fc00000u;
  for (int a = 0; a < 4; a++) {
    float f;
    __builtin_memcpy(&f, &q, sizeof(f));
    out[a] = f;
  }
}

// THE DEFINITION: from the query p (as stored), the number m of its neighbours and their sums about the query
// (S1 = sum e, S2 = sum e e^T as xx xy xz yy yz zz, e = (double)p_j - (double)p) to the record (nx, ny, nz, curvature).
// Returns whether the record is valid (else it is four quiet NaNs); *collinear: a valid record of a neighbourhood that is a line.
NDT_NORMAL_HD inline bool normal_from_sums(int min_neighbors, const double viewpoint[3], const float p[3], int m, const double S1[3],
                                           const double S2[6], float out[4], int* collinear) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  *collinear = 0;
  normal_nan_record(out);
  if (m < min_neighbors || m < 1) return false;
  const double md = static_cast<double>(m);
  const double mu[3] = {S1[0] / md, S1[1] / md, S1[2] / md};
  double C[6];
  C[0] = S2[0] / md - mu[0] * mu[0];
  C[1] = S2[1] / md - mu[0] * mu[1];
  C[2] = S2[2] / md - mu[0] * mu[2];
  C[3] = S2[3] / md - mu[1] * mu[1];
  C[4] = S2[4] / md - mu[1] * mu[2];
  C[5] = S2[5] / md - mu[2] * mu[2];
  for (int a = 0; a < 6; a++)
    if (!(fabs(C[a]) <= 1.7976931348623157e308)) return false;  // NaN or infinite
  double w[3], V[3][3];
  normal_eig3(C, w, V);
  const double t = (w[0] + w[1]) + w[2];
  if (!(t > 0.0)) return false;
  double n[3] = {V[0][0], V[1][0], V[2][0]};
  const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  for (int a = 0; a < 3; a++) n[a] = n[a] / len;
  const double v[3] = {viewpoint[0] - static_cast<double>(p[0]), viewpoint[1] - static_cast<double>(p[1]),
                       viewpoint[2] - static_cast<double>(p[2])};
  const double s = (n[0] * v[0] + n[1] * v[1]) + n[2] * v[2];
  bool flip = s < 0.0;
  if (s == 0.0) {  // the component of largest magnitude (the first on ties) is made positive
    int big = 0;
    if (fabs(n[1]) > fabs(n[big])) big = 1;
    if (fabs(n[2]) > fabs(n[big])) big = 2;
    flip = n[big] < 0.0;
  }
  if (flip)
    for (int a = 0; a < 3; a++) n[a] = -n[a];
  const double l0 = w[0] > 0.0 ? w[0] : 0.0;
  out[0] = static_cast<float>(n[0]);
  out[1] = static_cast<float>(n[1]);
  out[2] = static_cast<float>(n[2]);
  out[3] = static_cast<float>(l0 / t);
  if (out[0] != out[0] || out[1] != out[1] || out[2] != out[2] || out[3] != out[3]) {  // (a solve that did not survive: no normal)
    normal_nan_record(out);
    return false;
  }
  *collinear = (w[1] <= kNormalCollinear * w[2]) ? 1 : 0;
  return true;
}

// the filter's predicate on a stored record: is the point kept?
NDT_NORMAL_HD inline bool normal_keep(const ndt_normal_filter& f, const float r[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (r[0] != r[0] || r[1] != r[1] || r[2] != r[2] || r[3] != r[3]) return false;  // an invalid record is never kept
  bool keep = true;
  if (f.flags & NDT_NORMAL_KEEP_CURVATURE) keep = keep && f.curvature_lo <= r[3] && r[3] <= f.curvature_hi;
  if (f.flags & NDT_NORMAL_KEEP_ANGLE) {
    const double nx = static_cast<double>(r[0]), ny = static_cast<double>(r[1]), nz = static_cast<double>(r[2]);
    const double a = fabs((nx * f.axis[0] + ny * f.axis[1]) + nz * f.axis[2]);
    keep = keep && f.cos_lo <= a && a <= f.cos_hi;
  }
  return (f.flags & NDT_NORMAL_KEEP_NEGATE) ? !keep : keep;
}

}  // namespace ndt
