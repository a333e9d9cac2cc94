// ndt_plane.hpp -- the plane of a cloud (ndt_cloud_segment_plane, include/ndt_mi355.h): ONE definition, for the host entries
// (ndt_host_plane_sample / _model / _distance / _fit) and the kernels (ndt_plane.hip), of the sample of a hypothesis, the
// model of a triple, the signed distance of a point and the fit of the refinement; the validity of a spec and the launch
// plans.  Modelled on pcl::SACSegmentation (SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE, RANSAC); PCL's RNG and its early
// exit are not reproducible and no bit parity with PCL is claimed.
// Every f64 operation of the bodies is rounded on its own: they are compiled with contraction off for host and device alike
// (the pragmas below, as ndt_rays.hpp's body), so the two sides differ only where their f64 division or square root would.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "ndt_cloud_ops.hpp"
#include "ndt_mi355.h"

#if defined(__HIPCC__)
#define NDT_PLANE_HD __host__ __device__
#else
#define NDT_PLANE_HD
#endif

namespace ndt {

constexpr int kPlaneBlock = 256;          // threads of a count block = hypotheses of a hypothesis block (four waves)
constexpr int kPlaneTile = 1024;          // points of a tile: 24 KiB of LDS as f64
constexpr int kPlaneMaxBlocks = 4096;     // count blocks of one cloud at most: beyond it the blocks stride over the tiles
constexpr int kPlaneMaxHypotheses = 65536;
constexpr int kPlaneSumBlock = 256;       // threads of a block of the refinement's sums
constexpr int kPlaneSumChunk = 4096;      // points of one such block, until ...
constexpr int kPlaneSumMaxBlocks = 64;    // ... that would take more blocks than this
constexpr double kPlaneDegenerate = 1e-8; // a triple is degenerate unless |u x v|^2 > this * (|u|^2 |v|^2)
constexpr double kPlaneFitRank = 1e-12;   // a fit is taken only when lambda_mid > this * lambda_max

enum { kPlaneValid = 0, kPlaneDegenerateState = 1, kPlaneRejected = 2 };

// What the kernels are handed of a spec: the threshold widened, the unit axis and the cosine of the angle (host, f64, once)
struct PlaneParams {
  double T;
  double axis[3];  // unit; unused without use_axis
  double cos_eps;
  unsigned long long seed;
  int n_hypotheses, use_axis;
};

// the standard splitmix64 finaliser of state + 0x9e3779b97f4a7c15 (Steele, Lea, Flood; Vigna's splitmix64.c): the first
// outputs for seed 0 are 0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f
NDT_PLANE_HD inline unsigned long long plane_mix(unsigned long long x) {
  unsigned long long z = x + 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// index j (0, 1, 2) of hypothesis h over a cloud of n > 0 points
NDT_PLANE_HD inline int plane_sample(unsigned long long seed, int h, int j, int n) {
  const unsigned long long k = seed + 3ull * static_cast<unsigned long long>(h) + static_cast<unsigned long long>(j);
  return static_cast<int>(plane_mix(k) % static_cast<unsigned long long>(n));
}

// n (unit) flipped by the orientation rule; false: REJECTED by the angle test (n is still the oriented normal)
NDT_PLANE_HD inline bool plane_orient(const PlaneParams& P, double n[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (P.use_axis) {
    double dot = (n[0] * P.axis[0] + n[1] * P.axis[1]) + n[2] * P.axis[2];
    if (dot < 0.0) {
      n[0] = -n[0];
      n[1] = -n[1];
      n[2] = -n[2];
      dot = -dot;
    }
    return dot >= P.cos_eps;
  }
  const double last = n[2] != 0.0 ? n[2] : n[1] != 0.0 ? n[1] : n[0];
  if (last < 0.0) {
    n[0] = -n[0];
    n[1] = -n[1];
    n[2] = -n[2];
  }
  return true;
}

// The model of the triple (a, b, c) (stored f32 values); same_index: two of the three indices are equal.  Returns the state;
// coeff = (nx, ny, nz, d), all 0 for a degenerate triple, the oriented plane for a valid or a rejected one.
NDT_PLANE_HD inline int plane_model(const PlaneParams& P, const float a32[3], const float b32[3], const float c32[3], bool same_index,
                                    double coeff[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  coeff[0] = coeff[1] = coeff[2] = coeff[3] = 0.0;
  if (same_index) return kPlaneDegenerateState;
  for (int k = 0; k < 3; k++)
    if (!(__builtin_isfinite(a32[k]) && __builtin_isfinite(b32[k]) && __builtin_isfinite(c32[k]))) return kPlaneDegenerateState;
  const double a[3] = {static_cast<double>(a32[0]), static_cast<double>(a32[1]), static_cast<double>(a32[2])};
  const double u[3] = {static_cast<double>(b32[0]) - a[0], static_cast<double>(b32[1]) - a[1], static_cast<double>(b32[2]) - a[2]};
  const double v[3] = {static_cast<double>(c32[0]) - a[0], static_cast<double>(c32[1]) - a[1], static_cast<double>(c32[2]) - a[2]};
  const double m[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const double len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
  const double uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
  const double vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  if (!(len2 > kPlaneDegenerate * (uu * vv))) return kPlaneDegenerateState;
  const double len = sqrt(len2);
  double n[3] = {m[0] / len, m[1] / len, m[2] / len};
  const bool ok = plane_orient(P, n);
  coeff[0] = n[0];
  coeff[1] = n[1];
  coeff[2] = n[2];
  coeff[3] = -((n[0] * a[0] + n[1] * a[1]) + n[2] * a[2]);
  return ok ? kPlaneValid : kPlaneRejected;
}

// the signed distance s of a point (widened) from the plane (nx, ny, nz, d)
NDT_PLANE_HD inline double plane_distance(double nx, double ny, double nz, double d, double px, double py, double pz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return ((nx * px + ny * py) + nz * pz) + d;
}
NDT_PLANE_HD inline bool plane_inlier(double s, double T) { return -T <= s && s <= T; }

// null = a valid spec, else what is wrong with it
inline const char* plane_spec_error(const ndt_plane_spec& s) {
  if (!std::isfinite(s.distance_threshold) || !(s.distance_threshold > 0.0f)) return "distance_threshold must be finite and > 0";
  if (s.n_hypotheses < 1 || s.n_hypotheses > kPlaneMaxHypotheses) return "n_hypotheses must be 1 ... 65536";
  if (s.use_axis != 0 && s.use_axis != 1) return "use_axis must be 0 or 1";
  if (s.refine != 0 && s.refine != 1) return "refine must be 0 or 1";
  if (s.use_axis) {
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(s.axis[k])) return "the axis must be finite";
    if (s.axis[0] == 0.0f && s.axis[1] == 0.0f && s.axis[2] == 0.0f) return "the axis must not be zero";
    if (!(s.eps_angle >= 0.0f) || !(static_cast<double>(s.eps_angle) <= 1.5707963267948966)) return "eps_angle must lie in 0 ... pi/2";
  }
  return nullptr;
}

// a valid spec as the kernels see it
inline PlaneParams plane_params(const ndt_plane_spec& s) {
  PlaneParams P{};
  P.T = static_cast<double>(s.distance_threshold);
  P.seed = s.seed;
  P.n_hypotheses = s.n_hypotheses;
  P.use_axis = s.use_axis;
  P.cos_eps = 0.0;
  if (s.use_axis) {
    const double x = static_cast<double>(s.axis[0]), y = static_cast<double>(s.axis[1]), z = static_cast<double>(s.axis[2]);
    const double len = std::sqrt((x * x + y * y) + z * z);
    P.axis[0] = x / len;
    P.axis[1] = y / len;
    P.axis[2] = z / len;
    P.cos_eps = std::cos(static_cast<double>(s.eps_angle));
  }
  return P;
}

// The count kernel's grid over a cloud of n points and H hypotheses: tiles of kPlaneTile points x hypothesis blocks of
// kPlaneBlock hypotheses; one block per (tile, hypothesis block) until that would take more than max_blocks, then
// *tile_blocks < *tiles and tile slot t takes the tiles t, t + *tile_blocks, ...  Block b of the cloud: hypothesis block
// b % *hyp_blocks, tile slot b / *hyp_blocks.  n == 0: no block.
inline void plane_plan(size_t n, int n_hypotheses, int max_blocks, int* tiles, int* hyp_blocks, int* tile_blocks) {
  const size_t t = (n + kPlaneTile - 1) / kPlaneTile;
  const int hb = (n_hypotheses + kPlaneBlock - 1) / kPlaneBlock;
  size_t tb = static_cast<size_t>(max_blocks / hb > 1 ? max_blocks / hb : 1);
  if (t < tb) tb = t;
  *tiles = static_cast<int>(t);
  *hyp_blocks = hb;
  *tile_blocks = static_cast<int>(tb);
}

// The plan of the refinement's sums (range_plan), a function of n alone: block b sums the points [b * chunk, min(n, (b + 1) * chunk));
// the rows are added in block order.
inline void plane_sum_plan(size_t n, int* blocks, int* chunk) { range_plan(n, kPlaneSumChunk, kPlaneSumMaxBlocks, blocks, chunk); }

// The fit of the refinement: count inliers, S1 = sum q (x, y, z), S2 = sum q q^T (xx, xy, xz, yy, yz, zz), q = p - a.
// The covariance S2/count - (S1/count)(S1/count)^T is solved by cyclic Jacobi rotations in f64; the normal is the eigenvector
// of the smallest eigenvalue, oriented by the rule of the spec (the angle test is not repeated), d = -n.(a + S1/count).
// false (coeff untouched): count < 3, a number that is not finite, or lambda_mid <= 1e-12 lambda_max.
inline bool plane_fit(const PlaneParams& P, double count, const double S1[3], const double S2[6], const double a[3], double coeff[4],
                      double lambda[3]) {
  if (!(count >= 3.0)) return false;
  const double mu[3] = {S1[0] / count, S1[1] / count, S1[2] / count};
  double A[3][3];
  A[0][0] = S2[0] / count - mu[0] * mu[0];
  A[0][1] = A[1][0] = S2[1] / count - mu[0] * mu[1];
  A[0][2] = A[2][0] = S2[2] / count - mu[0] * mu[2];
  A[1][1] = S2[3] / count - mu[1] * mu[1];
  A[1][2] = A[2][1] = S2[4] / count - mu[1] * mu[2];
  A[2][2] = S2[5] / count - mu[2] * mu[2];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      if (!std::isfinite(A[i][j])) return false;
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 32; sweep++) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    if (off == 0.0) break;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; k++) {  // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; k++) {  // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        A[p][q] = A[q][p] = 0.0;
        for (int k = 0; k < 3; k++) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int o[3] = {0, 1, 2};  // ascending eigenvalues
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 2 - i; j++)
      if (A[o[j]][o[j]] > A[o[j + 1]][o[j + 1]]) {
        const int t = o[j];
        o[j] = o[j + 1];
        o[j + 1] = t;
      }
  const double l0 = A[o[0]][o[0]], l1 = A[o[1]][o[1]], l2 = A[o[2]][o[2]];
  if (!(std::isfinite(l0) && std::isfinite(l1) && std::isfinite(l2))) return false;
  if (!(l1 > kPlaneFitRank * l2)) return false;
  double n[3] = {V[0][o[0]], V[1][o[0]], V[2][o[0]]};
  const double len = std::sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  if (!(len > 0.0) || !std::isfinite(len)) return false;
  for (int k = 0; k < 3; k++) n[k] /= len;
  (void)plane_orient(P, n);
  const double c[3] = {a[0] + mu[0], a[1] + mu[1], a[2] + mu[2]};
  const double d = -((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]);
  if (!(std::isfinite(d) && std::isfinite(n[0]) && std::isfinite(n[1]) && std::isfinite(n[2]))) return false;
  coeff[0] = n[0];
  coeff[1] = n[1];
  coeff[2] = n[2];
  coeff[3] = d;
  if (lambda) {
    lambda[0] = l0;
    lambda[1] = l1;
    lambda[2] = l2;
  }
  return true;
}

}  // namespace ndt
