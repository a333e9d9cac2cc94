// ndt_voxel_finish.hpp -- the two halves of VoxelGridCovariance::applyFilter for ONE voxel, shared by the kernel units that
// finish voxels: K1's grid build (ndt_grid_kernels.hip) and the accumulating target (ndt_accumulate.hip).  The first pass
// is a set of running sums (VoxelSums), the second (finish_voxel) reads nothing but those sums and the count -- which is what
// lets a target keep a voxel's sums and continue them with the next scan.
#pragma once
#include "ndt_device.hpp"

namespace ndt {
namespace {

// First-pass sums of one voxel (applyFilter's first loop, _impl.hpp:209-263): mean_ += pt ; cov_ += pt*pt^T with cov_
// seeded Identity (.h:107); centroid.head<4>() += pt in f32 (:240-244).  Points must be added in ascending point
// order: the f64 sums then round exactly like the reference's sequential pass.
struct VoxelSums {
  double sx = 0, sy = 0, sz = 0;
  double cxx = 1, cxy = 0, cxz = 0, cyy = 1, cyz = 0, czz = 1;
  float fx = 0, fy = 0, fz = 0;
  __device__ __forceinline__ void add(float px, float py, float pz) {
#pragma clang fp contract(off)
    const double x = px, y = py, z = pz;
    sx += x; sy += y; sz += z;
    cxx += x * x; cxy += x * y; cxz += x * z; cyy += y * y; cyz += y * z; czz += z * z;
    fx += px; fy += py; fz += pz;
  }
};

// Second pass of applyFilter for one voxel (_impl.hpp:282-367): mean, covariance with the reference's quirks, 3x3
// eigen-solve, eigenvalue inflation, inverse, validity; writes the 64-B record, the centroid, the look-up table slot
// and (dump mode) the per-leaf outputs.  o: leaf ordinal, r: record ordinal (-1: fewer than min_pts points).
// Returns whether the voxel is valid for the DIRECT searches.
__device__ __forceinline__ bool finish_voxel(const VoxelSums& S, int cnt, int o, int r, int cell, int min_pts, double eig_ratio,
                                             VoxelRec* __restrict__ recs, VoxelSide* __restrict__ centroids, int* __restrict__ lut,
                                             const GridGeom& geom, const FinalizeDump& dump) {
  // No FMA contraction: the reference target (SSE4.2) never fuses, and its covariance formula (_impl.hpp:329-330)
  // cancels catastrophically when the coordinates are large against the voxel size, so a single fused multiply-add
  // shows up in the 7th digit of cov / icov.
#pragma clang fp contract(off)
  const double sx = S.sx, sy = S.sy, sz = S.sz;
  const double cxx = S.cxx, cxy = S.cxy, cxz = S.cxz, cyy = S.cyy, cyz = S.cyz, czz = S.czz;
  float fx = S.fx, fy = S.fy, fz = S.fz;
  const double n = cnt;
  const double ps[3] = {sx, sy, sz};
  const double mean[3] = {sx / n, sy / n, sz / n};  // :293
  fx /= static_cast<float>(cnt); fy /= static_cast<float>(cnt); fz /= static_cast<float>(cnt);  // :289

  double cov[3][3] = {{cxx, cxy, cxz}, {cxy, cyy, cyz}, {cxz, cyz, czz}};
  double icov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  double evals[3] = {0, 0, 0};
  int nr_points = cnt;
  bool is_valid = false;

  if (cnt >= min_pts) {
    // :329-330
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) cov[i][j] = (cov[i][j] - 2 * (ps[i] * mean[j])) / n + mean[i] * mean[j];
    const double f = (n - 1.0) / n;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) cov[i][j] *= f;
    double w[3] = {0, 0, 0}, V[3][3];
    // The eigen-decomposition is needed only (a) to reject a voxel with a non-positive eigenvalue and (b) to inflate
    // the small eigenvalues of a flat or thin one; a voxel that is PROVABLY positive definite with
    // lambda_min >= eig_ratio lambda_max goes straight to the inverse of the untouched covariance -- bit for bit what
    // the full path computes for it.  Proof used: leading minors > 0 (Sylvester); lambda_max <= trace;
    // lambda_min = det / (lambda_mid lambda_max) >= det / (trace / 2)^2.  (Dump mode reports the eigenvalues: full path.)
    bool well_conditioned = false;
    if (!dump.nr_points) {
      const double m2 = cov[0][0] * cov[1][1] - cov[0][1] * cov[0][1];
      const double det = cov[0][0] * (cov[1][1] * cov[2][2] - cov[1][2] * cov[1][2]) - cov[0][1] * (cov[0][1] * cov[2][2] - cov[1][2] * cov[0][2]) +
                         cov[0][2] * (cov[0][1] * cov[1][2] - cov[1][1] * cov[0][2]);
      const double tr = cov[0][0] + cov[1][1] + cov[2][2];
      well_conditioned = cov[0][0] > 0 && m2 > 1e-12 * cov[0][0] * cov[1][1] && det > 0 && 4.0 * det > 1.05 * eig_ratio * tr * tr * tr && eig_ratio < 0.9;
    }
    if (well_conditioned) {
      w[0] = w[1] = w[2] = 1.0;  // (placeholders: positive, no inflation)
    } else {
      eig3_jacobi(cov, w, V);
    }
    if (w[0] < 0 || w[1] < 0 || w[2] <= 0) {  // :337-341
      nr_points = -1;
    } else {
      const double min_ev = eig_ratio * w[2];  // :345-356
      if (!well_conditioned && w[0] < min_ev) {
        w[0] = min_ev;
        if (w[1] < min_ev) w[1] = min_ev;
        double Vi[3][3], VL[3][3];
        inv3_cofactor(V, Vi);
        for (int i = 0; i < 3; i++)
          for (int j = 0; j < 3; j++) VL[i][j] = V[i][j] * w[j];
        for (int i = 0; i < 3; i++)
          for (int j = 0; j < 3; j++) cov[i][j] = (VL[i][0] * Vi[0][j] + VL[i][1] * Vi[1][j]) + VL[i][2] * Vi[2][j];
      }
      evals[0] = w[0]; evals[1] = w[1]; evals[2] = w[2];
      inv3_cofactor(cov, icov);  // :359
      double mx = -DBL_MAX, mn = DBL_MAX;
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { mx = fmax(mx, icov[i][j]); mn = fmin(mn, icov[i][j]); }
      if (mx == static_cast<double>(INFINITY) || mn == -static_cast<double>(INFINITY)) nr_points = -1;  // :360-364
    }
    {
      // Every voxel that reached min_points_per_voxel gets a record: the reference pushes its
      // centroid to the KD-tree BEFORE the eigenvalue / inverse checks (_impl.hpp:302-326 vs
      // :337-341,:360-364), so KDTREE search still returns a rejected voxel (trap 7), with the
      // icov_ it was left with (zero, or the inf-bearing inverse).  DIRECT searches skip it
      // (nr_points = -1): the LUT entry is lut_rejected(r).
      VoxelRec rec;
      rec.mean[0] = mean[0]; rec.mean[1] = mean[1]; rec.mean[2] = mean[2];
      const float c00 = static_cast<float>(icov[0][0]), c01 = static_cast<float>(icov[0][1]), c02 = static_cast<float>(icov[0][2]);
      const float c11 = static_cast<float>(icov[1][1]), c12 = static_cast<float>(icov[1][2]), c22 = static_cast<float>(icov[2][2]);
      rec.c[0] = c00; rec.c[1] = c01; rec.c[2] = c02;
      rec.c[3] = c12; rec.c[4] = c11; rec.c[5] = c22;
      rec.n = cnt;
      rec.pad = 0;
      rec.c01c11[0] = c01; rec.c01c11[1] = c11;
      recs[r] = rec;
      VoxelSide side;
      side.cx = fx; side.cy = fy; side.cz = fz; side.pad = 0.0f;
      side.icov[0] = icov[0][0]; side.icov[1] = icov[0][1]; side.icov[2] = icov[0][2];
      side.icov[3] = icov[1][1]; side.icov[4] = icov[1][2]; side.icov[5] = icov[2][2];
      centroids[r] = side;
      const int entry = (nr_points >= min_pts) ? r : lut_rejected(r);
      is_valid = nr_points >= min_pts;
      if (geom.hash_bits) {
        // sparse grid: claim a slot of the hash table (keys are unique: one insert per voxel)
        int2* tab = reinterpret_cast<int2*>(lut);
        const unsigned mask = (1u << geom.hash_bits) - 1u;
        for (unsigned hslot = hash_slot(cell, geom.hash_bits);; hslot = (hslot + 1u) & mask) {
          const int seen = atomicCAS(&tab[hslot].x, -1, cell);
          if (seen == -1 || seen == cell) {
            tab[hslot].y = entry;
            break;
          }
        }
      } else {
        // the cell's slot in the padded look-up table
        const int c = cell;
        const int cz = c / geom.mul[2], cy = (c - cz * geom.mul[2]) / geom.mul[1], cx = c - cz * geom.mul[2] - cy * geom.mul[1];
        const long long slot = static_cast<long long>(cx + kLutBorder) + static_cast<long long>(cy + kLutBorder) * geom.pmul[1] +
                               static_cast<long long>(cz + kLutBorder) * geom.pmul[2];
        lut[slot] = entry;
      }
    }
  }
  if (dump.nr_points) {
    dump.nr_points[o] = nr_points;
    for (int k = 0; k < 3; k++) {
      dump.mean[o * 3 + k] = mean[k];
      dump.evals[o * 3 + k] = evals[k];
    }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        dump.cov[o * 9 + i * 3 + j] = cov[i][j];
        dump.icov[o * 9 + i * 3 + j] = icov[i][j];
      }
  }
  return is_valid;
}

}  // namespace
}  // namespace ndt
