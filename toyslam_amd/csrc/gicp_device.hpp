// gicp_device.hpp -- device building blocks the GICP kernel units share (gicp_kernels.hip: point targets; gicp_grid.hip: voxel
// targets), in an anonymous namespace like ndt_device.hpp.  Every product and sum is spelled out and contraction is off, so
// a value is the same bits whichever unit computed it.
#pragma once
#include "gicp_kernels.hpp"
#include "ndt_device.hpp"

namespace gicp {
namespace {

// [Eigen] Matrix4f * Vector4f (column by column): row r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3 * 1
__device__ __forceinline__ void matvec_eigen(const float* T12, float x, float y, float z, float& ox, float& oy, float& oz) {
#pragma clang fp contract(off)
  ox = ((T12[0] * x + T12[1] * y) + T12[2] * z) + T12[3] * 1.0f;
  oy = ((T12[4] * x + T12[5] * y) + T12[6] * z) + T12[7] * 1.0f;
  oz = ((T12[8] * x + T12[9] * y) + T12[10] * z) + T12[11] * 1.0f;
}

__device__ __forceinline__ void load_sym(const double* __restrict__ c6, double C[3][3]) {
  C[0][0] = c6[0]; C[0][1] = c6[1]; C[0][2] = c6[2];
  C[1][0] = c6[1]; C[1][1] = c6[3]; C[1][2] = c6[4];
  C[2][0] = c6[2]; C[2][1] = c6[4]; C[2][2] = c6[5];
}

// The Mahalanobis matrix of one correspondence (gicp_omp_impl.hpp:436-452): maha9 = (R C1 R^T + C2)^-1 as f32, row-major; C1 / C2:
// the packed covariances of the source point and of its target (a point's, or a voxel's).  One lane's work.
__device__ __forceinline__ void mahalanobis_store(const double* __restrict__ c1_6, const double* __restrict__ c2_6, const Rot3d& R,
                                                  float* __restrict__ maha9) {
#pragma clang fp contract(off)
  double C1[3][3], C2[3][3], M[3][3], tmp[3][3], inv[3][3];
  load_sym(c1_6, C1);
  load_sym(c2_6, C2);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) M[r][c] = (R.m[r * 3] * C1[0][c] + R.m[r * 3 + 1] * C1[1][c]) + R.m[r * 3 + 2] * C1[2][c];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++)
      tmp[r][c] = ((M[r][0] * R.m[c * 3] + M[r][1] * R.m[c * 3 + 1]) + M[r][2] * R.m[c * 3 + 2]) + C2[r][c];
  ndt::inv3_cofactor(tmp, inv);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) maha9[r * 3 + c] = static_cast<float>(inv[r][c]);
}

}  // namespace
}  // namespace gicp
