// ndt_pose_cov.hip -- 6x6 covariance of a registered pose (x y z roll pitch yaw), Laplace (scale A^-1) or sandwich
// (A^-1 B_c A^-1): of the handle's source against its target (ndt_pose_covariance), of every pair of the last pairs call in
// one launch (ndt_pairs_pose_covariances), the host algebra alone (ndt_host_pose_covariance) and what the last device call did
// (ndt_diag_pose_covariance).  The definition is in include/ndt_mi355.h; the kernels (k_grad_outer, k_grad_outer_multi) are in
// ndt_kernels.hip.
//   A : minus the symmetrised all-f64 Hessian, from k_hessian64 over the blocks and the points ndt_eval_hessian_f64 walks
//       (derivative_blocks, the source's k2 order), so its bits are that call's
//   B : the sums of the per-point gradients and of their outer products, from k_grad_outer over the same points and blocks
//   one handle : both kernels, two launch_reduce, one wait.  Pairs: k_hessian64 per member (a member's own blocks: the
//       lock-step's k_pairs_step walks a re-ordered source in contiguous runs, another summation order than a handle's), ONE
//       k_grad_outer_multi for all members, two launch_reduce, one wait.
// Nothing of the handle's target, source, grid, last result, statistics or other diag counters is touched: the scratch is the
// partial rows and the pinned result rows every evaluation overwrites, and the handle's pc_* counters.
#include "ndt_internal.hpp"

#include <cmath>

namespace ndtc {

namespace {

// cyclic Jacobi of a symmetric 6x6 (f64, no contraction): eigenvalues in w (unsorted), eigenvectors in the columns of V
void eig6_jacobi(const double* A_in, double w[6], double V[6][6]) {
#pragma clang fp contract(off)
  double A[6][6];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      A[i][j] = A_in[i * 6 + j];
      V[i][j] = (i == j) ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 100; sweep++) {
    double off = 0.0, dia = 0.0;
    for (int i = 0; i < 6; i++) {
      dia += std::fabs(A[i][i]);
      for (int j = i + 1; j < 6; j++) off += std::fabs(A[i][j]);
    }
    // quadratic convergence: below this the next sweep changes nothing that 1/lambda and V diag V^T keep
    if (!(off > 1e-300) || off <= dia * 1e-22) break;
    for (int p = 0; p < 5; p++)
      for (int q = p + 1; q < 6; q++) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        // the smaller root of t^2 + 2 theta t - 1 = 0, without forming theta (eig3_jacobi's form)
        const double d = A[q][q] - A[p][p], b2 = 2.0 * apq;
        const double t = b2 / (d + std::copysign(std::sqrt(d * d + b2 * b2), d));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 6; k++) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 6; k++) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 6; k++) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < 6; i++) w[i] = A[i][i];
}

// steps 7 and 8 of the definition
void pose_cov_algebra(const double* A, const double* B, const double* g, size_t n_found, int method, double scale, double* cov,
                      double* eig_min, double* eig_max, int* flags) {
#pragma clang fp contract(off)
  double w[6], V[6][6];
  eig6_jacobi(A, w, V);
  double lo = w[0], hi = w[0];
  bool nan = false;
  for (int k = 0; k < 36; k++)
    if (!std::isfinite(A[k])) nan = true;  // (the sweeps stop at once on such a matrix: its diagonal says nothing)
  for (int k = 0; k < 6; k++) {
    if (w[k] != w[k]) nan = true;
    if (w[k] < lo) lo = w[k];
    if (w[k] > hi) hi = w[k];
  }
  if (nan) lo = hi = std::nan("");
  if (eig_min) *eig_min = lo;
  if (eig_max) *eig_max = hi;
  const bool indefinite = n_found < 6 || !(lo > 1e-12 * hi);
  if (flags) *flags = indefinite ? NDT_COV_INDEFINITE : 0;
  if (indefinite) {
    for (int k = 0; k < 36; k++) cov[k] = std::nan("");
    return;
  }
  double Ai[6][6];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double s = 0.0;
      for (int k = 0; k < 6; k++) s += V[i][k] * (1.0 / w[k]) * V[j][k];
      Ai[i][j] = s;
    }
  double M[6][6];
  if (method == NDT_COV_LAPLACE) {
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) M[i][j] = scale * Ai[i][j];
  } else {
    double Bc[6][6], T[6][6];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) Bc[i][j] = n_found ? B[i * 6 + j] - g[i] * g[j] / static_cast<double>(n_found) : B[i * 6 + j];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) {
        double s = 0.0;
        for (int k = 0; k < 6; k++) s += Ai[i][k] * Bc[k][j];
        T[i][j] = s;
      }
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) {
        double s = 0.0;
        for (int k = 0; k < 6; k++) s += T[i][k] * Ai[k][j];
        M[i][j] = s;
      }
  }
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) cov[i * 6 + j] = (M[i][j] + M[j][i]) / 2;
}

ndt_status method_checks(const ndt_context* h, const double* cov, int method, double scale) {
  if (!h) return fail(NDT_ERR_INVALID, "null handle");
  if (!cov) return fail(NDT_ERR_INVALID, "null cov");
  if (method != NDT_COV_LAPLACE && method != NDT_COV_SANDWICH) return fail(NDT_ERR_INVALID, "unknown covariance method");
  if (method == NDT_COV_LAPLACE && !(std::isfinite(scale) && scale > 0)) return fail(NDT_ERR_INVALID, "scale must be finite and > 0");
  if (h->comm || h->allreduce)
    return fail(NDT_ERR_INVALID, "the pose covariance is not sharded: the handle has a communicator or an all-reduce hook");
  return NDT_OK;
}

// the Hessian row (slots 7..27) and the gradient-sum row of one member -> its information and its covariance
void finish_member(const double* rowH, const double* rowB, int method, double scale, double* cov, ndt_pose_information* info) {
  ndt_pose_information I;
  ndt::EvalResult H, G;
  double nn = 0.0;
  unpack_row(rowH, true, H, nullptr);
  unpack_row(rowB, true, G, &nn);
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      I.A[i * 6 + j] = -(H.H[i * 6 + j] + H.H[j * 6 + i]) / 2;
      I.B[i * 6 + j] = G.H[i * 6 + j];
    }
  for (int k = 0; k < 6; k++) I.g[k] = G.g[k];
  I.n_found = static_cast<size_t>(nn);
  pose_cov_algebra(I.A, I.B, I.g, I.n_found, method, scale, cov, &I.eig_min, &I.eig_max, &I.flags);
  if (info) *info = I;
}

void h64_params_at(const ndt_context* h, const float* T, ndt::Hess64Params& P) {
  ndt::EvalRequest rq;
  rq.kind = ndt::EVAL_HESSIAN_F64;
  std::memcpy(rq.T, T, sizeof(rq.T));
  ndt::matrix_to_pose(T, rq.p);
  fill_h64_params(rq, ndt::gauss_constants(h->resolution, h->outlier_ratio), kd_radius2(h->resolution), P);
}

}  // namespace

}  // namespace ndtc

extern "C" {

ndt_status ndt_host_pose_covariance(const double* A, const double* B, const double* g, size_t n_found, int method, double scale,
                                    double* cov, double* eig_min, double* eig_max, int* flags) {
  if (!A || !B || !g || !cov) return fail(NDT_ERR_INVALID, "bad arguments");
  if (method != NDT_COV_LAPLACE && method != NDT_COV_SANDWICH) return fail(NDT_ERR_INVALID, "unknown covariance method");
  if (method == NDT_COV_LAPLACE && !(std::isfinite(scale) && scale > 0)) return fail(NDT_ERR_INVALID, "scale must be finite and > 0");
  pose_cov_algebra(A, B, g, n_found, method, scale, cov, eig_min, eig_max, flags);
  return NDT_OK;
}

ndt_status ndt_pose_covariance(ndt_handle h, const float* transform, int method, double scale, double* cov, ndt_pose_information* info) {
  ndt_status s = method_checks(h, cov, method, scale);
  if (s) return s;
  s = ensure_device(h);
  if (s) return s;
  if (!h->grid || !h->target) return fail(NDT_ERR_NO_INPUT, "no input target");
  if (!h->source) return fail(NDT_ERR_NO_INPUT, "no input source");
  h->pc_launches = 0;
  h->pc_blocks = 0;
  s = ensure_host_rows(h, 2);
  if (s) return s;
  const int n = h->source->k2_n();
  double* rows = h->host_result;
  if (h->grid->empty || h->source->n == 0 || n == 0) {  // nothing contributes
    std::memset(rows, 0, 2 * ndt::kEvalStride * sizeof(double));
  } else {
    ndt::Hess64Params P;
    h64_params_at(h, transform ? transform : h->final_T, P);
    const int nblk = ndt::derivative_blocks(n, NDT_DIRECT1);  // ndt_eval_hessian_f64's grid: the same walk
    const size_t part = static_cast<size_t>(nblk) * ndt::kEvalStride;
    const ndt::GridView gv = h->grid->view();
    HIP_TRY(h->partials.reserve(2 * part));
    HIP_TRY(hipMemsetAsync(h->partials.p, 0, 2 * part * sizeof(double), h->stream));
    HIP_TRY(ndt::launch_hessian64(h->source->k2_pts(), n, gv, P, h->search, nullptr, nullptr, 1, nblk, nblk, h->partials.p, h->stream));
    HIP_TRY(ndt::launch_grad_outer(h->source->k2_pts(), n, gv, P, h->search, nblk, h->partials.p + part, h->stream));
    HIP_TRY(ndt::launch_reduce(h->partials.p, nblk, 2, nullptr, rows, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->pc_launches = 1;
    h->pc_blocks = static_cast<size_t>(nblk);
  }
  finish_member(rows, rows + ndt::kEvalStride, method, scale, cov, info);
  return NDT_OK;
}

ndt_status ndt_pairs_pose_covariances(ndt_handle h, const float* transforms, int method, double scale, double* cov,
                                      ndt_pose_information* info) {
  ndt_status s = method_checks(h, cov, method, scale);
  if (s) return s;
  s = ensure_device(h);
  if (s) return s;
  const size_t n_pairs = h->pairs_sources.size();
  if (n_pairs == 0) return fail(NDT_ERR_NO_INPUT, "no pairs: the last ndt_align_pairs* call failed, had no pair or was never made");
  h->pc_launches = 0;
  h->pc_blocks = 0;
  s = ensure_host_rows(h, 2 * n_pairs);
  if (s) return s;
  std::vector<ndt::GridView> views(n_pairs);
  std::vector<ndt::GradOuterMember> mem(n_pairs);
  int max_blocks = 0;
  size_t blocks = 0;
  for (size_t k = 0; k < n_pairs; k++) {
    DeviceCloud* c = h->pairs_sources[k].get();
    if (!c->made_on || !DevPool::instance().retired(c->made_on)) {  // a caller's cloud of another stream (see ndt_pairs_fitness_scores)
      s = cloud_use_on(h, c);
      if (s) return s;
    }
    const DeviceGrid& g = *h->pairs_targets[k];
    ndt::GradOuterMember& m = mem[k];
    m.src = c->pts.p;  // the caller's point order: what a handle holding this pair walks (below its ordering size)
    m.n = static_cast<int>(c->n);
    const bool live = !g.empty && c->n > 0;
    views[k] = live ? g.view() : ndt::GridView{};
    m.blocks = live ? ndt::derivative_blocks(m.n, NDT_DIRECT1) : 0;
    h64_params_at(h, (transforms ? transforms : h->pairs_T.data()) + 16 * k, m.P);
    max_blocks = std::max(max_blocks, m.blocks);
    blocks += static_cast<size_t>(m.blocks);
  }
  double* rows = h->host_result;
  if (max_blocks == 0) {
    std::memset(rows, 0, 2 * n_pairs * ndt::kEvalStride * sizeof(double));
  } else {
    // partial rows: [n_pairs][max_blocks] of the Hessians, then as many of the gradient sums; result rows likewise
    const size_t per = static_cast<size_t>(max_blocks) * ndt::kEvalStride, part = n_pairs * per;
    DevBuf<ndt::GridView> d_views;
    DevBuf<ndt::GradOuterMember> d_mem;
    HIP_TRY(d_views.reserve(n_pairs));
    HIP_TRY(d_mem.reserve(n_pairs));
    HIP_TRY(hipMemcpyAsync(d_views.p, views.data(), n_pairs * sizeof(ndt::GridView), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_mem.p, mem.data(), n_pairs * sizeof(ndt::GradOuterMember), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h->partials.reserve(2 * part));
    HIP_TRY(hipMemsetAsync(h->partials.p, 0, 2 * part * sizeof(double), h->stream));
    for (size_t k = 0; k < n_pairs; k++)
      if (mem[k].blocks)
        HIP_TRY(ndt::launch_hessian64(mem[k].src, mem[k].n, views[k], mem[k].P, h->search, nullptr, nullptr, 1, mem[k].blocks, mem[k].blocks,
                                      h->partials.p + k * per, h->stream));
    HIP_TRY(ndt::launch_grad_outer_multi(d_views.p, d_mem.p, static_cast<int>(n_pairs), h->search, max_blocks, h->partials.p + part,
                                         h->stream));
    HIP_TRY(ndt::launch_reduce(h->partials.p, max_blocks, static_cast<int>(2 * n_pairs), nullptr, rows, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // (also: `views` and `mem` are pageable, the copies have read them)
    h->pc_launches = 1;
    h->pc_blocks = blocks;
  }
  for (size_t k = 0; k < n_pairs; k++)
    finish_member(rows + k * ndt::kEvalStride, rows + (n_pairs + k) * ndt::kEvalStride, method, scale, cov + 36 * k, info ? info + k : nullptr);
  return NDT_OK;
}

ndt_status ndt_diag_pose_covariance(ndt_handle h, size_t* launches, size_t* blocks) {
  if (!h || !launches || !blocks) return fail(NDT_ERR_INVALID, "bad arguments");
  *launches = h->pc_launches;
  *blocks = h->pc_blocks;
  return NDT_OK;
}

}  // extern "C"
