// Dense QP family: the scalar decisions of the interior-point iteration, stated once for the thread / wavefront text (oh_qp.hip) and the
// block-per-instance kernel (oh_qp_block.hip).  oracle/qp_ipm.py restates them in numpy.  Each function is one expression of the kernels as
// they were, operation for operation: the results keep their bits.
#pragma once
#include <hip/hip_runtime.h>

namespace qp_rules {

// start: s = max(M x + c, 1), lam = mu / s
__device__ __forceinline__ double initial_slack(const double mx_plus_c) { return fmax(mx_plus_c, 1.0); }
__device__ __forceinline__ double initial_multiplier(const double mu, const double s) { return mu / s; }

// an entry of r_d an iteration can go on from (not nan, not inf, not about to be)
__device__ __forceinline__ bool finite(const double v) { return (v == v) && (fabs(v) < 1e300); }
__device__ __forceinline__ bool converged(const double stat, const double feas, const double gap, const double tol) {
  return stat <= tol && feas <= tol && gap <= tol;
}

// diagonal shift of H: relative to its largest diagonal entry; a failed pivot rebuilds H and retries with a 1000 times larger one
constexpr int SHIFT_ATTEMPTS = 8;
constexpr double SHIFT_GROWTH = 1e3;
__device__ __forceinline__ double first_shift(const double dmax) { return 1e-13 * fmax(dmax, 1.0); }

// what the diagonal entry S_ii of the Schur complement A H^{-1} A^T is raised by
__device__ __forceinline__ double schur_regularisation(const double sii) { return 1e-14 * fmax(1.0, sii); }

// fraction to the boundary: the step length at which v (a slack or a multiplier) moving along dv < 0 has lost 99.5 % of itself
__device__ __forceinline__ double boundary_step(const double v, const double dv) { return -0.995 * v / dv; }

// mu of the next iteration (m > 0) from the step lengths taken and the complementarity sum_i s_i lam_i after the step
__device__ __forceinline__ double next_mu(const double ap, const double ad, const double comp, const int m, const double tol) {
  const double am = fmin(ap, ad);
  const double sigma = (am > 0.9) ? 0.1 : ((am > 0.5) ? 0.3 : 0.8);
  return fmax(sigma * comp / m, 1e-2 * tol);
}

}  // namespace qp_rules
