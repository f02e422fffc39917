// The rules of the point-mass interior-point iteration (oh_pointmass.hip: k_pm_solve and k_pm_solve_wave; what a kernel keeps written out is listed there): constraint rows,
// the stage terms of a knot, the Riccati step of a stage, the row step of a knot, the verdict, the barrier update, the Euler step and the seed.
// Values in, values out: where they are kept (work arrays in HBM, or the registers of the knot's lane) is the calling kernel's business.
// Algorithm and constants mirror oracle/pointmass_ipm.py.
#pragma once

#include "oh_device.h"
#include "oh_kernels.h"

#define PM_GO_ON (-1)  // pm_verdict: none yet

// c (9 rows) and the nonzero Jacobian entries of stage t: box rows are +-e_j, obstacle row is 2 (y - o)
OH_DEV void pm_cons(const PmParams& P, const double* x, const double ox, const double oy, double (&c)[9], double& jx, double& jy) {
  c[0] = x[0] + P.ylim; c[1] = P.ylim - x[0];
  c[2] = x[1] + P.ylim; c[3] = P.ylim - x[1];
  c[4] = x[2] + P.vlim; c[5] = P.vlim - x[2];
  c[6] = x[3] + P.vlim; c[7] = P.vlim - x[3];
  const double dx = x[0] - ox, dy = x[1] - oy;
  c[8] = dx * dx + dy * dy - P.safe_sq;
  jx = 2.0 * dx; jy = 2.0 * dy;
}
// y = J^T w for the 9 rows (J rows: +e0,-e0,+e1,-e1,+e2,-e2,+e3,-e3,(jx,jy,0,0))
OH_DEV void pm_JTw(const double (&w)[9], const double jx, const double jy, double (&y)[4]) {
  y[0] = w[0] - w[1] + jx * w[8];
  y[1] = w[2] - w[3] + jy * w[8];
  y[2] = w[4] - w[5];
  y[3] = w[6] - w[7];
}
// d = J v
OH_DEV void pm_Jv(const double* v, const double jx, const double jy, double (&d)[9]) {
  d[0] = v[0]; d[1] = -v[0]; d[2] = v[1]; d[3] = -v[1];
  d[4] = v[2]; d[5] = -v[2]; d[6] = v[3]; d[7] = -v[3];
  d[8] = jx * v[0] + jy * v[1];
}

// rc = c - s with the obstacle row's Jacobian entries
OH_DEV void pm_residuals(const PmParams& P, const double* x, const double ox, const double oy, const double (&s)[9], double (&rc)[9], double& jx, double& jy) {
  double c[9];
  pm_cons(P, x, ox, oy, c, jx, jy);
  for (int i = 0; i < 9; ++i) rc[i] = c[i] - s[i];
}

// x <- A x + B a,  A = [[I, dt I],[0, I]],  B = [0; dt I]
OH_DEV void pm_euler(const double dt, double (&x)[4], const double a0, const double a1) {
  const double n0 = x[0] + dt * x[2], n1 = x[1] + dt * x[3], n2 = x[2] + dt * a0, n3 = x[3] + dt * a1;
  x[0] = n0; x[1] = n1; x[2] = n2; x[3] = n3;
}

// seed: velocities from x0's dY block (v: [t][2]), v_0 = dcurr, controls = velocity differences, states by roll-out from pb = (curr, dcurr).
// keep_state(t, x): knot t's state; keep_control(t, a0, a1): the control between knots t and t + 1
template <class KeepState, class KeepControl>
OH_DEV void pm_seed(const PmParams& P, const double* pb, const double* v, KeepState keep_state, KeepControl keep_control) {
  const int T = P.T;
  double vprev[2] = {pb[2], pb[3]};
  double x[4] = {pb[0], pb[1], pb[2], pb[3]};
  keep_state(0, x);
  for (int t = 0; t < T - 1; ++t) {
    double v1[2] = {v[2 * (t + 1)], v[2 * (t + 1) + 1]};
    if (P.fix_vf && t == T - 2) v1[0] = v1[1] = 0.0;  // terminal row dy_{T-1} = 0 (point_mass_planner.py:34-35)
    const double a0 = (v1[0] - vprev[0]) / P.dt, a1 = (v1[1] - vprev[1]) / P.dt;
    keep_control(t, a0, a1);
    pm_euler(P.dt, x, a0, a1);
    keep_state(t + 1, x);
    vprev[0] = v1[0]; vprev[1] = v1[1];
  }
}
// slacks off their rows by at least 1e-2, multipliers on the central path
OH_DEV void pm_first_rows(const double (&c)[9], const double mu, double (&s)[9], double (&lam)[9]) {
  for (int i = 0; i < 9; ++i) {
    s[i] = fmax(c[i], 1e-2);
    lam[i] = mu / s[i];
  }
}

// ---- the stage terms of knot t ------------------------------------------------------------------------------------------------------------------
struct PmKnot {
  double jx, jy;        // the obstacle row's Jacobian entries
  double rc[9];         // c - s
  double lx[4], q[4];   // gradient of the Lagrangian, and of the condensed stage cost
  double Q0, Q1, Q5, Q10, Q15;  // Q_t = diag(2 wt, 2 wt, 2 w_vel, 2 w_vel) + J^T Sig J: entries [0], [1] = [4], [5], [10], [15] of the row-major 4x4
};
OH_DEV void pm_Q16(const double Q0, const double Q1, const double Q5, const double Q10, const double Q15, double (&Q)[16]) {
  for (int j = 0; j < 16; ++j) Q[j] = 0.0;
  Q[0] = Q0; Q[5] = Q5; Q[1] = Q[4] = Q1; Q[10] = Q10; Q[15] = Q15;
}
// Returns the knot's share of the objective (state terms; the caller adds w |a_t|^2).  counts: the knot's rows enter the maxima fe, co behind feas and
// compl (every knot but 0, whose state is pinned: its Q, q are never used either).  fmax drops NaNs: a NaN row residual (a NaN obstacle entry, say) is
// carried apart from the maxima in `bad`, for every knot's rows, knot 0 included.
OH_DEV double pm_stage_terms(const PmParams& P, const int t, const bool counts, const double (&x)[4], const double (&s)[9], const double (&lam)[9],
                             const double g0, const double g1, const double o0, const double o1, const double mu, PmKnot& k, double& fe, double& co, bool& bad) {
  pm_residuals(P, x, o0, o1, s, k.rc, k.jx, k.jy);
  const double jx = k.jx, jy = k.jy;
  const double wt = (P.final_only && t < P.T - 1) ? 0.0 : 1.0;  // tracking on every knot (MPC) or on the last one only (planner)
  const double gx[4] = {-2.0 * wt * (g0 - x[0]), -2.0 * wt * (g1 - x[1]), 2.0 * P.w_vel * x[2], 2.0 * P.w_vel * x[3]};
  const double f = wt * ((g0 - x[0]) * (g0 - x[0]) + (g1 - x[1]) * (g1 - x[1])) + P.w_vel * (x[2] * x[2] + x[3] * x[3]);
  double sig[9], wq[9], jl[4], jq[4];
  for (int i = 0; i < 9; ++i) {
    sig[i] = lam[i] / s[i];
    wq[i] = mu / s[i] - sig[i] * k.rc[i];
    if (counts) { fe = fmax(fe, fabs(k.rc[i])); co = fmax(co, lam[i] * s[i]); }
    bad = bad || !(k.rc[i] == k.rc[i]) || !(lam[i] * s[i] == lam[i] * s[i]);
  }
  pm_JTw(lam, jx, jy, jl);
  pm_JTw(wq, jx, jy, jq);
  for (int j = 0; j < 4; ++j) { k.lx[j] = gx[j] - jl[j]; k.q[j] = gx[j] - jq[j]; }
  k.Q0 = 2.0 * wt + sig[0] + sig[1] + sig[8] * jx * jx;
  k.Q5 = 2.0 * wt + sig[2] + sig[3] + sig[8] * jy * jy;
  k.Q1 = sig[8] * jx * jy;
  k.Q10 = 2.0 * P.w_vel + sig[4] + sig[5];
  k.Q15 = 2.0 * P.w_vel + sig[6] + sig[7];
  return f;
}

// ---- the Riccati step of stage t ----------------------------------------------------------------------------------------------------------------
struct PmCostToGo {  // of stage t + 1 going in, of stage t coming out
  double Pm[16], pv[4], padj[4];  // value Hessian and gradient; the adjoint of the dynamics rows (for the stationarity residual)
};
struct PmExpansion {  // what a_t sees of stage t + 1
  double PA[16], Qux[8], q00, q01, q11, qu0, qu1, gu0, gu1;
};
// Before the symmetrisation: P_t = Q_t + A^T P A + Qux^T K ;  p_t = q_t + A^T p + Qux^T k ;  padj_t = lx_t + A^T padj ;  (A^T M)[r] = M[r] (+ dt M[r-2] for r >= 2).
// PINNED: K is the fixed feedback [0 0 -1/dt 0; 0 0 0 -1/dt] with k = 0, which adds K^T Qux + K^T Quu K to P and K^T qu to p, and the control
// gradient flows into the state adjoint: padj += K^T gu
template <bool PINNED>
OH_DEV void pm_cost_to_go(const double dt, const double (&Q)[16], const double (&q)[4], const double (&lx)[4], const PmExpansion& e, const double (&Kt)[8],
                          const double (&kt)[2], const PmCostToGo& V, double (&Pn)[16], double (&pn)[4], double (&pa)[4]) {
  for (int r = 0; r < 4; ++r)
    for (int cc = 0; cc < 4; ++cc) {
      double v = e.PA[4 * r + cc];
      if (r >= 2) v += dt * e.PA[4 * (r - 2) + cc];
      v += e.Qux[r] * Kt[cc] + e.Qux[4 + r] * Kt[4 + cc];                       // Qux^T K
      if constexpr (PINNED) v += Kt[r] * e.Qux[cc] + Kt[4 + r] * e.Qux[4 + cc];  // K^T Qux
      Pn[4 * r + cc] = Q[4 * r + cc] + v;
    }
  const double kf = -1.0 / dt;
  if constexpr (PINNED) { Pn[10] += kf * kf * e.q00; Pn[11] += kf * kf * e.q01; Pn[14] += kf * kf * e.q01; Pn[15] += kf * kf * e.q11; }  // K^T Quu K
  for (int r = 0; r < 4; ++r) {
    double v = V.pv[r], va = V.padj[r];
    if (r >= 2) { v += dt * V.pv[r - 2]; va += dt * V.padj[r - 2]; }
    if constexpr (PINNED) pn[r] = q[r] + v;
    else pn[r] = q[r] + v + e.Qux[r] * kt[0] + e.Qux[4 + r] * kt[1];
    pa[r] = lx[r] + va;
  }
  if constexpr (PINNED) {
    pn[2] += kf * e.qu0; pn[3] += kf * e.qu1;
    pa[2] += kf * e.gu0; pa[3] += kf * e.gu1;
  }
}
// V: stage t + 1's on entry (unread at t = T - 1), stage t's on return.  Kt, kt: the feedback da_t = k + K dx_t (unset at t = T - 1, which has no
// control).  stat: running maximum of the control gradients of the Lagrangian.  (a0, a1) = a_t acts between knots t and t + 1.
template <class KeepGain>
OH_DEV void pm_riccati_step(const PmParams& P, const int t, const double (&Q)[16], const double (&q)[4], const double (&lx)[4], const double a0, const double a1,
                            PmCostToGo& V, double& stat, KeepGain keep_gain) {
  const double dt = P.dt, w = P.w_acc;
  if (t == P.T - 1) {
    for (int j = 0; j < 16; ++j) V.Pm[j] = Q[j];
    for (int j = 0; j < 4; ++j) { V.pv[j] = q[j]; V.padj[j] = lx[j]; }
    return;
  }
  const double* Pm = V.Pm;
  PmExpansion e;
  // control gradient of the Lagrangian: 2 w a + B^T padj, B^T z = dt (z2, z3)
  const bool pinned = P.fix_vf && t == P.T - 2;  // a_{T-2} = -v_{T-2} / dt is a function of the state, not a free control
  e.gu0 = 2.0 * w * a0 + dt * V.padj[2]; e.gu1 = 2.0 * w * a1 + dt * V.padj[3];
  if (!pinned) stat = fmax(stat, fmax(fabs(e.gu0), fabs(e.gu1)));
  // Quu = R + B^T P B = 2w I + dt^2 P[2:4,2:4] ; Qux = B^T P A = dt (P[2:4,:] A)
  for (int r = 0; r < 4; ++r) {  // P A : column j<2 same as P, column j>=2: P[:,j] + dt P[:,j-2]
    e.PA[4 * r + 0] = Pm[4 * r + 0]; e.PA[4 * r + 1] = Pm[4 * r + 1];
    e.PA[4 * r + 2] = Pm[4 * r + 2] + dt * Pm[4 * r + 0];
    e.PA[4 * r + 3] = Pm[4 * r + 3] + dt * Pm[4 * r + 1];
  }
  e.q00 = 2.0 * w + dt * dt * Pm[10]; e.q01 = dt * dt * Pm[11]; e.q11 = 2.0 * w + dt * dt * Pm[15];
  for (int j = 0; j < 4; ++j) { e.Qux[j] = dt * e.PA[8 + j]; e.Qux[4 + j] = dt * e.PA[12 + j]; }
  e.qu0 = 2.0 * w * a0 + dt * V.pv[2]; e.qu1 = 2.0 * w * a1 + dt * V.pv[3];
  // 2x2 Cholesky solve
  // (reciprocal square roots and products: the 21 divisions of the textbook substitution were half the instructions of a knot step)
  const double i00 = rsqrt(e.q00), l10 = e.q01 * i00, i11 = rsqrt(e.q11 - l10 * l10);
  double Pn[16], pn[4], pa[4], Kt[8], kt[2];
  if (pinned) {
    for (int j = 0; j < 8; ++j) Kt[j] = 0.0;
    Kt[2] = Kt[4 + 3] = -1.0 / dt;
    kt[0] = kt[1] = 0.0;
    keep_gain(Kt, kt);
    pm_cost_to_go<true>(dt, Q, q, lx, e, Kt, kt, V, Pn, pn, pa);
  } else {
    for (int j = 0; j < 4; ++j) {
      const double y0 = e.Qux[j] * i00, y1 = (e.Qux[4 + j] - l10 * y0) * i11;
      const double z1 = y1 * i11, z0 = (y0 - l10 * z1) * i00;
      Kt[j] = -z0; Kt[4 + j] = -z1;
    }
    const double y0 = e.qu0 * i00, y1 = (e.qu1 - l10 * y0) * i11;
    const double z1 = y1 * i11, z0 = (y0 - l10 * z1) * i00;
    kt[0] = -z0; kt[1] = -z1;
    keep_gain(Kt, kt);
    pm_cost_to_go<false>(dt, Q, q, lx, e, Kt, kt, V, Pn, pn, pa);
  }
  for (int r = 0; r < 4; ++r)
    for (int cc = 0; cc < 4; ++cc) V.Pm[4 * r + cc] = 0.5 * (Pn[4 * r + cc] + Pn[4 * cc + r]);
  for (int j = 0; j < 4; ++j) { V.pv[j] = pn[j]; V.padj[j] = pa[j]; }
}

// da_t = k + K dx_t, then dx_{t+1} = A dx_t + B da_t
OH_DEV void pm_newton_step(const double dt, const double (&K)[8], const double (&k)[2], double (&dx)[4], double& da0, double& da1) {
  da0 = k[0]; da1 = k[1];
  for (int j = 0; j < 4; ++j) { da0 += K[j] * dx[j]; da1 += K[4 + j] * dx[j]; }
  pm_euler(dt, dx, da0, da1);
}

// ---- the row step of a knot: ds = J dx + (c - s), dl = (mu / s - lam) - (lam / s) ds; counts: its rows bound the fraction-to-the-boundary steps ap, ad ----
OH_DEV void pm_row_step(const double (&dx)[4], const double jx, const double jy, const double (&rc)[9], const double (&s)[9], const double (&lam)[9], const double mu,
                        const bool counts, double (&ds)[9], double (&dl)[9], double& ap, double& ad) {
  double d[9];
  pm_Jv(dx, jx, jy, d);
  for (int i = 0; i < 9; ++i) {
    ds[i] = d[i] + rc[i];
    dl[i] = (mu / s[i] - lam[i]) - (lam[i] / s[i]) * ds[i];
    if (counts) {
      if (ds[i] < 0.0) ap = fmin(ap, -0.995 * s[i] / ds[i]);
      if (dl[i] < 0.0) ad = fmin(ad, -0.995 * lam[i] / dl[i]);
    }
  }
}

// ---- the verdict on an evaluation: PM_GO_ON or the status the solve ends with ---------------------------------------------------------------------
OH_DEV int pm_verdict(const PmParams& P, const int it, const double stat, const double fval, const double feas, const double compl_) {
  if (!(stat == stat) || !(fval == fval) || !(fabs(fval) < 1e300) || !(feas == feas) || !(compl_ == compl_)) return OH_STATUS_NUMERICAL;
  if (stat <= P.tol && feas <= P.tol && compl_ <= P.tol) return OH_STATUS_CONVERGED;
  // No feasible plan (the reference: IPOPT's Infeasible_Problem_Detected -> did_solve() False, solver.py:407-412): the obstacle is a parameter of every knot,
  // so a problem whose pinned knot is fine can still have none -- the obstacle lands where the mass cannot leave in time.  The infeasible-start iteration
  // then shows its textbook signature: the slack residual stalls at the violation it cannot remove while the multipliers of those rows leave every bound
  // (lam s from 1e-1 to 1e8 in three steps, 1e240 a dozen steps later; oracle/pointmass_ipm.py has the same rule).  A healthy run keeps lam s at the size of
  // the barrier parameter (<= 1).
  if (compl_ > 1e6 && feas > 1e3 * P.tol) return OH_STATUS_INFEASIBLE;
  return it == P.max_iter ? OH_STATUS_MAX_ITER : PM_GO_ON;
}

// ---- the barrier update: gap = sum of s lam over the rows of knots 1 .. T - 1 after the step --------------------------------------------------------
OH_DEV double pm_barrier(const PmParams& P, double gap, const double ap, const double ad) {
  gap /= (double)(9 * (P.T - 1));
  const double am = fmin(ap, ad);
  const double sigma = (am > 0.9) ? 0.1 : ((am > 0.5) ? 0.3 : 0.8);
  return fmax(sigma * gap, 1e-2 * P.tol);
}
