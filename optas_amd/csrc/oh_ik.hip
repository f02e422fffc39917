// Inverse-kinematics family (BASELINE config 1, example/example.py:13-60):
//
//     min_q  w ||q - q_nominal||^2   s.t.  h(q) = p_goal - p_link(q) = 0   (builder.py:354: rhs - lhs)
//                                          lo <= q <= up                     (enforce_model_limits, builder.py:471-509)
//
// One thread owns one instance for its whole solve (nx = ndof <= 7: everything lives in registers): bound-constrained
// augmented Lagrangian, inner iteration = projected Newton (Bertsekas active set) with the exact Hessian of the
// augmented Lagrangian -- 2wI + rho Jp^T Jp - sum_k y_k d2p_k, the position curvature is y.(omega_a x Jp_b) -- a
// Levenberg shift when the masked matrix is not positive definite, and Armijo backtracking along the projected arc.
// The state machine is the one oracle/ik_al.py restates in numpy (test infrastructure only).
#include <hip/hip_runtime.h>

#include "oh_device.h"
#include "oh_kernels.h"

namespace {

template <int N>
OH_DEV void ik_eval(const oh_chain* __restrict__ ch, const double (&q)[N], double (&e)[3], double (&Jp)[N][3], double (&om)[N][3]) {
  double R[9], p[3], pj[N][3];
  fk_chain<N>(ch, q, R, p, om, pj);
  double t[3];
  mv3(R, ch->p_tool, t);
  e[0] = p[0] + t[0]; e[1] = p[1] + t[1]; e[2] = p[2] + t[2];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (ch->jtype[k] == 0) {
      const double d[3] = {e[0] - pj[k][0], e[1] - pj[k][1], e[2] - pj[k][2]};
      cross3(om[k], d, Jp[k]);
    } else {
      Jp[k][0] = om[k][0]; Jp[k][1] = om[k][1]; Jp[k][2] = om[k][2];
      om[k][0] = om[k][1] = om[k][2] = 0.0;
    }
  }
}

template <int N>
OH_DEV double ik_merit(const IkParams& P, const double (&q)[N], const double (&qn)[N], const double (&e)[3], const double (&pg)[3],
                       const double (&lam)[3], double rho) {
  double c = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) c += (q[i] - qn[i]) * (q[i] - qn[i]);
  double m = P.w * c;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double h = pg[k] - e[k];
    m += lam[k] * h + 0.5 * rho * h * h;
  }
  return m;
}

template <int N>
__global__ void __launch_bounds__(64) k_ik_solve(const oh_chain* __restrict__ ch, IkParams P, int B, const double* __restrict__ x0,
                                                 const double* __restrict__ par, double* __restrict__ x, double* __restrict__ f,
                                                 double* __restrict__ kkt, int* __restrict__ iters, int* __restrict__ status,
                                                 double* __restrict__ mult) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  constexpr int NP = N * (N + 1) / 2;
  double q[N], qn[N], pg[3], lam[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < N; ++i) {
    qn[i] = par[(size_t)b * (N + 3) + i];
    q[i] = fmin(fmax(x0[(size_t)b * N + i], P.lo[i]), P.up[i]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) pg[k] = par[(size_t)b * (N + 3) + N + k];
  double e[3], Jp[N][3], om[N][3];
  ik_eval<N>(ch, q, e, Jp, om);
  int it = 1, st = OH_STATUS_MAX_ITER;
  double rho = P.rho0, shift = 0.0, h_prev = 1e300;
  double grad[N];
  bool act[N];
  {
    // non-finite seed / parameters: report, do not iterate (fmax-based norms would hide a NaN)
    const double m_init = ik_merit<N>(P, q, qn, e, pg, lam, rho);
    if (!(m_init == m_init) || !(fabs(m_init) < 1e300)) st = OH_STATUS_NUMERICAL;
  }
  while (it < P.max_iter && st != OH_STATUS_NUMERICAL) {
    // ---- inner: projected Newton on the augmented Lagrangian ----
    while (it < P.max_iter) {
      double y[3], hmax = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double h = pg[k] - e[k];
        y[k] = lam[k] + rho * h;
        hmax = fmax(hmax, fabs(h));
      }
      double pgn = 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        grad[i] = 2.0 * P.w * (q[i] - qn[i]) - (Jp[i][0] * y[0] + Jp[i][1] * y[1] + Jp[i][2] * y[2]);
        act[i] = (q[i] <= P.lo[i] && grad[i] > 0.0) || (q[i] >= P.up[i] && grad[i] < 0.0);
        if (!act[i]) pgn = fmax(pgn, fabs(grad[i]));
      }
      if (pgn <= fmax(0.5 * P.tol, fmin(1e-2, 0.1 * hmax))) break;
      double H[NP];
#pragma unroll
      for (int a = 0; a < N; ++a) {
#pragma unroll
        for (int c = 0; c <= a; ++c) {
          double t[3];
          cross3(om[c], Jp[a], t);
          double v = rho * (Jp[a][0] * Jp[c][0] + Jp[a][1] * Jp[c][1] + Jp[a][2] * Jp[c][2]) - (y[0] * t[0] + y[1] * t[1] + y[2] * t[2]);
          if (a == c) v += 2.0 * P.w;
          H[tri(a, c)] = v;
        }
      }
      double L[NP];
      for (;;) {
#pragma unroll
        for (int a = 0; a < N; ++a) {
#pragma unroll
          for (int c = 0; c <= a; ++c) {
            double v = H[tri(a, c)];
            if (a == c) v += shift;
            if (act[a] || act[c]) v = (a == c) ? 1.0 : 0.0;
            L[tri(a, c)] = v;
          }
        }
        if (chol_packed<N>(L, 0.0)) break;
        shift = fmax(10.0 * shift, 1e-3 * rho);
        if (!(shift < 1e300)) break;
      }
      double d[N];
#pragma unroll
      for (int i = 0; i < N; ++i) d[i] = act[i] ? 0.0 : -grad[i];
      fsub<N>(L, d);
      bsub<N>(L, d);
      const double m0 = ik_merit<N>(P, q, qn, e, pg, lam, rho);
      double alpha = 1.0;
      bool ok = false;
      double qt[N], et[3], Jt[N][3], ot[N][3];
      for (int ls = 0; ls < 30; ++ls) {
        double slope = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          qt[i] = fmin(fmax(q[i] + alpha * d[i], P.lo[i]), P.up[i]);
          slope += grad[i] * (qt[i] - q[i]);
        }
        ik_eval<N>(ch, qt, et, Jt, ot);
        ++it;
        // (rounding slack: that of the merit itself plus what the rounding of the link position, a few 1e-16, is worth through the effective
        //  multiplier y = lam + rho h -- without the second part one instance in 65 536 of the config-1 batch, with |y| ~ 10 and a step that
        //  predicts a decrease of 1e-17, failed the test at every step length until the iteration cap; round 3)
        if (ik_merit<N>(P, qt, qn, et, pg, lam, rho) <= m0 + 1e-4 * slope + 4e-16 * fmax(1.0, fabs(m0)) + 8e-16 * (fabs(y[0]) + fabs(y[1]) + fabs(y[2]))) {
          ok = true;
          break;
        }
        alpha *= 0.5;
        if (it >= P.max_iter) break;
      }
      if (!ok) {
        shift = fmax(10.0 * shift, 1e-3 * rho);
        if (shift > 1e12 * rho) {
          st = OH_STATUS_NUMERICAL;
          break;
        }
        continue;
      }
      shift = shift > 1e-12 ? 0.1 * shift : 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        q[i] = qt[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          Jp[i][k] = Jt[i][k];
          om[i][k] = ot[i][k];
        }
      }
      e[0] = et[0]; e[1] = et[1]; e[2] = et[2];
    }
    if (st == OH_STATUS_NUMERICAL) break;
    // ---- outer: multiplier update ----
    double hn = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double h = pg[k] - e[k];
      lam[k] += rho * h;
      hn = fmax(hn, fabs(h));
    }
    double stat = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double g = 2.0 * P.w * (q[i] - qn[i]) - (Jp[i][0] * lam[0] + Jp[i][1] * lam[1] + Jp[i][2] * lam[2]);
      const bool a = (q[i] <= P.lo[i] && g > 0.0) || (q[i] >= P.up[i] && g < 0.0);
      if (!a) stat = fmax(stat, fabs(g));
    }
    if (hn <= P.tol_feas && stat <= P.tol) {
      st = OH_STATUS_CONVERGED;
      break;
    }
    if (hn > 0.1 * h_prev) rho = fmin(rho * 10.0, 1e8);
    h_prev = hn;
  }
  // ---- results in the reference's form: v = [q - lo; up - q; h; -h] >= 0 (optimization.py:47-51) ----
  double stat = 0.0, feas = 0.0, cost = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) feas = fmax(feas, fabs(pg[k] - e[k]));
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double g = 2.0 * P.w * (q[i] - qn[i]) - (Jp[i][0] * lam[0] + Jp[i][1] * lam[1] + Jp[i][2] * lam[2]);
    const bool lo = q[i] <= P.lo[i] && g > 0.0, up = q[i] >= P.up[i] && g < 0.0;
    if (!(lo || up)) stat = fmax(stat, fabs(g));
    cost += (q[i] - qn[i]) * (q[i] - qn[i]);
    if (x) x[(size_t)b * N + i] = q[i];
    if (mult) {
      mult[(size_t)b * (3 + 2 * N) + 3 + i] = lo ? g : 0.0;
      mult[(size_t)b * (3 + 2 * N) + 3 + N + i] = up ? -g : 0.0;
    }
  }
  if (mult) {
#pragma unroll
    for (int k = 0; k < 3; ++k) mult[(size_t)b * (3 + 2 * N) + k] = -lam[k];
  }
  if (f) f[b] = P.w * cost;
  if (kkt) {
    kkt[(size_t)b * 3 + 0] = stat;
    kkt[(size_t)b * 3 + 1] = feas;
    kkt[(size_t)b * 3 + 2] = 0.0;  // multipliers are non-zero only on rows that sit exactly on their bound
  }
  if (iters) iters[b] = it;
  if (status) status[b] = st;
}

// ---- full-pose goal (oh_ik_desc.orientation): seven equality rows -------------------------------------------------------------------
//
//     h = [p_goal - p_link(q); quat_goal - quat_link(q)]     (the reference's second equality on get_global_link_quaternion, literal sign)
//
// quat_link is the reference's chain product (xyzw, half-angle factors, quat0[k], quat_tool: oh_fkjac_unit.h), smooth in q; its column for a
// revolute joint j is Jq_j = 1/2 (om_j, 0) (x) quat and, for a not after b on the chain, d2quat / dq_a dq_b = 1/4 (om_a, 0) (x) (om_b, 0) (x) quat.
// Neither is formed: with y = [yp; yq] the effective multipliers and wq = vec(yq (x) conj(quat)),
//     yq . Jq_j          = 1/2 om_j . wq
//     Jq_a . Jq_c        = 1/4 |quat|^2 om_a . om_c                               (right multiplication by quat is |quat| times a rotation of R^4)
//     yq . d2quat_{c,a}  = 1/4 ((om_c x om_a) . wq - (om_c . om_a) (yq . quat))   ((om_c,0) (x) (om_a,0) = (om_c x om_a, -om_c . om_a))
// so the quaternion rows cost one 3-vector and two scalars per iteration on top of the position kernel's registers.  A prismatic joint has om = 0.
// The state machine is k_ik_solve's, which stays as it is (its code objects are the parent's); tests/pose_ik_ref.py restates this one in numpy.
template <int N>
OH_DEV void ik_pose_eval(const oh_chain* __restrict__ ch, const double (&q)[N], double (&v)[7], double (&Jp)[N][3], double (&om)[N][3]) {
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0}, quat[4] = {0, 0, 0, 1}, pj[N][3];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double t[3], qn[4];
    mv3(R, ch->p0[k], t);
    p[0] += t[0]; p[1] += t[1]; p[2] += t[2];
    if (!ch->r0ident[k]) {
      double Rn[9];
      mm3(R, ch->R0[k], Rn);
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    }
    pj[k][0] = p[0]; pj[k][1] = p[1]; pj[k][2] = p[2];
    qmul(quat, ch->quat0[k], qn);
    if (ch->jtype[k] == 0) {
      double sh, chh;
      sincos_joint(0.5 * q[k], &sh, &chh);  // half angle for the quaternion, the full angle from it for Rodrigues (as fk_jac_unit)
      const double s = 2.0 * sh * chh, c = 1.0 - 2.0 * sh * sh;
      if (ch->axcode[k] != 0) rot_principal_right(R, ch->axcode[k], s, c, om[k]);
      else rot_axis_right(R, ch->axis[k], s, c, om[k]);
      const double qa[4] = {sh * ch->axis[k][0], sh * ch->axis[k][1], sh * ch->axis[k][2], chh};
      qmul(qn, qa, quat);
    } else {
      mv3(R, ch->axis[k], om[k]);
      p[0] += om[k][0] * q[k]; p[1] += om[k][1] * q[k]; p[2] += om[k][2] * q[k];
      quat[0] = qn[0]; quat[1] = qn[1]; quat[2] = qn[2]; quat[3] = qn[3];
    }
  }
  double t[3];
  mv3(R, ch->p_tool, t);
  v[0] = p[0] + t[0]; v[1] = p[1] + t[1]; v[2] = p[2] + t[2];
  qmul(quat, ch->quat_tool, &v[3]);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (ch->jtype[k] == 0) {
      const double d[3] = {v[0] - pj[k][0], v[1] - pj[k][1], v[2] - pj[k][2]};
      cross3(om[k], d, Jp[k]);
    } else {
      Jp[k][0] = om[k][0]; Jp[k][1] = om[k][1]; Jp[k][2] = om[k][2];
      om[k][0] = om[k][1] = om[k][2] = 0.0;
    }
  }
}

template <int N>
OH_DEV double ik_pose_merit(const IkParams& P, const double (&q)[N], const double (&qn)[N], const double (&v)[7], const double (&g)[7],
                            const double (&lam)[7], double rho) {
  double c = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) c += (q[i] - qn[i]) * (q[i] - qn[i]);
  double m = P.w * c;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const double h = g[k] - v[k];
    m += lam[k] * h + 0.5 * rho * h * h;
  }
  return m;
}

// wq = vec(yq (x) conj(quat)): yq . (1/2 (om, 0) (x) quat) = 1/2 om . wq
OH_DEV void ik_pose_wq(const double* yq, const double* quat, double (&wq)[3]) {
  wq[0] = yq[0] * quat[3] - yq[1] * quat[2] + yq[2] * quat[1] - yq[3] * quat[0];
  wq[1] = yq[0] * quat[2] + yq[1] * quat[3] - yq[2] * quat[0] - yq[3] * quat[1];
  wq[2] = yq[1] * quat[0] - yq[0] * quat[1] + yq[2] * quat[3] - yq[3] * quat[2];
}

// gradient in q_i of f + y . h: 2 w (q_i - qn_i) - Jp_i . yp - Jq_i . yq
template <int N>
OH_DEV double ik_pose_grad(const IkParams& P, const int i, const double (&q)[N], const double (&qn)[N], const double (&Jp)[N][3],
                           const double (&om)[N][3], const double (&y)[7], const double (&wq)[3]) {
  return 2.0 * P.w * (q[i] - qn[i]) - (Jp[i][0] * y[0] + Jp[i][1] * y[1] + Jp[i][2] * y[2]) - 0.5 * (om[i][0] * wq[0] + om[i][1] * wq[1] + om[i][2] * wq[2]);
}

template <int N>
__global__ void __launch_bounds__(64) k_ik_pose_solve(const oh_chain* __restrict__ ch, IkParams P, int B, const double* __restrict__ x0,
                                                      const double* __restrict__ par, double* __restrict__ x, double* __restrict__ f,
                                                      double* __restrict__ kkt, int* __restrict__ iters, int* __restrict__ status,
                                                      double* __restrict__ mult) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  constexpr int NP = N * (N + 1) / 2;
  double q[N], qn[N], g[7], lam[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < N; ++i) {
    qn[i] = par[(size_t)b * (N + 7) + i];
    q[i] = fmin(fmax(x0[(size_t)b * N + i], P.lo[i]), P.up[i]);
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) g[k] = par[(size_t)b * (N + 7) + N + k];
  double v[7], Jp[N][3], om[N][3];  // v = [p_link; quat_link]
  ik_pose_eval<N>(ch, q, v, Jp, om);
  int it = 1, st = OH_STATUS_MAX_ITER;
  double rho = P.rho0, shift = 0.0, h_prev = 1e300;
  double grad[N];
  bool act[N];
  {
    const double m_init = ik_pose_merit<N>(P, q, qn, v, g, lam, rho);
    if (!(m_init == m_init) || !(fabs(m_init) < 1e300)) st = OH_STATUS_NUMERICAL;
  }
  while (it < P.max_iter && st != OH_STATUS_NUMERICAL) {
    // ---- inner: projected Newton on the augmented Lagrangian ----
    while (it < P.max_iter) {
      double y[7], hmax = 0.0, ysum = 0.0;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const double h = g[k] - v[k];
        y[k] = lam[k] + rho * h;
        hmax = fmax(hmax, fabs(h));
        ysum += fabs(y[k]);
      }
      double wq[3];
      ik_pose_wq(&y[3], &v[3], wq);
      double pgn = 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        grad[i] = ik_pose_grad<N>(P, i, q, qn, Jp, om, y, wq);
        act[i] = (q[i] <= P.lo[i] && grad[i] > 0.0) || (q[i] >= P.up[i] && grad[i] < 0.0);
        if (!act[i]) pgn = fmax(pgn, fabs(grad[i]));
      }
      if (pgn <= fmax(0.5 * P.tol, fmin(1e-2, 0.1 * hmax))) break;
      // 2wI + rho J^T J - sum_k y_k d2p_k - sum_k y_{3+k} d2quat_k  (h = goal - value: both curvatures enter with the minus sign)
      const double kq = 0.25 * (rho * (v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6]) + (y[3] * v[3] + y[4] * v[4] + y[5] * v[5] + y[6] * v[6]));
      double H[NP];
#pragma unroll
      for (int a = 0; a < N; ++a) {
#pragma unroll
        for (int c = 0; c <= a; ++c) {
          double t[3], u[3];
          cross3(om[c], Jp[a], t);
          cross3(om[c], om[a], u);
          double e = rho * (Jp[a][0] * Jp[c][0] + Jp[a][1] * Jp[c][1] + Jp[a][2] * Jp[c][2]) - (y[0] * t[0] + y[1] * t[1] + y[2] * t[2]);
          e += kq * (om[a][0] * om[c][0] + om[a][1] * om[c][1] + om[a][2] * om[c][2]) - 0.25 * (u[0] * wq[0] + u[1] * wq[1] + u[2] * wq[2]);
          if (a == c) e += 2.0 * P.w;
          H[tri(a, c)] = e;
        }
      }
      double L[NP];
      for (;;) {
#pragma unroll
        for (int a = 0; a < N; ++a) {
#pragma unroll
          for (int c = 0; c <= a; ++c) {
            double e = H[tri(a, c)];
            if (a == c) e += shift;
            if (act[a] || act[c]) e = (a == c) ? 1.0 : 0.0;
            L[tri(a, c)] = e;
          }
        }
        if (chol_packed<N>(L, 0.0)) break;
        shift = fmax(10.0 * shift, 1e-3 * rho);
        if (!(shift < 1e300)) break;
      }
      double d[N];
#pragma unroll
      for (int i = 0; i < N; ++i) d[i] = act[i] ? 0.0 : -grad[i];
      fsub<N>(L, d);
      bsub<N>(L, d);
      const double m0 = ik_pose_merit<N>(P, q, qn, v, g, lam, rho);
      double alpha = 1.0;
      bool ok = false;
      double qt[N], vt[7], Jt[N][3], ot[N][3];
      for (int ls = 0; ls < 30; ++ls) {
        double slope = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          qt[i] = fmin(fmax(q[i] + alpha * d[i], P.lo[i]), P.up[i]);
          slope += grad[i] * (qt[i] - q[i]);
        }
        ik_pose_eval<N>(ch, qt, vt, Jt, ot);
        ++it;
        // (rounding slack as in k_ik_solve, |y| summed over all seven rows)
        if (ik_pose_merit<N>(P, qt, qn, vt, g, lam, rho) <= m0 + 1e-4 * slope + 4e-16 * fmax(1.0, fabs(m0)) + 8e-16 * ysum) {
          ok = true;
          break;
        }
        alpha *= 0.5;
        if (it >= P.max_iter) break;
      }
      if (!ok) {
        shift = fmax(10.0 * shift, 1e-3 * rho);
        if (shift > 1e12 * rho) {
          st = OH_STATUS_NUMERICAL;
          break;
        }
        continue;
      }
      shift = shift > 1e-12 ? 0.1 * shift : 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        q[i] = qt[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          Jp[i][k] = Jt[i][k];
          om[i][k] = ot[i][k];
        }
      }
#pragma unroll
      for (int k = 0; k < 7; ++k) v[k] = vt[k];
    }
    if (st == OH_STATUS_NUMERICAL) break;
    // ---- outer: multiplier update ----
    double hn = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const double h = g[k] - v[k];
      lam[k] += rho * h;
      hn = fmax(hn, fabs(h));
    }
    double wq[3];
    ik_pose_wq(&lam[3], &v[3], wq);
    double stat = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double gi = ik_pose_grad<N>(P, i, q, qn, Jp, om, lam, wq);
      const bool a = (q[i] <= P.lo[i] && gi > 0.0) || (q[i] >= P.up[i] && gi < 0.0);
      if (!a) stat = fmax(stat, fabs(gi));
    }
    if (hn <= P.tol_feas && stat <= P.tol) {
      st = OH_STATUS_CONVERGED;
      break;
    }
    if (hn > 0.1 * h_prev) rho = fmin(rho * 10.0, 1e8);
    h_prev = hn;
  }
  // ---- results in the reference's form: v = [q - lo; up - q; h; -h] >= 0 (optimization.py:47-51), h of seven rows ----
  constexpr int NM = 7 + 2 * N;
  double stat = 0.0, feas = 0.0, cost = 0.0, wq[3];
  ik_pose_wq(&lam[3], &v[3], wq);
#pragma unroll
  for (int k = 0; k < 7; ++k) feas = fmax(feas, fabs(g[k] - v[k]));
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double gi = ik_pose_grad<N>(P, i, q, qn, Jp, om, lam, wq);
    const bool lo = q[i] <= P.lo[i] && gi > 0.0, up = q[i] >= P.up[i] && gi < 0.0;
    if (!(lo || up)) stat = fmax(stat, fabs(gi));
    cost += (q[i] - qn[i]) * (q[i] - qn[i]);
    if (x) x[(size_t)b * N + i] = q[i];
    if (mult) {
      mult[(size_t)b * NM + 7 + i] = lo ? gi : 0.0;
      mult[(size_t)b * NM + 7 + N + i] = up ? -gi : 0.0;
    }
  }
  if (mult) {
#pragma unroll
    for (int k = 0; k < 7; ++k) mult[(size_t)b * NM + k] = -lam[k];
  }
  if (f) f[b] = P.w * cost;
  if (kkt) {
    kkt[(size_t)b * 3 + 0] = stat;
    kkt[(size_t)b * 3 + 1] = feas;
    kkt[(size_t)b * 3 + 2] = 0.0;
  }
  if (iters) iters[b] = it;
  if (status) status[b] = st;
}

// ---- the state machine over a rows policy (oh_ik_set_axis_goal is its first user) -----------------------------------------------------------------
//
// The two kernels above differ only in their equality rows.  ik_rows_solve is their state machine once more, with everything that knows the rows
// behind a policy `Rows`; a new goal is a new policy, and the two older kernels can move onto theirs without touching the iteration (they stay as
// they are for now: their code objects are the parent's).  A policy states, for h = goal - value(q) with NH rows, y the effective multipliers:
//     NH                                  number of rows; p rows are [q_nominal (N); goal (NH)], multiplier rows [-lam (NH); z_lo (N); z_up (N)]
//     eval(ch, P, q, v, Jp, om)           value v[NH] and the chain's linear columns Jp / joint axes om (om = 0 for a prismatic joint)
//     Dual, dual(y, v, rho, D)            whatever of y the next two need, formed once per multiplier vector
//     jty(i, Jp, om, y, D)                (J^T y)_i, J the Jacobian of the value: the rows' share of the gradient is -jty
//     hess(a, c, Jp, om, v, y, rho, D)    rho (J^T J)_{ac} - sum_k y_k d2 value_k / dq_a dq_c for c not after a on the chain
// The |y| sum of the Armijo slack and the feasibility norms run over all NH rows here.
//
// Axis goal: value = [p_link; u], u = R_link a, a the unit link-frame axis (P.a_tool = R_tool a: fk_chain's R stops before the tool).  With
// yu = y[3..5]:
//     du/dq_j = om_j x u                          yu . du/dq_j = om_j . (u x yu)
//     (om_a x u) . (om_c x u) = |u|^2 om_a . om_c - (om_a . u)(om_c . u)           (|u|^2 kept as computed, like |quat|^2 in the pose kernel)
//     d2u/dq_c dq_a = om_c x (om_a x u)           yu . d2u_{c,a} = (yu . om_a)(om_c . u) - (yu . u)(om_a . om_c)         (c not after a)
// so with D.c = u x yu, D.r = rho u + yu, D.k = rho |u|^2 + yu . u the axis rows add  om_i . D.c  to jty and  D.k om_a . om_c - (om_c . u)(om_a . D.r)
// to hess: one 3-vector per multiplier vector and dot products, no 3 x n Jacobian.  |u| = 1, so the three rows have rank 2 (u^T du/dq = 0); no
// system in the rows is solved, and lam along u moves only at second order for a unit goal.  The goal is literal: one that is not of unit length is
// infeasible as posed and ends with a non-zero status.  tests/axis_ik_ref.py restates the iteration in numpy with the Jacobian written out.
struct IkAxisRows {
  static constexpr int NH = 6;
  struct Dual {
    double c[3], r[3], k;
  };

  template <int N>
  static OH_DEV void eval(const oh_chain* __restrict__ ch, const IkParams& P, const double (&q)[N], double (&v)[NH], double (&Jp)[N][3], double (&om)[N][3]) {
    double R[9], p[3], pj[N][3];
    fk_chain<N>(ch, q, R, p, om, pj);
    double t[3];
    mv3(R, ch->p_tool, t);
    v[0] = p[0] + t[0]; v[1] = p[1] + t[1]; v[2] = p[2] + t[2];
    mv3(R, P.a_tool, &v[3]);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (ch->jtype[k] == 0) {
        const double d[3] = {v[0] - pj[k][0], v[1] - pj[k][1], v[2] - pj[k][2]};
        cross3(om[k], d, Jp[k]);
      } else {
        Jp[k][0] = om[k][0]; Jp[k][1] = om[k][1]; Jp[k][2] = om[k][2];
        om[k][0] = om[k][1] = om[k][2] = 0.0;
      }
    }
  }

  static OH_DEV void dual(const double (&y)[NH], const double (&v)[NH], const double rho, Dual& D) {
    cross3(&v[3], &y[3], D.c);
#pragma unroll
    for (int k = 0; k < 3; ++k) D.r[k] = rho * v[3 + k] + y[3 + k];
    D.k = rho * dot3(&v[3], &v[3]) + dot3(&y[3], &v[3]);
  }

  template <int N>
  static OH_DEV double jty(const int i, const double (&Jp)[N][3], const double (&om)[N][3], const double (&y)[NH], const Dual& D) {
    return dot3(Jp[i], y) + dot3(om[i], D.c);
  }

  template <int N>
  static OH_DEV double hess(const int a, const int c, const double (&Jp)[N][3], const double (&om)[N][3], const double (&v)[NH], const double (&y)[NH],
                            const double rho, const Dual& D) {
    double t[3];
    cross3(om[c], Jp[a], t);
    return rho * dot3(Jp[a], Jp[c]) - dot3(y, t) + D.k * dot3(om[a], om[c]) - dot3(om[c], &v[3]) * dot3(om[a], D.r);
  }
};

template <int N, int NH>
OH_DEV double ik_rows_merit(const IkParams& P, const double (&q)[N], const double (&qn)[N], const double (&v)[NH], const double (&g)[NH],
                            const double (&lam)[NH], double rho) {
  double c = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) c += (q[i] - qn[i]) * (q[i] - qn[i]);
  double m = P.w * c;
#pragma unroll
  for (int k = 0; k < NH; ++k) {
    const double h = g[k] - v[k];
    m += lam[k] * h + 0.5 * rho * h * h;
  }
  return m;
}

template <int N, class Rows>
OH_DEV void ik_rows_solve(const oh_chain* __restrict__ ch, const IkParams& P, const int b, const double* __restrict__ x0, const double* __restrict__ par,
                          double* __restrict__ x, double* __restrict__ f, double* __restrict__ kkt, int* __restrict__ iters, int* __restrict__ status,
                          double* __restrict__ mult) {
  constexpr int NH = Rows::NH, NP = N * (N + 1) / 2, NM = NH + 2 * N;
  double q[N], qn[N], g[NH], lam[NH];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    qn[i] = par[(size_t)b * (N + NH) + i];
    q[i] = fmin(fmax(x0[(size_t)b * N + i], P.lo[i]), P.up[i]);
  }
#pragma unroll
  for (int k = 0; k < NH; ++k) {
    g[k] = par[(size_t)b * (N + NH) + N + k];
    lam[k] = 0.0;
  }
  double v[NH], Jp[N][3], om[N][3];
  Rows::template eval<N>(ch, P, q, v, Jp, om);
  int it = 1, st = OH_STATUS_MAX_ITER;
  double rho = P.rho0, shift = 0.0, h_prev = 1e300;
  double grad[N];
  bool act[N];
  typename Rows::Dual D;
  {
    // non-finite seed / parameters: report, do not iterate (as in k_ik_solve)
    const double m_init = ik_rows_merit<N, NH>(P, q, qn, v, g, lam, rho);
    if (!(m_init == m_init) || !(fabs(m_init) < 1e300)) st = OH_STATUS_NUMERICAL;
  }
  while (it < P.max_iter && st != OH_STATUS_NUMERICAL) {
    const int it_pass = it;
    // ---- inner: projected Newton on the augmented Lagrangian ----
    while (it < P.max_iter) {
      double y[NH], hmax = 0.0, ysum = 0.0;
#pragma unroll
      for (int k = 0; k < NH; ++k) {
        const double h = g[k] - v[k];
        y[k] = lam[k] + rho * h;
        hmax = fmax(hmax, fabs(h));
        ysum += fabs(y[k]);
      }
      Rows::dual(y, v, rho, D);
      double pgn = 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        grad[i] = 2.0 * P.w * (q[i] - qn[i]) - Rows::template jty<N>(i, Jp, om, y, D);
        act[i] = (q[i] <= P.lo[i] && grad[i] > 0.0) || (q[i] >= P.up[i] && grad[i] < 0.0);
        if (!act[i]) pgn = fmax(pgn, fabs(grad[i]));
      }
      if (pgn <= fmax(0.5 * P.tol, fmin(1e-2, 0.1 * hmax))) break;
      // 2wI + rho J^T J - sum_k y_k d2 value_k  (h = goal - value: the curvature enters with the minus sign)
      double H[NP];
#pragma unroll
      for (int a = 0; a < N; ++a) {
#pragma unroll
        for (int c = 0; c <= a; ++c) {
          double e = Rows::template hess<N>(a, c, Jp, om, v, y, rho, D);
          if (a == c) e += 2.0 * P.w;
          H[tri(a, c)] = e;
        }
      }
      double L[NP];
      for (;;) {
#pragma unroll
        for (int a = 0; a < N; ++a) {
#pragma unroll
          for (int c = 0; c <= a; ++c) {
            double e = H[tri(a, c)];
            if (a == c) e += shift;
            if (act[a] || act[c]) e = (a == c) ? 1.0 : 0.0;
            L[tri(a, c)] = e;
          }
        }
        if (chol_packed<N>(L, 0.0)) break;
        shift = fmax(10.0 * shift, 1e-3 * rho);
        if (!(shift < 1e300)) break;
      }
      double d[N];
#pragma unroll
      for (int i = 0; i < N; ++i) d[i] = act[i] ? 0.0 : -grad[i];
      fsub<N>(L, d);
      bsub<N>(L, d);
      const double m0 = ik_rows_merit<N, NH>(P, q, qn, v, g, lam, rho);
      double alpha = 1.0;
      bool ok = false;
      double qt[N], vt[NH], Jt[N][3], ot[N][3];
      for (int ls = 0; ls < 30; ++ls) {
        double slope = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          qt[i] = fmin(fmax(q[i] + alpha * d[i], P.lo[i]), P.up[i]);
          slope += grad[i] * (qt[i] - q[i]);
        }
        Rows::template eval<N>(ch, P, qt, vt, Jt, ot);
        ++it;
        // (rounding slack as in k_ik_solve, |y| summed over all rows)
        if (ik_rows_merit<N, NH>(P, qt, qn, vt, g, lam, rho) <= m0 + 1e-4 * slope + 4e-16 * fmax(1.0, fabs(m0)) + 8e-16 * ysum) {
          ok = true;
          break;
        }
        alpha *= 0.5;
        if (it >= P.max_iter) break;
      }
      if (!ok) {
        shift = fmax(10.0 * shift, 1e-3 * rho);
        if (shift > 1e12 * rho) {
          st = OH_STATUS_NUMERICAL;
          break;
        }
        continue;
      }
      shift = shift > 1e-12 ? 0.1 * shift : 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        q[i] = qt[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          Jp[i][k] = Jt[i][k];
          om[i][k] = ot[i][k];
        }
      }
#pragma unroll
      for (int k = 0; k < NH; ++k) v[k] = vt[k];
    }
    if (st == OH_STATUS_NUMERICAL) break;
    // ---- outer: multiplier update ----
    double hn = 0.0;
#pragma unroll
    for (int k = 0; k < NH; ++k) {
      const double h = g[k] - v[k];
      lam[k] += rho * h;
      hn = fmax(hn, fabs(h));
    }
    Rows::dual(lam, v, 0.0, D);
    double stat = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double gi = 2.0 * P.w * (q[i] - qn[i]) - Rows::template jty<N>(i, Jp, om, lam, D);
      const bool a = (q[i] <= P.lo[i] && gi > 0.0) || (q[i] >= P.up[i] && gi < 0.0);
      if (!a) stat = fmax(stat, fabs(gi));
    }
    if (hn <= P.tol_feas && stat <= P.tol) {
      st = OH_STATUS_CONVERGED;
      break;
    }
    if (hn > 0.1 * h_prev) rho = fmin(rho * 10.0, 1e8);
    h_prev = hn;
    // a pass whose inner loop had nothing to do counts as one evaluation towards the cap: pinned at an infeasible stationary point with every free
    // joint's gradient below the inner tolerance (a goal out of reach, all joints on their bounds) such passes only grow lam, and would do so
    // without end (the two older kernels share the loop and not this line; there the case has not been seen)
    if (it == it_pass) ++it;
  }
  // ---- results in the reference's form: v = [q - lo; up - q; h; -h] >= 0 (optimization.py:47-51), h of NH rows ----
  double stat = 0.0, feas = 0.0, cost = 0.0;
  Rows::dual(lam, v, 0.0, D);
#pragma unroll
  for (int k = 0; k < NH; ++k) feas = fmax(feas, fabs(g[k] - v[k]));
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double gi = 2.0 * P.w * (q[i] - qn[i]) - Rows::template jty<N>(i, Jp, om, lam, D);
    const bool lo = q[i] <= P.lo[i] && gi > 0.0, up = q[i] >= P.up[i] && gi < 0.0;
    if (!(lo || up)) stat = fmax(stat, fabs(gi));
    cost += (q[i] - qn[i]) * (q[i] - qn[i]);
    if (x) x[(size_t)b * N + i] = q[i];
    if (mult) {
      mult[(size_t)b * NM + NH + i] = lo ? gi : 0.0;
      mult[(size_t)b * NM + NH + N + i] = up ? -gi : 0.0;
    }
  }
  if (mult) {
#pragma unroll
    for (int k = 0; k < NH; ++k) mult[(size_t)b * NM + k] = -lam[k];
  }
  if (f) f[b] = P.w * cost;
  if (kkt) {
    kkt[(size_t)b * 3 + 0] = stat;
    kkt[(size_t)b * 3 + 1] = feas;
    kkt[(size_t)b * 3 + 2] = 0.0;
  }
  if (iters) iters[b] = it;
  if (status) status[b] = st;
}

template <int N>
__global__ void __launch_bounds__(64) k_ik_axis_solve(const oh_chain* __restrict__ ch, IkParams P, int B, const double* __restrict__ x0,
                                                      const double* __restrict__ par, double* __restrict__ x, double* __restrict__ f,
                                                      double* __restrict__ kkt, int* __restrict__ iters, int* __restrict__ status,
                                                      double* __restrict__ mult) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  ik_rows_solve<N, IkAxisRows>(ch, P, b, x0, par, x, f, kkt, iters, status, mult);
}

template <typename K>
bool ik_kernel_info(K kernel, OhKernelInfo* out) {
  hipFuncAttributes a{};
  if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(kernel)) != hipSuccess) return false;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 64, 0) != hipSuccess) nb = 0;
  *out = OhKernelInfo{a.numRegs, (int)a.localSizeBytes, (int)a.sharedSizeBytes, 64, nb};
  return true;
}

}  // namespace

// "k_ik_solve" / "k_ik_pose_solve" / "k_ik_axis_solve": the 7-joint instantiations; with "_N" appended: N = 2 ... 8
bool oh_kernel_info_ik(const char* name, OhKernelInfo* out) {
  std::string n(name);
  int N = 7;
  if (n.size() > 2 && n[n.size() - 2] == '_' && n.back() >= '2' && n.back() <= '8') {
    N = n.back() - '0';
    n.resize(n.size() - 2);
  }
  const bool pose = n == "k_ik_pose_solve", axis = n == "k_ik_axis_solve";
  if (!pose && !axis && n != "k_ik_solve") return false;
  switch (N) {
#define C(NN) case NN: return axis ? ik_kernel_info(k_ik_axis_solve<NN>, out) : pose ? ik_kernel_info(k_ik_pose_solve<NN>, out) : ik_kernel_info(k_ik_solve<NN>, out)
    C(2); C(3); C(4); C(5); C(6); C(7); C(8);
#undef C
  }
  return false;
}

bool oh_launch_ik_pose_solve(hipStream_t stream, const oh_chain* d_chain, const IkParams& P, int B, const double* x0, const double* p, double* x,
                             double* f, double* kkt, int* iters, int* status, double* mult) {
  const dim3 block(64), grid((B + 63) / 64);
  switch (P.ndof) {
#define C(NN) case NN: hipLaunchKernelGGL(k_ik_pose_solve<NN>, grid, block, 0, stream, d_chain, P, B, x0, p, x, f, kkt, iters, status, mult); break
    C(2); C(3); C(4); C(5); C(6); C(7); C(8);
#undef C
    default: return false;
  }
  return true;
}

bool oh_launch_ik_axis_solve(hipStream_t stream, const oh_chain* d_chain, const IkParams& P, int B, const double* x0, const double* p, double* x,
                             double* f, double* kkt, int* iters, int* status, double* mult) {
  const dim3 block(64), grid((B + 63) / 64);
  switch (P.ndof) {
#define C(NN) case NN: hipLaunchKernelGGL(k_ik_axis_solve<NN>, grid, block, 0, stream, d_chain, P, B, x0, p, x, f, kkt, iters, status, mult); break
    C(2); C(3); C(4); C(5); C(6); C(7); C(8);
#undef C
    default: return false;
  }
  return true;
}

bool oh_launch_ik_solve(hipStream_t stream, const oh_chain* d_chain, const IkParams& P, int B, const double* x0, const double* p, double* x,
                        double* f, double* kkt, int* iters, int* status, double* mult) {
  const dim3 block(64), grid((B + 63) / 64);
  switch (P.ndof) {  // chain lengths 2 ... 8 (round 5: planar_3dof, the tester robots, 8-joint arms)
#define C(NN) case NN: hipLaunchKernelGGL(k_ik_solve<NN>, grid, block, 0, stream, d_chain, P, B, x0, p, x, f, kkt, iters, status, mult); break
    C(2); C(3); C(4); C(5); C(6); C(7); C(8);
#undef C
    default: return false;
  }
  return true;
}
