// The inverse-kinematics iteration (oh_ik.hip), as the text of a function body: oh_ik.hip includes it where the iteration runs.  It reads the names
//     N, Rows                                  chain length and rows policy (template parameters of the including function)
//     ch, P, b                                 chain constants, IkParams, index of the instance
//     x0, par, x, f, kkt, iters, status, mult  inputs and outputs of oh_launch_ik
// and nothing else of its surroundings.  No include guard: it is a body, not a set of declarations.
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
    // non-finite seed / parameters: report, do not iterate (fmax-based norms would hide a NaN)
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
        grad[i] = Rows::template grad<N>(i, 2.0 * P.w * (q[i] - qn[i]), Jp, om, y, D);
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
        // (rounding slack: that of the merit itself plus what the rounding of the value, a few 1e-16 per row, is worth through the effective
        //  multiplier y = lam + rho h, |y| summed over all rows -- without the second part one instance in 65 536 of the config-1 batch, with
        //  |y| ~ 10 and a step that predicts a decrease of 1e-17, failed the test at every step length until the iteration cap; round 3)
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
      const double gi = Rows::template grad<N>(i, 2.0 * P.w * (q[i] - qn[i]), Jp, om, lam, D);
      const bool a = (q[i] <= P.lo[i] && gi > 0.0) || (q[i] >= P.up[i] && gi < 0.0);
      if (!a) stat = fmax(stat, fabs(gi));
    }
    if (hn <= P.tol_feas && stat <= P.tol) {
      st = OH_STATUS_CONVERGED;
      break;
    }
    if (hn > 0.1 * h_prev) rho = fmin(rho * 10.0, 1e8);
    h_prev = hn;
    if (Rows::idle_pass_counts && it == it_pass) ++it;
  }
  // ---- results in the reference's form: v = [q - lo; up - q; h; -h] >= 0 (optimization.py:47-51), h of NH rows ----
  double stat = 0.0, feas = 0.0, cost = 0.0;
  Rows::dual(lam, v, 0.0, D);
#pragma unroll
  for (int k = 0; k < NH; ++k) feas = fmax(feas, fabs(g[k] - v[k]));
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double gi = Rows::template grad<N>(i, 2.0 * P.w * (q[i] - qn[i]), Jp, om, lam, D);
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
    kkt[(size_t)b * 3 + 2] = 0.0;  // multipliers are non-zero only on rows that sit exactly on their bound
  }
  if (iters) iters[b] = it;
  if (status) status[b] = st;
