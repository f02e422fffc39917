// Truncated Newton-CG inner solver of the generic tape family (option tape_newton; k_tape_solve_newton of oh_tape.hip): the outer
// Powell-Hestenes-Rockafellar loop of oh_tape_solver.h -- multiplier update, penalty growth, omega schedule, statuses, tolerances -- around a line-search
// Newton-CG iteration (Nocedal & Wright, algorithm 7.1, preconditioned) whose every CG iteration is ONE exact product of the merit's generalised Hessian
// with a vector, E::hess_vec, computed on the device by forward-over-reverse on the registers and adjoints the last E::phi left behind.
//
// Included by oh_tape.hip alone, after oh_tape_solver.h, and NOT part of the text handed to hiprtc: oh_tape_solver.h is embedded in every generated
// program and keys the disk cache, so it is not touched, and what this solver shares with it -- TapeParams, TapeWork / TIDX, tape_al_ineq, tape_al_eq --
// it takes from there.  COPIED from tape_solve_instance, not shared, for that reason: the outer iteration, and the Armijo acceptance test with its rounding
// `slack` and its gradient-decides end game (tape_newton_armijo below).  A change to either there must be made here too; oracle/tape_ref.py:solve_tape_al and
// tests/tape_newton_ref.py:solve_tape_newton are the two numpy restatements.
//
// INVARIANT of E::hess_vec: it follows an E::phi at the same point with the same multipliers and penalty, with nothing that writes the evaluator's
// registers in between.  The state machine keeps it: the accepted trial becomes x (the last phi was the trial's), a failed line search re-evaluates at x,
// an outer update re-evaluates at x under the new multipliers and penalty.
//
// No n x n matrix and no (s, y) pairs: nine vectors of n, the multipliers and the rows.  max_iter caps phi evaluations PLUS products; iters reports their sum.
#ifndef OH_TAPE_NEWTON_H
#define OH_TAPE_NEWTON_H

struct TapeNewtonWork {
  TapeWork W;  // x, xt, g, gt, d, lam, mu, rowv as the evaluators know them (H, s, hy: null)
  double *r, *y, *p, *hp;  // CG: residual, preconditioned residual, search direction, H p
};

// rows of the solver's work set (the interpreter's four register columns -- val, adj, dval, dadj -- come on top: oh_tape_newton_work_rows)
__host__ __device__ inline size_t tape_newton_rows(const TapeParams& T) {
  return 9 * (size_t)T.nx + 2 * (size_t)(T.n_ineq > 0 ? T.n_ineq : 1) + 2 * (size_t)(T.n_eq > 0 ? T.n_eq : 1);
}

__device__ inline TapeNewtonWork tape_newton_carve(const TapeParams& T, double* w, const int Bp) {
  const size_t n = T.nx, ni = T.n_ineq > 0 ? T.n_ineq : 1, ne = T.n_eq > 0 ? T.n_eq : 1;
  TapeNewtonWork N{};
  auto take = [&](size_t rows) { double* o = w; w += rows * (size_t)Bp; return o; };
  N.W.x = take(n); N.W.xt = take(n); N.W.g = take(n); N.W.gt = take(n); N.W.d = take(n);
  N.r = take(n); N.y = take(n); N.p = take(n); N.hp = take(n);
  N.W.lam = take(ni); N.W.mu = take(ne); N.W.rowv = take(ni + ne);
  return N;
}

// The acceptance test of tape_solve_instance's line search (oh_tape_solver.h), copied: sufficient decrease where the merit resolves it, otherwise any
// resolved decrease, otherwise -- the merit within its rounding `slack` -- a strictly smaller gradient decides.  gt: the trial's gradient.
__device__ inline bool tape_newton_armijo(const int n, const int Bp, const int b, const double vt, const double val, const double alpha, const double slope,
                                          const double slack, const double gg, const double* __restrict__ gt) {
  const double need = -1e-4 * alpha * slope;
  if (need > slack) return (vt == vt) && vt <= val - need + slack;
  if ((vt == vt) && vt <= val - slack) return true;
  if ((vt == vt) && vt <= val + slack) {
    double ggt = 0.0;
    for (int k = 0; k < n; ++k) ggt += gt[TIDX(k)] * gt[TIDX(k)];
    return ggt <= (1.0 - 1e-4 * alpha) * gg && ggt < gg;
  }
  return false;
}

// y = M r: the handle's metric H0 (symmetric: row k read as column k, the same matrix for every lane -> scalar loads; the loop of the two-loop recursion),
// else the identity
__device__ inline void tape_newton_precond(const TapeParams& T, const int Bp, const int b, const double* __restrict__ r, double* __restrict__ y) {
  const int n = T.nx;
  if (T.h0 == nullptr) {
    for (int k = 0; k < n; ++k) y[TIDX(k)] = r[TIDX(k)];
    return;
  }
  for (int k = 0; k < n; ++k) {
    double acc = 0.0;
    for (int j = 0; j < n; ++j) acc += T.h0[(size_t)j * n + k] * r[TIDX(j)];
    y[TIDX(k)] = acc;
  }
}

// E::phi as in oh_tape_solver.h; E::hess_vec(v, rho, out): out = (generalised Hessian of the merit at the point of the last phi) v, all SoA.
// cg_cap: CG iterations per Newton step (option tape_newton_cg; the host resolves "by size" to min(nx, 50)).  stats: [B][2] (Newton steps, products).
template <class E>
__device__ inline void tape_newton_instance(const TapeParams& T, E& ev, const TapeNewtonWork& N, const int cg_cap, const int Bp, const int b, const int gb,
                                            const double* __restrict__ x0, double* __restrict__ xo, double* __restrict__ fo, double* __restrict__ kkt,
                                            int* __restrict__ iters, int* __restrict__ status, double* __restrict__ mult, int* __restrict__ stats) {
  const TapeWork& W = N.W;
  const int n = T.nx;
  for (int k = 0; k < n; ++k) W.x[TIDX(k)] = x0[(size_t)gb * n + k];
  for (int i = 0; i < T.n_ineq; ++i) W.lam[TIDX(i)] = 0.0;
  for (int i = 0; i < T.n_eq; ++i) W.mu[TIDX(i)] = 0.0;
  const bool metric = T.h0 != nullptr;
  double rho = T.rho0, omega = fmax(T.tol, 1e-2), meas_prev = 1e300;
  double msum = 0.0;
  double fval, cmax, meas;
  double val = ev.phi(W.x, W.g, rho, &fval, &cmax, &meas);
  int evals = 1, hvps = 0, steps = 0, st = OH_TAPE_ST_MAX_ITER;
  bool force_sd = false;  // the last search, from a Newton direction, failed: this step is steepest descent
  double stat = 0.0;
  for (;;) {
    stat = 0.0;
    for (int k = 0; k < n; ++k) stat = fmax(stat, fabs(W.g[TIDX(k)]));
    bool finite = (val == val) && (fabs(val) < 1e300);
    for (int k = 0; k < n; ++k) finite = finite && (W.g[TIDX(k)] == W.g[TIDX(k)]);
    if (!finite) { st = OH_TAPE_ST_NUMERICAL; break; }
    if (stat <= omega) {
      if (stat <= T.tol && meas <= T.tol_feas) { st = OH_TAPE_ST_CONVERGED; break; }
      if (evals + hvps >= T.max_iter) break;
      // outer iteration, as in tape_solve_instance: multiplier update at x with the current penalty (rowv holds the rows of the last evaluation, at x)
      msum = 0.0;
      for (int i = 0; i < T.n_eq; ++i) {
        const double v = W.mu[TIDX(i)] - rho * W.rowv[TIDX(T.n_ineq + i)];
        W.mu[TIDX(i)] = v;
        msum += fabs(v);
      }
      for (int i = 0; i < T.n_ineq; ++i) {
        const double v = fmax(0.0, W.lam[TIDX(i)] - rho * W.rowv[TIDX(i)]);
        W.lam[TIDX(i)] = v;
        msum += v;
      }
      if (meas > 0.25 * meas_prev) rho = fmin(rho * 10.0, 1e8);
      meas_prev = meas;
      omega = fmax(T.tol, fmin(omega, 0.1 * meas));
      val = ev.phi(W.x, W.g, rho, &fval, &cmax, &meas);  // (and the registers hess_vec reads are those of the new merit)
      ++evals;
      continue;
    }
    if (evals + hvps >= T.max_iter) break;
    bool newton = !force_sd;  // a failed search from this direction may retry with steepest descent
    bool unit = false;        // the direction carries no Newton scale: first trial within unit length
    if (newton) {
      // truncated CG on H d = -g: z (in W.d) = 0, r = g, y = M r, p = -y
      double ry = 0.0, gnorm2 = 0.0;
      tape_newton_precond(T, Bp, b, W.g, N.y);
      for (int k = 0; k < n; ++k) {
        const double gk = W.g[TIDX(k)], yk = N.y[TIDX(k)];
        W.d[TIDX(k)] = 0.0;
        N.r[TIDX(k)] = gk;
        N.p[TIDX(k)] = -yk;
        ry += gk * yk;
        gnorm2 += gk * gk;
      }
      const double gnorm = sqrt(gnorm2), eta = fmin(0.5, sqrt(gnorm));
      for (int j = 0; j < cg_cap; ++j) {
        ev.hess_vec(N.p, rho, N.hp);
        ++hvps;
        double kappa = 0.0, pp = 0.0;
        for (int k = 0; k < n; ++k) { const double pk = N.p[TIDX(k)]; kappa += pk * N.hp[TIDX(k)]; pp += pk * pk; }
        if (!(kappa > 1e-12 * pp)) {  // negative or vanishing curvature, or NaN
          if (j == 0) {
            for (int k = 0; k < n; ++k) W.d[TIDX(k)] = -N.y[TIDX(k)];
            unit = true;
            newton = metric;  // without a metric this IS steepest descent: a failed search from it ends the instance
          }
          break;
        }
        const double a = ry / kappa;
        double rr = 0.0;
        for (int k = 0; k < n; ++k) {
          W.d[TIDX(k)] += a * N.p[TIDX(k)];
          const double rk = N.r[TIDX(k)] + a * N.hp[TIDX(k)];
          N.r[TIDX(k)] = rk;
          rr += rk * rk;
        }
        if (sqrt(rr) <= eta * gnorm) break;
        if (j + 1 == cg_cap || evals + hvps + 1 >= T.max_iter) break;  // the cap; or what is left of the budget is the line search's first trial
        tape_newton_precond(T, Bp, b, N.r, N.y);
        double ryn = 0.0;
        for (int k = 0; k < n; ++k) ryn += N.r[TIDX(k)] * N.y[TIDX(k)];
        const double beta = ryn / ry;
        for (int k = 0; k < n; ++k) N.p[TIDX(k)] = -N.y[TIDX(k)] + beta * N.p[TIDX(k)];
        ry = ryn;
      }
    } else {
      for (int k = 0; k < n; ++k) W.d[TIDX(k)] = -W.g[TIDX(k)];
      unit = true;
    }
    double slope = 0.0;
    for (int k = 0; k < n; ++k) slope += W.g[TIDX(k)] * W.d[TIDX(k)];
    if (!(slope < 0.0)) {
      slope = 0.0;
      for (int k = 0; k < n; ++k) { W.d[TIDX(k)] = -W.g[TIDX(k)]; slope -= W.g[TIDX(k)] * W.g[TIDX(k)]; }
      unit = true;
      newton = false;
    }
    double alpha = 1.0, vt = 0.0, ft = 0.0, ct = 0.0, mt = 0.0;
    if (unit) {  // the cap tape_solve_instance applies to a fresh metric
      double dmax = 0.0;
      for (int k = 0; k < n; ++k) dmax = fmax(dmax, fabs(W.d[TIDX(k)]));
      alpha = fmin(1.0, 1.0 / dmax);
    }
    bool ok = false;
    const double slack = 4e-16 * (fmax(1.0, fabs(val)) + msum);
    double gg = 0.0;
    for (int k = 0; k < n; ++k) gg += W.g[TIDX(k)] * W.g[TIDX(k)];
    for (int ls = 0; ls < 40; ++ls) {
      for (int k = 0; k < n; ++k) W.xt[TIDX(k)] = W.x[TIDX(k)] + alpha * W.d[TIDX(k)];
      vt = ev.phi(W.xt, W.gt, rho, &ft, &ct, &mt);
      ++evals;
      if (tape_newton_armijo(n, Bp, b, vt, val, alpha, slope, slack, gg, W.gt)) { ok = true; break; }
      alpha *= 0.5;
      if (evals + hvps >= T.max_iter) break;
    }
    if (!ok) {
      // registers, adjoints and rowv belong to the rejected trial: re-evaluate at x before anything reads them again (the invariant of hess_vec)
      val = ev.phi(W.x, W.g, rho, &fval, &cmax, &meas);
      ++evals;
      if (!newton || evals + hvps >= T.max_iter) break;  // steepest descent cannot improve: rounding floor
      force_sd = true;
      continue;
    }
    force_sd = false;
    ++steps;
    for (int k = 0; k < n; ++k) { W.x[TIDX(k)] = W.xt[TIDX(k)]; W.g[TIDX(k)] = W.gt[TIDX(k)]; }
    val = vt; fval = ft; cmax = ct; meas = mt;
  }
  for (int k = 0; k < n; ++k)
    if (xo) xo[(size_t)gb * n + k] = W.x[TIDX(k)];
  if (fo) fo[gb] = fval;
  if (kkt) { kkt[3 * (size_t)gb] = stat; kkt[3 * (size_t)gb + 1] = cmax; kkt[3 * (size_t)gb + 2] = meas; }
  if (iters) iters[gb] = evals + hvps;
  if (status) status[gb] = st;
  if (stats) { stats[2 * (size_t)gb] = steps; stats[2 * (size_t)gb + 1] = hvps; }
  if (mult) {
    for (int i = 0; i < T.n_ineq; ++i) mult[(size_t)gb * (T.n_ineq + T.n_eq) + i] = W.lam[TIDX(i)];
    for (int i = 0; i < T.n_eq; ++i) mult[(size_t)gb * (T.n_ineq + T.n_eq) + T.n_ineq + i] = W.mu[TIDX(i)];
  }
}

#endif  // OH_TAPE_NEWTON_H
