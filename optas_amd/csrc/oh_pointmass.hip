// OH_PROBLEM_POINT_MASS_MPC: example/point_mass_mpc.py Controller (:88-154), BASELINE config 3.
// The whole primal-dual interior-point loop runs inside one launch, Newton steps by a Riccati sweep over the T stages (state (y,v) in R^4, control
// a in R^2).  The rules of the iteration are stated in oh_pm_rules.h: rows and their Jacobian (pm_cons, pm_residuals), the seed (pm_seed,
// pm_first_rows), the stage terms of a knot (pm_stage_terms), the Riccati step of a stage with its free and pinned branch (pm_riccati_step), the Newton
// direction and the Euler step (pm_newton_step, pm_euler), the row step of a knot (pm_row_step), the verdict (pm_verdict) and the barrier update
// (pm_barrier).
//   k_pm_solve       one thread per plant, calls the rules; its own: work arrays in HBM scratch laid out [row][b] (instance index fastest -> coalesced;
//                    ~6 KB per instance, so a 4096-batch stays resident in L2 / Infinity Cache), each sweep prefetching the next knot's rows
//                    (load_stage, load_gain, load_delta).
//   k_pm_solve_wave  one wavefront per plant, one lane per knot (T <= 64), everything in registers, calls the rules; its own: the lane == t
//                    ownership, the broadcasts from the knot's lane and the three reductions.
// Three pieces stay written out in one kernel each, because through the shared function that kernel left the bits or the device time of the texts
// these rules replaced (profiles/pm_one_text_pieces.json has the arrays and the points):
//   the row step of forward pass 2 in k_pm_solve   through pm_row_step x, f, kkt and the rollout states move in the last bit
//   the seed roll-out in k_pm_solve_wave           through pm_seed f moves in the last bit on some instances
//   the Riccati step in k_pm_solve_wave            through pm_riccati_step every wave point misses the timing criterion
#include <cstdlib>

#include "oh_device.h"
#include "oh_kernels.h"
#include "oh_pm_rules.h"

#define PIDX(row) ((size_t)(row) * Bp + b)

__global__ __launch_bounds__(64) void k_pm_solve(PmParams P, PmBuffers D, const double* __restrict__ x0, const double* __restrict__ pin,
                                                 double* __restrict__ xo, double* __restrict__ fo, double* __restrict__ kkt,
                                                 int* __restrict__ iters_o, int* __restrict__ status_o) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int Bp = D.Bp;
  if (b >= D.B) return;
  const int T = P.T;
  const double dt = P.dt, w = P.w_acc;
  const size_t np_ = 4 + 4 * (size_t)T, nx = 4 * (size_t)T;
  const double* pb = pin + (size_t)b * np_;
  const double* goal = pb + 4;           // [t][2]
  const double* obs = pb + 4 + 2 * T;    // [t][2]
  // work arrays (rows): a[2(T-1)], X[4T], s[9T], lam[9T], K[8(T-1)], kk[2(T-1)], dX[4T], da[2(T-1)]
  double* A_ = D.a; double* X_ = D.X; double* S_ = D.s; double* L_ = D.lam;
  double* K_ = D.K; double* k_ = D.kk; double* dX_ = D.dX; double* dA_ = D.da;

  pm_seed(P, pb, x0 + (size_t)b * nx + 2 * T,
          [&](const int t, const double (&x)[4]) { for (int j = 0; j < 4; ++j) X_[PIDX(4 * t + j)] = x[j]; },
          [&](const int t, const double a0, const double a1) { A_[PIDX(2 * t)] = a0; A_[PIDX(2 * t + 1)] = a1; });
  double mu = 0.1;
  for (int t = 0; t < T; ++t) {
    double x[4], c[9], jx, jy, s[9], lam[9];
    for (int j = 0; j < 4; ++j) x[j] = X_[PIDX(4 * t + j)];
    pm_cons(P, x, obs[2 * t], obs[2 * t + 1], c, jx, jy);
    pm_first_rows(c, mu, s, lam);
    for (int i = 0; i < 9; ++i) { S_[PIDX(9 * t + i)] = s[i]; L_[PIDX(9 * t + i)] = lam[i]; }
  }

  struct Stage {
    double x[4], s[9], l[9], a[2], g[2], o[2];
  };
  auto load_stage = [&](const int t, const bool with_goal) {
    Stage r;
    for (int j = 0; j < 4; ++j) r.x[j] = X_[PIDX(4 * t + j)];
    for (int i = 0; i < 9; ++i) { r.s[i] = S_[PIDX(9 * t + i)]; r.l[i] = L_[PIDX(9 * t + i)]; }
    r.a[0] = r.a[1] = 0.0;
    if (t < T - 1) { r.a[0] = A_[PIDX(2 * t)]; r.a[1] = A_[PIDX(2 * t + 1)]; }
    r.g[0] = r.g[1] = 0.0;
    if (with_goal) { r.g[0] = goal[2 * t]; r.g[1] = goal[2 * t + 1]; }
    r.o[0] = obs[2 * t]; r.o[1] = obs[2 * t + 1];
    return r;
  };
  int status = OH_STATUS_MAX_ITER, it = 0;
  double stat = 0.0, feas = 0.0, compl_ = 0.0, fval = 0.0;
  for (it = 0; it <= P.max_iter; ++it) {
    // ---- backward pass: residuals (adjoint) and Riccati recursion -----------------------------------------------
    PmCostToGo V;
    stat = 0.0; feas = 0.0; compl_ = 0.0; fval = 0.0;
    bool bad = false;
    // every sweep below walks the knots in a dependent chain while what it reads depends on the knot alone: the next knot's values are
    // requested before this one's arithmetic (otherwise each of the 3 x T knot steps of an iteration is a memory round trip: the whole
    // solve was 7.2 ms for any batch up to ~16 k instances)
    Stage nx_ = load_stage(T - 1, true);
    for (int t = T - 1; t >= 0; --t) {
      const Stage st = nx_;
      if (t > 0) nx_ = load_stage(t - 1, true);
      PmKnot kn;
      double Q[16];
      fval += pm_stage_terms(P, t, t >= 1, st.x, st.s, st.l, st.g[0], st.g[1], st.o[0], st.o[1], mu, kn, feas, compl_, bad);
      pm_Q16(kn.Q0, kn.Q1, kn.Q5, kn.Q10, kn.Q15, Q);
      if (t < T - 1) fval += w * (st.a[0] * st.a[0] + st.a[1] * st.a[1]);
      pm_riccati_step(P, t, Q, kn.q, kn.lx, st.a[0], st.a[1], V, stat, [&](const double (&Kt)[8], const double (&kt)[2]) {
        for (int j = 0; j < 8; ++j) K_[PIDX(8 * t + j)] = Kt[j];
        k_[PIDX(2 * t)] = kt[0]; k_[PIDX(2 * t + 1)] = kt[1];
      });
    }
    if (bad) feas = __builtin_nan("");
    const int verdict = pm_verdict(P, it, stat, fval, feas, compl_);
    if (verdict != PM_GO_ON) { status = verdict; break; }

    // ---- forward pass 1: Newton direction, fraction-to-the-boundary step lengths -------------------------------------------------
    double ap = 1.0, ad = 1.0;
    {
      double dx[4] = {0, 0, 0, 0};
      for (int j = 0; j < 4; ++j) dX_[PIDX(j)] = 0.0;
      struct Gain {
        double K[8], k[2];
      };
      auto load_gain = [&](const int t) {
        Gain r;
        for (int j = 0; j < 8; ++j) r.K[j] = t < T - 1 ? K_[PIDX(8 * t + j)] : 0.0;
        r.k[0] = t < T - 1 ? k_[PIDX(2 * t)] : 0.0;
        r.k[1] = t < T - 1 ? k_[PIDX(2 * t + 1)] : 0.0;
        return r;
      };
      Stage nx1 = load_stage(0, false);
      Gain ng1 = load_gain(0);
      for (int t = 0; t < T; ++t) {
        const Stage st = nx1;
        const Gain gn = ng1;
        if (t + 1 < T) { nx1 = load_stage(t + 1, false); ng1 = load_gain(t + 1); }
        if (t >= 1) {
          double rc[9], jx, jy, ds[9], dl[9];
          pm_residuals(P, st.x, st.o[0], st.o[1], st.s, rc, jx, jy);
          pm_row_step(dx, jx, jy, rc, st.s, st.l, mu, true, ds, dl, ap, ad);
        }
        if (t < T - 1) {
          double da0, da1;
          pm_newton_step(dt, gn.K, gn.k, dx, da0, da1);
          dA_[PIDX(2 * t)] = da0; dA_[PIDX(2 * t + 1)] = da1;
          for (int j = 0; j < 4; ++j) dX_[PIDX(4 * (t + 1) + j)] = dx[j];
        }
      }
    }
    // ---- forward pass 2: take the step (slacks / multipliers with the old Jacobians, states by exact roll-out) ------------------------
    double gap = 0.0;
    {
      double xn[4] = {pb[0], pb[1], pb[2], pb[3]};
      struct Delta {
        double dx[4], da[2];
      };
      auto load_delta = [&](const int t) {
        Delta r;
        for (int j = 0; j < 4; ++j) r.dx[j] = dX_[PIDX(4 * t + j)];
        r.da[0] = t < T - 1 ? dA_[PIDX(2 * t)] : 0.0;
        r.da[1] = t < T - 1 ? dA_[PIDX(2 * t + 1)] : 0.0;
        return r;
      };
      Stage nx2 = load_stage(0, false);
      Delta nd2 = load_delta(0);
      for (int t = 0; t < T; ++t) {
        const Stage st = nx2;
        const Delta dl_ = nd2;
        if (t + 1 < T) { nx2 = load_stage(t + 1, false); nd2 = load_delta(t + 1); }
        if (t >= 1) {
          // pm_row_step's ds and dl once more, written out (see the head of the file)
          double x[4], dx[4], c[9], jx, jy, d[9];
          for (int j = 0; j < 4; ++j) { x[j] = st.x[j]; dx[j] = dl_.dx[j]; }
          pm_cons(P, x, st.o[0], st.o[1], c, jx, jy);
          pm_Jv(dx, jx, jy, d);
          for (int i = 0; i < 9; ++i) {
            double s = st.s[i], lam = st.l[i];
            const double ds = d[i] + (c[i] - s);
            const double dl = (mu / s - lam) - (lam / s) * ds;
            s += ap * ds; lam += ad * dl;
            S_[PIDX(9 * t + i)] = s; L_[PIDX(9 * t + i)] = lam;
            gap += s * lam;
          }
        }
        for (int j = 0; j < 4; ++j) X_[PIDX(4 * t + j)] = xn[j];
        if (t < T - 1) {
          const double a0 = st.a[0] + ap * dl_.da[0], a1 = st.a[1] + ap * dl_.da[1];
          A_[PIDX(2 * t)] = a0; A_[PIDX(2 * t + 1)] = a1;
          pm_euler(dt, xn, a0, a1);
        }
      }
    }
    mu = pm_barrier(P, gap, ap, ad);
  }
  // ---- results in the reference layout x = [vec(Y 2xT); vec(dY 2xT)] --------------------------------------------------------------------
  if (xo) {
    double* xb = xo + (size_t)b * nx;
    for (int t = 0; t < T; ++t) {
      xb[2 * t] = X_[PIDX(4 * t)]; xb[2 * t + 1] = X_[PIDX(4 * t + 1)];
      xb[2 * T + 2 * t] = X_[PIDX(4 * t + 2)]; xb[2 * T + 2 * t + 1] = X_[PIDX(4 * t + 3)];
    }
  }
  if (fo) fo[b] = fval;
  if (kkt) { kkt[3 * (size_t)b] = stat; kkt[3 * (size_t)b + 1] = feas; kkt[3 * (size_t)b + 2] = compl_; }
  if (iters_o) iters_o[b] = it > P.max_iter ? P.max_iter : it;
  if (status_o) status_o[b] = status;
}

// ---- the same solve, ONE WAVEFRONT PER INSTANCE, one lane per knot (T <= 64) ---------------------------------------------------------------
// One lane per instance walks 3 x T knots per iteration with ~1000 dependent instructions each: 134 us per iteration whatever the batch, and
// BASELINE's 4096 plants are 64 wavefronts on 1024 SIMDs.  Here everything that belongs to a knot (constraint values, slacks, multipliers,
// the stage's Q, q and Lagrangian gradient, step lengths, the slack / multiplier update) is computed by the knot's lane from registers -- no
// work arrays at all -- and only the three recursions stay serial: the Riccati sweep, the Newton direction and the roll-out, executed by all
// lanes alike on values broadcast from the knot's lane (v_readlane), each lane keeping what belongs to its knot (gains, dx, da, x).  The
// recursions perform the thread kernel's operations in the thread kernel's order, and so does the sum behind the barrier parameter; only the
// reported objective is summed across lanes.  One iteration: ~20 us.
__global__ __launch_bounds__(64) void k_pm_solve_wave(PmParams P, int B, const double* __restrict__ x0, const double* __restrict__ pin, double* __restrict__ xo,
                                                      double* __restrict__ fo, double* __restrict__ kkt, int* __restrict__ iters_o, int* __restrict__ status_o) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int T = P.T;
  const bool on = lane < T;
  const double dt = P.dt, w = P.w_acc;
  const size_t np_ = 4 + 4 * (size_t)T, nx = 4 * (size_t)T;
  const double* pb = pin + (size_t)b * np_;
  const int tk = on ? lane : T - 1;
  const double g0 = pb[4 + 2 * tk], g1 = pb[4 + 2 * tk + 1];                  // goal of this knot
  const double o0 = pb[4 + 2 * T + 2 * tk], o1 = pb[4 + 2 * T + 2 * tk + 1];  // obstacle centre at this knot
  double X[4] = {0, 0, 0, 0}, a[2] = {0, 0};
  // ---- seed: pm_seed written out with the lane == t ownership (see the head of the file)
  {
    double vprev[2] = {pb[2], pb[3]};
    double x[4] = {pb[0], pb[1], pb[2], pb[3]};
    if (lane == 0)
      for (int j = 0; j < 4; ++j) X[j] = x[j];
    for (int t = 0; t < T - 1; ++t) {
      double v1[2] = {x0[(size_t)b * nx + 2 * T + 2 * (t + 1)], x0[(size_t)b * nx + 2 * T + 2 * (t + 1) + 1]};
      if (P.fix_vf && t == T - 2) v1[0] = v1[1] = 0.0;
      const double a0 = (v1[0] - vprev[0]) / dt, a1 = (v1[1] - vprev[1]) / dt;
      if (lane == t) { a[0] = a0; a[1] = a1; }
      pm_euler(dt, x, a0, a1);
      if (lane == t + 1)
        for (int j = 0; j < 4; ++j) X[j] = x[j];
      vprev[0] = v1[0]; vprev[1] = v1[1];
    }
  }
  double mu = 0.1;
  double s[9], lam[9];
  {
    double c[9], jx, jy;
    pm_cons(P, X, o0, o1, c, jx, jy);
    pm_first_rows(c, mu, s, lam);
  }
  int status = OH_STATUS_MAX_ITER, it = 0;
  double stat = 0.0, feas = 0.0, compl_ = 0.0, fval = 0.0;
  for (it = 0; it <= P.max_iter; ++it) {
    // ---- per knot: constraints, residuals, the stage's Q, q and Lagrangian gradient --------------------------------------------------
    PmKnot kn;
    double fe = 0.0, co = 0.0;
    bool bad = false;
    double fl = pm_stage_terms(P, lane, on && lane >= 1, X, s, lam, g0, g1, o0, o1, mu, kn, fe, co, bad);
    if (lane < T - 1) fl += w * (a[0] * a[0] + a[1] * a[1]);
    fval = wave64_sum(on ? fl : 0.0);
    feas = wave64_max(fe);
    compl_ = wave64_max(co);
    if (__any(on && bad)) feas = __builtin_nan("");
    // ---- backward: Riccati recursion, all lanes alike; lane t keeps K_t, k_t (pm_riccati_step written out: see the head of the file) ---------
    double Pm[16], pv[4], padj[4];
    double Kmine[8] = {0, 0, 0, 0, 0, 0, 0, 0}, kmine[2] = {0, 0};
    stat = 0.0;
    for (int t = T - 1; t >= 0; --t) {
      double Q[16];
      for (int j = 0; j < 16; ++j) Q[j] = 0.0;
      Q[0] = readlane_f64(kn.Q0, t); Q[5] = readlane_f64(kn.Q5, t); Q[1] = Q[4] = readlane_f64(kn.Q1, t); Q[10] = readlane_f64(kn.Q10, t); Q[15] = readlane_f64(kn.Q15, t);
      double qs[4], lxs[4];
      for (int j = 0; j < 4; ++j) { qs[j] = readlane_f64(kn.q[j], t); lxs[j] = readlane_f64(kn.lx[j], t); }
      if (t == T - 1) {
        for (int j = 0; j < 16; ++j) Pm[j] = Q[j];
        for (int j = 0; j < 4; ++j) { pv[j] = qs[j]; padj[j] = lxs[j]; }
        continue;
      }
      const double a0 = readlane_f64(a[0], t), a1 = readlane_f64(a[1], t);
      const bool pinned = P.fix_vf && t == T - 2;
      const double gu0 = 2.0 * w * a0 + dt * padj[2], gu1 = 2.0 * w * a1 + dt * padj[3];
      if (!pinned) stat = fmax(stat, fmax(fabs(gu0), fabs(gu1)));
      double PA[16];
      for (int r = 0; r < 4; ++r) {
        PA[4 * r + 0] = Pm[4 * r + 0]; PA[4 * r + 1] = Pm[4 * r + 1];
        PA[4 * r + 2] = Pm[4 * r + 2] + dt * Pm[4 * r + 0];
        PA[4 * r + 3] = Pm[4 * r + 3] + dt * Pm[4 * r + 1];
      }
      const double q00 = 2.0 * w + dt * dt * Pm[10], q01 = dt * dt * Pm[11], q11 = 2.0 * w + dt * dt * Pm[15];
      double Qux[8];
      for (int j = 0; j < 4; ++j) { Qux[j] = dt * PA[8 + j]; Qux[4 + j] = dt * PA[12 + j]; }
      const double qu0 = 2.0 * w * a0 + dt * pv[2], qu1 = 2.0 * w * a1 + dt * pv[3];
      // (reciprocal square roots and products: the 21 divisions of the textbook substitution were half the instructions of a knot step)
      const double i00 = rsqrt(q00), l10 = q01 * i00, i11 = rsqrt(q11 - l10 * l10);
      double Kt[8], kt[2];
      double Pn[16], pn[4], pa[4];
      if (pinned) {
        for (int j = 0; j < 8; ++j) Kt[j] = 0.0;
        Kt[2] = Kt[4 + 3] = -1.0 / dt;
        kt[0] = kt[1] = 0.0;
        const double kf = -1.0 / dt;
        for (int r = 0; r < 4; ++r)
          for (int cc = 0; cc < 4; ++cc) {
            double v = PA[4 * r + cc];
            if (r >= 2) v += dt * PA[4 * (r - 2) + cc];
            v += Qux[r] * Kt[cc] + Qux[4 + r] * Kt[4 + cc];
            v += Kt[r] * Qux[cc] + Kt[4 + r] * Qux[4 + cc];
            Pn[4 * r + cc] = Q[4 * r + cc] + v;
          }
        Pn[10] += kf * kf * q00; Pn[11] += kf * kf * q01; Pn[14] += kf * kf * q01; Pn[15] += kf * kf * q11;
        for (int r = 0; r < 4; ++r) {
          double v = pv[r], va = padj[r];
          if (r >= 2) { v += dt * pv[r - 2]; va += dt * padj[r - 2]; }
          pn[r] = qs[r] + v;
          pa[r] = lxs[r] + va;
        }
        pn[2] += kf * qu0; pn[3] += kf * qu1;
        pa[2] += kf * gu0; pa[3] += kf * gu1;
      } else {
        for (int j = 0; j < 4; ++j) {
          const double y0 = Qux[j] * i00, y1 = (Qux[4 + j] - l10 * y0) * i11;
          const double z1 = y1 * i11, z0 = (y0 - l10 * z1) * i00;
          Kt[j] = -z0; Kt[4 + j] = -z1;
        }
        const double y0 = qu0 * i00, y1 = (qu1 - l10 * y0) * i11;
        const double z1 = y1 * i11, z0 = (y0 - l10 * z1) * i00;
        kt[0] = -z0; kt[1] = -z1;
        for (int r = 0; r < 4; ++r)
          for (int cc = 0; cc < 4; ++cc) {
            double v = PA[4 * r + cc];
            if (r >= 2) v += dt * PA[4 * (r - 2) + cc];
            v += Qux[r] * Kt[cc] + Qux[4 + r] * Kt[4 + cc];
            Pn[4 * r + cc] = Q[4 * r + cc] + v;
          }
        for (int r = 0; r < 4; ++r) {
          double v = pv[r], va = padj[r];
          if (r >= 2) { v += dt * pv[r - 2]; va += dt * padj[r - 2]; }
          pn[r] = qs[r] + v + Qux[r] * kt[0] + Qux[4 + r] * kt[1];
          pa[r] = lxs[r] + va;
        }
      }
      if (lane == t) {
        for (int j = 0; j < 8; ++j) Kmine[j] = Kt[j];
        kmine[0] = kt[0]; kmine[1] = kt[1];
      }
      for (int r = 0; r < 4; ++r)
        for (int cc = 0; cc < 4; ++cc) Pm[4 * r + cc] = 0.5 * (Pn[4 * r + cc] + Pn[4 * cc + r]);
      for (int j = 0; j < 4; ++j) { pv[j] = pn[j]; padj[j] = pa[j]; }
    }
    const int verdict = pm_verdict(P, it, stat, fval, feas, compl_);
    if (verdict != PM_GO_ON) { status = verdict; break; }

    // ---- forward 1: Newton direction (serial), then the step lengths per knot ---------------------------------------------------------
    double dxm[4] = {0, 0, 0, 0}, dam[2] = {0, 0};
    {
      double dx[4] = {0, 0, 0, 0};
      for (int t = 0; t < T - 1; ++t) {
        double K[8], k[2], da0, da1;
        k[0] = readlane_f64(kmine[0], t); k[1] = readlane_f64(kmine[1], t);
        for (int j = 0; j < 8; ++j) K[j] = readlane_f64(Kmine[j], t);
        pm_newton_step(dt, K, k, dx, da0, da1);
        if (lane == t) { dam[0] = da0; dam[1] = da1; }
        if (lane == t + 1)
          for (int j = 0; j < 4; ++j) dxm[j] = dx[j];
      }
    }
    double ds[9], dl[9];
    double ap = 1.0, ad = 1.0;
    pm_row_step(dxm, kn.jx, kn.jy, kn.rc, s, lam, mu, on && lane >= 1, ds, dl, ap, ad);
    ap = wave64_min(ap);
    ad = wave64_min(ad);
    // ---- forward 2: take the step; the barrier parameter from the products summed in the thread kernel's order -----------------------
    double prod[9];
    for (int i = 0; i < 9; ++i) {
      if (on && lane >= 1) {
        s[i] += ap * ds[i];
        lam[i] += ad * dl[i];
      }
      prod[i] = s[i] * lam[i];
    }
    double gap = 0.0;
    for (int t = 1; t < T; ++t)
      for (int i = 0; i < 9; ++i) gap += readlane_f64(prod[i], t);
    if (lane < T - 1) { a[0] += ap * dam[0]; a[1] += ap * dam[1]; }
    {
      double xn[4] = {pb[0], pb[1], pb[2], pb[3]};
      for (int t = 0; t < T; ++t) {
        if (lane == t)
          for (int j = 0; j < 4; ++j) X[j] = xn[j];
        if (t < T - 1) pm_euler(dt, xn, readlane_f64(a[0], t), readlane_f64(a[1], t));
      }
    }
    mu = pm_barrier(P, gap, ap, ad);
  }
  if (xo && on) {
    double* xb = xo + (size_t)b * nx;
    xb[2 * lane] = X[0]; xb[2 * lane + 1] = X[1];
    xb[2 * T + 2 * lane] = X[2]; xb[2 * T + 2 * lane + 1] = X[3];
  }
  if (lane == 0) {
    if (fo) fo[b] = fval;
    if (kkt) { kkt[3 * (size_t)b] = stat; kkt[3 * (size_t)b + 1] = feas; kkt[3 * (size_t)b + 2] = compl_; }
    if (iters_o) iters_o[b] = it > P.max_iter ? P.max_iter : it;
    if (status_o) status_o[b] = status;
  }
}

// ---- closed-loop receding horizon kept on the device (example/point_mass_mpc.py main loop, :293-306 + Controller.next_state :156-161) ----
// parameters of one tick from the current plant state: p = [curr; dcurr; goal; obs], goal[:, i] = curr + ramp * i,
// obs[:, i] = obstacle centre at time index tick * advance + i of the table
__global__ __launch_bounds__(64) void k_pm_tick_params(int B, int T, int tick, int advance, double ramp, const double* __restrict__ state,
                                                       const double* __restrict__ obs_table, double* __restrict__ p) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double* pb = p + (size_t)b * (4 + 4 * (size_t)T);
  const double c0 = state[4 * (size_t)b], c1 = state[4 * (size_t)b + 1];
  pb[0] = c0; pb[1] = c1; pb[2] = state[4 * (size_t)b + 2]; pb[3] = state[4 * (size_t)b + 3];
  for (int i = 0; i < T; ++i) {
    pb[4 + 2 * i] = c0 + ramp * i;
    pb[4 + 2 * i + 1] = c1 + ramp * i;
    pb[4 + 2 * T + 2 * i] = obs_table[2 * ((size_t)tick * advance + i)];
    pb[4 + 2 * T + 2 * i + 1] = obs_table[2 * ((size_t)tick * advance + i) + 1];
  }
}
// the plant follows the plan for `advance` knots (the reference evaluates its linear interpolant at advance * dt, i.e. at a knot)
__global__ __launch_bounds__(64) void k_pm_advance(int B, int T, int advance, const double* __restrict__ x, double* __restrict__ state_next) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* xb = x + (size_t)b * 4 * T;
  state_next[4 * (size_t)b] = xb[2 * advance];
  state_next[4 * (size_t)b + 1] = xb[2 * advance + 1];
  state_next[4 * (size_t)b + 2] = xb[2 * T + 2 * advance];
  state_next[4 * (size_t)b + 3] = xb[2 * T + 2 * advance + 1];
}
void oh_launch_pm_tick_params(hipStream_t s, int B, int T, int tick, int advance, double ramp, const double* state, const double* obs_table, double* p) {
  hipLaunchKernelGGL(k_pm_tick_params, dim3((B + 63) / 64), dim3(64), 0, s, B, T, tick, advance, ramp, state, obs_table, p);
}
void oh_launch_pm_advance(hipStream_t s, int B, int T, int advance, const double* x, double* state_next) {
  hipLaunchKernelGGL(k_pm_advance, dim3((B + 63) / 64), dim3(64), 0, s, B, T, advance, x, state_next);
}

// The plant's state (y_0, dy_0) = (curr, dcurr) is pinned by equality rows, so the box rows and the obstacle row of knot 0 are constants of an instance
// (the reference writes them for every knot, point_mass_mpc.py:96-123).  A start outside the box or inside the obstacle has no feasible plan: IPOPT reports an
// infeasible problem (did_solve() False, solver.py:407-412) -- here OH_STATUS_INFEASIBLE, kkt[1] = the violation (round 5; SURVEY C3 rejects such starts).
__global__ __launch_bounds__(64) void k_pm_infeasible(PmParams P, int B, const double* __restrict__ pin, double* __restrict__ kkt, int* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* pb = pin + (size_t)b * (4 + 4 * (size_t)P.T);
  double c[9], jx, jy;
  pm_cons(P, pb, pb[4 + 2 * P.T], pb[4 + 2 * P.T + 1], c, jx, jy);
  double worst = 0.0;
  for (int i = 0; i < 9; ++i) worst = fmin(worst, c[i]);
  if (worst < -P.tol) {
    if (status) status[b] = OH_STATUS_INFEASIBLE;
    if (kkt) kkt[3 * (size_t)b + 1] = fmax(kkt[3 * (size_t)b + 1], -worst);
  }
}

void oh_launch_pm_solve(hipStream_t s, const PmParams& P, const PmBuffers& D, const double* x0, const double* p, double* x, double* f, double* kkt,
                        int* iters, int* status, const int wave_max) {
  // a wavefront per instance while that leaves the chip room (the thread kernel issues ~8x fewer instructions per instance, but needs ~10^5
  // instances to fill the SIMDs: 1024 plants take 3.5 ms with it and 0.7 ms here); wave_max: option "pm_wave_max", default 20480
  // (16 384 plants 6.8 / 5.8 ms thread / wave kernel, 32 768 9.8 / 11.3 ms: figures of a batch sweep whose tool and output are no longer in the tree;
  // profiles/pm_one_text_ab.json has both kernels at 4096 plants)
  if (P.T <= 64 && D.B <= wave_max) hipLaunchKernelGGL(k_pm_solve_wave, dim3(D.B), dim3(64), 0, s, P, D.B, x0, p, x, f, kkt, iters, status);
  else hipLaunchKernelGGL(k_pm_solve, dim3((D.B + 63) / 64), dim3(64), 0, s, P, D, x0, p, x, f, kkt, iters, status);
  if (status || kkt) hipLaunchKernelGGL(k_pm_infeasible, dim3((D.B + 63) / 64), dim3(64), 0, s, P, D.B, p, kkt, status);
}
