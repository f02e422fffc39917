// OH_PROBLEM_TORQUE_MPC -- BASELINE configs[4] / SURVEY 8(a) H5, App. B.5: joint-space torque MPC with the inverse dynamics
// RobotModel.rnea (optas/models.py:1731-1884) as equality rows,
//     x = [vec(Q); vec(dQ); vec(ddQ); vec(TAU)]  (robot time_derivs [0,1,2] + TaskModel "tau", derivs_align; builder.py:90-99)
//     a = [qc - q_0; dqc - dq_0; Euler rows of integrate_model_states(.., 1, dt) and (.., 2, dt)]      (builder.py:419-469,525-539)
//     h = TAU - rnea(Q, dQ, ddQ)                                                                        (builder.py:354)
//     k = [TAU - lo; up - TAU]                                enforce_model_limits("tau")               (builder.py:471-509)
//     f = w_path sum ||p_link(q_t) - goal_t||^2 + w_vel sum ||dQ||^2 + w_tau sum ||TAU||^2.
// Lowering: the linear rows and h are eliminated exactly (TAU_t = rnea(q_t, dq_t, ddq_t); q, dq rolled out from u_t = ddq_t with
// x_{t+1} = A x_t + B u_t, A = [[I, dt I], [0, I]], B = [0; dt I]).  The inequality rows enter through a primal-dual interior point (round 4; the
// reference's own algorithm class, solver.py:355-398 -> IPOPT): log barrier with multipliers of their own, relaxed below delta = theta mu_b, barrier
// parameter lowered by the monotone rule of Waechter & Biegler (2006) without re-evaluation; steps are Levenberg-Marquardt / Newton steps from a Riccati
// sweep over the stages z_t = (q_t, dq_t | u_t), scaled by the fraction-to-the-boundary rule on the linearised rows.  Near the solution the stage blocks
// hold the exact Hessian of the Lagrangian (k_tq_curv).  numpy restatement of this state machine: oracle/torque_ipm.py:solve_torque_ipm; the
// augmented-Lagrangian machine of rounds 1-3 survives as oracle/torque.py:solve_torque_lm, the independent second solver of the same problem.
//
// Kernels:
//   k_tq_eval3  one lane per (instance, knot, joint), 9 units x 7 joints per wavefront: the reference's Newton-Euler recursion on dual numbers seeded
//               with q_j, dq_j, ddq_j (the derivative is the derivative of the literal recursion by construction), the chain walk for p_link, then
//               the lanes of a unit exchange their columns through LDS and write the stage block H_t (packed lower 21 x 21), the gradients of cost
//               and barrier, and d tau / d z.
//   k_tq_curv   same mapping: second derivatives of the inverse dynamics and of the link position, added to H_t for instances in the Newton phase.
//   k_tq_step   one wavefront per instance, lane 8 r + c = entry (r, c) of every N x N block: ratio test, costate recursion for the stationarity measure,
//               barrier update, Riccati sweep by Gauss-Jordan steps across the lanes (no LDS, no barrier), fraction to the boundary, rollout of the trial.
//               Its scalar state machine is oh_tq_machine.h.
// Records (TqKnot, TqStage, TqLam), the table of the per-instance scalars and TqInst: oh_kernels.h.
#include "oh_kernels.h"
#include "oh_rnea.h"
#include "oh_tq_machine.h"

namespace {
using namespace oh_dyn;

// One address helper per array: the record of knot t of instance b (xs, st, lam: in slot 0 / 1).
OH_DEV size_t tq_knot(const TqBuffers& D, const int T, const int slot, const int b, const int t) { return ((size_t)slot * D.B + b) * T + t; }
OH_DEV double* tq_xs(const TqBuffers& D, const int T, const int slot, const int b, const int t) { return D.xs + tq_knot(D, T, slot, b, t) * TqKnot::size; }
OH_DEV double* tq_st(const TqBuffers& D, const int T, const int slot, const int b, const int t) { return D.st + tq_knot(D, T, slot, b, t) * TqStage::size; }
OH_DEV double* tq_lam(const TqBuffers& D, const int T, const int slot, const int b, const int t) { return D.lam + tq_knot(D, T, slot, b, t) * TqLam::size; }
OH_DEV double* tq_goal(const TqBuffers& D, const int T, const int b, const int t) { return D.goal + tq_knot(D, T, 0, b, t) * 4; }
OH_DEV double* tq_hc(const TqBuffers& D, const int T, const int b, const int t) { return D.hc + tq_knot(D, T, 0, b, t) * TQ_HC; }
OH_DEV double* tq_gains(const TqBuffers& D, const int T, const int b, const int t) { return D.gains + tq_knot(D, T, 0, b, t) * TQ_GN; }

// ---- setup: reference layouts -> device records ---------------------------------------------------------------------------------
// x0 [B][4 N T] = [vec(Q); vec(dQ); vec(ddQ); vec(TAU)] (only ddQ is a free variable: q, dq are rolled out, tau follows from the dynamics rows);
// p [B][2 N + 3 T] = [qc; dqc; vec(goal 3 x T)].
template <int N>
__global__ __launch_bounds__(64) void k_tq_setup(TqParams P, TqBuffers D, const double* __restrict__ x0, const double* __restrict__ p) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= D.B) return;
  const int T = P.T;
  const double* xb = x0 + (size_t)b * P.nx;
  const double* pb = p + (size_t)b * P.np;
  double q[N], dq[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    q[j] = pb[j];
    dq[j] = pb[N + j];
  }
  for (int t = 0; t < T; ++t) {
    double* r = tq_xs(D, T, 0, b, t);
    double* r1 = tq_xs(D, T, 1, b, t);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double u = xb[2 * N * T + N * t + j];
      r[TqKnot::q + j] = r1[TqKnot::q + j] = q[j];
      r[TqKnot::dq + j] = r1[TqKnot::dq + j] = dq[j];
      r[TqKnot::ddq + j] = r1[TqKnot::ddq + j] = u;
      q[j] = q[j] + P.dt * dq[j];
      dq[j] = dq[j] + P.dt * u;
    }
    for (const int blk : {TqKnot::q, TqKnot::dq, TqKnot::ddq}) r[blk + TqKnot::pad] = r1[blk + TqKnot::pad] = 0.0;
    double* gl = tq_goal(D, T, b, t);
    gl[0] = pb[2 * N + 3 * t];
    gl[1] = pb[2 * N + 3 * t + 1];
    gl[2] = pb[2 * N + 3 * t + 2];
    gl[3] = 0.0;
  }
  TqInst::fresh(P).store(D, b);
  D.list[b] = b;
}

__global__ __launch_bounds__(256) void k_tq_list(TqBuffers D) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= D.B) return;
  if (D.status[b] < 0) D.list[atomicAdd(D.n_list, 1)] = b;
}

// ---- evaluation -----------------------------------------------------------------------------------------------------------------------
// One inequality row s >= 0 under the relaxed log barrier (numpy: oracle/torque_ipm.py:evalp).  In: the slack at the trial point, slack and
// multiplier at the accepted point (none at the seed).  Out: the new multiplier (linearised complementarity  s dlam + lam ds = mu_b - lam s  with
// the slack change the step really produced, kept above 0.5 % of the old one), bco = -psi'(s) / mu_b, sig = the row's weight in the stage block,
// and the row's barrier value per unit mu_b.  Below delta = theta mu_b the logarithm is continued by its second-order Taylor polynomial.
struct TqRow {
  double lam, bco, sig, bar;
  bool relaxed;
};
OH_DEV TqRow tq_row(const double s, const double s_old, const double lam_old, const bool have_old, const double mub, const double delta, const double lam_floor) {
  TqRow r;
  r.relaxed = s < delta;
  const double sc = r.relaxed ? delta : s;
  if (r.relaxed) {
    r.bco = (2.0 * delta - s) / (delta * delta);
    r.lam = mub * r.bco;
    r.sig = mub / (delta * delta);
    const double e = (s - delta) / delta;
    r.bar = -log(delta) - e + 0.5 * e * e;
  } else {
    double lam = mub / sc;
    if (have_old) {
      lam = (mub - lam_old * (s - s_old)) / fmax(s_old, delta);
      lam = fmax(lam, lam_floor * lam_old);
      lam = fmin(fmax(lam, mub / (1e10 * sc)), 1e10 * mub / sc);
    }
    r.lam = lam;
    r.bco = 1.0 / sc;
    r.sig = lam / sc;
    r.bar = -log(sc);
  }
  return r;
}

// The lane map of both evaluation kernels: lane -> (unit in the wavefront, joint), unit -> (entry of the running list, knot).  64 / N units per
// wavefront; the lanes behind the last whole unit (lane 63 of the 7-joint arm) have none: they ride along on the last unit and keep their hands off
// LDS (lane_ok).  Units past the end of the list are clamped onto its last one and are not `active`, as are those of an instance that has finished.
template <int N>
struct TqUnit {
  static constexpr int UPW = 64 / N;  // units per wavefront (9 of the 7-joint arm)
  int ul, j, t, b;
  bool lane_ok, active;
  OH_DEV TqUnit(const TqBuffers& D, const int T, const int lane, const int block) {
    ul = lane / N, j = lane - ul * N;
    lane_ok = ul < UPW;
    if (!lane_ok) {
      ul = UPW - 1;
      j = N - 1;
    }
    const long long n_units = (long long)D.n_run * T;
    long long unit = (long long)block * UPW + ul;
    active = lane_ok && unit < n_units;
    if (unit >= n_units) unit = n_units - 1;
    const int li = (int)(unit / T);
    t = (int)(unit - (long long)li * T);
    b = D.list[li];
    if (D.status[b] >= 0) active = false;
  }
};

// Link position e = p + R p_tool at the configuration qv (models.py:826-868), its residual r = e - goal and column j of its Jacobian (models.py:1211-1264:
// z_j x (e - o_j) for a revolute joint, z_j for a prismatic one); z: the joint axes, which the second derivative needs as well.
template <int N>
OH_DEV void tq_link_column(const oh_chain* chain, const double (&qv)[N], const double* gl, const int j, double (&r)[3], double (&jp)[3], double (&z)[N][3]) {
  double R[9], pp[3], pj[N][3];
  fk_chain<N>(chain, qv, R, pp, z, pj);
  double e[3], tv3[3];
  mv3(R, chain->p_tool, tv3);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    e[k] = pp[k] + tv3[k];
    r[k] = e[k] - gl[k];
  }
  double zd[3] = {0.0, 0.0, 0.0}, pd[3] = {0.0, 0.0, 0.0};
  int jt_d = 0;
#pragma unroll
  for (int k = 0; k < N; ++k)
    if (k == j) {
      zd[0] = z[k][0]; zd[1] = z[k][1]; zd[2] = z[k][2];
      pd[0] = pj[k][0]; pd[1] = pj[k][1]; pd[2] = pj[k][2];
      jt_d = chain->jtype[k];
    }
  if (jt_d == 0) {
    const double dd[3] = {e[0] - pd[0], e[1] - pd[1], e[2] - pd[2]};
    cross3(zd, dd, jp);
  } else {
    jp[0] = zd[0]; jp[1] = zd[1]; jp[2] = zd[2];
  }
}

// One lane per (instance, knot, JOINT): 9 units x 7 joints per wavefront.  Lane j runs the reference's Newton-Euler recursion once on (Jet<1>, Jet<3>)
// scalars seeded with q_j, dq_j and ddq_j (d tau / d z is the tangent output: the derivative of the literal recursion by construction), so it ends up
// with columns j, N + j and 2 N + j of d tau / d z; the chain walk for p_link adds column j of its Jacobian.  The columns meet in LDS and every lane
// writes ITS THREE columns of the packed stage block  J^T diag(2 w_tau + Sigma) J + 2 w_p Jp^T Jp + ...,  of the two gradients (cost, barrier per unit
// mu_b) and of d tau / d z itself.  Bound: f64 FMA issue (268 registers, one wavefront per SIMD).
template <int N, bool VEL = false, bool IDS = true>
__global__ __launch_bounds__(64, IDS ? 2 : 1) void k_tq_eval3(TqParams P, TqBuffers D) {
  constexpr int NZ = 3 * N;
  constexpr int UPW = TqUnit<N>::UPW;
  // A unit's LDS.  Closed-form path: IdsWs<N> (277 doubles: two blocks per SIMD).  Jet path: tile [N + 3][NZ + 1], row coefficients, (q|dq|ddq).
  using L = IdsWs<N>;
  constexpr int TW = IDS ? L::TW : NZ + 1;                  // pitch of rows 0 .. N-1 of the tile (d tau / dz)
  constexpr int JP = IDS ? L::JP : N * (NZ + 1);            // rows of d p_link / dz, pitch NZ + 1
  constexpr int QS = IDS ? L::QS : (N + 3) * (NZ + 1) + 8 * N;
  constexpr int WS = IDS ? L::SIZE : ((QS + 24) | 1);
  __shared__ double lds_raw[UPW * WS];
  // row coefficients of joint m: which = 0 cf, 1 cb, 2 dw, 3 bar, 4 nrel, 5 viol, 6 cmpl, 7 fsum
  auto rw = [](double* tl, const int which, const int m) -> double& {
    if constexpr (IDS) return which < 6 ? tl[m * L::TW + L::RW + which] : tl[L::RW2 + (which - 6) * N + m];
    else return tl[(N + 3) * (NZ + 1) + which * N + m];
  };
  const int T = P.T;
  const int lane = threadIdx.x;
  if (blockIdx.x == 0 && lane == 0) *D.n_running = 0;  // k_tq_step, next in the stream, counts the instances that go on
  const TqUnit<N> U(D, T, lane, blockIdx.x);
  const int ul = U.ul, j = U.j, t = U.t, b = U.b;
  const bool lane_ok = U.lane_ok, active = U.active;
  if (!__any(active)) return;
  const int cur = D.cur[b], ts = 1 - cur;
  const double* xr = tq_xs(D, T, ts, b, t);
  const bool have_old = D.first[b] == 0;
  const double mub = D.mub[b], delta = P.theta * mub;

  // 1. torques and their derivative: lane j leaves its three columns in the unit's tile and keeps tau_j
  double* tl = lds_raw + ul * WS;
  double* qs_u = tl + QS;
  const double qj = xr[TqKnot::q + j], dqj = xr[TqKnot::dq + j];
  if (lane_ok) {  // the recursions read (q | dq | ddq) of their unit by a loop counter: LDS, not a lane-private array (laid out as the knot record)
    qs_u[TqKnot::q + j] = qj;
    qs_u[TqKnot::dq + j] = dqj;
    qs_u[TqKnot::ddq + j] = xr[TqKnot::ddq + j];
  }
  __syncthreads();
  double qv[N];
#pragma unroll
  for (int k = 0; k < N; ++k) qv[k] = qs_u[k];
  double tvj;
  if constexpr (IDS) {
    tvj = rnea_idsva<N>(D.dyn, tl, j, lane_ok);
  } else {
    Jet<3> tau[N];
    rnea_vw3<N + 1, Jet<3>>(D.dyn, qs_u, j, tau);
    tvj = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      tvj = (i == j) ? tau[i].v : tvj;
      if (lane_ok) {
        tl[i * TW + j] = tau[i].d[0];
        tl[i * TW + N + j] = tau[i].d[1];
        tl[i * TW + 2 * N + j] = tau[i].d[2];
      }
    }
  }

  // 2. inequality rows under the barrier: lane j takes the rows of joint j (a row costs two divisions and a logarithm: ~350 instructions -- with every
  // lane computing all 14 of them, as until round 4, they were a third of the kernel); the unit shares cf, cb, dw and the sums through LDS
  const double* lm_old = tq_lam(D, T, cur, b, t);
  double* lm_new = tq_lam(D, T, ts, b, t);
  const double* sr_old = tq_st(D, T, cur, b, t);
  const double* xr_old = tq_xs(D, T, cur, b, t);
  double cbv = 0.0, dvj = 0.0;
  {
    double tlo = 0.0, tup = 0.0, vlo = 0.0, vup = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {  // (P lives in scalar registers: no indexing by the lane)
      tlo = (i == j) ? P.tau_lo[i] : tlo;
      tup = (i == j) ? P.tau_up[i] : tup;
      if constexpr (VEL) {
        vlo = (i == j) ? P.dq_lo[i] : vlo;
        vup = (i == j) ? P.dq_up[i] : vup;
      }
    }
    const double tv_old = have_old ? sr_old[TqStage::tau + j] : 0.0;
    const TqRow lo = tq_row(tvj - tlo, tv_old - tlo, have_old ? lm_old[j] : 0.0, have_old, mub, delta, 1.0 - P.tau_ftb);
    const TqRow up = tq_row(tup - tvj, tup - tv_old, have_old ? lm_old[N + j] : 0.0, have_old, mub, delta, 1.0 - P.tau_ftb);
    double bar_j = lo.bar + up.bar;
    double nrel_j = (lo.relaxed ? 1.0 : 0.0) + (up.relaxed ? 1.0 : 0.0);
    double viol_j = fmax(tlo - tvj, tvj - tup);
    double cmpl_j = fmax(lo.lam * (tvj - tlo), up.lam * (tup - tvj));
    if (active) {
      lm_new[j] = lo.lam;
      lm_new[N + j] = up.lam;
    }
    // joint-velocity rows on the velocity states (enforce_model_limits(name, time_deriv=1), builder.py:471-509): stage-local, linear in the state
    if constexpr (VEL) {
      const double dv_old = have_old ? xr_old[TqKnot::dq + j] : 0.0;
      const TqRow l2 = tq_row(dqj - vlo, dv_old - vlo, have_old ? lm_old[TqLam::vel + j] : 0.0, have_old, mub, delta, 1.0 - P.tau_ftb);
      const TqRow u2 = tq_row(vup - dqj, vup - dv_old, have_old ? lm_old[TqLam::vel + N + j] : 0.0, have_old, mub, delta, 1.0 - P.tau_ftb);
      bar_j += l2.bar + u2.bar;
      nrel_j += (l2.relaxed ? 1.0 : 0.0) + (u2.relaxed ? 1.0 : 0.0);
      viol_j = fmax(viol_j, fmax(vlo - dqj, dqj - vup));
      cmpl_j = fmax(cmpl_j, fmax(l2.lam * (dqj - vlo), u2.lam * (vup - dqj)));
      cbv = u2.bco - l2.bco;
      dvj = l2.sig + u2.sig;
      if (active) {
        lm_new[TqLam::vel + j] = l2.lam;
        lm_new[TqLam::vel + N + j] = u2.lam;
      }
    }
    __syncthreads();  // (the last row of d tau / dz is in its slot: the slots' spare words are free)
    if (lane_ok) {
      rw(tl, 0, j) = 2.0 * P.w_tau * tvj;              // cf
      rw(tl, 1, j) = up.bco - lo.bco;                  // cb
      rw(tl, 2, j) = 2.0 * P.w_tau + lo.sig + up.sig;  // dw
      rw(tl, 3, j) = bar_j;
      rw(tl, 4, j) = nrel_j;
      rw(tl, 5, j) = viol_j;
      rw(tl, 6, j) = cmpl_j;
      rw(tl, 7, j) = fma(P.w_tau * tvj, tvj, P.w_vel * dqj * dqj);
    }
  }

  // 3. link position and column j of its Jacobian (models.py:826-868, 1211-1264); its rows take the place of the screws and of (q | dq | ddq)
  double jp[3], r[3];
  {
    double z[N][3];
    tq_link_column<N>(D.chain, qv, tq_goal(D, T, b, t), j, r, jp, z);
  }
  if (lane_ok) {  // the link position has no dq / ddq columns
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      tl[JP + k * (NZ + 1) + j] = jp[k];
      tl[JP + k * (NZ + 1) + N + j] = 0.0;
      tl[JP + k * (NZ + 1) + 2 * N + j] = 0.0;
    }
  }
  __syncthreads();

  // 4. components j, N + j, 2 N + j of the gradient of the cost and of the barrier (per unit mu_b), the lane's three columns of the stage block
  double dw[N], J0[N], J1[N], J2[N];
  double g0 = 0.0, g1 = 0.0, g2 = 0.0, h0 = 0.0, h1 = 0.0, h2 = 0.0;
  double bar = 0.0, viol = 0.0, cmpl = 0.0, fsum = 0.0;
  int nrel = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double cf = rw(tl, 0, i), cb = rw(tl, 1, i);
    dw[i] = rw(tl, 2, i);
    bar += rw(tl, 3, i);
    nrel += (int)rw(tl, 4, i);
    viol = fmax(viol, rw(tl, 5, i));
    cmpl = fmax(cmpl, rw(tl, 6, i));
    fsum += rw(tl, 7, i);
    J0[i] = tl[i * TW + j];
    J1[i] = tl[i * TW + N + j];
    J2[i] = tl[i * TW + 2 * N + j];
    g0 = fma(cf, J0[i], g0);
    g1 = fma(cf, J1[i], g1);
    g2 = fma(cf, J2[i], g2);
    h0 = fma(cb, J0[i], h0);
    h1 = fma(cb, J1[i], h1);
    h2 = fma(cb, J2[i], h2);
  }
  g0 += 2.0 * P.w_path * dot3(jp, r);
  g1 += 2.0 * P.w_vel * dqj;
  h1 += cbv;
  double* sr = tq_st(D, T, ts, b, t);
  // exact curvature, stored term (D.curv = 2: k_tq_curv computed it at an earlier evaluation of this instance and skips this one): added as the block is written
  const double* hc = tq_hc(D, T, b, t);
  const bool add_hc = D.curv[b] == 2;
  if (active) {
#pragma unroll
    for (int c3 = 0; c3 < 3; ++c3) {
      const int d = c3 * N + j;
      double col[N];
#pragma unroll
      for (int i = 0; i < N; ++i) col[i] = dw[i] * (c3 == 0 ? J0[i] : (c3 == 1 ? J1[i] : J2[i]));
      for (int rr = d; rr < NZ; ++rr) {
        double hv = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) hv = fma(tl[i * TW + rr], col[i], hv);
        if (c3 == 0) {
          double hp = 0.0;
#pragma unroll
          for (int k = 0; k < 3; ++k) hp = fma(tl[JP + k * (NZ + 1) + rr], jp[k], hp);
          hv = fma(2.0 * P.w_path, hp, hv);
        }
        if (rr == d && c3 == 1) {
          hv += 2.0 * P.w_vel;
          hv += dvj;
        }
        if (add_hc) hv += hc[tq_packed(rr, d)];
        sr[TqStage::H + tq_packed(rr, d)] = hv;
      }
#pragma unroll
      for (int i = 0; i < N; ++i) sr[TqStage::J + i * NZ + d] = c3 == 0 ? J0[i] : (c3 == 1 ? J1[i] : J2[i]);
    }
    sr[TqStage::g_f + j] = g0;
    sr[TqStage::g_f + N + j] = g1;
    sr[TqStage::g_f + 2 * N + j] = g2;
    sr[TqStage::g_b + j] = h0;
    sr[TqStage::g_b + N + j] = h1;
    sr[TqStage::g_b + 2 * N + j] = h2;
    if (j == 0) {
      sr[TqStage::f] = P.w_path * dot3(r, r) + fsum;
      sr[TqStage::barrier] = bar;
      sr[TqStage::relaxed] = (double)nrel;
      sr[TqStage::viol] = viol;
      sr[TqStage::cmpl] = cmpl;
    }
    sr[TqStage::tau + j] = tvj;
  }
}

// Exact curvature of the Lagrangian for the instances the step kernel has switched to Newton steps (D.curv): adds
//     sum_i cH_i d^2 tau_i / dz^2,  cH = 2 w_tau tau - lam_lo + lam_up   (the multiplier of the dynamics row TAU_i - rnea_i = 0 at a stationary point)
//   + 2 w_p sum_k r_k d^2 p_k / dq^2,  d^2 p / dq_a dq_b = z_b x (z_a x (e - o_a)) for b <= a
// to the stage block k_tq_eval3 has just written.  One lane per (instance, knot, joint) again: lane j runs the hand-written adjoint of the recursion on
// (Jet<1>, Jet<2>) scalars seeded with q_j and dq_j, which yields rows q_j and dq_j of the first term; every packed entry is owned by exactly one lane.
// Round 5: the term also goes to a record of its own (D.hc), and an instance computes it afresh only at every
// (curv_lag + 1)-th evaluation (D.curv: 1 compute here, 2 k_tq_eval3 adds the stored term as it writes the block and this kernel skips the instance).  Near the solution the term moves little between steps: with a lag of 3 the
// port takes 24.70 instead of 24.64 steps on 256 instances and computes the term 3.2 times per solve instead of 11.3 (oracle/torque_ipm.py, HISTORY).
#ifndef OH_TQ_CURV_WAVES
#define OH_TQ_CURV_WAVES 1
#endif
template <int N>
__global__ __launch_bounds__(64, OH_TQ_CURV_WAVES) void k_tq_curv(TqParams P, TqBuffers D) {
  constexpr int UPW = TqUnit<N>::UPW;
  __shared__ double zs_l[UPW][TqKnot::size + 8];  // a unit's knot record (q | dq | ddq) and, behind it, cH
  const int T = P.T;
  const int lane = threadIdx.x;
  const TqUnit<N> U(D, T, lane, blockIdx.x);
  const int ul = U.ul, j = U.j, t = U.t, b = U.b;
  const bool lane_ok = U.lane_ok;
  const bool comp = U.active && D.curv[b] == 1;  // (2: k_tq_eval3 has added the stored term already)
  if (!__any(comp)) return;
  const int ts = 1 - D.cur[b];
  const double* xr = tq_xs(D, T, ts, b, t);
  double* sr = tq_st(D, T, ts, b, t);
  double* H = sr + TqStage::H;
  double* hc = tq_hc(D, T, b, t);
  const double* lm = tq_lam(D, T, ts, b, t);
  const bool direct = P.curv_lag <= 0;
  if (lane_ok) {
    zs_l[ul][TqKnot::q + j] = xr[TqKnot::q + j];
    zs_l[ul][TqKnot::dq + j] = xr[TqKnot::dq + j];
    zs_l[ul][TqKnot::ddq + j] = xr[TqKnot::ddq + j];
    zs_l[ul][TqKnot::size + j] = 2.0 * P.w_tau * sr[TqStage::tau + j] - lm[j] + lm[N + j];
  }
  __syncthreads();
  // curvature of the tracking term
  double inner[3], r[3], z[N][3];
  {
    double qv[N];
#pragma unroll
    for (int k = 0; k < N; ++k) qv[k] = zs_l[ul][TqKnot::q + k];
    tq_link_column<N>(D.chain, qv, tq_goal(D, T, b, t), j, r, inner, z);
  }
  if (comp) {
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (k <= j) {  // rows q_j, columns up to the diagonal (this lane's entries: the store initialises them, the adjoint below adds to them)
        double x[3] = {0.0, 0.0, 0.0};
        if (D.chain->jtype[k] == 0) cross3(z[k], inner, x);
        const double v = 2.0 * P.w_path * dot3(r, x);
        H[tq_packed(j, k)] += v;
        if (!direct) hc[tq_packed(j, k)] = v;
      }
  }
  rnea_ctau_grad_inv<N + 1, Jet<2>, Jet<1>>(D.dyn, zs_l[ul], j, [&](const int k, const Jet<2> gq, const Jet<2> gqd, const Jet<2> gqdd) {
    if (!comp) return;
    // onto the stage block ...
    if (k <= j) {
      H[tq_packed(j, k)] += gq.d[0];
      H[tq_packed(N + j, N + k)] += gqd.d[1];
    }
    H[tq_packed(N + j, k)] += gq.d[1];
    H[tq_packed(2 * N + k, j)] += gqdd.d[0];
    if (direct) return;  // curv_lag = 0: nothing is kept
    // ... and into the record the next evaluations of this instance add instead (k_tq_eval3)
    if (k <= j) {  // rows q_j and dq_j, columns up to the diagonal
      hc[tq_packed(j, k)] += gq.d[0];
      hc[tq_packed(N + j, N + k)] = gqd.d[1];
    }
    hc[tq_packed(N + j, k)] = gq.d[1];        // (dq_j, q_k)
    hc[tq_packed(2 * N + k, j)] = gqdd.d[0];  // (ddq_k, q_j)
  });
}

// ---- step ------------------------------------------------------------------------------------------------------------------------------
OH_DEV double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
OH_DEV double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}
OH_DEV double wave_min(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
  return v;
}
OH_DEV double row_sum8(double v) {  // sum over the 8 lanes of a row (lane = 8 r + c)
  v += __shfl_xor(v, 1, 8);
  v += __shfl_xor(v, 2, 8);
  v += __shfl_xor(v, 4, 8);
  return v;
}

// One wavefront per instance (round 4; rounds 1-3: 16 lanes per instance around a value matrix in LDS, every lane factorising Q_uu for itself, three
// block barriers per knot -- 105 us per sweep however small the batch).  Lane 8 r + c owns entry (r, c) of every N x N block of the stage matrix
//     M = H_t + [A^T P A, A^T P B; B^T P A, B^T P B] + mu I_x   over (q, dq | u),
// column c = N holds the vectors.  With A = [[I, dt I], [0, I]], B = [0; dt I] every block of M is an entry-wise combination of the four blocks of P,
// so forming M needs nothing from another lane; the N pivots of the u rows are then eliminated by Gauss-Jordan steps whose operands travel by lane
// shuffles (row r of the pivot column, column c of the pivot row): no LDS, no barrier.  What remains in the x rows is the Schur complement
// P' = Q_xx - Q_ux^T Q_uu^{-1} Q_ux (exactly symmetric: mirrored entries subtract the same product), in the u rows the gains K = Q_uu^{-1} Q_ux and
// k = Q_uu^{-1} q_u; the pivots are those of the Cholesky factorisation (positive iff Q_uu is positive definite).  The roll-outs and the costate
// recursion use the same layout: entry-wise work on the lanes that hold it, row sums by three shuffles.  numpy: oracle/torque_ipm.py.
template <int N>
struct TqLanes {
  int lane, r, c;
  bool mat, vec;  // an entry of the N x N blocks; an entry of the vectors
  OH_DEV explicit TqLanes(const int l) : lane(l), r(l >> 3), c(l & 7), mat(r < N && c < N), vec(r < N && c == N) {}
};

// Step 1, lane-parallel part: the sums over the trial's stage records (knots over the lanes).
OH_DEV TqTrial tq_trial_sums(const TqBuffers& D, const int T, const int b, const int ts, const int lane) {
  TqTrial tr{0.0, 0.0, 0.0, 0.0};
  for (int t = lane; t < T; t += 64) {
    const double* sr = tq_st(D, T, ts, b, t);
    tr.f += sr[TqStage::f];
    tr.bsum += sr[TqStage::barrier];
    tr.nrel += sr[TqStage::relaxed];
    tr.viol = fmax(tr.viol, sr[TqStage::viol]);
  }
  tr.f = wave_sum(tr.f);
  tr.bsum = wave_sum(tr.bsum);
  tr.nrel = wave_sum(tr.nrel);
  tr.viol = wave_max(tr.viol);
  return tr;
}

// Step 2: reduced gradient of the accepted point: gradient of the rolled-out merit w.r.t. u_t by the costate recursion, for mu_b, for its successor and
// for the watchdog's.  Entry-wise per joint: lanes (r, N) carry the costates of q_r and dq_r for the cost and the barrier part; what a knot needs from
// memory is requested one knot ahead.
template <int N>
OH_DEV TqStat tq_reduced_gradient(const TqBuffers& D, const int T, const int b, const int cur, const TqLanes<N>& L, const double dt, const double mub, const TqBarrier& nb) {
  constexpr int NX = 2 * N;
  const int r = L.r;
  const bool vec = L.vec;
  double stat = 0.0, stat_next = 0.0, stat_up = 0.0;
  double lfq = 0.0, lfd = 0.0, lbq = 0.0, lbd = 0.0;
  double g_n[6] = {0, 0, 0, 0, 0, 0};
  auto fetch = [&](const int t) {
    if (vec) {
      const double* sr = tq_st(D, T, cur, b, t);
      g_n[0] = sr[TqStage::g_f + r]; g_n[1] = sr[TqStage::g_f + N + r]; g_n[2] = sr[TqStage::g_f + NX + r];
      g_n[3] = sr[TqStage::g_b + r]; g_n[4] = sr[TqStage::g_b + N + r]; g_n[5] = sr[TqStage::g_b + NX + r];
    }
  };
  fetch(T - 1);
  for (int t = T - 1; t >= 0; --t) {
    const double gfq = g_n[0], gfd = g_n[1], gfu = g_n[2], gbq = g_n[3], gbd = g_n[4], gbu = g_n[5];
    if (t > 0) fetch(t - 1);
    const double rf = fma(dt, lfd, gfu), rb = fma(dt, lbd, gbu);
    stat = fmax(stat, fabs(fma(mub, rb, rf)));
    stat_next = fmax(stat_next, fabs(fma(nb.next, rb, rf)));
    stat_up = fmax(stat_up, fabs(fma(nb.up, rb, rf)));
    const double nfd = gfd + fma(dt, lfq, lfd), nbd = gbd + fma(dt, lbq, lbd);
    lfq = gfq + lfq;
    lbq = gbq + lbq;
    lfd = nfd;
    lbd = nbd;
  }
  if (!vec) { stat = 0.0; stat_next = 0.0; stat_up = 0.0; }
  stat = wave_max(stat);
  stat_next = wave_max(stat_next);
  stat_up = wave_max(stat_up);
  if (!(stat == stat)) stat = 1e300;
  if (!(stat_next == stat_next)) stat_next = 1e300;
  if (!(stat_up == stat_up)) stat_up = 1e300;
  return TqStat{stat, stat_next, stat_up};
}

// Step 4: Riccati sweep (uniform over the wavefront: one instance); the gains go to D.gains, q_u^T k to S.qk.  A stage block of the exact Hessian that
// leaves Q_uu indefinite raises the damping and the sweep is repeated; true: twelve sweeps failed.
template <int N>
OH_DEV bool tq_riccati(const TqBuffers& D, const int T, const int b, const TqLanes<N>& L, const double dt, TqInst& S) {
  constexpr int NX = 2 * N;
  const int lane = L.lane, r = L.r, c = L.c, cur = S.cur;
  const bool mat = L.mat;
  const double mub = S.mub;
  // offsets of this lane's entries in the packed lower stage block; q at 0, dq at N, u at 2 N
  auto pk = [](const int row, const int col) { return TqStage::H + (row >= col ? tq_packed(row, col) : tq_packed(col, row)); };
  const int rr = mat ? r : 0, cc = mat ? c : 0;
  const int o_qq = pk(rr, cc), o_qd = pk(rr, N + cc), o_dq = pk(N + rr, cc), o_dd = pk(N + rr, N + cc), o_qu = pk(rr, NX + cc), o_du = pk(N + rr, NX + cc),
            o_uq = pk(NX + rr, cc), o_ud = pk(NX + rr, N + cc), o_uu = pk(NX + rr, NX + cc);
  const int rv = L.vec ? r : 0;
  bool failed = true;
  for (int attempt = 0; attempt < 12 && failed; ++attempt) {
    failed = false;
    S.qk = 0.0;
    double Pqq = 0.0, Pqd = 0.0, Pdq = 0.0, Pdd = 0.0;  // mat lanes: blocks of P; vec lanes: Pqq = p_q[r], Pdd = p_d[r]
    double h_n[9];
    auto fetch_rec = [&](const int t) {
      const double* sr = tq_st(D, T, cur, b, t);
      if (mat) {
        h_n[0] = sr[o_qq]; h_n[1] = sr[o_qd]; h_n[2] = sr[o_dq]; h_n[3] = sr[o_dd]; h_n[4] = sr[o_qu]; h_n[5] = sr[o_du]; h_n[6] = sr[o_uq]; h_n[7] = sr[o_ud];
        h_n[8] = sr[o_uu];
      } else {  // the stage gradient g_f + mu_b g_b
        h_n[0] = fma(mub, sr[TqStage::g_b + rv], sr[TqStage::g_f + rv]);
        h_n[1] = fma(mub, sr[TqStage::g_b + N + rv], sr[TqStage::g_f + N + rv]);
        h_n[2] = fma(mub, sr[TqStage::g_b + NX + rv], sr[TqStage::g_f + NX + rv]);
      }
    };
    fetch_rec(T - 1);
    for (int t = T - 1; t >= 0; --t) {
      double Mqq, Mqd, Mdq, Mdd, Mqu, Mdu, Muq, Mud, Muu;
      if (c < N) {
        const double dg = (r == c) ? S.mu : 0.0;
        Mqq = h_n[0] + Pqq + dg;
        Mqd = h_n[1] + fma(dt, Pqq, Pqd);
        Mdq = h_n[2] + fma(dt, Pqq, Pdq);
        Mdd = h_n[3] + fma(dt, fma(dt, Pqq, Pqd), fma(dt, Pdq, Pdd)) + dg;
        Mqu = h_n[4] + dt * Pqd;
        Mdu = h_n[5] + dt * fma(dt, Pqd, Pdd);
        Muq = h_n[6] + dt * Pdq;
        Mud = h_n[7] + dt * fma(dt, Pdq, Pdd);
        Muu = h_n[8] + dt * dt * Pdd;
      } else {  // vectors: m_q, m_d, m_u in the slots of column "u" of their block row (Mqu, Mdu, Muu)
        Mqq = Mqd = Mdq = Mdd = Muq = Mud = 0.0;
        Mqu = h_n[0] + Pqq;
        Mdu = h_n[1] + fma(dt, Pqq, Pdd);
        Muu = h_n[2] + dt * Pdd;
      }
      if (t > 0) fetch_rec(t - 1);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        // column j of this lane's row (blocks X u) and row j of this lane's column (blocks u Y; for the vector column: m_u[j])
        const double cq = __shfl(Mqu, 8 * r + j), cd = __shfl(Mdu, 8 * r + j), cu = __shfl(Muu, 8 * r + j);
        const double rq = __shfl(Muq, 8 * j + c), rd = __shfl(Mud, 8 * j + c), ru = __shfl(Muu, 8 * j + c);
        const double piv = readlane_f64(Muu, 9 * j);
        if (!(piv > 0.0) || !isfinite(piv)) failed = true;
        double d = __builtin_amdgcn_rcp(piv);  // reciprocal to the last bit or two (two Newton steps): an IEEE division is 30 instructions on the critical path of every pivot
        d = d * fma(-piv, d, 2.0);
        d = d * fma(-piv, d, 2.0);
        if (c < N) {
          Mqq = fma(-(cq * rq), d, Mqq);
          Mqd = fma(-(cq * rd), d, Mqd);
          Mdq = fma(-(cd * rq), d, Mdq);
          Mdd = fma(-(cd * rd), d, Mdd);
          Mqu = fma(-(cq * ru), d, Mqu);
          Mdu = fma(-(cd * ru), d, Mdu);
          if (r == j) {
            Muq *= d;
            Mud *= d;
            Muu *= d;
          } else {
            Muq = fma(-(cu * rq), d, Muq);
            Mud = fma(-(cu * rd), d, Mud);
            Muu = fma(-(cu * ru), d, Muu);
          }
        } else {  // ru = m_u[j] (forward-eliminated: row j has only been updated by the pivots before it)
          if (r == 0) S.qk = fma(ru * ru, d, S.qk);
          Mqu = fma(-(cq * ru), d, Mqu);
          Mdu = fma(-(cd * ru), d, Mdu);
          if (r == j) Muu *= d;
          else Muu = fma(-(cu * ru), d, Muu);
        }
      }
      // gains of knot t: K_q[r][c], K_d[r][c] on the matrix lanes, k[r] on the vector lanes; two doubles per lane
      double* gn = tq_gains(D, T, b, t);
      gn[2 * lane] = c < N ? Muq : Muu;
      gn[2 * lane + 1] = c < N ? Mud : 0.0;
      if (c < N) {
        Pqq = Mqq; Pqd = Mqd; Pdq = Mdq; Pdd = Mdd;
      } else {
        Pqq = Mqu; Pdd = Mdu; Pqd = Pdq = 0.0;
      }
    }
    S.qk = __shfl(S.qk, N);  // lane (0, N)
    failed = __any(failed && r < N) || !isfinite(S.qk);
    if (failed) tq_raise_damping(S);  // an indefinite stage block of the exact Hessian: more damping, same point
  }
  return failed;
}

// Step 5: closed-loop rollout of the unit step (du to LDS), fraction to the boundary on the linearised rows.  Lane (r, c) carries the state step of joint
// c (replicated over the rows) and multiplies it with its entries of the gains and of d tau / d z; row sums give du_r and d tau_r.  After a sweep
// (do_gains) |dx|^2 goes to S.ndx and the fraction alpha to S.alpha; a step that is only retried shorter keeps both.
template <int N, bool VEL>
OH_DEV void tq_unit_step(const TqParams& P, const TqBuffers& D, const int T, const int b, const TqLanes<N>& L, const double delta, double (*du_all)[8], const bool do_gains, TqInst& S) {
  constexpr int NX = 2 * N, NZ = 3 * N;
  const int lane = L.lane, r = L.r, c = L.c, cur = S.cur;
  const bool mat = L.mat;
  const double dt = P.dt;
  double dq = 0.0, dd = 0.0;
  double a_ftb = 1.0, ndx_acc = 0.0;
  double k_n[2], j_n[3], s_n[4] = {0, 0, 0, 0};
  auto fetch_knot = [&](const int t) {
    const double* gn = tq_gains(D, T, b, t);
    k_n[0] = gn[2 * lane];
    k_n[1] = gn[2 * lane + 1];
    const double* sr = tq_st(D, T, cur, b, t);
    if (mat) {
      j_n[0] = sr[TqStage::J + r * NZ + c];
      j_n[1] = sr[TqStage::J + r * NZ + N + c];
      j_n[2] = sr[TqStage::J + r * NZ + NX + c];
    } else {
      j_n[0] = j_n[1] = j_n[2] = 0.0;
    }
    if (r < N && c == 0) {
      const double tv = sr[TqStage::tau + r];
      s_n[0] = tv - P.tau_lo[r];
      s_n[1] = P.tau_up[r] - tv;
      if constexpr (VEL) {
        const double dv = tq_xs(D, T, cur, b, t)[TqKnot::dq + r];
        s_n[2] = dv - P.dq_lo[r];
        s_n[3] = P.dq_up[r] - dv;
      }
    }
  };
  fetch_knot(0);
  for (int t = 0; t < T; ++t) {
    const double kq = k_n[0], kd = k_n[1], jq = j_n[0], jd = j_n[1], ju = j_n[2];
    const double s_lo = s_n[0], s_up = s_n[1], v_lo = s_n[2], v_up = s_n[3];
    if (t + 1 < T) fetch_knot(t + 1);
    // du_r = -k_r - sum_c (K_q[r][c] dq_c + K_d[r][c] dd_c): the vector lane contributes k_r (its kq slot)
    const double part = c < N ? fma(kq, dq, kd * dd) : (c == N ? kq : 0.0);  // (columns beyond N exist on chains shorter than seven joints: idle lanes)
    const double du_r = -row_sum8(r < N ? part : 0.0);
    const double du_c = __shfl(du_r, 8 * c);  // du of joint c, from row c
    if (r == 0 && c < N) du_all[t][c] = du_c;
    if (r == 0 && c < N) ndx_acc = fma(dq, dq, fma(dd, dd, ndx_acc));
    const double ds = row_sum8(mat ? fma(jq, dq, fma(jd, dd, ju * du_c)) : 0.0);  // d tau_r of the unit step
    double dv = 0.0;
    if constexpr (VEL) dv = __shfl(dd, r);  // the velocity step of joint r sits on lane (0, r) (every lane takes part in the shuffle)
    if (r < N && c == 0) {
      if (ds < 0.0 && s_lo >= delta) a_ftb = fmin(a_ftb, -P.tau_ftb * s_lo / ds);
      if (ds > 0.0 && s_up >= delta) a_ftb = fmin(a_ftb, P.tau_ftb * s_up / ds);
      if constexpr (VEL) {
        if (dv < 0.0 && v_lo >= delta) a_ftb = fmin(a_ftb, -P.tau_ftb * v_lo / dv);
        if (dv > 0.0 && v_up >= delta) a_ftb = fmin(a_ftb, P.tau_ftb * v_up / dv);
      }
    }
    // dx_{t+1} = A dx_t + B du_t
    dq = fma(dt, dd, dq);
    dd = fma(dt, du_c, dd);
  }
  if (do_gains) {
    S.ndx = wave_sum(ndx_acc);
    S.alpha = wave_min(a_ftb);
  }
}

// Step 6: open-loop rollout of u + alpha du from the fixed initial state into the slot of the next trial: lane c < N carries joint c.
OH_DEV void tq_trial_rollout(const TqBuffers& D, const int T, const int b, const int cur, const int lane, const double dt, const double alpha, double (*du_all)[8]) {
  const int nts = 1 - cur;
  const double* x0r = tq_xs(D, T, cur, b, 0);
  double q = x0r[TqKnot::q + lane], dqv = x0r[TqKnot::dq + lane];
  double u_n = x0r[TqKnot::ddq + lane];
  for (int t = 0; t < T; ++t) {
    const double ucur = u_n;
    if (t + 1 < T) u_n = tq_xs(D, T, cur, b, t + 1)[TqKnot::ddq + lane];
    double* xn = tq_xs(D, T, nts, b, t);
    const double un = fma(alpha, du_all[t][lane], ucur);
    xn[TqKnot::ddq + lane] = un;
    xn[TqKnot::q + lane] = q;
    xn[TqKnot::dq + lane] = dqv;
    // x_{t+1} = A x_t + B u_t on the trial values themselves
    q = fma(dt, dqv, q);
    dqv = fma(dt, un, dqv);
  }
}

// The step of one instance (scalar steps: oh_tq_machine.h):
//   1. merit of the trial  f + mu_b B  and the ratio test against the decrease the damped model predicted for the scaled step; Levenberg-Marquardt update
//   2. reduced gradient of the accepted point by the costate recursion, for the barrier parameter in force and for the next one
//   3. convergence / barrier update (the stage gradient is  g_f + mu_b g_b,  the merit  f + mu_b B:  a new mu_b needs no re-evaluation)
//   4. Riccati sweep; a stage block of the exact Hessian that leaves Q_uu indefinite raises the damping and the sweep is repeated
//   5. closed-loop rollout of the unit step: the control steps go to LDS, the linearised rows give the fraction to the boundary alpha
//   6. open-loop rollout of  u + alpha du  on the trial values themselves (the Euler rows hold to the rounding of one operation)
// A trial that left the domain of the arithmetic, or a boundary-shortened step that was rejected, is retried shorter: steps 5-6 only.
#ifndef OH_TQ_STEP_WAVES
#define OH_TQ_STEP_WAVES 2
#endif
template <int N, bool VEL = false>
__global__ __launch_bounds__(64, OH_TQ_STEP_WAVES) void k_tq_step(TqParams P, TqBuffers D) {
  static_assert(N >= 1 && N <= 7, "the lane layout is 8 rows x 8 columns: up to 7 joints and the vector column (column N)");
  extern __shared__ double du_dyn[];  // [T][8]: the control steps of the unit step
  double (*du_all)[8] = reinterpret_cast<double (*)[8]>(du_dyn);
  const int T = P.T;
  const TqLanes<N> L(threadIdx.x);
  if ((int)blockIdx.x >= D.n_run) return;
  const int b = D.list[blockIdx.x];
  if (D.status[b] >= 0) return;
  TqInst S = TqInst::load(D, b);
  const TqTrial tr = tq_trial_sums(D, T, b, 1 - S.cur, L.lane);  // 1.
  TqVerdict v;
  tq_ratio_test(S, P, tr, v);
  const TqBarrier nb = tq_barrier_candidates(S.mub, P);  // 2.
  const TqStat st = tq_reduced_gradient<N>(D, T, b, S.cur, L, P.dt, S.mub, nb);
  TqPlan pl;
  tq_decide(S, P, v, st, nb, pl);  // 3.
  if (pl.do_gains && tq_riccati<N>(D, T, b, L, P.dt, S)) {  // 4.
    pl.status = OH_STATUS_NUMERICAL;
    pl.do_roll = false;
  }
  const double delta = P.theta * S.mub;  // rows below it are in the relaxed zone
  if (pl.do_roll) tq_unit_step<N, VEL>(P, D, T, b, L, delta, du_all, pl.do_gains, S);  // 5.
  __syncthreads();  // du_all
  if (pl.do_roll && L.lane < N) tq_trial_rollout(D, T, b, S.cur, L.lane, P.dt, S.alpha, du_all);  // 6.
  if (L.lane == 0) {
    tq_next_curvature(S, P, v.accept, pl.curv);
    S.first = pl.reeval ? 1 : 0;
    S.status = pl.status;
    S.store(D, b);
    if (S.status < 0) atomicAdd(D.n_running, 1);
  }
}

// ---- results in the reference layout ------------------------------------------------------------------------------------------------
// Multipliers: lam_i = mu_b / s_i, the point of the central path the iteration stopped at (lam_i s_i = mu_b <= tol_compl on every row, and with them
// the reduced gradient of the Lagrangian is the `stat` the iteration tested).
template <int N>
__global__ __launch_bounds__(64) void k_tq_finalize(TqParams P, TqBuffers D, double* __restrict__ x, double* __restrict__ f, double* __restrict__ kkt,
                                                    int* __restrict__ iters, int* __restrict__ status, double* __restrict__ mult) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= D.B) return;
  const int T = P.T, cur = D.cur[b];
  const double mub = D.mub[b];
  double cmpl = 0.0;
  for (int t = 0; t < T; ++t) {
    const double* xr = tq_xs(D, T, cur, b, t);
    const double* sr = tq_st(D, T, cur, b, t);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      if (x) {
        double* xb = x + (size_t)b * P.nx;
        xb[N * t + j] = xr[TqKnot::q + j];
        xb[N * T + N * t + j] = xr[TqKnot::dq + j];
        xb[2 * N * T + N * t + j] = xr[TqKnot::ddq + j];
        xb[3 * N * T + N * t + j] = sr[TqStage::tau + j];
      }
      const double tv = sr[TqStage::tau + j];
      const double s_lo = tv - P.tau_lo[j], s_up = P.tau_up[j] - tv;
      const double l_lo = mub / fmax(s_lo, 1e-300), l_up = mub / fmax(s_up, 1e-300);
      cmpl = fmax(cmpl, fmax(fabs(l_lo * s_lo), fabs(l_up * s_up)));
      const int NR = P.vel ? 4 * N : 2 * N;  // rows per knot: effort rows, then (with velocity limits) [dq - dq_lo; dq_up - dq]
      if (mult) {
        mult[((size_t)b * T + t) * NR + j] = l_lo;
        mult[((size_t)b * T + t) * NR + N + j] = l_up;
      }
      if (P.vel) {
        const double v_lo = xr[TqKnot::dq + j] - P.dq_lo[j], v_up = P.dq_up[j] - xr[TqKnot::dq + j];
        const double m_lo = mub / fmax(v_lo, 1e-300), m_up = mub / fmax(v_up, 1e-300);
        cmpl = fmax(cmpl, fmax(fabs(m_lo * v_lo), fabs(m_up * v_up)));
        if (mult) {
          mult[((size_t)b * T + t) * NR + 2 * N + j] = m_lo;
          mult[((size_t)b * T + t) * NR + 3 * N + j] = m_up;
        }
      }
    }
  }
  if (f) f[b] = D.f_true[b];
  if (kkt) {
    kkt[3 * b] = D.stat[b];
    kkt[3 * b + 1] = fmax(0.0, D.viol[b]);
    kkt[3 * b + 2] = cmpl;
  }
  if (iters) iters[b] = D.iters[b];
  int st = D.status[b] < 0 ? OH_STATUS_MAX_ITER : D.status[b];
  if (P.vel) {
    // dq_0 = dqc is pinned (fix_configuration on the velocity state), so its velocity-limit rows are constants of the instance: outside them there is no
    // feasible point -- IPOPT's "infeasible problem" (solver.py:407-412); the interior point above can only sit in the relaxed barrier until its cap
    const double* x0r = tq_xs(D, T, cur, b, 0);
    double worst = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) worst = fmin(worst, fmin(x0r[TqKnot::dq + j] - P.dq_lo[j], P.dq_up[j] - x0r[TqKnot::dq + j]));
    if (worst < -1e-9) {
      st = OH_STATUS_INFEASIBLE;
      if (kkt) kkt[3 * b + 1] = fmax(kkt[3 * b + 1], -worst);
    }
  }
  if (status) status[b] = st;
}

}  // namespace

// The solver's kernels by chain length: 2 .. 7 joints (k_tq_step's lane layout is 8 x 8: N joints and the vector column)
#define OH_TQ_DISPATCH(n, C) \
  switch (n) {               \
    case 2: C(2); break;     \
    case 3: C(3); break;     \
    case 4: C(4); break;     \
    case 5: C(5); break;     \
    case 6: C(6); break;     \
    case 7: C(7); break;     \
    default: return false;   \
  }
bool oh_launch_tq_setup(hipStream_t s, const TqParams& P, const TqBuffers& D, const double* x0, const double* p) {
#define C(NN) hipLaunchKernelGGL(k_tq_setup<NN>, dim3((D.B + 63) / 64), dim3(64), 0, s, P, D, x0, p)
  OH_TQ_DISPATCH(P.N, C)
#undef C
  return true;
}
void oh_launch_tq_list(hipStream_t s, const TqBuffers& D) { hipLaunchKernelGGL(k_tq_list, dim3((D.B + 255) / 256), dim3(256), 0, s, D); }
bool oh_launch_tq_eval(hipStream_t s, const TqParams& P, const TqBuffers& D) {
  const long long units = (long long)D.n_run * P.T;
  // (the variants with joint-velocity rows are instantiations of their own: as a run-time branch the rows cost k_tq_eval3 21 % at 8192 instances)
  // a wavefront holds 64 / N units (nine of the 7-joint arm)
#define C(NN)                                                                                             \
  {                                                                                                       \
    const dim3 grid((unsigned)((units + (64 / NN) - 1) / (64 / NN)));                                     \
    if (P.jac_closed_form) {                                                                              \
      if (P.vel) hipLaunchKernelGGL((k_tq_eval3<NN, true, true>), grid, dim3(64), 0, s, P, D);            \
      else hipLaunchKernelGGL((k_tq_eval3<NN, false, true>), grid, dim3(64), 0, s, P, D);                 \
    } else {                                                                                              \
      if (P.vel) hipLaunchKernelGGL((k_tq_eval3<NN, true, false>), grid, dim3(64), 0, s, P, D);           \
      else hipLaunchKernelGGL((k_tq_eval3<NN, false, false>), grid, dim3(64), 0, s, P, D);                \
    }                                                                                                     \
    hipLaunchKernelGGL(k_tq_curv<NN>, grid, dim3(64), 0, s, P, D); /* exits at once where no instance takes Newton steps */ \
  }
  OH_TQ_DISPATCH(P.N, C)
#undef C
  return true;
}
bool oh_launch_tq_step(hipStream_t s, const TqParams& P, const TqBuffers& D) {
#define C(NN)                                                                                                              \
  {                                                                                                                        \
    if (P.vel) hipLaunchKernelGGL((k_tq_step<NN, true>), dim3(D.n_run), dim3(64), sizeof(double) * 8 * P.T, s, P, D);      \
    else hipLaunchKernelGGL((k_tq_step<NN>), dim3(D.n_run), dim3(64), sizeof(double) * 8 * P.T, s, P, D);                  \
  }
  OH_TQ_DISPATCH(P.N, C)
#undef C
  return true;
}
// ---- receding horizon, resident on the device (oh_tq_rollout, round 5) ----------------------------------------------------------------------
// One thread per plant.  The reference's pattern (example/point_mass_mpc.py:156-175): parameters of the tick from the plant's state, seed = the
// previous solution, solve, the plant takes the plan's next state.  Reference layouts: x [B][4 N T] = [vec(Q); vec(dQ); vec(ddQ); vec(TAU)],
// p [B][2 N + 3 T] = [qc; dqc; vec(goal 3 x T)].
__global__ __launch_bounds__(64) void k_tq_tick_params(const int B, const int T, const int N, const int first_row, const int n_rows, const double* __restrict__ state,
                                                       const double* __restrict__ goal_table, double* __restrict__ p) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double* pb = p + (size_t)b * (2 * N + 3 * T);
  for (int i = 0; i < 2 * N; ++i) pb[i] = state[(size_t)b * 2 * N + i];
  const double* gt = goal_table + ((size_t)b * n_rows + first_row) * 3;
  for (int i = 0; i < 3 * T; ++i) pb[2 * N + i] = gt[i];
}
// seed of the next tick: the accelerations of the plan shifted by `advance` knots, the last one repeated (only the ddQ block of a seed is read:
// the states are rolled out from the plant's state, the torques follow from the dynamics rows)
__global__ __launch_bounds__(64) void k_tq_shift_seed(const int B, const int T, const int N, const int advance, const double* __restrict__ x_prev,
                                                      double* __restrict__ x_seed) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* u = x_prev + (size_t)b * 4 * N * T + 2 * N * T;
  double* us = x_seed + (size_t)b * 4 * N * T + 2 * N * T;
  for (int t = 0; t < T; ++t) {
    const int ts = t + advance < T ? t + advance : T - 1;
    for (int j = 0; j < N; ++j) us[N * t + j] = u[N * ts + j];
  }
}
// the plant follows the plan for `advance` knots (the plan's states ARE the Euler roll-out of its accelerations, and its torques those of the
// inverse dynamics at its states: tau_t = rnea(q_t, dq_t, ddq_t) to 1e-14); the torque applied at the tick is the one of knot 0
__global__ __launch_bounds__(64) void k_tq_advance(const int B, const int T, const int N, const int advance, const double* __restrict__ x, double* __restrict__ state_next,
                                                   double* __restrict__ tau0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* xb = x + (size_t)b * 4 * N * T;
  for (int j = 0; j < N; ++j) {
    state_next[(size_t)b * 2 * N + j] = xb[N * advance + j];
    state_next[(size_t)b * 2 * N + N + j] = xb[N * T + N * advance + j];
    if (tau0) tau0[(size_t)b * N + j] = xb[3 * N * T + j];
  }
}
void oh_launch_tq_tick_params(hipStream_t s, int B, int T, int N, int first_row, int n_rows, const double* state, const double* goal_table, double* p) {
  hipLaunchKernelGGL(k_tq_tick_params, dim3((B + 63) / 64), dim3(64), 0, s, B, T, N, first_row, n_rows, state, goal_table, p);
}
void oh_launch_tq_shift_seed(hipStream_t s, int B, int T, int N, int advance, const double* x_prev, double* x_seed) {
  hipLaunchKernelGGL(k_tq_shift_seed, dim3((B + 63) / 64), dim3(64), 0, s, B, T, N, advance, x_prev, x_seed);
}
void oh_launch_tq_advance(hipStream_t s, int B, int T, int N, int advance, const double* x, double* state_next, double* tau0) {
  hipLaunchKernelGGL(k_tq_advance, dim3((B + 63) / 64), dim3(64), 0, s, B, T, N, advance, x, state_next, tau0);
}
bool oh_launch_tq_finalize(hipStream_t s, const TqParams& P, const TqBuffers& D, double* x, double* f, double* kkt, int* iters, int* status, double* mult) {
#define C(NN) hipLaunchKernelGGL(k_tq_finalize<NN>, dim3((D.B + 63) / 64), dim3(64), 0, s, P, D, x, f, kkt, iters, status, mult)
  OH_TQ_DISPATCH(P.N, C)
#undef C
  return true;
}

namespace {
template <class K>
bool kernel_info(K kernel, int block, OhKernelInfo* out) {
  hipFuncAttributes a;
  if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(kernel)) != hipSuccess) return false;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, 0) != hipSuccess) nb = 0;
  *out = OhKernelInfo{a.numRegs, (int)a.localSizeBytes, (int)a.sharedSizeBytes, block, nb};
  return true;
}
}  // namespace
// "k_tq_eval", "k_tq_curv", "k_tq_step": the 7-joint arm's instantiations; with "_N" behind them (N = 2 .. 7) those of an N-joint chain
bool oh_kernel_info_torque(const char* name, OhKernelInfo* out) {
  std::string n(name);
  int N = 7;
  if (n.size() > 2 && n[n.size() - 2] == '_' && n.back() >= '0' && n.back() <= '9') {
    N = n.back() - '0';
    n.resize(n.size() - 2);
  }
#define C(NN)                                                            \
  {                                                                      \
    if (n == "k_tq_eval") return kernel_info(k_tq_eval3<NN>, 64, out);   \
    if (n == "k_tq_curv") return kernel_info(k_tq_curv<NN>, 64, out);    \
    if (n == "k_tq_step") return kernel_info(k_tq_step<NN>, 64, out);    \
  }
  OH_TQ_DISPATCH(N, C)
#undef C
  return false;
}
