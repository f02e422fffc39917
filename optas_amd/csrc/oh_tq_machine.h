// The scalar state machine of the torque-MPC interior point: what k_tq_step (oh_torque.hip) decides between its lane-parallel steps, one function per
// step, to be read side by side with oracle/torque_ipm.py:solve_torque_ipm.  Functions of the instance's registers (TqInst), the parameters and the
// few values the wavefront has reduced: no lane index, no memory access.  Needs TqParams, TqInst (oh_kernels.h), OH_DEV and <cmath> only.
// (The verdict and the plan come back through references: returned by value, the small structs of flags travel packed into one integer and
//  k_tq_step<7> with velocity rows needs 169 registers instead of 167 -- two wavefronts per SIMD instead of three.)
#pragma once
#include <cmath>

struct TqTrial { double f, bsum, nrel, viol; };  // sums over the stage records of the trial point
struct TqVerdict { bool accept, new_gains; };    // new_gains false: the pending step is retried shorter on the gains of the last sweep
struct TqBarrier { double mu_min, next, up; };   // the barrier parameter's floor, its successor (Waechter & Biegler 2006, eq. 7), the watchdog's way back up
struct TqStat { double cur, next, up; };         // reduced gradient of the accepted point under mu_b, under its successor and under the watchdog's
struct TqPlan {
  int status;
  bool do_gains, do_roll;
  bool reeval;  // the next "trial" is this point itself under a lower barrier parameter (round 6)
  bool curv;    // the next evaluation takes the exact curvature
};

// More damping, same point: a rejected full step, or a stage block of the exact Hessian that left Q_uu indefinite (torque_ipm.py:189-190, 254-255).
OH_DEV void tq_raise_damping(TqInst& S) {
  S.mu = fmax(S.mu * S.nun, 0.1);
  S.nun *= 2.0;
}

// Step 1 (torque_ipm.py:162-197): merit of the trial  f + mu_b B,  ratio test against the decrease the damped model predicted for the scaled step,
// Levenberg-Marquardt update; an accepted trial becomes the instance's point.
OH_DEV void tq_ratio_test(TqInst& S, const TqParams& P, const TqTrial& tr, TqVerdict& v) {
  const double f_t = tr.f + S.mub * tr.bsum;
  v = TqVerdict{false, true};
  if (S.first != 0) {
    v.accept = true;
  } else if (!isfinite(f_t)) {  // the trial left the domain of the arithmetic: same gains, a tenth of the feed-forward (the model is not to blame)
    v.accept = false;
    v.new_gains = false;
    S.alpha *= 0.1;
    S.rejected += 1;
  } else {
    const double pred = (S.alpha - 0.5 * S.alpha * S.alpha) * S.qk + 0.5 * S.alpha * S.alpha * S.mu * S.ndx;
    const double ratio = (S.f_cur - f_t) / fmax(pred, 1e-300);
    v.accept = ratio > 1e-4 || (pred <= 1e-15 * fabs(S.f_cur) && f_t <= S.f_cur + 1e-14 * fabs(S.f_cur));
    if (v.accept) {
      const double w = 2.0 * ratio - 1.0;
      S.mu *= ratio > 0.9 ? P.mu_dec : fmax(1.0 / 3.0, 1.0 - w * w * w);
      if (S.mu < 1e-7) S.mu = 0.0;
      S.nun = 4.0;
    } else if ((S.alpha < 1.0 || (P.ls_curv && S.curv != 0)) && S.n_back < P.max_back) {
      // a step the boundary rule had shortened already: the rows near their bounds are to blame (the logarithm is far from its quadratic model
      // there), not the model of the states -- a quarter of the feed-forward, same gains, same damping.  Round 5: likewise a full Newton step
      // (exact curvature) that was rejected -- measured on stragglers (tools/gpu_tq_param_sweep.py, HISTORY): the full step gives up more barrier
      // than it gains (a slack drops to a third), 0.3 of it follows the model to 8 %, and the damping, which acts on the states, does not shorten a
      // step that lives in the accelerations: five rejections and six careful steps afterwards, or one quartering
      v.new_gains = false;
      S.alpha *= 0.25;
      S.n_back += 1;
      S.rejected += 1;
    } else {
      tq_raise_damping(S);
      S.rejected += 1;
    }
  }
  if (v.accept || v.new_gains) S.n_back = 0;
  if (v.accept) {
    S.cur = 1 - S.cur;
    S.f_cur = f_t; S.f_true = tr.f; S.bsum = tr.bsum;
    S.nrel = (int)tr.nrel; S.viol = tr.viol;
  }
}

// The barrier parameters step 2 measures the reduced gradient under (torque_ipm.py:212, 244).
OH_DEV TqBarrier tq_barrier_candidates(const double mub, const TqParams& P) {
  TqBarrier nb;
  nb.mu_min = 0.1 * P.tol_compl;
  nb.next = fmax(nb.mu_min, fmin(P.kappa_mu * mub, pow(mub, P.theta_mu)));
  nb.up = fmin(P.mu_b0, 100.0 * mub);
  return nb;
}

// Step 3 (torque_ipm.py:203-249): convergence, barrier update, watchdog, ACCEPTABLE / INFEASIBLE, curvature of the next evaluation.  The stage gradient is
// g_f + mu_b g_b  and the merit  f + mu_b B:  a new mu_b needs no re-evaluation, its reduced gradient is the one step 2 measured beside the current one.
OH_DEV void tq_decide(TqInst& S, const TqParams& P, const TqVerdict& v, const TqStat& st, const TqBarrier& nb, TqPlan& pl) {
  pl = TqPlan{-1, false, false, false, S.curv != 0};  // (curv: the pending trial was evaluated with exact curvature -- 1 computed, 2 the stored term)
  S.stat = st.cur;
  if (!isfinite(S.f_cur)) {
    pl.status = OH_STATUS_NUMERICAL;
  } else if (S.stat <= P.tol && S.mub <= P.tol_compl && S.nrel == 0) {
    pl.status = OH_STATUS_CONVERGED;
  } else if (S.iters >= P.max_iter) {
    pl.status = OH_STATUS_MAX_ITER;
  } else {
    S.iters += 1;
    pl.do_roll = true;
    if (v.new_gains) {
      pl.do_gains = true;
      if (v.accept && S.stat <= P.kappa_eps * S.mub && S.nrel == 0 && S.mub > nb.mu_min) {
        S.mub = nb.next;
        S.f_cur = S.f_true + S.mub * S.bsum;
        S.stat = st.next;
        S.n_barrier += 1;
        S.stall = 0;
      } else if (v.accept && S.stat <= P.kappa_eps * S.mub && S.nrel > 0 && S.mub > nb.mu_min) {
        // Round 6: stationary for this mu_b with rows inside the relaxed zone (slack below theta mu_b: a row whose multiplier exceeds 1 / theta -- a velocity limit
        // the tracking cost pushes hard against).  Merit and gradient are not affine in mu_b there, so the update above does not apply; without one the instance sat at
        // this point until the cap (null steps "rejected" at rounding level, the damping doubling).  The barrier parameter is lowered all the same and the point itself
        // evaluated again under it: a null step (alpha = 0 on the gains of the last sweep), accepted as it is (D.first).  oracle/torque_ipm.py alike.
        S.mub = nb.next;
        S.n_barrier += 1;
        S.stall = 0;
        pl.reeval = true;
        pl.do_gains = false;
        S.alpha = 0.0;
      } else if (v.accept && S.stat <= 10.0 * P.tol && S.nrel > 0 && S.mub <= nb.mu_min && S.viol > P.tol_compl) {
        // ... and at the floor of the barrier parameter a stationary point that still violates a row has no feasible neighbour (the relaxed barrier is a penalty of
        // weight 1 / (theta^2 mu_b) by now): IPOPT's Infeasible_Problem_Detected, did_solve() False (solver.py:133-134, 407-412)
        pl.status = OH_STATUS_INFEASIBLE;
        S.iters -= 1;
        pl.do_roll = false;
        pl.do_gains = false;
      } else {
        S.stall += 1;
        if (S.stall >= P.stall_max && S.nrel == 0 && S.mub <= nb.mu_min && S.stat <= 10.0 * P.tol) {
          // "acceptable level" (IPOPT's acceptable_tol / acceptable_iter in spirit): stall_max steps at the floor of the barrier parameter without
          // meeting tol while within ten times of it -- the arithmetic floor of the reduced gradient: an active row with slack s carries mu_b / s,
          // and s = up - tau inherits the ~1e-14 of the recursion, so at s ~ 1e-8 the multiplier is good to ~1e-6 relative and the reduced gradient to
          // ~1e-6 absolute.  Without this such an instance (1 of 8192 in one of nine batches) fed the watchdog below and ended NUMERICAL at the optimum.
          pl.status = OH_STATUS_ACCEPTABLE;
          S.iters -= 1;
          pl.do_roll = false;
          pl.do_gains = false;
        } else if (S.stall >= P.stall_max && S.nrel == 0 && v.accept) {
          // watchdog: stall_max steps without reaching the barrier test -- the iterate sits far from the central path of this mu_b (slacks of the active
          // rows collapse and recover in turn).  Back to a larger barrier parameter: the path is regained there and followed down again.
          S.mub = nb.up;
          S.f_cur = S.f_true + S.mub * S.bsum;
          S.stat = st.up;
          S.stall = 0;
        }
      }
      if (!pl.reeval) pl.curv = S.stat <= P.curv_from || (S.n_barrier >= P.curv_after && S.stat <= P.curv_late);
    }
  }
}

// After step 6 (torque_ipm.py:192-193, and evalp's store): the next evaluation takes the curvature term afresh, or the stored one while it is younger
// than curv_lag evaluations.
OH_DEV void tq_next_curvature(TqInst& S, const TqParams& P, const bool accept, const bool curv) {
  int age = S.curv_age, mode = 0;
  if (!accept && S.curv == 1) age = -1;  // a term computed at a point that was refused (possibly outside the domain of the arithmetic) is not kept
  if (curv) {
    if (age >= 0 && age < P.curv_lag) { mode = 2; age += 1; }
    else { mode = 1; age = 0; }
  } else age = -1;
  S.curv = mode;
  S.curv_age = age;
}
