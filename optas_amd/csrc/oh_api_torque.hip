// Host side of the torque-MPC family (OH_PROBLEM_TORQUE_MPC): creation, the interior-point launch loop, the closed-loop rollout.
// State: oh_handle::tq.
#include <cmath>

#include "oh_handle.h"

extern "C" int oh_create_torque(const oh_torque_desc* desc, oh_handle** out) {
  if (!desc || !out) return fail(OH_ERR_INVALID, "oh_create_torque: null argument");
  *out = nullptr;
  if (desc->ndof < 2 || desc->ndof > 7) return fail(OH_ERR_INVALID, "oh_create_torque: kernels are instantiated for ndof 2 .. 7");
  if (desc->T < 2 || desc->T > OH_MAX_T) return fail(OH_ERR_INVALID, "oh_create_torque: T must be in [2, OH_MAX_T]");
  if (!(desc->dt > 0.0) || !(desc->w_tau > 0.0) || !(desc->w_path >= 0.0) || !(desc->w_vel >= 0.0))
    return fail(OH_ERR_INVALID, "oh_create_torque: dt and w_tau must be positive, w_path and w_vel non-negative");
  for (int i = 0; i < desc->ndof; ++i)
    if (!(desc->tau_lo[i] < desc->tau_up[i])) return fail(OH_ERR_INVALID, "oh_create_torque: tau_lo must be below tau_up");
  if (desc->vel_limits)
    for (int i = 0; i < desc->ndof; ++i)
      if (!(desc->dq_lo[i] < desc->dq_up[i])) return fail(OH_ERR_INVALID, "oh_create_torque: dq_lo must be below dq_up");
  int rc = OH_OK;
  oh_handle* h = open_handle("oh_create_torque", OH_PROBLEM_TORQUE_MPC, desc->T, desc->ndof, OPEN_CHAIN | OPEN_FLAG, &rc);
  if (!h) return rc;
  oh_torque_desc& d = h->tq.desc;
  d = *desc;
  if (d.max_iter <= 0) d.max_iter = 300;
  if (!(d.tol > 0.0)) d.tol = 1e-6;
  if (!(d.tol_compl > 0.0)) d.tol_compl = 1e-8;
  if (!(d.mu_barrier0 > 0.0)) d.mu_barrier0 = 0.1;
  if (!(d.mu0 >= 0.0)) d.mu0 = 0.0;
  *out = h;
  return OH_OK;
}

int tq_solve_device(oh_handle* h, const Solve& a, const double mu_b0_warm) {
  if (!h->have_chain) return fail(OH_ERR_STATE, "oh_solve_device: call oh_set_constants first");
  if (!h->have_dyn) return fail(OH_ERR_STATE, "oh_solve_device: call oh_set_dynamics first");
  if (!solver_chain_ok(h->chain_host) || h->chain_host.has_lead)
    return fail(OH_ERR_INVALID, "oh_solve_device: the solver needs a chain that covers every model joint in order");
  TqState& tq = h->tq;
  const oh_torque_desc& d = tq.desc;
  const int B = a.B, N = d.ndof, T = d.T;
  if (h->dyn_host.ndof != N) return fail(OH_ERR_INVALID, "oh_solve_device: the inverse-dynamics tables must have ndof + 1 bodies");
  HIPCHK(hipSetDevice(h->device));
  TqParams& P = tq.P;
  P = TqParams{};
  P.T = T; P.N = N; P.max_iter = d.max_iter;
  P.dt = d.dt; P.w_path = d.w_path; P.w_vel = d.w_vel; P.w_tau = d.w_tau;
  P.tol = d.tol; P.tol_compl = d.tol_compl; P.mu_b0 = mu_b0_warm > 0.0 ? mu_b0_warm : d.mu_barrier0; P.mu0 = d.mu0;
  // interior point: relaxed barrier below theta mu_b; monotone barrier update of Waechter & Biegler (2006, eq. 7) -- IPOPT's constants except theta_mu (1.35 for 1.5: the hardest of 8192 instances needs 127 steps instead of 198) and, round 5, kappa_mu (0.4 for 0.2: tools/gpu_tq_param_sweep.py); exact
  // curvature of the Lagrangian once the reduced gradient is below curv_from (oracle/torque_ipm.py:solve_torque_ipm has the same defaults: OPT_TABLE's)
  P.theta = 0.01;
  P.stall_max = (int)optv(h, "tq_stall");
  P.curv_after = (int)optv(h, "tq_curv_after");
  P.tau_ftb = optv(h, "tq_ftb");
  P.theta_mu = optv(h, "tq_theta_mu");
  P.kappa_mu = optv(h, "tq_kappa_mu");
  P.curv_from = optv(h, "tq_curv_from");  // 0: Gauss-Newton blocks throughout (A/B)
  P.curv_late = optv(h, "tq_curv_late");
  P.kappa_eps = optv(h, "tq_kappa_eps");
  // (a warm-started tick of oh_tq_rollout starts next to its optimum: there the damping comes down faster)
  P.mu_dec = mu_b0_warm > 0.0 ? optv(h, "tq_mu_dec_warm") : optv(h, "tq_mu_dec");
  P.ls_curv = (int)optv(h, "tq_ls_curv");
  P.curv_lag = (int)optv(h, "tq_curv_lag");
  P.max_back = (int)optv(h, "tq_max_back");
  P.vel = d.vel_limits ? 1 : 0;
  // d tau / dz in closed form needs the tables to describe a rigid-body chain: unit joint axes that the joint-origin rotation leaves in place (then
  // the angular velocity the reference adds, iRp @ axis, is the axis its rotation turns about; models.py:1821-1823).  Otherwise: dual numbers.
  P.jac_closed_form = 1;
  for (int i = 0; i < N; ++i) {
    const double* a = h->dyn_host.axis[i];
    const double* R = h->dyn_host.R0[i];
    double dev = fabs(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] - 1.0);
    for (int k = 0; k < 3; ++k) dev = fmax(dev, fabs(R[k] * a[0] + R[3 + k] * a[1] + R[6 + k] * a[2] - a[k]));
    if (!(dev <= 1e-12)) P.jac_closed_form = 0;
  }
  if (optv(h, "tq_jac_dual") != 0.0) P.jac_closed_form = 0;  // the dual-number path whatever the tables (A/B, tests)
  for (int i = 0; i < N; ++i) {
    P.tau_lo[i] = d.tau_lo[i];
    P.tau_up[i] = d.tau_up[i];
    P.dq_lo[i] = d.dq_lo[i];
    P.dq_up[i] = d.dq_up[i];
  }
  P.nx = (int)shape_of(h).nx;
  P.np = (int)shape_of(h).npar;
  TqBuffers& D = tq.D;
  const size_t BT = (size_t)B * T;
  if (BT * TQ_HC > tq.hc.cap) {  // the pool, the multipliers and the curvature terms grow together (tq.hc last: its capacity is the batch all three hold)
    HIPCHK(hipStreamSynchronize(h->stream));
    tq.pool.release();
    tq.mult.release();
    tq.hc.release();
    Carver measure(nullptr, Carver::Packed);
    layout_tq(measure, D, B, T);
    HIPCHK(tq.pool.reserve(measure.bytes()));
    HIPCHK(tq.mult.reserve(BT * 4 * N));  // effort rows, and room for the velocity rows
    HIPCHK(tq.hc.reserve(BT * TQ_HC));
    HIPCHK(hipMemsetAsync(tq.hc, 0, sizeof(double) * BT * TQ_HC, h->stream));  // entries the adjoint never writes stay zero
  }
  {
    // D.B is the live batch: the strides of the [slot][B][T] arrays follow it, inside a pool that holds the largest batch so far
    Carver carve(tq.pool.p, Carver::Packed);
    layout_tq(carve, D, B, T);
    D.B = B;
    D.chain = h->d_chain;
    D.dyn = h->d_dyn;
    D.hc = tq.hc;
    D.n_run = B;
  }
  hipStream_t s = h->stream;
  HIPCHK(hipEventRecord(h->ev0, s));
  if (!oh_launch_tq_setup(s, P, D, a.x0, a.p)) return fail(OH_ERR_INVALID, "oh_solve_device: unsupported ndof");
  // iteration k: evaluate the pending trial of every running instance, then ratio test / Riccati sweep / next trial.  The host only looks at
  // the running count every tq_check iterations (instances that finished in between cost nothing: their lanes exit at once).
  int launched = 0;
  double work = 0.0;
  int running = B;
  const int cap = P.max_iter + 2;
  // oh_set_profiling(1): one event before the evaluation pair (k_tq_eval3 + k_tq_curv), one after it, one after k_tq_step, every iteration -- the
  // per-kernel device times behind the family's roofline object (tools/bench_configs.py); such a solve runs on one stream
  const bool prof = h->profiling;
  size_t ne = 0;
  if (prof) {
    const size_t need = 3 * (size_t)cap + 4;
    while (h->prof_events.size() < need) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      h->prof_events.push_back(e);
    }
  }
  while (launched < cap) {
    if (prof) HIPCHK(hipEventRecord(h->prof_events[ne++], s));
    oh_launch_tq_eval(s, P, D);  // also resets the running count
    if (prof) HIPCHK(hipEventRecord(h->prof_events[ne++], s));
    oh_launch_tq_step(s, P, D);
    if (prof) HIPCHK(hipEventRecord(h->prof_events[ne++], s));
    ++launched;
    work += running;
    if (launched % h->sch.tq_check == 0 || launched == cap) {
      HIPCHK(hipMemcpyAsync(h->h_flag, D.n_running, sizeof(int), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      running = *h->h_flag;
      if (running == 0) break;
      const double rebuild = optv(h, "tq_rebuild");
      if (running <= rebuild * D.n_run) {  // rebuild the list of running instances: grids shrink with the batch
        HIPCHK(hipMemsetAsync(D.n_list, 0, sizeof(int), s));
        oh_launch_tq_list(s, D);
        D.n_run = running;
      }
    }
  }
  oh_launch_tq_finalize(s, P, D, a.x, a.f, a.kkt, a.iters, a.status, tq.mult);
  if (const int rc = finish_solve(h, launched)) return rc;
  if (prof) {
    for (size_t i = 0; i + 3 <= ne; i += 3) {
      float a = 0.f, b2 = 0.f;
      hipEventElapsedTime(&a, h->prof_events[i], h->prof_events[i + 1]);
      hipEventElapsedTime(&b2, h->prof_events[i + 1], h->prof_events[i + 2]);
      h->timing[0] += a;
      h->timing[2] += b2;
    }
    h->timing[1] = h->timing[3] = launched;
  }
  h->timing[6] = work;
  return OH_OK;
}

extern "C" int oh_tq_rollout(oh_handle* h, int B, int n_ticks, int advance, double mu_warm, const double* state0, const double* goal_table, double* states,
                             double* tau0, double* f, int* iters, int* status) {
  if (!h || !state0 || !goal_table) return fail(OH_ERR_INVALID, "oh_tq_rollout: null argument");
  if (h->desc.kind != OH_PROBLEM_TORQUE_MPC) return fail(OH_ERR_STATE, "oh_tq_rollout: handle is not a torque-MPC problem");
  const int T = h->tq.desc.T, N = h->tq.desc.ndof;
  if (B < 1 || n_ticks < 1 || advance < 1 || advance >= T) return fail(OH_ERR_INVALID, "oh_tq_rollout: need B >= 1, n_ticks >= 1, 1 <= advance < T");
  if (!(mu_warm > 0.0)) mu_warm = 1e-6;
  HIPCHK(hipSetDevice(h->device));
  h->last = LastSolve{};
  const size_t nB = (size_t)B, n_rows = (size_t)n_ticks * advance + T;
  const size_t nx = shape_of(h).nx, np_ = shape_of(h).npar;
  const size_t b_states = sizeof(double) * 2 * N * nB * (n_ticks + 1), b_goal = sizeof(double) * 3 * n_rows * nB, b_x = sizeof(double) * nx * nB,
               b_tau = sizeof(double) * N * nB * n_ticks, b_f = sizeof(double) * nB * n_ticks, b_i = sizeof(int) * nB * n_ticks;
  double *d_states, *d_goal, *d_p, *d_xa, *d_xb, *d_tau, *d_f;
  int *d_it, *d_st;
  int rc = stage_carve(h, [&](Carver c) {
    d_states = c.take<double>(2 * N * nB * (n_ticks + 1));
    d_goal = c.take<double>(3 * n_rows * nB);
    d_p = c.take<double>(np_ * nB);
    d_xa = c.take<double>(nx * nB);
    d_xb = c.take<double>(nx * nB);
    d_tau = c.take<double>(N * nB * n_ticks);
    d_f = c.take<double>(nB * n_ticks);
    d_it = c.take<int>(nB * n_ticks);
    d_st = c.take<int>(nB * n_ticks);
    return c.bytes();
  });
  if (rc) return rc;
  hipStream_t s = h->stream;
  HIPCHK(hipMemcpyAsync(d_states, state0, sizeof(double) * 2 * N * (size_t)B, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_goal, goal_table, b_goal, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(d_xa, 0, b_x, s));  // first tick: zero accelerations (the cold solve of oh_solve from a constant-configuration seed)
  double ms_total = 0.0, launched = 0.0, work = 0.0;
  for (int k = 0; k < n_ticks; ++k) {
    double* st_k = d_states + 2 * (size_t)N * B * k;
    oh_launch_tq_tick_params(s, B, T, N, k * advance, (int)n_rows, st_k, d_goal, d_p);
    double* x_seed = d_xa;  // the seed of this tick; the solution lands in d_xb and is shifted back into d_xa for the next one
    double* x_sol = d_xb;
    rc = tq_solve_device(h, Solve{B, x_seed, d_p, x_sol, d_f + (size_t)B * k, nullptr, d_it + (size_t)B * k, d_st + (size_t)B * k}, k > 0 ? mu_warm : 0.0);
    if (rc) return rc;
    ms_total += h->timing[4];
    launched += h->timing[5];
    work += h->timing[6];
    oh_launch_tq_advance(s, B, T, N, advance, x_sol, st_k + 2 * (size_t)N * B, tau0 ? d_tau + (size_t)N * B * k : nullptr);
    oh_launch_tq_shift_seed(s, B, T, N, advance, x_sol, x_seed);
  }
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  reset_counters(h);
  h->timing[4] = ms_total;  // device time of the solves (HIP events around each)
  h->timing[5] = launched;
  h->timing[6] = work;
  if (states) HIPCHK(hipMemcpy(states, d_states, b_states, hipMemcpyDeviceToHost));
  if (tau0) HIPCHK(hipMemcpy(tau0, d_tau, b_tau, hipMemcpyDeviceToHost));
  if (f) HIPCHK(hipMemcpy(f, d_f, b_f, hipMemcpyDeviceToHost));
  if (iters) HIPCHK(hipMemcpy(iters, d_it, b_i, hipMemcpyDeviceToHost));
  if (status) HIPCHK(hipMemcpy(status, d_st, b_i, hipMemcpyDeviceToHost));
  h->last = LastSolve{B, {{h, B}}, false};
  return OH_OK;
}
