// Host side of the point-mass MPC family (OH_PROBLEM_POINT_MASS_MPC): creation, the pool, the solve, the closed-loop rollout.
// State: oh_handle::pm.
#include "oh_handle.h"

extern "C" int oh_create_pointmass(const oh_pointmass_desc* desc, oh_handle** out) {
  if (!desc || !out) return fail(OH_ERR_INVALID, "oh_create_pointmass: null argument");
  *out = nullptr;
  if (desc->T < 2 || desc->T > OH_MAX_T) return fail(OH_ERR_INVALID, "oh_create_pointmass: T must be in [2, OH_MAX_T]");
  if (!(desc->dt > 0.0) || !(desc->w_acc > 0.0) || !(desc->ylim > 0.0) || !(desc->vlim > 0.0) || !(desc->safe >= 0.0) || !(desc->w_vel >= 0.0) ||
      (desc->fix_final_velocity && desc->T < 3))
    return fail(OH_ERR_INVALID, "oh_create_pointmass: dt, w_acc, ylim, vlim must be positive and safe non-negative");
  int rc = OH_OK;
  oh_handle* h = open_handle("oh_create_pointmass", OH_PROBLEM_POINT_MASS_MPC, desc->T, 2, 0, &rc);
  if (!h) return rc;
  oh_pointmass_desc& d = h->pm.desc;
  d = *desc;
  if (d.max_iter <= 0) d.max_iter = 100;
  if (!(d.tol > 0.0)) d.tol = 1e-8;
  *out = h;
  return OH_OK;
}

// the pool for B instances (grow-only) and the kernels' parameters
static int pm_prepare(oh_handle* h, int B) {
  HIPCHK(hipSetDevice(h->device));
  PmState& pm = h->pm;
  const oh_pointmass_desc& d = pm.desc;
  const int T = d.T;
  const int Bp = (B + 63) / 64 * 64;  // (padding the row stride like the trajectory families do was measured: no effect, the solve is latency bound)
  if (Bp > pm.cap_B || !pm.pool) {
    pm.pool.release();
    Carver measure(nullptr, Carver::Packed);
    layout_pm(measure, pm.D, T, Bp);
    const hipError_t e = pm.pool.reserve(measure.bytes());
    if (e != hipSuccess) return fail(OH_ERR_HIP, std::string("device pool allocation failed: ") + hipGetErrorString(e));
    pm.cap_B = Bp;
    pm.D.Bp = Bp;
    Carver carve(pm.pool.p, Carver::Packed);
    layout_pm(carve, pm.D, T, Bp);
  }
  pm.D.B = B;
  pm.P = PmParams{T, d.dt, d.w_acc, d.ylim, d.vlim, d.safe * d.safe, d.tol, d.max_iter, d.track_final_only ? 1 : 0, d.w_vel, d.fix_final_velocity ? 1 : 0};
  return OH_OK;
}
// one solve on the prepared handle: a solve of its own, or a tick of the rollout
static void pm_launch(oh_handle* h, const Solve& a) {
  oh_launch_pm_solve(h->stream, h->pm.P, h->pm.D, a.x0, a.p, a.x, a.f, a.kkt, a.iters, a.status, (int)optv(h, "pm_wave_max"));
}

int pm_solve_device(oh_handle* h, const Solve& a) {
  if (const int rc = pm_prepare(h, a.B)) return rc;
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  pm_launch(h, a);
  return finish_solve(h, 1);
}

extern "C" int oh_pm_rollout(oh_handle* h, int B, int n_ticks, int advance, double ramp, const double* state0, const double* obs_table,
                             double* states, double* f, int* iters, int* status) {
  if (!h || !state0 || !obs_table) return fail(OH_ERR_INVALID, "oh_pm_rollout: null argument");
  if (h->desc.kind != OH_PROBLEM_POINT_MASS_MPC) return fail(OH_ERR_STATE, "oh_pm_rollout: handle is not a point-mass MPC problem");
  const int T = h->pm.desc.T;
  if (B < 1 || n_ticks < 1 || advance < 1 || advance >= T) return fail(OH_ERR_INVALID, "oh_pm_rollout: need B >= 1, n_ticks >= 1, 1 <= advance < T");
  h->last = LastSolve{};
  int rc = pm_prepare(h, B);
  if (rc) return rc;
  const size_t nB = (size_t)B, n_obs = (size_t)n_ticks * advance + T;
  const size_t b_states = sizeof(double) * 4 * nB * (n_ticks + 1), b_obs = sizeof(double) * 2 * n_obs, b_x = sizeof(double) * 4 * (size_t)T * nB;
  const size_t b_f = sizeof(double) * nB * n_ticks, b_i = sizeof(int) * nB * n_ticks;
  double *d_states, *d_obs, *d_p, *d_xa, *d_xb, *d_f;
  int *d_it, *d_st;
  rc = stage_carve(h, [&](Carver c) {
    d_states = c.take<double>(4 * nB * (n_ticks + 1));
    d_obs = c.take<double>(2 * n_obs);
    d_p = c.take<double>((4 + 4 * (size_t)T) * nB);
    d_xa = c.take<double>(4 * (size_t)T * nB);
    d_xb = c.take<double>(4 * (size_t)T * nB);
    d_f = c.take<double>(nB * n_ticks);
    d_it = c.take<int>(nB * n_ticks);
    d_st = c.take<int>(nB * n_ticks);
    return c.bytes();
  });
  if (rc) return rc;
  hipStream_t s = h->stream;
  HIPCHK(hipMemcpyAsync(d_states, state0, sizeof(double) * 4 * (size_t)B, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_obs, obs_table, b_obs, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(d_xa, 0, b_x, s));  // first tick: zero seed (solver.py:76)
  HIPCHK(hipEventRecord(h->ev0, s));
  for (int k = 0; k < n_ticks; ++k) {
    double* st_k = d_states + 4 * (size_t)B * k;
    oh_launch_pm_tick_params(s, B, T, k, advance, ramp, st_k, d_obs, d_p);
    double* x_seed = (k & 1) ? d_xb : d_xa;  // previous solution = warm start of this tick
    double* x_sol = (k & 1) ? d_xa : d_xb;
    pm_launch(h, Solve{B, x_seed, d_p, x_sol, d_f + (size_t)B * k, nullptr, d_it + (size_t)B * k, d_st + (size_t)B * k});
    oh_launch_pm_advance(s, B, T, advance, x_sol, st_k + 4 * (size_t)B);
  }
  if ((rc = finish_solve(h, n_ticks))) return rc;
  if (states) HIPCHK(hipMemcpy(states, d_states, b_states, hipMemcpyDeviceToHost));
  if (f) HIPCHK(hipMemcpy(f, d_f, b_f, hipMemcpyDeviceToHost));
  if (iters) HIPCHK(hipMemcpy(iters, d_it, b_i, hipMemcpyDeviceToHost));
  if (status) HIPCHK(hipMemcpy(status, d_st, b_i, hipMemcpyDeviceToHost));
  h->last = LastSolve{B, {{h, B}}, false};
  return OH_OK;
}
