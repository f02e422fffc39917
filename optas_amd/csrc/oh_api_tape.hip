// Host side of the tape family (OH_PROBLEM_TAPE; the tape of a QP handle): validation, evaluator choice, the tape's device arrays,
// probes and the solve.  State: oh_handle::tape.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "oh_handle.h"

int tape_validate(const oh_tape_desc* d, const char* who) {
  const std::string w(who);
  if (d->nx < 1 || d->nx > OH_TAPE_MAX_N || d->np < 0 || d->len < 1 || d->len > OH_TAPE_MAX_LEN || d->n_ineq < 0 || d->n_eq < 0 || !d->op || !d->a ||
      !d->b || !d->c || (d->n_ineq + d->n_eq > 0 && !d->rows) || d->out_cost < 0 || d->out_cost >= d->len)
    return fail(OH_ERR_INVALID, (w + ": bad sizes or null arrays").c_str());
  for (int i = 0; i < d->len; ++i) {
    const int o = d->op[i], n = tape_op_arity(o);  // (b of a unary instruction is not looked at, here or by any evaluator)
    if (o < 0 || o >= OP_COUNT || (o == OP_X && (d->a[i] < 0 || d->a[i] >= d->nx)) || (o == OP_P && (d->a[i] < 0 || d->a[i] >= d->np)) ||
        (n >= 1 && (d->a[i] < 0 || d->a[i] >= i)) || (n == 2 && (d->b[i] < 0 || d->b[i] >= i)))
      return fail(OH_ERR_INVALID, (w + ": malformed instruction (operands must be earlier registers / valid indices)").c_str());
  }
  for (int i = 0; i < d->n_ineq + d->n_eq; ++i)
    if (d->rows[i] < 0 || d->rows[i] >= d->len) return fail(OH_ERR_INVALID, (w + ": row register out of range").c_str());
  return OH_OK;
}

TapeParams tape_params(const oh_tape_desc* d, const int lbfgs_opt) {
  // dense inverse-Hessian BFGS up to 48 variables (n^2 doubles per instance), the limited-memory form with 12 pairs beyond (option tape_lbfgs overrides:
  // 0 forces the dense matrix, m > 0 the m-pair form at any size)
  int lb = d->nx > 48 ? 12 : 0;
  if (lbfgs_opt >= 0) lb = lbfgs_opt > 64 ? 64 : lbfgs_opt;
  return TapeParams{d->len, d->nx, d->np, d->n_ineq, d->n_eq, d->out_cost, d->max_iter > 0 ? d->max_iter : 2000, d->tol > 0.0 ? d->tol : 1e-6,
                    d->tol_feas > 0.0 ? d->tol_feas : 1e-9, d->rho0 > 0.0 ? d->rho0 : 10.0, lb, nullptr};
}

extern "C" int oh_tape_compile(const oh_tape_desc* d, size_t* code_bytes, char* source, size_t source_cap, size_t* source_len) {
  if (!d) return fail(OH_ERR_INVALID, "oh_tape_compile: null argument");
  if (const int rc = tape_validate(d, "oh_tape_compile")) return rc;
  const std::string src = oh_tape_jit_source(tape_params(d), d->op, d->a, d->b, d->c, d->rows);
  if (source_len) *source_len = src.size();
  if (source && source_cap > 0) {
    const size_t k = src.size() < source_cap - 1 ? src.size() : source_cap - 1;
    memcpy(source, src.data(), k);
    source[k] = 0;
  }
  std::vector<char> code;
  std::string err;
  if (oh_tape_jit_compile(src, &code, &err)) return fail(OH_ERR_HIP, ("oh_tape_compile: " + err).c_str());
  if (code_bytes) *code_bytes = code.size();
  return OH_OK;
}

// (Re)build the evaluator of an OH_PROBLEM_TAPE handle from its host copy of the tape and its options: the wavefront-per-instance schedule where it
// applies (tape_wave != 0, limited-memory regime, LDS fit), otherwise generated code (desc.jit) or the interpreter.  With tape_newton != 0 the solves run
// k_tape_solve_newton on the interpreter: neither the schedule nor generated code is built for an evaluator that will not run -- unless tape_newton_wave != 0
// asks for the schedule too, under the same rules, for k_tape_wave_newton (generated code is never built for a Newton-CG handle).
int tape_configure(oh_handle* h) {
  TapeState& tp = h->tape;
  oh_tape_desc d = tp.desc;
  d.op = tp.h_op.data(); d.a = tp.h_a.data(); d.b = tp.h_b.data(); d.c = tp.h_c.data(); d.rows = tp.h_rows.empty() ? nullptr : tp.h_rows.data();
  tp.P = tape_params(&d, (int)optv(h, "tape_lbfgs"));
  tp.P.h0 = tp.h0;  // (a metric handed over before an option rebuilt the evaluator stays)
  oh_tape_wave_release(&tp.wave);
  tp.wave = TapeWave{};
  tp.work.release();  // the work arrays were sized for the other evaluator
  tp.mult.release();
  const bool newton = optv(h, "tape_newton") != 0.0;
  if (newton && optv(h, "tape_newton_wave") == 0.0) return OH_OK;
  int lds_limit = 0;
  if (optv(h, "tape_wave") != 0.0 && hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device) == hipSuccess) {
    std::string err;
    if (oh_tape_wave_build(tp.P, d.op, d.a, d.b, d.c, d.rows, (size_t)lds_limit, (int)optv(h, "tape_wave_nt"), (int)optv(h, "tape_wave_regs"),
                           (int)optv(h, "tape_wave_hist"), &tp.wave, &err))
      return fail(OH_ERR_HIP, ("oh_create_tape: " + err).c_str());
  }
  if (d.jit && !newton && !tp.wave.ready && !tp.jit.fn) {
    std::vector<char> code;
    std::string err;
    const std::string src = oh_tape_jit_source(tp.P, d.op, d.a, d.b, d.c, d.rows);
    bool ok = !oh_tape_jit_compile(src, &code, &err) && !oh_tape_jit_load(code, &tp.jit, &err);
    if (!ok && !code.empty()) {  // an object that compiled (or came from the disk cache) and does not load: drop it, recompile once (as oh_jit_figure8 does)
      oh_tape_jit_forget(src);
      code.clear();
      ok = !oh_tape_jit_compile(src, &code, &err) && !oh_tape_jit_load(code, &tp.jit, &err);
    }
    if (!ok) return fail(OH_ERR_HIP, ("oh_create_tape: " + err).c_str());
  }
  return OH_OK;
}

// the five device arrays of a tape (op_override: the opcodes to upload in place of d->op)
int upload_tape(oh_handle* h, const oh_tape_desc* d, const int* op_override) {
  TapeState& tp = h->tape;
  const size_t len = (size_t)d->len, nrow = (size_t)(d->n_ineq + d->n_eq);
  for (DevBuf<int>* b : {&tp.op, &tp.a, &tp.b, &tp.rows}) b->release();  // (sized for this tape, not grown from the last one's)
  tp.c.release();
  HIPCHK(tp.op.reserve(len));
  HIPCHK(tp.a.reserve(len));
  HIPCHK(tp.b.reserve(len));
  HIPCHK(tp.c.reserve(len));
  HIPCHK(tp.rows.reserve(nrow + 1));
  HIPCHK(hipMemcpy(tp.op, op_override ? op_override : d->op, sizeof(int) * len, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(tp.a, d->a, sizeof(int) * len, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(tp.b, d->b, sizeof(int) * len, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(tp.c, d->c, sizeof(double) * len, hipMemcpyHostToDevice));
  if (nrow > 0) HIPCHK(hipMemcpy(tp.rows, d->rows, sizeof(int) * nrow, hipMemcpyHostToDevice));
  return OH_OK;
}

extern "C" int oh_create_tape(const oh_tape_desc* d, oh_handle** out) {
  if (!d || !out) return fail(OH_ERR_INVALID, "oh_create_tape: null argument");
  *out = nullptr;
  if (const int rc = tape_validate(d, "oh_create_tape")) return rc;
  int rc = OH_OK;
  oh_handle* h = open_handle("oh_create_tape", OH_PROBLEM_TAPE, 1, d->nx, 0, &rc);
  if (!h) return rc;
  TapeState& tp = h->tape;
  // the tape stays with the handle: the evaluator is rebuilt when an option that shapes it changes
  tp.h_op.assign(d->op, d->op + d->len);
  tp.h_a.assign(d->a, d->a + d->len);
  tp.h_b.assign(d->b, d->b + d->len);
  tp.h_c.assign(d->c, d->c + d->len);
  tp.h_rows.assign(d->rows ? d->rows : d->op, (d->rows ? d->rows : d->op) + (d->rows ? d->n_ineq + d->n_eq : 0));
  tp.desc = *d;
  if (d->no_wave && !h->opt.count("tape_wave")) h->opt["tape_wave"] = 0.0;
  if (d->lbfgs != 0 && !h->opt.count("tape_lbfgs")) h->opt["tape_lbfgs"] = d->lbfgs > 0 ? (double)d->lbfgs : 0.0;
  if ((rc = tape_configure(h))) {
    delete h;  // (releases the wavefront schedule / the generated module as well)
    return rc;
  }
  // the interpreter's copy of the opcodes carries OP_DEAD on every instruction that neither the cost nor a row depends on (oh_tape_ops.h)
  std::vector<int> op_dev(d->op, d->op + d->len);
  const std::vector<char> live = tape_live(d->len, d->op, d->a, d->b, d->rows, d->n_ineq + d->n_eq, d->out_cost);
  for (int i = 0; i < d->len; ++i)
    if (!live[i]) op_dev[i] |= OP_DEAD;
  if ((rc = upload_tape(h, d, op_dev.data()))) {
    delete h;
    return rc;
  }
  *out = h;
  return OH_OK;
}

extern "C" int oh_tape_probe(oh_handle* h, int B, const double* x, const double* p, int n_regs, const int* regs, double* val, const double* seeds, double* adj,
                             double* grad) {
  if (!h || !x) return fail(OH_ERR_INVALID, "oh_tape_probe: null argument");
  if (h->desc.kind != OH_PROBLEM_TAPE) return fail(OH_ERR_STATE, "oh_tape_probe: handle is not an OH_PROBLEM_TAPE problem");
  TapeState& tp = h->tape;
  const TapeParams& T = tp.P;
  if (B < 1 || n_regs < 0 || (n_regs > 0 && !regs) || (T.np > 0 && !p)) return fail(OH_ERR_INVALID, "oh_tape_probe: bad sizes");
  for (int i = 0; i < n_regs; ++i)
    if (regs[i] < 0 || regs[i] >= T.len) return fail(OH_ERR_INVALID, "oh_tape_probe: register out of range");
  HIPCHK(hipSetDevice(h->device));
  const int Bp = (B + 63) / 64 * 64;
  const int nrow = T.n_ineq + T.n_eq;
  const size_t nB = (size_t)B, b_x = sizeof(double) * (size_t)T.nx * nB, b_s = sizeof(double) * (size_t)(1 + nrow) * nB;
  double *d_x, *d_g, *d_p, *d_v, *d_a, *d_s, *d_w;
  int* d_r;
  auto layout = [&](Carver c) {
    d_x = c.take<double>((size_t)T.nx * nB);
    d_g = c.take<double>((size_t)T.nx * nB);
    d_p = c.take<double>((size_t)(T.np > 0 ? T.np : 1) * nB);
    d_r = c.take<int>((size_t)n_regs + 1);
    d_v = c.take<double>((size_t)(n_regs + 1) * nB);
    d_a = c.take<double>((size_t)(n_regs + 1) * nB);
    d_s = c.take<double>((size_t)(1 + nrow) * nB);
    d_w = c.take<double>((2 * (size_t)T.len + 2 * (size_t)T.nx) * Bp);
    return c.bytes();
  };
  if (const int rc = stage_carve(h, layout)) return rc;
  hipStream_t s = h->stream;
  HIPCHK(hipMemcpyAsync(d_x, x, b_x, hipMemcpyHostToDevice, s));
  if (T.np > 0) HIPCHK(hipMemcpyAsync(d_p, p, sizeof(double) * (size_t)T.np * B, hipMemcpyHostToDevice, s));
  if (n_regs > 0) HIPCHK(hipMemcpyAsync(d_r, regs, sizeof(int) * (size_t)n_regs, hipMemcpyHostToDevice, s));
  if (seeds) HIPCHK(hipMemcpyAsync(d_s, seeds, b_s, hipMemcpyHostToDevice, s));
  oh_launch_tape_probe(s, T, tp.op, tp.a, tp.b, tp.c, tp.rows, B, Bp, d_x, d_p, d_w, n_regs, d_r, val ? d_v : nullptr,
                       seeds ? d_s : nullptr, (seeds && adj) ? d_a : nullptr, (seeds && grad) ? d_g : nullptr);
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  if (val && n_regs > 0) HIPCHK(hipMemcpy(val, d_v, sizeof(double) * (size_t)n_regs * B, hipMemcpyDeviceToHost));
  if (seeds && adj && n_regs > 0) HIPCHK(hipMemcpy(adj, d_a, sizeof(double) * (size_t)n_regs * B, hipMemcpyDeviceToHost));
  if (seeds && grad) HIPCHK(hipMemcpy(grad, d_g, b_x, hipMemcpyDeviceToHost));
  return OH_OK;
}

extern "C" int oh_tape_hvp(oh_handle* h, int B, const double* x, const double* p, const double* seeds, int nv, const double* V, double* HV, double* grad) {
  if (!h || !x || !seeds || !HV) return fail(OH_ERR_INVALID, "oh_tape_hvp: null argument");
  if (h->desc.kind != OH_PROBLEM_TAPE) return fail(OH_ERR_STATE, "oh_tape_hvp: handle is not an OH_PROBLEM_TAPE problem");
  TapeState& tp = h->tape;
  const TapeParams& T = tp.P;
  if (B < 1 || nv < 1 || (T.np > 0 && !p)) return fail(OH_ERR_INVALID, "oh_tape_hvp: bad sizes");
  if (!V && nv != T.nx) return fail(OH_ERR_INVALID, "oh_tape_hvp: V == NULL means the identity and needs nv == nx");
  const size_t nB = (size_t)B, U = nB * (size_t)nv;  // units: (instance, direction)
  if (U > (size_t)0x7fffffc0) return fail(OH_ERR_INVALID, "oh_tape_hvp: B * nv does not fit an int");
  HIPCHK(hipSetDevice(h->device));
  // option tape_hvp_wave on a handle whose wavefront schedule is ready: one block per unit on that schedule (k_tape_wave_hvp), the four register columns in
  // LDS (one launch) or in a work area of 4 n_reg doubles per unit in flight; every other handle, and a schedule whose columns fit nowhere: the interpreter
  const int path = optv(h, "tape_hvp_wave") != 0.0 ? oh_tape_wave_hvp_place(tp.wave) : 0;
  // the work area stays under the budget: whole 64-lane blocks of the interpreter per launch, units of the wavefront kernel (at least one block either way)
  const size_t per_unit = sizeof(double) * (path ? 4 * (size_t)tp.wave.n_reg : oh_tape_hvp_work_rows(T));
  const size_t grain = path ? 1 : 64;
  const double budget = optv(h, "tape_hvp_work_mb") * 1048576.0;
  size_t chunk = budget > 0.0 ? (size_t)(budget / (double)per_unit) / grain * grain : 0;
  if (chunk < grain) chunk = grain;
  const size_t Up = (U + grain - 1) / grain * grain;
  if (chunk > Up || path == 1) chunk = Up;  // (registers in LDS: no work area, one launch)
  const int nrow = T.n_ineq + T.n_eq;
  const size_t b_x = sizeof(double) * (size_t)T.nx * nB, b_u = sizeof(double) * (size_t)T.nx * U;
  double *d_x, *d_g, *d_p, *d_s, *d_v, *d_hv, *d_w;
  auto layout = [&](Carver c) {
    d_x = c.take<double>((size_t)T.nx * nB);
    d_g = c.take<double>((size_t)T.nx * nB);
    d_p = c.take<double>((size_t)(T.np > 0 ? T.np : 1) * nB);
    d_s = c.take<double>((size_t)(1 + nrow) * nB);
    d_v = c.take<double>(V ? (size_t)T.nx * U : 1);
    d_hv = c.take<double>((size_t)T.nx * U);
    d_w = c.take<double>(path == 1 ? 1 : per_unit / sizeof(double) * chunk);
    return c.bytes();
  };
  if (const int rc = stage_carve(h, layout)) return rc;
  hipStream_t s = h->stream;
  HIPCHK(hipMemcpyAsync(d_x, x, b_x, hipMemcpyHostToDevice, s));
  if (T.np > 0) HIPCHK(hipMemcpyAsync(d_p, p, sizeof(double) * (size_t)T.np * nB, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_s, seeds, sizeof(double) * (size_t)(1 + nrow) * nB, hipMemcpyHostToDevice, s));
  if (V) HIPCHK(hipMemcpyAsync(d_v, V, b_u, hipMemcpyHostToDevice, s));
  tp.hvp_launches = 0;
  tp.hvp_path = path;
  HIPCHK(hipEventRecord(h->ev0, s));  // oh_get_timing out[4]: device time of the launches, the copies outside
  for (size_t u0 = 0; u0 < U; u0 += chunk) {  // (one stream: a launch has the work area to itself)
    const size_t n = U - u0 < chunk ? U - u0 : chunk;
    if (path)
      HIPCHK(oh_launch_tape_wave_hvp(s, tp.wave, T, path == 1, (int)u0, (int)n, nv, d_x, d_p, d_s, V ? d_v : nullptr, d_w, d_hv, grad ? d_g : nullptr));
    else
      oh_launch_tape_hvp(s, T, tp.op, tp.a, tp.b, tp.c, tp.rows, (int)u0, (int)n, (int)chunk, nv, d_x, d_p, d_s, V ? d_v : nullptr, d_w, d_hv, grad ? d_g : nullptr);
    ++tp.hvp_launches;
  }
  if (const int rc = finish_solve(h, tp.hvp_launches)) return rc;
  HIPCHK(hipMemcpy(HV, d_hv, b_u, hipMemcpyDeviceToHost));
  if (grad) HIPCHK(hipMemcpy(grad, d_g, b_x, hipMemcpyDeviceToHost));
  return OH_OK;
}

extern "C" int oh_tape_phi_hvp(oh_handle* h, int B, const double* x, const double* p, const double* lam, const double* mu, double rho, int nv, const double* V,
                               double* HV, double* grad) {
  if (!h || !x || !V || !HV) return fail(OH_ERR_INVALID, "oh_tape_phi_hvp: null argument");
  if (h->desc.kind != OH_PROBLEM_TAPE) return fail(OH_ERR_STATE, "oh_tape_phi_hvp: handle is not an OH_PROBLEM_TAPE problem");
  TapeState& tp = h->tape;
  const TapeParams& T = tp.P;
  if (B < 1 || nv < 1 || (T.np > 0 && !p) || (T.n_ineq > 0 && !lam) || (T.n_eq > 0 && !mu)) return fail(OH_ERR_INVALID, "oh_tape_phi_hvp: bad sizes");
  if (!(rho > 0.0)) return fail(OH_ERR_INVALID, "oh_tape_phi_hvp: the penalty must be positive");
  HIPCHK(hipSetDevice(h->device));
  const int Bp = (B + 63) / 64 * 64;
  const size_t nB = (size_t)B, b_u = sizeof(double) * (size_t)T.nx * nB * (size_t)nv;
  // options tape_newton + tape_newton_wave on a handle whose schedule is ready: the sweep k_tape_wave_newton runs, one block per (instance, direction); every
  // other handle, and a schedule whose work set fits nowhere: the interpreter's hess_vec
  if (nB * (size_t)nv > (size_t)0x3fffffff) return fail(OH_ERR_INVALID, "oh_tape_phi_hvp: B * nv does not fit an int");
  const int path = (optv(h, "tape_newton") != 0.0 && optv(h, "tape_newton_wave") != 0.0) ? oh_tape_wave_newton_place(tp.wave, T) : 0;
  const int nrow1 = T.n_ineq + T.n_eq > 0 ? T.n_ineq + T.n_eq : 1;
  double *d_x, *d_g, *d_p, *d_l, *d_m, *d_v, *d_hv, *d_w;
  auto layout = [&](Carver c) {
    d_x = c.take<double>((size_t)T.nx * nB);
    d_g = c.take<double>((size_t)T.nx * nB);
    d_p = c.take<double>((size_t)(T.np > 0 ? T.np : 1) * nB);
    d_l = c.take<double>((size_t)(T.n_ineq > 0 ? T.n_ineq : 1) * nB);
    d_m = c.take<double>((size_t)(T.n_eq > 0 ? T.n_eq : 1) * nB);
    d_v = c.take<double>((size_t)T.nx * nB * nv);
    d_hv = c.take<double>((size_t)T.nx * nB * nv);
    d_w = c.take<double>(path ? (4 + (size_t)nrow1) * nB : oh_tape_newton_work_rows(T) * Bp);
    return c.bytes();
  };
  if (const int rc = stage_carve(h, layout)) return rc;
  hipStream_t s = h->stream;
  HIPCHK(hipMemcpyAsync(d_x, x, sizeof(double) * (size_t)T.nx * nB, hipMemcpyHostToDevice, s));
  if (T.np > 0) HIPCHK(hipMemcpyAsync(d_p, p, sizeof(double) * (size_t)T.np * nB, hipMemcpyHostToDevice, s));
  if (T.n_ineq > 0) HIPCHK(hipMemcpyAsync(d_l, lam, sizeof(double) * (size_t)T.n_ineq * nB, hipMemcpyHostToDevice, s));
  if (T.n_eq > 0) HIPCHK(hipMemcpyAsync(d_m, mu, sizeof(double) * (size_t)T.n_eq * nB, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_v, V, b_u, hipMemcpyHostToDevice, s));
  tp.newton_path = path;
  if (path)
    HIPCHK(oh_launch_tape_wave_phi_hvp(s, tp.wave, T, path, B, nv, d_x, d_p, d_l, d_m, rho, d_v, d_hv, d_g, d_w));
  else
    oh_launch_tape_phi_hvp(s, T, tp.op, tp.a, tp.b, tp.c, tp.rows, B, Bp, d_x, d_p, d_l, d_m, rho, nv, d_v, d_w, d_hv, grad ? d_g : nullptr);
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(HV, d_hv, b_u, hipMemcpyDeviceToHost));
  if (grad) HIPCHK(hipMemcpy(grad, d_g, sizeof(double) * (size_t)T.nx * nB, hipMemcpyDeviceToHost));
  return OH_OK;
}

extern "C" int oh_tape_newton_stats(oh_handle* h, int B, int* steps, int* hvps) {
  if (!h || !steps || !hvps) return fail(OH_ERR_INVALID, "oh_tape_newton_stats: null argument");
  if (h->desc.kind != OH_PROBLEM_TAPE) return fail(OH_ERR_STATE, "oh_tape_newton_stats: handle is not an OH_PROBLEM_TAPE problem");
  TapeState& tp = h->tape;
  if (!tp.last_newton || B < 1 || B != tp.nstat_B) return fail(OH_ERR_STATE, "oh_tape_newton_stats: the last solve of this handle was not a Newton-CG solve of B instances");
  HIPCHK(hipSetDevice(h->device));
  std::vector<int> both(2 * (size_t)B);
  HIPCHK(hipMemcpy(both.data(), tp.nstat, sizeof(int) * both.size(), hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) { steps[b] = both[2 * (size_t)b]; hvps[b] = both[2 * (size_t)b + 1]; }
  return OH_OK;
}

extern "C" int oh_tape_set_metric(oh_handle* h, const double* H0) {
  if (!h) return fail(OH_ERR_INVALID, "oh_tape_set_metric: null argument");
  if (h->desc.kind != OH_PROBLEM_TAPE) return fail(OH_ERR_INVALID, "oh_tape_set_metric: not an OH_PROBLEM_TAPE handle");
  HIPCHK(hipSetDevice(h->device));
  TapeState& tp = h->tape;
  const size_t n = (size_t)tp.P.nx;
  if (!H0) {
    tp.h0.release();
    tp.P.h0 = nullptr;
    return OH_OK;
  }
  // symmetric with a positive diagonal is what can be checked here without factorising; a matrix that is not positive definite costs the solver a
  // reset to steepest descent whenever the direction it gives does not descend (oh_tape_solver.h), never a wrong answer
  for (size_t i = 0; i < n; ++i) {
    if (!(H0[i * n + i] > 0.0)) return fail(OH_ERR_INVALID, "oh_tape_set_metric: diagonal entry not positive");
    for (size_t j = 0; j < i; ++j) {
      const double a = H0[i * n + j], b = H0[j * n + i];
      if (!(fabs(a - b) <= 1e-10 * (fabs(a) + fabs(b)) + 1e-300)) return fail(OH_ERR_INVALID, "oh_tape_set_metric: matrix not symmetric");
    }
  }
  HIPCHK(tp.h0.reserve(n * n));
  HIPCHK(hipMemcpy(tp.h0, H0, sizeof(double) * n * n, hipMemcpyHostToDevice));
  tp.P.h0 = tp.h0;
  return OH_OK;
}

// work arrays of the thread-per-instance evaluators and the multipliers' buffer for batches of up to Bp instances
static int tape_ensure_work(oh_handle* h, const int Bp) {
  TapeState& tp = h->tape;
  if (Bp > tp.cap()) {  // both at the new stride, or (an allocation failed) cap() == 0
    tp.work.release();
    tp.mult.release();
    size_t rows = oh_tape_work_rows(tp.P, tp.jit.fn != nullptr);
    // (a Newton-CG handle: its own work set, and room for the interpreter's layout, which oh_tape_phi launches on such a handle)
    if (optv(h, "tape_newton") != 0.0) rows = std::max(oh_tape_newton_work_rows(tp.P), oh_tape_work_rows(tp.P, false));
    // (a Newton-CG handle with a schedule keeps the interpreter's arrays too: k_tape_solve_newton is where it falls back to when the work set fits nowhere)
    if (!tp.wave.ready || (optv(h, "tape_newton") != 0.0 && oh_tape_wave_newton_place(tp.wave, tp.P) == 0)) HIPCHK(tp.work.reserve(rows * Bp));
    HIPCHK(tp.mult.reserve((size_t)(tp.P.n_ineq + tp.P.n_eq + 1) * Bp));
  }
  return OH_OK;
}

extern "C" int oh_tape_phi(oh_handle* h, int B, const double* x, const double* p, const double* lam, const double* mu, double rho, double* merit, double* f,
                           double* rows, double* grad, double* cmax, double* meas) {
  if (!h || !x || !merit || !f || !grad || !cmax || !meas) return fail(OH_ERR_INVALID, "oh_tape_phi: null argument");
  if (h->desc.kind != OH_PROBLEM_TAPE) return fail(OH_ERR_STATE, "oh_tape_phi: handle is not an OH_PROBLEM_TAPE problem");
  TapeState& tp = h->tape;
  const TapeParams& T = tp.P;
  const int nrow = T.n_ineq + T.n_eq;
  if (B < 1 || (T.np > 0 && !p) || (T.n_ineq > 0 && !lam) || (T.n_eq > 0 && !mu) || (nrow > 0 && !rows)) return fail(OH_ERR_INVALID, "oh_tape_phi: bad sizes");
  if (!(rho > 0.0)) return fail(OH_ERR_INVALID, "oh_tape_phi: the penalty must be positive");
  HIPCHK(hipSetDevice(h->device));
  const int Bp = (B + 63) / 64 * 64;
  if (tp.jit.fn && !tp.wave.ready && !tp.jit_phi.fn) {
    std::vector<char> code;
    std::string err;
    const std::string src = oh_tape_jit_source(T, tp.h_op.data(), tp.h_a.data(), tp.h_b.data(), tp.h_c.data(), tp.h_rows.empty() ? nullptr : tp.h_rows.data(), false);
    if (oh_tape_jit_compile(src, &code, &err) || oh_tape_jit_load(code, &tp.jit_phi, &err, false)) return fail(OH_ERR_HIP, ("oh_tape_phi: " + err).c_str());
  }
  if (const int rc = tape_ensure_work(h, Bp)) return rc;
  double *d_x, *d_g, *d_p, *d_l, *d_m, *d_r, *d_v, *d_f, *d_c, *d_s;
  auto layout = [&](Carver c) {
    const size_t nB = (size_t)B;
    d_x = c.take<double>((size_t)T.nx * nB);
    d_g = c.take<double>((size_t)T.nx * nB);
    d_p = c.take<double>((size_t)(T.np > 0 ? T.np : 1) * nB);
    d_l = c.take<double>((size_t)(T.n_ineq > 0 ? T.n_ineq : 1) * nB);
    d_m = c.take<double>((size_t)(T.n_eq > 0 ? T.n_eq : 1) * nB);
    d_r = c.take<double>((size_t)(nrow > 0 ? nrow : 1) * nB);
    for (double** q : {&d_v, &d_f, &d_c, &d_s}) *q = c.take<double>(nB);
    return c.bytes();
  };
  if (const int rc = stage_carve(h, layout)) return rc;
  hipStream_t s = h->stream;
  HIPCHK(hipMemcpyAsync(d_x, x, sizeof(double) * (size_t)T.nx * B, hipMemcpyHostToDevice, s));
  if (T.np > 0) HIPCHK(hipMemcpyAsync(d_p, p, sizeof(double) * (size_t)T.np * B, hipMemcpyHostToDevice, s));
  if (T.n_ineq > 0) HIPCHK(hipMemcpyAsync(d_l, lam, sizeof(double) * (size_t)T.n_ineq * B, hipMemcpyHostToDevice, s));
  if (T.n_eq > 0) HIPCHK(hipMemcpyAsync(d_m, mu, sizeof(double) * (size_t)T.n_eq * B, hipMemcpyHostToDevice, s));
  tp.phi_lds = 0;
  // the evaluator oh_solve launches for this handle and this B (tape_solve_device)
  if (tp.wave.ready)
    HIPCHK(oh_launch_tape_wave_phi(s, tp.wave, T, B, d_x, d_p, d_l, d_m, rho, d_v, d_f, d_r, d_g, d_c, d_s));
  else if (tp.jit.fn)
    HIPCHK(oh_launch_tape_jit_phi(s, tp.jit_phi, T, B, tp.cap(), d_x, d_p, d_l, d_m, rho, tp.work, d_v, d_f, d_r, d_g, d_c, d_s,
                                  (int)optv(h, "tape_lds_max"), &tp.phi_lds));
  else
    oh_launch_tape_phi(s, T, tp.op, tp.a, tp.b, tp.c, tp.rows, B, tp.cap(), d_x, d_p, d_l, d_m, rho, tp.work, d_v, d_f,
                       d_r, d_g, d_c, d_s);
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(merit, d_v, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(f, d_f, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cmax, d_c, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(meas, d_s, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(grad, d_g, sizeof(double) * (size_t)T.nx * B, hipMemcpyDeviceToHost));
  if (nrow > 0) HIPCHK(hipMemcpy(rows, d_r, sizeof(double) * (size_t)nrow * B, hipMemcpyDeviceToHost));
  return OH_OK;
}

int tape_solve_device(oh_handle* h, const Solve& a) {
  HIPCHK(hipSetDevice(h->device));
  TapeState& tp = h->tape;
  const int B = a.B, Bp = (B + 63) / 64 * 64;
  if (const int rc = tape_ensure_work(h, Bp)) return rc;
  tp.last_newton = optv(h, "tape_newton") != 0.0 ? 1 : 0;
  if (tp.last_newton) {
    const int cg = (int)optv(h, "tape_newton_cg");
    HIPCHK(tp.nstat.reserve(2 * (size_t)B));
    tp.nstat_B = B;
    // option tape_newton_wave on a handle whose schedule is ready and whose work set has a placement: one block per instance on the level schedule
    tp.newton_path = optv(h, "tape_newton_wave") != 0.0 ? oh_tape_wave_newton_place(tp.wave, tp.P) : 0;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    if (tp.newton_path) {
      HIPCHK(oh_launch_tape_wave_newton(h->stream, tp.wave, tp.P, tp.newton_path, B, cg > 0 ? cg : std::min(tp.P.nx, 50), a.x0, a.p, a.x, a.f, a.kkt, a.iters, a.status,
                                        tp.mult, tp.nstat));
      return finish_solve(h, 1);
    }
    oh_launch_tape_solve_newton(h->stream, tp.P, tp.op, tp.a, tp.b, tp.c, tp.rows, B, tp.cap(), cg > 0 ? cg : std::min(tp.P.nx, 50), a.x0, a.p, tp.work, a.x, a.f,
                                a.kkt, a.iters, a.status, tp.mult, tp.nstat);
    return finish_solve(h, 1);
  }
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  if (tp.wave.ready)
    HIPCHK(oh_launch_tape_wave(h->stream, tp.wave, tp.P, B, a.x0, a.p, a.x, a.f, a.kkt, a.iters, a.status, tp.mult));
  else if (tp.jit.fn)
    HIPCHK(oh_launch_tape_jit(h->stream, tp.jit, tp.P, B, tp.cap(), a.x0, a.p, tp.work, a.x, a.f, a.kkt, a.iters, a.status, tp.mult,
                              (int)optv(h, "tape_lds_max")));
  else
    oh_launch_tape_solve(h->stream, tp.P, tp.op, tp.a, tp.b, tp.c, tp.rows, B, tp.cap(), a.x0, a.p, tp.work, a.x, a.f, a.kkt, a.iters, a.status, tp.mult);
  return finish_solve(h, 1);
}
