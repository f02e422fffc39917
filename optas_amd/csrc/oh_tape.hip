// Generic small dense NLP family (SURVEY 8(f) rank 1 in spirit: the reference hands CasADi SX tapes to IPOPT; here the host compiles the
// problem's expression trees into ONE scalar instruction tape, optas_amd/tape.py, and the GPU evaluates it):
//
//     min f(x, p)   s.t.  rows[0 .. n_ineq) >= 0,   rows[n_ineq .. n_ineq + n_eq) = 0            (optimization.py:27-51 without the mirrored rows)
//
// One thread owns one instance.  An evaluation is one forward sweep and ONE reverse sweep seeded with the augmented-Lagrangian weights of
// all rows at once (cost 1, equality rows -mu + rho c, active inequality rows -(lam - rho g)), so the gradient of the merit costs two
// passes over the tape whatever the number of rows.  What an opcode computes and how its adjoint propagates is stated in oh_tape_ops.h; this file holds
// the two thread-per-instance evaluators behind the solver of oh_tape_solver.h (the third, one wavefront per instance, is oh_tape_wave.hip):
//   * the interpreter (InterpEval; k_tape_solve, k_tape_phi, k_tape_probe, with tangents beside it k_tape_hvp, and behind the Newton-CG solver of
//     oh_tape_newton.h k_tape_solve_newton and k_tape_phi_hvp, which call InterpEval::hess_vec): all lanes of a wavefront execute
//     the same tape instruction on registers that live in HBM/L2 as val[i][b] (every access one coalesced line).  No set-up cost, but each
//     instruction is a dependent memory round trip: latency bound;
//   * straight-line HIP code written by generate() below and compiled with hiprtc for gfx950 when the handle is created (desc.jit): SSA values
//     become VGPRs, the device compiler schedules, folds and shares the transcendentals.  Both compute the same IEEE operations in the
//     same order (contraction is switched off inside the generated evaluator), so they agree bit for bit.
// numpy restatement of evaluator and solver: oracle/tape_ref.py.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "oh_jit.h"  // the disk cache of run-time compiled code objects
#include "oh_kernels.h"
#include "oh_tape_solver_src.h"  // OH_TAPE_SOLVER_SRC: the text of oh_tape_solver.h, written by optas_amd/build.py
#include "oh_tape_newton.h"      // the truncated Newton-CG state machine behind InterpEval::hess_vec (option tape_newton); never part of a generated program

namespace {

struct TapeView {
  const int* __restrict__ op;
  const int* __restrict__ a;
  const int* __restrict__ bb;
  const double* __restrict__ c;
  const int* __restrict__ rows;
};

// What the rules of oh_tape_ops.h see of instruction i of an interpreter: a register read is a load from val[register][lane], a contribution a
// read-modify-write of adj[register][lane] (TIDX), each a dependent round trip -- a rule that does not name an operand does not load it.
struct InterpRegs {
  const TapeView& tv;
  const double* __restrict__ val;
  double* __restrict__ adj;
  const double* __restrict__ xs;   // the point, [variable][lane]
  const double* __restrict__ pb;   // the instance's parameters
  double* __restrict__ grad;       // [variable][lane]
  const int i, ia, ib, Bp, lane;
  __device__ size_t at(const int r) const { return (size_t)r * Bp + lane; }
  __device__ double cst() const { return tv.c[i]; }
  __device__ double x() const { return xs[at(ia)]; }
  __device__ double p() const { return pb[ia]; }
  __device__ double a() const { return val[at(ia)]; }
  __device__ double b() const { return val[at(ib)]; }
  __device__ double self() const { return val[at(i)]; }
  __device__ void add_a(const double v) { adj[at(ia)] += v; }
  __device__ void add_b(const double v) { adj[at(ib)] += v; }
  __device__ void sub_a(const double v) { adj[at(ia)] -= v; }
  __device__ void sub_b(const double v) { adj[at(ib)] -= v; }
  __device__ void add_x(const double v) { grad[at(ia)] += v; }
};

struct InterpEval {
  const TapeParams& T;
  const TapeView& tv;
  const TapeWork& W;
  double* __restrict__ val;
  double* __restrict__ adj;
  const double* __restrict__ pb;
  const int Bp, b;
  double* __restrict__ dval = nullptr;  // tangents and the adjoints' directional derivatives, [len][Bp] each: set only where hess_vec is called
  double* __restrict__ dadj = nullptr;

  // contraction off: one IEEE operation per tape operation, like the generated code and the numpy restatement
  __device__ void forward(const double* __restrict__ xs) {
#pragma clang fp contract(off)
    for (int i = 0; i < T.len; ++i) {
      const int o = tv.op[i] & OP_MASK;
      val[TIDX(i)] = tape_value(o, InterpRegs{tv, val, adj, xs, pb, nullptr, i, tv.a[i], tv.bb[i], Bp, b});
    }
  }

  // adj holds the seeds on entry (zero elsewhere); grad[k][b] accumulates d/dx_k
  __device__ void reverse(double* __restrict__ grad) {
#pragma clang fp contract(off)
    for (int k = 0; k < T.nx; ++k) grad[TIDX(k)] = 0.0;
    for (int i = T.len - 1; i >= 0; --i) {
      const double w = adj[TIDX(i)];
      const int o = tv.op[i];
      if (o & OP_DEAD) continue;  // no part in the gradient (oh_tape_ops.h)
      InterpRegs r{tv, val, adj, nullptr, pb, grad, i, tv.a[i], tv.bb[i], Bp, b};
      tape_adjoint(o, w, r);
    }
  }

  __device__ double phi(const double* __restrict__ xs, double* __restrict__ gout, const double rho, double* fout, double* cmax, double* meas) {
    forward(xs);
    for (int i = 0; i < T.len; ++i) adj[TIDX(i)] = 0.0;
    const double f = val[TIDX(T.out_cost)];
    adj[TIDX(T.out_cost)] = 1.0;
    double v = f, cm = 0.0, ms = 0.0;
    for (int i = 0; i < T.n_ineq; ++i) {
      const int r = tv.rows[i];
      const double g = val[TIDX(r)];
      adj[TIDX(r)] += tape_al_ineq(g, W.lam[TIDX(i)], rho, v, cm, ms);
      W.rowv[TIDX(i)] = g;
    }
    for (int i = 0; i < T.n_eq; ++i) {
      const int r = tv.rows[T.n_ineq + i];
      const double c = val[TIDX(r)];
      adj[TIDX(r)] += tape_al_eq(c, W.mu[TIDX(i)], rho, v, cm, ms);
      W.rowv[TIDX(T.n_ineq + i)] = c;
    }
    reverse(gout);
    *fout = f;
    *cmax = cm;
    *meas = ms;
    return v;
  }

  // out = (generalised Hessian of the merit at x) v, forward-over-reverse with SEED TANGENTS (v, out: SoA [variable][lane]).
  // INVARIANT: the call follows a phi at the same x with the same multipliers (W.lam, W.mu) and the same rho, and nothing has written val, adj or W.rowv
  // since.  Then val[] holds the values and adj[] every register's FINAL adjoint -- the w of the second-order reverse rules -- so a product is one tangent
  // sweep and one dadj sweep and repeats no primal work.  An inequality row with lam - rho g > 0 (tape_al_ineq's own expression: a tie is inactive) has the
  // seed -(lam - rho g), whose tangent is rho dval[row]; an inactive one seed and tangent 0; an equality row -mu + rho c and rho dval[row].  Kinks hold the
  // selection of the base point, as k_tape_hvp documents.  Dead instructions take no part in either sweep (no live one reads them).
  // The second-order lines are written out here a second time beside k_tape_hvp's: there each stands next to the primal accumulation adj += ... it
  // differentiates, which this method must NOT repeat (adj is final), and that kernel's text is kept as measured (see its comment).  Names: oh_tape_ops.h.
  __device__ void hess_vec(const double* __restrict__ v, const double rho, double* __restrict__ out) {
#pragma clang fp contract(off)
    for (int i = 0; i < T.len; ++i) {
      const int o = tv.op[i], ia = tv.a[i], ib = tv.bb[i];
      if (o & OP_DEAD) continue;
      double t;
      switch (o) {
        case OP_X: t = v[TIDX(ia)]; break;
        case OP_ADD: t = dval[TIDX(ia)] + dval[TIDX(ib)]; break;
        case OP_SUB: t = dval[TIDX(ia)] - dval[TIDX(ib)]; break;
        case OP_MUL: t = dval[TIDX(ia)] * val[TIDX(ib)] + val[TIDX(ia)] * dval[TIDX(ib)]; break;
        case OP_DIV: t = (dval[TIDX(ia)] - val[TIDX(i)] * dval[TIDX(ib)]) / val[TIDX(ib)]; break;
        case OP_NEG: t = -dval[TIDX(ia)]; break;
        case OP_SIN: t = cos(val[TIDX(ia)]) * dval[TIDX(ia)]; break;
        case OP_COS: t = -(sin(val[TIDX(ia)]) * dval[TIDX(ia)]); break;
        case OP_ATAN2: {
          const double va = val[TIDX(ia)], vb = val[TIDX(ib)];
          t = (vb * dval[TIDX(ia)] - va * dval[TIDX(ib)]) / (va * va + vb * vb);
        } break;
        case OP_SQRT: t = 0.5 / val[TIDX(i)] * dval[TIDX(ia)]; break;
        case OP_SQR: t = 2.0 * val[TIDX(ia)] * dval[TIDX(ia)]; break;
        case OP_ASIN: { const double va = val[TIDX(ia)]; t = dval[TIDX(ia)] / sqrt((1.0 - va) * (1.0 + va)); } break;
        case OP_FABS: { const double va = val[TIDX(ia)]; t = (va > 0.0 ? 1.0 : (va < 0.0 ? -1.0 : 0.0)) * dval[TIDX(ia)]; } break;
        case OP_FMIN: t = val[TIDX(ia)] <= val[TIDX(ib)] ? dval[TIDX(ia)] : dval[TIDX(ib)]; break;
        case OP_FMAX: t = val[TIDX(ia)] >= val[TIDX(ib)] ? dval[TIDX(ia)] : dval[TIDX(ib)]; break;
        case OP_IFZ: t = val[TIDX(ia)] != 0.0 ? dval[TIDX(ib)] : 0.0; break;
        case OP_EXP: t = val[TIDX(i)] * dval[TIDX(ia)]; break;
        case OP_LOG: t = dval[TIDX(ia)] / val[TIDX(ia)]; break;
        default: t = 0.0; break;  // CONST, P, LT .. OR
      }
      dval[TIDX(i)] = t;
    }
    for (int i = 0; i < T.len; ++i) dadj[TIDX(i)] = 0.0;
    for (int i = 0; i < T.n_ineq; ++i) {
      const int r = tv.rows[i];
      double v0 = 0.0, c0 = 0.0, m0 = 0.0;
      if (tape_al_ineq(W.rowv[TIDX(i)], W.lam[TIDX(i)], rho, v0, c0, m0) < 0.0) dadj[TIDX(r)] += rho * dval[TIDX(r)];  // the seed phi planted is not zero: active
    }
    for (int i = 0; i < T.n_eq; ++i) {
      const int r = tv.rows[T.n_ineq + i];
      dadj[TIDX(r)] += rho * dval[TIDX(r)];
    }
    for (int k = 0; k < T.nx; ++k) out[TIDX(k)] = 0.0;
    for (int i = T.len - 1; i >= 0; --i) {
      const int o = tv.op[i], ia = tv.a[i], ib = tv.bb[i];
      if (o & OP_DEAD) continue;
      const double w = adj[TIDX(i)], dw = dadj[TIDX(i)];
      switch (o) {
        case OP_X: out[TIDX(ia)] += dw; break;
        case OP_ADD: dadj[TIDX(ia)] += dw; dadj[TIDX(ib)] += dw; break;
        case OP_SUB: dadj[TIDX(ia)] += dw; dadj[TIDX(ib)] -= dw; break;
        case OP_MUL: {
          const double va = val[TIDX(ia)], vb = val[TIDX(ib)], ta = dval[TIDX(ia)], tb = dval[TIDX(ib)];
          dadj[TIDX(ia)] += dw * vb + w * tb;
          dadj[TIDX(ib)] += dw * va + w * ta;
        } break;
        case OP_DIV: {
          const double va = val[TIDX(ia)], vb = val[TIDX(ib)], ta = dval[TIDX(ia)], tb = dval[TIDX(ib)];
          dadj[TIDX(ia)] += (dw - w * tb / vb) / vb;
          dadj[TIDX(ib)] -= (dw * va + w * ta - 2.0 * (w * va) * tb / vb) / (vb * vb);
        } break;
        case OP_NEG: dadj[TIDX(ia)] -= dw; break;
        case OP_SIN: { const double va = val[TIDX(ia)]; dadj[TIDX(ia)] += dw * cos(va) - w * sin(va) * dval[TIDX(ia)]; } break;
        case OP_COS: { const double va = val[TIDX(ia)]; dadj[TIDX(ia)] -= dw * sin(va) + w * cos(va) * dval[TIDX(ia)]; } break;
        case OP_ATAN2: {
          const double va = val[TIDX(ia)], vb = val[TIDX(ib)], ta = dval[TIDX(ia)], tb = dval[TIDX(ib)], d = va * va + vb * vb;
          const double dd = 2.0 * (va * ta + vb * tb);
          dadj[TIDX(ia)] += (dw * vb + w * (tb - vb * dd / d)) / d;
          dadj[TIDX(ib)] -= (dw * va + w * (ta - va * dd / d)) / d;
        } break;
        case OP_SQRT: { const double r = val[TIDX(i)], q = 0.5 / r; dadj[TIDX(ia)] += dw * q - w * (q * dval[TIDX(i)] / r); } break;
        case OP_SQR: dadj[TIDX(ia)] += dw * 2.0 * val[TIDX(ia)] + w * 2.0 * dval[TIDX(ia)]; break;
        case OP_ASIN: {
          const double va = val[TIDX(ia)], s = (1.0 - va) * (1.0 + va), r = sqrt(s);
          dadj[TIDX(ia)] += dw / r + w * (va * dval[TIDX(ia)] / (s * r));
        } break;
        case OP_FABS: { const double va = val[TIDX(ia)]; dadj[TIDX(ia)] += dw * (va > 0.0 ? 1.0 : (va < 0.0 ? -1.0 : 0.0)); } break;
        case OP_FMIN: if (val[TIDX(ia)] <= val[TIDX(ib)]) dadj[TIDX(ia)] += dw; else dadj[TIDX(ib)] += dw; break;
        case OP_FMAX: if (val[TIDX(ia)] >= val[TIDX(ib)]) dadj[TIDX(ia)] += dw; else dadj[TIDX(ib)] += dw; break;
        case OP_IFZ: if (val[TIDX(ia)] != 0.0) dadj[TIDX(ib)] += dw; break;
        case OP_EXP: dadj[TIDX(ia)] += dw * val[TIDX(i)] + w * dval[TIDX(i)]; break;
        case OP_LOG: { const double va = val[TIDX(ia)]; dadj[TIDX(ia)] += (dw - w * dval[TIDX(ia)] / va) / va; } break;
        default: break;  // CONST, P, LT .. OR
      }
    }
  }
};

__global__ __launch_bounds__(64) void k_tape_solve(TapeParams T, TapeView tv, int B, int Bp, const double* __restrict__ x0, const double* __restrict__ par,
                                                   double* __restrict__ work, double* __restrict__ xo, double* __restrict__ fo, double* __restrict__ kkt,
                                                   int* __restrict__ iters, int* __restrict__ status, double* __restrict__ mult) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const TapeWork W = tape_carve(T, work + 2 * (size_t)T.len * Bp, Bp);
  InterpEval ev{T, tv, W, work, work + (size_t)T.len * Bp, par + (size_t)b * T.np, Bp, b};
  tape_solve_instance(T, ev, W, Bp, b, b, x0, xo, fo, kkt, iters, status, mult);
}

// The Newton-CG solve (option tape_newton): one thread per instance.  work: [4 len + tape_newton_rows][Bp] -- registers, adjoints, tangents, the adjoints'
// directional derivatives, then the solver's vectors (tape_newton_carve).
__global__ __launch_bounds__(64) void k_tape_solve_newton(TapeParams T, TapeView tv, int B, int Bp, int cg_cap, const double* __restrict__ x0,
                                                          const double* __restrict__ par, double* __restrict__ work, double* __restrict__ xo,
                                                          double* __restrict__ fo, double* __restrict__ kkt, int* __restrict__ iters, int* __restrict__ status,
                                                          double* __restrict__ mult, int* __restrict__ stats) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const size_t L = (size_t)T.len * Bp;
  const TapeNewtonWork N = tape_newton_carve(T, work + 4 * L, Bp);
  InterpEval ev{T, tv, N.W, work, work + L, par + (size_t)b * T.np, Bp, b, work + 2 * L, work + 3 * L};
  tape_newton_instance(T, ev, N, cg_cap, Bp, b, b, x0, xo, fo, kkt, iters, status, mult, stats);
}

// One InterpEval::phi per instance at given points, multipliers and penalty, then nv calls of the hess_vec the solver calls (oh_tape_phi_hvp).
// V, HV: [B][nv][nx]; grad (may be null): the gradient that phi returned.  work: the Newton solve kernel's layout.
__global__ __launch_bounds__(64) void k_tape_phi_hvp(TapeParams T, TapeView tv, int B, int Bp, const double* __restrict__ x, const double* __restrict__ par,
                                                     const double* __restrict__ lam, const double* __restrict__ mu, double rho, int nv,
                                                     const double* __restrict__ V, double* __restrict__ work, double* __restrict__ HV,
                                                     double* __restrict__ grad) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const size_t L = (size_t)T.len * Bp;
  const TapeNewtonWork N = tape_newton_carve(T, work + 4 * L, Bp);
  const TapeWork& W = N.W;
  InterpEval ev{T, tv, W, work, work + L, par + (size_t)b * T.np, Bp, b, work + 2 * L, work + 3 * L};
  const int n = T.nx;
  for (int k = 0; k < n; ++k) W.x[TIDX(k)] = x[(size_t)b * n + k];
  for (int i = 0; i < T.n_ineq; ++i) W.lam[TIDX(i)] = lam[(size_t)b * T.n_ineq + i];
  for (int i = 0; i < T.n_eq; ++i) W.mu[TIDX(i)] = mu[(size_t)b * T.n_eq + i];
  double fv, cm, ms;
  ev.phi(W.x, W.g, rho, &fv, &cm, &ms);
  if (grad)
    for (int k = 0; k < n; ++k) grad[(size_t)b * n + k] = W.g[TIDX(k)];
  for (int d = 0; d < nv; ++d) {
    const size_t at = ((size_t)b * nv + d) * n;
    for (int k = 0; k < n; ++k) N.p[TIDX(k)] = V[at + k];
    ev.hess_vec(N.p, rho, N.hp);
    for (int k = 0; k < n; ++k) HV[at + k] = N.hp[TIDX(k)];
  }
}

// One forward sweep (and, seeded, one reverse sweep) at given points: values / adjoints of chosen registers and the gradient wrt x (oh_tape_probe).
// work: [2 len + 2 nx][Bp] -- registers, adjoints, the point and the gradient in the interpreter's SoA layout.
__global__ __launch_bounds__(64) void k_tape_probe(TapeParams T, TapeView tv, int B, int Bp, const double* __restrict__ x, const double* __restrict__ par,
                                                   double* __restrict__ work, int n_regs, const int* __restrict__ regs, double* __restrict__ val_out,
                                                   const double* __restrict__ seeds, double* __restrict__ adj_out, double* __restrict__ grad_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double* val = work;
  double* adj = work + (size_t)T.len * Bp;
  double* xs = work + 2 * (size_t)T.len * Bp;
  double* gr = xs + (size_t)T.nx * Bp;
  for (int k = 0; k < T.nx; ++k) xs[TIDX(k)] = x[(size_t)b * T.nx + k];
  const TapeWork none{};
  InterpEval ev{T, tv, none, val, adj, par + (size_t)b * T.np, Bp, b};
  ev.forward(xs);
  if (val_out)
    for (int i = 0; i < n_regs; ++i) val_out[(size_t)b * n_regs + i] = val[TIDX(regs[i])];
  if (!seeds) return;
  for (int i = 0; i < T.len; ++i) adj[TIDX(i)] = 0.0;
  const int nrow = T.n_ineq + T.n_eq;
  const double* sd = seeds + (size_t)b * (1 + nrow);
  adj[TIDX(T.out_cost)] += sd[0];
  for (int i = 0; i < nrow; ++i) adj[TIDX(tv.rows[i])] += sd[1 + i];
  ev.reverse(gr);
  // (the reverse sweep leaves in adj[i] the derivative of the seeded combination with respect to register i)
  if (adj_out)
    for (int i = 0; i < n_regs; ++i) adj_out[(size_t)b * n_regs + i] = adj[TIDX(regs[i])];
  if (grad_out)
    for (int k = 0; k < T.nx; ++k) grad_out[(size_t)b * T.nx + k] = gr[TIDX(k)];
}

// Exact Hessian-vector products of the seeded combination of (cost, rows) by forward-over-reverse on the interpreter (oh_tape_hvp).  One lane per unit
// u = b nv + d (instance b, direction d, the direction fastest); the launch covers the units [u0, u0 + n) and lane l = u - u0 owns column l of the work
// area [4 len + 3 nx][Bp]: registers, tangents, adjoints, the adjoints' directional derivatives, then the point, the gradient and H v.  The forward sweep is
// InterpEval::forward with the tangent dval = (d val / d x) v beside every value, the reverse sweep InterpEval::reverse with dadj = (d adj / d x) v
// beside every adjoint: the primal operations are those sweeps' operations in their order, so the gradient has oh_tape_probe's bits, and a unit
// reads nothing of another unit, so its result does not depend on B, nv or the launch it falls into.  A kink holds the selection of the base point
// (FMIN / FMAX: value, tangent and adjoint of the chosen operand, a tie to a; FABS: slope +-1 or 0, no curvature; IFZ: b where a != 0, nothing to the
// condition; LT .. OR: zero tangent, no adjoint).  Zero adjoints and tangents are multiplied through like every other.
// V null: direction d is e_d (nv == nx), formed here.  The tape is the one the handle holds: on a wave handle the re-associated one.
// The primal lines are written out beside their second-order lines, with oh_tape_ops.h's names -- a third statement of the rules, to be changed
// with them: taken from tape_value / tape_adjoint (one call per case, the tangent and dadj lines kept here) every bit was the same and the dense
// Hessian of the 280-variable planner at B = 256 took 351.5 ms against 349.5 ms (six runs each, no overlap).
__global__ __launch_bounds__(64) void k_tape_hvp(TapeParams T, TapeView tv, int u0, int n, int Bp, int nv, const double* __restrict__ x,
                                                 const double* __restrict__ par, const double* __restrict__ seeds, const double* __restrict__ V,
                                                 double* __restrict__ work, double* __restrict__ HV, double* __restrict__ grad_out) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;  // the unit's column of the work area (TIDX)
  if (b >= n) return;
  const size_t u = (size_t)u0 + b;
  const size_t inst = u / (size_t)nv;
  const int dir = (int)(u % (size_t)nv);
  const size_t L = (size_t)T.len * Bp;
  double* __restrict__ val = work;
  double* __restrict__ dval = work + L;
  double* __restrict__ adj = work + 2 * L;
  double* __restrict__ dadj = work + 3 * L;
  double* __restrict__ xs = work + 4 * L;
  double* __restrict__ gr = xs + (size_t)T.nx * Bp;
  double* __restrict__ hv = gr + (size_t)T.nx * Bp;
  const double* __restrict__ pb = par + inst * T.np;
  const double* __restrict__ vd = V ? V + u * T.nx : nullptr;
  for (int k = 0; k < T.nx; ++k) xs[TIDX(k)] = x[inst * T.nx + k];
  // ---- forward: tape_value's rules (InterpEval::forward), and the tangent of every register
  for (int i = 0; i < T.len; ++i) {
    const int o = tv.op[i] & OP_MASK, ia = tv.a[i], ib = tv.bb[i];
    double v, t;
    switch (o) {
      case OP_CONST: v = tv.c[i]; t = 0.0; break;
      case OP_X: v = xs[TIDX(ia)]; t = vd ? vd[ia] : (ia == dir ? 1.0 : 0.0); break;
      case OP_P: v = pb[ia]; t = 0.0; break;
      case OP_ADD: v = val[TIDX(ia)] + val[TIDX(ib)]; t = dval[TIDX(ia)] + dval[TIDX(ib)]; break;
      case OP_SUB: v = val[TIDX(ia)] - val[TIDX(ib)]; t = dval[TIDX(ia)] - dval[TIDX(ib)]; break;
      case OP_MUL: { const double va = val[TIDX(ia)], vb = val[TIDX(ib)]; v = va * vb; t = dval[TIDX(ia)] * vb + va * dval[TIDX(ib)]; } break;
      case OP_DIV: { const double va = val[TIDX(ia)], vb = val[TIDX(ib)]; v = va / vb; t = (dval[TIDX(ia)] - v * dval[TIDX(ib)]) / vb; } break;
      case OP_NEG: v = -val[TIDX(ia)]; t = -dval[TIDX(ia)]; break;
      case OP_SIN: { const double va = val[TIDX(ia)]; v = sin(va); t = cos(va) * dval[TIDX(ia)]; } break;
      case OP_COS: { const double va = val[TIDX(ia)]; v = cos(va); t = -(sin(va) * dval[TIDX(ia)]); } break;
      case OP_ATAN2: {
        const double va = val[TIDX(ia)], vb = val[TIDX(ib)];
        v = atan2(va, vb);
        t = (vb * dval[TIDX(ia)] - va * dval[TIDX(ib)]) / (va * va + vb * vb);
      } break;
      case OP_SQRT: v = sqrt(val[TIDX(ia)]); t = 0.5 / v * dval[TIDX(ia)]; break;
      case OP_SQR: { const double va = val[TIDX(ia)]; v = va * va; t = 2.0 * va * dval[TIDX(ia)]; } break;
      case OP_ASIN: { const double va = val[TIDX(ia)]; v = asin(va); t = dval[TIDX(ia)] / sqrt((1.0 - va) * (1.0 + va)); } break;
      case OP_FABS: { const double va = val[TIDX(ia)]; v = fabs(va); t = (va > 0.0 ? 1.0 : (va < 0.0 ? -1.0 : 0.0)) * dval[TIDX(ia)]; } break;
      case OP_FMIN: { const double va = val[TIDX(ia)], vb = val[TIDX(ib)]; v = fmin(va, vb); t = va <= vb ? dval[TIDX(ia)] : dval[TIDX(ib)]; } break;
      case OP_FMAX: { const double va = val[TIDX(ia)], vb = val[TIDX(ib)]; v = fmax(va, vb); t = va >= vb ? dval[TIDX(ia)] : dval[TIDX(ib)]; } break;
      case OP_LT: v = val[TIDX(ia)] < val[TIDX(ib)] ? 1.0 : 0.0; t = 0.0; break;
      case OP_LE: v = val[TIDX(ia)] <= val[TIDX(ib)] ? 1.0 : 0.0; t = 0.0; break;
      case OP_EQ: v = val[TIDX(ia)] == val[TIDX(ib)] ? 1.0 : 0.0; t = 0.0; break;
      case OP_NE: v = val[TIDX(ia)] != val[TIDX(ib)] ? 1.0 : 0.0; t = 0.0; break;
      case OP_NOT: v = val[TIDX(ia)] == 0.0 ? 1.0 : 0.0; t = 0.0; break;
      case OP_AND: v = (val[TIDX(ia)] != 0.0 && val[TIDX(ib)] != 0.0) ? 1.0 : 0.0; t = 0.0; break;
      case OP_OR: v = (val[TIDX(ia)] != 0.0 || val[TIDX(ib)] != 0.0) ? 1.0 : 0.0; t = 0.0; break;
      case OP_IFZ: { const bool on = val[TIDX(ia)] != 0.0; v = on ? val[TIDX(ib)] : 0.0; t = on ? dval[TIDX(ib)] : 0.0; } break;
      case OP_EXP: v = exp(val[TIDX(ia)]); t = v * dval[TIDX(ia)]; break;
      default: { const double va = val[TIDX(ia)]; v = log(va); t = dval[TIDX(ia)] / va; } break;  // OP_LOG
    }
    val[TIDX(i)] = v;
    dval[TIDX(i)] = t;
  }
  // ---- seeds: oh_tape_probe's (the weights do not depend on x: their tangent is zero)
  for (int i = 0; i < T.len; ++i) { adj[TIDX(i)] = 0.0; dadj[TIDX(i)] = 0.0; }
  const int nrow = T.n_ineq + T.n_eq;
  const double* sd = seeds + inst * (1 + nrow);
  adj[TIDX(T.out_cost)] += sd[0];
  for (int i = 0; i < nrow; ++i) adj[TIDX(tv.rows[i])] += sd[1 + i];
  // ---- reverse: tape_adjoint's rules (InterpEval::reverse), and beside every  adj[r] += w q  its derivative along v,  dadj[r] += dw q + w dq
  // (the operands' values and tangents are read before anything is accumulated, and the two accumulations of a binary instruction are separate
  //  read-modify-writes: MUL a a adds both contributions to the one register)
  for (int k = 0; k < T.nx; ++k) { gr[TIDX(k)] = 0.0; hv[TIDX(k)] = 0.0; }
  for (int i = T.len - 1; i >= 0; --i) {
    const double w = adj[TIDX(i)], dw = dadj[TIDX(i)];
    const int o = tv.op[i], ia = tv.a[i], ib = tv.bb[i];
    if (o & OP_DEAD) continue;  // dead: no part in the gradient, none in H v
    switch (o) {
      case OP_CONST: case OP_P: break;
      case OP_X: gr[TIDX(ia)] += w; hv[TIDX(ia)] += dw; break;
      case OP_ADD: adj[TIDX(ia)] += w; adj[TIDX(ib)] += w; dadj[TIDX(ia)] += dw; dadj[TIDX(ib)] += dw; break;
      case OP_SUB: adj[TIDX(ia)] += w; adj[TIDX(ib)] -= w; dadj[TIDX(ia)] += dw; dadj[TIDX(ib)] -= dw; break;
      case OP_MUL: {
        const double va = val[TIDX(ia)], vb = val[TIDX(ib)], ta = dval[TIDX(ia)], tb = dval[TIDX(ib)];
        adj[TIDX(ia)] += w * vb;
        adj[TIDX(ib)] += w * va;
        dadj[TIDX(ia)] += dw * vb + w * tb;
        dadj[TIDX(ib)] += dw * va + w * ta;
      } break;
      case OP_DIV: {
        const double va = val[TIDX(ia)], vb = val[TIDX(ib)], ta = dval[TIDX(ia)], tb = dval[TIDX(ib)];
        adj[TIDX(ia)] += w / vb;
        adj[TIDX(ib)] -= w * va / (vb * vb);
        // d (1 / b) = -tb / b^2;   d (a / b^2) = ta / b^2 - 2 a tb / b^3
        dadj[TIDX(ia)] += (dw - w * tb / vb) / vb;
        dadj[TIDX(ib)] -= (dw * va + w * ta - 2.0 * (w * va) * tb / vb) / (vb * vb);
      } break;
      case OP_NEG: adj[TIDX(ia)] -= w; dadj[TIDX(ia)] -= dw; break;
      case OP_SIN: {
        const double va = val[TIDX(ia)], ta = dval[TIDX(ia)], c = cos(va);
        adj[TIDX(ia)] += w * c;
        dadj[TIDX(ia)] += dw * c - w * sin(va) * ta;
      } break;
      case OP_COS: {
        const double va = val[TIDX(ia)], ta = dval[TIDX(ia)], s = sin(va);
        adj[TIDX(ia)] -= w * s;
        dadj[TIDX(ia)] -= dw * s + w * cos(va) * ta;
      } break;
      case OP_ATAN2: {
        const double va = val[TIDX(ia)], vb = val[TIDX(ib)], ta = dval[TIDX(ia)], tb = dval[TIDX(ib)], d = va * va + vb * vb;
        adj[TIDX(ia)] += w * vb / d;
        adj[TIDX(ib)] -= w * va / d;
        // d (b / d) = (tb - b dd / d) / d,  d (a / d) = (ta - a dd / d) / d  with  dd = 2 (a ta + b tb)
        const double dd = 2.0 * (va * ta + vb * tb);
        dadj[TIDX(ia)] += (dw * vb + w * (tb - vb * dd / d)) / d;
        dadj[TIDX(ib)] -= (dw * va + w * (ta - va * dd / d)) / d;
      } break;
      case OP_SQRT: {  // q = 0.5 / sqrt(a);  dq = -q (q ta) / sqrt(a)
        const double r = val[TIDX(i)], q = 0.5 / r;
        adj[TIDX(ia)] += w * 0.5 / r;
        dadj[TIDX(ia)] += dw * q - w * (q * dval[TIDX(i)] / r);
      } break;
      case OP_SQR: {
        const double va = val[TIDX(ia)];
        adj[TIDX(ia)] += w * 2.0 * va;
        dadj[TIDX(ia)] += dw * 2.0 * va + w * 2.0 * dval[TIDX(ia)];
      } break;
      case OP_ASIN: {  // q = 1 / sqrt((1 - a)(1 + a));  dq = a ta q / ((1 - a)(1 + a))
        const double va = val[TIDX(ia)], s = (1.0 - va) * (1.0 + va), r = sqrt(s);
        adj[TIDX(ia)] += w / r;
        dadj[TIDX(ia)] += dw / r + w * (va * dval[TIDX(ia)] / (s * r));
      } break;
      case OP_FABS: {
        const double va = val[TIDX(ia)], sg = va > 0.0 ? 1.0 : (va < 0.0 ? -1.0 : 0.0);
        adj[TIDX(ia)] += w * sg;
        dadj[TIDX(ia)] += dw * sg;
      } break;
      case OP_FMIN:
        if (val[TIDX(ia)] <= val[TIDX(ib)]) { adj[TIDX(ia)] += w; dadj[TIDX(ia)] += dw; } else { adj[TIDX(ib)] += w; dadj[TIDX(ib)] += dw; }
        break;
      case OP_FMAX:
        if (val[TIDX(ia)] >= val[TIDX(ib)]) { adj[TIDX(ia)] += w; dadj[TIDX(ia)] += dw; } else { adj[TIDX(ib)] += w; dadj[TIDX(ib)] += dw; }
        break;
      case OP_IFZ:
        if (val[TIDX(ia)] != 0.0) { adj[TIDX(ib)] += w; dadj[TIDX(ib)] += dw; }
        break;
      case OP_EXP: {  // q = exp(a) = val[i], dq = dval[i]
        adj[TIDX(ia)] += w * val[TIDX(i)];
        dadj[TIDX(ia)] += dw * val[TIDX(i)] + w * dval[TIDX(i)];
      } break;
      case OP_LOG: {
        const double va = val[TIDX(ia)];
        adj[TIDX(ia)] += w / va;
        dadj[TIDX(ia)] += (dw - w * dval[TIDX(ia)] / va) / va;
      } break;
      default: break;  // LT .. OR
    }
  }
  for (int k = 0; k < T.nx; ++k) HV[u * T.nx + k] = hv[TIDX(k)];
  if (grad_out && dir == 0)
    for (int k = 0; k < T.nx; ++k) grad_out[inst * T.nx + k] = gr[TIDX(k)];
}

// One InterpEval::phi per instance at given points, multipliers and penalty (oh_tape_phi).  work: the solve kernel's layout.
__global__ __launch_bounds__(64) void k_tape_phi(TapeParams T, TapeView tv, int B, int Bp, const double* __restrict__ x, const double* __restrict__ par,
                                                 const double* __restrict__ lam, const double* __restrict__ mu, double rho, double* __restrict__ work,
                                                 double* __restrict__ merit, double* __restrict__ fo, double* __restrict__ rows, double* __restrict__ grad,
                                                 double* __restrict__ cmax, double* __restrict__ meas) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const TapeWork W = tape_carve(T, work + 2 * (size_t)T.len * Bp, Bp);
  InterpEval ev{T, tv, W, work, work + (size_t)T.len * Bp, par + (size_t)b * T.np, Bp, b};
  tape_phi_instance(T, ev, W, Bp, b, b, x, lam, mu, rho, merit, fo, rows, grad, cmax, meas);
}

// ---- code generation ------------------------------------------------------------------------------------------------------------------
void emit(std::string& s, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  s += buf;
}

// A double as a C++ expression: hexadecimal floating literal; the non-finite values, which have no literal, through the compiler's builtins
// (fmin(x, inf) is a legal casadi graph)
std::string literal(const double v) {
  if (v != v) return "__builtin_nan(\"\")";
  if (v == HUGE_VAL) return "__builtin_inf()";
  if (v == -HUGE_VAL) return "(-__builtin_inf())";
  char buf[64];
  snprintf(buf, sizeof buf, "%a", v);
  return buf;
}

// solve: the two solver kernels behind the evaluator (what a handle is created with); otherwise the two single-evaluation kernels of oh_tape_phi,
// a program of its own compiled when first asked for
std::string generate(const TapeParams& T, const int* op, const int* a, const int* bb, const double* c, const int* rows, const bool solve = true) {
  std::string s;
  s.reserve(64 * (size_t)T.len + sizeof(OH_TAPE_SOLVER_SRC) + 4096);
  emit(s, "#define OH_TAPE_ST_CONVERGED %d\n#define OH_TAPE_ST_MAX_ITER %d\n#define OH_TAPE_ST_NUMERICAL %d\n", (int)OH_STATUS_CONVERGED, (int)OH_STATUS_MAX_ITER,
       (int)OH_STATUS_NUMERICAL);
  s += OH_TAPE_SOLVER_SRC;
  s += "\nstruct JitEval {\n  const TapeWork& W;\n  const double* __restrict__ pb;\n  const int Bp, b;\n"
       "  __device__ double phi(const double* __restrict__ xs, double* __restrict__ gout, const double rho, double* fout, double* cmax, double* meas) {\n"
       "#pragma clang fp contract(off)\n";
  // which registers the reverse sweep reaches: everything the cost and the rows depend on
  const std::vector<char> live = tape_live(T.len, op, a, bb, rows, T.n_ineq + T.n_eq, T.out_cost);
  // value table: the text of tape_value's rules (oh_tape_ops.h) -- keep the two in step
  for (int i = 0; i < T.len; ++i) {
    if (!live[i]) continue;
    switch (op[i]) {
      case OP_CONST: emit(s, "    const double v%d = %s;\n", i, literal(c[i]).c_str()); break;
      case OP_X: emit(s, "    const double v%d = xs[TIDX(%d)];\n", i, a[i]); break;
      case OP_P: emit(s, "    const double v%d = pb[%d];\n", i, a[i]); break;
      case OP_ADD: emit(s, "    const double v%d = v%d + v%d;\n", i, a[i], bb[i]); break;
      case OP_SUB: emit(s, "    const double v%d = v%d - v%d;\n", i, a[i], bb[i]); break;
      case OP_MUL: emit(s, "    const double v%d = v%d * v%d;\n", i, a[i], bb[i]); break;
      case OP_DIV: emit(s, "    const double v%d = v%d / v%d;\n", i, a[i], bb[i]); break;
      case OP_NEG: emit(s, "    const double v%d = -v%d;\n", i, a[i]); break;
      case OP_SIN: emit(s, "    const double v%d = sin(v%d);\n", i, a[i]); break;
      case OP_COS: emit(s, "    const double v%d = cos(v%d);\n", i, a[i]); break;
      case OP_ATAN2: emit(s, "    const double v%d = atan2(v%d, v%d);\n", i, a[i], bb[i]); break;
      case OP_SQRT: emit(s, "    const double v%d = sqrt(v%d);\n", i, a[i]); break;
      case OP_SQR: emit(s, "    const double v%d = v%d * v%d;\n", i, a[i], a[i]); break;
      case OP_ASIN: emit(s, "    const double v%d = asin(v%d);\n", i, a[i]); break;
      case OP_FABS: emit(s, "    const double v%d = fabs(v%d);\n", i, a[i]); break;
      case OP_FMIN: emit(s, "    const double v%d = fmin(v%d, v%d);\n", i, a[i], bb[i]); break;
      case OP_FMAX: emit(s, "    const double v%d = fmax(v%d, v%d);\n", i, a[i], bb[i]); break;
      case OP_LT: emit(s, "    const double v%d = v%d < v%d ? 1.0 : 0.0;\n", i, a[i], bb[i]); break;
      case OP_LE: emit(s, "    const double v%d = v%d <= v%d ? 1.0 : 0.0;\n", i, a[i], bb[i]); break;
      case OP_EQ: emit(s, "    const double v%d = v%d == v%d ? 1.0 : 0.0;\n", i, a[i], bb[i]); break;
      case OP_NE: emit(s, "    const double v%d = v%d != v%d ? 1.0 : 0.0;\n", i, a[i], bb[i]); break;
      case OP_NOT: emit(s, "    const double v%d = v%d == 0.0 ? 1.0 : 0.0;\n", i, a[i]); break;
      case OP_AND: emit(s, "    const double v%d = (v%d != 0.0 && v%d != 0.0) ? 1.0 : 0.0;\n", i, a[i], bb[i]); break;
      case OP_OR: emit(s, "    const double v%d = (v%d != 0.0 || v%d != 0.0) ? 1.0 : 0.0;\n", i, a[i], bb[i]); break;
      case OP_IFZ: emit(s, "    const double v%d = v%d != 0.0 ? v%d : 0.0;\n", i, a[i], bb[i]); break;
      case OP_EXP: emit(s, "    const double v%d = exp(v%d);\n", i, a[i]); break;
      case OP_LOG: emit(s, "    const double v%d = log(v%d);\n", i, a[i]); break;
    }
  }
  for (int i = 0; i < T.len; ++i)
    if (live[i] && tape_op_has_adjoint(op[i])) emit(s, "    double a%d = 0.0;\n", i);
  for (int k = 0; k < T.nx; ++k) emit(s, "    double g%d = 0.0;\n", k);
  emit(s, "    double val = v%d, cm = 0.0, ms = 0.0;\n", T.out_cost);
  auto has_adj = [&](int i) { return tape_op_has_adjoint(op[i]); };
  if (has_adj(T.out_cost)) emit(s, "    a%d = 1.0;\n", T.out_cost);
  for (int i = 0; i < T.n_ineq; ++i) {
    const int r = rows[i];
    emit(s, "    { const double w = tape_al_ineq(v%d, W.lam[TIDX(%d)], rho, val, cm, ms); W.rowv[TIDX(%d)] = v%d;", r, i, i, r);
    if (has_adj(r)) emit(s, " a%d += w;", r);
    s += " }\n";
  }
  for (int i = 0; i < T.n_eq; ++i) {
    const int r = rows[T.n_ineq + i];
    emit(s, "    { const double w = tape_al_eq(v%d, W.mu[TIDX(%d)], rho, val, cm, ms); W.rowv[TIDX(%d)] = v%d;", r, i, T.n_ineq + i, r);
    if (has_adj(r)) emit(s, " a%d += w;", r);
    s += " }\n";
  }
  // adjoint table: the text of tape_adjoint's rules
  for (int i = T.len - 1; i >= 0; --i) {
    if (!live[i]) continue;
    const int ia = a[i], ib = bb[i];
    const bool da = tape_op_arity(op[i]) >= 1 && has_adj(ia), db = tape_op_arity(op[i]) == 2 && has_adj(ib);
    switch (op[i]) {
      case OP_CONST: case OP_P: break;
      case OP_X: emit(s, "    g%d += a%d;\n", ia, i); break;
      case OP_ADD:
        if (da) emit(s, "    a%d += a%d;\n", ia, i);
        if (db) emit(s, "    a%d += a%d;\n", ib, i);
        break;
      case OP_SUB:
        if (da) emit(s, "    a%d += a%d;\n", ia, i);
        if (db) emit(s, "    a%d -= a%d;\n", ib, i);
        break;
      case OP_MUL:
        if (da) emit(s, "    a%d += a%d * v%d;\n", ia, i, ib);
        if (db) emit(s, "    a%d += a%d * v%d;\n", ib, i, ia);
        break;
      case OP_DIV:
        if (da) emit(s, "    a%d += a%d / v%d;\n", ia, i, ib);
        if (db) emit(s, "    a%d -= a%d * v%d / (v%d * v%d);\n", ib, i, ia, ib, ib);
        break;
      case OP_NEG:
        if (da) emit(s, "    a%d -= a%d;\n", ia, i);
        break;
      case OP_SIN:
        if (da) emit(s, "    a%d += a%d * cos(v%d);\n", ia, i, ia);
        break;
      case OP_COS:
        if (da) emit(s, "    a%d -= a%d * sin(v%d);\n", ia, i, ia);
        break;
      case OP_ATAN2:
        emit(s, "    { const double d = v%d * v%d + v%d * v%d;", ia, ia, ib, ib);
        if (da) emit(s, " a%d += a%d * v%d / d;", ia, i, ib);
        if (db) emit(s, " a%d -= a%d * v%d / d;", ib, i, ia);
        s += " }\n";
        break;
      case OP_SQRT:
        if (da) emit(s, "    a%d += a%d * 0.5 / v%d;\n", ia, i, i);
        break;
      case OP_SQR:
        if (da) emit(s, "    a%d += a%d * 2.0 * v%d;\n", ia, i, ia);
        break;
      case OP_ASIN:
        if (da) emit(s, "    a%d += a%d / sqrt((1.0 - v%d) * (1.0 + v%d));\n", ia, i, ia, ia);
        break;
      case OP_FABS:
        if (da) emit(s, "    a%d += a%d * (v%d > 0.0 ? 1.0 : (v%d < 0.0 ? -1.0 : 0.0));\n", ia, i, ia, ia);
        break;
      case OP_FMIN:
      case OP_FMAX: {
        const char* cmp = op[i] == OP_FMIN ? "<=" : ">=";
        if (da && db) emit(s, "    if (v%d %s v%d) a%d += a%d; else a%d += a%d;\n", ia, cmp, ib, ia, i, ib, i);
        else if (da) emit(s, "    if (v%d %s v%d) a%d += a%d;\n", ia, cmp, ib, ia, i);
        else if (db) emit(s, "    if (!(v%d %s v%d)) a%d += a%d;\n", ia, cmp, ib, ib, i);
      } break;
      case OP_IFZ:
        if (db) emit(s, "    if (v%d != 0.0) a%d += a%d;\n", ia, ib, i);
        break;
      case OP_EXP:
        if (da) emit(s, "    a%d += a%d * v%d;\n", ia, i, i);
        break;
      case OP_LOG:
        if (da) emit(s, "    a%d += a%d / v%d;\n", ia, i, ia);
        break;
      default:  // LT .. OR: comparisons and logic are piecewise constant
        break;
    }
  }
  for (int k = 0; k < T.nx; ++k) emit(s, "    gout[TIDX(%d)] = g%d;\n", k, k);
  emit(s, "    *fout = v%d; *cmax = cm; *meas = ms;\n    return val;\n  }\n};\n", T.out_cost);
  if (!solve) {
    s += "extern \"C\" __global__ __launch_bounds__(64) void k_tape_jit_phi(TapeParams T, int B, int Bp, const double* __restrict__ x, const double* __restrict__ par,\n"
         "    const double* __restrict__ lam, const double* __restrict__ mu, double rho, double* __restrict__ work, double* __restrict__ merit, double* __restrict__ fo,\n"
         "    double* __restrict__ rows, double* __restrict__ grad, double* __restrict__ cmax, double* __restrict__ meas) {\n"
         "  const int b = blockIdx.x * blockDim.x + threadIdx.x;\n  if (b >= B) return;\n"
         "  const TapeWork W = tape_carve(T, work, Bp);\n  JitEval ev{W, par + (size_t)b * T.np, Bp, b};\n"
         "  tape_phi_instance(T, ev, W, Bp, b, b, x, lam, mu, rho, merit, fo, rows, grad, cmax, meas);\n}\n";
    s += "extern \"C\" __global__ __launch_bounds__(64) void k_tape_jit_phi_lds(TapeParams T, int B, int Bp_unused, const double* __restrict__ x, const double* __restrict__ par,\n"
         "    const double* __restrict__ lam, const double* __restrict__ mu, double rho, double* __restrict__ work_unused, double* __restrict__ merit, double* __restrict__ fo,\n"
         "    double* __restrict__ rows, double* __restrict__ grad, double* __restrict__ cmax, double* __restrict__ meas) {\n"
         "  extern __shared__ double tape_lds[];\n"
         "  const int gb = blockIdx.x * blockDim.x + threadIdx.x;\n  if (gb >= B) return;\n"
         "  const int Bp = blockDim.x, b = threadIdx.x;\n"
         "  const TapeWork W = tape_carve(T, tape_lds, Bp);\n  JitEval ev{W, par + (size_t)gb * T.np, Bp, b};\n"
         "  tape_phi_instance(T, ev, W, Bp, b, gb, x, lam, mu, rho, merit, fo, rows, grad, cmax, meas);\n}\n";
    return s;
  }
  s += "extern \"C\" __global__ __launch_bounds__(64) void k_tape_jit(TapeParams T, int B, int Bp, const double* __restrict__ x0, const double* __restrict__ par,\n"
       "    double* __restrict__ work, double* __restrict__ xo, double* __restrict__ fo, double* __restrict__ kkt, int* __restrict__ iters,\n"
       "    int* __restrict__ status, double* __restrict__ mult) {\n"
       "  const int b = blockIdx.x * blockDim.x + threadIdx.x;\n  if (b >= B) return;\n"
       "  const TapeWork W = tape_carve(T, work, Bp);\n  JitEval ev{W, par + (size_t)b * T.np, Bp, b};\n"
       "  tape_solve_instance(T, ev, W, Bp, b, b, x0, xo, fo, kkt, iters, status, mult);\n}\n";
  // the same with the solver's work arrays (x, gradients, the BFGS matrix, multipliers, rows) in LDS, [row][lane of the block]: for small
  // batches every access of the quasi-Newton loop is otherwise a dependent round trip to the global buffer
  s += "extern \"C\" __global__ __launch_bounds__(64) void k_tape_jit_lds(TapeParams T, int B, int Bp_unused, const double* __restrict__ x0, const double* __restrict__ par,\n"
       "    double* __restrict__ work_unused, double* __restrict__ xo, double* __restrict__ fo, double* __restrict__ kkt, int* __restrict__ iters,\n"
       "    int* __restrict__ status, double* __restrict__ mult) {\n"
       "  extern __shared__ double tape_lds[];\n"
       "  const int gb = blockIdx.x * blockDim.x + threadIdx.x;\n  if (gb >= B) return;\n"
       "  const int Bp = blockDim.x, b = threadIdx.x;\n"
       "  const TapeWork W = tape_carve(T, tape_lds, Bp);\n  JitEval ev{W, par + (size_t)gb * T.np, Bp, b};\n"
       "  tape_solve_instance(T, ev, W, Bp, b, gb, x0, xo, fo, kkt, iters, status, mult);\n}\n";
  return s;
}

std::mutex g_cache_mutex;
std::unordered_map<std::string, std::vector<char>> g_code_cache;  // generated source -> code object (same problem built again: no recompile)

}  // namespace

size_t oh_tape_work_rows(const TapeParams& T, bool jit) { return tape_solver_rows(T) + (jit ? 0 : 2 * (size_t)T.len); }

void oh_launch_tape_solve(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int B, int Bp,
                          const double* x0, const double* p, double* work, double* x, double* f, double* kkt, int* iters, int* status, double* mult) {
  TapeView tv{op, a, b, c, rows};
  hipLaunchKernelGGL(k_tape_solve, dim3((B + 63) / 64), dim3(64), 0, s, T, tv, B, Bp, x0, p, work, x, f, kkt, iters, status, mult);
}

size_t oh_tape_newton_work_rows(const TapeParams& T) { return 4 * (size_t)T.len + tape_newton_rows(T); }

void oh_launch_tape_solve_newton(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int B, int Bp,
                                 int cg_cap, const double* x0, const double* p, double* work, double* x, double* f, double* kkt, int* iters, int* status,
                                 double* mult, int* stats) {
  TapeView tv{op, a, b, c, rows};
  hipLaunchKernelGGL(k_tape_solve_newton, dim3((B + 63) / 64), dim3(64), 0, s, T, tv, B, Bp, cg_cap, x0, p, work, x, f, kkt, iters, status, mult, stats);
}

void oh_launch_tape_phi_hvp(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int B, int Bp,
                            const double* x, const double* p, const double* lam, const double* mu, double rho, int nv, const double* V, double* work,
                            double* HV, double* grad) {
  TapeView tv{op, a, b, c, rows};
  hipLaunchKernelGGL(k_tape_phi_hvp, dim3((B + 63) / 64), dim3(64), 0, s, T, tv, B, Bp, x, p, lam, mu, rho, nv, V, work, HV, grad);
}

void oh_launch_tape_probe(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int B, int Bp,
                          const double* x, const double* p, double* work, int n_regs, const int* regs, double* val, const double* seeds, double* adj, double* grad) {
  TapeView tv{op, a, b, c, rows};
  hipLaunchKernelGGL(k_tape_probe, dim3((B + 63) / 64), dim3(64), 0, s, T, tv, B, Bp, x, p, work, n_regs, regs, val, seeds, adj, grad);
}

size_t oh_tape_hvp_work_rows(const TapeParams& T) { return 4 * (size_t)T.len + 3 * (size_t)T.nx; }

void oh_launch_tape_hvp(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int u0, int n, int Bp,
                        int nv, const double* x, const double* p, const double* seeds, const double* V, double* work, double* HV, double* grad) {
  TapeView tv{op, a, b, c, rows};
  hipLaunchKernelGGL(k_tape_hvp, dim3((n + 63) / 64), dim3(64), 0, s, T, tv, u0, n, Bp, nv, x, p, seeds, V, work, HV, grad);
}

void oh_launch_tape_phi(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int B, int Bp,
                        const double* x, const double* p, const double* lam, const double* mu, double rho, double* work, double* merit, double* f, double* rowv,
                        double* grad, double* cmax, double* meas) {
  TapeView tv{op, a, b, c, rows};
  hipLaunchKernelGGL(k_tape_phi, dim3((B + 63) / 64), dim3(64), 0, s, T, tv, B, Bp, x, p, lam, mu, rho, work, merit, f, rowv, grad, cmax, meas);
}

std::string oh_tape_jit_source(const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, const bool solve) {
  return generate(T, op, a, b, c, rows, solve);
}

int oh_tape_jit_compile(const std::string& src, std::vector<char>* code, std::string* err) {
  {
    std::lock_guard<std::mutex> lk(g_cache_mutex);
    auto it = g_code_cache.find(src);
    if (it != g_code_cache.end()) { *code = it->second; return 0; }
  }
  // a trajectory-sized tape is minutes of compilation: its object is kept on disk like the chain-specialised kernels' (the key is the
  // generated text, which contains the solver and every constant of the problem)
  // (the disk key is the generated text plus the compile options below: an object built with other options is another object)
  static const std::string kOptKey = "// --offload-arch=gfx950 -O3 -std=c++17\n";
  if (src.size() > 100000 && oh_jit_disk_lookup(kOptKey + src, "tape", code)) {
    std::lock_guard<std::mutex> lk(g_cache_mutex);
    g_code_cache.emplace(src, *code);
    return 0;
  }
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), "oh_tape_jit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) { *err = "hiprtcCreateProgram failed"; return 1; }
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
  const hiprtcResult r = hiprtcCompileProgram(prog, 3, opts);
  if (r != HIPRTC_SUCCESS) {
    size_t ls = 0;
    hiprtcGetProgramLogSize(prog, &ls);
    std::string log(ls, '\0');
    if (ls > 1) hiprtcGetProgramLog(prog, log.data());
    *err = std::string("hiprtc: ") + hiprtcGetErrorString(r) + ": " + log.substr(0, 1500);
    hiprtcDestroyProgram(&prog);
    return 1;
  }
  size_t cs = 0;
  hiprtcGetCodeSize(prog, &cs);
  code->resize(cs);
  hiprtcGetCode(prog, code->data());
  hiprtcDestroyProgram(&prog);
  if (src.size() > 100000) oh_jit_disk_store(kOptKey + src, "tape", *code);
  std::lock_guard<std::mutex> lk(g_cache_mutex);
  g_code_cache.emplace(src, *code);
  return 0;
}

// Forget a code object that did not load (a truncated or stale file of the disk cache): the next oh_tape_jit_compile of the same source recompiles.
void oh_tape_jit_forget(const std::string& src) {
  oh_jit_disk_drop(std::string("// --offload-arch=gfx950 -O3 -std=c++17\n") + src, "tape");
  std::lock_guard<std::mutex> lk(g_cache_mutex);
  g_code_cache.erase(src);
}

int oh_tape_jit_load(const std::vector<char>& code, TapeJit* out, std::string* err, const bool solve) {
  const char* name = solve ? "k_tape_jit" : "k_tape_jit_phi";
  const char* name_lds = solve ? "k_tape_jit_lds" : "k_tape_jit_phi_lds";
  if (hipModuleLoadData(&out->mod, code.data()) != hipSuccess) {
    (void)hipGetLastError();
    *err = "hipModuleLoadData failed for the generated tape kernel";
    return 1;
  }
  if (hipModuleGetFunction(&out->fn, out->mod, name) != hipSuccess) {
    hipModuleUnload(out->mod);
    out->mod = nullptr;
    *err = std::string("hipModuleGetFunction(") + name + ") failed";
    return 1;
  }
  if (hipModuleGetFunction(&out->fn_lds, out->mod, name_lds) != hipSuccess) out->fn_lds = nullptr;
  return 0;
}

void oh_tape_jit_release(TapeJit* j) {
  if (j->mod) hipModuleUnload(j->mod);
  j->mod = nullptr;
  j->fn = nullptr;
  j->fn_lds = nullptr;
}

// the launch of either program of a generated evaluator (solve kernels / single-evaluation kernels): the same choice of entry and block size
static hipError_t launch_jit(hipStream_t s, const TapeJit& j, const TapeParams& T, int B, void** args, int lds_max);

hipError_t oh_launch_tape_jit_phi(hipStream_t s, const TapeJit& j, TapeParams T, int B, int Bp, const double* x, const double* p, const double* lam, const double* mu,
                                  double rho, double* work, double* merit, double* f, double* rowv, double* grad, double* cmax, double* meas, const int lds_max,
                                  int* used_lds) {
  void* args[] = {&T, &B, &Bp, &x, &p, &lam, &mu, &rho, &work, &merit, &f, &rowv, &grad, &cmax, &meas};
  if (used_lds) *used_lds = (j.fn_lds && B <= lds_max && sizeof(double) * tape_solver_rows(T) * 16 <= 48 * 1024) ? 1 : 0;
  return launch_jit(s, j, T, B, args, lds_max);
}

hipError_t oh_launch_tape_jit(hipStream_t s, const TapeJit& j, TapeParams T, int B, int Bp, const double* x0, const double* p, double* work, double* x, double* f,
                              double* kkt, int* iters, int* status, double* mult, const int lds_max) {
  void* args[] = {&T, &B, &Bp, &x0, &p, &work, &x, &f, &kkt, &iters, &status, &mult};
  return launch_jit(s, j, T, B, args, lds_max);
}

static hipError_t launch_jit(hipStream_t s, const TapeJit& j, const TapeParams& T, int B, void** args, const int lds_max) {
  // the solver's work set in LDS when it fits 48 KB at 64, 32 or 16 instances per block (tools/gpu_tape_sweep.py, the 7-joint IK problem: one
  // instance 5.0 -> 3.4 ms, 2048 14.3 -> 10.9 ms, 32 768 25.8 -> 21.0 ms; lds_max: option tape_lds_max, 0 switches it off)
  // (round 2: level above 32 768 instances -- 65 536: 30.2 / 33.5 ms, 131 072: 47.5 / 44.9 ms global / LDS; with the solver of round 3's end, which
  // spends 65 evaluations instead of 266 on the median instance, the LDS set wins at every size: 65 536: 9.8 / 7.7 ms, 131 072: 17.5 / 13.2 ms)
  if (j.fn_lds && B <= lds_max) {
    const size_t per = sizeof(double) * tape_solver_rows(T);
    for (int bs : {64, 32, 16})
      if (per * bs <= 48 * 1024) return hipModuleLaunchKernel(j.fn_lds, (B + bs - 1) / bs, 1, 1, bs, 1, 1, (unsigned)(per * bs), s, args, nullptr);
  }
  return hipModuleLaunchKernel(j.fn, (B + 63) / 64, 1, 1, 64, 1, 1, 0, s, args, nullptr);
}
