// Small dense QP family (the QuadraticCost* classes the reference hands to OSQP / CVXOPT / qpOASES,
// solver.py:421-584; its own known-answer solver test, tests/test_solver.py:22-54, is one of them):
//
//     min_x  x^T P x + q^T x      s.t.  M x + c >= 0,   A x + b = 0           (optimization.py:219-260: no factor 1/2)
//
// Infeasible-start primal-dual interior point with slacks s = Mx + c, Newton system reduced to H = P + P^T + M^T (lam/s) M (dense Cholesky,
// n <= 32, m <= 256, me <= 32; larger handles, up to OH_QP_MAX_N / _M / _ME, are solved by one workgroup per instance: oh_qp_block.hip) and the
// Schur complement A H^{-1} A^T for the equality rows.  The iteration is written ONCE, qp_ipm, over a team: the lanes that own one instance.
//   QpThread  one thread per instance (k_qp_solve<0|1|2>: work set in the global buffer, in LDS, in LDS together with the instance's row)
//   QpWave    one wavefront per instance, everything in LDS (k_qp_solve_wave: a few instances; a controller's tick is one)
// The four kernels decide where the row and the work set lie and call it.  The scalar rules are those of oh_qp_rules.h, the layouts those of
// oh_qp_layout.h.  The matrices differ per instance (P, M, A may depend on the parameters: the Booth test has a * y in its cost), so every
// instance brings its own [P | q | M | c | A | b] row.  numpy restatement of the same iteration: oracle/qp_ipm.py.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <string>

#include "oh_device.h"
#include "oh_kernels.h"
#include "oh_qp_layout.h"
#include "oh_qp_rules.h"

namespace {

// A work array of one instance: element k lives at p[k * stride].  The instance's slices sit either in LDS ([k][lane], when the whole work set of
// a block fits: the iteration is a chain of dependent accesses, and from global memory every one of them is a round trip -- 2 ms per solve at
// B = 1) or in the global work buffer ([k][instance]: the lanes of a wavefront touch one line per access).
struct QArr {
  double* p;
  int stride;
  __device__ double& operator[](const int i) const { return p[(size_t)i * stride]; }
  __device__ QArr operator+(const size_t off) const { return QArr{p + off * stride, stride}; }
};

// The lanes that own one instance.  Loops over rows, columns and entries run `for (i = lane; i < count; i += step)`: every entry has ONE owner,
// which accumulates its dot product in ascending index -- the same arithmetic whatever the team.  A team says how its lanes agree (sync, the
// reductions, all / any), who does the short serial parts (leader) and how the lower triangle of H and its rows are dealt (lower).
struct QpThread {
  static constexpr int lane = 0, step = 1;
  // Nothing: the threads of a k_qp_solve block own different instances, return early (b >= B) and leave the iteration at different counts, so
  // there must be NO barrier on this team's path.
  __device__ static void sync() {}
  __device__ static double max(const double v) { return v; }
  __device__ static double min(const double v) { return v; }
  __device__ static double sum(const double v) { return v; }
  __device__ static bool all(const bool p) { return p; }
  __device__ static bool any(const bool p) { return p; }
  __device__ static bool leader() { return true; }
  template <class F, class G>
  __device__ static void lower(const int n, F entry, G row) {  // entry(i, j) for j <= i < n; row(i) right after row i (its column of M is at hand)
    for (int i = 0; i < n; ++i) {
      for (int j = 0; j <= i; ++j) entry(i, j);
      row(i);
    }
  }
};
// The block IS the wavefront (64 threads): the barrier orders the LDS traffic of its lanes.  Every exit of the iteration is taken from a value
// all 64 lanes hold (after a reduction, all(), or read from the same LDS word after a barrier), so every lane meets every barrier.
struct QpWave {
  const int lane;
  static constexpr int step = 64;
  __device__ static void sync() { __syncthreads(); }
  __device__ static double max(const double v) { return wave64_max(v); }
  __device__ static double min(const double v) { return wave64_min(v); }
  __device__ static double sum(const double v) { return wave64_sum(v); }  // per-lane partial sums, then the ladder: equal to the thread's sum to rounding
  __device__ static bool all(const bool p) { return __all(p); }
  __device__ static bool any(const bool p) { return __any(p); }
  __device__ bool leader() const { return lane == 0; }
  template <class F, class G>
  __device__ void lower(const int n, F entry, G row) const {  // entry e = i (i + 1) / 2 + j by lane e % 64, then row i by lane i % 64
    for (int e = lane; e < n * (n + 1) / 2; e += 64) {
      int i = 0, r = e;
      while (r > i) { r -= i + 1; ++i; }
      entry(i, r);
    }
    for (int i = lane; i < n; i += 64) row(i);
  }
};

// in-place left-looking Cholesky of the n x n row-major SPD matrix H (lower triangle): the pivot of column j by every lane alike, the rows below
// it dealt over the team; returns false (on every lane) on a non-positive pivot
template <class Team>
__device__ __forceinline__ bool qp_chol(const Team team, const QArr H, const int n) {
  for (int j = 0; j < n; ++j) {
    double d = H[j * n + j];
    for (int k = 0; k < j; ++k) d -= H[j * n + k] * H[j * n + k];
    if (!(d > 0.0)) return false;
    const double l = sqrt(d);
    for (int i = j + 1 + team.lane; i < n; i += team.step) {  // (column j is read by its owners only: written in place)
      double v = H[i * n + j];
      for (int k = 0; k < j; ++k) v -= H[i * n + k] * H[j * n + k];
      H[i * n + j] = v / l;
    }
    team.sync();  // every lane has read the pivot
    if (team.leader()) H[j * n + j] = l;
    team.sync();
  }
  return true;
}
__device__ void qp_solve_chol(const QArr L, const int n, const QArr x) {  // x <- (L L^T)^{-1} x, by one lane
  for (int i = 0; i < n; ++i) {
    double v = x[i];
    for (int k = 0; k < i; ++k) v -= L[i * n + k] * x[k];
    x[i] = v / L[i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double v = x[i];
    for (int k = i + 1; k < n; ++k) v -= L[k * n + i] * x[k];
    x[i] = v / L[i * n + i];
  }
}

// The iteration on instance b: `row` holds its [P | q | M | c | A | b] (read only), `work` its work set.
template <class Team>
__device__ __forceinline__ void qp_ipm(const Team team, const QpParams& Q, const int b, const QArr row, const QArr work, const double* __restrict__ x0,
                                       double* __restrict__ xo, double* __restrict__ fo, double* __restrict__ kkt, int* __restrict__ iters,
                                       int* __restrict__ status, double* __restrict__ mult) {
  const int n = Q.n, m = Q.m, me = Q.me, lane = team.lane, step = team.step;
  const QpRow<QArr> R = qp_row(row, n, m, me);
  const QpWork<QArr> W = qp_work(work, n, m, me);
  const QArr P = R.P, q = R.q, M = R.M, c = R.c, A = R.A, bv = R.b;
  const QArr x = W.x, s = W.s, lam = W.lam, nu = W.nu, H = W.H, rhs = W.rhs, dx = W.dx, ds = W.ds, dl = W.dl, Y = W.Y, S = W.S, dnu = W.dnu, rd = W.rd;
  for (int i = lane; i < n; i += step) x[i] = x0[(size_t)b * n + i];
  for (int i = lane; i < me; i += step) nu[i] = 0.0;
  team.sync();
  double mu = 1.0;
  for (int i = lane; i < m; i += step) {
    double v = c[i];
    for (int j = 0; j < n; ++j) v += M[i * n + j] * x[j];
    s[i] = qp_rules::initial_slack(v);
    lam[i] = qp_rules::initial_multiplier(mu, s[i]);
  }
  team.sync();
  int st = OH_STATUS_MAX_ITER, it = 0;
  double stat = 0.0, feas = 0.0, gap = 0.0;
  for (; it <= Q.max_iter; ++it) {
    // residuals
    stat = 0.0; feas = 0.0; gap = 0.0;
    bool finite = true;
    for (int i = lane; i < n; i += step) {
      double v = q[i];
      for (int j = 0; j < n; ++j) v += (P[i * n + j] + P[j * n + i]) * x[j];  // gradient of x^T P x: P need not be symmetric
      for (int k = 0; k < m; ++k) v -= M[k * n + i] * lam[k];
      for (int k = 0; k < me; ++k) v -= A[k * n + i] * nu[k];
      rd[i] = v;
      stat = fmax(stat, fabs(v));
      finite = finite && qp_rules::finite(v);
    }
    for (int i = lane; i < m; i += step) {
      double v = c[i] - s[i];
      for (int j = 0; j < n; ++j) v += M[i * n + j] * x[j];
      ds[i] = v;  // r_p
      feas = fmax(feas, fabs(v));
      gap = fmax(gap, s[i] * lam[i]);
      dl[i] = lam[i] / s[i];  // (dl is free until the step: one division per row instead of one per use)
    }
    for (int i = lane; i < me; i += step) {
      double v = bv[i];
      for (int j = 0; j < n; ++j) v += A[i * n + j] * x[j];
      dnu[i] = v;  // r_e
      feas = fmax(feas, fabs(v));
    }
    finite = team.all(finite);
    const bool feas_nan = team.any(!(feas == feas));
    stat = team.max(stat);
    feas = team.max(feas);
    gap = team.max(gap);
    team.sync();
    if (!finite || feas_nan) { st = OH_STATUS_NUMERICAL; break; }
    if (qp_rules::converged(stat, feas, gap, Q.tol)) { st = OH_STATUS_CONVERGED; break; }
    if (it == Q.max_iter) break;
    // H = P + P^T + M^T diag(lam/s) M (+ tiny shift), rhs = -rd + M^T [(mu/s - lam) - (lam/s) r_p]
    auto entry = [&](const int i, const int j) {
      double v = P[i * n + j] + P[j * n + i];
      for (int k = 0; k < m; ++k) v += M[k * n + i] * dl[k] * M[k * n + j];
      H[i * n + j] = v;
    };
    team.lower(n, entry, [&](const int i) {
      double r = -rd[i];
      for (int k = 0; k < m; ++k) r += M[k * n + i] * ((mu / s[k] - lam[k]) - dl[k] * ds[k]);
      rhs[i] = r;
    });
    team.sync();
    double dmax = 0.0;
    for (int i = 0; i < n; ++i) dmax = fmax(dmax, fabs(H[i * n + i]));
    double shift = qp_rules::first_shift(dmax);
    bool ok = false;
    for (int attempt = 0; attempt < qp_rules::SHIFT_ATTEMPTS && !ok; ++attempt) {
      if (attempt > 0) {  // rebuild with a larger shift (singular P without enough active rows)
        team.sync();
        team.lower(n, entry, [](const int) {});
        shift *= qp_rules::SHIFT_GROWTH;
        team.sync();
      }
      for (int i = lane; i < n; i += step) H[i * n + i] += shift;
      team.sync();
      ok = qp_chol(team, H, n);
    }
    if (!ok) { st = OH_STATUS_NUMERICAL; break; }
    // the substitution for dx and the factor of S are short and serial: the leader's
    for (int i = lane; i < n; i += step) dx[i] = rhs[i];
    team.sync();
    if (team.leader()) qp_solve_chol(H, n, dx);  // H^{-1} rhs
    team.sync();
    if (me > 0) {
      // A dx = -r_e with dx = H^{-1}(rhs + A^T dnu):  (A H^{-1} A^T) dnu = -r_e - A H^{-1} rhs
      for (int i = lane; i < me; i += step) {  // row i of Y = H^{-1} A_i
        for (int j = 0; j < n; ++j) Y[i * n + j] = A[i * n + j];
        qp_solve_chol(H, n, Y + (size_t)(i * n));
      }
      team.sync();
      for (int i = lane; i < me; i += step) {
        double r = -dnu[i];
        for (int j = 0; j < n; ++j) r -= A[i * n + j] * dx[j];
        for (int k = 0; k <= i; ++k) {
          double v = 0.0;
          for (int j = 0; j < n; ++j) v += A[i * n + j] * Y[k * n + j];
          S[i * me + k] = v;
        }
        S[i * me + i] += qp_rules::schur_regularisation(S[i * me + i]);
        dnu[i] = r;
      }
      team.sync();
      bool oks = true;
      if (team.leader()) {
        oks = qp_chol(QpThread{}, S, me);
        if (oks) {
          qp_solve_chol(S, me, dnu);
          for (int i = 0; i < me; ++i)
            for (int j = 0; j < n; ++j) dx[j] += Y[i * n + j] * dnu[i];
        }
      }
      oks = team.all(oks);
      team.sync();
      if (!oks) { st = OH_STATUS_NUMERICAL; break; }
    }
    // ds = M dx + r_p ; dlam = (mu/s - lam) - (lam/s) ds ; fraction to the boundary
    double ap = 1.0, ad = 1.0;
    for (int i = lane; i < m; i += step) {
      double v = ds[i];
      for (int j = 0; j < n; ++j) v += M[i * n + j] * dx[j];
      const double d2 = (mu / s[i] - lam[i]) - dl[i] * v;
      ds[i] = v;
      dl[i] = d2;
      if (v < 0.0) ap = fmin(ap, qp_rules::boundary_step(s[i], v));
      if (d2 < 0.0) ad = fmin(ad, qp_rules::boundary_step(lam[i], d2));
    }
    ap = team.min(ap);
    ad = team.min(ad);
    for (int i = lane; i < n; i += step) x[i] += ap * dx[i];
    double comp = 0.0;
    for (int i = lane; i < m; i += step) {
      s[i] += ap * ds[i];
      lam[i] += ad * dl[i];
      comp += s[i] * lam[i];
    }
    comp = team.sum(comp);
    for (int i = lane; i < me; i += step) nu[i] += ad * dnu[i];
    if (m > 0) mu = qp_rules::next_mu(ap, ad, comp, m, Q.tol);
    team.sync();
  }
  double fval = 0.0;
  for (int i = lane; i < n; i += step) {
    double v = q[i];
    for (int j = 0; j < n; ++j) v += P[i * n + j] * x[j];
    fval += v * x[i];
    if (xo) xo[(size_t)b * n + i] = x[i];
  }
  fval = team.sum(fval);
  if (team.leader()) {
    if (fo) fo[b] = fval;
    if (kkt) { kkt[3 * (size_t)b] = stat; kkt[3 * (size_t)b + 1] = feas; kkt[3 * (size_t)b + 2] = gap; }
    if (iters) iters[b] = it;
    if (status) status[b] = st;
  }
  if (mult) {
    for (int i = lane; i < m; i += step) mult[(size_t)b * (m + me) + i] = lam[i];
    for (int i = lane; i < me; i += step) mult[(size_t)b * (m + me) + m + i] = nu[i];
  }
}

// One thread per instance.  MODE 0: work set in the global buffer [k][Bp]; 1: in LDS [k][lane]; 2: in LDS together with the instance's row
template <int MODE>
__global__ __launch_bounds__(64) void k_qp_solve(QpParams Q, int B, int Bp, const double* __restrict__ x0, const double* __restrict__ par, double* __restrict__ work,
                                                 double* __restrict__ xo, double* __restrict__ fo, double* __restrict__ kkt, int* __restrict__ iters,
                                                 int* __restrict__ status, double* __restrict__ mult) {
  extern __shared__ double qp_sm[];
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  QArr w = MODE ? QArr{qp_sm + threadIdx.x, (int)blockDim.x} : QArr{work + b, Bp};
  // (the row is read-only; const_cast only to share the accessor type)
  QArr row{const_cast<double*>(par) + (size_t)b * Q.np, 1};
  if (MODE == 2) {
    for (int k = 0; k < Q.np; ++k) w[k] = row[k];
    row = w;
    w = w + (size_t)Q.np;
  }
  qp_ipm(QpThread{}, Q, b, row, w, x0, xo, fo, kkt, iters, status, mult);
}

// One wavefront per instance, row and work set in LDS [k].  One thread per instance is a chain of ~3000 dependent LDS accesses per iteration
// (80 us); here an iteration is a few hundred.
__global__ __launch_bounds__(64) void k_qp_solve_wave(QpParams Q, int B, const double* __restrict__ x0, const double* __restrict__ par, double* __restrict__ xo,
                                                      double* __restrict__ fo, double* __restrict__ kkt, int* __restrict__ iters, int* __restrict__ status,
                                                      double* __restrict__ mult) {
  extern __shared__ double qp_sm[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const QArr row{qp_sm, 1};
  for (int k = lane; k < Q.np; k += 64) row[k] = par[(size_t)b * Q.np + k];  // (qp_ipm's first barrier stands before the first read of it)
  qp_ipm(QpWave{lane}, Q, b, row, row + (size_t)Q.np, x0, xo, fo, kkt, iters, status, mult);
}

// ---- QP data read off the problem's instruction tape on the device (oh_qp_set_tape) -----------------------------------------------------
// The reference's QuadraticCost* classes hold P, q, M, c, A, b as cs.Functions of the parameters (optimization.py:219-260); the mirror reads
// them off f, k, a by probing on the host (optas_amd/optimization.py: values at 0, +-e_i, e_i + e_j -- exact for a quadratic cost and affine
// rows), 36 tree evaluations per instance for n = 7: 1.8 ms.  Here one thread per instance runs the same probes through the problem's
// instruction tape (optas_amd/tape.py; the interpreter of oh_tape.hip, forward sweep only, registers val[i][b] in a global work array) and
// leaves the [P | q | M | c | A | b] row k_qp_solve reads, plus the cost's constant term f(0, p).  Same formulas in the same order as the host.
struct QpTape {
  int len, out_cost;
  const int* __restrict__ op;
  const int* __restrict__ a;
  const int* __restrict__ bb;
  const double* __restrict__ c;
  const int* __restrict__ rows;
  int n_xdep;                     // instructions whose value depends on x (the kinematics of a velocity-IK problem depend on p only:
  const int* __restrict__ xdep;   // 139 of its 474 instructions are left), in tape order
};
constexpr int QP_SMALL_N = 32;  // n of the handles the thread / wavefront kernels serve; bounds k_qp_assemble's per-thread arrays, nothing else
#define QIDX(i) ((size_t)(i) * Bp + b)
// What tape_value (oh_tape_ops.h) sees of an instruction here: operand values the caller has loaded (b only where the opcode has one).  CONST, X and P
// never arrive (what X loads is what the two assemblies differ in), nor do ADD, SUB and MUL, which the callers keep as cases of their own.
struct QpRegs {
  const double va, vb;
  __device__ double cst() const { return 0.0; }
  __device__ double x() const { return 0.0; }
  __device__ double p() const { return 0.0; }
  __device__ double a() const { return va; }
  __device__ double b() const { return vb; }
};
// FULL: every instruction; else only the x-dependent ones (the others keep the values of an earlier full sweep at the same p)
template <bool FULL>
__device__ double qp_tape_forward(const QpTape& tp, const double* xs, const double* __restrict__ pb, double* __restrict__ val, const int Bp, const int b) {
#pragma clang fp contract(off)
  const int cnt = FULL ? tp.len : tp.n_xdep;
  for (int k = 0; k < cnt; ++k) {
    const int i = FULL ? k : tp.xdep[k];
    const int o = tp.op[i], ia = tp.a[i], ib = tp.bb[i];
    double v;
    switch (o) {
      case OP_CONST: v = tp.c[i]; break;
      case OP_X: v = xs[ia]; break;
      case OP_P: v = pb[ia]; break;
      case OP_ADD: v = val[QIDX(ia)] + val[QIDX(ib)]; break;  // (these three make up a QP's tape: as cases of their own 0.5 - 2 % faster, 72-variable MPC at B = 256)
      case OP_SUB: v = val[QIDX(ia)] - val[QIDX(ib)]; break;
      case OP_MUL: v = val[QIDX(ia)] * val[QIDX(ib)]; break;
      default: v = tape_value(o, QpRegs{val[QIDX(ia)], tape_op_arity(o) == 2 ? val[QIDX(ib)] : 0.0}); break;  // (coefficients may be any function of p)
    }
    val[QIDX(i)] = v;
  }
  return val[QIDX(tp.out_cost)];
}
__global__ __launch_bounds__(64) void k_qp_assemble(QpParams Q, QpTape tp, int np_raw, int B, int Bp, const double* __restrict__ par, double* __restrict__ val,
                                                    double* __restrict__ rows_out, double* __restrict__ f0_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = Q.n, m = Q.m, me = Q.me;
  const double* pb = par + (size_t)b * np_raw;
  const QpRow<double*> R = qp_row(rows_out + (size_t)b * Q.np, n, m, me);
  double *const P = R.P, *const q = R.q, *const M = R.M, *const c = R.c, *const A = R.A, *const bv = R.b;
  double x[QP_SMALL_N], f1[QP_SMALL_N];
  for (int i = 0; i < n; ++i) x[i] = 0.0;
  const double f0 = qp_tape_forward<true>(tp, x, pb, val, Bp, b);
  for (int r = 0; r < m; ++r) c[r] = val[QIDX(tp.rows[r])];
  for (int r = 0; r < me; ++r) bv[r] = val[QIDX(tp.rows[m + r])];
  for (int i = 0; i < n; ++i) {
    x[i] = 1.0;
    f1[i] = qp_tape_forward<false>(tp, x, pb, val, Bp, b);
    for (int r = 0; r < m; ++r) M[r * n + i] = val[QIDX(tp.rows[r])] - c[r];
    for (int r = 0; r < me; ++r) A[r * n + i] = val[QIDX(tp.rows[m + r])] - bv[r];
    x[i] = -1.0;
    const double fm = qp_tape_forward<false>(tp, x, pb, val, Bp, b);
    x[i] = 0.0;
    q[i] = 0.5 * (f1[i] - fm);
  }
  for (int i = 0; i < n; ++i) {
    P[i * n + i] = f1[i] - f0 - q[i];
    for (int j = 0; j < i; ++j) {
      x[i] = x[j] = 1.0;
      const double fij = qp_tape_forward<false>(tp, x, pb, val, Bp, b);
      x[i] = x[j] = 0.0;
      P[i * n + j] = P[j * n + i] = 0.5 * (fij - f1[i] - f1[j] + f0);
    }
  }
  f0_out[b] = f0;
}
// The same with one BLOCK per instance and one lane per probe point (1 + 2 n + n (n - 1) / 2 of them, 64 at a time): every large handle
// (oh_qp_block.hip solves them), and a small one with a few instances -- a tick of a velocity-IK controller is one: 36 probes side by side instead
// of one after the other (the sweep is a chain of dependent memory round trips either way).  No per-lane x: the value of an `X a` instruction
// follows from the probe's (i, j, sign).  The probes' values sit in dynamic LDS (8385 doubles at n = 128).  nb instances per launch: registers of
// lane l of instance b at val[(i * nb + b) * 64 + l]; for large handles the host loop (oh_launch_qp_assemble_block) keeps nb * len * 64 doubles
// under a fixed budget.
__global__ __launch_bounds__(64) void k_qp_assemble_block(QpParams Q, QpTape tp, int np_raw, int nb, const double* __restrict__ par, double* __restrict__ val,
                                                          double* __restrict__ rows_out, double* __restrict__ f0_out) {
#pragma clang fp contract(off)
  extern __shared__ double qa_fs[];
  double* fs = qa_fs;
  const int inst = blockIdx.x, lane = threadIdx.x;
  const int n = Q.n, m = Q.m, me = Q.me;
  const int n_probe = 1 + 2 * n + n * (n - 1) / 2;
  const double* pb = par + (size_t)inst * np_raw;
  const QpRow<double*> R = qp_row(rows_out + (size_t)inst * Q.np, n, m, me);
  double *const P = R.P, *const q = R.q, *const M = R.M, *const c = R.c, *const A = R.A, *const bv = R.b;
  const int Bp = nb * 64, b = inst * 64 + lane;  // QIDX(i) = (i * nb + inst) * 64 + lane
  for (int base = 0; base < n_probe; base += 64) {
    const int pid = base + lane;
    const bool live = pid < n_probe;
    // probe pid: 0 at x = 0; 1 .. n at e_i; n + 1 .. 2 n at -e_i; then the pairs e_i + e_j, j < i
    int pi = -1, pj = -1;
    double sign = 1.0;
    if (live && pid >= 1) {
      if (pid <= n) pi = pid - 1;
      else if (pid <= 2 * n) { pi = pid - 1 - n; sign = -1.0; }
      else {
        int k = pid - 1 - 2 * n, i = 1;
        while (k >= i) { k -= i; ++i; }
        pi = i;
        pj = k;
      }
    }
    for (int i = 0; i < tp.len; ++i) {  // full sweep on the first pass (the p-only instructions), the x-dependent ones afterwards
      if (base > 0) {
        if (i >= tp.n_xdep) break;
      }
      const int k = base > 0 ? tp.xdep[i] : i;
      const int o = tp.op[k], ia = tp.a[k], ib = tp.bb[k];
      double v;
      switch (o) {
        case OP_CONST: v = tp.c[k]; break;
        case OP_X: v = (ia == pi || ia == pj) ? sign : 0.0; break;
        case OP_P: v = pb[ia]; break;
        case OP_ADD: v = val[QIDX(ia)] + val[QIDX(ib)]; break;  // (as in qp_tape_forward)
        case OP_SUB: v = val[QIDX(ia)] - val[QIDX(ib)]; break;
        case OP_MUL: v = val[QIDX(ia)] * val[QIDX(ib)]; break;
        default: v = tape_value(o, QpRegs{val[QIDX(ia)], tape_op_arity(o) == 2 ? val[QIDX(ib)] : 0.0}); break;
      }
      val[QIDX(k)] = v;
    }
    if (live) fs[pid] = val[QIDX(tp.out_cost)];
    if (base == 0) {  // the rows at 0 first, then the columns of M and A relative to them
      if (lane == 0) {
        for (int r = 0; r < m; ++r) c[r] = val[QIDX(tp.rows[r])];
        for (int r = 0; r < me; ++r) bv[r] = val[QIDX(tp.rows[m + r])];
      }
      __syncthreads();
    }
    if (live && pid >= 1 && pid <= n) {
      const int i = pid - 1;
      for (int r = 0; r < m; ++r) M[(size_t)r * n + i] = val[QIDX(tp.rows[r])] - c[r];
      for (int r = 0; r < me; ++r) A[r * n + i] = val[QIDX(tp.rows[m + r])] - bv[r];
    }
  }
  __syncthreads();
  const double f0 = fs[0];
  for (int i = lane; i < n; i += 64) {
    const double qi = 0.5 * (fs[1 + i] - fs[1 + n + i]);
    q[i] = qi;
    P[i * n + i] = fs[1 + i] - f0 - qi;
  }
  for (int k = lane; k < n * (n - 1) / 2; k += 64) {
    int kk = k, i = 1;
    while (kk >= i) { kk -= i; ++i; }
    P[i * n + kk] = P[kk * n + i] = 0.5 * (fs[1 + 2 * n + k] - fs[1 + i] - fs[1 + kk] + f0);
  }
  if (lane == 0) f0_out[inst] = f0;
}
__global__ __launch_bounds__(256) void k_qp_add_constant(int B, double* __restrict__ f, const double* __restrict__ f0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) f[b] += f0[b];
}

size_t assemble_lds_bytes(const int n) { return sizeof(double) * (size_t)(1 + 2 * n + n * (n - 1) / 2); }  // a double per probe point
size_t g_assemble_lds[64];

}  // namespace

bool grant_dynamic_lds(const void* fn, const size_t bytes, size_t* granted /* [64], by device */) {
  static std::mutex mtx;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
  std::lock_guard<std::mutex> lock(mtx);
  if (bytes <= granted[dev]) return true;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
  granted[dev] = bytes;
  return true;
}

void oh_launch_qp_assemble(hipStream_t s, const QpParams& Q, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows,
                           const int* xdep, int n_xdep, int B, int Bp, const double* p_raw, double* val, double* rows_out, double* f0) {
  const QpTape tp{T.len, T.out_cost, op, a, b, c, rows, n_xdep, xdep};
  // room for a lane per probe: a block per instance (n <= QP_SMALL_N: 4488 bytes of LDS at the most, nothing to be granted)
  if ((size_t)B * 64 <= (size_t)Bp) hipLaunchKernelGGL(k_qp_assemble_block, dim3(B), dim3(64), assemble_lds_bytes(Q.n), s, Q, tp, T.np, B, p_raw, val, rows_out, f0);
  else hipLaunchKernelGGL(k_qp_assemble, dim3((B + 63) / 64), dim3(64), 0, s, Q, tp, T.np, B, Bp, p_raw, val, rows_out, f0);
}

int oh_qp_assemble_block_chunk(const TapeParams& T, int B) {
  // instances per launch: the register file (len * 64 doubles per instance in flight) stays under 256 MB whatever B is
  const size_t per = sizeof(double) * 64 * (size_t)(T.len > 0 ? T.len : 1);
  size_t nb = ((size_t)256 << 20) / per;
  if (nb < 1) nb = 1;
  return (int)(nb < (size_t)B ? nb : (size_t)B);
}
int oh_launch_qp_assemble_block(hipStream_t s, const QpParams& Q, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows,
                                const int* xdep, int n_xdep, int B, int chunk, const double* p_raw, double* val, double* rows_out, double* f0, std::string* err) {
  const QpTape tp{T.len, T.out_cost, op, a, b, c, rows, n_xdep, xdep};
  const size_t lds = assemble_lds_bytes(Q.n);
  if (!grant_dynamic_lds(reinterpret_cast<const void*>(k_qp_assemble_block), lds, g_assemble_lds)) {
    (void)hipGetLastError();
    *err = "k_qp_assemble_block: " + std::to_string(lds) + " bytes of LDS per block were refused";
    return 1;
  }
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nb = B - b0 < chunk ? B - b0 : chunk;
    hipLaunchKernelGGL(k_qp_assemble_block, dim3(nb), dim3(64), lds, s, Q, tp, T.np, nb, p_raw + (size_t)b0 * T.np, val, rows_out + (size_t)b0 * Q.np, f0 + b0);
  }
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    *err = std::string("k_qp_assemble_block: launch failed: ") + hipGetErrorString(e);
    return 1;
  }
  return 0;
}
void oh_launch_qp_add_constant(hipStream_t s, int B, double* f, const double* f0) {
  hipLaunchKernelGGL(k_qp_add_constant, dim3((B + 255) / 256), dim3(256), 0, s, B, f, f0);
}

bool oh_qp_is_large(const QpParams& Q) { return Q.n > QP_SMALL_N || Q.m > 256 || Q.me > 32; }
bool oh_qp_takes_block(const QpParams& Q, const int forced) { return forced == 3 || oh_qp_is_large(Q); }

int oh_launch_qp_solve(hipStream_t s, const QpParams& Q, int B, int Bp, const double* x0, const double* p, double* work, double* x, double* f, double* kkt,
                       int* iters, int* status, double* mult, const int forced, std::string* err) {
  // beyond n = 32, m = 256, me = 32 a workgroup per instance for every B (a forced 0 / 1 / 2 does not fit there and falls back to it); forced == 3: on any handle
  if (oh_qp_takes_block(Q, forced)) return oh_launch_qp_solve_block(s, Q, B, x0, p, work, x, f, kkt, iters, status, mult, err);
  // the work set of a block in LDS when it fits 48 KB at 64, 32 or 16 instances per block; for a few instances the problem row as well
  const size_t work_bytes = sizeof(double) * qp_work_doubles(Q.n, Q.m, Q.me), row_bytes = sizeof(double) * qp_row_doubles(Q.n, Q.m, Q.me);
  auto fit = [](const size_t bytes) {
    for (int c : {64, 32, 16})
      if (bytes * c <= 48 * 1024) return c;
    return 0;
  };
  const int bs2 = fit(work_bytes + row_bytes), bs1 = fit(work_bytes);
  if (forced != 0 && forced != 1 && forced != 2 && B <= 64 && work_bytes + row_bytes <= 48 * 1024) {  // a few instances: one wavefront each
    hipLaunchKernelGGL(k_qp_solve_wave, dim3(B), dim3(64), work_bytes + row_bytes, s, Q, B, x0, p, x, f, kkt, iters, status, mult);
    return 0;
  }
  int mode = bs2 ? 2 : (bs1 ? 1 : 0);  // forced: option "qp_mode" (experiments)
  if (forced == 0 || (forced == 1 && bs1) || (forced == 2 && bs2)) mode = forced;
  if (mode == 2)
    hipLaunchKernelGGL(k_qp_solve<2>, dim3((B + bs2 - 1) / bs2), dim3(bs2), (work_bytes + row_bytes) * bs2, s, Q, B, Bp, x0, p, work, x, f, kkt, iters, status, mult);
  else if (mode == 1) hipLaunchKernelGGL(k_qp_solve<1>, dim3((B + bs1 - 1) / bs1), dim3(bs1), work_bytes * bs1, s, Q, B, Bp, x0, p, work, x, f, kkt, iters, status, mult);
  else hipLaunchKernelGGL(k_qp_solve<0>, dim3((B + 63) / 64), dim3(64), 0, s, Q, B, Bp, x0, p, work, x, f, kkt, iters, status, mult);
  return 0;
}
