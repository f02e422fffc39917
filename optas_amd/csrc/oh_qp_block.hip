// Dense QP family beyond one thread / one wavefront per instance (n <= 128, m <= 1024, me <= 128): ONE WORKGROUP of 256 threads per instance.
//
//     min_x  x^T P x + q^T x      s.t.  M x + c >= 0,   A x + b = 0
//
// The iteration is the one of qp_ipm (oh_qp.hip) and of oracle/qp_ipm.py: infeasible start, the same residuals and statuses, and the scalar rules
// of oh_qp_rules.h (start, stopping test, diagonal shift and retries, Schur regularisation, fraction to the boundary, next mu), which both call.
// The algorithms are this mapping's own.  Sums associate differently: results agree to rounding, not bit for bit.
//
// What lives where:
//   global, streamed   the instance's row [P | q | M | c | A | b] (1.3 MB at the maximum sizes; M alone 1 MB)
//   LDS                H = P + P^T + M^T diag(lam/s) M as a packed lower triangle (n (n + 1) / 2 doubles, <= 66 KB), factored in place;
//                      x, rhs, dx, rd (4 n); s, lam, ds, dl (4 m); nu, dnu, r_e (3 me); a staging tile of 16 matrix rows; reduction scratch
//   global work slice  W^T = (L^{-1} A^T)^T as [n][me] and the packed lower triangle of S = W^T W (me n + me^2 doubles per instance)
// The equality rows take one triangular solve each: W = L^{-1} A^T, S = W^T W, dx = L^{-T} (y + W dnu) with y = L^{-1} rhs -- the same step as
// Y = H^{-1} A^T, S = A Y of the port.
//
// Control flow is block-uniform: every decision that leaves the iteration or skips a phase is taken from values all 256 threads read from LDS
// (or the work slice) after a barrier.
#include <hip/hip_runtime.h>

#include <string>

#include "oh_device.h"
#include "oh_kernels.h"
#include "oh_qp_layout.h"
#include "oh_qp_rules.h"

namespace {

constexpr int NT = 256;   // threads of a block
constexpr int KT = 16;    // matrix rows staged per step of the rank-k update
constexpr int TS = 4;     // register tile of the rank-k update: TS x TS entries
constexpr int NSLOT = 3;  // tiles per thread: 32 * 33 / 2 = 528 tiles of the 128 x 128 lower triangle <= 3 * 256
constexpr int SCRATCH = 1024;  // doubles the staging area has at least (partial sums of the transposed passes)

__device__ __forceinline__ int tri(const int i) { return i * (i + 1) / 2; }

// out(r, sum_j Mat[r][j] vec[j]) for every row r < rows of the row-major global matrix; 16 lanes share a row (128-byte segments)
template <class Out>
__device__ __forceinline__ void row_pass(const double* Mat, const int rows, const int cols, const double* vec, Out out) {
  const int g = threadIdx.x >> 4, sub = threadIdx.x & 15;
  for (int r0 = 0; r0 < rows; r0 += NT / 16) {  // (uniform trip count: the shuffles below run with every lane)
    const int r = r0 + g;
    double v = 0.0;
    if (r < rows)
      for (int j = sub; j < cols; j += 16) v += Mat[(size_t)r * cols + j] * vec[j];
#pragma unroll
    for (int k = 8; k >= 1; k >>= 1) v += __shfl_xor(v, k);
    if (r < rows && sub == 0) out(r, v);
  }
}

// partial sums of sum_k Mat[k][i] w0(k) and sum_k Mat[k][i] w1(k): column i by lane (coalesced), the rows dealt over 256 / cw groups;
// part[(a * NT) + g * cw + i]; col_sum adds the groups up after a barrier
__device__ __forceinline__ int col_width(const int cols) { return cols <= 32 ? 32 : (cols <= 64 ? 64 : 128); }
template <class W0, class W1>
__device__ __forceinline__ void col_pass(const double* Mat, const int rows, const int cols, double* part, W0 w0, W1 w1) {
  const int cw = col_width(cols), i = threadIdx.x % cw, g = threadIdx.x / cw, ng = NT / cw;
  double a0 = 0.0, a1 = 0.0;
  if (i < cols)
    for (int k = g; k < rows; k += ng) {
      const double v = Mat[(size_t)k * cols + i];
      a0 += v * w0(k);
      a1 += v * w1(k);
    }
  part[threadIdx.x] = a0;
  part[NT + threadIdx.x] = a1;
}
__device__ __forceinline__ double col_sum(const double* part, const int cols, const int i) {
  const int cw = col_width(cols), ng = NT / cw;
  double v = 0.0;
  for (int g = 0; g < ng; ++g) v += part[g * cw + i];
  return v;
}

// Lower triangle of Mat^T diag(d) Mat for the row-major global Mat [K][nc] (d == nullptr: no scaling): KT rows at a time through the staging
// tile, every thread owns up to NSLOT register tiles of TS x TS entries; out(i, j, value) for j <= i < nc.  Block-uniform; ends after a barrier.
template <class Out>
__device__ __forceinline__ void rank_k(const double* Mat, const int K, const int nc, const double* d, double* stage, Out out) {
  const int nt = (nc + TS - 1) / TS, npad = nt * TS, ntile = nt * (nt + 1) / 2;
  int ti[NSLOT], tj[NSLOT];
#pragma unroll
  for (int sl = 0; sl < NSLOT; ++sl) {
    const int t = threadIdx.x + sl * NT;
    int i = 0, r = t < ntile ? t : 0;
    while (r > i) { r -= i + 1; ++i; }  // t = i (i + 1) / 2 + j
    ti[sl] = t < ntile ? i : -1;
    tj[sl] = r;
  }
  double acc[NSLOT][TS][TS];
#pragma unroll
  for (int sl = 0; sl < NSLOT; ++sl)
#pragma unroll
    for (int a = 0; a < TS; ++a)
#pragma unroll
      for (int b = 0; b < TS; ++b) acc[sl][a][b] = 0.0;
  __syncthreads();  // the staging area is free
  for (int e = threadIdx.x; e < KT * (npad - nc); e += NT) stage[(e / (npad - nc)) * npad + nc + e % (npad - nc)] = 0.0;  // the padding columns
  for (int k0 = 0; k0 < K; k0 += KT) {
    const int kn = min(KT, K - k0);
    __syncthreads();
    for (int e = threadIdx.x; e < kn * nc; e += NT) stage[(e / nc) * npad + e % nc] = Mat[(size_t)k0 * nc + e];
    __syncthreads();
    for (int k = 0; k < kn; ++k) {
      const double* row = stage + k * npad;
      const double dk = d ? d[k0 + k] : 1.0;
#pragma unroll
      for (int sl = 0; sl < NSLOT; ++sl) {
        if (ti[sl] < 0) continue;
        double ri[TS], cj[TS];
#pragma unroll
        for (int a = 0; a < TS; ++a) {
          ri[a] = dk * row[ti[sl] * TS + a];
          cj[a] = row[tj[sl] * TS + a];
        }
#pragma unroll
        for (int a = 0; a < TS; ++a)
#pragma unroll
          for (int b = 0; b < TS; ++b) acc[sl][a][b] += ri[a] * cj[b];
      }
    }
  }
#pragma unroll
  for (int sl = 0; sl < NSLOT; ++sl) {
    if (ti[sl] < 0) continue;
#pragma unroll
    for (int a = 0; a < TS; ++a)
#pragma unroll
      for (int b = 0; b < TS; ++b) {
        const int i = ti[sl] * TS + a, j = tj[sl] * TS + b;
        if (i < nc && j <= i) out(i, j, acc[sl][a][b]);
      }
  }
  __syncthreads();
}

// In-place Cholesky of the packed lower triangle L (LDS or the global work slice), column by column across the block: two lanes share a row's
// dot product.  The verdict is read by every thread from L itself after a barrier: block-uniform.  Returns false on a non-positive pivot.
__device__ __forceinline__ bool chol_packed(double* L, const int n) {
  const int half = threadIdx.x & 1, rr = threadIdx.x >> 1;
  for (int j = 0; j < n; ++j) {
    const double* Lj = L + tri(j);
    for (int r0 = j; r0 < n; r0 += NT / 2) {  // rows j (the pivot) ... n - 1
      const int i = r0 + rr;
      double v = 0.0;
      if (i < n) {
        const double* Li = L + tri(i);
        for (int k = half; k < j; k += 2) v += Li[k] * Lj[k];
      }
      v += __shfl_xor(v, 1);
      if (i < n && half == 0) L[tri(i) + j] -= v;
    }
    __syncthreads();
    const double dd = Lj[j];
    if (!(dd > 0.0)) return false;
    const double l = sqrt(dd);
    __syncthreads();  // every thread has read the pivot
    for (int i = j + threadIdx.x; i < n; i += NT) L[tri(i) + j] = (i == j) ? l : L[tri(i) + j] / l;
    __syncthreads();
  }
  return true;
}

// y <- L^{-1} y (TR = false) or L^{-T} y (TR = true) for a packed lower triangle with n <= 128, by ONE wavefront: lane l holds rows l and l + 64
template <bool TR>
__device__ __forceinline__ void wave_trisolve(const double* L, const int n, double* y, const int lane) {
  const int i0 = lane, i1 = lane + 64;
  double y0 = i0 < n ? y[i0] : 0.0, y1 = i1 < n ? y[i1] : 0.0;
  for (int jj = 0; jj < n; ++jj) {
    const int j = TR ? n - 1 - jj : jj;
    const double yj = __shfl(j < 64 ? y0 : y1, j & 63) / L[tri(j) + j];
    if (lane == (j & 63)) {
      if (j < 64) y0 = yj;
      else y1 = yj;
    }
    if (TR) {
      if (i0 < j) y0 -= L[tri(j) + i0] * yj;
      if (i1 < j) y1 -= L[tri(j) + i1] * yj;
    } else {
      if (i0 > j && i0 < n) y0 -= L[tri(i0) + j] * yj;
      if (i1 > j && i1 < n) y1 -= L[tri(i1) + j] * yj;
    }
  }
  if (i0 < n) y[i0] = y0;
  if (i1 < n) y[i1] = y1;
}

// Reductions over the block of up to three values at once: red[4][3]; every thread returns with the same results.
struct Red3 { double a, b, c; };
template <class FA, class FB, class FC>
__device__ __forceinline__ Red3 block_reduce(double a, double b, double c, double* red, FA fa, FB fb, FC fc) {
  a = fa(a); b = fb(b); c = fc(c);  // over the wavefront
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[3 * w] = a; red[3 * w + 1] = b; red[3 * w + 2] = c; }
  __syncthreads();
  Red3 r{red[0], red[1], red[2]};
  for (int k = 1; k < NT / 64; ++k) {
    // (pairwise through the same functors: fa of a wavefront whose lanes all hold v is v for max / min; sums are added directly below)
    r.a = fa.pair(r.a, red[3 * k]);
    r.b = fb.pair(r.b, red[3 * k + 1]);
    r.c = fc.pair(r.c, red[3 * k + 2]);
  }
  return r;
}
struct OpMax { __device__ double operator()(double v) const { return wave64_max(v); } __device__ double pair(double x, double y) const { return fmax(x, y); } };
struct OpMin { __device__ double operator()(double v) const { return wave64_min(v); } __device__ double pair(double x, double y) const { return fmin(x, y); } };
struct OpSum { __device__ double operator()(double v) const { return wave64_sum(v); } __device__ double pair(double x, double y) const { return x + y; } };

__global__ __launch_bounds__(NT) void k_qp_solve_block(QpParams Q, int B, const double* __restrict__ x0, const double* __restrict__ par, double* __restrict__ work,
                                                       double* __restrict__ xo, double* __restrict__ fo, double* __restrict__ kkt, int* __restrict__ iters,
                                                       int* __restrict__ status, double* __restrict__ mult) {
  extern __shared__ double qb_sm[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = Q.n, m = Q.m, me = Q.me;
  const QpRow<const double*> R = qp_row(par + (size_t)b * Q.np, n, m, me);
  const double *const P = R.P, *const q = R.q, *const M = R.M, *const c = R.c, *const A = R.A, *const bv = R.b;
  double* Wt = work + (size_t)b * ((size_t)me * n + (size_t)me * me);  // [n][me]: column r = L^{-1} A_r
  double* S = Wt + (size_t)me * n;                                      // packed lower triangle, me (me + 1) / 2
  double* w = qb_sm;
  double* H = w; w += tri(n);
  double* x = w; w += n;
  double* rhs = w; w += n;
  double* dx = w; w += n;
  double* rd = w; w += n;
  double* s = w; w += m;
  double* lam = w; w += m;
  double* ds = w; w += m;
  double* dl = w; w += m;
  double* nu = w; w += me;
  double* dnu = w; w += me;
  double* re = w; w += me;
  double* red = w; w += 16;
  double* stage = w;  // max(KT * npad(n), KT * npad(me), SCRATCH) doubles

  for (int i = tid; i < n; i += NT) x[i] = x0[(size_t)b * n + i];
  for (int i = tid; i < me; i += NT) nu[i] = 0.0;
  __syncthreads();
  double mu = 1.0;
  row_pass(M, m, n, x, [&](const int r, const double v) {
    const double sv = qp_rules::initial_slack(v + c[r]);
    s[r] = sv;
    lam[r] = qp_rules::initial_multiplier(mu, sv);
  });
  __syncthreads();
  int st = OH_STATUS_MAX_ITER, it = 0;
  double stat = 0.0, feas = 0.0, gap = 0.0;
  for (; it <= Q.max_iter; ++it) {
    // ---- residuals: r_p -> ds, r_e -> re, r_d -> rd ------------------------------------------------------------------------------------
    row_pass(M, m, n, x, [&](const int r, const double v) { ds[r] = v + c[r] - s[r]; });
    row_pass(A, me, n, x, [&](const int r, const double v) { re[r] = v + bv[r]; });
    row_pass(P, n, n, x, [&](const int r, const double v) { rd[r] = v + q[r]; });  // P x; P^T x below: P need not be symmetric
    for (int k = tid; k < m; k += NT) dl[k] = lam[k] / s[k];
    __syncthreads();
    // M^T lam and M^T [(mu/s - lam) - (lam/s) r_p] in one sweep over M
    col_pass(M, m, n, stage, [&](const int k) { return lam[k]; }, [&](const int k) { return (mu / s[k] - lam[k]) - dl[k] * ds[k]; });
    __syncthreads();
    double mtl = 0.0, mtw = 0.0;
    if (tid < n) { mtl = col_sum(stage, n, tid); mtw = col_sum(stage + NT, n, tid); }
    __syncthreads();
    col_pass(P, n, n, stage, [&](const int k) { return x[k]; }, [&](const int) { return 0.0; });
    __syncthreads();
    double ptx = 0.0;
    if (tid < n) ptx = col_sum(stage, n, tid);
    __syncthreads();
    col_pass(A, me, n, stage, [&](const int k) { return nu[k]; }, [&](const int) { return 0.0; });
    __syncthreads();
    double l_stat = 0.0, l_feas = 0.0, l_gap = 0.0;
    bool finite = true;
    if (tid < n) {
      const double v = rd[tid] + ptx - mtl - col_sum(stage, n, tid);
      rd[tid] = v;
      rhs[tid] = -v + mtw;
      l_stat = fabs(v);
      finite = qp_rules::finite(v);
    }
    bool feas_nan = false;
    for (int k = tid; k < m; k += NT) {
      const double a = fabs(ds[k]);
      feas_nan = feas_nan || !(a == a);
      l_feas = fmax(l_feas, a);
      l_gap = fmax(l_gap, s[k] * lam[k]);
    }
    for (int k = tid; k < me; k += NT) {
      const double a = fabs(re[k]);
      feas_nan = feas_nan || !(a == a);
      l_feas = fmax(l_feas, a);
    }
    {
      const Red3 r = block_reduce(l_stat, l_feas, l_gap, red, OpMax{}, OpMax{}, OpMax{});
      stat = r.a; feas = r.b; gap = r.c;
      const Red3 f = block_reduce((finite && !feas_nan) ? 0.0 : 1.0, 0.0, 0.0, red, OpMax{}, OpMax{}, OpMax{});
      if (f.a != 0.0) { st = OH_STATUS_NUMERICAL; break; }
    }
    if (qp_rules::converged(stat, feas, gap, Q.tol)) { st = OH_STATUS_CONVERGED; break; }
    if (it == Q.max_iter) break;
    // ---- H = P + P^T + M^T diag(lam/s) M (+ shift), factored in place; rebuilt with a 1000 x larger shift on a failed pivot -------------
    auto build = [&]() { rank_k(M, m, n, dl, stage, [&](const int i, const int j, const double v) { H[tri(i) + j] = v + P[i * n + j] + P[j * n + i]; }); };
    build();
    double dmax = 0.0;
    for (int i = tid; i < n; i += NT) dmax = fmax(dmax, fabs(H[tri(i) + i]));
    dmax = block_reduce(dmax, 0.0, 0.0, red, OpMax{}, OpMax{}, OpMax{}).a;
    double shift = qp_rules::first_shift(dmax);
    bool ok = false;
    for (int attempt = 0; attempt < qp_rules::SHIFT_ATTEMPTS && !ok; ++attempt) {
      if (attempt > 0) {
        build();
        shift *= qp_rules::SHIFT_GROWTH;
      }
      for (int i = tid; i < n; i += NT) H[tri(i) + i] += shift;
      __syncthreads();
      ok = chol_packed(H, n);
      __syncthreads();
    }
    if (!ok) { st = OH_STATUS_NUMERICAL; break; }
    // ---- W = L^{-1} A^T and y = L^{-1} rhs: 16 lanes per right-hand side (the me rows of A, then rhs), entry k = l + 16 s of it in register s of
    //      lane l; row i of the substitution is a dot product over the 16 lanes, no memory traffic but the broadcast reads of L -------------------
    static_assert(OH_QP_MAX_N <= 16 * 8, "eight registers per lane hold a right-hand side");
    for (int r0 = 0; r0 <= me; r0 += NT / 16) {  // (uniform trip count: the shuffles below run with every lane)
      const int r = r0 + (tid >> 4), l = tid & 15;
      const bool live = r <= me;
      double wv[8];
#pragma unroll
      for (int sl = 0; sl < 8; ++sl) {
        const int k = l + 16 * sl;
        wv[sl] = (live && k < n) ? (r < me ? A[r * n + k] : rhs[k]) : 0.0;
      }
      for (int i = 0; i < n; ++i) {
        const double* Li = H + tri(i);
        double part = 0.0;
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) {
          const int k = l + 16 * sl;
          if (k < i) part += Li[k] * wv[sl];
        }
#pragma unroll
        for (int k = 8; k >= 1; k >>= 1) part += __shfl_xor(part, k);
        const double Lii = Li[i];
#pragma unroll
        for (int sl = 0; sl < 8; ++sl)
          if (l + 16 * sl == i) wv[sl] = (wv[sl] - part) / Lii;
      }
#pragma unroll
      for (int sl = 0; sl < 8; ++sl) {
        const int k = l + 16 * sl;
        if (live && k < n) {
          if (r < me) Wt[(size_t)k * me + r] = wv[sl];
          else rhs[k] = wv[sl];
        }
      }
    }
    __syncthreads();
    if (me > 0) {
      // S = W^T W (+ regularisation), S dnu = -r_e - W^T y, z = y + W dnu
      rank_k(Wt, n, me, nullptr, stage, [&](const int i, const int j, const double v) { S[tri(i) + j] = (i == j) ? v + qp_rules::schur_regularisation(v) : v; });
      col_pass(Wt, n, me, stage, [&](const int k) { return rhs[k]; }, [&](const int) { return 0.0; });
      __syncthreads();
      if (tid < me) dnu[tid] = -re[tid] - col_sum(stage, me, tid);
      __syncthreads();
      const bool oks = chol_packed(S, me);
      __syncthreads();
      if (!oks) { st = OH_STATUS_NUMERICAL; break; }
      if (tid < 64) {
        wave_trisolve<false>(S, me, dnu, tid);
        wave_trisolve<true>(S, me, dnu, tid);
      }
      __syncthreads();
      row_pass(Wt, n, me, dnu, [&](const int r, const double v) { rhs[r] += v; });
      __syncthreads();
    }
    if (tid < 64) wave_trisolve<true>(H, n, rhs, tid);
    __syncthreads();
    for (int i = tid; i < n; i += NT) dx[i] = rhs[i];
    __syncthreads();
    // ---- ds = M dx + r_p ; dlam = (mu/s - lam) - (lam/s) ds ; fraction to the boundary ---------------------------------------------------
    row_pass(M, m, n, dx, [&](const int r, const double mv) {
      const double v = ds[r] + mv;
      ds[r] = v;
      dl[r] = (mu / s[r] - lam[r]) - dl[r] * v;
    });
    __syncthreads();
    double ap = 1.0, ad = 1.0;
    for (int k = tid; k < m; k += NT) {
      const double v = ds[k], d2 = dl[k];
      if (v < 0.0) ap = fmin(ap, qp_rules::boundary_step(s[k], v));
      if (d2 < 0.0) ad = fmin(ad, qp_rules::boundary_step(lam[k], d2));
    }
    {
      const Red3 r = block_reduce(ap, ad, 0.0, red, OpMin{}, OpMin{}, OpMin{});
      ap = r.a; ad = r.b;
    }
    for (int i = tid; i < n; i += NT) x[i] += ap * dx[i];
    double comp = 0.0;
    for (int k = tid; k < m; k += NT) {
      s[k] += ap * ds[k];
      lam[k] += ad * dl[k];
      comp += s[k] * lam[k];
    }
    for (int k = tid; k < me; k += NT) nu[k] += ad * dnu[k];
    comp = block_reduce(comp, 0.0, 0.0, red, OpSum{}, OpSum{}, OpSum{}).a;
    if (m > 0) mu = qp_rules::next_mu(ap, ad, comp, m, Q.tol);
    __syncthreads();
  }
  // ---- outputs ---------------------------------------------------------------------------------------------------------------------------
  __syncthreads();
  row_pass(P, n, n, x, [&](const int r, const double v) { rd[r] = (v + q[r]) * x[r]; });
  __syncthreads();
  double fval = 0.0;
  for (int i = tid; i < n; i += NT) {
    fval += rd[i];
    if (xo) xo[(size_t)b * n + i] = x[i];
  }
  fval = block_reduce(fval, 0.0, 0.0, red, OpSum{}, OpSum{}, OpSum{}).a;
  if (tid == 0) {
    if (fo) fo[b] = fval;
    if (kkt) { kkt[3 * (size_t)b] = stat; kkt[3 * (size_t)b + 1] = feas; kkt[3 * (size_t)b + 2] = gap; }
    if (iters) iters[b] = it;
    if (status) status[b] = st;
  }
  if (mult) {
    for (int i = tid; i < m; i += NT) mult[(size_t)b * (m + me) + i] = lam[i];
    for (int i = tid; i < me; i += NT) mult[(size_t)b * (m + me) + m + i] = nu[i];
  }
}

size_t g_block_lds[64];  // (grant_dynamic_lds, oh_kernels.h)

size_t block_lds_bytes(const int n, const int m, const int me) {
  const int npad = (n + TS - 1) / TS * TS, mepad = (me + TS - 1) / TS * TS;
  size_t stage = (size_t)KT * (npad > mepad ? npad : mepad);
  if (stage < SCRATCH) stage = SCRATCH;
  return sizeof(double) * ((size_t)n * (n + 1) / 2 + 4 * (size_t)n + 4 * (size_t)m + 3 * (size_t)me + 16 + stage);
}

}  // namespace

size_t oh_qp_block_work_doubles(const QpParams& Q) { return (size_t)Q.me * Q.n + (size_t)Q.me * Q.me; }

int oh_launch_qp_solve_block(hipStream_t s, const QpParams& Q, int B, const double* x0, const double* p, double* work, double* x, double* f, double* kkt, int* iters,
                             int* status, double* mult, std::string* err) {
  const size_t lds = block_lds_bytes(Q.n, Q.m, Q.me);
  if (!grant_dynamic_lds(reinterpret_cast<const void*>(k_qp_solve_block), lds, g_block_lds)) {
    (void)hipGetLastError();
    *err = "k_qp_solve_block: " + std::to_string(lds) + " bytes of LDS per block were refused";
    return 1;
  }
  hipLaunchKernelGGL(k_qp_solve_block, dim3(B), dim3(NT), lds, s, Q, B, x0, p, work, x, f, kkt, iters, status, mult);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    *err = std::string("k_qp_solve_block: launch failed: ") + hipGetErrorString(e);
    return 1;
  }
  return 0;
}

bool oh_kernel_info_qp_block(const char* name, OhKernelInfo* out) {
  if (std::string(name) != "k_qp_solve_block") return false;
  const size_t lds = block_lds_bytes(OH_QP_MAX_N, OH_QP_MAX_M, OH_QP_MAX_ME);  // the largest instance
  const void* fn = reinterpret_cast<const void*>(k_qp_solve_block);
  if (!grant_dynamic_lds(fn, lds, g_block_lds)) return false;
  hipFuncAttributes a;
  if (hipFuncGetAttributes(&a, fn) != hipSuccess) return false;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_qp_solve_block, NT, lds) != hipSuccess) nb = 0;
  *out = OhKernelInfo{a.numRegs, (int)a.localSizeBytes, (int)(a.sharedSizeBytes + lds), NT, nb};
  return true;
}
