// Dense QP family: where things lie, stated once.  The row of one instance is [P | q | M | c | A | b]; the work set of the thread and wavefront
// kernels (oh_qp.hip) is [x | s | lam | nu | H | rhs | dx | ds | dl | Y | S | dnu | rd].  Both carves take any accessor with `acc + elements`:
// double*, const double*, QArr (oh_qp.hip: element k at p[k * stride]) or QpOffset, which turns a carve into a size.
// (k_qp_solve_block keeps another set in LDS: block_lds_bytes, oh_qp_block.hip.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

struct QpOffset {
  size_t at;
  __host__ __device__ QpOffset operator+(const size_t k) const { return QpOffset{at + k}; }
};

template <class Acc>
struct QpRow {
  Acc P;   // [n][n]
  Acc q;   // [n]
  Acc M;   // [m][n]
  Acc c;   // [m]
  Acc A;   // [me][n]
  Acc b;   // [me]
  Acc end;
};
template <class Acc>
__host__ __device__ inline QpRow<Acc> qp_row(const Acc p, const int n, const int m, const int me) {
  QpRow<Acc> r{p, p, p, p, p, p, p};
  r.q = r.P + n * n;  // (n, me <= 128)
  r.M = r.q + n;
  r.c = r.M + (size_t)m * n;
  r.A = r.c + m;
  r.b = r.A + me * n;
  r.end = r.b + me;
  return r;
}

template <class Acc>
struct QpWork {
  Acc x, s, lam, nu;
  Acc H;            // [n][n], lower triangle; its Cholesky factor in place
  Acc rhs, dx, ds, dl;
  Acc Y;            // [me][n]: H^{-1} A^T, row i = H^{-1} A_i
  Acc S;            // [me][me], lower triangle of A Y
  Acc dnu, rd;
  Acc end;
};
template <class Acc>
__host__ __device__ inline QpWork<Acc> qp_work(const Acc p, const int n, const int m, const int me) {
  QpWork<Acc> w{p, p, p, p, p, p, p, p, p, p, p, p, p, p};
  w.s = w.x + (size_t)n;
  w.lam = w.s + (size_t)m;
  w.nu = w.lam + (size_t)m;
  w.H = w.nu + (size_t)me;
  w.rhs = w.H + (size_t)n * n;
  w.dx = w.rhs + (size_t)n;
  w.ds = w.dx + (size_t)n;
  w.dl = w.ds + (size_t)m;
  w.Y = w.dl + (size_t)m;
  w.S = w.Y + (size_t)me * n;
  w.dnu = w.S + (size_t)me * me;
  w.rd = w.dnu + (size_t)me;
  w.end = w.rd + (size_t)n;
  return w;
}

// doubles of a row (QpParams::np; the parameter vector of a handle without a tape) and of a work set (QpParams::nwork)
__host__ __device__ inline size_t qp_row_doubles(const int n, const int m, const int me) { return qp_row(QpOffset{0}, n, m, me).end.at; }
__host__ __device__ inline size_t qp_work_doubles(const int n, const int m, const int me) { return qp_work(QpOffset{0}, n, m, me).end.at; }
