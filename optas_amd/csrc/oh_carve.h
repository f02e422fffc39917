// How the host API lays arrays out inside one allocation: a cursor (Carver) and, per pool and per staging area, ONE list of take() calls
// that both measures the allocation (null base) and carves it.  Host-only, no HIP runtime call: tests/pool_layout.hip runs every list on the CPU.
// A new array is one take() in one list.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "oh_kernels.h"

// A cursor over a byte range.  take<T>(n) returns n elements at the cursor and advances; with a null base it only advances and returns null
// (the measuring pass), and bytes() is then the size the range needs.
//   Packed: arrays follow each other with no padding beyond alignof(T) (device pools)
//   Slots:  every take starts on a multiple of 256 bytes, and bytes() is a whole number of slots (staging areas)
class Carver {
 public:
  enum Mode { Packed, Slots };
  Carver(void* base, const Mode mode) : base_((char*)base), mode_(mode) {}
  template <class T>
  T* take(const size_t n) {
    off_ = up(off_, mode_ == Slots ? 256 : alignof(T));
    T* const r = base_ ? (T*)(base_ + off_) : nullptr;
    if (log) log->push_back({off_, n * sizeof(T)});
    off_ += n * sizeof(T);
    return r;
  }
  size_t bytes() const { return mode_ == Slots ? up(off_, 256) : off_; }
  std::vector<std::pair<size_t, size_t>>* log = nullptr;  // (offset, bytes) of every take, for the layout test

 private:
  static size_t up(const size_t v, const size_t a) { return (v + a - 1) / a * a; }
  char* base_;
  Mode mode_;
  size_t off_ = 0;
};

// ---- device pools (Packed) -------------------------------------------------------------------------------------------------------------

// Trajectory families (ensure_capacity): SoA stage arrays of row stride Bp.
inline void layout_fig(Carver& c, FigBuffers& D, const int N, const int lock, const int T, const int Bp) {
  const int NZ = lock ? N - 3 : N;
  const size_t per_q = (size_t)T * N * Bp;
  // Householder vectors of the null-space basis: 3N - 3 rows per knot (HV_ROWS).  (Until round 3 this was carved as N x NZ rows, the size of Z
  // itself: at 393 216 instances the second slot then started 4.4 GB after the first and the sweep's 32-bit slot offset wrapped.)
  const size_t per_Z = (size_t)T * (3 * N - 3) * Bp;
  const size_t per_Dr = (size_t)T * (NZ * (NZ + 1) / 2) * Bp;
  const size_t per_t = (size_t)T * Bp;
  for (int s = 0; s < 2; ++s) D.q[s] = c.take<double>(per_q);
  for (int s = 0; s < 2; ++s) D.q_spare[s] = c.take<double>(per_q);
  for (int s = 0; s < 2; ++s) D.Z[s] = c.take<double>(per_Z);
  for (int s = 0; s < 2; ++s) D.Dr[s] = c.take<double>(per_Dr);
  for (int s = 0; s < 2; ++s) D.g[s] = c.take<double>(per_q);
  for (int s = 0; s < 2; ++s) D.phi[s] = c.take<double>(per_t);
  for (int s = 0; s < 2; ++s) D.cv[s] = c.take<double>(per_t);
  // (the sweep with the coupling folded in addresses G of either slot as a 32-bit offset from the lowest of these three: the carried
  //  compaction swaps Gfull[] with the spare, so Gfull[0], Gfull[1], G_spare stay adjacent in the pool)
  for (int s = 0; s < 2; ++s) D.Gfull[s] = c.take<double>(per_q);
  D.G_spare = c.take<double>(per_q);
  for (int s = 0; s < 2; ++s) D.mdl[s] = c.take<double>((size_t)T * (3 + 3 * NZ) * Bp);
  for (int s = 0; s < 2; ++s) D.E[s] = c.take<double>((size_t)T * NZ * NZ * Bp);
  for (int s = 0; s < 2; ++s) D.gt[s] = c.take<double>((size_t)T * NZ * Bp);
  for (int s = 0; s < 2; ++s) D.merit[s] = c.take<double>(per_t);
  D.zstep = c.take<double>((size_t)T * NZ * Bp);
  D.Kmat = c.take<double>((size_t)T * NZ * NZ * Bp);
  D.kvec = c.take<double>((size_t)T * NZ * Bp);
  D.ref = c.take<double>((size_t)12 * Bp);
  D.fconst = c.take<double>(Bp);
  D.f_cur = c.take<double>(Bp);
  D.pred = c.take<double>(Bp);
  D.mu = c.take<double>(Bp);
  D.nun = c.take<double>(Bp);
  D.stat = c.take<double>(Bp);
  D.feas = c.take<double>(Bp);
  D.lam_h = c.take<double>((size_t)4 * T * Bp);
  D.lead = c.take<double>(per_t);  // lead-joint angles
  // (the two index arrays of the lean carried compaction live in the room of lead[]: that sequence runs on chains without a lead joint only, whose
  //  kernels never touch lead[], and T doubles per instance hold two ints for every T >= 1 -- no array is added, every recorded offset stays)
  D.oldidx = D.lead ? (int*)D.lead : nullptr;
  D.rescue_list = D.lead ? (int*)D.lead + Bp : nullptr;
  if (!lock) D.lam_h = nullptr;    // no quaternion rows, no multipliers to report (the room stays)
  D.cur = c.take<int>(Bp);
  D.first = c.take<int>(Bp);
  D.skip = c.take<int>(Bp);
  D.polish = c.take<int>(Bp);
  D.stale = c.take<int>(Bp);
  D.status = c.take<int>(Bp);
  D.iters = c.take<int>(Bp);
  D.orig = c.take<int>(Bp);
  D.newidx = c.take<int>(Bp);
  D.n_running = c.take<int>(1);
  D.n_new = c.take<int>(1);
  D.work = c.take<unsigned long long>(14);  // the counter block (8-byte aligned: 9 Bp + 2 ints lie before it, Bp a multiple of 64)
  D.n_defer = D.work ? (int*)(D.work + 3) : nullptr;  // (two ints inside the spare part of the counter block: zeroed with it at the start of a solve)
  // (work[4]: the length of the rescue list; work[5], work[6]: instances rescued / instances whose gradient moved, summed over a solve)
  D.n_rescue = D.work ? (int*)(D.work + 4) : nullptr;
  D.scan_blk = c.take<int>(8 * 1024);
  D.defer_list = c.take<int>(2 * (size_t)Bp);  // [2][Bp]
  c.take<int>(2);  // slack the pool has always had behind its last array
}

// Inequality rows of the trajectory families (ensure_guards); D.fpsi lives here, between meas_prev and mcv.
inline void layout_guards(Carver& c, GuardBuffers& GB, double*& fpsi, const GuardParams& GP, const int N, const int T, const int Bp) {
  const size_t npar = (size_t)GP.n_links + 4 * (size_t)GP.n_obs;
  const size_t n_lam = (size_t)T * GP.NC * Bp, n_lamv = GP.vel ? (size_t)T * 2 * N * Bp : 0;
  GB.lam = c.take<double>(n_lam);
  GB.par = c.take<double>(npar * Bp);
  GB.psi[0] = c.take<double>((size_t)T * Bp);
  GB.psi[1] = c.take<double>((size_t)T * Bp);
  GB.rho = c.take<double>(Bp);
  GB.rho_next = c.take<double>(Bp);
  GB.omega = c.take<double>(Bp);
  GB.meas_prev = c.take<double>(Bp);
  fpsi = c.take<double>(Bp);
  GB.mcv[0] = c.take<double>((size_t)T * Bp);
  GB.mcv[1] = c.take<double>((size_t)T * Bp);
  GB.meas = c.take<double>(Bp);
  GB.lamv = GP.vel ? c.take<double>(n_lamv) : nullptr;
  GB.lam_out = c.take<double>(n_lam);
  GB.lamv_out = GP.vel ? c.take<double>(n_lamv) : nullptr;
  GB.scr = c.take<double>(n_lam + n_lamv + (npar + 8) * Bp);  // the compaction scratch
  GB.ls_gd = c.take<double>(Bp);
  GB.ls_q = c.take<double>(Bp);
  GB.outer = c.take<int>(Bp);
  GB.n_outer = c.take<int>(Bp);
  GB.ls_count = c.take<int>(Bp);
}

// Torque MPC (tq_solve_device): unit-contiguous records; the strides of the [slot][B][T] arrays follow the live batch B.
inline void layout_tq(Carver& c, TqBuffers& D, const int B, const int T) {
  const size_t BT = (size_t)B * T;
  D.xs = c.take<double>(2 * BT * TQ_XS);
  D.st = c.take<double>(2 * BT * TQ_SD);
  D.lam = c.take<double>(2 * BT * TQ_LAM);
  D.gains = c.take<double>(BT * TQ_GN);
  D.goal = c.take<double>(BT * 4);
#define X(type, name, init) D.name = c.take<type>(B);
  OH_TQ_INST(X)  // the doubles, then the ints
#undef X
  D.list = c.take<int>(B);
  D.n_running = c.take<int>(1);
  D.n_list = c.take<int>(1);
  c.take<int>(14);  // slack the pool has always had behind its last array (12 B + 16 ints in all)
}

// Point-mass MPC (pm_prepare): [rows][Bp] each.
inline void layout_pm(Carver& c, PmBuffers& D, const int T, const int Bp) {
  const size_t T1 = (size_t)(T - 1), Tn = (size_t)T;
  D.a = c.take<double>(2 * T1 * Bp);
  D.X = c.take<double>(4 * Tn * Bp);
  D.s = c.take<double>(9 * Tn * Bp);
  D.lam = c.take<double>(9 * Tn * Bp);
  D.K = c.take<double>(8 * T1 * Bp);
  D.kk = c.take<double>(2 * T1 * Bp);
  D.dX = c.take<double>(4 * Tn * Bp);
  D.da = c.take<double>(2 * T1 * Bp);
}

// ---- staging of the host-buffer solves (Slots) -------------------------------------------------------------------------------------------

// Doubles per instance of a handle's problem: x, p, and the multipliers oh_get_multipliers returns (0: the problem has none).
struct Shape { size_t nx, npar, mult; };

// Staging area of a host-buffer solve of B instances: inputs [x0 | p], then outputs [x | f | kkt | iters | status].  The pinned mirror of a small
// oh_solve is carved by the same list, so that each of the two spans moves in one transfer.
struct StageLayout {
  double *x0, *p, *x, *f, *kkt;
  int *iters, *status;
  size_t b_x, b_p, b_f, b_k, b_i, total;  // bytes of x0 / x, p, f, kkt, iters / status, and of the whole area
  size_t in_bytes() const { return (size_t)((char*)p - (char*)x0) + b_p; }          // the span [x0 | p]
  size_t out_bytes() const { return (size_t)((char*)status - (char*)x) + b_i; }     // the span [x ... status]
};
inline void layout_stage(Carver& c, StageLayout& L, const Shape& sh, const size_t B) {
  L.b_x = sizeof(double) * sh.nx * B; L.b_p = sizeof(double) * sh.npar * B; L.b_f = sizeof(double) * B; L.b_k = sizeof(double) * 3 * B; L.b_i = sizeof(int) * B;
  L.x0 = c.take<double>(sh.nx * B);
  L.p = c.take<double>(sh.npar * B);
  L.x = c.take<double>(sh.nx * B);
  L.f = c.take<double>(B);
  L.kkt = c.take<double>(3 * B);
  L.iters = c.take<int>(B);
  L.status = c.take<int>(B);
  L.total = c.bytes();
}
