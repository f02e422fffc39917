// Shared host/device declarations between the kernel sources (device code) and the host sources of the C ABI (oh_api.hip, oh_api_<family>.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "optas_hip.h"
#include "oh_types.h"

// Code-object facts of a kernel by name (hipFuncGetAttributes + occupancy query): what bench.py reports as roofline.occupancy.
struct OhKernelInfo {
  int vgprs, scratch_bytes, lds_bytes, block, blocks_per_cu;
};
bool oh_kernel_info_figure8(const char* name, OhKernelInfo* out);
bool oh_kernel_info_fkjac(const char* name, OhKernelInfo* out);
bool oh_kernel_info_torque(const char* name, OhKernelInfo* out);
bool oh_kernel_info_linkkin(const char* name, OhKernelInfo* out);
bool oh_kernel_info_qp_block(const char* name, OhKernelInfo* out);
bool oh_kernel_info_tape_wave(const char* name, OhKernelInfo* out);
bool oh_kernel_info_ik(const char* name, OhKernelInfo* out);

void oh_launch_fk_jac(hipStream_t s, bool soa, const oh_chain* d_chain, int n_chain, int ndof, int n, const double* q, double* pose, double* J);
// What oh_set_link_frames keeps on the device for k_link_kin (oh_linkkin.hip): the chains root->link and root->base, and the number of leading
// actuated joints the two have in common (same joint, same folded constants).
struct OhLinkFrames {
  oh_chain link, base;
  int n_shared;
};
// a3: the unit vector of the axis output (read only with out.axis); out: device pointers, any of them null
void oh_launch_link_kin(hipStream_t s, bool soa, const OhLinkFrames* d_frames, int n_link, int n, const double* q, const double* a3, const oh_link_out& out);
bool oh_launch_setup(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, const double* x0, const double* p);
bool oh_launch_eval(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int slot, int part = 0);
bool oh_launch_carry(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int phase, int Bnew, int slot);  // phase 0: gather, 1: scatter, 2: the gather's rest after a moving retraction
bool oh_launch_eval_lead(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int slot);
bool oh_launch_couple(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int slot);
bool oh_launch_couple_vel(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const GuardBuffers& GB, int slot);
// with_copy: k_defer_copy right behind the sweep of the folded-coupling family (false: the host launches oh_launch_sweep_lists itself)
bool oh_launch_step(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int slot, bool with_copy = true);
// k_defer_copy's work and, behind the sweep of a lean carried compaction (rescue), the accepted knots of the instances in D.rescue_list from the old
// layout to q_spare[1], in one launch; count: entries of the longer list, -1 unknown
bool oh_launch_sweep_lists(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int slot, bool rescue, int count);
bool oh_launch_eval_free(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int slot);
bool oh_launch_couple_free(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int slot);
bool oh_launch_couple_free_vel(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const GuardBuffers& GB, int slot);
// Sweep of a position-tracking launch, chosen by the host (oh_api.hip: free_sweep): one lane per instance (k_step_free), or a block per instance
// by cyclic reduction (k_step_free_pcr), by cyclic reduction with eight lanes per knot (k_step_free_cp), by the twisted factorisation
// (k_step_free_bb, 7 joints); or the whole solve in one launch (k_free_persist).  The block-per-instance sweeps are instantiated for 6 and 7 joints.
enum FreeSweep { FREE_SERIAL, FREE_PCR, FREE_CP, FREE_BB, FREE_PERSIST };
bool oh_launch_step_free(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int slot, FreeSweep sweep);
void oh_launch_move_rows(hipStream_t s, void* arr, void* scr, int rows, int Bp, int B, int Bnew, const int* newidx, bool is_int);
void oh_launch_move_rows_live(hipStream_t s, double* a0, double* a1, double* scr, int rows, int Bp, int B, int Bnew, const int* newidx, const int* cur, const int* curn);
bool oh_launch_setup_guards(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const GuardBuffers& GB, const double* p);
void oh_launch_guard_infeasible(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const double* p, int B, double* kkt, int* status);
bool oh_launch_eval_guarded(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const GuardBuffers& GB, int slot);
bool oh_launch_free_persist(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const GuardBuffers& GB);  // whole solve, one block per instance
bool oh_launch_step_guarded(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const GuardBuffers& GB, int slot,
                            FreeSweep sweep);
bool oh_launch_eval_locked_guarded(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const GuardBuffers& GB, int slot, int part);
bool oh_launch_step_locked_guarded(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const GuardBuffers& GB, int slot);
void oh_launch_guard_emit(hipStream_t s, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const GuardBuffers& GB, int NV, int only_done);
void oh_launch_guard_compact(hipStream_t s, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const GuardBuffers& GB, int NV, int phase, int Bnew);
bool oh_launch_tail(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int slot);
bool oh_launch_tail_vel(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, const GuardParams& GP, const GuardBuffers& GB, int slot);
bool oh_launch_finalize(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int only_done, double* x, double* f, double* kkt,
                        int* iters, int* status, int parts = 3);  // parts: 1 the solution x (LDS transpose), 2 scalars + multipliers, 3 both
void oh_launch_scan_running(hipStream_t s, const FigBuffers& D, int sort);
bool oh_launch_compact(hipStream_t s, int n, const FigParams& P, const FigBuffers& D, int phase, int Bnew, int slot);

// ---- OH_PROBLEM_POINT_MASS_MPC ---------------------------------------------------------------------------
struct PmParams {
  int T;
  double dt, w_acc, ylim, vlim, safe_sq, tol;
  int max_iter;
  int final_only;  // 1: tracking cost on the last knot only (point_mass_planner.py:43), 0: on every knot (point_mass_mpc.py:131)
  double w_vel;    // weight of sum ||dy_t||^2 (point_mass_planner.py:45-47; 0 in the MPC script)
  int fix_vf;      // 1: terminal row dy_{T-1} = 0 (point_mass_planner.py:34-35)
};
struct PmBuffers {
  int B, Bp;
  double *a, *X, *s, *lam, *K, *kk, *dX, *da;  // [rows][Bp], rows: 2(T-1), 4T, 9T, 9T, 8(T-1), 2(T-1), 4T, 2(T-1)
};
void oh_launch_pm_solve(hipStream_t s, const PmParams& P, const PmBuffers& D, const double* x0, const double* p, double* x, double* f, double* kkt,
                        int* iters, int* status, int wave_max);  // wave_max: a wavefront per plant up to this many plants (option pm_wave_max)

void oh_launch_pm_tick_params(hipStream_t s, int B, int T, int tick, int advance, double ramp, const double* state, const double* obs_table, double* p);
void oh_launch_pm_advance(hipStream_t s, int B, int T, int advance, const double* x, double* state_next);

// ---- OH_PROBLEM_TORQUE_MPC (BASELINE configs[4]: RNEA dynamics rows) -------------------------------
// Layouts are unit-contiguous ([instance][knot][...]): the evaluation kernels work with one lane per (instance, knot,
// joint) and the step kernel with one wavefront per instance, so a wavefront reads whole records.
// The records, named once (offsets in doubles; every block of N joints has room for 8):
struct TqKnot {  // per knot of D.xs
  static constexpr int q = 0, dq = 8, ddq = 16, size = 24;
  static constexpr int pad = 7;  // the 8th word of each block: zero
};
struct TqStage {  // per knot of D.st
  static constexpr int H = 0;          // stage block, packed lower (3N)(3N+1)/2: tq_packed(row, col) over (q | dq | ddq)
  static constexpr int g_f = 231;      // gradient of the cost (3N)
  static constexpr int f = 252, barrier = 253, relaxed = 254, viol = 255;  // cost, barrier sum per unit mu_b, rows in the relaxed zone, worst violation
  static constexpr int tau = 256;      // torques (N)
  static constexpr int cmpl = 263;     // max lam s
  static constexpr int g_b = 272;      // gradient of the barrier per unit mu_b (3N): the stage gradient is g_f + mu_b g_b
  static constexpr int J = 296;        // d tau / d z, N x 3N row-major: the step kernel's fraction-to-the-boundary rule needs the linearised rows
  static constexpr int size = 448;
};
struct TqLam {  // per knot of D.lam: multipliers of tau - lo >= 0 (N) at 0, of up - tau >= 0 (N) at N; velocity rows alike from `vel`
  static constexpr int vel = 16, size = 32;
};
constexpr int tq_packed(const int row, const int col) { return row * (row + 1) / 2 + col; }  // row >= col
constexpr int TQ_NZ_MAX = 3 * 7;  // (q | dq | ddq) of the longest chain
static_assert(TqStage::g_f == tq_packed(TQ_NZ_MAX, 0) && TqStage::g_f == TQ_NZ_MAX * (TQ_NZ_MAX + 1) / 2, "the gradient follows the packed 21 x 21 block");
static_assert(TqStage::f == TqStage::g_f + TQ_NZ_MAX && TqStage::barrier == TqStage::f + 1 && TqStage::relaxed == TqStage::barrier + 1 && TqStage::viol == TqStage::relaxed + 1,
              "the four sums follow the gradient");
static_assert(TqStage::tau == TqStage::viol + 1 && TqStage::cmpl == TqStage::tau + 7 && TqStage::g_b > TqStage::cmpl && TqStage::J >= TqStage::g_b + TQ_NZ_MAX &&
                  TqStage::J + 7 * TQ_NZ_MAX <= TqStage::size,
              "no two fields of the stage record overlap, the last one ends inside it");
static_assert(TqKnot::dq >= TqKnot::q + 7 && TqKnot::ddq >= TqKnot::dq + 7 && TqKnot::size >= TqKnot::ddq + 7 && TqKnot::pad == 7, "three blocks of up to 7 joints");
static_assert(TqLam::vel >= 2 * 7 && TqLam::size >= TqLam::vel + 2 * 7, "two blocks of 2 N multipliers");
#define TQ_XS TqKnot::size
#define TQ_SD TqStage::size
#define TQ_LAM TqLam::size
#define TQ_HC 232   // per knot: the packed lower triangle of the 3N x 3N curvature term (231 entries at N = 7)
#define TQ_GN 128   // per knot: two doubles per lane of k_tq_step (lane 8 r + c: K_q[r][c], K_dq[r][c]; c = 7: k[r], 0)
static_assert(TQ_HC >= TqStage::g_f, "the curvature term is a packed block of its own");
struct TqParams {
  int T, N, max_iter;
  double dt, w_path, w_vel, w_tau, tol, tol_compl, mu_b0, mu0;
  double theta;      // rows below delta = theta mu_b continue the logarithm by its second-order Taylor polynomial (relaxed barrier)
  double mu_dec;                        // factor on the Levenberg-Marquardt damping after a step whose gain ratio exceeded 0.9 (option tq_mu_dec)
  double kappa_eps, kappa_mu, theta_mu;  // barrier update (Waechter & Biegler 2006, eq. 7): mu_b <- max(mu_min, min(kappa_mu mu_b, mu_b^theta_mu)) once stat <= kappa_eps mu_b
  double curv_from;  // exact Lagrangian curvature in the stage blocks once the reduced gradient is below this ...
  double curv_late;  // ... or below this after curv_after barrier updates (a Gauss-Newton iteration that stalls just above curv_from late in the solve)
  int curv_after;
  int stall_max;     // watchdog: this many steps at one barrier parameter without reaching its test send the instance back to 100 mu_b
  double tau_ftb;    // fraction to the boundary: a step leaves every slack (and multiplier) at least 1 - tau_ftb of itself
  int max_back;      // quarterings of a boundary-shortened step before the damping is raised instead
  int curv_lag;      // exact curvature is evaluated afresh at most every (curv_lag + 1)-th evaluation of an instance, the stored term added in between (option tq_curv_lag; 0: always afresh)
  int ls_curv;       // 1: a rejected Newton step (exact curvature) is quartered like a boundary-shortened one before the damping is raised (option tq_ls_curv)
  double tau_lo[OH_MAX_CHAIN], tau_up[OH_MAX_CHAIN];
  double dq_lo[OH_MAX_CHAIN], dq_up[OH_MAX_CHAIN];  // joint-velocity rows on the velocity states (vel != 0)
  int vel;
  int jac_closed_form;  // d tau / dz in closed form (rnea_idsva) -- the dynamics tables describe a rigid-body chain; 0: dual numbers through the recursion
  int nx, np;
};
// The per-instance scalars and counters, listed ONCE as (type, name, value at setup; P: the TqParams): TqBuffers' [B] arrays, layout_tq's takes (in this
// order: the doubles, then the ints -- the pool's offsets depend on it), TqInst's fields, its load and its store all come from this table.
#define OH_TQ_INST(X)                                                                                                                  \
  X(double, f_cur, 0.0)    /* merit of the accepted point */                                                                           \
  X(double, f_true, 0.0)   /* its cost */                                                                                              \
  X(double, bsum, 0.0)     /* its barrier sum per unit mu_b */                                                                         \
  X(double, mu, P.mu0)     /* Levenberg-Marquardt damping */                                                                           \
  X(double, nun, 4.0)      /* its growth factor */                                                                                     \
  X(double, mub, P.mu_b0)  /* barrier parameter */                                                                                     \
  X(double, stat, 0.0)     /* reduced gradient */                                                                                      \
  X(double, alpha, 1.0)    /* scale of the feed-forward of the pending trial */                                                        \
  X(double, qk, 0.0)       /* q_u^T k of the unit step ... */                                                                          \
  X(double, ndx, 0.0)      /* ... and its |dx|^2: predicted decrease of a scaled step */                                               \
  X(double, viol, 0.0)     /* worst violation of a row at the accepted point */                                                        \
  X(int, cur, 1)           /* slot of the accepted point (the seed sits in slot 0 = the first "trial") */                              \
  X(int, first, 1)         /* the pending trial is accepted as it is */                                                                \
  X(int, curv, 0)          /* exact curvature at the pending evaluation: 1 k_tq_curv computes it, 2 k_tq_eval3 adds the stored term */ \
  X(int, status, -1)                                                                                                                   \
  X(int, iters, 0)                                                                                                                     \
  X(int, rejected, 0)                                                                                                                  \
  X(int, n_barrier, 0)     /* barrier updates so far */                                                                                \
  X(int, nrel, 0)          /* rows of the accepted point inside the relaxed zone */                                                    \
  X(int, n_back, 0)        /* quarterings of the pending step */                                                                       \
  X(int, stall, 0)         /* steps at this barrier parameter without reaching its test */                                             \
  X(int, curv_age, -1)     /* evaluations since the stored curvature term was computed (-1: none stored) */
struct TqBuffers {
  int B;
  const oh_chain* chain;
  const oh_dynamics* dyn;
  double* xs;      // [2][B][T][TQ_XS]
  double* st;      // [2][B][T][TQ_SD]
  double* lam;     // [2][B][T][TQ_LAM]  (slot = the point they were updated at: a rejected trial leaves the accepted point's multipliers alone)
  double* gains;   // [B][T][TQ_GN]
  double* goal;    // [B][T][4]
  double* hc;      // [cap][T][TQ_HC]  the curvature term k_tq_curv last computed for a knot (entries it never writes stay 0)
#define X(type, name, init) type* name;
  OH_TQ_INST(X)  // [B] each
#undef X
  int* n_running;  // [1]
  int* list;       // [B] instances still running when the list was last rebuilt (kernels walk this list: finished instances cost nothing)
  int* n_list;     // [1]
  int n_run;       // length of the list the launches below cover
};
// One instance's scalars in registers: k_tq_setup stores a fresh one, k_tq_step loads one, walks its steps and stores it.
struct TqInst {
#define X(type, name, init) type name;
  OH_TQ_INST(X)
#undef X
  static __device__ __forceinline__ TqInst fresh(const TqParams& P) {
    TqInst S;
#define X(type, name, init) S.name = init;
    OH_TQ_INST(X)
#undef X
    return S;
  }
  static __device__ __forceinline__ TqInst load(const TqBuffers& D, const int b) {
    TqInst S;
#define X(type, name, init) S.name = D.name[b];
    OH_TQ_INST(X)
#undef X
    return S;
  }
  __device__ __forceinline__ void store(const TqBuffers& D, const int b) const {
#define X(type, name, init) D.name[b] = name;
    OH_TQ_INST(X)
#undef X
  }
};
void oh_launch_tq_list(hipStream_t s, const TqBuffers& D);
bool oh_launch_tq_setup(hipStream_t s, const TqParams& P, const TqBuffers& D, const double* x0, const double* p);
bool oh_launch_tq_eval(hipStream_t s, const TqParams& P, const TqBuffers& D);
bool oh_launch_tq_step(hipStream_t s, const TqParams& P, const TqBuffers& D);
bool oh_launch_tq_finalize(hipStream_t s, const TqParams& P, const TqBuffers& D, double* x, double* f, double* kkt, int* iters, int* status, double* mult);
void oh_launch_tq_tick_params(hipStream_t s, int B, int T, int N, int first_row, int n_rows, const double* state, const double* goal_table, double* p);
void oh_launch_tq_shift_seed(hipStream_t s, int B, int T, int N, int advance, const double* x_prev, double* x_seed);
void oh_launch_tq_advance(hipStream_t s, int B, int T, int N, int advance, const double* x, double* state_next, double* tau0);

// ---- OH_PROBLEM_IK -----------------------------------------------------------------------------------------
struct IkParams {
  int ndof, max_iter;
  double w, tol, tol_feas, rho0;
  double lo[OH_MAX_CHAIN], up[OH_MAX_CHAIN];
  double a_tool[3];  // axis goal (oh_ik_set_axis_goal): R_tool times the unit link-frame axis, so that u = R a_tool with fk_chain's R
};
// What the equality rows of an IK handle are, in the values of the "ik_goal" flag.  With nh rows, p rows are [q_nominal; goal] (ndof + nh) and
// multiplier rows nh + 2 ndof:
enum class IkGoal : int {
  Position = 0,  // p_goal: 3 rows
  Pose = 1,      // oh_ik_desc.orientation: [p_goal; quat_goal], 7 rows
  Axis = 2,      // oh_ik_set_axis_goal: [p_goal; u_goal], 6 rows
};
bool oh_launch_ik(hipStream_t s, IkGoal goal, const oh_chain* d_chain, const IkParams& P, int B, const double* x0, const double* p, double* x, double* f,
                  double* kkt, int* iters, int* status, double* mult);

// ---- OH_PROBLEM_QP -----------------------------------------------------------------------------------------
struct QpParams {
  int n, m, me, np, nwork, max_iter;
  double tol;
};
// work: [Q.nwork][Bp] (used when the work set of a block does not fit LDS), or B slices of oh_qp_block_work_doubles when oh_qp_takes_block
// mode: -1 automatic, 0 / 1 / 2 force a work-set placement, 3 forces the block-per-instance kernel (option qp_mode).  Non-zero: *err says why.
int oh_launch_qp_solve(hipStream_t s, const QpParams& Q, int B, int Bp, const double* x0, const double* p, double* work, double* x, double* f, double* kkt,
                       int* iters, int* status, double* mult, int mode, std::string* err);
bool oh_qp_is_large(const QpParams& Q);                  // beyond n = 32, m = 256, me = 32: block-per-instance kernels only
bool oh_qp_takes_block(const QpParams& Q, int mode);     // the solve runs k_qp_solve_block (oh_qp_block.hip)
size_t oh_qp_block_work_doubles(const QpParams& Q);      // per instance: W^T [n][me] and the Schur complement
int oh_launch_qp_solve_block(hipStream_t s, const QpParams& Q, int B, const double* x0, const double* p, double* work, double* x, double* f, double* kkt, int* iters,
                             int* status, double* mult, std::string* err);
// hipFuncAttributeMaxDynamicSharedMemorySize is per device and sticky: asks only when a launch of fn needs more than this device has been granted
// (granted: the kernel's own [64], by device).  false: the request was refused.  (oh_qp.hip)
bool grant_dynamic_lds(const void* fn, size_t bytes, size_t* granted);

// ---- OH_PROBLEM_TAPE ---------------------------------------------------------------------------------------
#define OH_TAPE_ST_CONVERGED OH_STATUS_CONVERGED
#define OH_TAPE_ST_MAX_ITER OH_STATUS_MAX_ITER
#define OH_TAPE_ST_NUMERICAL OH_STATUS_NUMERICAL
#include "oh_tape_solver.h"  // TapeParams, TapeWork and the solver shared by the interpreter and the generated code
#include "oh_tape_ops.h"     // the tape vocabulary: named opcodes, arity, value and adjoint rule of each, liveness
// QP data read off a tape on the device (oh_qp_set_tape): val = [T.len][Bp] work, rows_out = [B][Q.np], f0 = [B]
void oh_launch_qp_assemble(hipStream_t s, const QpParams& Q, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows,
                           const int* xdep, int n_xdep, int B, int Bp, const double* p_raw, double* val, double* rows_out, double* f0);  // xdep: x-dependent instructions
void oh_launch_qp_add_constant(hipStream_t s, int B, double* f, const double* f0);
// the same for handles beyond the old limits: `chunk` (oh_qp_assemble_block_chunk) instances per launch, val = [T.len][chunk * 64]
int oh_qp_assemble_block_chunk(const TapeParams& T, int B);
int oh_launch_qp_assemble_block(hipStream_t s, const QpParams& Q, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows,
                                const int* xdep, int n_xdep, int B, int chunk, const double* p_raw, double* val, double* rows_out, double* f0, std::string* err);
struct TapeJit {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  hipFunction_t fn_lds = nullptr;  // the same kernel with the solver's work arrays in LDS (small batches)
};
// wavefront-per-instance evaluator of trajectory-sized tapes (oh_tape_wave.hip): the level schedule built when the handle is created
struct TapeWave {
  bool ready = false, hist_lds = false, reg_lds = true;  // placement of the last launch: the quasi-Newton pairs / the tape's registers in LDS or in global memory
  bool reg_lds_fits = false, hist_lds_by[2] = {false, false};  // by placement of the registers: [0] global memory, [1] LDS
  size_t lds_bytes_by[2] = {0, 0};
  int reg_choice = -1;  // OH_TAPE_WAVE_REGS: -1 by batch size, 0 global, 1 lds
  int nt = 256;  // threads per instance
  int n_reg = 0, n_fw_pass = 0, n_rv_pass = 0, n_cst = 0, n_par = 0, n_seed = 0, n_seed_rows = 0, seed_cost = -1, n_small = 0, n_levels = 0;
  size_t lds_bytes = 0;
  int4 *d_fw = nullptr, *d_rv = nullptr;
  int *d_cons = nullptr, *d_cst_reg = nullptr, *d_par_reg = nullptr, *d_par_k = nullptr, *d_small = nullptr;
  double *d_cst_val = nullptr, *d_hist = nullptr, *d_regs = nullptr;
  int hist_cap = 0, regs_cap = 0;
  size_t lds_limit = 0;  // what oh_tape_wave_build was given: the product kernel's placement is decided against it per call
};
// nt: threads per instance (256 or 64; option tape_wave_nt), regs: register file -1 chosen per launch, 0 global memory, 1 LDS (tape_wave_regs),
// hist: quasi-Newton pairs -1 in LDS when they fit, 0 global memory (tape_wave_hist)
int oh_tape_wave_build(const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, size_t lds_limit, int nt, int regs,
                       int hist, TapeWave* out, std::string* err);
void oh_tape_wave_release(TapeWave* w);
hipError_t oh_launch_tape_wave(hipStream_t s, TapeWave& W, const TapeParams& T, int B, const double* x0, const double* p, double* x, double* f, double* kkt,
                               int* iters, int* status, double* mult);
// one WaveEval::phi (the level-schedule sweep without tangents) per instance (oh_tape_phi): the register placement oh_launch_tape_wave would choose for this B
hipError_t oh_launch_tape_wave_phi(hipStream_t s, TapeWave& W, const TapeParams& T, int B, const double* x, const double* p, const double* lam, const double* mu,
                                   double rho, double* merit, double* f, double* rowv, double* grad, double* cmax, double* meas);
// the same sweep with tangents and given weights, one block per unit (oh_tape_hvp with option tape_hvp_wave; k_tape_wave_hvp): oh_tape_wave_hvp_place says where
// the four register columns go (0: the interpreter stays, 1: LDS, 2: global memory); a launch covers the units [u0, u0 + n),
// regs (global placement only) is [n][4 n_reg]; x, p, seeds, V (null: the unit vectors), HV and grad (may be null) are the whole batch's arrays
int oh_tape_wave_hvp_place(const TapeWave& W);
size_t oh_tape_wave_hvp_lds_bytes(const TapeWave& W, bool reg_lds);
hipError_t oh_launch_tape_wave_hvp(hipStream_t s, const TapeWave& W, const TapeParams& T, bool reg_lds, int u0, int n, int nv, const double* x, const double* p,
                                   const double* seeds, const double* V, double* regs, double* HV, double* grad);
// truncated Newton-CG on the level schedule, one block per instance (options tape_newton + tape_newton_wave; k_tape_wave_newton): oh_tape_wave_newton_place
// says where the four register columns go (0: the interpreter's kernel stays, 1: LDS, 2: the global register buffer)
int oh_tape_wave_newton_place(const TapeWave& W, const TapeParams& T);
size_t oh_tape_wave_newton_lds_bytes(const TapeParams& T, const TapeWave& W, bool reg_lds);
hipError_t oh_launch_tape_wave_newton(hipStream_t s, TapeWave& W, const TapeParams& T, int place, int B, int cg_cap, const double* x0, const double* p, double* x,
                                      double* f, double* kkt, int* iters, int* status, double* mult, int* stats);
// oh_tape_phi_hvp on such a handle: one k_tape_wave_phi per instance (grad; scratch: [(4 + max(nrows, 1)) B] doubles), then the merit's product by the
// solver's sweep, one block per (instance, direction) (k_tape_wave_merit_hvp)
hipError_t oh_launch_tape_wave_phi_hvp(hipStream_t s, TapeWave& W, const TapeParams& T, int place, int B, int nv, const double* x, const double* p, const double* lam,
                                       const double* mu, double rho, const double* V, double* HV, double* grad, double* scratch);
size_t oh_tape_work_rows(const TapeParams& T, bool jit);
// one InterpEval::phi per instance (oh_tape_phi); work as for oh_launch_tape_solve
void oh_launch_tape_phi(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int B, int Bp,
                        const double* x, const double* p, const double* lam, const double* mu, double rho, double* work, double* merit, double* f, double* rowv,
                        double* grad, double* cmax, double* meas);
void oh_launch_tape_probe(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int B, int Bp,
                          const double* x, const double* p, double* work, int n_regs, const int* regs, double* val, const double* seeds, double* adj, double* grad);
// forward-over-reverse on the interpreter (oh_tape_hvp): the units [u0, u0 + n) of u = instance * nv + direction, one lane each; work is
// [oh_tape_hvp_work_rows][Bp] with Bp >= n; x, p, seeds, V (null: the unit vectors), HV and grad are the whole batch's arrays
size_t oh_tape_hvp_work_rows(const TapeParams& T);  // 4 len + 3 nx
void oh_launch_tape_hvp(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int u0, int n, int Bp,
                        int nv, const double* x, const double* p, const double* seeds, const double* V, double* work, double* HV, double* grad);
// truncated Newton-CG on the interpreter (option tape_newton; oh_tape_newton.h): work is [oh_tape_newton_work_rows][Bp], stats [B][2] (Newton steps, products)
size_t oh_tape_newton_work_rows(const TapeParams& T);  // 4 len + tape_newton_rows
void oh_launch_tape_solve_newton(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int B, int Bp,
                                 int cg_cap, const double* x0, const double* p, double* work, double* x, double* f, double* kkt, int* iters, int* status,
                                 double* mult, int* stats);
// one InterpEval::phi, then nv InterpEval::hess_vec per instance (oh_tape_phi_hvp); work as for oh_launch_tape_solve_newton; grad may be null
void oh_launch_tape_phi_hvp(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int B, int Bp,
                            const double* x, const double* p, const double* lam, const double* mu, double rho, int nv, const double* V, double* work,
                            double* HV, double* grad);
void oh_launch_tape_solve(hipStream_t s, const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, int B, int Bp,
                          const double* x0, const double* p, double* work, double* x, double* f, double* kkt, int* iters, int* status, double* mult);
// solve = false: the program of the single-evaluation kernels (k_tape_jit_phi, k_tape_jit_phi_lds) around the same evaluator text
std::string oh_tape_jit_source(const TapeParams& T, const int* op, const int* a, const int* b, const double* c, const int* rows, bool solve = true);
int oh_tape_jit_compile(const std::string& src, std::vector<char>* code, std::string* err);  // hiprtc for gfx950; needs no device
int oh_tape_jit_load(const std::vector<char>& code, TapeJit* out, std::string* err, bool solve = true);
void oh_tape_jit_forget(const std::string& src);  // drop a cached object that did not load (disk and memory)
void oh_tape_jit_release(TapeJit* j);
hipError_t oh_launch_tape_jit_phi(hipStream_t s, const TapeJit& j, TapeParams T, int B, int Bp, const double* x, const double* p, const double* lam, const double* mu,
                                  double rho, double* work, double* merit, double* f, double* rowv, double* grad, double* cmax, double* meas, int lds_max,
                                  int* used_lds);  // used_lds: whether the launch took the entry with the work set in LDS
hipError_t oh_launch_tape_jit(hipStream_t s, const TapeJit& j, TapeParams T, int B, int Bp, const double* x0, const double* p, double* work, double* x, double* f,
                              double* kkt, int* iters, int* status, double* mult, int lds_max);  // lds_max: the work set in LDS up to this many instances (option tape_lds_max)
