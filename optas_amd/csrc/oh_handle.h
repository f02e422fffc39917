// What the host sources of the C ABI share (oh_api.hip and one oh_api_<family>.hip per family): the handle, the state struct of every
// self-contained family, the typed arguments of a device solve, the options, and the few functions that cross sources.  Host-only, internal.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <map>
#include <string>
#include <vector>

#include "oh_kernels.h"
#include "oh_carve.h"
#include "oh_jit.h"

// the error of this host thread (oh_last_error; defined in oh_api.hip): returns code
int fail(int code, const std::string& msg);

#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess) {                                                                            \
      return fail(OH_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                     \
    }                                                                                                  \
  } while (0)

#define OH_PINNED_STAGE_BYTES (256 * 1024)

// An owned device (or pinned host) array of `cap` elements: grows only, freed by release() and by the destructor.
template <class T, bool PINNED = false>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  operator T*() const { return p; }
  void release() {
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  // room for n elements; *grew (may be null): the array was reallocated, its content is gone.  A failed allocation leaves {nullptr, 0}.
  hipError_t reserve(const size_t n, bool* grew = nullptr) {
    if (grew) *grew = false;
    if (n <= cap) return hipSuccess;
    release();
    const hipError_t e = PINNED ? hipHostMalloc((void**)&p, n * sizeof(T)) : hipMalloc((void**)&p, n * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = n;
    if (grew) *grew = true;
    return hipSuccess;
  }
};

// The arguments of a device solve of B instances, all device pointers: x0 [B][nx], p [B][npar] in; x [B][nx], f [B], kkt [B][3], iters [B],
// status [B] out (f, kkt and iters may be null).  Filled once where a solve enters, then passed down by reference.
struct Solve {
  int B;
  const double *x0, *p;
  double *x, *f, *kkt;
  int *iters, *status;
  // the record of instances [lo, lo + n); a null stays null
  Solve part(const size_t lo, const int n, const Shape& sh) const {
    const auto at = [lo](auto* q, const size_t per) -> decltype(q) { return q ? q + lo * per : nullptr; };
    return {n, at(x0, sh.nx), at(p, sh.npar), at(x, sh.nx), at(f, 1), at(kkt, 3), at(iters, 1), at(status, 1)};
  }
};

// Scheduling state of a handle, set by name through the field-backed options (FIELD_OPTS): a peer takes it over in one assignment.
struct Sched {
  int compaction = 1;
  int compact_carry = 1;     // compaction carries the pending trial along instead of restarting the survivors (k_carry_*)
  int compact_fused = 2;     // ... and the retraction compiled for the chain lays the knots down at their new index itself (oh_spec_retract_move;
                             // 0: k_retract, then k_carry_gather moves them); 2: lean -- hybrid / exact curvature: the accepted knot stays behind
                             // and the gradient moves only where the evaluation reads it (eval_unit<.., MOVE>), and the list-driven copies behind
                             // a sweep are launched only when their list is not empty
  int tail_vel_threshold = 1 << 30;  // ... from this many instances down: always (see locked_loop)
  int lg_split = 1;          // orientation-locked handles with limit rows and no sphere rows: k_retract + k_evalb_lg instead of the fused k_eval_lg (OH_LG_SPLIT=0)
  int tail_vel = 1;          // velocity-limited handles drain in the persistent kernel too (k_tail_vel; OH_TAIL_VEL=0: batched launches to the end)
  int compact_sort = 1;      // order the survivors of a compaction by progress (k_scan_*)
  double compact_frac = 0.97;  // compact the batch once this fraction of it (or less) is still running (0.9 until the carried compaction
                               // stopped copying back: 0.95 ... 0.99 are +1 ... 2 % over 0.9 on two boxes, interleaved runs)
  double compact_frac_restart = 0.9;  // the same for the compaction that restarts the survivors (guarded handles, free family): it costs an evaluation
  int tail_threshold = 16384;  // hand the last instances to the persistent one-wave-per-instance kernel (round 2: with the kernel compiled for the
                               // chain 8192 against 2048 was +1.3 ... 3 % at B = 262 144 and -21 % on a batch of 4096; with four of its blocks per CU
                               // (two-pass exchange, 40 KB of LDS) 16 384 is level at B = 262 144 and -6 ... 13 % on batches of 16 ... 24 k)
  int sparse_check_below = 2048;  // OH_SPARSE_CHECK_BELOW (0: look every iteration whatever the batch)
  int fuse_couple = 1;        // OH_FUSE_COUPLE=0 restores the three-kernel iteration (k_couple between evaluation and sweep) for A/B runs
  int free_pcr_max = 1536;    // position-tracking family: K3 by cyclic reduction, one block per instance, while at most this many are in the launch
  int specialize = OH_SPECIALIZE_AUTO;  // option "specialize": 0 never, 1 at the first solve, 2 auto: at the first solve of >= specialize_min_B instances
  int tq_check = 4;  // the host looks at the running count every tq_check iterations
  std::array<double, 4> inv_saved{1.0, 16384.0, 1.0, -2.0};  // compaction, tail_threshold, tail_vel, free_persist (-2: unset) as they were before batch_invariant
};

// The last successful solve or rollout of a handle: B, and where each instance's multipliers live -- on the handles of `parts` (n instances
// each, in instance order) or, after a pipelined oh_solve, in the handle's d_pipe_mult.  Cleared by every entry that solves and by drop_peers.
struct oh_handle;
struct LastSolve {
  struct Part { const oh_handle* q; int n; };
  int B = 0;
  std::vector<Part> parts;
  bool pipe_cache = false;
};

// ---- state of the self-contained families: a handle is of one kind and uses one of these (a QP handle with oh_qp_set_tape: qp and tape) ----

// Tape family (oh_api_tape.hip)
struct TapeState {
  TapeParams P{};
  DevBuf<int> op, a, b, rows;
  DevBuf<double> c;
  DevBuf<double> work;   // [oh_tape_work_rows][cap()]; grows with mult
  DevBuf<double> mult;   // [n_ineq + n_eq + 1][cap()]
  DevBuf<double> h0;     // oh_tape_set_metric: initial metric of the limited-memory form [nx][nx]
  int cap() const { return (int)(mult.cap / (size_t)(P.n_ineq + P.n_eq + 1)); }  // instances the two work arrays hold: their row stride
  TapeJit jit;
  TapeJit jit_phi;   // the single-evaluation kernels of the same generated evaluator: compiled by the first oh_tape_phi, not with the handle
  int phi_lds = 0;   // whether the last oh_tape_phi ran the generated code's entry with the work set in LDS
  int hvp_launches = 0;  // launches the last oh_tape_hvp took (oh_get_flag "tape_hvp_launches")
  int hvp_path = 0;      // what they ran: 0 k_tape_hvp, 1 / 2 k_tape_wave_hvp with its registers in LDS / in global memory ("tape_hvp_path")
  DevBuf<int> nstat;     // [nstat_B][2]: Newton steps and Hessian-vector products of every instance of the last Newton-CG solve (oh_tape_newton_stats)
  int nstat_B = 0;
  int last_newton = 0;   // the last solve ran a Newton-CG kernel (oh_get_flag "tape_newton")
  int newton_path = 0;   // what the last Newton-CG solve or oh_tape_phi_hvp ran: 0 the interpreter (k_tape_solve_newton, k_tape_phi_hvp), 1 / 2 the level
                         // schedule (k_tape_wave_newton, k_tape_wave_merit_hvp) with its registers in LDS / in global memory ("tape_newton_path")
  TapeWave wave;     // trajectory-sized tapes: one wavefront per instance (oh_tape_wave.hip)
  // host copy of the tape of an OH_PROBLEM_TAPE handle: the evaluator is rebuilt when an option that shapes it changes (tape_wave, tape_lbfgs, ...)
  std::vector<int> h_op, h_a, h_b, h_rows;
  std::vector<double> h_c;
  oh_tape_desc desc{};
};

// Dense QP family (oh_api_qp.hip)
struct QpState {
  oh_qp_desc desc{};
  DevBuf<double> work;    // [Q.nwork][Bp]
  DevBuf<double> mult;    // [m + me + 1][Bp]
  DevBuf<double> blk;     // k_qp_solve_block: [B][me n + me^2] (oh_qp_block_work_doubles), a contiguous slice per instance
  int last_block = 0;     // the last solve ran k_qp_solve_block (oh_get_flag "qp_block")
  bool use_tape = false;  // oh_qp_set_tape: p of a solve is the problem's parameter vector, the QP data is read off the tape (the handle's TapeState) on the device
  // the three grow together (qp_solve_device): [Bv][qp_np] assembled [P | q | M | c | A | b]; [tape.P.len][Bv] registers of the tape interpreter (large
  // handles: [tape.P.len][64 x instances per launch of k_qp_assemble_block]); [Bv] f(0, p)
  DevBuf<double> rows, val, f0;
  DevBuf<int> xdep;       // indices of the tape's x-dependent instructions
  int n_xdep = 0;
};

// Inverse-kinematics family (oh_api_ik.hip)
struct IkState {
  oh_ik_desc desc{};
  DevBuf<double> mult;  // [B][ik_rows + 2 ndof]
  bool axis_goal = false;  // oh_ik_set_axis_goal: position rows plus three rows on a link axis
  double axis_link[3] = {0.0, 0.0, 0.0};  // that axis in the link frame, unit length
  bool solved = false;  // a solve has been launched: the goal shape is fixed from then on
};
// which goal a handle has, read here and nowhere else (oh_ik_set_axis_goal refuses a handle with a full-pose goal, so the two do not meet)
inline IkGoal ik_goal(const IkState& s) { return s.axis_goal ? IkGoal::Axis : s.desc.orientation ? IkGoal::Pose : IkGoal::Position; }
// equality rows of an IK handle; p rows are ndof + ik_rows wide, multiplier rows ik_rows + 2 ndof
inline size_t ik_rows(const IkState& s) {
  switch (ik_goal(s)) {
    case IkGoal::Pose: return 7;
    case IkGoal::Axis: return 6;
    default: return 3;
  }
}

// Torque-MPC family (oh_api_torque.hip)
struct TqState {
  oh_torque_desc desc{};
  TqParams P{};
  TqBuffers D{};
  // the three grow together (tq_solve_device): the pool of layout_tq; [B][T][4 ndof] multipliers; [B][T][TQ_HC] stored curvature terms (k_tq_curv)
  DevBuf<char> pool;
  DevBuf<double> mult, hc;
};

// Point-mass family (oh_api_pointmass.hip)
struct PmState {
  oh_pointmass_desc desc{};
  PmParams P{};
  PmBuffers D{};
  DevBuf<char> pool;  // layout_pm, carved for a row stride of cap_B
  int cap_B = 0;
};

struct oh_handle {
  // ---- every kind: description, device, stream, events, options, staging, the record of the last solve, timing ----
  oh_problem_desc desc;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evt0 = nullptr, evt1 = nullptr;
  Sched sch;
  // options set by name (oh_set_option; OH_DEBUG_OPTIONS at creation) that are not backed by a field of sch: read with optv() where they are used
  std::map<std::string, double> opt;
  // staging for the host-buffer entry points, and its pinned mirror for small oh_solve calls (OH_PINNED_STAGE_BYTES)
  DevBuf<char> stage;
  DevBuf<char, true> h_stage;
  LastSolve last;  // where the results of the last successful solve live (oh_get_multipliers)
  bool profiling = false;
  std::vector<hipEvent_t> prof_events;
  std::vector<int> prof_tags;  // per recorded event: 0 base marker, 1 after eval, 2 after step
  double timing[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double timing_couple = 0;
  double rejects = 0;
  double tail_iters = 0;
  double rescued = 0, grad_moved = 0, lanes_moved = 0;  // lean carried compactions: instances through the rescue list; instances whose gradient moved, of these moved
  DevBuf<int, true> h_flag;  // pinned
  // ---- constants: the chain (every kind that takes one), the two chains of oh_link_kin*, the inverse-dynamics tables ----
  bool have_chain = false;
  oh_chain chain_host;
  DevBuf<oh_chain> d_chain;
  bool have_frames = false;  // oh_set_link_frames: independent of the chain above
  OhLinkFrames frames_host;
  DevBuf<OhLinkFrames> d_frames;
  bool have_dyn = false;
  oh_dynamics dyn_host;
  DevBuf<oh_dynamics> d_dyn;
  const FkSpec* fk_spec = nullptr;  // K1 compiled for this chain (any handle with constants)
  bool fk_spec_failed = false;
  int specialize_min_units = 1 << 16;
  // ---- the self-contained families ----
  TapeState tape;
  QpState qp;
  IkState ik;
  TqState tq;
  PmState pm;
  // ---- trajectory families (oh_api.hip) ----
  std::vector<double> local_path;
  DevBuf<double> d_local_path;
  int cap_B = 0;
  FigBuffers D{};
  FigParams P{};
  DevBuf<char> pool;  // layout_fig, carved for a row stride of cap_B
  // inequality rows of the position-tracking family
  bool have_guards = false;
  oh_guards guards{};
  GuardParams GP{};
  GuardBuffers GB{};
  DevBuf<char> gpool;
  int gcap = 0;              // the row stride (D.Bp) the guard pool was carved for
  DevBuf<char> move_scr;     // scratch of the compaction that moves every array (move_everything)
  int free_sweep_last = -1;    // position-tracking family: the FreeSweep the last solve started with (oh_get_flag "free_sweep"; -1: none yet)
  int free_sweeps_used = 0;    // ... and bit (1 << FreeSweep) of every sweep its loop used, those chosen after compactions included ("free_sweeps_used")
  // run-time specialised evaluation kernels of the orientation-locked figure-eight family (oh_jit.hip)
  int specialize_min_B = 4096;
  const FigSpec* spec = nullptr;
  bool spec_failed = false;
  bool spec_move_failed = false;  // the moving retraction did not launch once: this handle's carried compactions gather as before
  bool spec_cache_checked = false;  // automatic mode has looked for a cached code object once (reset with the constants)
  double spec_seconds = 0.0;  // of the last oh_specialize
  // a large batch of the trajectory and torque families is solved in parts on handles (streams, host threads) of their own: solve_split
  std::vector<oh_handle*> peers;
  DevBuf<double> d_pipe_mult;    // multipliers of every chunk of a pipelined oh_solve, in instance order
  bool is_peer = false;          // this handle is a lane of another one (fan_out): it never fans out itself
  // the lanes first, then everything this handle launched has to be over before its events, the tape's modules, stream and (the DevBuf members) memory go
  ~oh_handle() {
    for (oh_handle* p : peers) delete p;
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    for (hipEvent_t e : prof_events) hipEventDestroy(e);
    for (hipEvent_t e : {ev0, ev1, evt0, evt1})
      if (e) hipEventDestroy(e);
    oh_tape_jit_release(&tape.jit);
    oh_tape_jit_release(&tape.jit_phi);
    oh_tape_wave_release(&tape.wave);
    if (stream) hipStreamDestroy(stream);
  }
};

// ---- per-handle options ----------------------------------------------------------------------------------------------------------------
// Every knob is an option of ONE handle, set by name; the single environment hook is OH_DEBUG_OPTIONS ("name=value,name=value"), applied to
// every handle when it is created (tools/, A/B runs).
struct OptDoc { const char* name; double dflt; };
// map-backed options and their defaults, the one place a default is written (field-backed ones: FIELD_OPTS; batch_invariant: set_option_impl)
static constexpr OptDoc OPT_TABLE[] = {
    {"check_every", 1},        {"lean_count", 0},        {"row_pad", 13},          {"retract_min", 1e-13}, {"hyb_switch", 1e-5},   {"relax", 1.5},          {"relax_from", 4},         {"settle_k", 1.0},   {"al_fuse", 1},   {"streams", 2},         {"split_min", 65536},  {"tq_split_min", 1024}, {"free_split_min", 256},
    {"free_bb", 1},            {"free_persist", -1},     {"free_cp_max", 512},   {"pm_wave_max", 20480}, {"qp_mode", -1},         {"tape_lds_max", 1 << 30}, {"tape_hvp_work_mb", 256}, {"tape_hvp_wave", 0},
    {"tape_newton", 0},        {"tape_newton_cg", -1},   {"tape_newton_wave", 0},
    {"tape_wave", 1},          {"tape_lbfgs", -1},       {"tape_wave_nt", 256},  {"tape_wave_regs", -1}, {"tape_wave_hist", -1},  {"tq_stall", 25},
    {"tq_curv_after", 3},      {"tq_ftb", 0.995},        {"tq_theta_mu", 1.35},  {"tq_kappa_mu", 0.4},   {"tq_curv_from", 0.1},   {"tq_jac_dual", 0},
    {"tq_rebuild", 0.9},         {"compact_move_all", 1},  {"tq_curv_late", 1.0},  {"tq_kappa_eps", 10.0}, {"tq_max_back", 3},     {"tq_mu_dec", 1.0 / 3.0},     {"tq_ls_curv", 1},   {"tq_mu_dec_warm", 0.1}, {"tq_curv_lag", 3},
    {"tol", 0},                {"pipe", 1},               {"pipe_chunk", 32768},                {"invariant_compact_frac", 0.65}, {"invariant_split", 1}, {"invariant_move_slim", 1}, {"invariant_move_live", 1},
};
// row of a map-backed option in OPT_TABLE (-1: none)
constexpr int opt_row(const char* name) {
  for (int i = 0; i < (int)(sizeof(OPT_TABLE) / sizeof(OPT_TABLE[0])); ++i) {
    int k = 0;
    while (OPT_TABLE[i].name[k] && OPT_TABLE[i].name[k] == name[k]) ++k;
    if (OPT_TABLE[i].name[k] == name[k]) return i;
  }
  return -1;
}
template <int ROW>
constexpr int known_opt() {
  static_assert(ROW >= 0, "optv: the option is not in OPT_TABLE");
  return ROW;
}
// an option of a handle: as set by name, else its default in the table
inline double opt_value(const oh_handle* h, const OptDoc& d) {
  const auto it = h->opt.find(d.name);
  return it == h->opt.end() ? d.dflt : it->second;
}
// optv(h, "name"): a map-backed option of a handle; a name that is not in OPT_TABLE does not compile
#define optv(h, name) opt_value(h, OPT_TABLE[known_opt<opt_row(name)>()])
// option batch_invariant: kept in the map but outside the table (set_option_impl parks the scheduling fields it overrides); 0 until set
inline double batch_invariant(const oh_handle* h) {
  const auto it = h->opt.find("batch_invariant");
  return it == h->opt.end() ? 0.0 : it->second;
}

// ---- oh_api.hip: what every family's source uses ------------------------------------------------------------------------------------------
// What every oh_create* does once its description is checked: a device must be there; a fresh handle on the current device with a stream, the four
// events and -- by `want` -- the device copy of the chain and the pinned flag.  nullptr: *rc is the code, oh_last_error says why.
enum { OPEN_CHAIN = 1, OPEN_FLAG = 2 };
oh_handle* open_handle(const std::string& who, int kind, int T, int ndof, int want, int* rc);
// every solve reports counters of its own only (oh_get_timing)
void reset_counters(oh_handle* h);
// the tail every solve shares: wait for the launches since ev0, report a launch error, time the solve ([4]) and count its launches ([5])
int finish_solve(oh_handle* h, double launched);
// Shape (oh_carve.h) of a handle's problem; zeros: a handle without a problem
Shape shape_of(const oh_handle* h);
// the chain covers every model joint in order (what the solvers need)
bool solver_chain_ok(const oh_chain& c);
int validate_chain(const oh_handle* h, const oh_chain& c);
// the handle has new constants: everything compiled for, or remembered about, the previous chain goes
void adopt_chain(oh_handle* h, const oh_chain& c);
// a setter changed what the peers were built from: they, and the record of the last solve, go
void drop_peers(oh_handle* h);
int ensure_stage(oh_handle* h, size_t bytes);
// The staging area of a host-buffer entry point: layout(Carver) is its one list of takes, each a 256-byte slot, and returns the carver's bytes().
// It runs on a null base to size the area, then on the area itself.
template <class Layout>
int stage_carve(oh_handle* h, Layout&& layout) {
  if (const int rc = ensure_stage(h, layout(Carver(nullptr, Carver::Slots)))) return rc;
  layout(Carver(h->stage.p, Carver::Slots));
  return OH_OK;
}

// ---- the families: what solve_device, shape_of and the options call -------------------------------------------------------------------------
int tape_solve_device(oh_handle* h, const Solve& a);
int qp_solve_device(oh_handle* h, const Solve& a);
int ik_solve_device(oh_handle* h, const Solve& a);
int pm_solve_device(oh_handle* h, const Solve& a);
int tq_solve_device(oh_handle* h, const Solve& a, double mu_b0_warm = 0.0);  // mu_b0_warm > 0: a warm-started tick of oh_tq_rollout
int tape_validate(const oh_tape_desc* d, const char* who);
TapeParams tape_params(const oh_tape_desc* d, int lbfgs_opt = -1);
int tape_configure(oh_handle* h);
int upload_tape(oh_handle* h, const oh_tape_desc* d, const int* op_override);
size_t qp_np(const oh_qp_desc& q);
int specialize_fk(oh_handle* h);
