// C ABI of liboptas_hip.so (see include/optas_hip.h).  Host-side orchestration only: buffer
// ownership, the SQP launch loop (eval kernel + Riccati/step kernel per iteration), HIP-event timing.
// Memory: every device or pinned allocation of a handle is a DevBuf member (grow-only, freed by the handle's destructor); what lives inside a pool
// or the staging area is laid out by ONE list of Carver takes (oh_carve.h) that both measures and carves it.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is opened with dlopen when a communicator is first asked for

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "oh_kernels.h"
#include "oh_carve.h"
#include "oh_jit.h"
#include "oh_rnea.h"

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

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

// Scheduling state of a handle, set by name through the field-backed options (FIELD_OPTS): a peer takes it over in one assignment.
struct Sched {
  int compaction = 1;
  int compact_carry = 1;     // compaction carries the pending trial along instead of restarting the survivors (k_carry_*)
  int compact_fused = 1;     // ... and the retraction compiled for the chain lays the knots down at their new index itself (oh_spec_retract_move;
                             // 0: k_retract, then k_carry_gather moves them)
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

struct oh_handle {
  oh_problem_desc desc;
  std::vector<double> local_path;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evt0 = nullptr, evt1 = nullptr;
  bool have_chain = false;
  oh_chain chain_host;
  DevBuf<oh_chain> d_chain;
  bool have_frames = false;  // oh_set_link_frames: the two chains of oh_link_kin*, independent of the chain above
  OhLinkFrames frames_host;
  DevBuf<OhLinkFrames> d_frames;
  bool have_dyn = false;
  oh_dynamics dyn_host;
  DevBuf<oh_dynamics> d_dyn;
  DevBuf<double> d_local_path;
  // point-mass family
  oh_pointmass_desc pm{};
  PmParams PmP{};
  PmBuffers PmD{};
  // inequality rows of the position-tracking family
  bool have_guards = false;
  oh_guards guards{};
  GuardParams GP{};
  GuardBuffers GB{};
  DevBuf<char> gpool;
  int gcap = 0;              // the row stride (D.Bp) the guard pool was carved for
  DevBuf<char> move_scr;     // scratch of the compaction that moves every array (move_everything)
  // tape family
  TapeParams TP{};
  DevBuf<int> d_tape_op, d_tape_a, d_tape_b, d_tape_rows;
  DevBuf<double> d_tape_c;
  DevBuf<double> d_tape_work;   // [oh_tape_work_rows][tape_cap]; grows with d_tape_mult
  DevBuf<double> d_tape_mult;   // [n_ineq + n_eq + 1][tape_cap]
  DevBuf<double> d_tape_h0;     // oh_tape_set_metric: initial metric of the limited-memory form [nx][nx]
  int tape_cap() const { return (int)(d_tape_mult.cap / (size_t)(TP.n_ineq + TP.n_eq + 1)); }  // instances the two work arrays hold: their row stride
  TapeJit tape_jit;
  TapeJit tape_jit_phi;       // the single-evaluation kernels of the same generated evaluator: compiled by the first oh_tape_phi, not with the handle
  int tape_phi_lds = 0;       // whether the last oh_tape_phi ran the generated code's entry with the work set in LDS
  TapeWave tape_wave;  // trajectory-sized tapes: one wavefront per instance (oh_tape_wave.hip)
  // dense QP family
  oh_qp_desc qp{};
  DevBuf<char, true> h_stage;  // pinned mirror of the staging area for small oh_solve calls (OH_PINNED_STAGE_BYTES)
  DevBuf<double> d_qp_work;    // [Q.nwork][Bp]
  DevBuf<double> d_qp_mult;    // [m + me + 1][Bp]
  DevBuf<double> d_qp_blk;     // k_qp_solve_block: [B][me n + me^2] (oh_qp_block_work_doubles), a contiguous slice per instance
  int qp_last_block = 0;       // the last solve ran k_qp_solve_block (oh_get_flag "qp_block")
  int free_sweep_last = -1;    // position-tracking family: the FreeSweep the last solve started with (oh_get_flag "free_sweep"; -1: none yet)
  int free_sweeps_used = 0;    // ... and bit (1 << FreeSweep) of every sweep its loop used, those chosen after compactions included ("free_sweeps_used")
  bool qp_tape = false;       // oh_qp_set_tape: p of a solve is the problem's parameter vector, the QP data is read off the tape (h->TP, d_tape_*) on the device
  // the three grow together (qp_solve_device): [Bv][qp_np] assembled [P | q | M | c | A | b]; [TP.len][Bv] registers of the tape interpreter (large
  // handles: [TP.len][64 x instances per launch of k_qp_assemble_block]); [Bv] f(0, p)
  DevBuf<double> d_qp_rows, d_qp_val, d_qp_f0;
  DevBuf<int> d_qp_xdep;        // indices of the tape's x-dependent instructions
  int qp_n_xdep = 0;
  // inverse-kinematics family
  oh_ik_desc ik{};
  DevBuf<double> d_ik_mult;  // [B][3 + 2 ndof]
  // torque-MPC family
  oh_torque_desc tq{};
  TqParams TqP{};
  TqBuffers TqD{};
  // the three grow together (tq_solve_device): the pool of layout_tq; [B][T][4 ndof] multipliers; [B][T][TQ_HC] stored curvature terms (k_tq_curv)
  DevBuf<char> tq_pool;
  DevBuf<double> d_tq_mult, d_tq_hc;
  // solver buffers
  int cap_B = 0;
  FigBuffers D{};
  FigParams P{};
  DevBuf<char> pool;  // layout_fig, or (point-mass handles) layout_pm, carved for a row stride of cap_B
  LastSolve last;  // where the results of the last successful solve live (oh_get_multipliers)
  // staging for the host-buffer entry points
  DevBuf<char> stage;
  // profiling
  bool profiling = false;
  std::vector<hipEvent_t> prof_events;
  double timing[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double timing_couple = 0;
  double rejects = 0;
  double tail_iters = 0;
  DevBuf<int, true> h_flag;  // pinned
  // a large batch of the plain orientation-locked family is solved in parts on handles (streams, host threads) of their own: solve_split
  std::vector<oh_handle*> peers;
  DevBuf<double> d_pipe_mult;    // multipliers of every chunk of a pipelined oh_solve, in instance order
  bool is_peer = false;          // this handle is a lane of another one (fan_out): it never fans out itself
  Sched sch;
  // run-time specialised evaluation kernels of the orientation-locked figure-eight family (oh_jit.hip)
  int specialize_min_B = 4096;
  const FigSpec* spec = nullptr;
  bool spec_failed = false;
  bool spec_move_failed = false;  // the moving retraction did not launch once: this handle's carried compactions gather as before
  bool spec_cache_checked = false;  // automatic mode has looked for a cached code object once (reset with the constants)
  const FkSpec* fk_spec = nullptr;  // K1 for this chain (any handle with constants)
  bool fk_spec_failed = false;
  int specialize_min_units = 1 << 16;
  double spec_seconds = 0.0;  // of the last oh_specialize
  std::vector<int> prof_tags;  // per recorded event: 0 base marker, 1 after eval, 2 after step
  // options set by name (oh_set_option; OH_DEBUG_OPTIONS at creation) that are not backed by a field above: read with optv() where they are used
  std::map<std::string, double> opt;
  // host copy of the tape of an OH_PROBLEM_TAPE handle: the evaluator is rebuilt when an option that shapes it changes (tape_wave, tape_lbfgs, ...)
  std::vector<int> t_op, t_a, t_b, t_rows;
  std::vector<double> t_c;
  oh_tape_desc t_desc{};
  // the lanes first, then everything this handle launched has to be over before its events, modules, stream and (the DevBuf members) memory go
  ~oh_handle() {
    for (oh_handle* p : peers) delete p;
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    for (hipEvent_t e : prof_events) hipEventDestroy(e);
    for (hipEvent_t e : {ev0, ev1, evt0, evt1})
      if (e) hipEventDestroy(e);
    oh_tape_jit_release(&tape_jit);
    oh_tape_jit_release(&tape_jit_phi);
    oh_tape_wave_release(&tape_wave);
    if (stream) hipStreamDestroy(stream);
  }
};

extern "C" int oh_specialize(oh_handle* h);
static bool spec_applies(const oh_handle* h);
static bool spec_tail_vel_applies(const oh_handle* h);
static int specialize_fk(oh_handle* h);
extern "C" const char* oh_last_error(void) { return g_err.c_str(); }
extern "C" const char* oh_version(void) { return "optas_hip 0.2 (gfx950)"; }
extern "C" int oh_abi_version(void) { return OH_ABI_VERSION; }

// ---- per-handle options (round 5) ----------------------------------------------------------------------------------------------------
// Until round 4 forty OH_* environment variables were read inside the library: two handles of one process could not differ and a result
// depended on the caller's environment.  Now every knob is an option of ONE handle, set by name; the single environment hook left is
// OH_DEBUG_OPTIONS ("name=value,name=value"), applied to every handle when it is created (tools/, A/B runs).
struct OptDoc { const char* name; double dflt; };
// map-backed options and their defaults, the one place a default is written (field-backed ones: FIELD_OPTS; batch_invariant: set_option_impl)
static constexpr OptDoc OPT_TABLE[] = {
    {"check_every", 1},        {"row_pad", 13},          {"retract_min", 1e-13}, {"hyb_switch", 1e-5},   {"relax", 1.5},          {"relax_from", 4},         {"settle_k", 1.0},   {"al_fuse", 1},   {"streams", 2},         {"split_min", 65536},  {"tq_split_min", 1024}, {"free_split_min", 256},
    {"free_bb", 1},            {"free_persist", -1},     {"free_cp_max", 512},   {"pm_wave_max", 20480}, {"qp_mode", -1},         {"tape_lds_max", 1 << 30},
    {"tape_wave", 1},          {"tape_lbfgs", -1},       {"tape_wave_nt", 256},  {"tape_wave_regs", -1}, {"tape_wave_hist", -1},  {"tq_stall", 25},
    {"tq_curv_after", 3},      {"tq_ftb", 0.995},        {"tq_theta_mu", 1.35},  {"tq_kappa_mu", 0.4},   {"tq_curv_from", 0.1},   {"tq_jac_dual", 0},
    {"tq_rebuild", 0.9},         {"compact_move_all", 1},  {"tq_curv_late", 1.0},  {"tq_kappa_eps", 10.0}, {"tq_max_back", 3},     {"tq_mu_dec", 1.0 / 3.0},     {"tq_ls_curv", 1},   {"tq_mu_dec_warm", 0.1}, {"tq_curv_lag", 3},
    {"tol", 0},                {"pipe", 1},               {"pipe_chunk", 32768},                {"invariant_compact_frac", 0.65}, {"invariant_split", 1}, {"invariant_move_slim", 1}, {"invariant_move_live", 1},
};
// row of a map-backed option in OPT_TABLE (-1: none)
static constexpr int opt_row(const char* name) {
  for (int i = 0; i < (int)(sizeof(OPT_TABLE) / sizeof(OPT_TABLE[0])); ++i) {
    int k = 0;
    while (OPT_TABLE[i].name[k] && OPT_TABLE[i].name[k] == name[k]) ++k;
    if (OPT_TABLE[i].name[k] == name[k]) return i;
  }
  return -1;
}
template <int ROW>
static constexpr int known_opt() {
  static_assert(ROW >= 0, "optv: the option is not in OPT_TABLE");
  return ROW;
}
// an option of a handle: as set by name, else its default in the table
static double opt_value(const oh_handle* h, const OptDoc& d) {
  const auto it = h->opt.find(d.name);
  return it == h->opt.end() ? d.dflt : it->second;
}
// optv(h, "name"): a map-backed option of a handle; a name that is not in OPT_TABLE does not compile
#define optv(h, name) opt_value(h, OPT_TABLE[known_opt<opt_row(name)>()])
// option batch_invariant: kept in the map but outside the table (set_option_impl parks the scheduling fields it overrides); 0 until set
static double batch_invariant(const oh_handle* h) {
  const auto it = h->opt.find("batch_invariant");
  return it == h->opt.end() ? 0.0 : it->second;
}
// field-backed options: the one list of name -> field of Sched that oh_set_option and oh_get_option read (a flag stores v != 0)
struct FieldOpt {
  const char* name;
  int Sched::*i;
  double Sched::*d = nullptr;
  bool flag = false;
  double get(const Sched& s) const { return d ? s.*d : s.*i; }
  void set(Sched& s, const double v) const { if (d) s.*d = v; else s.*i = flag ? v != 0.0 : (int)v; }
};
static const FieldOpt FIELD_OPTS[] = {
    {"tail_threshold", &Sched::tail_threshold}, {"free_pcr_max", &Sched::free_pcr_max}, {"compaction", &Sched::compaction, nullptr, true},
    {"compact_frac", nullptr, &Sched::compact_frac}, {"compact_sort", &Sched::compact_sort}, {"compact_carry", &Sched::compact_carry},
    {"compact_fused", &Sched::compact_fused, nullptr, true},
    {"tail_vel", &Sched::tail_vel}, {"lg_split", &Sched::lg_split}, {"tail_vel_threshold", &Sched::tail_vel_threshold},
    {"fuse_couple", &Sched::fuse_couple, nullptr, true}, {"sparse_check_below", &Sched::sparse_check_below}, {"specialize", &Sched::specialize},
    {"tq_check", &Sched::tq_check},
};
static const FieldOpt* field_opt(const std::string& name) {
  for (const FieldOpt& f : FIELD_OPTS)
    if (name == f.name) return &f;
  return nullptr;
}
static int tape_configure(oh_handle* h);
static int set_option_impl(oh_handle* h, const std::string& name, double v) {
  Sched& sc = h->sch;
  if (name == "compact_frac") sc.compact_frac = sc.compact_frac_restart = v;
  else if (name == "specialize") sc.specialize = v == 0.0 ? OH_SPECIALIZE_NEVER : (v == 1.0 ? OH_SPECIALIZE_ALWAYS : OH_SPECIALIZE_AUTO);
  else if (name == "tq_check") sc.tq_check = v >= 1.0 ? (int)v : 1;
  else if (name == "batch_invariant") {
    // every instance takes the batched launches to the end, nothing restarts, nothing is handed to the persistent kernel; the batch is compacted only
    // by moving a survivor with everything it owns (move_everything): the path of an instance is then a function of the instance alone, bit for bit
    // (the price: 1.3 x the device time of a 262 144 batch -- 3.0 x before the moving compaction --, and small batches pay launches)
    // (the scheduling fields the option overrides are parked and come back when it is switched off: a threshold the user set earlier is not replaced
    //  by the default -- ADVICE r5)
    const bool was = batch_invariant(h) != 0.0;
    h->opt[name] = v;
    if (v != 0.0 && !was) {
      sc.inv_saved = {sc.compaction ? 1.0 : 0.0, (double)sc.tail_threshold, (double)sc.tail_vel, h->opt.count("free_persist") ? h->opt["free_persist"] : -2.0};
      sc.compaction = false; sc.tail_threshold = 0; sc.tail_vel = 0; h->opt["free_persist"] = 0;
    } else if (v == 0.0 && was) {
      sc.compaction = sc.inv_saved[0] != 0.0; sc.tail_threshold = (int)sc.inv_saved[1]; sc.tail_vel = (int)sc.inv_saved[2];
      if (sc.inv_saved[3] == -2.0) h->opt.erase("free_persist"); else h->opt["free_persist"] = sc.inv_saved[3];
    }
  } else if (const FieldOpt* f = field_opt(name)) f->set(sc, v);
  else {
    bool known = false;
    for (const OptDoc& d : OPT_TABLE) known = known || name == d.name;
    if (!known) return fail(OH_ERR_INVALID, "oh_set_option: unknown option '" + name + "'");
    h->opt[name] = v;
    if (h->desc.kind == OH_PROBLEM_TAPE && !h->t_op.empty() && name.rfind("tape_", 0) == 0 && name != "tape_lds_max") return tape_configure(h);
  }
  return OH_OK;
}
extern "C" int oh_set_option(oh_handle* h, const char* name, double value) {
  if (!h || !name) return fail(OH_ERR_INVALID, "oh_set_option: null argument");
  return set_option_impl(h, name, value);
}
extern "C" int oh_get_option(oh_handle* h, const char* name, double* value) {
  if (!h || !name || !value) return fail(OH_ERR_INVALID, "oh_get_option: null argument");
  const std::string n(name);
  if (n == "batch_invariant") *value = batch_invariant(h);
  else if (const FieldOpt* f = field_opt(n)) *value = f->get(h->sch);
  else {
    for (const OptDoc& d : OPT_TABLE)
      if (n == d.name) { *value = opt_value(h, d); return OH_OK; }
    return fail(OH_ERR_INVALID, "oh_get_option: unknown option '" + n + "'");
  }
  return OH_OK;
}
// OH_DEBUG_OPTIONS="name=value,name=value": the one environment hook of the library, applied to a handle when it is created
static int apply_debug_options(oh_handle* h) {
  const char* e = getenv("OH_DEBUG_OPTIONS");
  if (!e || !*e) return OH_OK;
  std::string str(e);
  size_t pos = 0;
  while (pos < str.size()) {
    size_t end = str.find_first_of(",;", pos);
    if (end == std::string::npos) end = str.size();
    const std::string item = str.substr(pos, end - pos);
    pos = end + 1;
    if (item.empty()) continue;
    const size_t eq = item.find('=');
    if (eq == std::string::npos) return fail(OH_ERR_INVALID, "OH_DEBUG_OPTIONS: expected name=value, got '" + item + "'");
    char* endp = nullptr;
    const std::string val = item.substr(eq + 1);
    const double v = strtod(val.c_str(), &endp);
    if (endp == val.c_str()) return fail(OH_ERR_INVALID, "OH_DEBUG_OPTIONS: '" + item + "' has no numeric value");
    if (const int rc = set_option_impl(h, item.substr(0, eq), v)) return rc;
  }
  return OH_OK;
}
// every oh_create*: a fresh handle with the debug options applied (nullptr: a bad OH_DEBUG_OPTIONS, oh_last_error says which)
static oh_handle* new_handle() {
  oh_handle* h = new oh_handle();
  if (apply_debug_options(h) != OH_OK) {
    delete h;
    return nullptr;
  }
  return h;
}

// What every oh_create* does once its description is checked: a device must be there; a fresh handle on the current device with a stream, the four
// events and -- by `want` -- the device copy of the chain and the pinned flag.  nullptr: *rc is the code, oh_last_error says why.  (The peers of
// ensure_peers come through oh_create / oh_create_torque and so through here: a peer wants the defaults those fill in.)
enum { OPEN_CHAIN = 1, OPEN_FLAG = 2 };
static oh_handle* open_handle(const std::string& who, const int kind, const int T, const int ndof, const int want, int* rc) {
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) {
    *rc = fail(OH_ERR_HIP, who + ": no HIP device available (this library has no CPU path)");
    return nullptr;
  }
  oh_handle* h = new_handle();
  if (!h) {
    *rc = OH_ERR_INVALID;
    return nullptr;
  }
  h->desc = oh_problem_desc{};
  h->desc.kind = kind;
  h->desc.T = T;
  h->desc.ndof = ndof;
  hipGetDevice(&h->device);
  bool ok = hipStreamCreate(&h->stream) == hipSuccess;
  for (hipEvent_t* e : {&h->ev0, &h->ev1, &h->evt0, &h->evt1}) ok = ok && hipEventCreate(e) == hipSuccess;
  if ((want & OPEN_CHAIN) && ok) ok = h->d_chain.reserve(1) == hipSuccess;
  if ((want & OPEN_FLAG) && ok) ok = h->h_flag.reserve(1) == hipSuccess;
  if (!ok) {
    delete h;
    *rc = fail(OH_ERR_HIP, who + (want ? ": stream/event/allocation failed" : ": stream/event creation failed"));
    return nullptr;
  }
  return h;
}

// every solve reports counters of its own only (oh_get_timing)
static void reset_counters(oh_handle* h) {
  for (double& t : h->timing) t = 0.0;
  h->timing_couple = h->rejects = h->tail_iters = 0.0;
}
// the tail every solve shares: wait for the launches since ev0, report a launch error, time the solve ([4]) and count its launches ([5])
static int finish_solve(oh_handle* h, const double launched) {
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  reset_counters(h);
  h->timing[4] = ms;
  h->timing[5] = launched;
  return OH_OK;
}

extern "C" int oh_device_count(int* n) {
  if (!n) return fail(OH_ERR_INVALID, "oh_device_count: null");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    return fail(OH_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *n = c;
  return OH_OK;
}
extern "C" int oh_set_device(int index) {
  HIPCHK(hipSetDevice(index));
  return OH_OK;
}
extern "C" int oh_device_malloc(void** ptr, size_t nbytes) {
  if (!ptr) return fail(OH_ERR_INVALID, "oh_device_malloc: null");
  HIPCHK(hipMalloc(ptr, nbytes ? nbytes : 8));
  return OH_OK;
}
extern "C" int oh_device_free(void* ptr) {
  HIPCHK(hipFree(ptr));
  return OH_OK;
}
extern "C" int oh_memcpy_h2d(void* dst, const void* src, size_t nbytes) {
  HIPCHK(hipMemcpy(dst, src, nbytes, hipMemcpyHostToDevice));
  return OH_OK;
}
extern "C" int oh_memcpy_d2h(void* dst, const void* src, size_t nbytes) {
  HIPCHK(hipMemcpy(dst, src, nbytes, hipMemcpyDeviceToHost));
  return OH_OK;
}
extern "C" int oh_device_synchronize(void) {
  HIPCHK(hipDeviceSynchronize());
  return OH_OK;
}

extern "C" int oh_create(const oh_problem_desc* desc, oh_handle** out) {
  if (!desc || !out) return fail(OH_ERR_INVALID, "oh_create: null argument");
  *out = nullptr;
  if (desc->kind != OH_PROBLEM_FIGURE_EIGHT && desc->kind != OH_PROBLEM_KINEMATICS)
    return fail(OH_ERR_INVALID, "oh_create: unknown problem kind");
  if (desc->kind == OH_PROBLEM_KINEMATICS) {
    if (desc->ndof < 1 || desc->ndof > OH_MAX_CHAIN) return fail(OH_ERR_INVALID, "oh_create: ndof must be in [1, OH_MAX_CHAIN]");
    int rc = OH_OK;
    oh_handle* hk = open_handle("oh_create", desc->kind, desc->T, desc->ndof, OPEN_CHAIN, &rc);
    if (!hk) return rc;
    hk->desc = *desc;
    hk->desc.local_path = nullptr;
    *out = hk;
    return OH_OK;
  }
  if (desc->T < 3 || desc->T > OH_MAX_T) return fail(OH_ERR_INVALID, "oh_create: T must be in [3, OH_MAX_T]");
  if (desc->ndof < (desc->lock_orientation ? 4 : 2) || desc->ndof > 8)
    return fail(OH_ERR_INVALID, "oh_create: the trajectory kernels are instantiated for 2 ... 8 actuated joints, the orientation-locked ones (three rows per "
                                "knot, null space of ndof - 3 dimensions) for 4 ... 8");
  if (!(desc->dt > 0.0)) return fail(OH_ERR_INVALID, "oh_create: dt must be positive");
  if (!desc->local_path) return fail(OH_ERR_INVALID, "oh_create: local_path is null");
  if (desc->hessian != OH_HESSIAN_GAUSS_NEWTON && desc->hessian != OH_HESSIAN_EXACT && desc->hessian != OH_HESSIAN_HYBRID)
    return fail(OH_ERR_INVALID, "oh_create: bad hessian mode");
  int rc = OH_OK;
  oh_handle* h = open_handle("oh_create", desc->kind, desc->T, desc->ndof, OPEN_CHAIN | OPEN_FLAG, &rc);
  if (!h) return rc;
  h->desc = *desc;
  h->local_path.assign(desc->local_path, desc->local_path + 3 * (size_t)desc->T);
  h->desc.local_path = nullptr;
  if (h->desc.max_iter <= 0) h->desc.max_iter = 200;
  if (!(h->desc.tol > 0.0)) h->desc.tol = 1e-6;
  if (!(h->desc.tol_feas > 0.0)) h->desc.tol_feas = 1e-9;
  if (h->desc.mu0 < 0.0) h->desc.mu0 = 0.0;
  if (h->d_local_path.reserve(3 * (size_t)desc->T) != hipSuccess) {
    delete h;
    return fail(OH_ERR_HIP, "oh_create: device allocation failed");
  }
  hipMemcpy(h->d_local_path, h->local_path.data(), sizeof(double) * 3 * (size_t)desc->T, hipMemcpyHostToDevice);
  *out = h;
  return OH_OK;
}

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
  h->pm = *desc;
  if (h->pm.max_iter <= 0) h->pm.max_iter = 100;
  if (!(h->pm.tol > 0.0)) h->pm.tol = 1e-8;
  *out = h;
  return OH_OK;
}

static int tape_validate(const oh_tape_desc* d, const char* who) {
  const std::string w(who);
  if (d->nx < 1 || d->nx > OH_TAPE_MAX_N || d->np < 0 || d->len < 1 || d->len > OH_TAPE_MAX_LEN || d->n_ineq < 0 || d->n_eq < 0 || !d->op || !d->a ||
      !d->b || !d->c || (d->n_ineq + d->n_eq > 0 && !d->rows) || d->out_cost < 0 || d->out_cost >= d->len)
    return fail(OH_ERR_INVALID, (w + ": bad sizes or null arrays").c_str());
  for (int i = 0; i < d->len; ++i) {
    const int o = d->op[i];
    const bool two = (o >= 3 && o <= 6) || o == 10 || (o >= 15 && o <= 20) || (o >= 22 && o <= 24);
    const bool one = o == 7 || o == 8 || o == 9 || o == 11 || o == 12 || o == 13 || o == 14 || o == 21 || o == 25 || o == 26;
    if (o < 0 || o > 26 || (o == 1 && (d->a[i] < 0 || d->a[i] >= d->nx)) || (o == 2 && (d->a[i] < 0 || d->a[i] >= d->np)) ||
        ((one || two) && (d->a[i] < 0 || d->a[i] >= i)) || (two && (d->b[i] < 0 || d->b[i] >= i)))
      return fail(OH_ERR_INVALID, (w + ": malformed instruction (operands must be earlier registers / valid indices)").c_str());
  }
  for (int i = 0; i < d->n_ineq + d->n_eq; ++i)
    if (d->rows[i] < 0 || d->rows[i] >= d->len) return fail(OH_ERR_INVALID, (w + ": row register out of range").c_str());
  return OH_OK;
}

static TapeParams tape_params(const oh_tape_desc* d, const int lbfgs_opt = -1) {
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
// applies (tape_wave != 0, limited-memory regime, LDS fit), otherwise generated code (desc.jit) or the interpreter.
static int tape_configure(oh_handle* h) {
  oh_tape_desc d = h->t_desc;
  d.op = h->t_op.data(); d.a = h->t_a.data(); d.b = h->t_b.data(); d.c = h->t_c.data(); d.rows = h->t_rows.empty() ? nullptr : h->t_rows.data();
  h->TP = tape_params(&d, (int)optv(h, "tape_lbfgs"));
  h->TP.h0 = h->d_tape_h0;  // (a metric handed over before an option rebuilt the evaluator stays)
  oh_tape_wave_release(&h->tape_wave);
  h->tape_wave = TapeWave{};
  h->d_tape_work.release();  // the work arrays were sized for the other evaluator
  h->d_tape_mult.release();
  int lds_limit = 0;
  if (optv(h, "tape_wave") != 0.0 && hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device) == hipSuccess) {
    std::string err;
    if (oh_tape_wave_build(h->TP, d.op, d.a, d.b, d.c, d.rows, (size_t)lds_limit, (int)optv(h, "tape_wave_nt"), (int)optv(h, "tape_wave_regs"),
                           (int)optv(h, "tape_wave_hist"), &h->tape_wave, &err))
      return fail(OH_ERR_HIP, ("oh_create_tape: " + err).c_str());
  }
  if (d.jit && !h->tape_wave.ready && !h->tape_jit.fn) {
    std::vector<char> code;
    std::string err;
    const std::string src = oh_tape_jit_source(h->TP, d.op, d.a, d.b, d.c, d.rows);
    bool ok = !oh_tape_jit_compile(src, &code, &err) && !oh_tape_jit_load(code, &h->tape_jit, &err);
    if (!ok && !code.empty()) {  // an object that compiled (or came from the disk cache) and does not load: drop it, recompile once (as oh_jit_figure8 does)
      oh_tape_jit_forget(src);
      code.clear();
      ok = !oh_tape_jit_compile(src, &code, &err) && !oh_tape_jit_load(code, &h->tape_jit, &err);
    }
    if (!ok) return fail(OH_ERR_HIP, ("oh_create_tape: " + err).c_str());
  }
  return OH_OK;
}

// the five device arrays of a tape (op_override: the opcodes to upload in place of d->op)
static int upload_tape(oh_handle* h, const oh_tape_desc* d, const int* op_override) {
  const size_t len = (size_t)d->len, nrow = (size_t)(d->n_ineq + d->n_eq);
  for (DevBuf<int>* b : {&h->d_tape_op, &h->d_tape_a, &h->d_tape_b, &h->d_tape_rows}) b->release();  // (sized for this tape, not grown from the last one's)
  h->d_tape_c.release();
  HIPCHK(h->d_tape_op.reserve(len));
  HIPCHK(h->d_tape_a.reserve(len));
  HIPCHK(h->d_tape_b.reserve(len));
  HIPCHK(h->d_tape_c.reserve(len));
  HIPCHK(h->d_tape_rows.reserve(nrow + 1));
  HIPCHK(hipMemcpy(h->d_tape_op, op_override ? op_override : d->op, sizeof(int) * len, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_tape_a, d->a, sizeof(int) * len, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_tape_b, d->b, sizeof(int) * len, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_tape_c, d->c, sizeof(double) * len, hipMemcpyHostToDevice));
  if (nrow > 0) HIPCHK(hipMemcpy(h->d_tape_rows, d->rows, sizeof(int) * nrow, hipMemcpyHostToDevice));
  return OH_OK;
}

extern "C" int oh_create_tape(const oh_tape_desc* d, oh_handle** out) {
  if (!d || !out) return fail(OH_ERR_INVALID, "oh_create_tape: null argument");
  *out = nullptr;
  if (const int rc = tape_validate(d, "oh_create_tape")) return rc;
  int rc = OH_OK;
  oh_handle* h = open_handle("oh_create_tape", OH_PROBLEM_TAPE, 1, d->nx, 0, &rc);
  if (!h) return rc;
  // the tape stays with the handle: the evaluator is rebuilt when an option that shapes it changes
  h->t_op.assign(d->op, d->op + d->len);
  h->t_a.assign(d->a, d->a + d->len);
  h->t_b.assign(d->b, d->b + d->len);
  h->t_c.assign(d->c, d->c + d->len);
  h->t_rows.assign(d->rows ? d->rows : d->op, (d->rows ? d->rows : d->op) + (d->rows ? d->n_ineq + d->n_eq : 0));
  h->t_desc = *d;
  if (d->no_wave && !h->opt.count("tape_wave")) h->opt["tape_wave"] = 0.0;
  if (d->lbfgs != 0 && !h->opt.count("tape_lbfgs")) h->opt["tape_lbfgs"] = d->lbfgs > 0 ? (double)d->lbfgs : 0.0;
  if ((rc = tape_configure(h))) {
    delete h;  // (releases the wavefront schedule / the generated module as well)
    return rc;
  }
  // the interpreter's copy of the opcodes carries bit 5 on every instruction that neither the cost nor a row depends on: its reverse sweep passes them by
  // (oh_tape.hip:InterpEval::reverse), as the generated code and the wavefront schedule do
  std::vector<int> op_dev(d->op, d->op + d->len);
  {
    std::vector<char> live(d->len, 0);
    live[d->out_cost] = 1;
    for (int i = 0; i < d->n_ineq + d->n_eq; ++i) live[d->rows[i]] = 1;
    for (int i = d->len - 1; i >= 0; --i) {
      if (!live[i]) { op_dev[i] |= 32; continue; }
      if (d->op[i] >= 3) {
        live[d->a[i]] = 1;
        if (tape_op_arity(d->op[i]) == 2) live[d->b[i]] = 1;
      }
    }
  }
  if ((rc = upload_tape(h, d, op_dev.data()))) {
    delete h;
    return rc;
  }
  *out = h;
  return OH_OK;
}

static int ensure_stage(oh_handle* h, size_t bytes);
// The staging area of a host-buffer entry point: layout(Carver) is its one list of takes, each a 256-byte slot, and returns the carver's bytes().
// It runs on a null base to size the area, then on the area itself.
template <class Layout>
static int stage_carve(oh_handle* h, Layout&& layout) {
  if (const int rc = ensure_stage(h, layout(Carver(nullptr, Carver::Slots)))) return rc;
  layout(Carver(h->stage.p, Carver::Slots));
  return OH_OK;
}
extern "C" int oh_tape_probe(oh_handle* h, int B, const double* x, const double* p, int n_regs, const int* regs, double* val, const double* seeds, double* adj,
                             double* grad) {
  if (!h || !x) return fail(OH_ERR_INVALID, "oh_tape_probe: null argument");
  if (h->desc.kind != OH_PROBLEM_TAPE) return fail(OH_ERR_STATE, "oh_tape_probe: handle is not an OH_PROBLEM_TAPE problem");
  const TapeParams& T = h->TP;
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
  oh_launch_tape_probe(s, T, h->d_tape_op, h->d_tape_a, h->d_tape_b, h->d_tape_c, h->d_tape_rows, B, Bp, d_x, d_p, d_w, n_regs, d_r, val ? d_v : nullptr,
                       seeds ? d_s : nullptr, (seeds && adj) ? d_a : nullptr, (seeds && grad) ? d_g : nullptr);
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  if (val && n_regs > 0) HIPCHK(hipMemcpy(val, d_v, sizeof(double) * (size_t)n_regs * B, hipMemcpyDeviceToHost));
  if (seeds && adj && n_regs > 0) HIPCHK(hipMemcpy(adj, d_a, sizeof(double) * (size_t)n_regs * B, hipMemcpyDeviceToHost));
  if (seeds && grad) HIPCHK(hipMemcpy(grad, d_g, b_x, hipMemcpyDeviceToHost));
  return OH_OK;
}

extern "C" int oh_tape_set_metric(oh_handle* h, const double* H0) {
  if (!h) return fail(OH_ERR_INVALID, "oh_tape_set_metric: null argument");
  if (h->desc.kind != OH_PROBLEM_TAPE) return fail(OH_ERR_INVALID, "oh_tape_set_metric: not an OH_PROBLEM_TAPE handle");
  HIPCHK(hipSetDevice(h->device));
  const size_t n = (size_t)h->TP.nx;
  if (!H0) {
    h->d_tape_h0.release();
    h->TP.h0 = nullptr;
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
  HIPCHK(h->d_tape_h0.reserve(n * n));
  HIPCHK(hipMemcpy(h->d_tape_h0, H0, sizeof(double) * n * n, hipMemcpyHostToDevice));
  h->TP.h0 = h->d_tape_h0;
  return OH_OK;
}

// work arrays of the thread-per-instance evaluators and the multipliers' buffer for batches of up to Bp instances
static int tape_ensure_work(oh_handle* h, const int Bp) {
  if (Bp > h->tape_cap()) {  // both at the new stride, or (an allocation failed) tape_cap() == 0
    h->d_tape_work.release();
    h->d_tape_mult.release();
    if (!h->tape_wave.ready) HIPCHK(h->d_tape_work.reserve((size_t)oh_tape_work_rows(h->TP, h->tape_jit.fn != nullptr) * Bp));
    HIPCHK(h->d_tape_mult.reserve((size_t)(h->TP.n_ineq + h->TP.n_eq + 1) * Bp));
  }
  return OH_OK;
}

extern "C" int oh_tape_phi(oh_handle* h, int B, const double* x, const double* p, const double* lam, const double* mu, double rho, double* merit, double* f,
                           double* rows, double* grad, double* cmax, double* meas) {
  if (!h || !x || !merit || !f || !grad || !cmax || !meas) return fail(OH_ERR_INVALID, "oh_tape_phi: null argument");
  if (h->desc.kind != OH_PROBLEM_TAPE) return fail(OH_ERR_STATE, "oh_tape_phi: handle is not an OH_PROBLEM_TAPE problem");
  const TapeParams& T = h->TP;
  const int nrow = T.n_ineq + T.n_eq;
  if (B < 1 || (T.np > 0 && !p) || (T.n_ineq > 0 && !lam) || (T.n_eq > 0 && !mu) || (nrow > 0 && !rows)) return fail(OH_ERR_INVALID, "oh_tape_phi: bad sizes");
  if (!(rho > 0.0)) return fail(OH_ERR_INVALID, "oh_tape_phi: the penalty must be positive");
  HIPCHK(hipSetDevice(h->device));
  const int Bp = (B + 63) / 64 * 64;
  if (h->tape_jit.fn && !h->tape_wave.ready && !h->tape_jit_phi.fn) {
    std::vector<char> code;
    std::string err;
    const std::string src = oh_tape_jit_source(T, h->t_op.data(), h->t_a.data(), h->t_b.data(), h->t_c.data(), h->t_rows.empty() ? nullptr : h->t_rows.data(), false);
    if (oh_tape_jit_compile(src, &code, &err) || oh_tape_jit_load(code, &h->tape_jit_phi, &err, false)) return fail(OH_ERR_HIP, ("oh_tape_phi: " + err).c_str());
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
  h->tape_phi_lds = 0;
  // the evaluator oh_solve launches for this handle and this B (tape_solve_device)
  if (h->tape_wave.ready)
    HIPCHK(oh_launch_tape_wave_phi(s, h->tape_wave, T, B, d_x, d_p, d_l, d_m, rho, d_v, d_f, d_r, d_g, d_c, d_s));
  else if (h->tape_jit.fn)
    HIPCHK(oh_launch_tape_jit_phi(s, h->tape_jit_phi, T, B, h->tape_cap(), d_x, d_p, d_l, d_m, rho, h->d_tape_work, d_v, d_f, d_r, d_g, d_c, d_s,
                                  (int)optv(h, "tape_lds_max"), &h->tape_phi_lds));
  else
    oh_launch_tape_phi(s, T, h->d_tape_op, h->d_tape_a, h->d_tape_b, h->d_tape_c, h->d_tape_rows, B, h->tape_cap(), d_x, d_p, d_l, d_m, rho, h->d_tape_work, d_v, d_f,
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

static int tape_solve_device(oh_handle* h, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt, void* d_iters, void* d_status) {
  HIPCHK(hipSetDevice(h->device));
  const int Bp = (B + 63) / 64 * 64;
  if (const int rc = tape_ensure_work(h, Bp)) return rc;
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  if (h->tape_wave.ready)
    HIPCHK(oh_launch_tape_wave(h->stream, h->tape_wave, h->TP, B, (const double*)d_x0, (const double*)d_p, (double*)d_x, (double*)d_f, (double*)d_kkt, (int*)d_iters,
                               (int*)d_status, h->d_tape_mult));
  else if (h->tape_jit.fn)
    HIPCHK(oh_launch_tape_jit(h->stream, h->tape_jit, h->TP, B, h->tape_cap(), (const double*)d_x0, (const double*)d_p, h->d_tape_work, (double*)d_x, (double*)d_f,
                              (double*)d_kkt, (int*)d_iters, (int*)d_status, h->d_tape_mult, (int)optv(h, "tape_lds_max")));
  else
    oh_launch_tape_solve(h->stream, h->TP, h->d_tape_op, h->d_tape_a, h->d_tape_b, h->d_tape_c, h->d_tape_rows, B, h->tape_cap(), (const double*)d_x0,
                         (const double*)d_p, h->d_tape_work, (double*)d_x, (double*)d_f, (double*)d_kkt, (int*)d_iters, (int*)d_status, h->d_tape_mult);
  return finish_solve(h, 1);
}

extern "C" int oh_create_qp(const oh_qp_desc* desc, oh_handle** out) {
  if (!desc || !out) return fail(OH_ERR_INVALID, "oh_create_qp: null argument");
  *out = nullptr;
  if (desc->n < 1 || desc->n > OH_QP_MAX_N || desc->m < 0 || desc->m > OH_QP_MAX_M || desc->me < 0 || desc->me > OH_QP_MAX_ME || desc->me > desc->n)
    return fail(OH_ERR_INVALID, "oh_create_qp: sizes out of range (1 <= n <= 128, 0 <= m <= 1024, 0 <= me <= min(128, n))");
  int rc = OH_OK;
  oh_handle* h = open_handle("oh_create_qp", OH_PROBLEM_QP, 1, desc->n, 0, &rc);
  if (!h) return rc;
  h->qp = *desc;
  if (h->qp.max_iter <= 0) h->qp.max_iter = 100;
  if (!(h->qp.tol > 0.0)) h->qp.tol = 1e-9;
  *out = h;
  return OH_OK;
}

static size_t qp_np(const oh_qp_desc& q) { return (size_t)q.n * q.n + q.n + (size_t)q.m * q.n + q.m + (size_t)q.me * q.n + q.me; }

// Shape (oh_carve.h) of a handle's problem
static Shape shape_of(const oh_handle* h) {
  const size_t N = h->desc.ndof, T = h->desc.T;
  switch (h->desc.kind) {
    case OH_PROBLEM_TORQUE_MPC: return {4 * N * T, 2 * N + 3 * T, T * (h->tq.vel_limits ? 4 : 2) * N};
    case OH_PROBLEM_TAPE: return {(size_t)h->TP.nx, (size_t)(h->TP.np > 0 ? h->TP.np : 1), (size_t)(h->TP.n_ineq + h->TP.n_eq)};
    case OH_PROBLEM_QP: return {(size_t)h->qp.n, h->qp_tape ? (size_t)(h->TP.np > 0 ? h->TP.np : 1) : qp_np(h->qp), (size_t)(h->qp.m + h->qp.me)};
    case OH_PROBLEM_POINT_MASS_MPC: return {4 * T, 4 + 4 * T, 0};
    case OH_PROBLEM_IK: return {N, N + 3, 3 + 2 * N};
    case OH_PROBLEM_FIGURE_EIGHT: {
      const oh_guards& g = h->guards;
      const size_t nx = N * T + N * (T - 1);
      if (h->chain_host.has_lead) return {nx, N + 1 + T, h->desc.lock_orientation ? 4 * T : 0};
      if (!h->have_guards) return {nx, N, h->desc.lock_orientation ? 4 * T : 0};
      // [T][NC (+ 2 ndof velocity rows)]: limits, spheres x obstacles
      return {nx, N + g.n_links + 4 * (size_t)g.n_obstacles, T * ((g.limits ? 2 * N : 0) + (size_t)g.n_links * g.n_obstacles + (g.vel_limits ? 2 * N : 0))};
    }
    default: return {0, 0, 0};
  }
}

extern "C" int oh_qp_set_tape(oh_handle* h, const oh_tape_desc* d) {
  if (!h || !d) return fail(OH_ERR_INVALID, "oh_qp_set_tape: null argument");
  if (h->desc.kind != OH_PROBLEM_QP) return fail(OH_ERR_STATE, "oh_qp_set_tape: not an OH_PROBLEM_QP handle");
  if (const int rc = tape_validate(d, "oh_qp_set_tape")) return rc;
  if (d->nx != h->qp.n || d->n_ineq != h->qp.m || d->n_eq != h->qp.me)
    return fail(OH_ERR_INVALID, "oh_qp_set_tape: the tape's nx / n_ineq / n_eq differ from the handle's n / m / me");
  HIPCHK(hipSetDevice(h->device));
  h->qp_tape = false;
  if (const int rc = upload_tape(h, d, nullptr)) return rc;
  h->TP = tape_params(d);
  {
    // instructions whose value depends on x: the probes after the first re-run only these
    std::vector<char> dep((size_t)d->len, 0);
    std::vector<int> list;
    for (int i = 0; i < d->len; ++i) {
      const int o = d->op[i];
      const bool two = tape_op_arity(o) == 2, one = tape_op_arity(o) == 1;
      dep[i] = o == 1 || ((one || two) && dep[d->a[i]]) || (two && dep[d->b[i]]);
      if (dep[i]) list.push_back(i);
    }
    h->d_qp_xdep.release();
    h->qp_n_xdep = (int)list.size();
    HIPCHK(h->d_qp_xdep.reserve(list.size() + 1));
    if (!list.empty()) HIPCHK(hipMemcpy(h->d_qp_xdep, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
  }
  for (DevBuf<double>* b : {&h->d_qp_rows, &h->d_qp_val, &h->d_qp_f0}) b->release();  // the register file of another tape: size it again at the next solve
  h->qp_tape = true;
  return OH_OK;
}

static int qp_solve_device(oh_handle* h, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt, void* d_iters, void* d_status) {
  HIPCHK(hipSetDevice(h->device));
  const oh_qp_desc& q = h->qp;
  QpParams Q{};
  Q.n = q.n; Q.m = q.m; Q.me = q.me; Q.np = (int)qp_np(q); Q.max_iter = q.max_iter; Q.tol = q.tol;
  Q.nwork = q.n + 2 * q.m + q.me + q.n * q.n + 2 * q.n + 2 * q.m + q.me * q.n + q.me * q.me + q.me + q.n;
  const int Bp = (B + 63) / 64 * 64;
  const int mode = (int)optv(h, "qp_mode");
  const bool large = oh_qp_is_large(Q), block = oh_qp_takes_block(Q, mode);
  HIPCHK(h->d_qp_mult.reserve((size_t)(q.m + q.me + 1) * Bp));
  // what k_qp_solve_block keeps in global memory: a slice per instance (its vectors and H live in LDS); the other kernels: [Q.nwork][Bp]
  if (block) HIPCHK(h->d_qp_blk.reserve(oh_qp_block_work_doubles(Q) * (size_t)B + 1));
  else HIPCHK(h->d_qp_work.reserve((size_t)Q.nwork * Bp));
  const int work_stride = (int)(h->d_qp_work.cap / (size_t)Q.nwork);  // the Bp d_qp_work was allocated for (0: never)
  // register file of the tape interpreter: a lane per instance, or (a few instances: B <= 64) a lane per probe point of every instance;
  // large handles: rows and f(0, p) by instance, the register file by the instances of one launch (64 lanes each)
  const int Bv = large ? B : (B <= 64 ? (B * 64 > Bp ? B * 64 : Bp) : Bp);
  const int chunk = (large && h->qp_tape) ? oh_qp_assemble_block_chunk(h->TP, B) : 0;
  // (d_qp_f0 is allocated last: its capacity is the Bv all three hold; large handles: d_qp_val holds 64 lanes for each of `chunk` instances)
  if (h->qp_tape && ((size_t)Bv > h->d_qp_f0.cap || (size_t)h->TP.len * chunk * 64 > h->d_qp_val.cap)) {
    for (DevBuf<double>* b : {&h->d_qp_rows, &h->d_qp_val, &h->d_qp_f0}) b->release();
    HIPCHK(h->d_qp_rows.reserve((size_t)Q.np * Bv));
    HIPCHK(h->d_qp_val.reserve((size_t)h->TP.len * (large ? (size_t)chunk * 64 : (size_t)Bv)));
    HIPCHK(h->d_qp_f0.reserve((size_t)Bv));
  }
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  std::string err;
  h->qp_last_block = block ? 1 : 0;
  if (h->qp_tape) {
    if (large) {
      if (oh_launch_qp_assemble_block(h->stream, Q, h->TP, h->d_tape_op, h->d_tape_a, h->d_tape_b, h->d_tape_c, h->d_tape_rows, h->d_qp_xdep, h->qp_n_xdep, B, chunk,
                                      (const double*)d_p, h->d_qp_val, h->d_qp_rows, h->d_qp_f0, &err))
        return fail(OH_ERR_HIP, "oh_solve: " + err);
    } else {
      oh_launch_qp_assemble(h->stream, Q, h->TP, h->d_tape_op, h->d_tape_a, h->d_tape_b, h->d_tape_c, h->d_tape_rows, h->d_qp_xdep, h->qp_n_xdep, B, B <= 64 ? B * 64 : (int)h->d_qp_f0.cap, (const double*)d_p,
                            h->d_qp_val, h->d_qp_rows, h->d_qp_f0);
    }
    d_p = h->d_qp_rows;
  }
  if (oh_launch_qp_solve(h->stream, Q, B, work_stride, (const double*)d_x0, (const double*)d_p, block ? h->d_qp_blk.p : h->d_qp_work.p, (double*)d_x, (double*)d_f, (double*)d_kkt,
                         (int*)d_iters, (int*)d_status, h->d_qp_mult, mode, &err))
    return fail(OH_ERR_HIP, "oh_solve: " + err);
  if (h->qp_tape && d_f) oh_launch_qp_add_constant(h->stream, B, (double*)d_f, h->d_qp_f0);
  return finish_solve(h, 1);
}

extern "C" int oh_create_ik(const oh_ik_desc* desc, oh_handle** out) {
  if (!desc || !out) return fail(OH_ERR_INVALID, "oh_create_ik: null argument");
  *out = nullptr;
  if (desc->ndof < 2 || desc->ndof > 8) return fail(OH_ERR_INVALID, "oh_create_ik: kernels are instantiated for 2 ... 8 actuated joints");
  if (!(desc->w_nominal > 0.0)) return fail(OH_ERR_INVALID, "oh_create_ik: w_nominal must be positive");
  for (int i = 0; i < desc->ndof; ++i)
    if (!(desc->q_lo[i] <= desc->q_up[i])) return fail(OH_ERR_INVALID, "oh_create_ik: q_lo must not exceed q_up");
  int rc = OH_OK;
  oh_handle* h = open_handle("oh_create_ik", OH_PROBLEM_IK, 1, desc->ndof, OPEN_CHAIN, &rc);
  if (!h) return rc;
  h->ik = *desc;
  if (h->ik.max_iter <= 0) h->ik.max_iter = 200;
  if (!(h->ik.tol > 0.0)) h->ik.tol = 1e-6;
  if (!(h->ik.tol_feas > 0.0)) h->ik.tol_feas = 1e-9;
  if (!(h->ik.rho0 > 0.0)) h->ik.rho0 = 100.0 * h->ik.w_nominal;
  *out = h;
  return OH_OK;
}

static bool solver_chain_ok(const oh_chain& c);

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
  h->tq = *desc;
  if (h->tq.max_iter <= 0) h->tq.max_iter = 300;
  if (!(h->tq.tol > 0.0)) h->tq.tol = 1e-6;
  if (!(h->tq.tol_compl > 0.0)) h->tq.tol_compl = 1e-8;
  if (!(h->tq.mu_barrier0 > 0.0)) h->tq.mu_barrier0 = 0.1;
  if (!(h->tq.mu0 >= 0.0)) h->tq.mu0 = 0.0;
  *out = h;
  return OH_OK;
}

static int tq_solve_device(oh_handle* h, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt, void* d_iters, void* d_status,
                           const double mu_b0_warm = 0.0) {
  if (!h->have_chain) return fail(OH_ERR_STATE, "oh_solve_device: call oh_set_constants first");
  if (!h->have_dyn) return fail(OH_ERR_STATE, "oh_solve_device: call oh_set_dynamics first");
  if (!solver_chain_ok(h->chain_host) || h->chain_host.has_lead)
    return fail(OH_ERR_INVALID, "oh_solve_device: the solver needs a chain that covers every model joint in order");
  const int N = h->tq.ndof, T = h->tq.T;
  if (h->dyn_host.ndof != N) return fail(OH_ERR_INVALID, "oh_solve_device: the inverse-dynamics tables must have ndof + 1 bodies");
  HIPCHK(hipSetDevice(h->device));
  TqParams& P = h->TqP;
  P = TqParams{};
  P.T = T; P.N = N; P.max_iter = h->tq.max_iter;
  P.dt = h->tq.dt; P.w_path = h->tq.w_path; P.w_vel = h->tq.w_vel; P.w_tau = h->tq.w_tau;
  P.tol = h->tq.tol; P.tol_compl = h->tq.tol_compl; P.mu_b0 = mu_b0_warm > 0.0 ? mu_b0_warm : h->tq.mu_barrier0; P.mu0 = h->tq.mu0;
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
  P.vel = h->tq.vel_limits ? 1 : 0;
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
    P.tau_lo[i] = h->tq.tau_lo[i];
    P.tau_up[i] = h->tq.tau_up[i];
    P.dq_lo[i] = h->tq.dq_lo[i];
    P.dq_up[i] = h->tq.dq_up[i];
  }
  P.nx = (int)shape_of(h).nx;
  P.np = (int)shape_of(h).npar;
  TqBuffers& D = h->TqD;
  const size_t BT = (size_t)B * T;
  if (BT * TQ_HC > h->d_tq_hc.cap) {  // the pool, the multipliers and the curvature terms grow together (d_tq_hc last: its capacity is the batch all three hold)
    HIPCHK(hipStreamSynchronize(h->stream));
    h->tq_pool.release();
    h->d_tq_mult.release();
    h->d_tq_hc.release();
    Carver measure(nullptr, Carver::Packed);
    layout_tq(measure, D, B, T);
    HIPCHK(h->tq_pool.reserve(measure.bytes()));
    HIPCHK(h->d_tq_mult.reserve(BT * 4 * N));  // effort rows, and room for the velocity rows
    HIPCHK(h->d_tq_hc.reserve(BT * TQ_HC));
    HIPCHK(hipMemsetAsync(h->d_tq_hc, 0, sizeof(double) * BT * TQ_HC, h->stream));  // entries the adjoint never writes stay zero
  }
  {
    // D.B is the live batch: the strides of the [slot][B][T] arrays follow it, inside a pool that holds the largest batch so far
    Carver carve(h->tq_pool.p, Carver::Packed);
    layout_tq(carve, D, B, T);
    D.B = B;
    D.chain = h->d_chain;
    D.dyn = h->d_dyn;
    D.hc = h->d_tq_hc;
    D.n_run = B;
  }
  hipStream_t s = h->stream;
  HIPCHK(hipEventRecord(h->ev0, s));
  if (!oh_launch_tq_setup(s, P, D, (const double*)d_x0, (const double*)d_p)) return fail(OH_ERR_INVALID, "oh_solve_device: unsupported ndof");
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
  oh_launch_tq_finalize(s, P, D, (double*)d_x, (double*)d_f, (double*)d_kkt, (int*)d_iters, (int*)d_status, h->d_tq_mult);
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

static int ik_solve_device(oh_handle* h, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt, void* d_iters,
                           void* d_status) {
  if (!h->have_chain) return fail(OH_ERR_STATE, "oh_solve_device: call oh_set_constants first");
  if (!solver_chain_ok(h->chain_host))
    return fail(OH_ERR_INVALID, "oh_solve_device: the solver needs a chain that covers every model joint in order");
  HIPCHK(hipSetDevice(h->device));
  const int N = h->ik.ndof;
  HIPCHK(h->d_ik_mult.reserve((3 + 2 * (size_t)N) * B));
  IkParams P{};
  P.ndof = N;
  P.max_iter = h->ik.max_iter;
  P.w = h->ik.w_nominal;
  P.tol = h->ik.tol;
  P.tol_feas = h->ik.tol_feas;
  P.rho0 = h->ik.rho0;
  for (int i = 0; i < N; ++i) {
    P.lo[i] = h->ik.q_lo[i];
    P.up[i] = h->ik.q_up[i];
  }
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  if (!oh_launch_ik_solve(h->stream, h->d_chain, P, B, (const double*)d_x0, (const double*)d_p, (double*)d_x, (double*)d_f, (double*)d_kkt,
                          (int*)d_iters, (int*)d_status, h->d_ik_mult))
    return fail(OH_ERR_INVALID, "oh_solve_device: unsupported ndof");
  return finish_solve(h, 1);
}

static int pm_prepare(oh_handle* h, int B) {
  HIPCHK(hipSetDevice(h->device));
  const int T = h->pm.T;
  const int Bp = (B + 63) / 64 * 64;  // (padding the row stride like the trajectory families do was measured: no effect, the solve is latency bound)
  if (Bp > h->cap_B || !h->pool) {
    h->pool.release();
    Carver measure(nullptr, Carver::Packed);
    layout_pm(measure, h->PmD, T, Bp);
    const hipError_t e = h->pool.reserve(measure.bytes());
    if (e != hipSuccess) return fail(OH_ERR_HIP, std::string("device pool allocation failed: ") + hipGetErrorString(e));
    h->cap_B = Bp;
    h->PmD.Bp = Bp;
    Carver carve(h->pool.p, Carver::Packed);
    layout_pm(carve, h->PmD, T, Bp);
  }
  h->PmD.B = B;
  h->PmP = PmParams{T, h->pm.dt, h->pm.w_acc, h->pm.ylim, h->pm.vlim, h->pm.safe * h->pm.safe, h->pm.tol, h->pm.max_iter,
                    h->pm.track_final_only ? 1 : 0, h->pm.w_vel, h->pm.fix_final_velocity ? 1 : 0};
  return OH_OK;
}

static int pm_solve_device(oh_handle* h, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt, void* d_iters,
                           void* d_status) {
  int rc = pm_prepare(h, B);
  if (rc) return rc;
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  oh_launch_pm_solve(h->stream, h->PmP, h->PmD, (const double*)d_x0, (const double*)d_p, (double*)d_x, (double*)d_f, (double*)d_kkt,
                     (int*)d_iters, (int*)d_status, (int)optv(h, "pm_wave_max"));
  return finish_solve(h, 1);
}

static int validate_chain(const oh_handle* h, const oh_chain& c) {
  if (c.n_chain < 1 || c.n_chain > OH_MAX_CHAIN || c.ndof < c.n_chain || c.ndof > OH_MAX_CHAIN)
    return fail(OH_ERR_INVALID, "oh_set_constants: bad n_chain/ndof");
  for (int k = 0; k < c.n_chain; ++k) {
    if (c.jtype[k] != 0 && c.jtype[k] != 1) return fail(OH_ERR_INVALID, "oh_set_constants: joint type not supported");
    if (c.qidx[k] < 0 || c.qidx[k] >= c.ndof) return fail(OH_ERR_INVALID, "oh_set_constants: qidx out of range");
  }
  if (c.ndof != h->desc.ndof) return fail(OH_ERR_INVALID, "oh_set_constants: chain.ndof != desc.ndof");
  return OH_OK;
}

// The parts of a split solve run on peer handles that were given the chain, dynamics and inequality rows of this handle when they were created
// (solve_split).  Any setter that changes one of those on the main handle destroys the peers: the next split solve builds them again from the new
// data (parts 1.. used to go on solving with the old chain / limits / obstacles, and guards set after a first split solve left the peers
// striding p by ndof only).  The record of the last solve goes with them: what it points at was computed with the old data.
static void drop_peers(oh_handle* h) {
  h->last = LastSolve{};
  if (h->is_peer) return;
  for (oh_handle* p : h->peers) delete p;
  h->peers.clear();
}

// the handle has new constants: everything compiled for, or remembered about, the previous chain goes (one place for the three entry
// points that set constants)
static void adopt_chain(oh_handle* h, const oh_chain& c) {
  drop_peers(h);
  h->chain_host = c;
  h->have_chain = true;
  h->spec = nullptr;
  h->spec_failed = false;
  h->spec_move_failed = false;
  h->spec_cache_checked = false;
  h->fk_spec = nullptr;
  h->fk_spec_failed = false;
}

extern "C" int oh_set_constants(oh_handle* h, const oh_chain* chain) {
  if (!h || !chain) return fail(OH_ERR_INVALID, "oh_set_constants: null argument");
  int rc = validate_chain(h, *chain);
  if (rc) return rc;
  HIPCHK(hipMemcpy(h->d_chain, chain, sizeof(oh_chain), hipMemcpyHostToDevice));
  adopt_chain(h, *chain);
  return OH_OK;
}

extern "C" int oh_set_constants_device(oh_handle* h, const void* d_chain, size_t nbytes) {
  if (!h || !d_chain) return fail(OH_ERR_INVALID, "oh_set_constants_device: null argument");
  if (nbytes != sizeof(oh_chain)) return fail(OH_ERR_INVALID, "oh_set_constants_device: nbytes != sizeof(oh_chain)");
  oh_chain tmp;
  HIPCHK(hipMemcpy(&tmp, d_chain, sizeof(oh_chain), hipMemcpyDeviceToHost));
  int rc = validate_chain(h, tmp);
  if (rc) return rc;
  HIPCHK(hipMemcpy(h->d_chain, d_chain, sizeof(oh_chain), hipMemcpyDeviceToDevice));
  adopt_chain(h, tmp);
  return OH_OK;
}

static bool solver_chain_ok(const oh_chain& c) {
  if (c.n_chain != c.ndof) return false;
  for (int k = 0; k < c.n_chain; ++k)
    if (c.qidx[k] != k) return false;
  return true;
}

// row stride of the SoA stage arrays for a batch of B (see ensure_capacity)
static int row_stride(const oh_handle* h, int B) {
  int Bp = (B + 63) / 64 * 64;
  if (Bp >= 4096) Bp += 64 * (int)optv(h, "row_pad");
  return Bp;
}
static bool stage_fits(const oh_handle* h, int B) {
  const int N = h->desc.ndof, NZ = h->desc.lock_orientation ? N - 3 : N, T = h->desc.T;
  if (!h->desc.lock_orientation) return true;
  if (!(((double)T * NZ * NZ + 1.0) * (double)row_stride(h, B) * 8.0 < 4294967296.0)) return false;
  if (!(((double)T * (3 * N - 3) + 1.0) * (double)row_stride(h, B) * 8.0 < 4294967296.0)) return false;  // slot offset of the Householder vectors
  // handles with the coupling folded in: the sweep addresses G of either slot and the spare as one 32-bit offset from the lowest of the three
  // adjacent arrays (oh_figure8_units.h:step_instance_zc): 3 T N doubles per instance have to stay below 4 GiB (round 3: found by the batch
  // sweep -- 524 288 instances ran through with wrapped offsets and converged nowhere; they are now refused here and split by the host)
  const bool zc = h->sch.fuse_couple && !h->have_guards && !h->chain_host.has_lead;
  return !zc || 3.0 * (double)T * N * (double)row_stride(h, B) * 8.0 < 4294967296.0;
}

// Largest batch one oh_solve / oh_solve_device call of this handle takes (0: no bound of the library's own, memory permitting): hosts chunk
// bigger batches.  The bound is the 32-bit byte offset of the sweep kernels' stage arrays, row pad included.
extern "C" int oh_max_batch(oh_handle* h, int* out) {
  if (!h || !out) return fail(OH_ERR_INVALID, "oh_max_batch: null argument");
  *out = 0;
  if (h->desc.kind != OH_PROBLEM_FIGURE_EIGHT || !h->desc.lock_orientation) return OH_OK;
  int lo = 64, hi = 1 << 30;  // largest multiple of 64 that fits, by bisection over the predicate ensure_capacity applies
  if (!stage_fits(h, lo)) return OH_OK;
  while (hi - lo > 64) {
    const int mid = ((lo + (hi - lo) / 2) / 64) * 64;
    if (stage_fits(h, mid)) lo = mid; else hi = mid;
  }
  *out = lo;
  return OH_OK;
}

// carve the handle's device pool for B instances
static int ensure_capacity(oh_handle* h, int B) {
  const int N = h->desc.ndof, T = h->desc.T;
  // Row stride of the SoA stage arrays: B rounded up to whole wavefronts, plus -- for large batches -- 13 x 512 B.  With a power-of-two batch
  // every row of every knot starts at a multiple of 2 MiB: the ~30 rows a sweep wave streams side by side then sit at the same offset of
  // their pages, and how the channel hash happens to spread them differed from process to process (k_couple 494 or 525 us per launch,
  // k_step 650...740, interleaved repeats on one box).  Off the power of two the spread is even: k_couple 455, k_step ~650, +3 % solves/s
  // (any of 1...13 x 512 B does it; OH_ROW_PAD overrides, 0 restores the old layout).
  const int Bp = row_stride(h, B);
  // the sweep kernels address one slot of a stage array with a 32-bit byte offset (buffer resources, oh_kernels.hip): the largest such
  // array, T x NZ^2 doubles per instance, has to stay below 4 GiB (about 670 000 instances at T = 50, N = 7; oh_max_batch says exactly)
  if (!stage_fits(h, B)) return fail(OH_ERR_INVALID, "batch too large for one call (stage array beyond 4 GiB): split the batch (oh_max_batch)");
  if (B <= h->cap_B && h->pool) {
    h->D.B = B;
    // keep the Bp the pool was carved with (stride), only the active count changes
    return OH_OK;
  }
  h->pool.release();
  FigBuffers& D = h->D;
  Carver measure(nullptr, Carver::Packed);
  layout_fig(measure, D, N, h->desc.lock_orientation, T, Bp);
  const size_t bytes = measure.bytes();
  const hipError_t e = h->pool.reserve(bytes);
  if (e != hipSuccess) return fail(OH_ERR_HIP, std::string("device pool allocation failed: ") + hipGetErrorString(e));
  hipMemsetAsync(h->pool, 0, bytes, h->stream);
  h->cap_B = Bp;
  Carver carve(h->pool.p, Carver::Packed);
  layout_fig(carve, D, N, h->desc.lock_orientation, T, Bp);
  D.B = B;
  D.Bp = Bp;
  D.chain = h->d_chain;
  return OH_OK;
}

extern "C" int oh_set_guards(oh_handle* h, const oh_guards* g) {
  if (!h || !g) return fail(OH_ERR_INVALID, "oh_set_guards: null argument");
  if (h->desc.kind != OH_PROBLEM_FIGURE_EIGHT) return fail(OH_ERR_INVALID, "oh_set_guards: not a trajectory family");
  if (g->n_links < 0 || g->n_links > OH_MAX_SPHERE_LINKS || g->n_obstacles < 0 || g->n_obstacles > OH_MAX_OBSTACLES)
    return fail(OH_ERR_INVALID, "oh_set_guards: too many sphere links / obstacles");
  if ((g->n_links == 0) != (g->n_obstacles == 0)) return fail(OH_ERR_INVALID, "oh_set_guards: sphere rows need both links and obstacles");
  if (!g->limits && g->n_links == 0 && !g->vel_limits) return fail(OH_ERR_INVALID, "oh_set_guards: no rows");
  // (the orientation-locked kernels that carry inequality rows -- k_eval_lg, k_tail_vel -- are instantiated for 6 and 7 joints only; any
  //  other chain used to launch nothing, finalise the seed and still return OH_OK)
  if (h->desc.lock_orientation && (h->desc.ndof < 4 || h->desc.ndof > 8))
    return fail(OH_ERR_INVALID, "oh_set_guards: inequality rows on an orientation-locked handle need 4 ... 8 joints");
  if (g->vel_limits) {
    for (int j = 0; j < h->desc.ndof; ++j)
      if (!(g->dq_lo[j] < g->dq_up[j])) return fail(OH_ERR_INVALID, "oh_set_guards: dq_lo must be below dq_up");
  }
  for (int l = 0; l < g->n_links; ++l)
    if (g->link_joint[l] < 0 || g->link_joint[l] >= h->desc.ndof)
      return fail(OH_ERR_INVALID, "oh_set_guards: sphere links must hang on an actuated joint of the chain");
  if (g->limits)
    for (int j = 0; j < h->desc.ndof; ++j)
      if (!(g->q_lo[j] < g->q_up[j])) return fail(OH_ERR_INVALID, "oh_set_guards: q_lo must be below q_up");
  if (h->gpool) {  // the pool was carved for the previous row count: rebuild it at the next solve
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->gpool.release();
    h->gcap = 0;
  }
  h->guards = *g;
  h->have_guards = true;
  drop_peers(h);
  return OH_OK;
}

static int ensure_guards(oh_handle* h) {
  const int N = h->desc.ndof, T = h->desc.T;
  const oh_guards& g = h->guards;
  GuardParams& GP = h->GP;
  GP = GuardParams{};
  GP.limits = g.limits ? 1 : 0;
  GP.n_links = g.n_links;
  GP.n_obs = g.n_obstacles;
  GP.NC = (g.limits ? 2 * N : 0) + g.n_links * g.n_obstacles;
  for (int l = 0; l < g.n_links; ++l) {
    GP.link_joint[l] = g.link_joint[l];
    for (int i = 0; i < 3; ++i) GP.link_off[l][i] = g.link_offset[l][i];
  }
  for (int j = 0; j < N; ++j) {
    GP.lo[j] = g.q_lo[j];
    GP.up[j] = g.q_up[j];
  }
  GP.rho0 = g.rho0 > 0.0 ? g.rho0 : 10.0 * h->desc.w_path;
  GP.vel = g.vel_limits ? 1 : 0;
  for (int j = 0; j < N; ++j) {
    GP.vlo[j] = g.dq_lo[j];
    GP.vup[j] = g.dq_up[j];
  }
  GP.vscale = h->desc.dt * h->desc.dt / 40.0;
  const int Bp = h->D.Bp;
  if (!h->gpool || h->gcap != Bp) {  // (not grow-only: the pool is rebuilt for the stride it is carved with)
    h->gpool.release();
    Carver measure(nullptr, Carver::Packed);
    layout_guards(measure, h->GB, h->D.fpsi, GP, N, T, Bp);
    const size_t bytes = measure.bytes();
    const hipError_t e = h->gpool.reserve(bytes);
    if (e != hipSuccess) return fail(OH_ERR_HIP, std::string("guard pool allocation failed: ") + hipGetErrorString(e));
    hipMemsetAsync(h->gpool, 0, bytes, h->stream);
    h->gcap = Bp;
  }
  // (every time: D.fpsi lives in the guard pool, and ensure_capacity may have rebuilt FigBuffers since)
  Carver carve(h->gpool.p, Carver::Packed);
  layout_guards(carve, h->GB, h->D.fpsi, GP, N, T, Bp);
  return OH_OK;
}

static void fill_params(oh_handle* h) {
  FigParams& P = h->P;
  const oh_problem_desc& d = h->desc;
  P.T = d.T;
  P.t0 = d.fix_dq0 ? 2 : 1;
  P.lock = d.lock_orientation;
  P.path_in_frame = d.path_in_frame;
  P.nx = (int)shape_of(h).nx;
  P.dt = d.dt;
  P.w_path = d.w_path;
  P.kappa = d.w_vel / (d.dt * d.dt);
  P.tol = optv(h, "tol") > 0.0 ? optv(h, "tol") : d.tol;  // (option "tol": the stopping tolerance of an existing trajectory handle, bench.py's second pass)
  P.tol_feas = d.tol_feas;
  P.tol_retract = fmin(1e-10, d.tol_feas);
  // (every handle since the end of round 3.  First built for handles with inequality rows; a tolerance sweep then showed the plain family in the
  //  same retraction-noise end game below tol = 1e-7 -- a tenth of a batch sitting at 1.5 x tol until the cap at 1e-9 -- and at the default 1e-6
  //  the rules cut the rejected steps from 1.7 % to 0.4 % and the median instance from 13 to 10 steps: 2.92 -> 3.0-3.1 M solves/s)
  P.tol_retract_min = fmin(optv(h, "retract_min"), P.tol_retract);  // (option: experiments)
  P.feas_accept = fmax(1e-8, 10.0 * d.tol_feas);
  P.max_retract = 4;
  P.max_iter = d.max_iter;
  P.hessian = d.hessian;
  // (The same switch for handles with limit rows.  Switching those earlier was measured and dropped: at 3e-5 x w_path 16 384 velocity-limited
  // instances take 20.4 instead of 22.0 steps on average with 99.95 % of them at the same optimum, at 1e-4 19.6 steps with 0.8 % forking -- but the
  // tail of the distribution moves about: of 24 576 instances one sits at the 600-step cap at 3e-5, takes 565 steps at 2e-5 and 166 at 5e-5, where
  // 1e-5 finishes every instance of every batch measured, 16 384 to 262 144, in at most 508; tools/gpu_vel_switch_quality.py, gpu_vel_24576_probe.py.)
  P.hyb_switch = optv(h, "hyb_switch") * d.w_path;  // (option: experiments)
  P.mu0 = d.mu0;
  P.relax = optv(h, "relax");
  P.relax_from = (int)optv(h, "relax_from");
  P.settle_k = optv(h, "settle_k");
  P.al_fuse = (int)optv(h, "al_fuse");
  P.local_path = h->d_local_path;
  P.np = (int)shape_of(h).npar;
  // coupling folded into evaluation and sweep (no k_couple launch): the plain orientation-locked handles, i.e. the batched path of config 2
  P.zc = (h->sch.fuse_couple && d.lock_orientation && !h->have_guards && !h->chain_host.has_lead) ? 1 : 0;
  P.zc_free = (h->sch.fuse_couple && !d.lock_orientation && !(h->have_guards && h->guards.vel_limits)) ? 1 : 0;
}

__global__ __launch_bounds__(256) static void k_gather_int(const int* __restrict__ src, int* __restrict__ dst, const int B, const int* __restrict__ newidx) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B && newidx[b] >= 0) dst[newidx[b]] = src[b];
}
// Every array of a running orientation-locked handle with inequality rows to its instance's new index (D.newidx from oh_launch_scan_running): both slots
// of the stage data, the pending step, multipliers, obstacle parameters, every per-instance scalar and flag.  Nothing restarts.
static int move_everything(oh_handle* h, hipStream_t s, int Bnew) {
  const int N = h->desc.ndof, NZ = N - 3, T = h->desc.T, Bp = h->D.Bp, B = h->D.B;
  FigBuffers& D = h->D;
  GuardBuffers& GB = h->GB;
  const GuardParams& GP = h->GP;
  struct Item { void* p; int rows; bool is_int; };
  std::vector<Item> items;
  auto dbl = [&](double* p, int rows) { if (p) items.push_back({p, rows, false}); };
  auto itg = [&](int* p) { if (p) items.push_back({p, 1, true}); };
  // What a handle's kernels never carry from one launch to the next stays behind: the folded-coupling family (P.zc) keeps no coupling blocks, reduced
  // gradients or per-knot tracking cost of its own (E, gt, phi: oh_figure8_units.h writes merit[] instead and the sweep rebuilds the rest), the Riccati gains
  // are written by the backward pass of a sweep and read by the forward pass of the same launch, and a chain without a lead joint has no lead[].
  const bool zc = h->P.zc != 0, slim = optv(h, "invariant_move_slim") != 0.0;
  // invariant_move_live (plain folded-coupling family only): of the per-slot stage data only the slot of the accepted point travels -- the other slot is the
  // trial the sweep has just judged: accepted, it IS the accepted slot by now; rejected, it is rewritten by the next evaluation before anything reads it.
  // The knots themselves travel in both slots (the pinned end knots of a slot are written once, by k_setup).
  struct Pair { double* a0; double* a1; int rows; };
  std::vector<Pair> live;
  const bool live_only = zc && !h->have_guards && optv(h, "invariant_move_live") != 0.0;
  if (live_only) {
    live.push_back({D.Z[0], D.Z[1], T * (3 * N - 3)}); live.push_back({D.Dr[0], D.Dr[1], T * (NZ * (NZ + 1) / 2)}); live.push_back({D.g[0], D.g[1], T * N});
    live.push_back({D.cv[0], D.cv[1], T}); live.push_back({D.Gfull[0], D.Gfull[1], T * N}); live.push_back({D.mdl[0], D.mdl[1], T * (3 + 3 * NZ)});
    live.push_back({D.merit[0], D.merit[1], T});
  }
  for (int sl = 0; sl < 2; ++sl) {
    dbl(D.q[sl], T * N);
    if (!live_only) {
      dbl(D.Z[sl], T * (3 * N - 3)); dbl(D.Dr[sl], T * (NZ * (NZ + 1) / 2)); dbl(D.g[sl], T * N); dbl(D.cv[sl], T);
      dbl(D.Gfull[sl], T * N); dbl(D.mdl[sl], T * (3 + 3 * NZ)); dbl(D.merit[sl], T);
    }
    if (!(zc && slim)) { dbl(D.phi[sl], T); dbl(D.E[sl], T * NZ * NZ); dbl(D.gt[sl], T * NZ); }
    dbl(GB.psi[sl], T); dbl(GB.mcv[sl], T);
  }
  dbl(D.zstep, T * NZ); dbl(D.ref, 12);
  if (!(zc && slim)) { dbl(D.Kmat, T * NZ * NZ); dbl(D.kvec, T * NZ); }
  if (h->chain_host.has_lead || !slim) dbl(D.lead, T);
  for (double* p : {D.fconst, D.f_cur, D.pred, D.mu, D.nun, D.stat, D.feas, D.fpsi, GB.rho, GB.rho_next, GB.omega, GB.meas_prev, GB.meas, GB.ls_gd, GB.ls_q}) dbl(p, 1);
  dbl(GB.lam, T * GP.NC); dbl(GB.lamv, GP.vel ? T * 2 * N : 0); dbl(GB.par, GP.n_links + 4 * GP.n_obs);
  for (int* p : {D.cur, D.first, D.skip, D.polish, D.stale, D.status, D.iters, D.orig, GB.outer, GB.n_outer, GB.ls_count}) itg(p);
  int max_rows = 1;
  for (const Item& it : items) max_rows = it.rows > max_rows ? it.rows : max_rows;
  for (const Pair& pr : live) max_rows = pr.rows > max_rows ? pr.rows : max_rows;
  const size_t need = sizeof(double) * ((size_t)max_rows + 1) * Bp;  // (+ one row: cur in the new order, for the live-slot moves)
  HIPCHK(h->move_scr.reserve(need));
  if (!live.empty()) {
    int* curn = (int*)((double*)h->move_scr.p + (size_t)max_rows * Bp);
    hipLaunchKernelGGL(k_gather_int, dim3((B + 255) / 256), dim3(256), 0, s, (const int*)D.cur, curn, B, (const int*)D.newidx);
    for (const Pair& pr : live) oh_launch_move_rows_live(s, pr.a0, pr.a1, (double*)h->move_scr.p, pr.rows, Bp, B, Bnew, D.newidx, D.cur, curn);
  }
  for (const Item& it : items) oh_launch_move_rows(s, it.p, h->move_scr.p, it.rows, Bp, B, Bnew, D.newidx, it.is_int);
  return OH_OK;
}

// ---- one batch, several streams (round 5) ----------------------------------------------------------------------------------------------------
// A solve of the plain orientation-locked family alternates bandwidth-bound launches over the whole batch with phases that leave the machine
// mostly idle: the persistent tail kernel (one wavefront per SIMD for milliseconds), the last launches before the hand-over, the compactions, the
// host's look at the running count after every iteration.  Two halves of the batch on two streams, each driven by a host thread of its own, fill
// each other's gaps: 262 144 instances 91.1 -> 84.6 ms on one box (2.88 -> 3.10 M solves/s; three parts 86.3, four 90.9: tools/gpu_two_streams.py).
// Instances are independent, so this is the multi-GPU sharding of DESIGN section 7 applied once more inside a GPU.  Each part is a handle of its own (peer:
// same description, constants, options, compiled kernels); profiling runs (events after every kernel) stay on one stream.
// peer handles of a trajectory / torque handle: same description, constants, dynamics and inequality rows, a stream of their own (parts of a split solve,
// lanes of the pipelined host-buffer solve)
static int ensure_peers(oh_handle* h, const int n) {
  const bool tqk = h->desc.kind == OH_PROBLEM_TORQUE_MPC;
  HIPCHK(hipSetDevice(h->device));  // peers are created on, and every part's host thread is bound to, the device of the handle (not the calling thread's)
  while ((int)h->peers.size() < n) {
    oh_handle* p = nullptr;
    int rc;
    if (tqk) rc = oh_create_torque(&h->tq, &p);
    else {
      oh_problem_desc d = h->desc;
      d.local_path = h->local_path.data();
      rc = oh_create(&d, &p);
    }
    if (rc) return rc;
    p->is_peer = true;
    p->device = h->device;
    rc = oh_set_constants(p, &h->chain_host);
    if (!rc && tqk) rc = oh_set_dynamics(p, &h->dyn_host);
    if (!rc && !tqk && h->have_guards) rc = oh_set_guards(p, &h->guards);
    if (rc) { delete p; return rc; }
    h->peers.push_back(p);
  }
  return OH_OK;
}
static int solve_device(oh_handle* h, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt, void* d_iters, void* d_status,
                        bool may_fan_out, LastSolve* rec);
// counters of the solves one lane ran, merged into the handle's timing by fan_out
struct Tally {
  double launched = 0, work = 0, compactions = 0, rejects = 0, tails = 0;
};
// one solve of a lane: never fans out again (the lanes ARE the streams)
static int lane_solve(oh_handle* q, Tally& t, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt, void* d_iters, void* d_status) {
  if (const int rc = solve_device(q, B, d_x0, d_p, d_x, d_f, d_kkt, d_iters, d_status, false, nullptr)) return rc;
  t.launched = std::max(t.launched, q->timing[5]);
  t.work += q->timing[6];
  t.compactions += q->timing[7];
  t.rejects += q->rejects;
  t.tails += q->tail_iters;
  return OH_OK;
}
// Runs work(lane, handle, tally) on n lanes: lane 0 is the handle itself on the calling thread, lanes 1 .. n-1 its peers, each on a host thread bound
// to the handle's device.  The first error of a lane is the call's; timing: [4] wall clock of the call, [5] the most launches of one solve, [6], [7],
// rejects, tail iterations summed over every solve of every lane.
template <class Work>
static int fan_out(oh_handle* h, const int n, Work&& work) {
  if (const int rc = ensure_peers(h, n - 1)) return rc;
  for (int i = 0; i + 1 < n; ++i) {  // the peers run with this handle's options and share the kernels compiled for its chain
    oh_handle* p = h->peers[i];
    p->sch = h->sch;
    p->opt = h->opt;
    p->spec = h->spec;
    p->spec_failed = h->spec_failed;
    p->spec_cache_checked = true;
  }
  std::vector<int> rcs(n, OH_OK);
  std::vector<std::string> errs(n);
  std::vector<Tally> tally(n);
  auto lane = [&](const int i) {
    oh_handle* q = i == 0 ? h : h->peers[i - 1];
    if (hipSetDevice(h->device) != hipSuccess) rcs[i] = fail(OH_ERR_HIP, "hipSetDevice failed on a lane's host thread");  // (a new host thread starts on device 0)
    else rcs[i] = work(i, q, tally[i]);
    if (rcs[i]) errs[i] = oh_last_error();
  };
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> th;
  for (int i = 1; i < n; ++i) th.emplace_back(lane, i);
  lane(0);
  for (std::thread& t : th) t.join();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (int i = 0; i < n; ++i)
    if (rcs[i]) return fail(rcs[i], errs[i]);
  reset_counters(h);
  h->timing[4] = ms;
  for (const Tally& t : tally) {
    h->timing[5] = std::max(h->timing[5], t.launched);
    h->timing[6] += t.work;
    h->timing[7] += t.compactions;
    h->rejects += t.rejects;
    h->tail_iters += t.tails;
  }
  return OH_OK;
}
// a batch in S contiguous parts, one per lane (parts start on multiples of 64: whole wavefronts of the thread-per-instance kernels)
static int solve_split(oh_handle* h, const int S, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt, void* d_iters, void* d_status,
                       LastSolve* rec) {
  const Shape sh = shape_of(h);
  std::vector<int> lo(S + 1, 0);
  for (int i = 1; i <= S; ++i) lo[i] = (int)((long long)B * i / S / 64 * 64);
  lo[S] = B;
  std::vector<LastSolve::Part> parts(S);
  const int rc = fan_out(h, S, [&](const int i, oh_handle* q, Tally& t) {
    const size_t o = (size_t)lo[i];
    auto off = [&](const void* ptr, const size_t bytes_per) -> void* { return ptr ? (void*)((char*)ptr + o * bytes_per) : nullptr; };
    parts[i] = {q, lo[i + 1] - lo[i]};
    return lane_solve(q, t, parts[i].n, off(d_x0, sh.nx * 8), off(d_p, sh.npar * 8), off(d_x, sh.nx * 8), off(d_f, 8), off(d_kkt, 24), off(d_iters, 4),
                      off(d_status, 4));
  });
  if (rc) return rc;
  rec->parts = parts;
  return OH_OK;
}

// ---- trajectory solve: a prologue, one loop per family (orientation-locked, position-tracking), an epilogue ----------------------------------
// A loop chooses its launches from the facts below, fixed before it, and re-tests only what a solve changes: D.B, a pending carried compaction,
// the cadence of the host's look at the running count, and that count.
struct Traj {
  int B, N, NV, check_every, hard_cap;  // batch, joints, velocity rows per knot, ...
  bool guarded, lead, prof, invariant;  // inequality rows, lead joint, profiling events, batch_invariant
  const FigSpec* spec;  // kernels compiled for the chain (plain orientation-locked handles), else nullptr
  FreeSweep sweep;      // position-tracking family: the sweep of the first launch
  const double* p;
  double *x, *f, *kkt;
  int *iters, *status;
  int launched, compactions;
  size_t ne;  // profiling events recorded
};
// The one place that chooses the sweep of a position-tracking launch of nb instances (the launchers in oh_free.hip take the choice).  start: nb is
// the batch of a solve that is starting; the choice then also fixes the stage layout of the whole solve -- instance-major when every launch takes
// the twisted factorisation, which holds to the end once it holds for the whole batch -- and may give the whole solve to one launch.
static FreeSweep free_sweep(oh_handle* h, const int nb, const bool start = false) {
  const int N = h->desc.ndof, nK = h->desc.T - h->P.t0;
  FreeSweep sw = FREE_SERIAL;
  // a block per instance for 6 and 7 joints, at most free_pcr_max instances and 128 knots (batch_invariant: the serial sweep whatever the batch --
  // the block-per-instance factorisations chosen by size round differently)
  if (!h->P.lock && batch_invariant(h) == 0.0 && nb <= h->sch.free_pcr_max && nK <= 128 && (N == 6 || N == 7)) {
    if (N == 7 && (int)optv(h, "free_bb") != 0) sw = FREE_BB;  // (free_bb = 0: the cyclic-reduction kernels of rounds 2-3; A/B, tests)
    // eight lanes per knot up to free_cp_max instances, and only up to 64 knots: 128 knots x 8 lanes are 1024 threads, which leaves 128 registers
    // per lane -- the kernel then spills and takes 147 us against k_step_free_pcr's 111 at T = 100; at T = 50 it is 61 against 87 us
    else sw = (nb <= (int)optv(h, "free_cp_max") && nK <= 64) ? FREE_CP : FREE_PCR;
  }
  if (!start) return sw;
  h->P.inst_major = sw == FREE_BB ? 1 : 0;
  // limit / sphere rows: the whole solve in one launch (k_free_persist).  Measured (HISTORY): same time per iteration as the launch pair (the
  // iteration is memory round trips inside the phases, not launch gaps), so it only wins where the host's sparse looks at the running count cost
  // idle launches and every block is resident: horizons up to 64 free knots, at most 512 instances (option free_persist = 1: always, 0: never)
  const int fp = (int)optv(h, "free_persist");
  const bool fits = (nK <= 64 && nb <= 512) || fp == 1;
  return (sw == FREE_BB && h->have_guards && !h->GP.vel && h->P.zc_free && !h->profiling && fits && fp != 0) ? FREE_PERSIST : sw;
}
// oh_set_profiling(1): an event, tagged 0 (a new base: nothing is billed for the gap before it), 1 after an evaluation, 2 after a sweep, 3 after a
// coupling, 4 after the evaluation before a carried compaction; none once fewer than `room` events are left
static int mark(oh_handle* h, Traj& r, const int tag, const size_t room = 2) {
  if (!r.prof || r.ne + room >= h->prof_events.size()) return OH_OK;
  size_t& ne = r.ne;
  hipStream_t s = h->stream;
  HIPCHK(hipEventRecord(h->prof_events[ne++], s));
  h->prof_tags.push_back(tag);
  return OH_OK;
}
// After iteration it the host looks at the running count (a copy + stream synchronisation, 20-30 us of a ~150 us iteration): every check_every-th
// iteration, or -- handles without a persistent tail kernel, whose last launches of a few hundred instances are pure latency -- every 8th (the
// price: up to 7 idle iterations of finished instances at the very end)
static bool check_after(const oh_handle* h, const Traj& r, const int it, const bool tail_ok) {
  return (it + 1) % ((!tail_ok && r.check_every == 1 && h->D.B <= h->sch.sparse_check_below) ? 8 : r.check_every) == 0;
}
// the running count the last sweep left, when the host looks (check); -1 otherwise
static int look(oh_handle* h, const bool check, int* nrun) {
  *nrun = -1;
  if (!check) return OH_OK;
  hipStream_t s = h->stream;
  HIPCHK(hipMemcpyAsync(h->h_flag, h->D.n_running, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *nrun = *h->h_flag;
  return OH_OK;
}
// results of finished instances (only_done) or of all: x through the library's LDS transpose, scalars and multipliers through the kernel compiled
// for the chain where there is one
static void finalize(oh_handle* h, const Traj& r, const int only_done) {
  hipStream_t s = h->stream;
  if (r.spec && r.spec->finalize) {
    oh_launch_finalize(s, r.N, h->P, h->D, only_done, r.x, r.f, r.kkt, r.iters, r.status, 1);
    if (oh_spec_launch_finalize(*r.spec, s, h->P, h->D, only_done, r.f, r.kkt, r.iters, r.status) == hipSuccess) return;
    (void)hipGetLastError();
    oh_launch_finalize(s, r.N, h->P, h->D, only_done, r.x, r.f, r.kkt, r.iters, r.status, 2);
    return;
  }
  oh_launch_finalize(s, r.N, h->P, h->D, only_done, r.x, r.f, r.kkt, r.iters, r.status);
}
// The batch down to its nrun survivors: finished instances' results (and multipliers) are written out, the survivors ordered (D.newidx); then they
// move with everything they own (move: nothing restarts), or their accepted knots -- with inequality rows also their multipliers and outer-loop
// state -- are laid down densely and re-evaluated from `slot`.
static int compact_batch(oh_handle* h, Traj& r, const int nrun, const int slot, const bool move) {
  hipStream_t s = h->stream;
  finalize(h, r, 1);
  if (r.guarded) oh_launch_guard_emit(s, h->P, h->D, h->GP, h->GB, r.NV, 1);
  oh_launch_scan_running(s, h->D, h->sch.compact_sort);
  if (move) {
    if (const int rc = move_everything(h, s, nrun)) return rc;
  } else {
    oh_launch_compact(s, r.N, h->P, h->D, 0, 0, 0);
    if (r.guarded) oh_launch_guard_compact(s, h->P, h->D, h->GP, h->GB, r.NV, 0, 0);
    oh_launch_compact(s, r.N, h->P, h->D, 1, nrun, slot);
    if (r.guarded) oh_launch_guard_compact(s, h->P, h->D, h->GP, h->GB, r.NV, 1, nrun);
  }
  h->D.B = nrun;
  ++r.compactions;
  return OH_OK;
}
static int traj_prologue(oh_handle* h, Traj& r, const void* d_x0) {
  if (const int rc = ensure_capacity(h, r.B)) return rc;
  fill_params(h);
  if ((spec_applies(h) || spec_tail_vel_applies(h)) && !h->spec && !h->spec_failed) {
    bool want = h->sch.specialize == OH_SPECIALIZE_ALWAYS || (h->sch.specialize == OH_SPECIALIZE_AUTO && r.B >= h->specialize_min_B);
    if (!want && h->sch.specialize == OH_SPECIALIZE_AUTO && !h->spec_cache_checked) {  // a compiled object is at hand: milliseconds, whatever the batch
      h->spec_cache_checked = true;
      want = oh_jit_figure8_cached(h->chain_host, h->desc.ndof);
    }
    if (want && oh_specialize(h) != OH_OK) h->spec_failed = true;
  }  // the generic kernels run (and no further attempt is made); oh_last_error keeps the reason
  if (r.lead && (r.guarded || !h->desc.lock_orientation || h->desc.ndof != 6))
    return fail(OH_ERR_INVALID, "oh_solve_device: a parameterised lead joint is lowered for the orientation-locked family with 6 optimised joints, "
                                "without inequality rows");
  if (!r.guarded) h->D.fpsi = nullptr;
  else if (const int rc = ensure_guards(h)) return rc;
  r.sweep = free_sweep(h, r.B, true);  // (and the stage layout, P.inst_major)
  r.NV = (r.guarded && h->GP.vel) ? 2 * r.N : 0;
  r.spec = spec_applies(h) ? h->spec : nullptr;
  // one small D2H read per iteration: with the cheap compaction timely decisions beat the saved round trips (every 2nd: -1.5 %)
  r.check_every = optv(h, "check_every") >= 1.0 ? (int)optv(h, "check_every") : 1;  // (option: experiments)
  // every instance needs at most max_iter steps (accepted + rejected) plus its first evaluation: a rejected step costs two launches, a compaction one
  r.hard_cap = 2 * h->desc.max_iter + 2 + 40 + 64;
  hipStream_t s = h->stream;
  if (r.prof) {
    // events: [0] start, then per iteration (after eval, after step), last = end
    const size_t need = 4 * (size_t)(2 * h->desc.max_iter + 44) + 64;
    while (h->prof_events.size() < need) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      h->prof_events.push_back(e);
    }
  }
  HIPCHK(hipEventRecord(h->ev0, s));
  HIPCHK(hipMemsetAsync(h->D.work, 0, 4 * sizeof(unsigned long long), s));  // (work[0..2] and the two deferral counters)
  if (!oh_launch_setup(s, r.N, h->P, h->D, (const double*)d_x0, r.p)) return fail(OH_ERR_INVALID, "oh_solve_device: unsupported ndof");
  if (r.guarded) oh_launch_setup_guards(s, r.N, h->P, h->D, h->GP, h->GB, r.p);
  h->prof_tags.clear();
  return mark(h, r, 0);
}
// the persistent one-wavefront-per-instance kernel (k_tail; k_tail_vel for limit rows), compiled for the chain where there is one
static bool launch_tail(oh_handle* h, const Traj& r, const bool tail_vel, const int slot) {
  hipStream_t s = h->stream;
  if (tail_vel && h->spec && spec_tail_vel_applies(h)) return oh_spec_launch_tail_vel(*h->spec, s, h->P, h->D, h->GP, h->GB, slot) == hipSuccess;
  if (tail_vel) return oh_launch_tail_vel(s, r.N, h->P, h->D, h->GP, h->GB, slot);
  if (r.spec) return oh_spec_launch_tail(*r.spec, s, h->P, h->D, slot) == hipSuccess;
  return oh_launch_tail(s, r.N, h->P, h->D, slot);
}
static void launch_eval(oh_handle* h, const Traj& r, const int slot, const int part) {
  if (!r.spec) oh_launch_eval(h->stream, r.N, h->P, h->D, slot, part);
  else oh_spec_launch_eval(*r.spec, h->stream, h->P, h->D, slot, part);
}

// The orientation-locked family (plain, with inequality rows or with a lead joint).  The batch is compacted whenever 3 % of it have finished
// (compact_frac): the regular compactions carry the pending trial along and cost no evaluation (k_carry_*), the hand-over to the tail kernel restarts.
static int locked_loop(oh_handle* h, Traj& r) {
  FigParams& P = h->P; FigBuffers& D = h->D; const GuardParams& GP = h->GP; const GuardBuffers& GB = h->GB;
  const hipStream_t s = h->stream;
  const int N = r.N;
  // persistent tail kernel: plain handles, and (round 3, k_tail_vel) those whose inequality rows are joint and / or joint-velocity limits (no sphere rows)
  const bool tail_vel = r.guarded && (GP.vel || GP.limits) && GP.n_links == 0 && h->sch.tail_vel;
  const bool tail_ok = (h->desc.T - P.t0 <= 64) && h->sch.tail_threshold > 0 && (!r.guarded || tail_vel) && !r.lead;
  // limit / velocity-limit handles: the batched launches (evaluation, velocity coupling in a launch of its own, sweep: 1.45 ms per iteration of
  // 40 000 instances) lose against the persistent kernel at every size measured -- 65 536 instances: 87.5 ms with the hand-over at 16 384,
  // 80.5 at 32 768, 76.3 when the whole batch starts there -- so these handles go to it whatever the batch (OH_TAIL_VEL_THRESHOLD overrides)
  const int tail_threshold = tail_vel ? h->sch.tail_vel_threshold : h->sch.tail_threshold;
  if (tail_ok && r.B <= tail_threshold) {  // small batch: the whole solve is one persistent launch
    if (!launch_tail(h, r, tail_vel, 0)) return fail(OH_ERR_INVALID, "oh_solve_device: no persistent kernel for this handle (ndof / rows)");
    return OH_OK;
  }
  // limit rows without sphere rows: retraction and evaluation as two launches like the plain family (k_evalb_lg in oh_kernels.hip)
  const bool lg_split = r.guarded && h->sch.lg_split && GP.n_links == 0, lg_spec = lg_split && h->spec && spec_tail_vel_applies(h);
  // coupling: folded into evaluation and sweep (P.zc: k_evalb_zc / k_step_zc), with the velocity rows (k_couple_vel), or k_couple
  const bool couple_vel = !P.zc && r.guarded && GP.vel, couple = !P.zc && !couple_vel;
  // compactions: carried (plain handles; k_carry_* park 22 per-instance scalars in the first rows of the spare Dr slot: T x NZ(NZ+1)/2 rows must
  // hold them), moving (batch_invariant), restarting -- with inequality rows moving too (round 5: the same iterates, bit for bit); a lead joint: none
  const bool carry = h->sch.compaction && h->sch.compact_carry && (size_t)h->desc.T * ((N - 3) * (N - 2) / 2) >= 22 && !r.guarded && !r.lead;
  const double inv_frac = optv(h, "invariant_compact_frac");
  const bool inv_move = r.invariant && !r.lead && inv_frac > 0.0, restart = h->sch.compaction && !r.lead, restart_moves = r.guarded && optv(h, "compact_move_all") != 0.0;
  int nrun = -1, carry_pending = 0;  // the running count at the last look (-1: none after the last iteration); > 0: a carried compaction to this many
  for (int it = 0; it < r.hard_cap; ++it) {
    if (nrun >= 0)  // host synced: do not bill the idle gap to the eval kernel
      if (const int rc = mark(h, r, 0, 3)) return rc;
    const int slot = it & 1;
    if (lg_split) {
      if (!(lg_spec && oh_spec_launch_eval(*h->spec, s, P, D, slot, 1) == hipSuccess)) oh_launch_eval_locked_guarded(s, N, P, D, GP, GB, slot, 1);
      oh_launch_eval_locked_guarded(s, N, P, D, GP, GB, slot, 2);
    } else if (r.guarded) oh_launch_eval_locked_guarded(s, N, P, D, GP, GB, slot, 0);
    else if (r.lead) oh_launch_eval_lead(s, N, P, D, slot);
    else if (carry_pending > 0) {
      // compaction with the trial carried along: retract on the old layout, move, evaluate on the dense one (k_carry_* in oh_kernels.hip)
      bool moved = false, scanned = false;
      if (r.spec && r.spec->retract_move && h->sch.compact_fused && !h->spec_move_failed) {
        // the new indices first (the scan reads status and stat, final since the last sweep; the retraction writes neither): the retraction compiled
        // for the chain then lays the free knots down where they go, and what is left to gather are the pinned knots and the scalars
        finalize(h, r, 1);
        oh_launch_scan_running(s, D, h->sch.compact_sort);
        scanned = true;
        if (const int rc = mark(h, r, 0)) return rc;
        moved = oh_spec_launch_eval(*r.spec, s, P, D, slot, 3) == hipSuccess;
        if (moved) {
          if (const int rc = mark(h, r, 4)) return rc;
          oh_launch_carry(s, N, P, D, 2, 0, slot);
        } else {
          (void)hipGetLastError();
          h->spec_move_failed = true;
        }
      }
      if (!moved) {
        launch_eval(h, r, slot, 1);
        if (const int rc = mark(h, r, 4)) return rc;
        if (!scanned) {  // (after a failed launch of the moving retraction the results are out and the scan is done already)
          finalize(h, r, 1);
          oh_launch_scan_running(s, D, h->sch.compact_sort);
        }
        oh_launch_carry(s, N, P, D, 0, 0, slot);
      }
      oh_launch_carry(s, N, P, D, 1, carry_pending, slot);
      // the knots were laid down densely in the spare arrays: they become q[] / Gfull[] for the launches that follow (no copy back)
      std::swap(D.q[slot], D.q_spare[0]);
      std::swap(D.q[1 - slot], D.q_spare[1]);
      if (P.hessian != OH_HESSIAN_GAUSS_NEWTON || P.zc) std::swap(D.Gfull[1 - slot], D.G_spare);
      D.B = carry_pending;
      carry_pending = 0;
      ++r.compactions;
      if (const int rc = mark(h, r, 0)) return rc;
      launch_eval(h, r, slot, 2);
    } else launch_eval(h, r, slot, 0);
    if (const int rc = mark(h, r, 1)) return rc;
    if (couple_vel) oh_launch_couple_vel(s, N, P, D, GP, GB, slot);
    else if (couple) oh_launch_couple(s, N, P, D, slot);
    const bool check = check_after(h, r, it, tail_ok);  // (k_couple resets the running count)
    if (const int rc = mark(h, r, 3)) return rc;
    if (r.guarded) oh_launch_step_locked_guarded(s, N, P, D, GP, GB, slot);
    else oh_launch_step(s, N, P, D, slot);
    if (const int rc = mark(h, r, 2)) return rc;
    ++r.launched;
    if (const int rc = look(h, check, &nrun)) return rc;
    if (nrun == 0) break;
    if (tail_ok && nrun > 0 && nrun <= tail_threshold) {
      // drain: compact the survivors and let one wavefront per instance finish them without further launches
      if (const int rc = compact_batch(h, r, nrun, (it + 1) & 1, false)) return rc;
      if (!launch_tail(h, r, tail_vel, (it + 1) & 1)) return fail(OH_ERR_INVALID, "oh_solve_device: no persistent kernel for this handle (ndof / rows)");
      break;
    }
    if (nrun < 0 || D.B < 512) continue;
    if (carry && (double)nrun <= h->sch.compact_frac * (double)D.B) {
      carry_pending = nrun;  // done after the next k_retract
    } else if (inv_move && (double)nrun <= inv_frac * (double)D.B) {  // (a coarse schedule: a move costs a few iterations' bandwidth)
      if (const int rc = compact_batch(h, r, nrun, 0, true)) return rc;
      if (const int rc = mark(h, r, 0)) return rc;
    } else if (restart && (double)nrun <= h->sch.compact_frac_restart * (double)D.B) {
      if (const int rc = compact_batch(h, r, nrun, (it + 1) & 1, restart_moves)) return rc;
      if (const int rc = mark(h, r, 0)) return rc;  // (the compaction kernels are accounted to neither eval nor step: restart the event pair)
    }
  }
  return OH_OK;
}
// The position-tracking family (oh_free.hip): restarting compactions (compact_frac_restart); the sweep follows the live batch (free_sweep).
static int free_loop(oh_handle* h, Traj& r) {
  FigParams& P = h->P; FigBuffers& D = h->D; const GuardParams& GP = h->GP; const GuardBuffers& GB = h->GB;
  const hipStream_t s = h->stream;
  const int N = r.N;
  FreeSweep sweep = r.sweep;  // (changes with D.B)
  h->free_sweep_last = (int)sweep;
  h->free_sweeps_used = 1 << (int)sweep;
  if (sweep == FREE_PERSIST) {
    if (!oh_launch_free_persist(s, N, P, D, GP, GB)) return fail(OH_ERR_INVALID, "oh_solve_device: no persistent kernel for this handle (ndof / rows)");
    r.launched = 1;
    return OH_OK;
  }
  // coupling: folded into the evaluation (P.zc_free), with the velocity rows (k_couple_free_vel), or k_couple_free
  const bool couple_vel = !P.zc_free && r.guarded && GP.vel, couple = !P.zc_free && !couple_vel;
  int nrun = -1;
  for (int it = 0; it < r.hard_cap; ++it) {
    if (nrun >= 0)  // host synced: do not bill the idle gap to the eval kernel
      if (const int rc = mark(h, r, 0, 3)) return rc;
    const int slot = it & 1;
    if (r.guarded) oh_launch_eval_guarded(s, N, P, D, GP, GB, slot);
    else oh_launch_eval_free(s, N, P, D, slot);
    if (const int rc = mark(h, r, 1)) return rc;
    if (couple_vel) oh_launch_couple_free_vel(s, N, P, D, GP, GB, slot);
    else if (couple) oh_launch_couple_free(s, N, P, D, slot);
    const bool check = check_after(h, r, it, false);
    if (check) HIPCHK(hipMemsetAsync(h->D.n_running, 0, sizeof(int), s));  // (the sweep counts the instances still running)
    if (const int rc = mark(h, r, 3)) return rc;
    if (r.guarded) oh_launch_step_guarded(s, N, P, D, GP, GB, slot, sweep);
    else oh_launch_step_free(s, N, P, D, slot, sweep);
    if (const int rc = mark(h, r, 2)) return rc;
    ++r.launched;
    if (const int rc = look(h, check, &nrun)) return rc;
    if (nrun == 0) break;
    if (nrun > 0 && h->sch.compaction && D.B >= 512 && (double)nrun <= h->sch.compact_frac_restart * (double)D.B) {
      if (const int rc = compact_batch(h, r, nrun, (it + 1) & 1, false)) return rc;
      sweep = free_sweep(h, D.B);
      h->free_sweeps_used |= 1 << (int)sweep;
      if (const int rc = mark(h, r, 0)) return rc;  // (the compaction kernels are accounted to neither eval nor step: restart the event pair)
    }
  }
  return OH_OK;
}
static int traj_epilogue(oh_handle* h, Traj& r) {
  hipStream_t s = h->stream;
  finalize(h, r, 0);
  if (r.guarded) oh_launch_guard_emit(s, h->P, h->D, h->GP, h->GB, r.NV, 0);
  h->D.B = r.B;
  if (r.guarded) oh_launch_guard_infeasible(s, r.N, h->P, h->D, h->GP, r.p, r.B, r.kkt, r.status);  // constant rows of the pinned knots
  if (const int frc = finish_solve(h, r.launched)) return frc;
  unsigned long long work[3] = {0, 0, 0};
  // (on the handle's own stream: a hipMemcpy is an operation of the legacy null stream and waits for the kernels of every other handle's stream -- the other
  //  part of a split solve, the other lane of a pipelined one)
  HIPCHK(hipMemcpyAsync(work, h->D.work, sizeof(work), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  h->timing[6] = (double)work[0];
  h->rejects = (double)work[1];
  h->tail_iters = (double)work[2];
  if (r.prof) {  // device time by tag (mark): evaluation (1 and 4), sweep, coupling; launches: evaluations (1), sweeps
    double ms[4] = {0, 0, 0, 0};
    int n[5] = {0, 0, 0, 0, 0};
    for (size_t i = 1; i < r.ne; ++i) {
      const int tag = h->prof_tags[i];
      float m = 0.f;
      if (tag) hipEventElapsedTime(&m, h->prof_events[i - 1], h->prof_events[i]);
      ms[tag == 4 ? 1 : tag] += m;
      ++n[tag];
    }
    h->timing[0] = ms[1]; h->timing[1] = n[1]; h->timing[2] = ms[2]; h->timing[3] = n[2]; h->timing_couple = ms[3];
  }
  h->timing[7] = r.compactions;
  return OH_OK;
}
static int traj_solve_device(oh_handle* h, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt, void* d_iters, void* d_status) {
  Traj r{};
  r.B = B; r.N = h->desc.ndof;
  r.guarded = h->have_guards; r.lead = h->chain_host.has_lead != 0; r.prof = h->profiling; r.invariant = batch_invariant(h) != 0.0;
  r.p = (const double*)d_p; r.x = (double*)d_x; r.f = (double*)d_f; r.kkt = (double*)d_kkt; r.iters = (int*)d_iters; r.status = (int*)d_status;
  if (const int rc = traj_prologue(h, r, d_x0)) return rc;
  if (const int rc = h->P.lock ? locked_loop(h, r) : free_loop(h, r)) return rc;
  return traj_epilogue(h, r);
}

// Parts a batch of the torque, orientation-locked or position-tracking family is solved in (solve_split; 1: this handle alone).  A lane (may_fan_out
// false) and a profiled handle never split.
static int split_parts(const oh_handle* h, const int B, const bool may_fan_out) {
  const int S = std::min(8, (int)optv(h, "streams"));
  if (!may_fan_out || h->profiling || S < 2) return 1;
  if (h->desc.kind == OH_PROBLEM_TORQUE_MPC) return (B >= (int)optv(h, "tq_split_min") && B / S >= 64 && h->have_chain && h->have_dyn) ? S : 1;
  // (batch_invariant handles take part in the split too since their compaction moves everything: an instance's answer does not depend on its part;
  //  a batch beyond oh_max_batch is refused by ensure_capacity, as ever)
  if (spec_applies(h) && (batch_invariant(h) == 0.0 || optv(h, "invariant_split") != 0.0) && B >= (int)optv(h, "split_min") && B / S >= 4096 && stage_fits(h, B))
    return S;
  // position-tracking family (every launch latency-bound, the machine far from full): two halves side by side -- 1024 arms 9.5 -> 7.3 ms
  return (!h->desc.lock_orientation && !h->chain_host.has_lead && batch_invariant(h) == 0.0 && B >= (int)optv(h, "free_split_min") && B / S >= 64) ? S : 1;
}

// The solve of every entry point and every lane, by problem kind: without may_fan_out the batch is never split.  rec (may be null): where the
// results live, on success.
static int solve_device(oh_handle* h, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt, void* d_iters, void* d_status,
                        const bool may_fan_out, LastSolve* rec) {
  if (B < 1) return fail(OH_ERR_INVALID, "oh_solve_device: B must be >= 1");
  if (!d_x0 || !d_p) return fail(OH_ERR_INVALID, "oh_solve_device: x0 and p are required");
  if (rec) *rec = LastSolve{B, {{h, B}}, false};
  switch (h->desc.kind) {
    case OH_PROBLEM_POINT_MASS_MPC: return pm_solve_device(h, B, d_x0, d_p, d_x, d_f, d_kkt, d_iters, d_status);
    case OH_PROBLEM_IK: return ik_solve_device(h, B, d_x0, d_p, d_x, d_f, d_kkt, d_iters, d_status);
    case OH_PROBLEM_QP: return qp_solve_device(h, B, d_x0, d_p, d_x, d_f, d_kkt, d_iters, d_status);
    case OH_PROBLEM_TAPE: return tape_solve_device(h, B, d_x0, d_p, d_x, d_f, d_kkt, d_iters, d_status);
    case OH_PROBLEM_TORQUE_MPC: break;
    case OH_PROBLEM_FIGURE_EIGHT:
      if (!h->have_chain) return fail(OH_ERR_STATE, "oh_solve_device: call oh_set_constants first");
      if (!solver_chain_ok(h->chain_host)) return fail(OH_ERR_INVALID, "oh_solve_device: the solver needs a chain that covers every model joint in order");
      HIPCHK(hipSetDevice(h->device));
      break;
    default: return fail(OH_ERR_STATE, "oh_solve_device: handle was created without a problem (OH_PROBLEM_KINEMATICS)");
  }
  if (const int S = split_parts(h, B, may_fan_out); S > 1) {
    // (the kernels compiled for the chain are shared: make sure they exist before the parts look for them)
    if (spec_applies(h) && !h->spec && !h->spec_failed && h->sch.specialize != OH_SPECIALIZE_NEVER && oh_specialize(h) != OH_OK) h->spec_failed = true;
    return solve_split(h, S, B, d_x0, d_p, d_x, d_f, d_kkt, d_iters, d_status, rec);
  }
  if (h->desc.kind == OH_PROBLEM_TORQUE_MPC) return tq_solve_device(h, B, d_x0, d_p, d_x, d_f, d_kkt, d_iters, d_status);
  return traj_solve_device(h, B, d_x0, d_p, d_x, d_f, d_kkt, d_iters, d_status);
}

extern "C" int oh_solve_device(oh_handle* h, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt,
                               void* d_iters, void* d_status) {
  if (!h) return fail(OH_ERR_INVALID, "oh_solve_device: null handle");
  h->last = LastSolve{};
  LastSolve rec;
  const int rc = solve_device(h, B, d_x0, d_p, d_x, d_f, d_kkt, d_iters, d_status, !h->is_peer, &rec);
  if (rc == OH_OK) h->last = rec;
  return rc;
}

static int ensure_stage(oh_handle* h, size_t bytes) {
  const hipError_t e = h->stage.reserve(bytes);
  if (e != hipSuccess) return fail(OH_ERR_HIP, std::string("staging allocation failed: ") + hipGetErrorString(e));
  return OH_OK;
}
// the staging area of a host-buffer solve of n instances on handle q (layout_stage), grown as needed
static int stage_solve(oh_handle* q, const Shape& sh, const size_t n, StageLayout& L) {
  return stage_carve(q, [&](Carver c) {
    layout_stage(c, L, sh, n);
    return c.bytes();
  });
}

// device pointer of a handle's multipliers, [B][shape.mult] (nullptr: none, or the guarded SoA layout that copy_multipliers transposes)
static const double* mult_ptr(const oh_handle* q) {
  switch (q->desc.kind) {
    case OH_PROBLEM_TORQUE_MPC: return q->d_tq_mult;
    case OH_PROBLEM_TAPE: return q->d_tape_mult;
    case OH_PROBLEM_QP: return q->d_qp_mult;
    case OH_PROBLEM_IK: return q->d_ik_mult;
    case OH_PROBLEM_FIGURE_EIGHT: return q->have_guards ? nullptr : q->D.lam_h;
    default: return nullptr;
  }
}
// the multipliers of the n instances handle q holds from the last solve, into the caller's layout [n][shape.mult]
static int copy_multipliers(const oh_handle* q, const int n, double* out) {
  const size_t per = shape_of(q).mult;
  if (!per) return OH_OK;
  if (!(q->desc.kind == OH_PROBLEM_FIGURE_EIGHT && q->have_guards)) {
    HIPCHK(hipMemcpy(out, mult_ptr(q), sizeof(double) * per * n, hipMemcpyDeviceToHost));
    return OH_OK;
  }
  // SoA [T][NC][Bp] on the device -> [B][T][NC (+ 2 ndof velocity rows)] for the caller
  const int T = q->desc.T, NC = q->GP.NC, Bp = q->D.Bp, NV = q->GP.vel ? 2 * q->desc.ndof : 0, NT = NC + NV;
  std::vector<double> tmp((size_t)T * NC * Bp);
  if (NC) HIPCHK(hipMemcpy(tmp.data(), q->GB.lam_out, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));  // original order (k_guard_emit)
  for (int b = 0; b < n; ++b)
    for (int t = 0; t < T; ++t)
      for (int i = 0; i < NC; ++i) out[((size_t)b * T + t) * NT + i] = tmp[((size_t)t * NC + i) * Bp + b];
  if (NV) {  // the device keeps the rows of dq_t = interval (t, t+1) in row block t + 1
    std::vector<double> tv((size_t)T * NV * Bp);
    HIPCHK(hipMemcpy(tv.data(), q->GB.lamv_out, tv.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int b = 0; b < n; ++b)
      for (int t = 0; t < T; ++t)
        for (int i = 0; i < NV; ++i) out[((size_t)b * T + t) * NT + NC + i] = (t + 1 < T) ? tv[((size_t)(t + 1) * NV + i) * Bp + b] : 0.0;
  }
  return OH_OK;
}

// oh_solve of a large batch: chunks of `chunk` instances alternate between two lanes; a lane uploads its chunk on its own stream, solves it on its own
// handle (lane 0: the handle itself, lane 1: a peer) and downloads the results, while the other lane is one phase ahead or behind.  Every chunk is solved
// as a batch of its own (like the parts of solve_split); timing[4] is the wall clock of the whole call.
static int solve_pipelined(oh_handle* h, const int B, const int chunk, const double* x0, const double* p, double* x, double* f, double* kkt, int* iters,
                           int* status) {
  if (spec_applies(h) && !h->spec && !h->spec_failed && h->sch.specialize != OH_SPECIALIZE_NEVER && chunk >= h->specialize_min_B && oh_specialize(h) != OH_OK)
    h->spec_failed = true;
  // multipliers of every chunk, kept on the device in instance order for oh_get_multipliers (a handle only remembers its last solve)
  const Shape sh = shape_of(h);
  HIPCHK(h->d_pipe_mult.reserve(sh.mult * B));
  const int C = (B + chunk - 1) / chunk;
  return fan_out(h, 2, [&](const int l, oh_handle* q, Tally& t) {
    for (int c = l; c < C; c += 2) {
      const size_t lo = (size_t)c * chunk;
      const int n = (int)std::min((size_t)chunk, (size_t)B - lo);
      StageLayout L{};
      if (const int rc = stage_solve(q, sh, (size_t)n, L)) return rc;
      hipStream_t s = q->stream;
      bool ok = hipMemcpyAsync(L.x0, x0 + lo * sh.nx, L.b_x, hipMemcpyHostToDevice, s) == hipSuccess &&
                hipMemcpyAsync(L.p, p + lo * sh.npar, L.b_p, hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
      if (!ok) return fail(OH_ERR_HIP, "oh_solve: upload failed");
      if (const int rc = lane_solve(q, t, n, L.x0, L.p, L.x, L.f, L.kkt, L.iters, L.status)) return rc;
      const double* mult = mult_ptr(q);
      if (sh.mult && mult) ok = ok && hipMemcpyAsync(h->d_pipe_mult.p + lo * sh.mult, mult, sizeof(double) * sh.mult * n, hipMemcpyDeviceToDevice, s) == hipSuccess;
      if (x) ok = ok && hipMemcpyAsync(x + lo * sh.nx, L.x, L.b_x, hipMemcpyDeviceToHost, s) == hipSuccess;
      if (f) ok = ok && hipMemcpyAsync(f + lo, L.f, L.b_f, hipMemcpyDeviceToHost, s) == hipSuccess;
      if (kkt) ok = ok && hipMemcpyAsync(kkt + 3 * lo, L.kkt, L.b_k, hipMemcpyDeviceToHost, s) == hipSuccess;
      if (iters) ok = ok && hipMemcpyAsync(iters + lo, L.iters, L.b_i, hipMemcpyDeviceToHost, s) == hipSuccess;
      if (status) ok = ok && hipMemcpyAsync(status + lo, L.status, L.b_i, hipMemcpyDeviceToHost, s) == hipSuccess;
      ok = ok && hipStreamSynchronize(s) == hipSuccess;
      if (!ok) return fail(OH_ERR_HIP, "oh_solve: download failed");
    }
    return (int)OH_OK;
  });
}

extern "C" int oh_solve(oh_handle* h, int B, const double* x0, const double* p, double* x, double* f, double* kkt, int* iters,
                        int* status) {
  if (!h) return fail(OH_ERR_INVALID, "oh_solve: null handle");
  if (B < 1) return fail(OH_ERR_INVALID, "oh_solve: B must be >= 1");
  if (!x0 || !p) return fail(OH_ERR_INVALID, "oh_solve: x0 and p are required");
  if (h->desc.kind != OH_PROBLEM_FIGURE_EIGHT && h->desc.kind != OH_PROBLEM_POINT_MASS_MPC && h->desc.kind != OH_PROBLEM_IK &&
      h->desc.kind != OH_PROBLEM_QP && h->desc.kind != OH_PROBLEM_TAPE && h->desc.kind != OH_PROBLEM_TORQUE_MPC)
    return fail(OH_ERR_STATE, "oh_solve: handle was created without a problem (OH_PROBLEM_KINEMATICS)");
  HIPCHK(hipSetDevice(h->device));
  h->last = LastSolve{};
  // large batches of the trajectory families from host buffers: chunks on two lanes (handles, streams, host threads), so that one lane's transfers over
  // PCIe run under the other lane's kernels (round 6; until then: upload everything, solve, download everything -- 38 % of the resident rate).  Such a
  // call stages chunks only: the whole batch is never staged.
  const bool tqk = h->desc.kind == OH_PROBLEM_TORQUE_MPC;
  const int chunk = std::max(1024, (int)optv(h, "pipe_chunk"));
  if ((h->desc.kind == OH_PROBLEM_FIGURE_EIGHT || tqk) && !h->is_peer && !h->profiling && optv(h, "pipe") != 0.0 && h->have_chain && !h->have_guards &&
      !h->chain_host.has_lead && B >= 2 * chunk && (!tqk || h->have_dyn)) {
    const int rc = solve_pipelined(h, B, chunk, x0, p, x, f, kkt, iters, status);
    if (rc == OH_OK) h->last = LastSolve{B, {}, true};
    return rc;
  }
  const Shape sh = shape_of(h);
  StageLayout L{};
  int rc = stage_solve(h, sh, (size_t)B, L);
  if (rc) return rc;
  LastSolve rec;
  // a controller's tick moves a few hundred bytes in seven pieces: through one pinned mirror of the staging area, carved like it, that is two
  // transfers, [x0 | p] up and [x ... status] down (each hipMemcpy of pageable memory is ~10-15 us of driver work whatever its size)
  const bool small = L.total <= OH_PINNED_STAGE_BYTES && (h->h_stage || h->h_stage.reserve(OH_PINNED_STAGE_BYTES) == hipSuccess);
  StageLayout M = L;  // (small: the image of the staging area in the mirror)
  if (small) {
    Carver mirror(h->h_stage.p, Carver::Slots);
    layout_stage(mirror, M, sh, (size_t)B);
    memcpy(M.x0, x0, L.b_x);
    memcpy(M.p, p, L.b_p);
    HIPCHK(hipMemcpy(L.x0, M.x0, L.in_bytes(), hipMemcpyHostToDevice));
  } else {
    HIPCHK(hipMemcpy(L.x0, x0, L.b_x, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(L.p, p, L.b_p, hipMemcpyHostToDevice));
  }
  rc = solve_device(h, B, L.x0, L.p, L.x, L.f, L.kkt, L.iters, L.status, !h->is_peer, &rec);
  if (rc) return rc;
  if (small) {
    HIPCHK(hipMemcpy(M.x, L.x, L.out_bytes(), hipMemcpyDeviceToHost));
    if (x) memcpy(x, M.x, L.b_x);
    if (f) memcpy(f, M.f, L.b_f);
    if (kkt) memcpy(kkt, M.kkt, L.b_k);
    if (iters) memcpy(iters, M.iters, L.b_i);
    if (status) memcpy(status, M.status, L.b_i);
  } else {
    if (x) HIPCHK(hipMemcpy(x, L.x, L.b_x, hipMemcpyDeviceToHost));
    if (f) HIPCHK(hipMemcpy(f, L.f, L.b_f, hipMemcpyDeviceToHost));
    if (kkt) HIPCHK(hipMemcpy(kkt, L.kkt, L.b_k, hipMemcpyDeviceToHost));
    if (iters) HIPCHK(hipMemcpy(iters, L.iters, L.b_i, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, L.status, L.b_i, hipMemcpyDeviceToHost));
  }
  h->last = rec;
  return OH_OK;
}

extern "C" int oh_pm_rollout(oh_handle* h, int B, int n_ticks, int advance, double ramp, const double* state0, const double* obs_table,
                             double* states, double* f, int* iters, int* status) {
  if (!h || !state0 || !obs_table) return fail(OH_ERR_INVALID, "oh_pm_rollout: null argument");
  if (h->desc.kind != OH_PROBLEM_POINT_MASS_MPC) return fail(OH_ERR_STATE, "oh_pm_rollout: handle is not a point-mass MPC problem");
  const int T = h->pm.T;
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
    oh_launch_pm_solve(s, h->PmP, h->PmD, x_seed, d_p, x_sol, d_f + (size_t)B * k, nullptr, d_it + (size_t)B * k, d_st + (size_t)B * k,
                       (int)optv(h, "pm_wave_max"));
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

extern "C" int oh_tq_rollout(oh_handle* h, int B, int n_ticks, int advance, double mu_warm, const double* state0, const double* goal_table, double* states,
                             double* tau0, double* f, int* iters, int* status) {
  if (!h || !state0 || !goal_table) return fail(OH_ERR_INVALID, "oh_tq_rollout: null argument");
  if (h->desc.kind != OH_PROBLEM_TORQUE_MPC) return fail(OH_ERR_STATE, "oh_tq_rollout: handle is not a torque-MPC problem");
  const int T = h->tq.T, N = h->tq.ndof;
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
    rc = tq_solve_device(h, B, x_seed, d_p, x_sol, d_f + (size_t)B * k, nullptr, d_it + (size_t)B * k, d_st + (size_t)B * k, k > 0 ? mu_warm : 0.0);
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

extern "C" int oh_get_multipliers(oh_handle* h, int B, double* lam_h) {
  if (!h || !lam_h) return fail(OH_ERR_INVALID, "oh_get_multipliers: null argument");
  const LastSolve& r = h->last;
  if ((h->desc.kind != OH_PROBLEM_FIGURE_EIGHT && h->desc.kind != OH_PROBLEM_IK && h->desc.kind != OH_PROBLEM_QP && h->desc.kind != OH_PROBLEM_TAPE &&
       h->desc.kind != OH_PROBLEM_TORQUE_MPC) ||
      B != r.B || B < 1)
    return fail(OH_ERR_STATE, "oh_get_multipliers: B does not match the last solve");
  HIPCHK(hipSetDevice(h->device));
  const size_t per = shape_of(h).mult;
  if (!per && h->desc.kind == OH_PROBLEM_FIGURE_EIGHT) return fail(OH_ERR_STATE, "oh_get_multipliers: this problem has no nonlinear equality rows");
  if (r.pipe_cache) {  // the last solve was a pipelined oh_solve: every chunk left its multipliers in the handle's cache
    HIPCHK(hipMemcpy(lam_h, h->d_pipe_mult, sizeof(double) * per * B, hipMemcpyDeviceToHost));
    return OH_OK;
  }
  size_t o = 0;
  for (const LastSolve::Part& part : r.parts) {  // (several parts: the last solve ran in parts, solve_split)
    if (const int rc = copy_multipliers(part.q, part.n, lam_h + o * per)) return rc;
    o += (size_t)part.n;
  }
  return OH_OK;
}

extern "C" int oh_set_dynamics(oh_handle* h, const oh_dynamics* dyn) {
  if (!h || !dyn) return fail(OH_ERR_INVALID, "oh_set_dynamics: null argument");
  if (dyn->n < 2 || dyn->n > OH_MAX_BODIES - 1 || dyn->ndof != dyn->n - 1)
    return fail(OH_ERR_INVALID, "oh_set_dynamics: need 2 <= n <= 9 bodies and ndof == n - 1");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(h->d_dyn.reserve(1));
  HIPCHK(hipMemcpy(h->d_dyn, dyn, sizeof(oh_dynamics), hipMemcpyHostToDevice));
  h->dyn_host = *dyn;
  h->have_dyn = true;
  drop_peers(h);
  return OH_OK;
}
// Launch, check the launch, wait: the one order of the dynamics entry points.  launch() returns false for an unsupported number of bodies.
template <class Launch>
static int run_dyn(oh_handle* h, const char* unsupported, Launch&& launch) {
  if (!launch()) return fail(OH_ERR_INVALID, unsupported);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return OH_OK;
}
// oh_rnea, oh_rnea_jac, oh_rnea_hess: the host inputs (n x ndof each) staged one behind the other in 256-byte aligned slots, the output of
// out_per_sample doubles per sample behind them; launch(d_in, d_out) runs on the staged copies, then the output is copied back.
template <size_t NIN, class Launch>
static int run_dyn_staged(oh_handle* h, const int n, const std::array<const double*, NIN>& in, double* out, const size_t out_per_sample,
                          const char* unsupported, Launch&& launch) {
  HIPCHK(hipSetDevice(h->device));
  const size_t n_in = h->dyn_host.ndof * (size_t)n, n_out = out_per_sample * (size_t)n;
  std::array<const double*, NIN> d_in;
  double* d_out;
  const int src = stage_carve(h, [&](Carver c) {
    for (size_t k = 0; k < NIN; ++k) d_in[k] = c.take<double>(n_in);
    d_out = c.take<double>(n_out);
    return c.bytes();
  });
  if (src) return src;
  for (size_t k = 0; k < NIN; ++k) HIPCHK(hipMemcpy((void*)d_in[k], in[k], sizeof(double) * n_in, hipMemcpyHostToDevice));
  if (const int rc = run_dyn(h, unsupported, [&] { return launch(d_in, d_out); })) return rc;
  HIPCHK(hipMemcpy(out, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost));
  return OH_OK;
}

extern "C" int oh_rnea_device(oh_handle* h, int n, const void* d_q, const void* d_qd, const void* d_qdd, void* d_tau) {
  if (!h) return fail(OH_ERR_INVALID, "oh_rnea: null handle");
  if (n < 1 || !d_q || !d_qd || !d_qdd || !d_tau) return fail(OH_ERR_INVALID, "oh_rnea: bad arguments");
  if (!h->have_dyn) return fail(OH_ERR_STATE, "oh_rnea: call oh_set_dynamics first");
  HIPCHK(hipSetDevice(h->device));
  return run_dyn(h, "oh_rnea: unsupported number of bodies", [&] {
    return oh_launch_rnea(h->stream, h->d_dyn, h->dyn_host.n, n, (const double*)d_q, (const double*)d_qd, (const double*)d_qdd, (double*)d_tau);
  });
}
extern "C" int oh_rnea(oh_handle* h, int n, const double* q, const double* qd, const double* qdd, double* tau) {
  if (!h) return fail(OH_ERR_INVALID, "oh_rnea: null handle");
  if (n < 1 || !q || !qd || !qdd || !tau) return fail(OH_ERR_INVALID, "oh_rnea: bad arguments");
  if (!h->have_dyn) return fail(OH_ERR_STATE, "oh_rnea: call oh_set_dynamics first");
  return run_dyn_staged<3>(h, n, {q, qd, qdd}, tau, h->dyn_host.ndof, "oh_rnea: unsupported number of bodies", [&](const auto& d, double* d_tau) {
    return oh_launch_rnea(h->stream, h->d_dyn, h->dyn_host.n, n, d[0], d[1], d[2], d_tau);
  });
}

extern "C" int oh_rnea_jac(oh_handle* h, int n, const double* q, const double* qd, const double* qdd, double* J) {
  if (!h) return fail(OH_ERR_INVALID, "oh_rnea_jac: null handle");
  if (n < 1 || !q || !qd || !qdd || !J) return fail(OH_ERR_INVALID, "oh_rnea_jac: bad arguments");
  if (!h->have_dyn) return fail(OH_ERR_STATE, "oh_rnea_jac: call oh_set_dynamics first");
  const size_t nd = h->dyn_host.ndof;
  return run_dyn_staged<3>(h, n, {q, qd, qdd}, J, 3 * nd * nd, "oh_rnea_jac: unsupported number of bodies", [&](const auto& d, double* d_J) {
    return oh_launch_rnea_jac(h->stream, h->d_dyn, h->dyn_host.n, n, d[0], d[1], d[2], d_J);
  });
}

extern "C" int oh_rnea_hess(oh_handle* h, int n, const double* q, const double* qd, const double* qdd, const double* c, double* H) {
  if (!h) return fail(OH_ERR_INVALID, "oh_rnea_hess: null handle");
  if (n < 1 || !q || !qd || !qdd || !c || !H) return fail(OH_ERR_INVALID, "oh_rnea_hess: bad arguments");
  if (!h->have_dyn) return fail(OH_ERR_STATE, "oh_rnea_hess: call oh_set_dynamics first");
  const size_t nd = h->dyn_host.ndof;
  return run_dyn_staged<4>(h, n, {q, qd, qdd, c}, H, 9 * nd * nd, "oh_rnea_hess: unsupported number of bodies", [&](const auto& d, double* d_H) {
    return oh_launch_rnea_hess(h->stream, h->d_dyn, h->dyn_host.n, n, d[0], d[1], d[2], d[3], d_H);
  });
}

static int fk_common(oh_handle* h, int n, bool soa, const void* d_q, void* d_pose, void* d_J) {
  if (!h) return fail(OH_ERR_INVALID, "oh_fk_jac: null handle");
  if (n < 1 || !d_q) return fail(OH_ERR_INVALID, "oh_fk_jac: bad arguments");
  if (!h->have_chain) return fail(OH_ERR_STATE, "oh_fk_jac: call oh_set_constants first");
  HIPCHK(hipSetDevice(h->device));
  if (!h->fk_spec && !h->fk_spec_failed && (h->sch.specialize == OH_SPECIALIZE_ALWAYS || (h->sch.specialize == OH_SPECIALIZE_AUTO && n >= h->specialize_min_units)))
    specialize_fk(h);  // on failure the generic kernel runs; oh_last_error keeps the reason
  if (h->fk_spec) HIPCHK(oh_spec_launch_fk(*h->fk_spec, h->stream, soa, n, (const double*)d_q, (double*)d_pose, (double*)d_J));
  else oh_launch_fk_jac(h->stream, soa, h->d_chain, h->chain_host.n_chain, h->chain_host.ndof, n, (const double*)d_q, (double*)d_pose, (double*)d_J);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return OH_OK;
}
extern "C" int oh_fk_jac_device(oh_handle* h, int n, const void* d_q, void* d_pose, void* d_J) {
  return fk_common(h, n, false, d_q, d_pose, d_J);
}
extern "C" int oh_fk_jac_soa_device(oh_handle* h, int n, const void* d_q, void* d_pose, void* d_J) {
  return fk_common(h, n, true, d_q, d_pose, d_J);
}
extern "C" int oh_fk_jac(oh_handle* h, int n, const double* q, double* pose, double* J) {
  if (!h) return fail(OH_ERR_INVALID, "oh_fk_jac: null handle");
  if (n < 1 || !q) return fail(OH_ERR_INVALID, "oh_fk_jac: bad arguments");
  if (!h->have_chain) return fail(OH_ERR_STATE, "oh_fk_jac: call oh_set_constants first");
  HIPCHK(hipSetDevice(h->device));
  const int ndof = h->chain_host.ndof;
  const size_t b_q = sizeof(double) * ndof * (size_t)n, b_p = sizeof(double) * 7 * (size_t)n,
               b_J = sizeof(double) * 6 * ndof * (size_t)n;
  double *d_q, *d_pose, *d_J;
  int rc = stage_carve(h, [&](Carver c) {
    d_q = c.take<double>(ndof * (size_t)n);
    d_pose = c.take<double>(7 * (size_t)n);
    d_J = c.take<double>(6 * ndof * (size_t)n);
    return c.bytes();
  });
  if (rc) return rc;
  HIPCHK(hipMemcpy(d_q, q, b_q, hipMemcpyHostToDevice));
  rc = fk_common(h, n, false, d_q, pose ? d_pose : nullptr, J ? d_J : nullptr);
  if (rc) return rc;
  if (pose) HIPCHK(hipMemcpy(pose, d_pose, b_p, hipMemcpyDeviceToHost));
  if (J) HIPCHK(hipMemcpy(J, d_J, b_J, hipMemcpyDeviceToHost));
  return OH_OK;
}

// ---- kinematics of a link in the frame of another link (k_link_kin, oh_linkkin.hip) ----------------------------------------------------------------
static int validate_frame_chain(const oh_chain& c, const char* which) {
  const std::string who = std::string("oh_set_link_frames: ") + which;
  if (c.ndof < 1 || c.ndof > OH_MAX_CHAIN || c.n_chain < 0 || c.n_chain > OH_MAX_CHAIN || c.n_chain > c.ndof) return fail(OH_ERR_INVALID, who + " chain: bad n_chain/ndof");
  for (int k = 0; k < c.n_chain; ++k) {
    if (c.jtype[k] != 0 && c.jtype[k] != 1) return fail(OH_ERR_INVALID, who + " chain: joint type not supported");
    if (c.qidx[k] < 0 || c.qidx[k] >= c.ndof) return fail(OH_ERR_INVALID, who + " chain: qidx out of range");
  }
  return OH_OK;
}

extern "C" int oh_set_link_frames(oh_handle* h, const oh_chain* link, const oh_chain* base) {
  if (!h || !link) return fail(OH_ERR_INVALID, "oh_set_link_frames: null argument");
  if (h->desc.kind != OH_PROBLEM_KINEMATICS) return fail(OH_ERR_INVALID, "oh_set_link_frames: the handle is not an OH_PROBLEM_KINEMATICS handle");
  OhLinkFrames f{};
  f.link = *link;
  if (base) {
    f.base = *base;
  } else {  // the root frame: no joints, identity tool transform
    f.base.ndof = link->ndof;
    f.base.R_tool[0] = f.base.R_tool[4] = f.base.R_tool[8] = 1.0;
    f.base.quat_tool[3] = 1.0;
  }
  int rc = validate_frame_chain(f.link, "link");
  if (!rc) rc = validate_frame_chain(f.base, "base");
  if (rc) return rc;
  if (f.link.ndof != f.base.ndof) return fail(OH_ERR_INVALID, "oh_set_link_frames: link.ndof != base.ndof");
  if (f.link.ndof != h->desc.ndof) return fail(OH_ERR_INVALID, "oh_set_link_frames: chain.ndof != desc.ndof");
  // common prefix: the same joint with the same folded constants on both chains (the kernel gives such a joint an exactly zero d rpy / d q)
  const oh_chain &a = f.link, &b = f.base;
  int ns = 0;
  while (ns < a.n_chain && ns < b.n_chain && a.qidx[ns] == b.qidx[ns] && a.jtype[ns] == b.jtype[ns] && !memcmp(a.R0[ns], b.R0[ns], sizeof a.R0[ns]) &&
         !memcmp(a.p0[ns], b.p0[ns], sizeof a.p0[ns]) && !memcmp(a.axis[ns], b.axis[ns], sizeof a.axis[ns]))
    ++ns;
  for (int k = ns; k < a.n_chain; ++k)
    for (int m = ns; m < b.n_chain; ++m)
      if (a.qidx[k] == b.qidx[m]) return fail(OH_ERR_INVALID, "oh_set_link_frames: a joint past the chains' common prefix is on both chains");
  f.n_shared = ns;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(h->d_frames.reserve(1));
  HIPCHK(hipMemcpy(h->d_frames, &f, sizeof f, hipMemcpyHostToDevice));
  h->frames_host = f;
  h->have_frames = true;
  return OH_OK;
}

// argument checks of both entry points (no device call before they pass); a3 <- axis3 / |axis3|
static int link_kin_check(const char* who, oh_handle* h, int n, const void* q, const double* axis3, const oh_link_out* out, double (&a3)[3]) {
  const std::string w(who);
  if (!h) return fail(OH_ERR_INVALID, w + ": null handle");
  if (!out) return fail(OH_ERR_INVALID, w + ": null out");
  if (n < 1 || !q) return fail(OH_ERR_INVALID, w + ": bad arguments");
  a3[0] = a3[1] = a3[2] = 0.0;
  if (out->axis) {
    if (!axis3) return fail(OH_ERR_INVALID, w + ": out->axis needs axis3");
    const double nrm = std::sqrt(axis3[0] * axis3[0] + axis3[1] * axis3[1] + axis3[2] * axis3[2]);
    if (!(nrm > 0.0) || !std::isfinite(nrm)) return fail(OH_ERR_INVALID, w + ": axis3 must be a nonzero finite vector");
    for (int i = 0; i < 3; ++i) a3[i] = axis3[i] / nrm;
  }
  if (!h->have_frames) return fail(OH_ERR_STATE, w + ": call oh_set_link_frames first");
  return OH_OK;
}

static int link_kin_launch(oh_handle* h, int n, bool soa, const double* d_q, const double (&a3)[3], const oh_link_out& d_out) {
  oh_launch_link_kin(h->stream, soa, h->d_frames, h->frames_host.link.n_chain, n, d_q, a3, d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return OH_OK;
}

extern "C" int oh_link_kin_device(oh_handle* h, int n, const void* d_q, const double* axis3, const oh_link_out* d_out_soa) {
  double a3[3];
  int rc = link_kin_check("oh_link_kin_device", h, n, d_q, axis3, d_out_soa, a3);
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->device));
  return link_kin_launch(h, n, true, (const double*)d_q, a3, *d_out_soa);
}

extern "C" int oh_link_kin(oh_handle* h, int n, const double* q, const double* axis3, const oh_link_out* out) {
  double a3[3];
  int rc = link_kin_check("oh_link_kin", h, n, q, axis3, out, a3);
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->device));
  const int ndof = h->frames_host.link.ndof;
  double* const host[7] = {out->pos, out->rot, out->quat, out->rpy, out->axis, out->Jg, out->Ja};
  const size_t comps[7] = {3, 9, 4, 3, 3, 6 * (size_t)ndof, 6 * (size_t)ndof};
  const size_t b_q = sizeof(double) * ndof * (size_t)n;
  double* d_q;
  double* dev[7] = {};
  rc = stage_carve(h, [&](Carver c) {
    d_q = c.take<double>(ndof * (size_t)n);
    for (int i = 0; i < 7; ++i)
      if (host[i]) dev[i] = c.take<double>(comps[i] * (size_t)n);
    return c.bytes();
  });
  if (rc) return rc;
  HIPCHK(hipMemcpy(d_q, q, b_q, hipMemcpyHostToDevice));
  const oh_link_out d_out{dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6]};
  rc = link_kin_launch(h, n, false, d_q, a3, d_out);
  if (rc) return rc;
  for (int i = 0; i < 7; ++i)
    if (host[i]) HIPCHK(hipMemcpy(host[i], dev[i], sizeof(double) * comps[i] * (size_t)n, hipMemcpyDeviceToHost));
  return OH_OK;
}

extern "C" int oh_set_profiling(oh_handle* h, int enable) {
  if (!h) return fail(OH_ERR_INVALID, "oh_set_profiling: null handle");
  h->profiling = enable != 0;
  return OH_OK;
}
extern "C" int oh_get_timing(oh_handle* h, double* out8) {
  if (!h || !out8) return fail(OH_ERR_INVALID, "oh_get_timing: null argument");
  for (int i = 0; i < 8; ++i) out8[i] = h->timing[i];
  out8[8] = h->timing_couple;
  out8[9] = h->rejects;
  out8[10] = h->tail_iters;
  return OH_OK;
}
extern "C" int oh_event_timer_start(oh_handle* h) {
  if (!h) return fail(OH_ERR_INVALID, "oh_event_timer_start: null handle");
  HIPCHK(hipEventRecord(h->evt0, h->stream));
  return OH_OK;
}
extern "C" int oh_event_timer_stop(oh_handle* h, double* ms) {
  if (!h || !ms) return fail(OH_ERR_INVALID, "oh_event_timer_stop: null argument");
  HIPCHK(hipEventRecord(h->evt1, h->stream));
  HIPCHK(hipEventSynchronize(h->evt1));
  float f = 0.f;
  HIPCHK(hipEventElapsedTime(&f, h->evt0, h->evt1));
  *ms = f;
  return OH_OK;
}

extern "C" void oh_destroy(oh_handle* h) {
  if (h) delete h;  // ~oh_handle
}


// ---------------------------------------------------------------------------------------------------------------------------
// Multi-GPU: one process per GPU, instances sharded by the host, no data-path collective.  The single exchange of a job is the
// broadcast of the URDF-derived constants from one rank; the library owns the RCCL communicator for it (and for the
// barrier / MAX / SUM reductions a benchmark harness needs), so a ctypes host needs no other GPU runtime.  librccl is opened on first
// use: single-GPU processes never load it.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;  // optional (oh_comm_allgather)
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;     // optional
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;  // optional
};
RcclApi g_rccl;
ncclComm_t g_comm = nullptr;
int g_comm_rank = -1, g_comm_world = 0, g_comm_device = 0;
hipStream_t g_comm_stream = nullptr;
double* g_comm_scratch = nullptr;  // device, 2 doubles

int rccl_load() {
  if (g_rccl.lib) return OH_OK;
  void* lib = nullptr;
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (lib) break;
  }
  if (!lib) return fail(OH_ERR_HIP, std::string("oh_comm: cannot open librccl: ") + dlerror());
  RcclApi a;
  a.lib = lib;
  a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
  a.CommInitRank = (decltype(a.CommInitRank))dlsym(lib, "ncclCommInitRank");
  a.CommDestroy = (decltype(a.CommDestroy))dlsym(lib, "ncclCommDestroy");
  a.Broadcast = (decltype(a.Broadcast))dlsym(lib, "ncclBroadcast");
  a.AllReduce = (decltype(a.AllReduce))dlsym(lib, "ncclAllReduce");
  a.AllGather = (decltype(a.AllGather))dlsym(lib, "ncclAllGather");
  a.GetErrorString = (decltype(a.GetErrorString))dlsym(lib, "ncclGetErrorString");
  a.CommCount = (decltype(a.CommCount))dlsym(lib, "ncclCommCount");
  a.CommUserRank = (decltype(a.CommUserRank))dlsym(lib, "ncclCommUserRank");
  if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.Broadcast || !a.AllReduce || !a.GetErrorString) {
    dlclose(lib);
    return fail(OH_ERR_HIP, "oh_comm: librccl lacks an expected symbol");
  }
  g_rccl = a;
  return OH_OK;
}
int rccl_fail(const char* what, ncclResult_t r) { return fail(OH_ERR_HIP, std::string(what) + ": " + g_rccl.GetErrorString(r)); }
#define RCCLCHK(expr)                                  \
  do {                                                 \
    ncclResult_t _r = (expr);                          \
    if (_r != ncclSuccess) return rccl_fail(#expr, _r); \
  } while (0)
}  // namespace

extern "C" int oh_comm_unique_id(char* id) {
  if (!id) return fail(OH_ERR_INVALID, "oh_comm_unique_id: null");
  static_assert(OH_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
  if (const int rc = rccl_load()) return rc;
  ncclUniqueId u;
  RCCLCHK(g_rccl.GetUniqueId(&u));
  memcpy(id, u.internal, OH_COMM_ID_BYTES);
  return OH_OK;
}

extern "C" int oh_comm_init(int rank, int world, const char* id) {
  if (!id || world < 1 || rank < 0 || rank >= world) return fail(OH_ERR_INVALID, "oh_comm_init: bad rank / world / id");
  if (g_comm) return fail(OH_ERR_STATE, "oh_comm_init: this process already holds a communicator");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) return fail(OH_ERR_HIP, "oh_comm_init: no HIP device available (this library has no CPU path)");
  if (const int rc = rccl_load()) return rc;
  HIPCHK(hipGetDevice(&g_comm_device));  // the device selected with oh_set_device
  ncclUniqueId u;
  memcpy(u.internal, id, OH_COMM_ID_BYTES);
  HIPCHK(hipStreamCreate(&g_comm_stream));
  // (oh_chain-sized: the broadcast of the constants lands here first and is validated before a handle adopts it)
  if (hipMalloc((void**)&g_comm_scratch, 2 * sizeof(double) + sizeof(oh_chain)) != hipSuccess) {
    hipStreamDestroy(g_comm_stream);
    g_comm_stream = nullptr;
    return fail(OH_ERR_HIP, "oh_comm_init: scratch allocation failed");
  }
  const ncclResult_t ir = g_rccl.CommInitRank(&g_comm, world, u, rank);
  if (ir != ncclSuccess) {  // a retry must not leak the stream and the scratch
    g_comm = nullptr;
    hipFree(g_comm_scratch);
    g_comm_scratch = nullptr;
    hipStreamDestroy(g_comm_stream);
    g_comm_stream = nullptr;
    return rccl_fail("ncclCommInitRank", ir);
  }
  g_comm_rank = rank;
  g_comm_world = world;
  return OH_OK;
}

extern "C" int oh_comm_destroy(void) {
  if (!g_comm) return OH_OK;
  hipSetDevice(g_comm_device);
  hipStreamSynchronize(g_comm_stream);
  g_rccl.CommDestroy(g_comm);
  g_comm = nullptr;
  hipFree(g_comm_scratch);
  g_comm_scratch = nullptr;
  hipStreamDestroy(g_comm_stream);
  g_comm_stream = nullptr;
  g_comm_rank = -1;
  g_comm_world = 0;
  return OH_OK;
}

static int comm_allreduce(double* value, ncclRedOp_t op, const char* who) {
  if (!value) return fail(OH_ERR_INVALID, std::string(who) + ": null");
  if (!g_comm) return fail(OH_ERR_STATE, std::string(who) + ": call oh_comm_init first");
  HIPCHK(hipSetDevice(g_comm_device));
  HIPCHK(hipMemcpyAsync(g_comm_scratch, value, sizeof(double), hipMemcpyHostToDevice, g_comm_stream));
  RCCLCHK(g_rccl.AllReduce(g_comm_scratch, g_comm_scratch + 1, 1, ncclFloat64, op, g_comm, g_comm_stream));
  HIPCHK(hipMemcpyAsync(value, g_comm_scratch + 1, sizeof(double), hipMemcpyDeviceToHost, g_comm_stream));
  HIPCHK(hipStreamSynchronize(g_comm_stream));
  return OH_OK;
}
extern "C" int oh_comm_allreduce_max(double* value) { return comm_allreduce(value, ncclMax, "oh_comm_allreduce_max"); }
extern "C" int oh_comm_allreduce_sum(double* value) { return comm_allreduce(value, ncclSum, "oh_comm_allreduce_sum"); }
extern "C" int oh_comm_barrier(void) {
  double one = 1.0;
  return comm_allreduce(&one, ncclSum, "oh_comm_barrier");
}

extern "C" int oh_comm_broadcast_constants(oh_handle* h, int root) {
  if (!h) return fail(OH_ERR_INVALID, "oh_comm_broadcast_constants: null handle");
  if (!g_comm) return fail(OH_ERR_STATE, "oh_comm_broadcast_constants: call oh_comm_init first");
  if (root < 0 || root >= g_comm_world) return fail(OH_ERR_INVALID, "oh_comm_broadcast_constants: bad root");
  if (!h->d_chain) return fail(OH_ERR_STATE, "oh_comm_broadcast_constants: this handle takes no kinematic constants");
  if (g_comm_rank == root && !h->have_chain) return fail(OH_ERR_STATE, "oh_comm_broadcast_constants: the root must call oh_set_constants first");
  HIPCHK(hipSetDevice(h->device));
  // one ncclBroadcast of the oh_chain block (2952 B) on the handle's stream: out of the root's constants buffer, into a scratch block on the
  // other ranks -- a chain this handle rejects (wrong ndof, unsupported joint) must not have replaced its constants already
  unsigned char* const land = (unsigned char*)(g_comm_scratch + 2);
  RCCLCHK(g_rccl.Broadcast(h->d_chain, g_comm_rank == root ? (void*)h->d_chain : (void*)land, sizeof(oh_chain), ncclUint8, root, g_comm, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (g_comm_rank != root) {
    oh_chain tmp;
    HIPCHK(hipMemcpy(&tmp, land, sizeof(oh_chain), hipMemcpyDeviceToHost));
    if (const int rc = validate_chain(h, tmp)) return rc;
    HIPCHK(hipMemcpy(h->d_chain, land, sizeof(oh_chain), hipMemcpyDeviceToDevice));
    adopt_chain(h, tmp);
  }
  return OH_OK;
}

// The optional gather of SURVEY 8(e): every rank contributes `bytes` bytes of a device buffer (objectives, statuses, or whole solutions of its shard) and
// receives all ranks' blocks in rank order -- one ncclAllGather over xGMI on the communicator's stream, after the solves; never part of the data path.
extern "C" int oh_comm_allgather(const void* d_send, void* d_recv, size_t bytes) {
  if (!d_send || !d_recv || bytes == 0) return fail(OH_ERR_INVALID, "oh_comm_allgather: null buffer or zero size");
  if (!g_comm) return fail(OH_ERR_STATE, "oh_comm_allgather: call oh_comm_init first");
  if (!g_rccl.AllGather) return fail(OH_ERR_HIP, "oh_comm_allgather: librccl lacks ncclAllGather");
  HIPCHK(hipSetDevice(g_comm_device));
  RCCLCHK(g_rccl.AllGather(d_send, d_recv, bytes, ncclUint8, g_comm, g_comm_stream));
  HIPCHK(hipStreamSynchronize(g_comm_stream));
  return OH_OK;
}

// world size and rank as RCCL sees them (a harness prints them to prove the communicator spans the job)
extern "C" int oh_comm_info(int* rank, int* world) {
  if (!g_comm) return fail(OH_ERR_STATE, "oh_comm_info: call oh_comm_init first");
  int r = -1, w = 0;
  if (g_rccl.CommUserRank) RCCLCHK(g_rccl.CommUserRank(g_comm, &r)); else r = g_comm_rank;
  if (g_rccl.CommCount) RCCLCHK(g_rccl.CommCount(g_comm, &w)); else w = g_comm_world;
  if (rank) *rank = r;
  if (world) *world = w;
  return OH_OK;
}

extern "C" int oh_get_constants(oh_handle* h, oh_chain* out) {
  if (!h || !out) return fail(OH_ERR_INVALID, "oh_get_constants: null argument");
  if (!h->have_chain) return fail(OH_ERR_STATE, "oh_get_constants: no constants set");
  *out = h->chain_host;
  return OH_OK;
}

static bool spec_applies(const oh_handle* h) {
  return h->desc.kind == OH_PROBLEM_FIGURE_EIGHT && h->have_chain && h->desc.lock_orientation && !h->have_guards && !h->chain_host.has_lead;
}
// handles with joint / joint-velocity limits only: their persistent kernel (k_tail_vel) comes out of the same module; the batched guarded
// kernels stay generic
static bool spec_tail_vel_applies(const oh_handle* h) {
  return h->desc.kind == OH_PROBLEM_FIGURE_EIGHT && h->have_chain && h->desc.lock_orientation && h->have_guards && !h->chain_host.has_lead &&
         (h->guards.limits || h->guards.vel_limits) && h->guards.n_links == 0 && h->sch.tail_vel;
}
static int specialize_fk(oh_handle* h) {
  if (h->fk_spec) return OH_OK;
  std::string err;
  const FkSpec* sp = nullptr;
  if (oh_jit_fkjac(h->chain_host, &sp, &err)) {
    h->fk_spec_failed = true;
    return fail(OH_ERR_HIP, "oh_specialize: " + err);
  }
  h->fk_spec = sp;
  return OH_OK;
}
extern "C" int oh_specialize(oh_handle* h) {
  if (!h) return fail(OH_ERR_INVALID, "oh_specialize: null handle");
  if (!h->have_chain) return fail(OH_ERR_STATE, "oh_specialize: call oh_set_constants first");
  HIPCHK(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  int rc = specialize_fk(h);  // K1: every handle with constants
  if (rc == OH_OK && (spec_applies(h) || spec_tail_vel_applies(h)) && !h->spec) {
    std::string err;
    const FigSpec* sp = nullptr;
    if (oh_jit_figure8(h->chain_host, h->desc.ndof, &sp, &err)) {
      h->spec_failed = true;
      rc = fail(OH_ERR_HIP, "oh_specialize: " + err);
    } else h->spec = sp;
  }
  h->spec_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}
extern "C" int oh_specialize_compile(const oh_chain* chain, double* info2) {
  if (!chain) return fail(OH_ERR_INVALID, "oh_specialize_compile: null chain");
  if (chain->ndof < 4 || chain->ndof > OH_MAX_CHAIN || chain->n_chain != chain->ndof || chain->has_lead)
    return fail(OH_ERR_INVALID, "oh_specialize_compile: the chain must cover every model joint in order (4..16 joints, no lead joint)");
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<char> code;
  bool from_disk = false;
  std::string err;
  bool fd2 = false;
  if (oh_jit_compile_cached(oh_jit_figure8_source(*chain, chain->ndof), &code, &from_disk, &err) || oh_jit_compile_cached(oh_jit_fkjac_source(*chain), &code, &fd2, &err))
    return fail(OH_ERR_HIP, "oh_specialize_compile: " + err);
  from_disk = from_disk && fd2;
  if (info2) {
    info2[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    info2[1] = from_disk ? 1.0 : 0.0;
  }
  return OH_OK;
}
extern "C" int oh_specialize_info(oh_handle* h, double* info4) {
  if (!h || !info4) return fail(OH_ERR_INVALID, "oh_specialize_info: null argument");
  info4[0] = h->spec ? 1.0 : 0.0;
  info4[1] = h->fk_spec ? 1.0 : 0.0;
  info4[2] = h->spec_seconds;
  info4[3] = ((h->spec && h->spec->from_disk) || (!h->spec && h->fk_spec && h->fk_spec->from_disk)) ? 1.0 : 0.0;
  return OH_OK;
}
// How the handle's last solve was (or its next one will be) scheduled, by name: "fuse_couple" (1: coupling folded into evaluation and sweep, no
// k_couple launch), "tail_threshold", "specialized"; tape handles: "tape_wave" (0: thread per instance, 1 / 2: wavefront per instance with the (s, y)
// pairs in global memory / in LDS), "tape_levels", "tape_passes" (dependency levels and 64-instruction passes of one evaluation), "tape_jit_lds" (1: the last
// oh_tape_phi ran the generated code's entry with the work set in LDS); QP handles: "qp_block" (1: the last solve ran the workgroup-per-instance kernel);
// position-tracking handles: "free_sweep" (the FreeSweep the last solve started with, -1 before the first), "free_sweeps_used" (bit mask over its launches).
extern "C" int oh_get_flag(oh_handle* h, const char* name, int* value) {
  if (!h || !name || !value) return fail(OH_ERR_INVALID, "oh_get_flag: null argument");
  const std::string n(name);
  if (n == "fuse_couple") {
    fill_params(h);
    *value = h->P.zc;
  } else if (n == "tail_threshold") *value = h->sch.tail_threshold;
  else if (n == "specialized") *value = h->spec ? 1 : 0;
  else if (n == "tape_wave") *value = h->tape_wave.ready ? (h->tape_wave.hist_lds ? 2 : 1) : 0;
  else if (n == "tape_regs_lds") *value = h->tape_wave.ready && h->tape_wave.reg_lds ? 1 : 0;
  else if (n == "tape_jit_lds") *value = h->tape_phi_lds;
  else if (n == "tape_metric") *value = (h->TP.h0 && h->TP.lbfgs > 0) ? 1 : 0;
  else if (n == "tape_levels") *value = h->tape_wave.n_levels;
  else if (n == "tape_passes") *value = h->tape_wave.n_fw_pass + h->tape_wave.n_rv_pass;
  else if (n == "qp_block") *value = h->qp_last_block;
  else if (n == "free_sweep") *value = h->free_sweep_last;
  else if (n == "free_sweeps_used") *value = h->free_sweeps_used;
  else return fail(OH_ERR_INVALID, "oh_get_flag: unknown flag " + n);
  return OH_OK;
}

extern "C" int oh_kernel_info(const char* kernel, int* out5);
extern "C" int oh_kernel_info_handle(oh_handle* h, const char* kernel, int* out5) {
  if (!h || !kernel || !out5) return fail(OH_ERR_INVALID, "oh_kernel_info_handle: null argument");
  OhKernelInfo k{};
  if ((h->spec && oh_spec_kernel_info(*h->spec, kernel, &k)) || (h->fk_spec && !strcmp(kernel, "k_fk_jac") && oh_spec_fk_kernel_info(*h->fk_spec, &k))) {
    out5[0] = k.vgprs; out5[1] = k.scratch_bytes; out5[2] = k.lds_bytes; out5[3] = k.block; out5[4] = k.blocks_per_cu;
    return OH_OK;
  }
  return oh_kernel_info(kernel, out5);
}

extern "C" int oh_kernel_info(const char* kernel, int* out5) {
  if (!kernel || !out5) return fail(OH_ERR_INVALID, "oh_kernel_info: null argument");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) return fail(OH_ERR_HIP, "oh_kernel_info: no HIP device available (this library has no CPU path)");
  OhKernelInfo k{};
  if (!oh_kernel_info_figure8(kernel, &k) && !oh_kernel_info_fkjac(kernel, &k) && !oh_kernel_info_linkkin(kernel, &k) && !oh_kernel_info_torque(kernel, &k) &&
      !oh_kernel_info_qp_block(kernel, &k))
    return fail(OH_ERR_INVALID, std::string("oh_kernel_info: unknown kernel or attribute query failed: ") + kernel);
  out5[0] = k.vgprs; out5[1] = k.scratch_bytes; out5[2] = k.lds_bytes; out5[3] = k.block; out5[4] = k.blocks_per_cu;
  return OH_OK;
}
