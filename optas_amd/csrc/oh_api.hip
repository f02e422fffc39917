// C ABI of liboptas_hip.so (see include/optas_hip.h), host side: the handle's life cycle, the options, the chain constants, the one place that
// switches on the problem kind (shape_of, mult_ptr, solve_device), the split and pipelined solves, and the whole trajectory solve (the SQP launch
// loop: eval kernel + Riccati/step kernel per iteration).  Each self-contained family has a source of its own, oh_api_<family>.hip, and its state in
// a struct of oh_handle.h; kinematics / dynamics entry points: oh_api_kin.hip; the RCCL communicator: oh_api_comm.hip.
// Memory: every device or pinned allocation of a handle is a DevBuf member (grow-only, freed by the handle's destructor); what lives inside a pool
// or the staging area is laid out by ONE list of Carver takes (oh_carve.h) that both measures and carves it.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "oh_handle.h"

static thread_local std::string g_err;  // per host thread: a lane of fan_out reads its own message

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

extern "C" int oh_specialize(oh_handle* h);
static bool spec_applies(const oh_handle* h);
static bool spec_tail_vel_applies(const oh_handle* h);
extern "C" const char* oh_last_error(void) { return g_err.c_str(); }
extern "C" const char* oh_version(void) { return "optas_hip 0.2 (gfx950)"; }
extern "C" int oh_abi_version(void) { return OH_ABI_VERSION; }

// ---- per-handle options (OPT_TABLE, optv: oh_handle.h) -----------------------------------------------------------------------------------
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
    {"compact_fused", &Sched::compact_fused},
    {"tail_vel", &Sched::tail_vel}, {"lg_split", &Sched::lg_split}, {"tail_vel_threshold", &Sched::tail_vel_threshold},
    {"fuse_couple", &Sched::fuse_couple, nullptr, true}, {"sparse_check_below", &Sched::sparse_check_below}, {"specialize", &Sched::specialize},
    {"tq_check", &Sched::tq_check},
};
static const FieldOpt* field_opt(const std::string& name) {
  for (const FieldOpt& f : FIELD_OPTS)
    if (name == f.name) return &f;
  return nullptr;
}
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
    if (name == "tape_newton_cg" && !(v >= 0.0)) return fail(OH_ERR_INVALID, "oh_set_option: tape_newton_cg must be a count of CG iterations (0: by size)");
    h->opt[name] = v;
    if (h->desc.kind == OH_PROBLEM_TAPE && !h->tape.h_op.empty() && name.rfind("tape_", 0) == 0 && name != "tape_lds_max" && name != "tape_hvp_work_mb" && name != "tape_hvp_wave") return tape_configure(h);
  }
  return OH_OK;
}
extern "C" int oh_set_option(oh_handle* h, const char* name, double value) {
  if (!h || !name) return fail(OH_ERR_INVALID, "oh_set_option: null argument");
  // (here, not in set_option_impl: OH_DEBUG_OPTIONS is applied to a handle before its kind is known, and to handles of every kind)
  if ((std::string(name) == "tape_newton" || std::string(name) == "tape_newton_wave") && value != 0.0 && h->desc.kind != OH_PROBLEM_TAPE)
    return fail(OH_ERR_INVALID, std::string("oh_set_option: ") + name + " is an option of OH_PROBLEM_TAPE handles");
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
oh_handle* open_handle(const std::string& who, const int kind, const int T, const int ndof, const int want, int* rc) {
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
  if ((want & OPEN_FLAG) && ok) ok = h->h_flag.reserve(16) == hipSuccess;  // (the look of the lean sequence brings the list counters along)
  if (!ok) {
    delete h;
    *rc = fail(OH_ERR_HIP, who + (want ? ": stream/event/allocation failed" : ": stream/event creation failed"));
    return nullptr;
  }
  return h;
}

// every solve reports counters of its own only (oh_get_timing)
void reset_counters(oh_handle* h) {
  for (double& t : h->timing) t = 0.0;
  h->timing_couple = h->rejects = h->tail_iters = h->rescued = h->grad_moved = h->lanes_moved = 0.0;
}
// the tail every solve shares: wait for the launches since ev0, report a launch error, time the solve ([4]) and count its launches ([5])
int finish_solve(oh_handle* h, const double launched) {
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

// Shape (oh_carve.h) of a handle's problem
Shape shape_of(const oh_handle* h) {
  const size_t N = h->desc.ndof, T = h->desc.T;
  const TapeParams& tp = h->tape.P;
  const oh_qp_desc& qp = h->qp.desc;
  switch (h->desc.kind) {
    case OH_PROBLEM_TORQUE_MPC: return {4 * N * T, 2 * N + 3 * T, T * (h->tq.desc.vel_limits ? 4 : 2) * N};
    case OH_PROBLEM_TAPE: return {(size_t)tp.nx, (size_t)(tp.np > 0 ? tp.np : 1), (size_t)(tp.n_ineq + tp.n_eq)};
    case OH_PROBLEM_QP: return {(size_t)qp.n, h->qp.use_tape ? (size_t)(tp.np > 0 ? tp.np : 1) : qp_np(qp), (size_t)(qp.m + qp.me)};
    case OH_PROBLEM_POINT_MASS_MPC: return {4 * T, 4 + 4 * T, 0};
    case OH_PROBLEM_IK: return {N, N + ik_rows(h->ik), ik_rows(h->ik) + 2 * N};
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

int validate_chain(const oh_handle* h, const oh_chain& c) {
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
void drop_peers(oh_handle* h) {
  h->last = LastSolve{};
  if (h->is_peer) return;
  for (oh_handle* p : h->peers) delete p;
  h->peers.clear();
}

// the handle has new constants: everything compiled for, or remembered about, the previous chain goes (one place for the three entry
// points that set constants)
void adopt_chain(oh_handle* h, const oh_chain& c) {
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

bool solver_chain_ok(const oh_chain& c) {
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
    if (tqk) rc = oh_create_torque(&h->tq.desc, &p);
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
static int solve_device(oh_handle* h, const Solve& a, bool may_fan_out, LastSolve* rec);
// counters of the solves one lane ran, merged into the handle's timing by fan_out
struct Tally {
  double launched = 0, work = 0, compactions = 0, rejects = 0, tails = 0, rescued = 0, grad_moved = 0, lanes_moved = 0;
};
// one solve of a lane: never fans out again (the lanes ARE the streams)
static int lane_solve(oh_handle* q, Tally& t, const Solve& a) {
  if (const int rc = solve_device(q, a, false, nullptr)) return rc;
  t.launched = std::max(t.launched, q->timing[5]);
  t.work += q->timing[6];
  t.compactions += q->timing[7];
  t.rejects += q->rejects;
  t.tails += q->tail_iters;
  t.rescued += q->rescued; t.grad_moved += q->grad_moved; t.lanes_moved += q->lanes_moved;
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
    h->rescued += t.rescued; h->grad_moved += t.grad_moved; h->lanes_moved += t.lanes_moved;
  }
  return OH_OK;
}
// a batch in S contiguous parts, one per lane (parts start on multiples of 64: whole wavefronts of the thread-per-instance kernels)
static int solve_split(oh_handle* h, const int S, const Solve& a, LastSolve* rec) {
  const Shape sh = shape_of(h);
  std::vector<int> lo(S + 1, 0);
  for (int i = 1; i <= S; ++i) lo[i] = (int)((long long)a.B * i / S / 64 * 64);
  lo[S] = a.B;
  std::vector<LastSolve::Part> parts(S);
  const int rc = fan_out(h, S, [&](const int i, oh_handle* q, Tally& t) {
    parts[i] = {q, lo[i + 1] - lo[i]};
    return lane_solve(q, t, a.part((size_t)lo[i], parts[i].n, sh));
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
  double lanes_moved;  // survivors of the lean carried compactions
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
// the running count the last sweep left, when the host looks (check); -1 otherwise.  lists (may be null): the same transfer also brings the lengths of
// the two deferral lists and of the rescue list -- n_running, n_new and the counter block follow each other in the pool (layout_fig)
struct ListCounts { int defer[2], rescue; };
static int look(oh_handle* h, const bool check, int* nrun, ListCounts* lists = nullptr) {
  *nrun = -1;
  if (!check) return OH_OK;
  hipStream_t s = h->stream;
  const FigBuffers& D = h->D;
  const size_t span = (size_t)((const char*)(D.n_rescue + 1) - (const char*)D.n_running);
  const bool wide = lists && (const char*)D.n_defer > (const char*)D.n_running && span <= 16 * sizeof(int);
  HIPCHK(hipMemcpyAsync(h->h_flag, D.n_running, wide ? span : sizeof(int), hipMemcpyDeviceToHost, s));
  if (lists && !wide) HIPCHK(hipMemcpyAsync(h->h_flag.p + 1, D.n_defer, 3 * sizeof(int), hipMemcpyDeviceToHost, s));  // (n_defer[2] and n_rescue are adjacent)
  HIPCHK(hipStreamSynchronize(s));
  *nrun = *h->h_flag;
  if (lists) {
    const int* c = wide ? h->h_flag.p + (D.n_defer - D.n_running) : h->h_flag.p + 1;
    *lists = ListCounts{{c[0], c[1]}, c[2]};
  }
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
static int traj_prologue(oh_handle* h, Traj& r, const double* x0) {
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
  HIPCHK(hipMemsetAsync(h->D.work, 0, 7 * sizeof(unsigned long long), s));  // (work[0..2], the two deferral counters, the rescue list's and its two sums)
  if (!oh_launch_setup(s, r.N, h->P, h->D, x0, r.p)) return fail(OH_ERR_INVALID, "oh_solve_device: unsupported ndof");
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
  // lean (compact_fused = 2; plain handles on the kernels compiled for the chain, hybrid or exact curvature): the moving retraction leaves the accepted
  // knot behind and moves the gradient where it will be read (eval_unit<.., MOVE>), k_sweep_lists fetches the knots of the few instances that fall back to
  // them, and the list-driven copies behind a sweep are launched after the look, only when their list is not empty
  const bool lean = carry && r.spec && r.spec->retract_move && h->sch.compact_fused >= 2 && P.zc && P.hessian != OH_HESSIAN_GAUSS_NEWTON && !r.invariant;
  D.lean = 0;
  if (lean) HIPCHK(h->h_flag.reserve(16));  // (room for the wide look)
  int rescue_slot = -1;  // >= 0: the slot of a lean compaction whose q[1 - slot] / q_spare[1] swap waits for the sweep (and the rescue) of its iteration
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
        D.lean = lean ? (optv(h, "lean_count") != 0.0 ? 3 : 1) : 0;  // (from here on: the scan writes the inverse map, the sweep's head fills the rescue list)
        oh_launch_scan_running(s, D, h->sch.compact_sort);
        scanned = true;
        if (const int rc = mark(h, r, 0)) return rc;
        moved = oh_spec_launch_eval(*r.spec, s, P, D, slot, 3) == hipSuccess;
        if (moved) {
          if (const int rc = mark(h, r, 4)) return rc;
          oh_launch_carry(s, N, P, D, 2, 0, slot);
          if (lean) {
            rescue_slot = slot;
            r.lanes_moved += carry_pending;
          }
        } else {
          (void)hipGetLastError();
          h->spec_move_failed = true;
          D.lean = 0;
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
      if (rescue_slot < 0) std::swap(D.q[1 - slot], D.q_spare[1]);  // (lean: after the sweep -- the accepted knots are still in the old layout)
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
    else oh_launch_step(s, N, P, D, slot, !lean);
    if (const int rc = mark(h, r, 2)) return rc;
    ++r.launched;
    ListCounts lists{{0, 0}, 0};
    if (const int rc = look(h, check, &nrun, lean ? &lists : nullptr)) return rc;
    if (lean) {
      // without a look: unconditionally, as the sweep's launcher does.  The consumer of one deferral list zeroes the other's counter: skipped only when both
      // are zero (and the rescue list is empty: the next scan zeroes that counter)
      const bool rescue = rescue_slot >= 0;
      if (!check || lists.defer[0] || lists.defer[1] || (rescue && lists.rescue))
        oh_launch_sweep_lists(s, N, P, D, slot, rescue, check ? std::max(lists.defer[slot], rescue ? lists.rescue : 0) : -1);
      if (rescue) {
        std::swap(D.q[1 - rescue_slot], D.q_spare[1]);  // free knots: the rescued instances'; pinned knots: k_carry_gather<REST>'s
        rescue_slot = -1;
      }
    }
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
  unsigned long long work[7] = {0, 0, 0, 0, 0, 0, 0};
  // (on the handle's own stream: a hipMemcpy is an operation of the legacy null stream and waits for the kernels of every other handle's stream -- the other
  //  part of a split solve, the other lane of a pipelined one)
  HIPCHK(hipMemcpyAsync(work, h->D.work, sizeof(work), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  h->timing[6] = (double)work[0];
  h->rejects = (double)work[1];
  h->tail_iters = (double)work[2];
  h->rescued = (double)work[5]; h->grad_moved = (double)work[6]; h->lanes_moved = r.lanes_moved;
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
static int traj_solve_device(oh_handle* h, const Solve& a) {
  Traj r{};
  r.B = a.B; r.N = h->desc.ndof;
  r.guarded = h->have_guards; r.lead = h->chain_host.has_lead != 0; r.prof = h->profiling; r.invariant = batch_invariant(h) != 0.0;
  r.p = a.p; r.x = a.x; r.f = a.f; r.kkt = a.kkt; r.iters = a.iters; r.status = a.status;
  if (const int rc = traj_prologue(h, r, a.x0)) return rc;
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
static int solve_device(oh_handle* h, const Solve& a, const bool may_fan_out, LastSolve* rec) {
  const int B = a.B;
  if (B < 1) return fail(OH_ERR_INVALID, "oh_solve_device: B must be >= 1");
  if (!a.x0 || !a.p) return fail(OH_ERR_INVALID, "oh_solve_device: x0 and p are required");
  if (rec) *rec = LastSolve{B, {{h, B}}, false};
  switch (h->desc.kind) {
    case OH_PROBLEM_POINT_MASS_MPC: return pm_solve_device(h, a);
    case OH_PROBLEM_IK: return ik_solve_device(h, a);
    case OH_PROBLEM_QP: return qp_solve_device(h, a);
    case OH_PROBLEM_TAPE: return tape_solve_device(h, a);
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
    return solve_split(h, S, a, rec);
  }
  return h->desc.kind == OH_PROBLEM_TORQUE_MPC ? tq_solve_device(h, a) : traj_solve_device(h, a);
}

extern "C" int oh_solve_device(oh_handle* h, int B, const void* d_x0, const void* d_p, void* d_x, void* d_f, void* d_kkt,
                               void* d_iters, void* d_status) {
  if (!h) return fail(OH_ERR_INVALID, "oh_solve_device: null handle");
  h->last = LastSolve{};
  LastSolve rec;
  const Solve a{B, (const double*)d_x0, (const double*)d_p, (double*)d_x, (double*)d_f, (double*)d_kkt, (int*)d_iters, (int*)d_status};
  const int rc = solve_device(h, a, !h->is_peer, &rec);
  if (rc == OH_OK) h->last = rec;
  return rc;
}

int ensure_stage(oh_handle* h, size_t bytes) {
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
    case OH_PROBLEM_TORQUE_MPC: return q->tq.mult;
    case OH_PROBLEM_TAPE: return q->tape.mult;
    case OH_PROBLEM_QP: return q->qp.mult;
    case OH_PROBLEM_IK: return q->ik.mult;
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
      if (const int rc = lane_solve(q, t, Solve{n, L.x0, L.p, L.x, L.f, L.kkt, L.iters, L.status})) return rc;
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
  if (!shape_of(h).nx) return fail(OH_ERR_STATE, "oh_solve: handle was created without a problem (OH_PROBLEM_KINEMATICS)");
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
  rc = solve_device(h, Solve{B, L.x0, L.p, L.x, L.f, L.kkt, L.iters, L.status}, !h->is_peer, &rec);
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

extern "C" int oh_get_multipliers(oh_handle* h, int B, double* lam_h) {
  if (!h || !lam_h) return fail(OH_ERR_INVALID, "oh_get_multipliers: null argument");
  const LastSolve& r = h->last;
  // (a handle without a problem never has a last solve; the point-mass family reports no multipliers)
  if (h->desc.kind == OH_PROBLEM_POINT_MASS_MPC || B != r.B || B < 1) return fail(OH_ERR_STATE, "oh_get_multipliers: B does not match the last solve");
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

extern "C" int oh_set_profiling(oh_handle* h, int enable) {
  if (!h) return fail(OH_ERR_INVALID, "oh_set_profiling: null handle");
  h->profiling = enable != 0;
  return OH_OK;
}
extern "C" int oh_get_timing(oh_handle* h, double* out8) {  // (14 entries, see optas_hip.h)
  if (!h || !out8) return fail(OH_ERR_INVALID, "oh_get_timing: null argument");
  for (int i = 0; i < 8; ++i) out8[i] = h->timing[i];
  out8[8] = h->timing_couple;
  out8[9] = h->rejects;
  out8[10] = h->tail_iters;
  out8[11] = h->rescued;
  out8[12] = h->grad_moved;
  out8[13] = h->lanes_moved;
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
// oh_tape_phi ran the generated code's entry with the work set in LDS), "tape_hvp_launches" (launches of the last oh_tape_hvp),
// "tape_hvp_path" (what the last oh_tape_hvp ran: 0 interpreter lanes, 1 / 2 k_tape_wave_hvp with its registers in LDS / in global memory); QP handles: "qp_block" (1: the last solve ran the workgroup-per-instance kernel);
// IK handles: "ik_orientation" (1: full-pose goal), "ik_goal" (0 position, 1 full pose, 2 position and link axis);
// position-tracking handles: "free_sweep" (the FreeSweep the last solve started with, -1 before the first), "free_sweeps_used" (bit mask over its launches).
extern "C" int oh_get_flag(oh_handle* h, const char* name, int* value) {
  if (!h || !name || !value) return fail(OH_ERR_INVALID, "oh_get_flag: null argument");
  const std::string n(name);
  if (n == "fuse_couple") {
    fill_params(h);
    *value = h->P.zc;
  } else if (n == "tail_threshold") *value = h->sch.tail_threshold;
  else if (n == "specialized") *value = h->spec ? 1 : 0;
  else if (n == "tape_wave") *value = h->tape.wave.ready ? (h->tape.wave.hist_lds ? 2 : 1) : 0;
  else if (n == "tape_regs_lds") *value = h->tape.wave.ready && h->tape.wave.reg_lds ? 1 : 0;
  else if (n == "tape_jit_lds") *value = h->tape.phi_lds;
  else if (n == "tape_hvp_launches") *value = h->tape.hvp_launches;
  else if (n == "tape_hvp_path") *value = h->tape.hvp_path;
  else if (n == "tape_newton") *value = h->tape.last_newton;
  else if (n == "tape_newton_path") *value = h->tape.newton_path;
  else if (n == "tape_metric") *value = (h->tape.P.h0 && h->tape.P.lbfgs > 0) ? 1 : 0;
  else if (n == "tape_levels") *value = h->tape.wave.n_levels;
  else if (n == "tape_passes") *value = h->tape.wave.n_fw_pass + h->tape.wave.n_rv_pass;
  else if (n == "qp_block") *value = h->qp.last_block;
  else if (n == "ik_orientation") *value = (h->desc.kind == OH_PROBLEM_IK && h->ik.desc.orientation) ? 1 : 0;
  else if (n == "ik_goal") *value = h->desc.kind != OH_PROBLEM_IK ? 0 : (int)ik_goal(h->ik);
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
      !oh_kernel_info_qp_block(kernel, &k) && !oh_kernel_info_tape_wave(kernel, &k) && !oh_kernel_info_ik(kernel, &k))
    return fail(OH_ERR_INVALID, std::string("oh_kernel_info: unknown kernel or attribute query failed: ") + kernel);
  out5[0] = k.vgprs; out5[1] = k.scratch_bytes; out5[2] = k.lds_bytes; out5[3] = k.block; out5[4] = k.blocks_per_cu;
  return OH_OK;
}
