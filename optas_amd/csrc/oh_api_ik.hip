// Host side of the inverse-kinematics family (OH_PROBLEM_IK): creation and the solve.  State: oh_handle::ik.
#include "oh_handle.h"

// orientation took the padding after max_iter: the descriptor is laid out as before it existed (OH_ABI_VERSION unchanged)
static_assert(sizeof(oh_ik_desc) == 48 + 2 * 8 * OH_MAX_CHAIN && offsetof(oh_ik_desc, tol) == 24 + 2 * 8 * OH_MAX_CHAIN, "oh_ik_desc layout");

static void mv3_host(const double* A, const double* v, double* o) {
  for (int i = 0; i < 3; ++i) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
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
  oh_ik_desc& d = h->ik.desc;
  d = *desc;
  d.orientation = d.orientation ? 1 : 0;
  if (d.max_iter <= 0) d.max_iter = 200;
  if (!(d.tol > 0.0)) d.tol = 1e-6;
  if (!(d.tol_feas > 0.0)) d.tol_feas = 1e-9;
  if (!(d.rho0 > 0.0)) d.rho0 = 100.0 * d.w_nominal;
  *out = h;
  return OH_OK;
}

// Position goal plus a goal for one axis of the link frame: h = [p_goal - p_link(q); u_goal - R_link(q) a], a = axis_link / |axis_link|.
extern "C" int oh_ik_set_axis_goal(oh_handle* h, const double axis_link[3]) {
  if (!h || !axis_link) return fail(OH_ERR_INVALID, "oh_ik_set_axis_goal: null argument");
  if (h->desc.kind != OH_PROBLEM_IK) return fail(OH_ERR_INVALID, "oh_ik_set_axis_goal: not an OH_PROBLEM_IK handle");
  if (h->ik.desc.orientation) return fail(OH_ERR_INVALID, "oh_ik_set_axis_goal: the handle has a full-pose goal (oh_ik_desc.orientation)");
  const double n2 = axis_link[0] * axis_link[0] + axis_link[1] * axis_link[1] + axis_link[2] * axis_link[2];
  if (!(n2 > 0.0) || !(n2 < 1e300)) return fail(OH_ERR_INVALID, "oh_ik_set_axis_goal: the axis must be finite and non-zero");
  if (h->ik.solved) return fail(OH_ERR_STATE, "oh_ik_set_axis_goal: the goal cannot change after the first solve");
  const double n = std::sqrt(n2);
  for (int i = 0; i < 3; ++i) h->ik.axis_link[i] = axis_link[i] / n;
  h->ik.axis_goal = true;
  return OH_OK;
}

int ik_solve_device(oh_handle* h, const Solve& a) {
  if (!h->have_chain) return fail(OH_ERR_STATE, "oh_solve_device: call oh_set_constants first");
  if (!solver_chain_ok(h->chain_host))
    return fail(OH_ERR_INVALID, "oh_solve_device: the solver needs a chain that covers every model joint in order");
  HIPCHK(hipSetDevice(h->device));
  const oh_ik_desc& d = h->ik.desc;
  const int N = d.ndof;
  HIPCHK(h->ik.mult.reserve((ik_rows(h->ik) + 2 * (size_t)N) * a.B));
  IkParams P{};
  P.ndof = N;
  P.max_iter = d.max_iter;
  P.w = d.w_nominal;
  P.tol = d.tol;
  P.tol_feas = d.tol_feas;
  P.rho0 = d.rho0;
  for (int i = 0; i < N; ++i) {
    P.lo[i] = d.q_lo[i];
    P.up[i] = d.q_up[i];
  }
  const IkGoal goal = ik_goal(h->ik);
  if (goal == IkGoal::Axis) mv3_host(h->chain_host.R_tool, h->ik.axis_link, P.a_tool);  // fk_chain's R stops before the tool transform
  h->ik.solved = true;
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  if (!oh_launch_ik(h->stream, goal, h->d_chain, P, a.B, a.x0, a.p, a.x, a.f, a.kkt, a.iters, a.status, h->ik.mult))
    return fail(OH_ERR_INVALID, "oh_solve_device: unsupported ndof");
  return finish_solve(h, 1);
}
