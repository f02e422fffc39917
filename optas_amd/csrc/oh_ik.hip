// Inverse-kinematics family (BASELINE config 1, example/example.py:13-60):
//
//     min_q  w ||q - q_nominal||^2   s.t.  h(q) = goal - value(q) = 0        (builder.py:354: rhs - lhs)
//                                          lo <= q <= up                     (enforce_model_limits, builder.py:471-509)
//
// One thread owns one instance for its whole solve (nx = ndof <= 8: everything lives in registers): bound-constrained
// augmented Lagrangian, inner iteration = projected Newton (Bertsekas active set) with the exact Hessian of the
// augmented Lagrangian -- 2wI + rho J^T J - sum_k y_k d2 value_k -- a Levenberg shift when the masked matrix is not
// positive definite, and Armijo backtracking along the projected arc.  The iteration is written once, oh_ik_iteration.h;
// what the equality rows are is a policy: IkPositionRows (value = p_link, 3 rows), IkPoseRows (p_link and the link
// quaternion, 7 rows), IkAxisRows (p_link and one axis of the link frame, 6 rows).  oracle/ik_al.py:solve_rows_al
// restates the iteration in numpy (test infrastructure only), with one rows object per goal shape as well.
#include <hip/hip_runtime.h>

#include "oh_device.h"
#include "oh_kernels.h"

namespace {

// Linear columns of the chain for the point e: Jp_k = om_k x (e - pj_k) for a revolute joint; a prismatic joint moves e along its axis and
// turns nothing, so its axis becomes the column and om_k = 0 from here on.
template <int N>
OH_DEV void ik_linear_columns(const oh_chain* __restrict__ ch, const double* e, const double (&pj)[N][3], double (&Jp)[N][3], double (&om)[N][3]) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (ch->jtype[k] == 0) {
      const double d[3] = {e[0] - pj[k][0], e[1] - pj[k][1], e[2] - pj[k][2]};
      cross3(om[k], d, Jp[k]);
    } else {
      Jp[k][0] = om[k][0]; Jp[k][1] = om[k][1]; Jp[k][2] = om[k][2];
      om[k][0] = om[k][1] = om[k][2] = 0.0;
    }
  }
}

// ---- the rows policies ------------------------------------------------------------------------------------------------------------------------------
//
// A policy states, for h = goal - value(q) with NH rows, y the effective multipliers:
//     NH                                  number of rows; p rows are [q_nominal (N); goal (NH)], multiplier rows [-lam (NH); z_lo (N); z_up (N)]
//     idle_pass_counts                    see IkAxisRows
//     eval(ch, P, q, v, Jp, om)           value v[NH] and the chain's linear columns Jp / joint axes om (om = 0 for a prismatic joint)
//     Dual, dual(y, v, rho, D)            whatever of y the next two need, formed once per multiplier vector
//     grad(i, base, Jp, om, y, D)         base - (J^T y)_i, J the Jacobian of the value and base = 2 w (q_i - qn_i): entry i of the gradient of f + y . h
//     hess(a, c, Jp, om, v, y, rho, D)    rho (J^T J)_{ac} - sum_k y_k d2 value_k / dq_a dq_c for c not after a on the chain
// The device build contracts multiply-adds, so how a policy groups its sums is part of its results: grad takes the base term because the pose rows
// subtract their two shares one after the other, where the axis rows subtract one sum.

// Position goal: value = p_link.  The curvature is y . (om_c x Jp_a).
struct IkPositionRows {
  static constexpr int NH = 3;
  static constexpr bool idle_pass_counts = false;
  struct Dual {};

  template <int N>
  static OH_DEV void eval(const oh_chain* __restrict__ ch, const IkParams&, const double (&q)[N], double (&v)[NH], double (&Jp)[N][3], double (&om)[N][3]) {
    double R[9], p[3], pj[N][3];
    fk_chain<N>(ch, q, R, p, om, pj);
    double t[3];
    mv3(R, ch->p_tool, t);
    v[0] = p[0] + t[0]; v[1] = p[1] + t[1]; v[2] = p[2] + t[2];
    ik_linear_columns<N>(ch, v, pj, Jp, om);
  }

  static OH_DEV void dual(const double (&)[NH], const double (&)[NH], const double, Dual&) {}

  template <int N>
  static OH_DEV double grad(const int i, const double base, const double (&Jp)[N][3], const double (&)[N][3], const double (&y)[NH], const Dual&) {
    return base - dot3(Jp[i], y);
  }

  template <int N>
  static OH_DEV double hess(const int a, const int c, const double (&Jp)[N][3], const double (&om)[N][3], const double (&)[NH], const double (&y)[NH],
                            const double rho, const Dual&) {
    double t[3];
    cross3(om[c], Jp[a], t);
    return rho * dot3(Jp[a], Jp[c]) - dot3(y, t);
  }
};

// Full-pose goal (oh_ik_desc.orientation): value = [p_link; quat_link], the reference's second equality on get_global_link_quaternion with the literal
// sign.  quat_link is the reference's chain product (xyzw, half-angle factors, quat0[k], quat_tool: oh_fkjac_unit.h), smooth in q; its column for a
// revolute joint j is Jq_j = 1/2 (om_j, 0) (x) quat and, for a not after b on the chain, d2quat / dq_a dq_b = 1/4 (om_a, 0) (x) (om_b, 0) (x) quat.
// Neither is formed: with y = [yp; yq] the effective multipliers and D.wq = vec(yq (x) conj(quat)),
//     yq . Jq_j          = 1/2 om_j . wq
//     Jq_a . Jq_c        = 1/4 |quat|^2 om_a . om_c                               (right multiplication by quat is |quat| times a rotation of R^4)
//     yq . d2quat_{c,a}  = 1/4 ((om_c x om_a) . wq - (om_c . om_a) (yq . quat))   ((om_c,0) (x) (om_a,0) = (om_c x om_a, -om_c . om_a))
// so with D.kq = 1/4 (rho |quat|^2 + yq . quat) the quaternion rows add  kq om_a . om_c - 1/4 (om_c x om_a) . wq  to hess: one 3-vector and one scalar
// per multiplier vector on top of the position rows' registers.  A prismatic joint has om = 0.  tests/pose_ik_ref.py writes the derivatives the long way.
struct IkPoseRows {
  static constexpr int NH = 7;
  static constexpr bool idle_pass_counts = false;
  struct Dual {
    double wq[3], kq;
  };

  // the chain walk with the quaternion product beside the rotation
  template <int N>
  static OH_DEV void eval(const oh_chain* __restrict__ ch, const IkParams&, const double (&q)[N], double (&v)[NH], double (&Jp)[N][3], double (&om)[N][3]) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0}, quat[4] = {0, 0, 0, 1}, pj[N][3];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double t[3], qn[4];
      mv3(R, ch->p0[k], t);
      p[0] += t[0]; p[1] += t[1]; p[2] += t[2];
      if (!ch->r0ident[k]) {
        double Rn[9];
        mm3(R, ch->R0[k], Rn);
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
      }
      pj[k][0] = p[0]; pj[k][1] = p[1]; pj[k][2] = p[2];
      qmul(quat, ch->quat0[k], qn);
      if (ch->jtype[k] == 0) {
        double sh, chh;
        sincos_joint(0.5 * q[k], &sh, &chh);  // half angle for the quaternion, the full angle from it for Rodrigues (as fk_jac_unit)
        const double s = 2.0 * sh * chh, c = 1.0 - 2.0 * sh * sh;
        if (ch->axcode[k] != 0) rot_principal_right(R, ch->axcode[k], s, c, om[k]);
        else rot_axis_right(R, ch->axis[k], s, c, om[k]);
        const double qa[4] = {sh * ch->axis[k][0], sh * ch->axis[k][1], sh * ch->axis[k][2], chh};
        qmul(qn, qa, quat);
      } else {
        mv3(R, ch->axis[k], om[k]);
        p[0] += om[k][0] * q[k]; p[1] += om[k][1] * q[k]; p[2] += om[k][2] * q[k];
        quat[0] = qn[0]; quat[1] = qn[1]; quat[2] = qn[2]; quat[3] = qn[3];
      }
    }
    double t[3];
    mv3(R, ch->p_tool, t);
    v[0] = p[0] + t[0]; v[1] = p[1] + t[1]; v[2] = p[2] + t[2];
    qmul(quat, ch->quat_tool, &v[3]);
    ik_linear_columns<N>(ch, v, pj, Jp, om);
  }

  // wq = vec(yq (x) conj(quat)): yq . (1/2 (om, 0) (x) quat) = 1/2 om . wq
  static OH_DEV void dual(const double (&y)[NH], const double (&v)[NH], const double rho, Dual& D) {
    const double *yq = &y[3], *quat = &v[3];
    D.wq[0] = yq[0] * quat[3] - yq[1] * quat[2] + yq[2] * quat[1] - yq[3] * quat[0];
    D.wq[1] = yq[0] * quat[2] + yq[1] * quat[3] - yq[2] * quat[0] - yq[3] * quat[1];
    D.wq[2] = yq[1] * quat[0] - yq[0] * quat[1] + yq[2] * quat[3] - yq[3] * quat[2];
    D.kq = 0.25 * (rho * (v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6]) + (y[3] * v[3] + y[4] * v[4] + y[5] * v[5] + y[6] * v[6]));
  }

  template <int N>
  static OH_DEV double grad(const int i, const double base, const double (&Jp)[N][3], const double (&om)[N][3], const double (&y)[NH], const Dual& D) {
    return base - dot3(Jp[i], y) - 0.5 * dot3(om[i], D.wq);
  }

  // (h = goal - value: both curvatures enter with the minus sign)
  template <int N>
  static OH_DEV double hess(const int a, const int c, const double (&Jp)[N][3], const double (&om)[N][3], const double (&)[NH], const double (&y)[NH],
                            const double rho, const Dual& D) {
    double t[3], u[3];
    cross3(om[c], Jp[a], t);
    cross3(om[c], om[a], u);
    double e = rho * dot3(Jp[a], Jp[c]) - dot3(y, t);
    e += D.kq * dot3(om[a], om[c]) - 0.25 * dot3(u, D.wq);
    return e;
  }
};

// Axis goal (oh_ik_set_axis_goal): value = [p_link; u], u = R_link a, a the unit link-frame axis (P.a_tool = R_tool a: fk_chain's R stops before the
// tool).  With yu = y[3..5]:
//     du/dq_j = om_j x u                          yu . du/dq_j = om_j . (u x yu)
//     (om_a x u) . (om_c x u) = |u|^2 om_a . om_c - (om_a . u)(om_c . u)           (|u|^2 kept as computed, like |quat|^2 in the pose rows)
//     d2u/dq_c dq_a = om_c x (om_a x u)           yu . d2u_{c,a} = (yu . om_a)(om_c . u) - (yu . u)(om_a . om_c)         (c not after a)
// so with D.c = u x yu, D.r = rho u + yu, D.k = rho |u|^2 + yu . u the axis rows add  om_i . D.c  to J^T y and  D.k om_a . om_c - (om_c . u)(om_a . D.r)
// to hess: one 3-vector per multiplier vector and dot products, no 3 x n Jacobian.  |u| = 1, so the three rows have rank 2 (u^T du/dq = 0); no
// system in the rows is solved, and lam along u moves only at second order for a unit goal.  The goal is literal: one that is not of unit length is
// infeasible as posed and ends with a non-zero status.  tests/axis_ik_ref.py writes the derivatives the long way, with the Jacobian written out.
struct IkAxisRows {
  static constexpr int NH = 6;
  // An outer pass whose inner loop had nothing to do counts as one evaluation towards the cap: pinned at an infeasible stationary point with every free
  // joint's gradient below the inner tolerance (a goal out of reach, all joints on their bounds) such passes only grow lam, and would do so without
  // end.  The position and the pose rows leave it off: near convergence most solves make outer passes without an evaluation, so their evaluation counts
  // would change everywhere, and no goal those two are given in the tests gets there.  Nothing bounds such a solve of theirs.
  static constexpr bool idle_pass_counts = true;
  struct Dual {
    double c[3], r[3], k;
  };

  template <int N>
  static OH_DEV void eval(const oh_chain* __restrict__ ch, const IkParams& P, const double (&q)[N], double (&v)[NH], double (&Jp)[N][3], double (&om)[N][3]) {
    double R[9], p[3], pj[N][3];
    fk_chain<N>(ch, q, R, p, om, pj);
    double t[3];
    mv3(R, ch->p_tool, t);
    v[0] = p[0] + t[0]; v[1] = p[1] + t[1]; v[2] = p[2] + t[2];
    mv3(R, P.a_tool, &v[3]);
    ik_linear_columns<N>(ch, v, pj, Jp, om);
  }

  static OH_DEV void dual(const double (&y)[NH], const double (&v)[NH], const double rho, Dual& D) {
    cross3(&v[3], &y[3], D.c);
#pragma unroll
    for (int k = 0; k < 3; ++k) D.r[k] = rho * v[3 + k] + y[3 + k];
    D.k = rho * dot3(&v[3], &v[3]) + dot3(&y[3], &v[3]);
  }

  template <int N>
  static OH_DEV double grad(const int i, const double base, const double (&Jp)[N][3], const double (&om)[N][3], const double (&y)[NH], const Dual& D) {
    return base - (dot3(Jp[i], y) + dot3(om[i], D.c));
  }

  template <int N>
  static OH_DEV double hess(const int a, const int c, const double (&Jp)[N][3], const double (&om)[N][3], const double (&v)[NH], const double (&y)[NH],
                            const double rho, const Dual& D) {
    double t[3];
    cross3(om[c], Jp[a], t);
    return rho * dot3(Jp[a], Jp[c]) - dot3(y, t) + D.k * dot3(om[a], om[c]) - dot3(om[c], &v[3]) * dot3(om[a], D.r);
  }
};

// ---- the iteration ------------------------------------------------------------------------------------------------------------------------------------

template <int N, int NH>
OH_DEV double ik_rows_merit(const IkParams& P, const double (&q)[N], const double (&qn)[N], const double (&v)[NH], const double (&g)[NH],
                            const double (&lam)[NH], double rho) {
  double c = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) c += (q[i] - qn[i]) * (q[i] - qn[i]);
  double m = P.w * c;
#pragma unroll
  for (int k = 0; k < NH; ++k) {
    const double h = g[k] - v[k];
    m += lam[k] * h + 0.5 * rho * h * h;
  }
  return m;
}

// The iteration is one text, oh_ik_iteration.h, and stands in two functions.  The device build contracts multiply-adds after the optimiser has ordered
// the operands of every sum, and that order depends on whether the text is compiled as the body of the kernel or as a function inlined into it: the
// same expression trees round differently in a few places (some 1e-16 of x; evaluation counts and statuses do not move).  The position and the pose
// goal had their iterations in their kernels, the axis goal had it in ik_rows_solve; each keeps its form, and with it its bits
// (tests/test_gpu_ik_rows_bits.py).  A change that re-pins the axis goal's bits can drop ik_rows_solve and k_ik_axis_solve.
template <int N, class Rows>
__global__ void __launch_bounds__(64) k_ik_rows_solve(const oh_chain* __restrict__ ch, IkParams P, int B, const double* __restrict__ x0,
                                                      const double* __restrict__ par, double* __restrict__ x, double* __restrict__ f,
                                                      double* __restrict__ kkt, int* __restrict__ iters, int* __restrict__ status,
                                                      double* __restrict__ mult) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
#include "oh_ik_iteration.h"
}

template <int N, class Rows>
OH_DEV void ik_rows_solve(const oh_chain* __restrict__ ch, const IkParams& P, const int b, const double* __restrict__ x0, const double* __restrict__ par,
                          double* __restrict__ x, double* __restrict__ f, double* __restrict__ kkt, int* __restrict__ iters, int* __restrict__ status,
                          double* __restrict__ mult) {
#include "oh_ik_iteration.h"
}

template <int N>
__global__ void __launch_bounds__(64) k_ik_axis_solve(const oh_chain* __restrict__ ch, IkParams P, int B, const double* __restrict__ x0,
                                                      const double* __restrict__ par, double* __restrict__ x, double* __restrict__ f,
                                                      double* __restrict__ kkt, int* __restrict__ iters, int* __restrict__ status,
                                                      double* __restrict__ mult) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  ik_rows_solve<N, IkAxisRows>(ch, P, b, x0, par, x, f, kkt, iters, status, mult);
}

// ---- goal x chain length -> instantiation ---------------------------------------------------------------------------------------------------------------

using IkKernel = void (*)(const oh_chain*, IkParams, int, const double*, const double*, double*, double*, double*, int*, int*, double*);

template <int N>
IkKernel ik_kernel_of_goal(const IkGoal goal) {
  switch (goal) {
    case IkGoal::Position: return k_ik_rows_solve<N, IkPositionRows>;
    case IkGoal::Pose: return k_ik_rows_solve<N, IkPoseRows>;
    case IkGoal::Axis: return k_ik_axis_solve<N>;
  }
  return nullptr;
}

IkKernel ik_kernel(const IkGoal goal, const int N) {
  switch (N) {  // chain lengths 2 ... 8 (round 5: planar_3dof, the tester robots, 8-joint arms)
#define C(NN) case NN: return ik_kernel_of_goal<NN>(goal)
    C(2); C(3); C(4); C(5); C(6); C(7); C(8);
#undef C
  }
  return nullptr;
}

}  // namespace

// "k_ik_solve" / "k_ik_pose_solve" / "k_ik_axis_solve" (the names the three goal shapes' kernels had as separate texts; tools and profiles keep
// them): the 7-joint instantiations; with "_N" appended: N = 2 ... 8
bool oh_kernel_info_ik(const char* name, OhKernelInfo* out) {
  std::string n(name);
  int N = 7;
  if (n.size() > 2 && n[n.size() - 2] == '_' && n.back() >= '2' && n.back() <= '8') {
    N = n.back() - '0';
    n.resize(n.size() - 2);
  }
  IkGoal goal;
  if (n == "k_ik_solve") goal = IkGoal::Position;
  else if (n == "k_ik_pose_solve") goal = IkGoal::Pose;
  else if (n == "k_ik_axis_solve") goal = IkGoal::Axis;
  else return false;
  const IkKernel kernel = ik_kernel(goal, N);
  hipFuncAttributes a{};
  if (!kernel || hipFuncGetAttributes(&a, reinterpret_cast<const void*>(kernel)) != hipSuccess) return false;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 64, 0) != hipSuccess) nb = 0;
  *out = OhKernelInfo{a.numRegs, (int)a.localSizeBytes, (int)a.sharedSizeBytes, 64, nb};
  return true;
}

bool oh_launch_ik(hipStream_t stream, IkGoal goal, const oh_chain* d_chain, const IkParams& P, int B, const double* x0, const double* p, double* x,
                  double* f, double* kkt, int* iters, int* status, double* mult) {
  const IkKernel kernel = ik_kernel(goal, P.ndof);
  if (!kernel) return false;
  hipLaunchKernelGGL(kernel, dim3((B + 63) / 64), dim3(64), 0, stream, d_chain, P, B, x0, p, x, f, kkt, iters, status, mult);
  return true;
}
