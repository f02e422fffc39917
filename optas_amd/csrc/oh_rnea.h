// Inverse dynamics on the device: RobotModel.rnea (models.py:1819-1880) on doubles or jets, the same torques by virtual work, d tau / d (q, dq, ddq)
// in closed form and the adjoint that gives second derivatives.  Users: the stand-alone kernels of oh_rnea.hip and the torque-MPC solver of
// oh_torque.hip.
#pragma once
#include <type_traits>
#include <utility>

#include "oh_device.h"

// launchers of oh_rnea.hip (called from oh_api_kin.hip); false: unsupported number of bodies
bool oh_launch_rnea(hipStream_t s, const oh_dynamics* d_dyn, int nbodies, int n, const double* q, const double* qd, const double* qdd, double* tau);
bool oh_launch_rnea_jac(hipStream_t s, const oh_dynamics* d_dyn, int nbodies, int n, const double* q, const double* qd, const double* qdd, double* J);
bool oh_launch_rnea_hess(hipStream_t s, const oh_dynamics* d_dyn, int nbodies, int n, const double* q, const double* qd, const double* qdd, const double* c, double* H);

namespace oh_dyn {

// ---- jets: a value and K tangents -------------------------------------------------------------------------------------------------------
// One lane differentiates the recursion along K seeded directions at once.  What depends on the joint angles alone -- sines, cosines, the joint
// rotations, the joint axes in their body frames -- varies only along the lane's joint angle: it is a Jet<1>, whose tangent is slot 0 of the
// wider jets of the velocities, accelerations and wrenches it meets.  Operations between the two never form the tangents that are zero by
// construction.  A product of jets puts the narrower operand first and forms each shared tangent with an fma; a sum puts the wider operand first.
template <int K>
struct Jet {
  double v, d[K];
};
template <class S>
constexpr int jet_k = 0;
template <int K>
constexpr int jet_k<Jet<K>> = K;

// a jet built from its value and a function of the tangent slot, in one aggregate initialisation (filled in member by member, the same
// arithmetic comes out of the compiler in another instruction order)
template <int K, class F, size_t... I>
OH_DEV Jet<K> jet_of(const double v, F&& f, std::index_sequence<I...>) {
  return {v, {f((int)I)...}};
}
template <int K, class F>
OH_DEV Jet<K> jet_of(const double v, F&& f) {
  return jet_of<K>(v, f, std::make_index_sequence<K>{});
}
template <int K, int M>
OH_DEV Jet<(K > M ? K : M)> operator+(const Jet<K> a, const Jet<M> b) {
  if constexpr (K < M) return b + a;
  else return jet_of<K>(a.v + b.v, [&](int k) { return k < M ? a.d[k] + b.d[k] : a.d[k]; });
}
template <int K, int M>
OH_DEV Jet<(K > M ? K : M)> operator-(const Jet<K> a, const Jet<M> b) {
  return jet_of<(K > M ? K : M)>(a.v - b.v, [&](int k) { return k < K && k < M ? a.d[k] - b.d[k] : k < K ? a.d[k] : -b.d[k]; });
}
template <int K, int M>
OH_DEV Jet<(K > M ? K : M)> operator*(const Jet<K> a, const Jet<M> b) {
  if constexpr (K > M) return b * a;
  else return jet_of<M>(a.v * b.v, [&](int k) { return k < K ? fma(a.v, b.d[k], a.d[k] * b.v) : a.v * b.d[k]; });
}
template <int K>
OH_DEV Jet<K> operator+(const Jet<K> a, const double b) { return jet_of<K>(a.v + b, [&](int k) { return a.d[k]; }); }
template <int K>
OH_DEV Jet<K> operator+(const double a, const Jet<K> b) { return jet_of<K>(a + b.v, [&](int k) { return b.d[k]; }); }
template <int K>
OH_DEV Jet<K> operator-(const Jet<K> a, const double b) { return jet_of<K>(a.v - b, [&](int k) { return a.d[k]; }); }
template <int K>
OH_DEV Jet<K> operator-(const double a, const Jet<K> b) { return jet_of<K>(a - b.v, [&](int k) { return -b.d[k]; }); }
template <int K>
OH_DEV Jet<K> operator*(const Jet<K> a, const double b) { return jet_of<K>(a.v * b, [&](int k) { return a.d[k] * b; }); }
template <int K>
OH_DEV Jet<K> operator*(const double a, const Jet<K> b) { return jet_of<K>(a * b.v, [&](int k) { return a * b.d[k]; }); }
template <int K>
OH_DEV Jet<K> operator-(const Jet<K> a) { return jet_of<K>(-a.v, [&](int k) { return -a.d[k]; }); }

OH_DEV void sincosT(const double x, double* s, double* c) { sincos_joint(x, s, c); }
OH_DEV void sincosT(const Jet<1> x, Jet<1>* s, Jet<1>* c) {
  double sv, cv;
  sincos_joint(x.v, &sv, &cv);
  *s = {sv, cv * x.d[0]};
  *c = {cv, -sv * x.d[0]};
}

// scalar class of what depends on the joint angles alone, given the class of the velocities / accelerations / wrenches
template <class S>
struct RotOf {
  using T = S;
};
template <int K>
struct RotOf<Jet<K>> {
  using T = Jet<1>;
};

// the class of a product or sum: double of two doubles, else the wider jet
template <class A, class B, int K = (jet_k<A> > jet_k<B> ? jet_k<A> : jet_k<B>)>
struct Prom {
  using T = Jet<K>;
};
template <class A, class B>
struct Prom<A, B, 0> {
  using T = double;
};

template <class A, class B>
OH_DEV void crossT(const A* a, const B* b, typename Prom<A, B>::T* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
// o = M v, o = M^T v (row-major 3x3)
template <class A, class B>
OH_DEV void mvT(const A* M, const B* v, typename Prom<A, B>::T* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = M[3 * i] * v[0] + M[3 * i + 1] * v[1] + M[3 * i + 2] * v[2];
}
template <class A, class B>
OH_DEV void mTvT(const A* M, const B* v, typename Prom<A, B>::T* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = M[i] * v[0] + M[3 + i] * v[1] + M[6 + i] * v[2];
}
template <class A, class B>
OH_DEV typename Prom<A, B>::T dotT(const A* a, const B* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// R = R0 Rot(a, theta), Rot = c I + s [a]x + (1 - c) a a^T (spatialmath.py:89-99), row-wise as in rot_axis_right
template <class S>
OH_DEV void joint_rotation(const double* R0, const double* a, const S s, const S c, S* R) {
  const S omc = 1.0 - c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double* r = R0 + 3 * i;
    double x[3];
    cross3(r, a, x);
    const double d = dot3(r, a);
    const S k = omc * d;
    R[3 * i + 0] = c * r[0] + s * x[0] + k * a[0];
    R[3 * i + 1] = c * r[1] + s * x[1] + k * a[1];
    R[3 * i + 2] = c * r[2] + s * x[2] + k * a[2];
  }
}

// RobotModel.rnea (models.py:1819-1880) on scalars S (double or Jet): NB bodies, the last one on a fixed joint.
// The loops over the bodies are kept rolled (the per-body wrenches f, nn and sin/cos live in lane-private memory, indexed by the
// loop counter): unrolled, the dual-number recursion needs ~1500 live registers and the compiler spills two thirds of them.
template <int NB, class S, class SR = typename RotOf<S>::T>
OH_DEV void rnea_forward_body(const oh_dynamics* __restrict__ dy, const int i, const bool moving, const SR qi, const S qdi, const S qddi, S (&om)[3],
                              S (&omD)[3], S (&vD)[3], S* __restrict__ fi, S* __restrict__ ni, SR& sji, SR& cji) {
  S omi[3], omDi[3], vDi[3];
  S t1[3], t2[3], t3[3], acc[3];
  crossT(omD, dy->xyz[i], t1);
  crossT(om, dy->xyz[i], t2);
  crossT(om, t2, t3);
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = vD[k] + t1[k] + t3[k];
  if (moving) {
    SR Rp[9];
    sincosT(qi, &sji, &cji);
    joint_rotation(dy->R0[i], dy->axis[i], sji, cji, Rp);
    SR a[3];
    S omp[3], omDp[3];
    mTvT(Rp, dy->axis[i], a);  // iaxisi
    mTvT(Rp, om, omp);
    mTvT(Rp, omD, omDp);
    S aq[3] = {a[0] * qdi, a[1] * qdi, a[2] * qdi};
    S cr[3];
    crossT(omp, aq, cr);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      omi[k] = omp[k] + aq[k];
      omDi[k] = omDp[k] + cr[k] + a[k] * qddi;
    }
    mTvT(Rp, acc, vDi);
  } else {
    mTvT(dy->R0[i], om, omi);
    mTvT(dy->R0[i], omD, omDi);
    mTvT(dy->R0[i], acc, vDi);
  }
  crossT(omDi, dy->com[i], t1);
  crossT(omi, dy->com[i], t2);
  crossT(omi, t2, t3);
#pragma unroll
  for (int k = 0; k < 3; ++k) fi[k] = dy->mass[i] * (vDi[k] + t1[k] + t3[k]);
  S Io[3], IoD[3];
  mvT(dy->inertia[i], omi, Io);
  mvT(dy->inertia[i], omDi, IoD);
  crossT(omi, Io, t1);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ni[k] = IoD[k] + t1[k];
    om[k] = omi[k];
    omD[k] = omDi[k];
    vD[k] = vDi[k];
  }
}

template <int NB, class S, class SR = typename RotOf<S>::T>
OH_DEV void rnea_lit(const oh_dynamics* __restrict__ dy, const SR (&q)[NB - 1], const S (&qd)[NB - 1], const S (&qdd)[NB - 1], S (&tau)[NB - 1]) {
  S f[NB][3], nn[NB][3];
  SR sj[NB], cj[NB];
  S om[3], omD[3], vD[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    om[k] = S{};
    omD[k] = S{};
    vD[k] = S{} + dy->vd0[k];
  }
#pragma unroll 1
  for (int i = 0; i < NB - 1; ++i) rnea_forward_body<NB, S>(dy, i, true, q[i], qd[i], qdd[i], om, omD, vD, f[i], nn[i], sj[i], cj[i]);
  rnea_forward_body<NB, S>(dy, NB - 1, false, SR{}, S{}, S{}, om, omD, vD, f[NB - 1], nn[NB - 1], sj[NB - 1], cj[NB - 1]);
  // backward (models.py:1858-1880); the reference's fs/ns lists carry a leading zero entry: fs[i] == f[i-1]
  S ifi[3] = {f[NB - 1][0], f[NB - 1][1], f[NB - 1][2]};
  S ini[3], t1[3];
  crossT(dy->com[NB - 1], f[NB - 1], t1);
#pragma unroll
  for (int k = 0; k < 3; ++k) ini[k] = nn[NB - 1][k] + t1[k];
#pragma unroll 1
  for (int i = NB - 1; i >= 1; --i) {
    S a1[3], a2[3], a3[3], a4[3];
    if (i < NB - 1) {
      SR pRi[9];
      joint_rotation(dy->R0[i], dy->axis[i], sj[i], cj[i], pRi);
      mvT(pRi, ini, a1);
      mvT(pRi, ifi, a3);
    } else {
      mvT(dy->R0[i], ini, a1);
      mvT(dy->R0[i], ifi, a3);
    }
    crossT(dy->com[i - 1], f[i - 1], a2);
    crossT(dy->xyz[i], a3, a4);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ini[k] = nn[i - 1][k] + a1[k] + a2[k] + a4[k];
      ifi[k] = a3[k] + f[i - 1][k];
    }
    SR pR[9], ax[3];
    joint_rotation(dy->R0[i - 1], dy->axis[i - 1], sj[i - 1], cj[i - 1], pR);
    mTvT(pR, dy->axis[i - 1], ax);  // pRi^T axis
    tau[i - 1] = ini[0] * ax[0] + ini[1] * ax[1] + ini[2] * ax[2];
  }
}

// ---- the same torques by virtual work, outward pass only (round 4) -------------------------------------------------------------------------------
// tau_k = sum_{b >= k} f_b . v_b^(k) + (n_b + com_b x f_b) . w_b^(k): the inertial wrench of body b (models.py:1819-1856, the outward pass of the
// reference) paired with the twist (w^(k), v^(k)) a unit rate of joint k alone gives the frame of body b -- what the reference's inward pass
// (models.py:1858-1880) sums by handing wrenches to the parents, summed the other way round.  The twists travel outward with the recursion itself,
// so nothing has to wait for the last body: no per-body arrays.  rnea_lit keeps 8 bodies x (f, n, sin, cos) of dual numbers in lane-private memory
// (1.8 KB per lane, written once and read once: 36 KB per unit of k_tq_eval3, which made that kernel HBM-bound on its own scratch at 1.6 % of the
// bytes being useful); here the state is 7 twists in registers.  The twists depend on the joint angles alone (SR).  Equal to rnea_lit up to rounding.
template <int NB, bool MOVING, class S, class SR>
OH_DEV void vw_body(const oh_dynamics* __restrict__ dy, const int i, const SR qi, const S qdi, const S qddi, S (&om)[3], S (&omD)[3], S (&vD)[3],
                    SR (&wk)[NB - 1][3], SR (&vk)[NB - 1][3], S (&tau)[NB - 1]) {
  constexpr int NJ = NB - 1;
  using RT = typename std::conditional<MOVING, SR, double>::type;
  S t1[3], t2[3], t3[3], acc[3];
  crossT(omD, dy->xyz[i], t1);
  crossT(om, dy->xyz[i], t2);
  crossT(om, t2, t3);
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = vD[k] + t1[k] + t3[k];
  RT Rp[9];
  SR a[3];
  if constexpr (MOVING) {
    SR sj, cj;
    sincosT(qi, &sj, &cj);
    joint_rotation(dy->R0[i], dy->axis[i], sj, cj, Rp);
    mTvT(Rp, dy->axis[i], a);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) Rp[k] = dy->R0[i][k];
  }
  // twists first: they need the parent's values of nothing else, and the registers of (om, omD, vD) of the parent die right after
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    if (k < i) {
      SR x[3], y[3], wn[3], vn[3];
      crossT(wk[k], dy->xyz[i], x);
#pragma unroll
      for (int c = 0; c < 3; ++c) y[c] = vk[k][c] + x[c];
      mTvT(Rp, y, vn);
      mTvT(Rp, wk[k], wn);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        wk[k][c] = wn[c];
        vk[k][c] = vn[c];
      }
    } else if (MOVING && k == i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        wk[k][c] = a[c];
        vk[k][c] = SR{};
      }
    }
  }
  S omi[3], omDi[3], vDi[3];
  {
    S omp[3], omDp[3];
    mTvT(Rp, om, omp);
    mTvT(Rp, omD, omDp);
    if constexpr (MOVING) {
      S aq[3] = {a[0] * qdi, a[1] * qdi, a[2] * qdi};
      S cr[3];
      crossT(omp, aq, cr);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        omi[k] = omp[k] + aq[k];
        omDi[k] = omDp[k] + cr[k] + a[k] * qddi;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        omi[k] = omp[k];
        omDi[k] = omDp[k];
      }
    }
    mTvT(Rp, acc, vDi);
  }
  S f[3], m[3];
  crossT(omDi, dy->com[i], t1);
  crossT(omi, dy->com[i], t2);
  crossT(omi, t2, t3);
#pragma unroll
  for (int k = 0; k < 3; ++k) f[k] = dy->mass[i] * (vDi[k] + t1[k] + t3[k]);
  {
    S Io[3], IoD[3];
    mvT(dy->inertia[i], omi, Io);
    mvT(dy->inertia[i], omDi, IoD);
    crossT(omi, Io, t1);
    crossT(dy->com[i], f, t2);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      m[k] = IoD[k] + t1[k] + t2[k];
      om[k] = omi[k];
      omD[k] = omDi[k];
      vD[k] = vDi[k];
    }
  }
#pragma unroll
  for (int k = 0; k < NJ; ++k)
    if (k <= i) tau[k] = tau[k] + (dotT(f, vk[k]) + dotT(m, wk[k]));
}

// qs: the unit's (q | dq | ddq) at offsets 0, 8, 16 (LDS or global: indexed by the loop counter); lane j seeds joint j.  Seed: S / SR from (value, is-seed).
template <class S>
struct VwSeed;
template <>
struct VwSeed<Jet<3>> {
  static OH_DEV Jet<1> q(double v, double one) { return {v, one}; }
  static OH_DEV Jet<3> qd(double v, double one) { return {v, 0.0, one, 0.0}; }
  static OH_DEV Jet<3> qdd(double v, double one) { return {v, 0.0, 0.0, one}; }
};
template <int NB, class S, class SR = typename RotOf<S>::T>
OH_DEV void rnea_vw3(const oh_dynamics* __restrict__ dy, const double* qs, const int j, S (&tau)[NB - 1]) {
  constexpr int NJ = NB - 1;
  S om[3], omD[3], vD[3];
  SR wk[NJ][3], vk[NJ][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    om[k] = S{};
    omD[k] = S{};
    vD[k] = S{} + dy->vd0[k];
  }
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    tau[k] = S{};
#pragma unroll
    for (int c = 0; c < 3; ++c) wk[k][c] = vk[k][c] = SR{};
  }
#pragma unroll 1
  for (int i = 0; i < NJ; ++i) {
    const double one = (i == j) ? 1.0 : 0.0;
    vw_body<NB, true, S, SR>(dy, i, VwSeed<S>::q(qs[i], one), VwSeed<S>::qd(qs[8 + i], one), VwSeed<S>::qdd(qs[16 + i], one), om, omD, vD, wk, vk, tau);
  }
  vw_body<NB, false, S, SR>(dy, NJ, SR{}, S{}, S{}, om, omD, vD, wk, vk, tau);
}

// ---- d tau / d (q, dq, ddq) in closed form (round 4; numpy: oracle/torque.py:rnea_jacobian_spatial) ----------------------------------------------
// The dual-number recursions above cost a unit 7 lanes x (1 primal + 3 tangents) of the whole chain: ~120 k instructions per unit, 0.45 of the batch's
// device time.  In world coordinates (spatial vectors about the world origin, Featherstone 2008) the same derivative has a closed form.  With
//     S_l = (z_l, o_l x z_l)            joint screw,  v_b = sum_{l<=b} S_l dq_l,  a_b = a_0 + sum_{l<=b} (S_l ddq_l + v_l x S_l dq_l),
//     W_b = I_b a_b + v_b x* I_b v_b,   tau_k = S_k . sum_{b>=k} W_b          (what the reference's two passes compute, models.py:1819-1880)
// and  dS_l/dq_m = S_m x S_l (m < l),  dI_b/dq_m = S_m x* I_b - I_b S_m x (m <= b)  the product rule collapses (Jacobi identity) to
//     dW_b/dddq_j = I_b S_j,    dW_b/ddq_j = 2 (B_b S_j + I_b Sd_j),    dW_b/dq_j = S_j x* W_b + I_b Sdd_j + 2 B_b Sd_j          (b >= j)
//     Sd_j = v_j x S_j,  Sdd_j = a_j x S_j + v_j x Sd_j,  2 B_b x = I_b (x x v_b) + x x* I_b v_b + v_b x* I_b x = (Xi_b w_x, -2 p_b x w_x)
// (2 B_b sees only the angular part of x: Xi_b 3 x 3, p_b the linear momentum; Carpentier & Mansard 2018 and Singh, Russell & Wensing 2022 arrive at the
// same terms).  Summed over the subtree (composites I^C, Xi^C, p^C, F^C of body m = max(k, j)):
//     d tau_k / d(q_j, dq_j, ddq_j) = S_k . u(max(k, j)),   u_ddq = I^C S_j,  u_dq = 2 (B^C S_j + I^C Sd_j),  u_q = I^C Sdd_j + 2 B^C Sd_j (+ S_j x* F^C_j if k <= j).
// Lane j of a unit: the serial world-frame chain (cheap, every lane), the world inertia / Xi / wrench of body j (the fixed last body rides on lane N-1),
// exchange through LDS, then the inward composite sums and column j.  ~3 k instructions per lane.  Valid when the reference's recursion is the
// dynamics of a rigid-body chain: unit axes that the joint-origin rotation leaves in place (R0^T axis = axis: the angular velocity the reference adds,
// iRp @ axis, is then the axis Rot(axis, q) turns about; models.py:1821-1823).  oh_create_torque checks it; other tables take the dual-number path.
template <int N>
struct IdsWs {
  // A unit's LDS in k_tq_eval3, 277 doubles for N = 7 (nine units: 19.9 KB, so that two blocks share a SIMD's quarter of the CU's 160 KB):
  static constexpr int TW = 28;                  // pitch of the per-body slots: 28 = m, h (3), A (6), Xi (9), p (3), W (6) whatever the chain length; once phase 3 has consumed body
                                                 // m its slot takes row m of d tau / dz (3 N entries) and, behind it, lane m's row coefficients (RW)
  static constexpr int BD = 0;
  static constexpr int RW = 3 * N + 1;           // offset inside a slot: cf, cb, dw, bar, nrel, viol (6 doubles; the slot has 28 - 22 = 6 to spare)
  static constexpr int S = N * TW;               // joint screws, 6 each (phases 1-3); then, together with QS, the three rows of d p_link / dz (JP)
  static constexpr int QS = S + 6 * N;           // (q | dq | ddq) at 0, 8, 16: read by the loop counter in phase 1 and by the chain walk
  static constexpr int JP = S;                   // pitch 3 N + 1
  static constexpr int RW2 = QS + 24;            // cmpl[N], fsum[N]
  static constexpr int SIZE = (RW2 + 2 * N) | 1;  // odd: the units of a wavefront land in different banks
  static_assert(3 * (3 * N + 1) <= 6 * N + 24, "the rows of d p_link / dz take the place of the screws and of (q | dq | ddq)");
  static_assert(3 * N + 1 + 6 <= TW, "row m of d tau / dz and the six row coefficients behind it fit the slot of body m");
};
OH_DEV void mcross6(const double* x, const double* y, double* o) {  // motion x motion
  double t[3];
  cross3(x, y, o);
  cross3(x, y + 3, o + 3);
  cross3(x + 3, y, t);
  o[3] += t[0]; o[4] += t[1]; o[5] += t[2];
}
OH_DEV void fcross6(const double* x, const double* f, double* o) {  // motion x* force
  double t[3];
  cross3(x, f, o);
  cross3(x + 3, f + 3, t);
  o[0] += t[0]; o[1] += t[1]; o[2] += t[2];
  cross3(x, f + 3, o + 3);
}
// (n, f) = I (w, v) for a rigid-body inertia about the world origin: n = A w + h x v, f = m v - h x w;  A = (xx xy xz yy yz zz)
OH_DEV void inert6(const double m, const double* h, const double* A, const double* x, double* o) {
  double t[3];
  cross3(h, x + 3, t);
  o[0] = A[0] * x[0] + A[1] * x[1] + A[2] * x[2] + t[0];
  o[1] = A[1] * x[0] + A[3] * x[1] + A[4] * x[2] + t[1];
  o[2] = A[2] * x[0] + A[4] * x[1] + A[5] * x[2] + t[2];
  cross3(h, x, t);
  o[3] = m * x[3] - t[0];
  o[4] = m * x[4] - t[1];
  o[5] = m * x[5] - t[2];
}
OH_DEV double dot6(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5]; }

// world inertia, momentum coupling and wrench of body b from its (R, o, v, a), added to acc[28]
OH_DEV void ids_body(const oh_dynamics* __restrict__ dy, const int b, const double* __restrict__ p1, double* acc) {
  const double* R = p1;
  const double* o = p1 + 9;
  const double* v = p1 + 12;
  const double* a = p1 + 18;
  double c[3], T[9], Ic[9];
  mv3(R, dy->com[b], c);
  c[0] += o[0]; c[1] += o[1]; c[2] += o[2];
  mm3(R, dy->inertia[b], T);
  mmT3(T, R, Ic);
  const double m = dy->mass[b];
  const double h[3] = {m * c[0], m * c[1], m * c[2]};
  const double c2 = dot3(c, c);
  double A[6];
  A[0] = Ic[0] + m * (c2 - c[0] * c[0]);
  A[1] = 0.5 * (Ic[1] + Ic[3]) - m * c[0] * c[1];
  A[2] = 0.5 * (Ic[2] + Ic[6]) - m * c[0] * c[2];
  A[3] = Ic[4] + m * (c2 - c[1] * c[1]);
  A[4] = 0.5 * (Ic[5] + Ic[7]) - m * c[1] * c[2];
  A[5] = Ic[8] + m * (c2 - c[2] * c[2]);
  double Pm[6], W[6], t6[6];
  inert6(m, h, A, v, Pm);
  inert6(m, h, A, a, W);
  fcross6(v, Pm, t6);
#pragma unroll
  for (int k = 0; k < 6; ++k) W[k] += t6[k];
  // Xi = [w]x A + ([w]x A)^T - (h vl^T + vl h^T - 2 (vl . h) 1) - [n_P]x
  const double* w = v;
  const double* vl = v + 3;
  const double Af[9] = {A[0], A[1], A[2], A[1], A[3], A[4], A[2], A[4], A[5]};
  double OA[9];  // columns w x A[:, k]
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double col[3] = {Af[k], Af[3 + k], Af[6 + k]};
    double x[3];
    cross3(w, col, x);
    OA[k] = x[0]; OA[3 + k] = x[1]; OA[6 + k] = x[2];
  }
  const double vh = dot3(vl, h);
  double Xi[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) Xi[3 * r + k] = OA[3 * r + k] + OA[3 * k + r] - h[r] * vl[k] - vl[r] * h[k] + (r == k ? 2.0 * vh : 0.0);
  Xi[1] += Pm[2]; Xi[2] -= Pm[1];
  Xi[3] -= Pm[2]; Xi[5] += Pm[0];
  Xi[6] += Pm[1]; Xi[7] -= Pm[0];
  acc[0] += m;
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[1 + k] += h[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[4 + k] += A[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[10 + k] += Xi[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[19 + k] += Pm[3 + k];
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[22 + k] += W[k];
}

// ws: the unit's LDS workspace (IdsWs<N>::SIZE doubles), qs: (q | dq | ddq) at 0, 8, 16; every lane of the unit calls (block of one wavefront).
// Lane j leaves column j, N + j, 2 N + j of d tau / d (q, dq, ddq) in rows 0 .. N-1 of the tile at ws[0] and returns tau_j.
template <int N>
OH_DEV double rnea_idsva(const oh_dynamics* __restrict__ dy, double* __restrict__ ws, const int j, const bool writer) {
  using L = IdsWs<N>;
  const double* qs = ws + L::QS;
  double Sj[6], Sdj[6], Sddj[6];
  double own[24];  // (R, o, v, a) of body j, picked up on the way (every lane walks the whole chain)
  {
    double Rw[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, ow[3] = {0.0, 0.0, 0.0};
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, a[6] = {0.0, 0.0, 0.0, dy->vd0[0], dy->vd0[1], dy->vd0[2]};
#pragma unroll
    for (int k = 0; k < 6; ++k) Sj[k] = Sdj[k] = Sddj[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 24; ++k) own[k] = 0.0;
#pragma unroll 1
    for (int i = 0; i < N; ++i) {
      double o[3], Ri[9];
      mv3(Rw, dy->xyz[i], o);
      o[0] += ow[0]; o[1] += ow[1]; o[2] += ow[2];
      double S[6], Sd[6], Sdd[6], t6[6], Rp[9], sj, cj;
      mv3(Rw, dy->axis[i], S);
      cross3(o, S, S + 3);
      sincos_joint(qs[i], &sj, &cj);
      joint_rotation(dy->R0[i], dy->axis[i], sj, cj, Rp);
      mm3(Rw, Rp, Ri);
      mcross6(v, S, Sd);
      const double qd = qs[8 + i], qdd = qs[16 + i];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        v[k] = fma(S[k], qd, v[k]);
        a[k] = fma(Sd[k], qd, fma(S[k], qdd, a[k]));
      }
      mcross6(a, S, Sdd);
      mcross6(v, Sd, t6);
      const bool mine = i == j;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        Sdd[k] += t6[k];
        Sj[k] = mine ? S[k] : Sj[k];
        Sdj[k] = mine ? Sd[k] : Sdj[k];
        Sddj[k] = mine ? Sdd[k] : Sddj[k];
        own[12 + k] = mine ? v[k] : own[12 + k];
        own[18 + k] = mine ? a[k] : own[18 + k];
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) own[k] = mine ? Ri[k] : own[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) own[9 + k] = mine ? o[k] : own[9 + k];
      if (writer && mine) {
#pragma unroll
        for (int k = 0; k < 6; ++k) ws[L::S + 6 * i + k] = S[k];
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) Rw[k] = Ri[k];
      ow[0] = o[0]; ow[1] = o[1]; ow[2] = o[2];
    }
  }
  {
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
    ids_body(dy, j, own, acc);
    {  // the fixed last body moves with body N - 1: its frame follows from that body's (lane N - 1 keeps the result)
      double last[24], t3[3];
      mm3(own, dy->R0[N], last);
      mv3(own, dy->xyz[N], t3);
      last[9] = own[9] + t3[0]; last[10] = own[10] + t3[1]; last[11] = own[11] + t3[2];
#pragma unroll
      for (int k = 12; k < 24; ++k) last[k] = own[k];
      double acc2[28];
#pragma unroll
      for (int k = 0; k < 28; ++k) acc2[k] = 0.0;
      ids_body(dy, N, last, acc2);
#pragma unroll
      for (int k = 0; k < 28; ++k) acc[k] += (j == N - 1) ? acc2[k] : 0.0;
    }
    if (writer) {
#pragma unroll
      for (int k = 0; k < 28; ++k) ws[L::BD + L::TW * j + k] = acc[k];
    }
  }
  __syncthreads();
  double C[28];
  double u0s[6], u1s[6], u2s[6];
  double tau_j = 0.0;
#pragma unroll
  for (int k = 0; k < 28; ++k) C[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) u0s[k] = u1s[k] = u2s[k] = 0.0;
#pragma unroll 1
  for (int m = N - 1; m >= 0; --m) {
    const double* bd = ws + L::BD + L::TW * m;
    double Sm[6];
#pragma unroll
    for (int k = 0; k < 28; ++k) C[k] += bd[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) Sm[k] = ws[L::S + 6 * m + k];
    const double* hC = C + 1;
    const double* AC = C + 4;
    const double* XC = C + 10;
    const double* pC = C + 19;
    const double* FC = C + 22;
    double u0[6], u1[6], u2[6], t6[6], x[3];
    inert6(C[0], hC, AC, Sj, u2);
    inert6(C[0], hC, AC, Sdj, t6);
    mv3(XC, Sj, u1);
    cross3(pC, Sj, x);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      u1[k] = fma(2.0, t6[k], u1[k]);
      u1[3 + k] = 2.0 * (t6[3 + k] - x[k]);
    }
    inert6(C[0], hC, AC, Sddj, u0);
    mv3(XC, Sdj, t6);
    cross3(pC, Sdj, x);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      u0[k] += t6[k];
      u0[3 + k] -= 2.0 * x[k];
    }
    if (m == j) {
      fcross6(Sj, FC, t6);
      tau_j = dot6(Sm, FC);
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        u0s[k] = u0[k] + t6[k];
        u1s[k] = u1[k];
        u2s[k] = u2[k];
      }
    }
    const bool below = m > j;  // row below the diagonal: the composites of body m; else what column j froze at its own body
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      u0[k] = below ? u0[k] : u0s[k];
      u1[k] = below ? u1[k] : u1s[k];
      u2[k] = below ? u2[k] : u2s[k];
    }
    const double e0 = dot6(Sm, u0), e1 = dot6(Sm, u1), e2 = dot6(Sm, u2);
    __syncthreads();  // every lane of the unit has taken body m out of its slot: the slot becomes row m of d tau / dz
    if (writer) {
      ws[m * L::TW + j] = e0;
      ws[m * L::TW + N + j] = e1;
      ws[m * L::TW + 2 * N + j] = e2;
    }
  }
  return tau_j;
}

// ---- gradient of c^T tau (round 4; numpy: oracle/torque.py:rnea_ctau_gradient) ------------------------------------------------------------------
// Virtual work: c^T rnea(q, qd, qdd) = sum_b f_b . v_b(c) + n_b . w_b(c), the inertial wrench of body b (models.py:1819-1856, the outward pass of the
// reference) paired with the twist the joint rates c would give it.  Both come out of one outward recursion, so the gradient with respect to
// (q, qd, qdd) is one inward adjoint recursion: body i hands the adjoints of its (om, omD, vD) and of the virtual (wc, vo) to its parent.  A joint
// angle enters only through R_i^T = Rot(axis, q_i)^T R0^T, and d(R_i^T v)/dq_i = -axis x (R_i^T v), which is what `sw` collects.  Run on (Jet<1>, Jet<2>)
// scalars seeded with q_j and dq_j it returns rows q_j and dq_j of  sum_i c_i d^2 tau_i / d(q, dq, ddq)^2  (the torques are linear in ddq, so the rows
// of ddq_j are the transposed columns of those).
// Scalars: S for what depends on (q, qd, qdd), SR for what depends on the joint angles alone (rotations, axes, the virtual twists); qdd and c carry
// no tangent (nothing is differentiated twice with respect to them: tau is linear in qdd, c is a multiplier).
// Nothing is stored per body: the outward recursion is invertible (from the state of body i and its joint the state of the parent follows,
// om_p = Rp (om_i - a dq_i), ...), so the inward pass rebuilds each parent on the way (~300 instructions per body, no lane-private memory).
// Inputs come from LDS by the loop counter: zs = the unit's (q | dq | ddq | c) at 0, 8, 16, 24; lane j seeds joint j.  sink(i, gq_i, gqd_i, gqdd_i).
template <class S>
struct CtSeed;
template <>
struct CtSeed<Jet<2>> {
  static OH_DEV Jet<1> q(double v, double one) { return {v, one}; }
  static OH_DEV Jet<2> qd(double v, double one) { return {v, 0.0, one}; }
};
template <>
struct CtSeed<double> {
  static OH_DEV double q(double v, double) { return v; }
  static OH_DEV double qd(double v, double) { return v; }
};
template <int NB, class S, class SR, class Sink>
OH_DEV void rnea_ctau_grad_inv(const oh_dynamics* __restrict__ dy, const double* zs, const int j, Sink&& sink) {
  S om[3], omD[3], vD[3];
  SR wc[3], vo[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    om[k] = S{};
    omD[k] = S{};
    vD[k] = S{} + dy->vd0[k];
    wc[k] = SR{};
    vo[k] = SR{};
  }
  // outward: only the state of the last body survives
#pragma unroll 1
  for (int i = 0; i < NB; ++i) {
    const bool moving = i < NB - 1;
    S t1[3], t2[3], t3[3], acc[3];
    SR w[3], tw[3];
    crossT(omD, dy->xyz[i], t1);
    crossT(om, dy->xyz[i], t2);
    crossT(om, t2, t3);
    crossT(wc, dy->xyz[i], tw);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      acc[k] = vD[k] + t1[k] + t3[k];
      w[k] = vo[k] + tw[k];
    }
    SR Rp[9];
    if (moving) {
      SR sj, cj;
      sincosT(CtSeed<S>::q(zs[i], i == j ? 1.0 : 0.0), &sj, &cj);
      joint_rotation(dy->R0[i], dy->axis[i], sj, cj, Rp);
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) Rp[k] = SR{} + dy->R0[i][k];
    }
    S omp[3], omDp[3];
    SR wcp[3];
    mTvT(Rp, om, omp);
    mTvT(Rp, omD, omDp);
    mTvT(Rp, wc, wcp);
    if (moving) {
      SR a[3];
      mTvT(Rp, dy->axis[i], a);
      const S qdi = CtSeed<S>::qd(zs[8 + i], i == j ? 1.0 : 0.0);
      const double qddi = zs[16 + i], ci = zs[24 + i];
      S aq[3] = {a[0] * qdi, a[1] * qdi, a[2] * qdi};
      S cr[3];
      crossT(omp, aq, cr);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        om[k] = omp[k] + aq[k];
        omD[k] = omDp[k] + cr[k] + a[k] * qddi;
        wc[k] = wcp[k] + a[k] * ci;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        om[k] = omp[k];
        omD[k] = omDp[k];
        wc[k] = wcp[k];
      }
    }
    S vDi[3];
    SR voi[3];
    mTvT(Rp, acc, vDi);
    mTvT(Rp, w, voi);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      vD[k] = vDi[k];
      vo[k] = voi[k];
    }
  }
  // inward: (om, omD, vD, wc, vo) is the state of body i; its parent is rebuilt from it
  S b_om[3], b_omD[3], b_vD[3], b_wc[3], b_vo[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) b_om[k] = b_omD[k] = b_vD[k] = b_wc[k] = b_vo[k] = S{};
#pragma unroll 1
  for (int i = NB - 1; i >= 0; --i) {
    const bool moving = i < NB - 1;
    SR Rp[9], a[3];
    S qdi = S{};
    double qddi = 0.0, ci = 0.0;
    if (moving) {
      SR sj, cj;
      sincosT(CtSeed<S>::q(zs[i], i == j ? 1.0 : 0.0), &sj, &cj);
      joint_rotation(dy->R0[i], dy->axis[i], sj, cj, Rp);
      mTvT(Rp, dy->axis[i], a);
      qdi = CtSeed<S>::qd(zs[8 + i], i == j ? 1.0 : 0.0);
      qddi = zs[16 + i];
      ci = zs[24 + i];
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) Rp[k] = SR{} + dy->R0[i][k];
#pragma unroll
      for (int k = 0; k < 3; ++k) a[k] = SR{};
    }
    const double* cm = dy->com[i];
    const double* r = dy->xyz[i];
    const double m = dy->mass[i];
    // the parent's state (the base: at rest, accelerating against gravity), and what it looked like in the frame of body i
    S om_p[3], omD_p[3], vD_p[3], omp[3], omDp[3];
    SR wc_p[3], vo_p[3], wcp[3];
    {
      S aq[3] = {a[0] * qdi, a[1] * qdi, a[2] * qdi};
#pragma unroll
      for (int k = 0; k < 3; ++k) omp[k] = om[k] - aq[k];
      S cr[3];
      crossT(omp, aq, cr);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        omDp[k] = omD[k] - cr[k] - a[k] * qddi;
        wcp[k] = wc[k] - a[k] * ci;
      }
      if (i > 0) {
        S accp[3], t1[3], t2[3], t3[3];
        SR wp[3], tw[3];
        mvT(Rp, omp, om_p);
        mvT(Rp, omDp, omD_p);
        mvT(Rp, wcp, wc_p);
        mvT(Rp, vD, accp);
        mvT(Rp, vo, wp);
        crossT(omD_p, r, t1);
        crossT(om_p, r, t2);
        crossT(om_p, t2, t3);
        crossT(wc_p, r, tw);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          vD_p[k] = accp[k] - t1[k] - t3[k];
          vo_p[k] = wp[k] - tw[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          om_p[k] = S{};
          omD_p[k] = S{};
          vD_p[k] = S{} + dy->vd0[k];
          wc_p[k] = SR{};
          vo_p[k] = SR{};
          omp[k] = S{};    // exactly, not up to the rounding of the inversion
          omDp[k] = S{};
          wcp[k] = SR{};
        }
      }
    }
    // local term f_i . vc_i + n_i . wc_i
    {
      S t1[3], t2[3], t3[3], fi[3], Io[3], IoD[3], ni[3];
      crossT(omD, cm, t1);
      crossT(om, cm, t2);
      crossT(om, t2, t3);
#pragma unroll
      for (int k = 0; k < 3; ++k) fi[k] = m * (vD[k] + t1[k] + t3[k]);
      mvT(dy->inertia[i], om, Io);
      mvT(dy->inertia[i], omD, IoD);
      crossT(om, Io, t1);
#pragma unroll
      for (int k = 0; k < 3; ++k) ni[k] = IoD[k] + t1[k];
      SR tw[3], vci[3];
      crossT(wc, cm, tw);
#pragma unroll
      for (int k = 0; k < 3; ++k) vci[k] = vo[k] + tw[k];
      S cf[3];
      crossT(cm, fi, cf);
      SR cv[3], Itw[3];
      crossT(cm, vci, cv);
      mTvT(dy->inertia[i], wc, Itw);
      const S oc = dotT(om, cm), ov = dotT(om, vci);
      const SR cvv = dotT(cm, vci);
      S wxo[3], Itwo[3], Ixw[3];
      crossT(wc, om, wxo);
      mTvT(dy->inertia[i], wxo, Itwo);
      crossT(Io, wc, Ixw);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        b_vo[k] = b_vo[k] + fi[k];
        b_wc[k] = b_wc[k] + cf[k] + ni[k];
        b_vD[k] = b_vD[k] + m * vci[k];
        b_omD[k] = b_omD[k] + m * cv[k] + Itw[k];
        b_om[k] = b_om[k] + m * (vci[k] * oc + cm[k] * ov - 2.0 * (om[k] * cvv)) + Itwo[k] + Ixw[k];
      }
    }
    // through the step of body i
    S b_omp[3];
    if (moving) {
      S aq[3] = {a[0] * qdi, a[1] * qdi, a[2] * qdi};
      S x1[3], x2[3], b_aq[3], b_a[3];
      crossT(aq, b_omD, x1);
      crossT(b_omD, omp, x2);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        b_omp[k] = b_om[k] + x1[k];
        b_aq[k] = b_om[k] + x2[k];
        b_a[k] = b_aq[k] * qdi + b_omD[k] * qddi + b_wc[k] * ci;
      }
      const S gqd_i = dotT(b_aq, a);
      const S gqdd_i = dotT(b_omD, a);
      S s1[3], s2[3], s3[3], s4[3], s5[3], s6[3];
      crossT(omp, b_omp, s1);
      crossT(omDp, b_omD, s2);
      crossT(wcp, b_wc, s3);
      crossT(a, b_a, s4);
      crossT(vD, b_vD, s5);
      crossT(vo, b_vo, s6);
      S sw[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) sw[k] = s1[k] + s2[k] + s3[k] + s4[k] + s5[k] + s6[k];
      sink(i, -dotT(sw, dy->axis[i]), gqd_i, gqdd_i);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) b_omp[k] = b_om[k];
    }
    if (i > 0) {
      S b_acc[3], b_w[3], Ro[3], RoD[3], Rw[3], x1[3], x2[3];
      mvT(Rp, b_vD, b_acc);
      mvT(Rp, b_vo, b_w);
      mvT(Rp, b_omp, Ro);
      mvT(Rp, b_omD, RoD);
      mvT(Rp, b_wc, Rw);
      crossT(r, b_acc, x1);
      crossT(r, b_w, x2);
      const S opr = dotT(om_p, r), opb = dotT(om_p, b_acc), rb = dotT(r, b_acc);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        b_om[k] = Ro[k] + b_acc[k] * opr + r[k] * opb - 2.0 * (om_p[k] * rb);
        b_omD[k] = RoD[k] + x1[k];
        b_vD[k] = b_acc[k];
        b_wc[k] = Rw[k] + x2[k];
        b_vo[k] = b_w[k];
        om[k] = om_p[k];
        omD[k] = omD_p[k];
        vD[k] = vD_p[k];
        wc[k] = wc_p[k];
        vo[k] = vo_p[k];
      }
    }
  }
}

}  // namespace oh_dyn
