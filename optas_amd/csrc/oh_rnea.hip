// The stand-alone inverse-dynamics kernels behind oh_rnea, oh_rnea_jac and oh_rnea_hess (their device code: oh_rnea.h).
#include "oh_rnea.h"

namespace {
using namespace oh_dyn;

// Batched recursive Newton-Euler inverse dynamics, one lane per sample, NB bodies (the last one rigidly attached).  Statement by statement
// RobotModel.rnea (optas/models.py:1819-1880); AoS [N][NB-1] at the ABI.  A double-precision copy of rnea_lit kept on purpose: rnea_lit<NB, double>
// keeps its body loops rolled, which costs this kernel 400 B of scratch per lane at NB = 8, and unrolled it needs 255 VGPRs against 219 here.
OH_DEV void mTv3(const double* A, const double* v, double* o) {  // o = A^T v
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}
template <int NB>
__global__ __launch_bounds__(256) void k_rnea(const oh_dynamics* __restrict__ dy, int n, const double* __restrict__ q,
                                              const double* __restrict__ qd, const double* __restrict__ qdd, double* __restrict__ tau) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  constexpr int ND = NB - 1;
  double f[NB][3], nn[NB][3], sj[NB], cj[NB];
  double om[3] = {0, 0, 0}, omD[3] = {0, 0, 0}, vD[3] = {dy->vd0[0], dy->vd0[1], dy->vd0[2]};
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    // iRp = (R0_i Rot(axis_i, q_i))^T ; for the last body no joint rotation (models.py:1820-1832)
    double Rp[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rp[k] = dy->R0[i][k];
    double qdi = 0.0, qddi = 0.0;
    if (i != NB - 1) {
      double s, c, zc[3];
      sincos_joint(q[(size_t)u * ND + i], &s, &c);
      sj[i] = s; cj[i] = c;
      rot_axis_right(Rp, dy->axis[i], s, c, zc);
      qdi = qd[(size_t)u * ND + i];
      qddi = qdd[(size_t)u * ND + i];
    } else {
      sj[i] = 0.0; cj[i] = 1.0;
    }
    double a[3], omp[3], omDp[3];
    mTv3(Rp, dy->axis[i], a);  // iaxisi
    mTv3(Rp, om, omp);
    mTv3(Rp, omD, omDp);
    double omi[3], omDi[3];
    if (i != NB - 1) {
      const double aq[3] = {a[0] * qdi, a[1] * qdi, a[2] * qdi};
      double cr[3];
      cross3(omp, aq, cr);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        omi[k] = omp[k] + aq[k];
        omDi[k] = omDp[k] + cr[k] + a[k] * qddi;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) { omi[k] = omp[k]; omDi[k] = omDp[k]; }
    }
    // vDi = iRp (vD + omD x r + om x (om x r)),  r = joint origin
    double t1[3], t2[3], t3[3], acc[3], vDi[3];
    cross3(omD, dy->xyz[i], t1);
    cross3(om, dy->xyz[i], t2);
    cross3(om, t2, t3);
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = vD[k] + t1[k] + t3[k];
    mTv3(Rp, acc, vDi);
    // fi = m (vDi + omDi x c + omi x (omi x c)) ; ni = I omDi + omi x (I omi)
    cross3(omDi, dy->com[i], t1);
    cross3(omi, dy->com[i], t2);
    cross3(omi, t2, t3);
#pragma unroll
    for (int k = 0; k < 3; ++k) f[i][k] = dy->mass[i] * (vDi[k] + t1[k] + t3[k]);
    double Io[3], IoD[3];
    mv3(dy->inertia[i], omi, Io);
    mv3(dy->inertia[i], omDi, IoD);
    cross3(omi, Io, t1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      nn[i][k] = IoD[k] + t1[k];
      om[k] = omi[k]; omD[k] = omDi[k]; vD[k] = vDi[k];
    }
  }
  // backward (models.py:1858-1880); reference lists fs/ns carry a leading zero entry: fs[i] == f[i-1]
  double ifi[3] = {f[NB - 1][0], f[NB - 1][1], f[NB - 1][2]};
  double ini[3], t1[3];
  cross3(dy->com[NB - 1], f[NB - 1], t1);
#pragma unroll
  for (int k = 0; k < 3; ++k) ini[k] = nn[NB - 1][k] + t1[k];
#pragma unroll
  for (int i = NB - 1; i >= 1; --i) {
    double pRi[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) pRi[k] = dy->R0[i][k];
    if (i < NB - 1) { double zc[3]; rot_axis_right(pRi, dy->axis[i], sj[i], cj[i], zc); }
    double a1[3], a2[3], a3[3], a4[3];
    mv3(pRi, ini, a1);
    cross3(dy->com[i - 1], f[i - 1], a2);
    mv3(pRi, ifi, a3);
    cross3(dy->xyz[i], a3, a4);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ini[k] = nn[i - 1][k] + a1[k] + a2[k] + a4[k];
      ifi[k] = a3[k] + f[i - 1][k];
    }
    double pR[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) pR[k] = dy->R0[i - 1][k];
    double zc[3];
    rot_axis_right(pR, dy->axis[i - 1], sj[i - 1], cj[i - 1], zc);
    double ax[3];
    mTv3(pR, dy->axis[i - 1], ax);  // pRi^T axis
    tau[(size_t)u * ND + (i - 1)] = dot3(ini, ax);
  }
}


// d tau / d (q, qd, qdd) of RobotModel.rnea (what the reference obtains with casadi.jacobian of the same graph, optimization.py:8-24): one lane per
// (sample, direction), the literal recursion on dual numbers.  q, qd, qdd [n][N] -> J [n][N][3 N] row-major.
template <int N>
__global__ __launch_bounds__(64) void k_rnea_jac(const oh_dynamics* __restrict__ dy, const int n, const double* __restrict__ q, const double* __restrict__ qd,
                                                 const double* __restrict__ qdd, double* __restrict__ J) {
  constexpr int NZ = 3 * N, UPW = 64 / NZ;
  const int lane = threadIdx.x;
  const int ul = lane / NZ, d = lane - ul * NZ;
  const long long u = (long long)blockIdx.x * UPW + ul;
  if (ul >= UPW || u >= n) return;
  Jet<1> a[N], b[N], c[N], tau[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    a[j] = {q[u * N + j], d == j ? 1.0 : 0.0};
    b[j] = {qd[u * N + j], d == N + j ? 1.0 : 0.0};
    c[j] = {qdd[u * N + j], d == 2 * N + j ? 1.0 : 0.0};
  }
  rnea_lit<N + 1, Jet<1>>(dy, a, b, c, tau);
#pragma unroll
  for (int i = 0; i < N; ++i) J[((size_t)u * N + i) * NZ + d] = tau[i].d[0];
}

// sum_i c_i d^2 tau_i / d (q, qd, qdd)^2 (what the reference obtains as ddh by AD of the CasADi graph, optimization.py:8-24): one lane per
// (sample, joint); q, qd, qdd, c [n][N] -> H [n][3 N][3 N] row-major.  Lane j writes rows j and N + j and, by symmetry, column j of the ddq rows.
template <int N>
__global__ __launch_bounds__(64) void k_rnea_hess(const oh_dynamics* __restrict__ dy, const int n, const double* __restrict__ q, const double* __restrict__ qd,
                                                  const double* __restrict__ qdd, const double* __restrict__ c, double* __restrict__ H) {
  constexpr int NZ = 3 * N, UPW = 64 / N;
  __shared__ double zs_l[UPW][32];
  const int lane = threadIdx.x;
  int ul = lane / N, j = lane - ul * N;
  const bool lane_ok = ul < UPW;
  if (!lane_ok) {
    ul = UPW - 1;
    j = N - 1;
  }
  long long u = (long long)blockIdx.x * UPW + ul;
  const bool active = lane_ok && u < n;
  if (u >= n) u = n - 1;
  if (lane_ok) {
    zs_l[ul][j] = q[u * N + j];
    zs_l[ul][8 + j] = qd[u * N + j];
    zs_l[ul][16 + j] = qdd[u * N + j];
    zs_l[ul][24 + j] = c[u * N + j];
  }
  __syncthreads();
  double* Hu = H + (size_t)u * NZ * NZ;
  rnea_ctau_grad_inv<N + 1, Jet<2>, Jet<1>>(dy, zs_l[ul], j, [&](const int k, const Jet<2> gq, const Jet<2> gqd, const Jet<2> gqdd) {
    if (!active) return;
    Hu[j * NZ + k] = gq.d[0];
    Hu[j * NZ + N + k] = gqd.d[0];
    Hu[j * NZ + 2 * N + k] = gqdd.d[0];
    Hu[(N + j) * NZ + k] = gq.d[1];
    Hu[(N + j) * NZ + N + k] = gqd.d[1];
    Hu[(N + j) * NZ + 2 * N + k] = 0.0;
    Hu[(2 * N + k) * NZ + j] = gqdd.d[0];
    Hu[(2 * N + k) * NZ + N + j] = 0.0;
    Hu[(2 * N + k) * NZ + 2 * N + j] = 0.0;
  });
}

}  // namespace

// the three kernels by chain length: C(N) for N = 1 .. 8 joints, nbodies = N + 1
#define OH_RNEA_DISPATCH(nbodies, C) \
  switch (nbodies) {                \
    case 2: C(1); break;            \
    case 3: C(2); break;            \
    case 4: C(3); break;            \
    case 5: C(4); break;            \
    case 6: C(5); break;            \
    case 7: C(6); break;            \
    case 8: C(7); break;            \
    case 9: C(8); break;            \
    default: return false;          \
  }
bool oh_launch_rnea(hipStream_t s, const oh_dynamics* d_dyn, int nbodies, int n, const double* q, const double* qd, const double* qdd, double* tau) {
#define C(NN) hipLaunchKernelGGL(k_rnea<NN + 1>, dim3((n + 255) / 256), dim3(256), 0, s, d_dyn, n, q, qd, qdd, tau)
  OH_RNEA_DISPATCH(nbodies, C)
#undef C
  return true;
}
bool oh_launch_rnea_jac(hipStream_t s, const oh_dynamics* d_dyn, int nbodies, int n, const double* q, const double* qd, const double* qdd, double* J) {
#define C(NN) hipLaunchKernelGGL(k_rnea_jac<NN>, dim3((unsigned)((n + (64 / (3 * NN)) - 1) / (64 / (3 * NN)))), dim3(64), 0, s, d_dyn, n, q, qd, qdd, J)
  OH_RNEA_DISPATCH(nbodies, C)
#undef C
  return true;
}
bool oh_launch_rnea_hess(hipStream_t s, const oh_dynamics* d_dyn, int nbodies, int n, const double* q, const double* qd, const double* qdd, const double* c, double* H) {
#define C(NN) hipLaunchKernelGGL(k_rnea_hess<NN>, dim3((unsigned)((n + (64 / NN) - 1) / (64 / NN))), dim3(64), 0, s, d_dyn, n, q, qd, qdd, c, H)
  OH_RNEA_DISPATCH(nbodies, C)
#undef C
  return true;
}
