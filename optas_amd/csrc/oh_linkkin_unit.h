// Body of k_link_kin (oh_linkkin.hip): kinematics of one link in the frame of another link of the same model, one lane per configuration.
//   T_L = (R_L, p_L), quat_L : global transform / reference-signed quaternion of the link  (root->link chain, as K1 walks it)
//   T_B = (R_B, p_B), quat_B : the same of the base link                                    (root->base chain)
//   rot  = R_L R_B^T, pos = p_L - rot p_B                 T_L invt(T_B)                      (models.py:884-898, 949-960, 1011-1023)
//   quat = quat_L * inv(quat_B), the reference's product  = inv(quat_B) (x) quat_L, Hamilton (models.py:1108-1122, spatialmath.py:298-328)
//   rpy  = getrpy(quat)                                                                      (models.py:1148-1197, spatialmath.py:384-404)
//   Jg   = blkdiag(R_B^T, R_B^T) J_L                                                         (models.py:1320-1344)
//   Ja   = [Jg rows 0-2; d rpy / d q]                                                        (models.py:1370-1385, 1590-1611)
//   axis = rot a, a a unit vector                                                            (models.py:1637-1670)
// The reference takes d rpy / d q from AD of the graph of rpy.  In closed form: quat is a unit quaternion of R_B^T R_L, and a revolute joint j moves
// that rotation with the angular velocity w_j = R_B^T (z_j [j on the link chain] - z_j [j on the base chain]) (world axes z_j), so
//   d quat / d q_j = 1/2 (w_j, 0) (x) quat      and      d rpy / d q_j = G(quat) 1/2 Q(quat) w_j = (E R_B^T) (z_j [link] - z_j [base])
// with G the 3x4 partial derivatives of getrpy.  A joint on the common prefix of the two chains has the same axis on both: its column is exactly zero
// (the relative rotation does not depend on it), and so is every column of a prismatic joint.  The host counts that prefix once (OhLinkFrames.n_shared).
#pragma once
#include "oh_device.h"
#include "oh_kernels.h"

// o = A^T v
OH_DEV void mtv3(const double* A, const double* v, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}

// One actuated joint of a chain, exactly the step of fk_jac_unit: (R, p, quat) move past joint k at joint value qk; z = its world axis, pj = its world origin.
OH_DEV void link_kin_joint(const oh_chain* __restrict__ ch, const int k, const double qk, double (&R)[9], double (&p)[3], double (&quat)[4], double (&z)[3],
                           double (&pj)[3]) {
  double t[3];
  mv3(R, ch->p0[k], t);
  p[0] += t[0]; p[1] += t[1]; p[2] += t[2];
  if (!ch->r0ident[k]) {
    double Rn[9];
    mm3(R, ch->R0[k], Rn);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rn[i];
  }
  pj[0] = p[0]; pj[1] = p[1]; pj[2] = p[2];
  double qn[4];
  qmul(quat, ch->quat0[k], qn);  // == fromrpy(rpy) * quat in the reference's reversed product
  if (ch->jtype[k] == 0) {
    double sh, chh;
    sincos_joint(0.5 * qk, &sh, &chh);
    const double s = 2.0 * sh * chh, c = 1.0 - 2.0 * sh * sh;
    if (ch->axcode[k] != 0) rot_principal_right(R, ch->axcode[k], s, c, z);
    else rot_axis_right(R, ch->axis[k], s, c, z);
    const double qa[4] = {sh * ch->axis[k][0], sh * ch->axis[k][1], sh * ch->axis[k][2], chh};
    qmul(qn, qa, quat);
  } else {
    mv3(R, ch->axis[k], z);
    p[0] += z[0] * qk; p[1] += z[1] * qk; p[2] += z[2] * qk;
    quat[0] = qn[0]; quat[1] = qn[1]; quat[2] = qn[2]; quat[3] = qn[3];
  }
}

// the frame of the link itself: the chain's constant tool transform after the last actuated joint
OH_DEV void link_kin_tool(const oh_chain* __restrict__ ch, double (&R)[9], double (&p)[3], double (&quat)[4]) {
  double t[3], Rn[9], qn[4];
  mv3(R, ch->p_tool, t);
  p[0] += t[0]; p[1] += t[1]; p[2] += t[2];
  mm3(R, ch->R_tool, Rn);
  qmul(quat, ch->quat_tool, qn);
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) quat[i] = qn[i];
}

// soa != 0: q[ndof][n] and every output [components][n] (unit index fastest); soa == 0: q[n][ndof], outputs [n][components] (the reference layout).
// One instantiation serves both layouts (only the addresses differ), so the two give the same bits.  NC: actuated joints of the link chain (0: run-time).
template <int NC>
__device__ void link_kin_unit(const OhLinkFrames* __restrict__ fr, const int n, const int soa, const double* __restrict__ q, const double a0, const double a1,
                              const double a2, const oh_link_out out) {
  constexpr int NM = NC ? NC : OH_MAX_CHAIN;
  const unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= (unsigned)n) return;
  const oh_chain* __restrict__ cl = &fr->link;
  const oh_chain* __restrict__ cb = &fr->base;
  const int nc = NC ? NC : cl->n_chain;
  const int nb = cb->n_chain;
  const int ns = fr->n_shared;
  const int ndof = cl->ndof;
  auto at = [&](const int comp, const int ncomp) -> size_t { return soa ? (size_t)comp * (unsigned)n + u : (size_t)u * (unsigned)ncomp + (unsigned)comp; };

  // ---- root -> link, keeping every joint's axis and origin for the Jacobian columns
  double RL[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pL[3] = {0, 0, 0}, qL[4] = {0, 0, 0, 1};
  double z[NM][3], pj[NM][3];
#pragma unroll
  for (int k = 0; k < NM; ++k) {
    if (NC || k < nc) link_kin_joint(cl, k, q[at(cl->qidx[k], ndof)], RL, pL, qL, z[k], pj[k]);
  }
  link_kin_tool(cl, RL, pL, qL);
  // ---- root -> base
  double RB[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pB[3] = {0, 0, 0}, qB[4] = {0, 0, 0, 1};
  for (int m = 0; m < nb; ++m) {
    double zb[3], pjb[3];
    link_kin_joint(cb, m, q[at(cb->qidx[m], ndof)], RB, pB, qB, zb, pjb);
  }
  link_kin_tool(cb, RB, pB, qB);

  double rot[9];
  mmT3(RL, RB, rot);
  if (out.pos) {
    double t[3];
    mv3(rot, pB, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) out.pos[at(i, 3)] = pL[i] - t[i];
  }
  if (out.rot) {
#pragma unroll
    for (int i = 0; i < 9; ++i) out.rot[at(i, 9)] = rot[i];
  }
  if (out.axis) {
    const double a[3] = {a0, a1, a2};
    double t[3];
    mv3(rot, a, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) out.axis[at(i, 3)] = t[i];
  }

  double M[9];  // d rpy / d q_j = M z_j (see the head of this file)
  if (out.quat || out.rpy || out.Ja) {
    const double sB = qB[0] * qB[0] + qB[1] * qB[1] + qB[2] * qB[2] + qB[3] * qB[3];  // Quaternion.inv divides by sumsqr (spatialmath.py:321-328)
    const double qBi[4] = {-qB[0] / sB, -qB[1] / sB, -qB[2] / sB, qB[3] / sB};
    double qr[4];
    qmul(qBi, qL, qr);
    if (out.quat) {
#pragma unroll
      for (int i = 0; i < 4; ++i) out.quat[at(i, 4)] = qr[i];
    }
    if (out.rpy || out.Ja) {
      const double x = qr[0], y = qr[1], zq = qr[2], w = qr[3];
      const double sr = 2.0 * (w * x + y * zq), cr = 1.0 - 2.0 * (x * x + y * y);
      const double sp = 2.0 * (w * y - zq * x);
      const double sy = 2.0 * (w * zq + x * y), cy = 1.0 - 2.0 * (y * y + zq * zq);
      const bool lock = fabs(sp) >= 1.0;  // the reference's branch: pitch = +pi/2 whatever the sign of sinp
      if (out.rpy) {
        out.rpy[at(0, 3)] = atan2(sr, cr);
        out.rpy[at(1, 3)] = lock ? 1.57079632679489661923 : asin(sp);
        out.rpy[at(2, 3)] = atan2(sy, cy);
      }
      if (out.Ja) {
        // G = d (roll, pitch, yaw) / d (x, y, z, w); the constant pitch branch has derivative zero
        const double ir = 1.0 / (sr * sr + cr * cr), iy = 1.0 / (sy * sy + cy * cy);
        const double ip = lock ? 0.0 : 1.0 / sqrt(1.0 - sp * sp);
        const double G[3][4] = {{(2.0 * cr * w + 4.0 * sr * x) * ir, (2.0 * cr * zq + 4.0 * sr * y) * ir, 2.0 * cr * y * ir, 2.0 * cr * x * ir},
                                {-2.0 * zq * ip, 2.0 * w * ip, -2.0 * x * ip, 2.0 * y * ip},
                                {2.0 * cy * y * iy, (2.0 * cy * x + 4.0 * sy * y) * iy, (2.0 * cy * w + 4.0 * sy * zq) * iy, 2.0 * cy * zq * iy}};
        double E[9];  // G times the 4x3 matrix of w -> 1/2 (w, 0) (x) quat
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          E[3 * r + 0] = 0.5 * (G[r][0] * w - G[r][1] * zq + G[r][2] * y - G[r][3] * x);
          E[3 * r + 1] = 0.5 * (G[r][0] * zq + G[r][1] * w - G[r][2] * x - G[r][3] * y);
          E[3 * r + 2] = 0.5 * (-G[r][0] * y + G[r][1] * x + G[r][2] * w - G[r][3] * zq);
        }
        mmT3(E, RB, M);
      }
    }
  }

  if (out.Jg || out.Ja) {
    const int rowlen = 6 * ndof;
    // columns of joints on neither chain are zero (models.py:1251-1254); Jg has no column for a joint that is on the base chain only
    if (out.Jg && nc != ndof)
      for (int i = 0; i < rowlen; ++i) out.Jg[at(i, rowlen)] = 0.0;
    if (out.Ja && nc + nb - ns != ndof)
      for (int i = 0; i < rowlen; ++i) out.Ja[at(i, rowlen)] = 0.0;
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      if (NC || k < nc) {
        const int col = cl->qidx[k];
        const bool rev = cl->jtype[k] == 0;
        double lin[3], g[6];
        if (rev) {
          const double d[3] = {pL[0] - pj[k][0], pL[1] - pj[k][1], pL[2] - pj[k][2]};
          cross3(z[k], d, lin);  // models.py:1236-1239
        } else {
          lin[0] = z[k][0]; lin[1] = z[k][1]; lin[2] = z[k][2];  // models.py:1245-1246
        }
        mtv3(RB, lin, g);
        if (rev) mtv3(RB, z[k], g + 3);
        else g[3] = g[4] = g[5] = 0.0;
        if (out.Jg) {
#pragma unroll
          for (int r = 0; r < 6; ++r) out.Jg[at(r * ndof + col, rowlen)] = g[r];
        }
        if (out.Ja) {
          double w3[3] = {0.0, 0.0, 0.0};
          if (rev && k >= ns) mv3(M, z[k], w3);
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            out.Ja[at(r * ndof + col, rowlen)] = g[r];
            out.Ja[at((3 + r) * ndof + col, rowlen)] = w3[r];
          }
        }
      }
    }
    // joints on the base chain only: they turn the frame the angles are taken in.  The base chain is walked once more instead of keeping its axes.
    if (out.Ja && nb > ns) {
      double Rw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pw[3] = {0, 0, 0}, qw[4] = {0, 0, 0, 1};
      for (int m = 0; m < nb; ++m) {
        double zb[3], pjb[3];
        link_kin_joint(cb, m, q[at(cb->qidx[m], ndof)], Rw, pw, qw, zb, pjb);
        if (m >= ns) {
          const int col = cb->qidx[m];
          double w3[3] = {0.0, 0.0, 0.0};
          if (cb->jtype[m] == 0) mv3(M, zb, w3);
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            out.Ja[at(r * ndof + col, rowlen)] = 0.0;
            out.Ja[at((3 + r) * ndof + col, rowlen)] = -w3[r];
          }
        }
      }
    }
  }
}
