// Host side of the kinematics and dynamics entry points of any handle with constants: inverse dynamics (oh_rnea*), forward kinematics and
// Jacobian (oh_fk_jac*), kinematics of a link in the frame of another (oh_link_kin*).
#include <cmath>
#include <cstring>
#include "oh_rnea.h"

#include "oh_handle.h"

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

// K1 compiled for the handle's chain (oh_specialize; fk_common by the "specialize" option)
int specialize_fk(oh_handle* h) {
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
