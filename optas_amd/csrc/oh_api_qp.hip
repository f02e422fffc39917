// Host side of the dense QP family (OH_PROBLEM_QP): creation, the optional tape the QP data is read from, the solve.  State: oh_handle::qp.
#include "oh_handle.h"
#include "oh_qp_layout.h"

extern "C" int oh_create_qp(const oh_qp_desc* desc, oh_handle** out) {
  if (!desc || !out) return fail(OH_ERR_INVALID, "oh_create_qp: null argument");
  *out = nullptr;
  if (desc->n < 1 || desc->n > OH_QP_MAX_N || desc->m < 0 || desc->m > OH_QP_MAX_M || desc->me < 0 || desc->me > OH_QP_MAX_ME || desc->me > desc->n)
    return fail(OH_ERR_INVALID, "oh_create_qp: sizes out of range (1 <= n <= 128, 0 <= m <= 1024, 0 <= me <= min(128, n))");
  int rc = OH_OK;
  oh_handle* h = open_handle("oh_create_qp", OH_PROBLEM_QP, 1, desc->n, 0, &rc);
  if (!h) return rc;
  oh_qp_desc& d = h->qp.desc;
  d = *desc;
  if (d.max_iter <= 0) d.max_iter = 100;
  if (!(d.tol > 0.0)) d.tol = 1e-9;
  *out = h;
  return OH_OK;
}

// doubles of the parameter vector of a handle without a tape: [P | q | M | c | A | b]
size_t qp_np(const oh_qp_desc& q) { return qp_row_doubles(q.n, q.m, q.me); }

extern "C" int oh_qp_set_tape(oh_handle* h, const oh_tape_desc* d) {
  if (!h || !d) return fail(OH_ERR_INVALID, "oh_qp_set_tape: null argument");
  if (h->desc.kind != OH_PROBLEM_QP) return fail(OH_ERR_STATE, "oh_qp_set_tape: not an OH_PROBLEM_QP handle");
  if (const int rc = tape_validate(d, "oh_qp_set_tape")) return rc;
  QpState& qp = h->qp;
  if (d->nx != qp.desc.n || d->n_ineq != qp.desc.m || d->n_eq != qp.desc.me)
    return fail(OH_ERR_INVALID, "oh_qp_set_tape: the tape's nx / n_ineq / n_eq differ from the handle's n / m / me");
  HIPCHK(hipSetDevice(h->device));
  qp.use_tape = false;
  if (const int rc = upload_tape(h, d, nullptr)) return rc;
  h->tape.P = tape_params(d);
  {
    // instructions whose value depends on x: the probes after the first re-run only these
    std::vector<char> dep((size_t)d->len, 0);
    std::vector<int> list;
    for (int i = 0; i < d->len; ++i) {
      const int o = d->op[i], n = tape_op_arity(o);
      dep[i] = o == OP_X || (n >= 1 && dep[d->a[i]]) || (n == 2 && dep[d->b[i]]);
      if (dep[i]) list.push_back(i);
    }
    qp.xdep.release();
    qp.n_xdep = (int)list.size();
    HIPCHK(qp.xdep.reserve(list.size() + 1));
    if (!list.empty()) HIPCHK(hipMemcpy(qp.xdep, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
  }
  for (DevBuf<double>* b : {&qp.rows, &qp.val, &qp.f0}) b->release();  // the register file of another tape: size it again at the next solve
  qp.use_tape = true;
  return OH_OK;
}

int qp_solve_device(oh_handle* h, const Solve& a) {
  HIPCHK(hipSetDevice(h->device));
  QpState& qp = h->qp;
  const TapeState& tp = h->tape;  // (qp.use_tape: the tape the QP data is read from)
  const oh_qp_desc& q = qp.desc;
  const int B = a.B;
  QpParams Q{};
  Q.n = q.n; Q.m = q.m; Q.me = q.me; Q.np = (int)qp_np(q); Q.max_iter = q.max_iter; Q.tol = q.tol;
  Q.nwork = (int)qp_work_doubles(q.n, q.m, q.me);
  const int Bp = (B + 63) / 64 * 64;
  const int mode = (int)optv(h, "qp_mode");
  const bool large = oh_qp_is_large(Q), block = oh_qp_takes_block(Q, mode);
  HIPCHK(qp.mult.reserve((size_t)(q.m + q.me + 1) * Bp));
  // what k_qp_solve_block keeps in global memory: a slice per instance (its vectors and H live in LDS); the other kernels: [Q.nwork][Bp]
  if (block) HIPCHK(qp.blk.reserve(oh_qp_block_work_doubles(Q) * (size_t)B + 1));
  else HIPCHK(qp.work.reserve((size_t)Q.nwork * Bp));
  const int work_stride = (int)(qp.work.cap / (size_t)Q.nwork);  // the Bp qp.work was allocated for (0: never)
  // register file of the tape interpreter: a lane per instance, or (a few instances: B <= 64) a lane per probe point of every instance;
  // large handles: rows and f(0, p) by instance, the register file by the instances of one launch (64 lanes each)
  const int Bv = large ? B : (B <= 64 ? (B * 64 > Bp ? B * 64 : Bp) : Bp);
  const int chunk = (large && qp.use_tape) ? oh_qp_assemble_block_chunk(tp.P, B) : 0;
  // (qp.f0 is allocated last: its capacity is the Bv all three hold; large handles: qp.val holds 64 lanes for each of `chunk` instances)
  if (qp.use_tape && ((size_t)Bv > qp.f0.cap || (size_t)tp.P.len * chunk * 64 > qp.val.cap)) {
    for (DevBuf<double>* b : {&qp.rows, &qp.val, &qp.f0}) b->release();
    HIPCHK(qp.rows.reserve((size_t)Q.np * Bv));
    HIPCHK(qp.val.reserve((size_t)tp.P.len * (large ? (size_t)chunk * 64 : (size_t)Bv)));
    HIPCHK(qp.f0.reserve((size_t)Bv));
  }
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  std::string err;
  qp.last_block = block ? 1 : 0;
  if (qp.use_tape) {
    if (large) {
      if (oh_launch_qp_assemble_block(h->stream, Q, tp.P, tp.op, tp.a, tp.b, tp.c, tp.rows, qp.xdep, qp.n_xdep, B, chunk,
                                      a.p, qp.val, qp.rows, qp.f0, &err))
        return fail(OH_ERR_HIP, "oh_solve: " + err);
    } else {
      oh_launch_qp_assemble(h->stream, Q, tp.P, tp.op, tp.a, tp.b, tp.c, tp.rows, qp.xdep, qp.n_xdep, B, B <= 64 ? B * 64 : (int)qp.f0.cap, a.p, qp.val,
                            qp.rows, qp.f0);
    }
  }
  const double* data = qp.use_tape ? qp.rows.p : a.p;  // [B][Q.np]: assembled from the tape, or the caller's
  if (oh_launch_qp_solve(h->stream, Q, B, work_stride, a.x0, data, block ? qp.blk.p : qp.work.p, a.x, a.f, a.kkt, a.iters, a.status, qp.mult, mode, &err))
    return fail(OH_ERR_HIP, "oh_solve: " + err);
  if (qp.use_tape && a.f) oh_launch_qp_add_constant(h->stream, B, a.f, qp.f0);
  return finish_solve(h, 1);
}
