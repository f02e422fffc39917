"""Numeric evaluation of ``optas_amd.expr`` trees at a given (x, p): the diagnostics of the reference's Solver
(``evaluate_cost``, ``evaluate_cost_terms``, ``violated_constraints``, optas/solver.py:167-237,269-314) need the value
of individual cost terms / constraint blocks.  Forward kinematics inside a tree goes through liboptas_hip
(``RobotModel.get_global_link_*`` -> ``oh_fk_jac``); everything else is elementwise host bookkeeping on the results.
"""
from __future__ import annotations

import numpy as np

from .builder import IntegrationResidual
from .expr import Add, Atan2, Block, Const, Expr, Gather, LinkFunction, MatMul, Mul, ParamCol, ParamRef, PathInFrame, RneaFunction, RobotStates, Rows, Scale, Square, StateCols, StateRef, Sub, SumSqr, VCat, VarRef


def _block(container, vec, label):
    off = container.offsets()[label]
    m, n = container[label].shape
    return vec[off : off + m * n].reshape(n, m).T


def evaluate(e: Expr, opt, x: np.ndarray, p: np.ndarray) -> np.ndarray:
    """Value of node ``e`` as a 2-D array (rows x cols like the CasADi matrix it stands for).  Link functions of parameters only
    (``J(qc)``, ``p(qc)``) are memoised per parameter vector: reading P, q, M, c off a QP evaluates the trees dozens of times with
    the same p, and each of those nodes is a round trip to the GPU."""
    if isinstance(e, Const):
        return e.value
    if isinstance(e, LinkFunction) and e.q.degree() == 0:
        cache = getattr(opt, "_link_cache", None)
        key = p.tobytes()
        if cache is None or cache[0] != key:
            cache = (key, {})
            opt._link_cache = cache
        if id(e) not in cache[1]:
            cache[1][id(e)] = _evaluate(e, opt, x, p)
        return cache[1][id(e)]
    return _evaluate(e, opt, x, p)


def _evaluate(e: Expr, opt, x: np.ndarray, p: np.ndarray) -> np.ndarray:
    if isinstance(e, Const):
        return e.value
    if isinstance(e, ParamRef):
        return _block(opt.parameters, p, e.name)
    if isinstance(e, ParamCol):
        return _block(opt.parameters, p, e.param.name)[:, [e.col]]
    if isinstance(e, StateRef):
        full = _block(opt.decision_variables, x, e.var_name)
        return full if e.t is None else full[:, [e.t]]
    if isinstance(e, StateCols):
        return _block(opt.decision_variables, x, e.state.var_name)[:, e.lo : e.hi]
    if isinstance(e, RobotStates):
        X = evaluate(e.states, opt, x, p)
        Pm = evaluate(e.params, opt, x, p)
        full = np.zeros(e.shape)
        full[list(e.opt_idx), :] = X
        full[list(e.par_idx), :] = Pm
        return full
    if isinstance(e, Rows):
        return evaluate(e.a, opt, x, p)[list(e.idx), :]
    if isinstance(e, Block):
        return np.asarray(evaluate(e.a, opt, x, p))[np.ix_(list(e.ridx), list(e.cidx))]
    if isinstance(e, VarRef):
        return _block(opt.decision_variables, x, e.var_name)
    if isinstance(e, Gather):
        va = np.broadcast_to(np.asarray(evaluate(e.a, opt, x, p), dtype=np.float64), e.a.shape).T.reshape(-1)
        return e.sign * va[np.maximum(e.idx, 0)]
    if isinstance(e, LinkFunction):
        q = evaluate(e.q, opt, x, p)
        if e.what == "position":
            return np.asarray(e.robot.get_global_link_position(e.link, q)).reshape(3, -1)
        if e.what == "quaternion":
            return np.asarray(e.robot.get_global_link_quaternion(e.link, q)).reshape(4, -1)
        if e.what == "geometric_jacobian":
            return np.asarray(e.robot.get_global_link_geometric_jacobian(e.link, q.reshape(-1)))
        if e.what == "axis":  # R_link(q) a, column by column
            return np.stack([np.asarray(e.robot.get_global_link_rotation(e.link, q[:, c])) @ e.axis for c in range(q.shape[1])], axis=1)
        return np.asarray(e.robot.get_global_link_rotation(e.link, q.reshape(-1)))
    if isinstance(e, RneaFunction):
        return np.asarray(e.robot.rnea(evaluate(e.q, opt, x, p), evaluate(e.qd, opt, x, p), evaluate(e.qdd, opt, x, p))).reshape(e.shape)
    if isinstance(e, PathInFrame):
        return evaluate(e.origin, opt, x, p).reshape(3, 1) + evaluate(e.rotation, opt, x, p) @ e.local
    if isinstance(e, IntegrationResidual):
        X = evaluate(e.x, opt, x, p)
        Xd = evaluate(e.xd, opt, x, p)[:, : e.n]
        return X[:, :-1][:, : e.n] + e.dt[None, :] * Xd - X[:, 1:][:, : e.n]
    if isinstance(e, Sub):
        return evaluate(e.a, opt, x, p) - evaluate(e.b, opt, x, p)
    if isinstance(e, Add):
        return evaluate(e.a, opt, x, p) + evaluate(e.b, opt, x, p)
    if isinstance(e, Scale):
        return e.w * evaluate(e.a, opt, x, p)
    if isinstance(e, Atan2):
        return np.arctan2(evaluate(e.y, opt, x, p), evaluate(e.x, opt, x, p))
    if isinstance(e, MatMul):
        return evaluate(e.a, opt, x, p) @ evaluate(e.b, opt, x, p)
    if isinstance(e, VCat):
        return np.vstack([np.broadcast_to(evaluate(q_, opt, x, p), q_.shape) for q_ in e.parts])
    if isinstance(e, Mul):
        return evaluate(e.a, opt, x, p) * evaluate(e.b, opt, x, p)
    if isinstance(e, Square):
        v = evaluate(e.a, opt, x, p)
        return v * v
    if isinstance(e, SumSqr):
        v = evaluate(e.a, opt, x, p)
        return np.array([[float(np.sum(v * v))]])
    raise NotImplementedError(f"cannot evaluate {type(e).__name__}")


# ---- first derivatives (the reference's df, dk, da, dg, dh, dv: casadi.jacobian of the same graphs, optimization.py:8-24) ----------------------
def _sel(container, label, rows_cols=None):
    """Indices into x of the column-major entries of a decision-variable block (optionally of the columns ``rows_cols``)."""
    off = container.offsets()[label]
    m, n = container[label].shape
    cols = range(n) if rows_cols is None else rows_cols
    return np.concatenate([off + m * c + np.arange(m) for c in cols]) if len(list(cols)) else np.zeros(0, dtype=int)


def jacobian(e: Expr, opt, x: np.ndarray, p: np.ndarray):
    """(value (m, n), J (m n, nx)): the node's value and the Jacobian of its column-major vec w.r.t. x, by forward propagation through the
    tree.  Kinematics derivatives come from the geometric Jacobian of oh_fk_jac (d p = J_lin dq, d quat = 1/2 (omega, 0) (x) quat,
    dR = [omega]x R), inverse dynamics from oh_rnea_jac: exact like CasADi's AD, no differencing."""
    nx = opt.nx
    val = evaluate(e, opt, x, p)
    val = np.asarray(val, dtype=np.float64)
    m, n = e.shape
    val = np.broadcast_to(val, (m, n)) if val.shape != (m, n) else val

    def zero():
        return val, np.zeros((m * n, nx))

    if e.degree() == 0 or isinstance(e, (Const, ParamRef, ParamCol)):
        return zero()
    if isinstance(e, (StateRef, VarRef, StateCols)):
        J = np.zeros((m * n, nx))
        if isinstance(e, StateRef):
            idx = _sel(opt.decision_variables, e.var_name, None if e.t is None else [e.t])
        elif isinstance(e, StateCols):
            idx = _sel(opt.decision_variables, e.state.var_name, range(e.lo, e.hi))
        else:
            idx = _sel(opt.decision_variables, e.var_name)
        J[np.arange(m * n), idx] = 1.0
        return val, J
    if isinstance(e, RobotStates):
        _, Js = jacobian(e.states, opt, x, p)
        J = np.zeros((m * n, nx))
        ms = e.states.shape[0]
        for c in range(n):
            for k, r in enumerate(e.opt_idx):
                J[c * m + r] = Js[c * ms + k]
        return val, J
    if isinstance(e, Rows):
        _, Ja = jacobian(e.a, opt, x, p)
        ma = e.a.shape[0]
        rows = [c * ma + r for c in range(n) for r in e.idx]
        return val, Ja[rows]
    if isinstance(e, Block):
        _, Ja = jacobian(e.a, opt, x, p)
        ma = e.a.shape[0]
        rows = [c * ma + r for c in e.cidx for r in e.ridx]
        return val, Ja[rows]
    if isinstance(e, Gather):
        _, Ja = jacobian(e.a, opt, x, p)
        return val, e.sign.T.reshape(-1, 1) * Ja[np.maximum(e.idx, 0).T.reshape(-1)]
    if isinstance(e, (Sub, Add)):
        _, Ja = jacobian(e.a, opt, x, p)
        _, Jb = jacobian(e.b, opt, x, p)
        Ja, Jb = _bcast_rows(Ja, e.a.shape, (m, n)), _bcast_rows(Jb, e.b.shape, (m, n))
        return val, (Ja - Jb) if isinstance(e, Sub) else (Ja + Jb)
    if isinstance(e, Scale):
        _, Ja = jacobian(e.a, opt, x, p)
        return val, e.w * Ja
    if isinstance(e, Square):
        va, Ja = jacobian(e.a, opt, x, p)
        return val, 2.0 * va.T.reshape(-1, 1) * Ja
    if isinstance(e, SumSqr):
        va, Ja = jacobian(e.a, opt, x, p)
        return val, (2.0 * va.T.reshape(1, -1)) @ Ja
    if isinstance(e, Mul):
        va, Ja = jacobian(e.a, opt, x, p)
        vb, Jb = jacobian(e.b, opt, x, p)
        Ja, Jb = _bcast_rows(Ja, e.a.shape, (m, n)), _bcast_rows(Jb, e.b.shape, (m, n))
        va, vb = np.broadcast_to(va, (m, n)), np.broadcast_to(vb, (m, n))
        return val, vb.T.reshape(-1, 1) * Ja + va.T.reshape(-1, 1) * Jb
    if isinstance(e, MatMul):
        va, Ja = jacobian(e.a, opt, x, p)
        vb, Jb = jacobian(e.b, opt, x, p)
        ma, ka = e.a.shape
        J = np.zeros((m * n, nx))
        for c in range(n):
            for r in range(m):
                for k in range(ka):  # (A B)[r, c] = sum_k A[r, k] B[k, c]
                    J[c * m + r] += Ja[k * ma + r] * vb[k, c] + va[r, k] * Jb[c * ka + k]
        return val, J
    if isinstance(e, VCat):
        J = np.zeros((m * n, nx))
        r0 = 0
        for part in e.parts:
            _, Jp = jacobian(part, opt, x, p)
            mp = part.shape[0]
            Jp = _bcast_rows(Jp, part.shape, (mp, n))
            for c in range(n):
                J[c * m + r0 : c * m + r0 + mp] = Jp[c * mp : (c + 1) * mp]
            r0 += mp
        return val, J
    if isinstance(e, Atan2):
        vy, Jy = jacobian(e.y, opt, x, p)
        vx, Jx = jacobian(e.x, opt, x, p)
        d = (vx * vx + vy * vy).T.reshape(-1, 1)
        return val, (vx.T.reshape(-1, 1) * Jy - vy.T.reshape(-1, 1) * Jx) / d
    if isinstance(e, IntegrationResidual):
        _, JX = jacobian(e.x, opt, x, p)
        _, JXd = jacobian(e.xd, opt, x, p)
        mm = e.x.shape[0]
        J = np.zeros((m * n, nx))
        for c in range(e.n):
            J[c * mm : (c + 1) * mm] = JX[c * mm : (c + 1) * mm] + e.dt[c] * JXd[c * mm : (c + 1) * mm] - JX[(c + 1) * mm : (c + 2) * mm]
        return val, J
    if isinstance(e, LinkFunction):
        q, Jq = jacobian(e.q, opt, x, p)  # (ndof, cols), (ndof cols, nx)
        nd, cols = q.shape
        pose, Jg = e.robot._kin(e.link).fk_jac(np.ascontiguousarray(q.T))  # (cols, 7), (cols, 6, ndof)
        J = np.zeros((m * n, nx))
        for c in range(cols):
            Jqc = Jq[c * nd : (c + 1) * nd]
            if e.what == "position":
                J[3 * c : 3 * c + 3] = Jg[c, :3] @ Jqc
            elif e.what == "quaternion":
                qx, qy, qz, qw = pose[c, 3:]
                Lq = 0.5 * np.array([[qw, qz, -qy], [-qz, qw, qx], [qy, -qx, qw], [-qx, -qy, -qz]])  # d quat = 1/2 (omega, 0) (x) quat
                J[4 * c : 4 * c + 4] = Lq @ Jg[c, 3:] @ Jqc
            elif e.what == "axis":  # d u = omega x u
                u = val[:, c]
                K = np.array([[0.0, u[2], -u[1]], [-u[2], 0.0, u[0]], [u[1], -u[0], 0.0]])  # omega x u = K omega
                J[3 * c : 3 * c + 3] = K @ Jg[c, 3:] @ Jqc
            elif e.what == "rotation":
                R = val
                W = Jg[c, 3:] @ Jqc  # omega per unit dx, (3, nx)
                for col in range(3):  # d R[:, col] = omega x R[:, col]; vec is column-major
                    r = R[:, col]
                    K = np.array([[0.0, r[2], -r[1]], [-r[2], 0.0, r[0]], [r[1], -r[0], 0.0]])  # omega x r = K omega
                    J[3 * col : 3 * col + 3] = K @ W
            else:
                raise NotImplementedError("derivative of the geometric Jacobian (second-order kinematics) is not provided")
        return val, J
    if isinstance(e, RneaFunction):
        q, Jq = jacobian(e.q, opt, x, p)
        qd, Jqd = jacobian(e.qd, opt, x, p)
        qdd, Jqdd = jacobian(e.qdd, opt, x, p)
        nd, cols = q.shape
        Jt = e.robot.rnea_jacobian(q, qd, qdd)  # (cols, nd, 3 nd)
        J = np.zeros((m * n, nx))
        for c in range(cols):
            sl = slice(c * nd, (c + 1) * nd)
            J[sl] = Jt[c, :, :nd] @ Jq[sl] + Jt[c, :, nd : 2 * nd] @ Jqd[sl] + Jt[c, :, 2 * nd :] @ Jqdd[sl]
        return val, J
    if isinstance(e, PathInFrame):
        if e.origin.degree() == 0 and e.rotation.degree() == 0:
            return zero()
        raise NotImplementedError("derivative of a path frame that depends on the decision variables is not provided")
    raise NotImplementedError(f"no derivative rule for {type(e).__name__}")


def _bcast_rows(J, shape_from, shape_to):
    """Rows of a Jacobian for an operand that CasADi-style broadcasting repeats (scalar or column against a matrix)."""
    (mf, nf), (mt, nt) = shape_from, shape_to
    if (mf, nf) == (mt, nt):
        return J
    if (mf, nf) == (1, 1):
        return np.repeat(J, mt * nt, axis=0)
    if mf == mt and nf == 1:
        return np.tile(J, (nt, 1))
    raise NotImplementedError(f"broadcast of a {shape_from} operand to {shape_to}")


# ---- second derivatives (the reference's ddf, ddg, ddh, ddv: casadi.jacobian of the Jacobians, optimization.py:8-24) ---------------------------
def _unbcast(W, shape_to, shape_from):
    """Weights of a broadcast operand: what `_bcast_rows` repeats is summed back."""
    (mt, nt), (mf, nf) = shape_to, shape_from
    if (mf, nf) == (mt, nt):
        return W
    if (mf, nf) == (1, 1):
        return np.array([[W.sum()]])
    if mf == mt and nf == 1:
        return W.sum(axis=1, keepdims=True)
    raise NotImplementedError(f"broadcast of a {shape_from} operand to {shape_to}")


def _rows_of(J, shape, c):
    m = shape[0]
    return J[c * m : (c + 1) * m]


def _hamilton_left(o, quat):
    """(o, 0) (x) quat, xyzw storage: the product behind d quat = 1/2 (omega, 0) (x) quat."""
    ox, oy, oz = o
    x, y, z, w = quat
    return np.array([ox * w + oy * z - oz * y, -ox * z + oy * w + oz * x, ox * y - oy * x + oz * w, -ox * x - oy * y - oz * z])


def weighted_hessian(e: Expr, opt, x: np.ndarray, p: np.ndarray, W: np.ndarray) -> np.ndarray:
    """sum over the entries of node ``e`` of W[r, c] * (Hessian of that entry w.r.t. x), nx x nx, exact: the weights travel down the tree
    (transposed through the linear nodes), every nonlinear node adds its own curvature from the first derivatives of its operands.  Second-order
    kinematics come out of the geometric Jacobian oh_fk_jac returns: d2 p / dq_i dq_j = z_i x Jp_j (i <= j), d2 quat, d2 R and d2 (R a) from the same axes.
    Inverse dynamics: oh_rnea_hess (round 4).  Raises NotImplementedError for nodes without a rule (the Jacobian-valued link function): the caller
    differences."""
    nx = opt.nx
    m, n = e.shape
    W = np.broadcast_to(np.asarray(W, dtype=np.float64), (m, n))
    Z = np.zeros((nx, nx))
    if e.degree() <= 1 and not isinstance(e, (LinkFunction, RneaFunction, Mul, MatMul, Square, SumSqr, Atan2)):
        return Z  # affine in x
    if isinstance(e, Rows):
        Wa = np.zeros(e.a.shape)
        Wa[list(e.idx), :] = W
        return weighted_hessian(e.a, opt, x, p, Wa)
    if isinstance(e, Block):
        Wa = np.zeros(e.a.shape)
        Wa[np.ix_(list(e.ridx), list(e.cidx))] = W
        return weighted_hessian(e.a, opt, x, p, Wa)
    if isinstance(e, RobotStates):
        return weighted_hessian(e.states, opt, x, p, W[list(e.opt_idx), :])
    if isinstance(e, Gather):
        wa = np.zeros(e.a.numel())
        np.add.at(wa, np.maximum(e.idx, 0).reshape(-1), (W * e.sign).reshape(-1))
        return weighted_hessian(e.a, opt, x, p, wa.reshape(e.a.shape[1], e.a.shape[0]).T)
    if isinstance(e, (Sub, Add)):
        Ha = weighted_hessian(e.a, opt, x, p, _unbcast(W, (m, n), e.a.shape))
        Hb = weighted_hessian(e.b, opt, x, p, _unbcast(W, (m, n), e.b.shape))
        return Ha - Hb if isinstance(e, Sub) else Ha + Hb
    if isinstance(e, Scale):
        return weighted_hessian(e.a, opt, x, p, e.w * W)
    if isinstance(e, VCat):
        H, r0 = Z.copy(), 0
        for part in e.parts:
            mp = part.shape[0]
            H += weighted_hessian(part, opt, x, p, _unbcast(W[r0 : r0 + mp], (mp, n), part.shape))
            r0 += mp
        return H
    if isinstance(e, SumSqr):
        va, Ja = jacobian(e.a, opt, x, p)
        w = float(W[0, 0])
        return 2.0 * w * (Ja.T @ Ja) + weighted_hessian(e.a, opt, x, p, 2.0 * w * va)
    if isinstance(e, Square):
        va, Ja = jacobian(e.a, opt, x, p)
        wv = W.T.reshape(-1)
        return 2.0 * (Ja.T * wv) @ Ja + weighted_hessian(e.a, opt, x, p, 2.0 * W * va)
    if isinstance(e, Mul):
        va, Ja = jacobian(e.a, opt, x, p)
        vb, Jb = jacobian(e.b, opt, x, p)
        Ja, Jb = _bcast_rows(Ja, e.a.shape, (m, n)), _bcast_rows(Jb, e.b.shape, (m, n))
        va, vb = np.broadcast_to(va, (m, n)), np.broadcast_to(vb, (m, n))
        wv = W.T.reshape(-1)
        C = (Ja.T * wv) @ Jb
        return C + C.T + weighted_hessian(e.a, opt, x, p, _unbcast(W * vb, (m, n), e.a.shape)) + weighted_hessian(e.b, opt, x, p, _unbcast(W * va, (m, n), e.b.shape))
    if isinstance(e, MatMul):
        va, Ja = jacobian(e.a, opt, x, p)
        vb, Jb = jacobian(e.b, opt, x, p)
        ma, ka = e.a.shape
        H = Z.copy()
        for c in range(n):
            for r in range(m):
                if W[r, c] != 0.0:
                    for k in range(ka):
                        C = np.outer(Ja[k * ma + r], Jb[c * ka + k])
                        H += W[r, c] * (C + C.T)
        return H + weighted_hessian(e.a, opt, x, p, W @ vb.T) + weighted_hessian(e.b, opt, x, p, va.T @ W)
    if isinstance(e, RneaFunction):
        # sum_{i,c} W[i, c] Hessian of tau_i(column c) = G_c^T (sum_i W[i, c] d^2 tau_i / d(q, qd, qdd)^2) G_c  (oh_rnea_hess: the adjoint of the
        # reference's recursion on dual numbers, exact like CasADi's AD of the same graph, optimization.py:8-24) + the curvature of the operands
        # weighted through d tau / d(q, qd, qdd)
        q, Jq = jacobian(e.q, opt, x, p)
        qd, Jqd = jacobian(e.qd, opt, x, p)
        qdd, Jqdd = jacobian(e.qdd, opt, x, p)
        nd, cols = q.shape
        Hc = e.robot.rnea_hessian(q, qd, qdd, W)  # (cols, 3 nd, 3 nd)
        Jt = e.robot.rnea_jacobian(q, qd, qdd)    # (cols, nd, 3 nd)
        H = Z.copy()
        Wq, Wqd, Wqdd = np.zeros((nd, cols)), np.zeros((nd, cols)), np.zeros((nd, cols))
        for c in range(cols):
            sl = slice(c * nd, (c + 1) * nd)
            G = np.concatenate([Jq[sl], Jqd[sl], Jqdd[sl]], 0)  # (3 nd, nx)
            H += G.T @ Hc[c] @ G
            wj = W[:, c] @ Jt[c]  # weights the operands' own second derivatives inherit
            Wq[:, c], Wqd[:, c], Wqdd[:, c] = wj[:nd], wj[nd : 2 * nd], wj[2 * nd :]
        return H + weighted_hessian(e.q, opt, x, p, Wq) + weighted_hessian(e.qd, opt, x, p, Wqd) + weighted_hessian(e.qdd, opt, x, p, Wqdd)
    if isinstance(e, Atan2):
        vy, Jy = jacobian(e.y, opt, x, p)
        vx, Jx = jacobian(e.x, opt, x, p)
        Jy, Jx = _bcast_rows(Jy, e.y.shape, (m, n)), _bcast_rows(Jx, e.x.shape, (m, n))
        vy, vx = np.broadcast_to(vy, (m, n)), np.broadcast_to(vx, (m, n))
        d = vx * vx + vy * vy
        tyy, txx, txy = -2.0 * vx * vy / d**2, 2.0 * vx * vy / d**2, (vy * vy - vx * vx) / d**2
        wv = W.T.reshape(-1)
        C = (Jy.T * (wv * txy.T.reshape(-1))) @ Jx
        H = (Jy.T * (wv * tyy.T.reshape(-1))) @ Jy + (Jx.T * (wv * txx.T.reshape(-1))) @ Jx + C + C.T
        return H + weighted_hessian(e.y, opt, x, p, _unbcast(W * vx / d, (m, n), e.y.shape)) + weighted_hessian(e.x, opt, x, p, _unbcast(-W * vy / d, (m, n), e.x.shape))
    if isinstance(e, LinkFunction):
        if e.what == "geometric_jacobian":
            raise NotImplementedError("second derivatives of the Jacobian-valued link function are not provided")
        q, Jq = jacobian(e.q, opt, x, p)
        nd, cols = q.shape
        pose, Jg = e.robot._kin(e.link).fk_jac(np.ascontiguousarray(q.T))
        H = Z.copy()
        Wq = np.zeros((nd, cols))
        for c in range(cols):
            Jp, Jw = Jg[c, :3], Jg[c, 3:]
            S = np.zeros((nd, nd))  # sum_k W[k, c] d2 out_k / dq dq
            if e.what == "position":
                w3 = W[:, c]
                for i in range(nd):
                    for j in range(i, nd):
                        S[i, j] = S[j, i] = float(w3 @ np.cross(Jw[:, i], Jp[:, j]))
                Wq[:, c] = Jp.T @ w3
            elif e.what == "quaternion":
                quat, w4 = pose[c, 3:], W[:, c]
                for i in range(nd):
                    hi = _hamilton_left(Jw[:, i], quat)
                    for j in range(i, nd):
                        dz = np.cross(Jw[:, i], Jw[:, j]) if i < j else np.zeros(3)
                        S[i, j] = S[j, i] = float(w4 @ (0.5 * _hamilton_left(dz, quat) + 0.25 * _hamilton_left(Jw[:, j], hi)))
                Wq[:, c] = np.array([0.5 * float(w4 @ _hamilton_left(Jw[:, k], quat)) for k in range(nd)])
            elif e.what == "axis":  # u = R a: d u = z x u, d2 u / dq_i dq_j = z_i x (z_j x u) for i not after j
                u = np.asarray(evaluate(e, opt, x, p))[:, c]
                w3 = W[:, c]
                for i in range(nd):
                    for j in range(i, nd):
                        S[i, j] = S[j, i] = float(w3 @ np.cross(Jw[:, i], np.cross(Jw[:, j], u)))
                Wq[:, c] = np.array([float(w3 @ np.cross(Jw[:, k], u)) for k in range(nd)])
            else:  # rotation: a single configuration, W is 3 x 3; d R = [omega]x R, d2 R / dq_i dq_j = [z_i x z_j]x R (i < j) + [z_j]x [z_i]x R
                R = np.asarray(evaluate(e, opt, x, p))

                def sk(v):
                    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])

                for i in range(nd):
                    for j in range(i, nd):
                        D2 = sk(Jw[:, j]) @ sk(Jw[:, i]) @ R
                        if i < j:
                            D2 = D2 + sk(np.cross(Jw[:, i], Jw[:, j])) @ R
                        S[i, j] = S[j, i] = float(np.sum(W * D2))
                Wq[:, 0] = np.array([float(np.sum(W * (sk(Jw[:, k]) @ R))) for k in range(nd)])
            Jqc = Jq[c * nd : (c + 1) * nd]
            H += Jqc.T @ S @ Jqc
        if e.q.degree() > 1:
            H += weighted_hessian(e.q, opt, x, p, Wq)
        return H
    raise NotImplementedError(f"no second-derivative rule for {type(e).__name__}")
