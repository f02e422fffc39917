"""Test helper (not collected): the position-plus-link-axis variant of the inverse-kinematics family in numpy.

    min_q  w ||q - qN||^2   s.t.  h(q) = [p_goal - p_link(q); u_goal - u(q)] = 0,   lo <= q <= up,      u(q) = R_link(q) a,  |a| = 1

`solve_axis_ik_al` is oracle/ik_al.py's state machine (what k_ik_axis_solve runs) with six equality rows; `AxisIKNLP` is the literal reference form of
the same problem for kkt_reference_form.  The axis derivatives are written the long way -- the 3 x n Jacobian with columns om_j x u, the curvature
y . (om_a x (om_b x u)) term by term -- not with the identities the kernel uses, so device against port also checks those."""
import numpy as np

from oracle.problems import IKExampleNLP
from oracle.robot import OracleRobot
from oracle.structured import FoldedChain
from pose_ik_ref import _first_then_second, position_curvature


def unit_axis(axis):
    """'x' / 'y' / 'z' or a 3-vector, normalised (the reference's get_link_axis)."""
    a = np.eye(3)["xyz".index(axis)] if isinstance(axis, str) else np.asarray(axis, dtype=np.float64).reshape(3)
    return a / np.linalg.norm(a)


def axis_frames(chain: FoldedChain, a, q):
    """Position, link axis u = R_link a, linear Jacobian (3, n) and joint axes om (n, 3; zero for a prismatic joint)."""
    e, Re, Jp, Jw = chain.jac(np.asarray(q, dtype=np.float64)[None])
    return e[0], Re[0] @ a, Jp[0], np.ascontiguousarray(Jw[0].T)


def axis_jacobian(om, u):
    """(3, n): column j = om_j x u."""
    return np.stack([np.cross(om[j], u) for j in range(len(om))], axis=1)


def axis_curvature(chain: FoldedChain, om, u, y):
    """C[a,b] = sum_k y_k d^2 u_k / dq_a dq_b = y . (om_a x (om_b x u)) for a not after b in chain order (symmetric)."""
    n = len(om)
    M = np.zeros((n, n))
    for a in range(n):
        for b in range(n):
            M[a, b] = y @ np.cross(om[a], np.cross(om[b], u))
    return _first_then_second(chain, M)


def merit_derivatives(chain, w, q, qn, frames, y, rho, hessian=True):
    """Gradient and Hessian in q of w||q - qn||^2 + y . h (+ rho/2 ||h||^2 through y = lam + rho h and the rho J^T J term)."""
    e, u, Jp, om = frames
    J = np.concatenate([Jp, axis_jacobian(om, u)], axis=0)  # (6, n) Jacobian of (p, u); dh/dq = -J
    grad = 2.0 * w * (q - qn) - J.T @ y
    if not hessian:
        return grad, None, J
    H = 2.0 * w * np.eye(chain.ndof) + rho * J.T @ J - position_curvature(chain, Jp, om, y[:3]) - axis_curvature(chain, om, u, y[3:])
    return grad, H, J


def solve_axis_ik_al(chain: FoldedChain, a, x0, qn, pg, ug, lo, up, w=1.0, tol=1e-6, tol_feas=1e-9, max_iter=200, rho0=100.0):
    """Returns dict(x, f, lam_h (6, signed multipliers of the h rows in the reference's v >= 0 form), z_lo, z_up, stationarity, feasibility,
    iterations (kinematics evaluations of accepted + rejected points, plus one for every outer pass that made none), status)."""
    n = chain.ndof
    goal = np.concatenate([pg, ug])
    q = np.minimum(np.maximum(np.asarray(x0, dtype=np.float64), lo), up)
    lam = np.zeros(6)
    rho = rho0
    it = 0
    status = 1

    def value(fr):
        return np.concatenate([fr[0], fr[1]])

    def merit(qq, fr):
        hh = goal - value(fr)
        return w * np.sum((qq - qn) ** 2) + lam @ hh + 0.5 * rho * hh @ hh

    fr = axis_frames(chain, a, q)
    it += 1
    h_prev = np.inf
    shift = 0.0
    if not np.isfinite(merit(q, fr)):
        status = 2
    while it < max_iter and status != 2:
        it_pass = it
        # ---- inner: projected Newton on the augmented Lagrangian ----
        while it < max_iter:
            h = goal - value(fr)
            y = lam + rho * h
            grad, H, _ = merit_derivatives(chain, w, q, qn, fr, y, rho)
            act = ((q <= lo) & (grad > 0.0)) | ((q >= up) & (grad < 0.0))
            pgn = np.max(np.abs(np.where(act, 0.0, grad)))
            if pgn <= max(tol * 0.5, min(1e-2, 0.1 * np.abs(h).max())):
                break
            free = ~act
            while True:
                Hs = H + shift * np.eye(n)
                Hs[act, :] = 0.0
                Hs[:, act] = 0.0
                Hs[act, act] = 1.0
                try:
                    L = np.linalg.cholesky(Hs)
                    break
                except np.linalg.LinAlgError:
                    shift = max(10.0 * shift, 1e-3 * rho)
            d = -np.linalg.solve(L.T, np.linalg.solve(L, np.where(free, grad, 0.0)))
            m0 = merit(q, fr)
            alpha = 1.0
            ok = False
            for _ in range(30):
                qt = np.minimum(np.maximum(q + alpha * d, lo), up)
                frt = axis_frames(chain, a, qt)
                it += 1
                if merit(qt, frt) <= m0 + 1e-4 * grad @ (qt - q) + 4e-16 * max(1.0, abs(m0)) + 8e-16 * np.abs(y).sum():
                    ok = True
                    break
                alpha *= 0.5
                if it >= max_iter:
                    break
            if not ok:
                shift = max(10.0 * shift, 1e-3 * rho)
                if shift > 1e12 * rho:
                    status = 2
                    break
                continue
            shift *= 0.1 if shift > 1e-12 else 0.0
            q, fr = qt, frt
        if status == 2:
            break
        # ---- outer: multiplier update ----
        h = goal - value(fr)
        lam = lam + rho * h
        hn = np.abs(h).max()
        grad, _, _ = merit_derivatives(chain, w, q, qn, fr, lam, 0.0, hessian=False)
        act = ((q <= lo) & (grad > 0.0)) | ((q >= up) & (grad < 0.0))
        stat = np.max(np.abs(np.where(act, 0.0, grad)))
        if hn <= tol_feas and stat <= tol:
            status = 0
            break
        if hn > 0.1 * h_prev:
            rho = min(rho * 10.0, 1e8)
        h_prev = hn
        if it == it_pass:  # a pass without an evaluation counts as one towards the cap (k_ik_axis_solve: such passes only grow lam)
            it += 1
    h = goal - value(fr)
    grad, _, _ = merit_derivatives(chain, w, q, qn, fr, lam, 0.0, hessian=False)
    at_lo, at_up = (q <= lo) & (grad > 0.0), (q >= up) & (grad < 0.0)
    z_lo, z_up = np.where(at_lo, grad, 0.0), np.where(at_up, -grad, 0.0)
    stat = np.max(np.abs(np.where(at_lo | at_up, 0.0, grad)))
    return dict(x=q, f=float(w * np.sum((q - qn) ** 2)), lam_h=-lam, z_lo=z_lo, z_up=z_up, stationarity=float(stat),
                feasibility=float(np.abs(h).max()), iterations=it, status=status)


class AxisIKNLP(IKExampleNLP):
    """examples/axis_ik.py in the reference's form: x = q; p = [q_nominal (n); p_goal (3); axis_goal (3)]; f = ||q - qn||^2;
    h = [p_goal - p_link(q); axis_goal - R_link(q) a] (builder.py:354: rhs - lhs, both equalities); k = [q - lo; up - q]."""

    def __init__(self, robot: OracleRobot, link="end_effector_ball", axis="z"):
        super().__init__(robot, link)
        self.np_, self.nh = self.n + 6, 6
        self.axis = unit_axis(axis)  # (not `a`: that is the reference's linear-equality member)

    def u(self, x):
        return np.asarray(self.robot.get_global_link_rotation(self.link, x), dtype=np.float64).reshape(3, 3) @ self.axis

    def h(self, x, p):
        n = self.n
        return np.concatenate([p[n : n + 3] - np.asarray(self.robot.get_global_link_position(self.link, x)).reshape(3), p[n + 3 :] - self.u(x)])

    def dh(self, x, p):
        Jw = np.asarray(self.robot.get_global_link_angular_geometric_jacobian(self.link, x), dtype=np.float64)
        u = self.u(x)
        return -np.concatenate([np.asarray(self.robot.get_global_link_linear_jacobian(self.link, x), dtype=np.float64),
                                np.stack([np.cross(Jw[:, j], u) for j in range(self.n)], axis=1)], axis=0)


def kuka_batch(rng, chain: FoldedChain, a, B: int, nominal, lo, up):
    """The distribution of test_gpu_ik.test_large_batch_properties with a link axis: qn = nominal + U(+-0.3), goal = position and axis at clip(qn + U(+-0.5))."""
    n = len(nominal)
    qn = nominal + rng.uniform(-0.3, 0.3, (B, n))
    qgoal = np.clip(qn + rng.uniform(-0.5, 0.5, (B, n)), lo, up)
    pg, Re, _, _ = chain.fk(qgoal)
    return qn, pg, Re @ a
