"""Test helper (not collected): the position-plus-link-axis variant of the inverse-kinematics family in numpy.

    min_q  w ||q - qN||^2   s.t.  h(q) = [p_goal - p_link(q); u_goal - u(q)] = 0,   lo <= q <= up,      u(q) = R_link(q) a,  |a| = 1

`solve_axis_ik_al` is oracle/ik_al.py's iteration (solve_rows_al: what the kernel runs) on `AxisRows`, six equality rows; `AxisIKNLP` is the literal reference form of
the same problem for kkt_reference_form.  The axis derivatives are written the long way -- the 3 x n Jacobian with columns om_j x u, the curvature
y . (om_a x (om_b x u)) term by term -- not with the identities the kernel uses, so device against port also checks those."""
import numpy as np

from oracle.ik_al import solve_rows_al
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


class AxisRows:
    """Rows of the position-plus-axis goal for oracle.ik_al.solve_rows_al: value = [p_link; R_link a], six rows, derivatives the long way
    (merit_derivatives).  A pass without an evaluation counts as one towards the cap (IkAxisRows in oh_ik.hip: such passes only grow lam)."""

    idle_pass_counts = True

    def __init__(self, chain: FoldedChain, a):
        self.chain, self.a = chain, a

    def frames(self, q):
        return axis_frames(self.chain, self.a, q)

    def value(self, frames):
        return np.concatenate([frames[0], frames[1]])

    def merit_derivatives(self, w, q, qn, frames, y, rho, hessian=True):
        return merit_derivatives(self.chain, w, q, qn, frames, y, rho, hessian)[:2]


def solve_axis_ik_al(chain: FoldedChain, a, x0, qn, pg, ug, lo, up, w=1.0, tol=1e-6, tol_feas=1e-9, max_iter=200, rho0=100.0):
    """Returns dict(x, f, lam_h (6, signed multipliers of the h rows in the reference's v >= 0 form), z_lo, z_up, stationarity, feasibility,
    iterations (kinematics evaluations of accepted + rejected points, plus one for every outer pass that made none), status)."""
    return solve_rows_al(AxisRows(chain, a), x0, qn, np.concatenate([pg, ug]), lo, up, w, tol, tol_feas, max_iter, rho0)


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
