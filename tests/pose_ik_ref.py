"""Test helper (not collected): the full-pose variant of the inverse-kinematics family in numpy.

    min_q  w ||q - qN||^2   s.t.  h(q) = [p_goal - p_link(q); quat_goal - quat_link(q)] = 0,   lo <= q <= up

`solve_pose_ik_al` is oracle/ik_al.py's iteration (solve_rows_al: what the kernel runs) on `PoseRows`, seven equality rows; `PoseIKNLP` is the literal reference
form of the same problem for kkt_reference_form; `slsqp_six_rows` is the independent solver on the six-row (minimal) form of the pose error.
The quaternion derivatives here are written the long way -- Jq_j = 1/2 (om_j, 0) (x) quat as a 4 x n matrix, d2quat = 1/4 (om_a, 0) (x) (om_b, 0) (x) quat
term by term -- not with the identities the kernel uses, so the comparison also checks those."""
import numpy as np

from oracle.ik_al import solve_rows_al
from oracle.problems import IKExampleNLP, _hamilton_left_pure
from oracle.robot import OracleRobot
from oracle.structured import FoldedChain


def _hlp(O, V):
    """(o, 0) (x) v, Hamilton product in xyzw storage, over leading axes: O (..., 3), V (..., 4) -> (..., 4) (oracle.problems._hamilton_left_pure, batched)."""
    ox, oy, oz = O[..., 0], O[..., 1], O[..., 2]
    x, y, z, w = V[..., 0], V[..., 1], V[..., 2], V[..., 3]
    return np.stack([ox * w + oy * z - oz * y, -ox * z + oy * w + oz * x, ox * y - oy * x + oz * w, -ox * x - oy * y - oz * z], axis=-1)


class _QuatChain:
    """OracleRobot.quaternion_batch for one link with the chain's constants looked up once (the same products in the same order: equal bit for bit,
    tests/test_pose_ik_cpu.py); the port evaluates it some twenty times per instance."""

    @classmethod
    def of(cls, robot: OracleRobot, link: str):
        made = robot.__dict__.setdefault("_pose_ik_quat_chains", {})
        if link not in made:
            made[link] = cls(robot, link)
        return made[link]

    def __init__(self, robot: OracleRobot, link: str):
        from oracle.spatialmath import Quaternion, unit

        self.steps = []  # (fixed-rotation quaternion, actuated index or None, unit axis)
        root = robot.get_root()
        for name in (robot.get_chain(root, link) if link != root else []):
            joint = robot.joint_map[name]
            _, rpy = robot.get_joint_origin(joint)
            spins = joint.type in {"revolute", "continuous"}
            self.steps.append((tuple(Quaternion.fromrpy(rpy).getquat()), robot.get_actuated_joint_index(joint.name) if spins else None,
                               unit(robot.get_joint_axis(joint)) if spins else None))

    @staticmethod
    def _mul(a, b):  # Quaternion.__mul__ (spatialmath.py:298-312): self = a, quat = b
        x0, y0, z0, w0 = a
        x1, y1, z1, w1 = b
        return (x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0, -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0, x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0, -x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0)

    def __call__(self, q):
        quat = (0.0, 0.0, 0.0, 1.0)
        for fixed, idx, ax in self.steps:
            quat = self._mul(fixed, quat)
            if idx is not None:
                s = np.sin(0.5 * q[idx])
                quat = self._mul((s * ax[0], s * ax[1], s * ax[2], np.cos(0.5 * q[idx])), quat)
        return np.array(quat, dtype=np.float64)


def pose_frames(robot: OracleRobot, link: str, chain: FoldedChain, q):
    """Position, reference-signed chain quaternion, linear Jacobian (3, n) and angular rates om (n, 3; zero for a prismatic joint)."""
    q = np.asarray(q, dtype=np.float64)
    e, _, Jp, Jw = chain.jac(q[None])
    return e[0], _QuatChain.of(robot, link)(q), Jp[0], np.ascontiguousarray(Jw[0].T)


def quaternion_jacobian(om, quat):
    """(4, n): column j = 1/2 (om_j, 0) (x) quat."""
    return 0.5 * _hlp(om, quat).T


def _chain_rank(chain: FoldedChain):
    rank = np.full(chain.ndof, chain.ndof)
    for k in range(chain.n_chain):
        rank[chain.qidx[k]] = k
    return rank


def _first_then_second(chain, M):
    """Symmetric matrix whose (a, b) entry is M[a, b] where a is not after b in chain order."""
    rank = _chain_rank(chain)
    return np.where(rank[:, None] <= rank[None, :], M, M.T)


def quaternion_curvature(chain: FoldedChain, om, quat, y):
    """C[a,b] = sum_k y_k d^2 quat_k / dq_a dq_b = y . 1/4 (om_a, 0) (x) (om_b, 0) (x) quat for a not after b in chain order (symmetric)."""
    X = _hlp(om, quat)  # (n, 4): (om_b, 0) (x) quat
    return _first_then_second(chain, 0.25 * _hlp(om[:, None, :], X[None, :, :]) @ y)


def position_curvature(chain: FoldedChain, Jp, om, y):
    """oracle.ik_al.position_curvature without the loop: C[a,b] = y . (om_a x Jp_b) = (y x om_a) . Jp_b for a not after b in chain order."""
    return _first_then_second(chain, np.cross(y[None, :], om) @ Jp)


def merit_derivatives(chain, w, q, qn, goal, frames, y, rho, hessian=True):
    """Gradient and Hessian in q of w||q - qn||^2 + y . h (+ rho/2 ||h||^2 through y = lam + rho h and the rho J^T J term)."""
    e, quat, Jp, om = frames
    J = np.concatenate([Jp, quaternion_jacobian(om, quat)], axis=0)  # (7, n) Jacobian of (p, quat); dh/dq = -J
    grad = 2.0 * w * (q - qn) - J.T @ y
    if not hessian:
        return grad, None, J
    # h = goal - value: both curvature terms enter with the minus sign
    H = 2.0 * w * np.eye(chain.ndof) + rho * J.T @ J - position_curvature(chain, Jp, om, y[:3]) - quaternion_curvature(chain, om, quat, y[3:])
    return grad, H, J


class PoseRows:
    """Rows of the full-pose goal for oracle.ik_al.solve_rows_al: value = [p_link; quat_link], seven rows, derivatives the long way (merit_derivatives)."""

    idle_pass_counts = False

    def __init__(self, robot: OracleRobot, link: str, chain: FoldedChain):
        self.robot, self.link, self.chain = robot, link, chain

    def frames(self, q):
        return pose_frames(self.robot, self.link, self.chain, q)

    def value(self, frames):
        return np.concatenate([frames[0], frames[1]])

    def merit_derivatives(self, w, q, qn, frames, y, rho, hessian=True):
        return merit_derivatives(self.chain, w, q, qn, None, frames, y, rho, hessian)[:2]


def solve_pose_ik_al(robot: OracleRobot, link: str, chain: FoldedChain, x0, qn, pg, qg, lo, up, w=1.0, tol=1e-6, tol_feas=1e-9, max_iter=200, rho0=100.0):
    """Returns dict(x, f, lam_h (7, signed multipliers of the h rows in the reference's v >= 0 form), z_lo, z_up, stationarity, feasibility,
    iterations (kinematics evaluations of accepted + rejected points), status)."""
    return solve_rows_al(PoseRows(robot, link, chain), x0, qn, np.concatenate([pg, qg]), lo, up, w, tol, tol_feas, max_iter, rho0)


class PoseIKNLP(IKExampleNLP):
    """examples/pose_ik.py in the reference's form: x = q; p = [q_nominal (n); p_goal (3); quat_goal (4)]; f = ||q - qn||^2;
    h = [p_goal - p_link(q); quat_goal - quat_link(q)] (builder.py:354: rhs - lhs, both equalities); k = [q - lo; up - q]."""

    def __init__(self, robot: OracleRobot, link="end_effector_ball"):
        super().__init__(robot, link)
        self.np_, self.nh = self.n + 7, 7

    def h(self, x, p):
        n = self.n
        return np.concatenate([p[n : n + 3] - self.robot.get_global_link_position(self.link, x), p[n + 3 :] - self.robot.get_global_link_quaternion(self.link, x)])

    def dh(self, x, p):
        return -np.concatenate([self.robot.get_global_link_linear_jacobian(self.link, x), self.robot.quaternion_jacobian(self.link, x)], axis=0)


def qmul_xyzw(a, b):
    """Hamilton product a (x) b, xyzw."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def slsqp_six_rows(nlp: PoseIKNLP, chain: FoldedChain, x0, p, lo, up):
    """scipy SLSQP on the minimal form of the same problem: [p_goal - p; 2 vec(conj(quat_goal) (x) quat(q))] = 0 with the bounds.
    Returns (result, violation of the six rows at result.x)."""
    from scipy.optimize import minimize

    n = nlp.n
    conj = np.array([-1.0, -1.0, -1.0, 1.0]) * p[n + 3 :]

    def rows(x):
        return np.concatenate([p[n : n + 3] - chain.fk(x[None])[0][0], 2.0 * qmul_xyzw(conj, nlp.robot.quaternion_batch(nlp.link, x[None])[0])[:3]])

    def jac(x):
        _, _, Jp, Jw = chain.jac(x[None])
        quat = nlp.robot.quaternion_batch(nlp.link, x[None])[0]
        return np.concatenate([-Jp[0], np.stack([qmul_xyzw(conj, _hamilton_left_pure(Jw[0][:, j], quat))[:3] for j in range(n)], axis=1)], axis=0)

    r = minimize(lambda x: nlp.f(x, p), x0, jac=lambda x: nlp.df(x, p), method="SLSQP", bounds=list(zip(lo, up)), constraints=[{"type": "eq", "fun": rows, "jac": jac}],
                 tol=1e-12, options={"maxiter": 100})
    return r, float(np.abs(rows(r.x)).max())


def kuka_batch(rng, chain: FoldedChain, robot: OracleRobot, link: str, B: int, nominal, lo, up):
    """The distribution of test_gpu_ik.test_large_batch_properties with an orientation: qn = nominal + U(+-0.3), goal = pose at clip(qn + U(+-0.5))."""
    n = len(nominal)
    qn = nominal + rng.uniform(-0.3, 0.3, (B, n))
    qgoal = np.clip(qn + rng.uniform(-0.5, 0.5, (B, n)), lo, up)
    pg, _, _, _ = chain.fk(qgoal)
    return qn, pg, robot.quaternion_batch(link, qgoal)
