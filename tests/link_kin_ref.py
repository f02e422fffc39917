"""Reference for oh_link_kin (kinematics of a link in the frame of a base link), built from the literal oracle: what tests/test_link_kin_cpu.py
and tests/test_gpu_link_kin.py compare against.  Test infrastructure, not product code.

  pos, rot, quat, Jg : OracleRobot.get_link_transform / get_link_quaternion / get_link_geometric_jacobian (optas/models.py:884-898, 1108-1122, 1320-1344)
  rpy                : oracle.spatialmath.Quaternion.fromvec(quat).getrpy()                               (models.py:1167-1177, spatialmath.py:384-404)
  axis               : rot a / |a|                                                                        (models.py:1637-1670)
  Ja                 : rows 0-2 of Jg over d rpy / d q                                                    (models.py:1370-1385, 1590-1611)

The reference differentiates the graph of get_link_rpy with CasADi.  Here the same derivative is the chain rule, factor by factor as the graph is
written: OracleRobot.quaternion_jacobian of link and base, the product quat_L * inv(quat_B) (spatialmath.py:298-328, inv divides by the squared
norm), and the partial derivatives of getrpy, whose constant pitch branch has derivative zero.
"""
import functools

import numpy as np

from conftest import KUKA_KIN, MED7_KIN, SEED, TESTER_KIN
from oracle.robot import OracleRobot
from oracle.spatialmath import Quaternion, unit

KINS = {"kuka": KUKA_KIN, "med7": MED7_KIN, "tester": TESTER_KIN}
# (robot, link, base): a base above and below the link, link chains without joints, a prismatic joint, a constant relative rotation (tester eff / link2)
CASES = [
    ("kuka", "end_effector_ball", "lwr_arm_0_link"),
    ("kuka", "end_effector_ball", "lwr_arm_6_link"),
    ("kuka", "lwr_arm_6_link", "end_effector_ball"),
    ("kuka", "lwr_arm_0_link", "end_effector_ball"),
    ("med7", "lbr_link_ee", "world"),
    ("med7", "lbr_link_ee", "lbr_link_4"),
    ("med7", "lbr_link_4", "lbr_link_ee"),
    ("med7", "world", "lbr_link_ee"),
    ("tester", "eff", "world"),
    ("tester", "eff", "link2"),
    ("tester", "link2", "eff"),
    ("tester", "world", "eff"),
]
AXIS3 = np.array([0.3, -0.2, 0.9])
N_CONFIGS = 40
SINP_MAX = 0.95
TOL = 1e-12  # the project's FK tolerance (tests/test_gpu_fk_jac.py)
TOL_JA = 1e-11  # d rpy / d q: the partial derivatives of getrpy amplify by at most 1 / cos^2(pitch) ~ 10 at |sinp| <= 0.95


@functools.lru_cache(maxsize=None)
def oracle(robot: str) -> OracleRobot:
    return OracleRobot(KINS[robot])


def sinp_of(quat) -> float:
    x, y, z, w = quat
    return 2.0 * (w * y - z * x)  # spatialmath.py:394


def getrpy_partials(quat) -> np.ndarray:
    """d (roll, pitch, yaw) / d (x, y, z, w) of Quaternion.getrpy (spatialmath.py:384-404); atan2(a, b)' = (b a' - a b') / (a^2 + b^2)."""
    x, y, z, w = quat
    G = np.zeros((3, 4))
    a, b = 2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y)
    da, db = np.array([2.0 * w, 2.0 * z, 2.0 * y, 2.0 * x]), np.array([-4.0 * x, -4.0 * y, 0.0, 0.0])
    G[0] = (b * da - a * db) / (a * a + b * b)
    sp = 2.0 * (w * y - z * x)
    if abs(sp) < 1.0:  # the other branch is the constant pi / 2
        G[1] = np.array([-2.0 * z, 2.0 * w, -2.0 * x, 2.0 * y]) / np.sqrt(1.0 - sp * sp)
    c, d = 2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z)
    dc, dd = np.array([2.0 * y, 2.0 * x, 2.0 * w, 2.0 * z]), np.array([0.0, -4.0 * y, -4.0 * z, 0.0])
    G[2] = (d * dc - c * dd) / (c * c + d * d)
    return G


def rpy_jacobian(orc: OracleRobot, link: str, base: str, q) -> np.ndarray:
    """d get_link_rpy / d q (3 x ndof) by the chain rule over the reference's own factors."""
    qL, qB = orc.get_global_link_quaternion(link, q), orc.get_global_link_quaternion(base, q)
    dL, dB = orc.quaternion_jacobian(link, q), orc.quaternion_jacobian(base, q)
    s = float(qB @ qB)
    conj = np.array([-1.0, -1.0, -1.0, 1.0])
    inv_B = conj * qB / s  # spatialmath.py:321-328
    quat = (Quaternion.fromvec(qL) * Quaternion.fromvec(inv_B)).getquat()
    dquat = np.zeros((4, dL.shape[1]))
    for j in range(dL.shape[1]):
        dinv = conj * dB[:, j] / s - conj * qB * (2.0 * float(qB @ dB[:, j])) / (s * s)
        # the product (spatialmath.py:298-312) is bilinear
        dquat[:, j] = (Quaternion.fromvec(dL[:, j]) * Quaternion.fromvec(inv_B)).getquat() + (Quaternion.fromvec(qL) * Quaternion.fromvec(dinv)).getquat()
    return getrpy_partials(quat) @ dquat


def reference(robot: str, link: str, base: str, q, axis3=AXIS3) -> dict:
    """Every output of oh_link_kin for one configuration."""
    orc = oracle(robot)
    q = np.asarray(q, dtype=float).reshape(-1)
    T = orc.get_link_transform(link, q, base)
    quat = orc.get_link_quaternion(link, q, base)
    Jg = orc.get_link_geometric_jacobian(link, q, base)
    return {
        "pos": T[:3, 3].copy(),
        "rot": T[:3, :3].copy(),
        "quat": quat,
        "rpy": Quaternion.fromvec(quat).getrpy(),
        "axis": T[:3, :3] @ unit(axis3),
        "Jg": Jg,
        "Ja": np.vstack([Jg[:3], rpy_jacobian(orc, link, base, q)]),
    }


def reference_batch(robot: str, link: str, base: str, Q, axis3=AXIS3) -> dict:
    """Q: n-by-ndof -> the outputs stacked along a leading axis of n."""
    rows = [reference(robot, link, base, q, axis3) for q in Q]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


@functools.lru_cache(maxsize=None)
def case_inputs(index: int) -> np.ndarray:
    """N_CONFIGS configurations of CASES[index] inside the joint limits clipped to +-3, fixed seed; a draw is kept only if the ORACLE's
    |sinp| <= SINP_MAX there (away from the pitch singularity, where d rpy / d q is unbounded).  n-by-ndof, read-only."""
    robot, link, base = CASES[index]
    orc = oracle(robot)
    lo = np.clip(orc.lower_actuated_joint_limits, -3.0, 3.0)
    up = np.clip(orc.upper_actuated_joint_limits, -3.0, 3.0)
    rng = np.random.default_rng(SEED + 1000 + index)
    kept = []
    while len(kept) < N_CONFIGS:
        q = rng.uniform(lo, up)
        if abs(sinp_of(orc.get_link_quaternion(link, q, base))) <= SINP_MAX:
            kept.append(q)
    Q = np.array(kept)
    Q.setflags(write=False)
    return Q


@functools.lru_cache(maxsize=None)
def case_reference(index: int) -> dict:
    """The reference outputs at case_inputs(index): computed once, shared by the tests, read-only."""
    robot, link, base = CASES[index]
    ref = reference_batch(robot, link, base, case_inputs(index))
    for a in ref.values():
        a.setflags(write=False)
    return ref


def wrap(d):
    """An angle difference in (-pi, pi] (roll and yaw are compared modulo 2 pi)."""
    return np.pi - np.mod(np.pi - d, 2.0 * np.pi)


def assert_outputs_match(got: dict, ref: dict, what: str = "") -> None:
    """The issue's tolerances: 1e-12 everywhere, roll / yaw modulo 2 pi, 1e-11 on rows 3-5 of Ja.  Prints each figure before it asserts."""
    for name in got:
        g, r = np.asarray(got[name]), np.asarray(ref[name])
        assert g.shape == r.shape, f"{what} {name}: shape {g.shape} != {r.shape}"
        if name == "rpy":
            d = g - r
            d[..., 0], d[..., 2] = wrap(d[..., 0]), wrap(d[..., 2])
            errs = [(np.abs(d).max(), TOL, "")]
        elif name == "Ja":
            errs = [(np.abs(g[..., :3, :] - r[..., :3, :]).max(), TOL, " rows 0-2"), (np.abs(g[..., 3:, :] - r[..., 3:, :]).max(), TOL_JA, " rows 3-5")]
        else:
            errs = [(np.abs(g - r).max(), TOL, "")]
        for err, tol, part in errs:
            print(f"{what} {name}{part}: max abs error {err:.3e} (tolerance {tol:g})")
            assert err <= tol, f"{what} {name}{part}: {err:.3e} > {tol:g}"
