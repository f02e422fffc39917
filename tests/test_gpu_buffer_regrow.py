"""Buffers of a handle that grow between calls (csrc/oh_api.hip: DevBuf members, pools and staging areas laid out by the lists of oh_carve.h).
One handle solves B = 96, then 320, then 96 again; every call must equal, bit for bit, a fresh handle that solves that batch alone: x, f, kkt,
iters, status and the multipliers.  The host-staged entry points are called with array sizes that are no multiple of 256 bytes after a larger call
on the same handle, and compared with the same call on a fresh handle."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, KUKA_KIN, MED7_KIN, SEED
from optas_amd import _lib
from optas_amd.backend import FigureEightBackend, IKBackend, PointMassBackend, QPBackend, TapeBackend, TorqueBackend
from optas_amd.models import KinematicsHandle, LinkFrameHandle, RobotModel
from tape_cases import B as TapeLines

pytestmark = pytest.mark.gpu
SIZES = (96, 320, 96)
LINK = "end_effector_ball"
TESTER_REV_KIN = os.path.join(GOLDEN, "tester_robot_revolute.kin.json")
ADD, SUB, MUL = 3, 4, 5


def _bits(be, x0, p, B, mult):
    r = be.solve(x0[:B], p[:B])
    return [r.x, r.f, r.kkt, r.iters, r.status] + [np.asarray(m) for m in mult(be, B)]


def _assert_same(got, want, what):
    names = ["x", "f", "kkt", "iters", "status"] + [f"multipliers[{i}]" for i in range(len(got) - 5)]
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {name} differs from a fresh handle's"


def _regrow(make, x0, p, mult, what):
    """make() -> a fresh handle.  The handle that went through SIZES is returned open."""
    fresh = {}
    for B in sorted(set(SIZES)):
        be = make()
        fresh[B] = _bits(be, x0, p, B, mult)
        be.close()
    assert _lib.status_ok(fresh[SIZES[1]][4]).mean() >= 0.5, f"{what}: most of the batch is meant to converge"  # (what is compared are real solves)
    be = make()
    for k, B in enumerate(SIZES):
        _assert_same(_bits(be, x0, p, B, mult), fresh[B], f"{what}, call {k} (B = {B})")
    return be


def _traj_inputs(B, T, seed):
    rng = np.random.default_rng(seed)
    qc = np.deg2rad([0, 30, 0, -90, 0, 60, 0])[None, :] + rng.uniform(-0.1, 0.1, (B, 7))
    x0 = np.concatenate([np.repeat(qc, T, axis=0).reshape(B, 7 * T), np.zeros((B, 7 * (T - 1)))], axis=1)
    return x0, qc


def _path(T):
    t = np.linspace(0.0, 1.0, T)
    return np.stack([0.05 * np.sin(2 * np.pi * t), 0.05 * (1 - np.cos(2 * np.pi * t)), 0.03 * t], axis=1)


def _one(be, B):
    return [be.multipliers(B)]


def test_orientation_locked_trajectory(hip_lib):
    T = 5
    chain = RobotModel(urdf_filename=KUKA_KIN).kinematic_chain(LINK)
    x0, qc = _traj_inputs(max(SIZES), T, SEED + 201)
    make = lambda: FigureEightBackend(chain, T, 0.1, _path(T), max_iter=300, tol=1e-6).set_options(batch_invariant=1)
    _regrow(make, x0, qc, _one, "orientation-locked").close()


def _guards(vel):
    g = _lib.oh_guards()
    g.limits = 1
    for j in range(7):
        g.q_lo[j], g.q_up[j] = -2.9, 2.9
    g.vel_limits = 1 if vel else 0
    for j in range(7):
        g.dq_lo[j], g.dq_up[j] = -0.8, 0.8
    return g


def test_position_tracking_with_guards_set_twice(hip_lib):
    T = 5
    chain = RobotModel(urdf_filename=KUKA_KIN).kinematic_chain(LINK)
    x0, qc = _traj_inputs(max(SIZES), T, SEED + 202)

    def make(g):
        return lambda: FigureEightBackend(chain, T, 0.1, _path(T), w_path=100.0, w_vel=0.01, max_iter=600, tol=1e-6, hessian=0, lock_orientation=False, fix_dq0=False,
                                          path_in_frame=False, guards=g).set_options(batch_invariant=1)

    both, limits = _guards(True), _guards(False)
    be = _regrow(make(both), x0, qc, _one, "limit + velocity rows")
    # another row count on the handle that has grown: the guard pool is dropped and carved again
    _lib.check(_lib.load().oh_set_guards(be.handle, C.byref(limits)), "oh_set_guards")
    be.guards, be.n_rows = limits, 14
    fresh = {}
    for B in sorted(set(SIZES)):
        other = make(limits)()
        fresh[B] = _bits(other, x0, qc, B, _one)
        other.close()
    for k, B in enumerate(SIZES):
        _assert_same(_bits(be, x0, qc, B, _one), fresh[B], f"limit rows after oh_set_guards, call {k} (B = {B})")
    be.close()


def _tester_robot():
    return RobotModel(urdf_filename=TESTER_REV_KIN, time_derivs=[0, 1, 2])


def _torque_backend(robot, T):
    return TorqueBackend(robot.kinematic_chain("eff"), robot.dynamics_tables(), T=T, dt=0.1, w_path=1000.0, w_vel=0.1, w_tau=1e-4, tau_lo=-1e3, tau_up=1e3)


def _torque_goals(robot, qc, rows):
    """(B, rows, 3): a small loop around each plant's own end-effector position"""
    pos = KinematicsHandle(robot.kinematic_chain("eff")).fk_jac(qc, want_jac=False)[0][:, :3]
    ts = np.arange(rows) * 0.1
    return pos[:, None, :] + 0.02 * np.stack([np.sin(ts * np.pi * 0.5), np.sin(ts * np.pi), np.zeros(rows)], axis=1)[None]


def test_torque_mpc(hip_lib):
    T, n = 4, 2
    robot = _tester_robot()
    B = max(SIZES)
    rng = np.random.default_rng(SEED + 203)
    qc = np.array([0.4, -0.3]) + rng.uniform(-0.1, 0.1, (B, n))
    x0 = np.concatenate([np.tile(qc, (1, T)), np.zeros((B, 3 * T * n))], axis=1)
    p = np.concatenate([qc, np.zeros((B, n)), _torque_goals(robot, qc, T).reshape(B, -1)], axis=1)
    _regrow(lambda: _torque_backend(robot, T), x0, p, _one, "torque MPC").close()


def _pm_parameters(B, T, seed):
    rng = np.random.default_rng(seed)
    curr = np.array([-0.9, 0.4]) + rng.uniform(-0.05, 0.05, (B, 2))
    ob = np.array([[0.15 * np.sin(np.pi * (0.05 * t) - np.pi), 0.15 * np.cos(np.pi * (0.05 * t) - np.pi) + 0.15] for t in range(T)])  # (T, 2)
    ramp = np.arange(T) / (T - 1.0)
    goal = np.clip(curr[:, None, :] + (1 - curr[:, None, :]) * ramp[None, :, None], -1.5, 1.5)  # (B, T, 2)
    return np.concatenate([curr, np.zeros((B, 2)), goal.reshape(B, -1), np.tile(ob.reshape(-1), (B, 1))], axis=1)


def test_point_mass(hip_lib):
    T = 4
    B = max(SIZES)
    _regrow(lambda: PointMassBackend(T=T, tol=1e-8), np.zeros((B, 4 * T)), _pm_parameters(B, T, SEED + 204), lambda be, n: [], "point mass").close()


def test_ik(hip_lib):
    robot = RobotModel(urdf_filename=KUKA_KIN)
    chain = robot.kinematic_chain(LINK)
    lo, up = np.asarray(robot.lower_actuated_joint_limits).reshape(-1), np.asarray(robot.upper_actuated_joint_limits).reshape(-1)
    B = max(SIZES)
    rng = np.random.default_rng(SEED + 205)
    qn = np.deg2rad([0, 30, 0, -90, 0, 60, 0])[None, :] + rng.uniform(-0.2, 0.2, (B, 7))
    goal = KinematicsHandle(chain).fk_jac(qn + rng.uniform(-0.15, 0.15, (B, 7)), want_jac=False)[0][:, :3]
    _regrow(lambda: IKBackend(chain, lo, up), qn, np.concatenate([qn, goal], axis=1), lambda be, n: list(be.multipliers(n)), "IK").close()


def _qp_batch(n, m, me, B, seed):
    """Packed [P | q | M | c | A | b] of B strictly convex QPs with a planted feasible point (the slacks at it are positive)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        G = rng.uniform(-1.0, 1.0, (n, n))
        P = 0.5 * G @ G.T + np.eye(n)
        M, A, xs = rng.uniform(-1.0, 1.0, (m, n)), rng.uniform(-1.0, 1.0, (me, n)), rng.uniform(-1.0, 1.0, n)
        out.append(QPBackend.pack(P, rng.uniform(-1.0, 1.0, n), M, rng.uniform(0.0, 0.5, m) - M @ xs, A, -A @ xs))
    return np.stack(out)


def _qp_tape(n, m, me, scale):
    """f = sum_i (1 + i / 4) scale x_i^2 + p_0 x_0 + x_1 x_2 / 4;  rows k: x_k + x_{k+1} + 1 + p_1 >= 0;  rows a: x_a - scale x_{n-1-a} + p_0 = 0."""
    t = TapeLines()
    x, p = [t.x(i) for i in range(n)], [t.p(0), t.p(1)]
    f = t.emit(MUL, p[0], x[0])
    for i in range(n):
        f = t.emit(ADD, f, t.emit(MUL, t.const((1 + i / 4.0) * scale), t.emit(MUL, x[i], x[i])))
    f = t.emit(ADD, f, t.emit(MUL, t.const(0.25), t.emit(MUL, x[1], x[2])))
    rows = [t.emit(ADD, t.emit(ADD, x[k % n], x[(k + 1) % n]), t.emit(ADD, t.const(1.0), p[1])) for k in range(m)]
    rows += [t.emit(ADD, t.emit(SUB, x[a], t.emit(MUL, t.const(scale), x[n - 1 - a])), p[0]) for a in range(me)]
    return t.tape(f, rows, m, me, n, 2)


def _two(be, B):
    return list(be.multipliers(B))


@pytest.mark.parametrize("n,m,me,block", [(4, 6, 1, 0), (40, 8, 2, 1)], ids=["lane-kernel", "block-kernel"])
def test_dense_qp_packed_and_with_its_tape_set_twice(hip_lib, n, m, me, block):
    B = max(SIZES)
    x0 = np.zeros((B, n))
    be = _regrow(lambda: QPBackend(n, m, me), x0, _qp_batch(n, m, me, B, SEED + 206 + n), _two, f"QP n = {n}")
    assert be.flag("qp_block") == block
    # the data read off a tape on the device; a second tape on the grown handle drops the register file of the first
    p = np.random.default_rng(SEED + 207).uniform(-0.5, 0.5, (B, 2))
    for scale in (1.0, 0.5):
        tape = _qp_tape(n, m, me, scale)
        be.set_tape(tape)
        fresh = {}
        for Bk in sorted(set(SIZES)):
            other = QPBackend(n, m, me, tape=tape)
            fresh[Bk] = _bits(other, x0, p, Bk, _two)
            other.close()
        for k, Bk in enumerate(SIZES):
            _assert_same(_bits(be, x0, p, Bk, _two), fresh[Bk], f"QP n = {n} with tape (scale {scale}), call {k} (B = {Bk})")
    be.close()


def test_tape_interpreter(hip_lib):
    """min (x0 - p0)^2 + (x1 - p1)^2 + x2^2 + x0 x1 / 2   s.t.  x0 + x1 - 1/2 >= 0,  x2 - x0 = 0  (thread-per-instance interpreter: jit = False)"""
    t = TapeLines()
    x, p = [t.x(i) for i in range(3)], [t.p(0), t.p(1)]
    d0, d1 = t.emit(SUB, x[0], p[0]), t.emit(SUB, x[1], p[1])
    f = t.emit(ADD, t.emit(ADD, t.emit(MUL, d0, d0), t.emit(MUL, d1, d1)), t.emit(ADD, t.emit(MUL, x[2], x[2]), t.emit(MUL, t.const(0.5), t.emit(MUL, x[0], x[1]))))
    rows = [t.emit(SUB, t.emit(ADD, x[0], x[1]), t.const(0.5)), t.emit(SUB, x[2], x[0])]
    tape = t.tape(f, rows, 1, 1, 3, 2)
    B = max(SIZES)
    rng = np.random.default_rng(SEED + 208)
    be = _regrow(lambda: TapeBackend(tape, tol=1e-7, jit=False), rng.uniform(-0.2, 0.2, (B, 3)), rng.uniform(-1.0, 1.0, (B, 2)), _two, "tape")
    assert not be.jit and not be.wave
    be.close()


# ---- host-staged entry points: sizes that are no multiple of 256 bytes, after a larger call on the same handle ------------------------------------


def _equal(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_fk_jac_33_after_200(hip_lib):
    chain = RobotModel(urdf_filename=KUKA_KIN).kinematic_chain(LINK)
    Q = np.random.default_rng(SEED + 209).uniform(-1.5, 1.5, (200, 7))
    grown, fresh = KinematicsHandle(chain), KinematicsHandle(chain)
    big = grown.fk_jac(Q)
    for got, want, ref in zip(grown.fk_jac(Q[:33]), fresh.fk_jac(Q[:33]), big):
        assert _equal(got, want) and _equal(got, ref[:33])


def test_link_kin_pos_and_Ja_33_after_all_outputs_200(hip_lib):
    robot = RobotModel(urdf_filename=KUKA_KIN)
    link, base = robot.kinematic_chain(LINK), robot.kinematic_chain("lwr_arm_3_link")
    Q = np.random.default_rng(SEED + 210).uniform(-1.5, 1.5, (200, 7))
    grown, fresh = LinkFrameHandle(link, base), LinkFrameHandle(link, base)
    big = grown.link_kin(Q, list(LinkFrameHandle.OUTPUTS), axis3=[0.0, 0.6, 0.8])
    got, want = grown.link_kin(Q[:33], ["pos", "Ja"]), fresh.link_kin(Q[:33], ["pos", "Ja"])
    for k in ("pos", "Ja"):
        assert _equal(got[k], want[k]) and _equal(got[k], big[k][:33])


def test_rnea_hess_33_after_200(hip_lib):
    lib = _lib.load()
    dyn = RobotModel(urdf_filename=MED7_KIN).dynamics_tables()
    nd = dyn.ndof
    A = [np.ascontiguousarray(a) for a in np.random.default_rng(SEED + 211).uniform(-1.0, 1.0, (4, 200, nd))]

    def hess(h, n):
        out = np.empty((n, 3 * nd, 3 * nd))
        _lib.check(lib.oh_rnea_hess(h, n, *[_lib._ptr(np.ascontiguousarray(a[:n])) for a in A], _lib._ptr(out)), "oh_rnea_hess")
        return out

    hs = []
    for _ in range(2):
        h = C.c_void_p()
        _lib.check(lib.oh_create(C.byref(_lib.oh_problem_desc(kind=_lib.OH_PROBLEM_KINEMATICS, ndof=nd)), C.byref(h)), "oh_create")
        _lib.check(lib.oh_set_dynamics(h, C.byref(dyn)), "oh_set_dynamics")
        hs.append(h)
    big = hess(hs[0], 200)
    got, want = hess(hs[0], 33), hess(hs[1], 33)
    assert _equal(got, want) and _equal(got, big[:33])
    for h in hs:
        lib.oh_destroy(h)


def test_rollouts_of_two_ticks_after_longer_ones(hip_lib):
    T = 4
    state0 = np.concatenate([np.array([-0.9, 0.4]) + np.random.default_rng(SEED + 212).uniform(-0.05, 0.05, (40, 2)), np.zeros((40, 2))], axis=1)
    tab = np.array([[0.15 * np.sin(np.pi * (0.05 * t) - np.pi), 0.15 * np.cos(np.pi * (0.05 * t) - np.pi) + 0.15] for t in range(4 * 2 + T)])
    grown, fresh = PointMassBackend(T=T, tol=1e-8), PointMassBackend(T=T, tol=1e-8)
    grown.rollout(state0, tab, 4)
    for got, want in zip(grown.rollout(state0[:5], tab, 2), fresh.rollout(state0[:5], tab, 2)):
        assert _equal(got, want)
    grown.close(), fresh.close()
    robot = _tester_robot()
    qc = np.array([0.4, -0.3]) + np.random.default_rng(SEED + 213).uniform(-0.1, 0.1, (40, 2))
    s0, goals = np.concatenate([qc, np.zeros((40, 2))], axis=1), _torque_goals(robot, qc, 4 + T)
    grown, fresh = _torque_backend(robot, T), _torque_backend(robot, T)
    grown.rollout(s0, goals, 4)
    for got, want in zip(grown.rollout(s0[:5], np.ascontiguousarray(goals[:5, : 2 + T]), 2), fresh.rollout(s0[:5], np.ascontiguousarray(goals[:5, : 2 + T]), 2)):
        assert _equal(got, want)
    grown.close(), fresh.close()
