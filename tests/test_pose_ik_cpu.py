"""Full-pose inverse kinematics without a GPU: the numpy port of the state machine k_ik_pose_solve runs (tests/pose_ik_ref.py) -- its derivatives
against central differences, its convergence with and without active limits, its optima against scipy SLSQP on the six-row form of the pose
error -- and the lowering of the builder's problem (examples/pose_ik.py) to the IK family."""
import os
import sys

import numpy as np
import pytest

from conftest import KUKA_KIN, SEED, TESTER_KIN
from oracle.robot import OracleRobot
from oracle.structured import FoldedChain
from oracle.ik_al import position_curvature as oracle_position_curvature
from pose_ik_ref import PoseIKNLP, kuka_batch, merit_derivatives, pose_frames, position_curvature, quaternion_curvature, quaternion_jacobian, slsqp_six_rows, solve_pose_ik_al

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from examples import example, pose_ik  # noqa: E402
from optas_amd import _lib  # noqa: E402
from optas_amd.builder import OptimizationBuilder  # noqa: E402
from optas_amd.expr import sumsqr  # noqa: E402
from optas_amd.lowering import IkSpec, LoweringError, lower, match_ik  # noqa: E402

LINK = "end_effector_ball"
NOMINAL = np.deg2rad([0, 45, 0, -90, 0, -45, 0])


@pytest.fixture(scope="module")
def kuka():
    orc = OracleRobot(KUKA_KIN)
    return orc, FoldedChain(orc, LINK), PoseIKNLP(orc, LINK)


def _central(fun, q, h=1e-5):
    cols = []
    for j in range(len(q)):
        d = np.zeros(len(q))
        d[j] = h
        cols.append((fun(q + d) - fun(q - d)) / (2.0 * h))
    return np.stack(cols, axis=-1)


def _check_derivatives(orc, link, ch, q, rng):
    quat_of = lambda x: orc.quaternion_batch(link, x[None])[0]
    _, quat, Jp, om = pose_frames(orc, link, ch, q)
    Jq = quaternion_jacobian(om, quat)
    assert np.abs(Jq - _central(quat_of, q)).max() <= 1e-8
    assert np.abs(Jq - orc.quaternion_jacobian(link, q)).max() <= 1e-14
    assert (quat == quat_of(q)).all()  # the helper's cached chain walk is quaternion_batch's
    yp = rng.uniform(-1.0, 1.0, 3)
    assert np.abs(position_curvature(ch, Jp, om, yp) - oracle_position_curvature(ch, Jp, om, yp)).max() <= 1e-15
    y = rng.uniform(-1.0, 1.0, 4)
    jty = lambda x: quaternion_jacobian(pose_frames(orc, link, ch, x)[3], quat_of(x)).T @ y
    C = quaternion_curvature(ch, om, quat, y)
    assert np.abs(C - _central(jty, q)).max() <= 1e-8
    assert np.abs(np.diag(C) + 0.25 * (y @ quat) * np.sum(om * om, axis=1)).max() <= 1e-15  # a = b: -1/4 quat (zero for a prismatic joint)
    # the merit's gradient and Hessian as a whole (sign of both curvature terms: h = goal - value)
    n = ch.ndof
    qn, goal, lam, rho, w = q + 0.1, np.concatenate([pose_frames(orc, link, ch, q + 0.2)[0], quat_of(q + 0.2)]), rng.uniform(-1.0, 1.0, 7), 7.0, 1.3

    def value(x):
        fr = pose_frames(orc, link, ch, x)
        return np.concatenate([fr[0], fr[1]])

    def merit(x):
        h = goal - value(x)
        return np.array(w * np.sum((x - qn) ** 2) + lam @ h + 0.5 * rho * h @ h)

    def grad(x):
        return merit_derivatives(ch, w, x, qn, goal, pose_frames(orc, link, ch, x), lam + rho * (goal - value(x)), rho)[0]

    g, H, _ = merit_derivatives(ch, w, q, qn, goal, pose_frames(orc, link, ch, q), lam + rho * (goal - value(q)), rho)
    assert np.abs(g - _central(merit, q)).max() <= 1e-8
    assert np.abs(H - _central(grad, q)).max() <= 1e-8 * max(1.0, np.abs(H).max())
    return Jq


def test_quaternion_jacobian_and_curvature_match_central_differences(kuka):
    orc, ch, _ = kuka
    rng = np.random.default_rng(SEED + 201)
    for q in (NOMINAL, NOMINAL + rng.uniform(-0.5, 0.5, 7), rng.uniform(-1.5, 1.5, 7)):
        _check_derivatives(orc, LINK, ch, q, rng)
    tester = OracleRobot(TESTER_KIN)
    tch = FoldedChain(tester, "eff")
    assert sorted(tch.jtype) == [0, 0, 1]
    Jq = _check_derivatives(tester, "eff", tch, np.array([0.4, -0.3, 0.5]), rng)
    prismatic = tch.qidx[tch.jtype.index(1)]
    assert (Jq[:, prismatic] == 0.0).all() and np.abs(Jq).sum(0).min() == 0.0 and (np.abs(np.delete(Jq, prismatic, axis=1)).sum(0) > 0).all()


@pytest.fixture(scope="module")
def port_runs(kuka):
    """The port on 64 KUKA instances with the full limits and on 64 with the limits narrowed to nominal +- 0.45 (computed once)."""
    orc, ch, nlp = kuka
    rng = np.random.default_rng(SEED + 202)
    out = {}
    for tag, lo, up in (("full", nlp.lo, nlp.up), ("narrow", np.maximum(nlp.lo, NOMINAL - 0.45), np.minimum(nlp.up, NOMINAL + 0.45))):
        qn, pg, qg = kuka_batch(rng, ch, orc, LINK, 64, NOMINAL, lo, up)
        if tag == "narrow":
            qn = np.clip(qn, lo, up)
        runs = [solve_pose_ik_al(orc, LINK, ch, qn[b], qn[b], pg[b], qg[b], lo, up, max_iter=300) for b in range(64)]
        out[tag] = (lo, up, qn, pg, qg, runs)
    return out


def test_port_converges_with_full_and_with_narrowed_limits(kuka, port_runs):
    orc, ch, nlp = kuka
    for tag in ("full", "narrow"):
        lo, up, qn, pg, qg, runs = port_runs[tag]
        assert all(r["status"] == 0 for r in runs), (tag, [r["status"] for r in runs])
        assert max(r["feasibility"] for r in runs) <= 1e-9 and max(r["stationarity"] for r in runs) <= 1e-6
        x = np.stack([r["x"] for r in runs])
        assert (x >= lo).all() and (x <= up).all()
        assert np.abs(ch.fk(x)[0] - pg).max() <= 1e-9 and np.abs(orc.quaternion_batch(LINK, x) - qg).max() <= 1e-9
        print(tag, "evaluations p50 %d max %d" % (np.median([r["iterations"] for r in runs]), max(r["iterations"] for r in runs)))
    active = sum(1 for r in port_runs["narrow"][5] if (r["z_lo"] > 0).any() or (r["z_up"] > 0).any())
    assert active >= 1
    print("instances with an active bound:", active)


def test_port_optima_agree_with_slsqp_on_the_six_row_form(kuka, port_runs):
    """Where SLSQP reports success with the six rows within 1e-8 its optimum is the port's: |f - f_port| <= 1e-6 (twenty times the worst gap
    seen when the iteration was prototyped).  SLSQP's own failures are not graded, but at least 40 of the 64 narrowed instances must be.
    The self-motion manifold of a 7-joint arm cut by the box can hold more than one stationary point, and SLSQP reports success on whichever it
    stops at: narrowed instance 7 of this seed ends at f = 0.56809 where the port, from the same seed and also from SLSQP's own answer, reaches the
    feasible f = 0.54510.  Such an instance is graded with the same bound from the other side: the port must be the lower one, and SLSQP started
    at the port's answer must succeed and stay within 1e-6 of it."""
    _, ch, nlp = kuka
    graded = {}
    for tag in ("narrow", "full"):
        lo, up, qn, pg, qg, runs = port_runs[tag]
        n_graded, worst, reseeded = 0, 0.0, []
        for b in range(64 if tag == "narrow" else 16):
            p = np.concatenate([qn[b], pg[b], qg[b]])
            r, viol = slsqp_six_rows(nlp, ch, qn[b], p, lo, up)
            if not (r.success and viol <= 1e-8):
                continue
            if abs(r.fun - runs[b]["f"]) > 1e-6:
                assert runs[b]["f"] < r.fun and runs[b]["feasibility"] <= 1e-9, (tag, b, r.fun, runs[b]["f"])
                reseeded.append((b, float(r.fun), runs[b]["f"]))
                r, viol = slsqp_six_rows(nlp, ch, runs[b]["x"], p, lo, up)
                assert r.success and viol <= 1e-8, (tag, b, r.message, viol)
            n_graded += 1
            worst = max(worst, abs(r.fun - runs[b]["f"]))
            assert abs(r.fun - runs[b]["f"]) <= 1e-6, (tag, b, r.fun, runs[b]["f"])
        graded[tag] = n_graded
        print(tag, "graded", n_graded, "worst |f - f_port| %.2e" % worst, "graded from the port's answer (b, f_slsqp, f_port):", reseeded)
        assert len(reseeded) <= 1
    assert graded["narrow"] >= 40 and graded["full"] >= 1


def test_the_goal_quaternion_is_literal(kuka, port_runs):
    """h = rhs - lhs with the reference's sign: -quat_goal is another goal (the same rotation, a far configuration or none)."""
    orc, ch, nlp = kuka
    lo, up, qn, pg, qg, runs = port_runs["full"]
    r = solve_pose_ik_al(orc, LINK, ch, qn[0], qn[0], pg[0], -qg[0], lo, up, max_iter=300)
    assert r["status"] != 0 or r["f"] > runs[0]["f"] + 1.0


def test_pose_problem_lowers_to_the_ik_family_with_orientation_set():
    robot, problem = pose_ik.setup_solver(build_only=True)
    kind, spec = lower(problem)
    assert kind == _lib.OH_PROBLEM_IK and isinstance(spec, IkSpec) and spec.orientation is True
    assert (spec.qn_name, spec.pg_name, spec.qg_name, spec.link) == ("q_nominal", "p_goal", "quat_goal", pose_ik.END_EFFECTOR)
    assert spec.lo.shape == (7,) and (spec.lo < spec.up).all() and spec.w_nominal == 1.0


def test_descriptor_layout_is_the_one_without_the_flag():
    """oh_ik_desc.orientation fills the four bytes of padding after max_iter: size and every other offset are unchanged, so the ABI version is."""
    import ctypes as C

    d = _lib.oh_ik_desc
    assert C.sizeof(d) == 304 and (d.max_iter.offset, d.orientation.offset, d.tol.offset, d.rho0.offset) == (272, 276, 280, 296)
    assert _lib.load().oh_abi_version() == _lib.OH_ABI_VERSION == 8
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "optas_hip.h")).read()
    assert header.index("int max_iter;     /* kinematics") < header.index("int orientation;") < header.index("double tol;       /* KKT stationarity")


def test_position_problem_still_lowers_with_orientation_unset():
    robot, problem = example.setup_solver(build_only=True)
    kind, spec = lower(problem)
    assert kind == _lib.OH_PROBLEM_IK and isinstance(spec, IkSpec) and spec.orientation is False and spec.qg_name is None
    assert (spec.qn_name, spec.pg_name) == ("q_nominal", "p_goal")


def _variant(order=("position", "quaternion"), quat_link=None, param_order=("q_nominal", "p_goal", "quat_goal")):
    import optas_amd

    robot = optas_amd.RobotModel.builtin("kuka_lwr")
    b = OptimizationBuilder(1, robots=robot)
    par = {}
    for name in param_order:
        par[name] = b.add_parameter(name, {"q_nominal": robot.ndof, "p_goal": 3, "quat_goal": 4}[name])
    state = b.get_model_state(robot.get_name(), 0)
    for what in order:
        if what == "position":
            b.add_equality_constraint("end_goal", robot.get_global_link_position(LINK, state), par["p_goal"])
        else:
            b.add_equality_constraint("end_orientation", robot.get_global_link_quaternion(quat_link or LINK, state), par["quat_goal"])
    b.add_cost_term("nominal", sumsqr(state - par["q_nominal"]))
    b.enforce_model_limits(robot.get_name())
    return b.build()


def test_refused_shapes_raise_from_match_ik_and_go_to_the_tape_family():
    assert match_ik(_variant()).orientation is True
    for problem in (_variant(order=("quaternion", "position")), _variant(order=("quaternion",), param_order=("q_nominal", "quat_goal")),
                    _variant(quat_link="lwr_arm_6_link"), _variant(param_order=("q_nominal", "quat_goal", "p_goal"))):
        with pytest.raises(LoweringError):
            match_ik(problem)
        assert lower(problem)[0] == _lib.OH_PROBLEM_TAPE
