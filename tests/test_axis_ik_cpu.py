"""Inverse kinematics with a position goal and a link-axis goal without a GPU: the numpy port of the state machine k_ik_axis_solve runs
(tests/axis_ik_ref.py) -- its derivatives against central differences, its optima against scipy SLSQP on a full-rank form of the same rows -- the lowering of the
builder's problems (examples/axis_ik.py) to the IK family, and the tape of the axis node.  The exact derivative members of such a problem go through
the library's kinematics, so that one test is marked gpu."""
import os
import sys

import numpy as np
import pytest

from axis_ik_ref import AxisIKNLP, axis_curvature, axis_frames, axis_jacobian, kuka_batch, merit_derivatives, solve_axis_ik_al, unit_axis
from conftest import KUKA_KIN, SEED, TESTER_KIN
from oracle import tape_ref
from oracle.robot import OracleRobot
from oracle.structured import FoldedChain

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from examples import axis_ik, example, pose_ik  # noqa: E402
import optas_amd  # noqa: E402
from optas_amd import _lib  # noqa: E402
from optas_amd.builder import OptimizationBuilder  # noqa: E402
from optas_amd.expr import LinkFunction, sumsqr  # noqa: E402
from optas_amd.lowering import IkSpec, LoweringError, lower, match_ik, match_tape  # noqa: E402

LINK = "end_effector_ball"
NOMINAL = np.deg2rad([0, 45, 0, -90, 0, -45, 0])
GENERAL = np.array([1.0, 2.0, -2.0]) / 3.0
AXES = ("x", "y", "z", GENERAL)


@pytest.fixture(scope="module")
def kuka():
    orc = OracleRobot(KUKA_KIN)
    return orc, FoldedChain(orc, LINK)


def _central(fun, q, h=1e-5):
    cols = []
    for j in range(len(q)):
        d = np.zeros(len(q))
        d[j] = h
        cols.append((fun(q + d) - fun(q - d)) / (2.0 * h))
    return np.stack(cols, axis=-1)


def _check_derivatives(ch, a, q, rng):
    _, u, Jp, om = axis_frames(ch, a, q)
    Ju = axis_jacobian(om, u)
    assert np.abs(Ju - _central(lambda x: axis_frames(ch, a, x)[1], q)).max() <= 1e-8
    assert np.abs(u @ Ju).max() <= 1e-15 and abs(u @ u - 1.0) <= 1e-14  # the three rows have rank 2
    y = rng.uniform(-1.0, 1.0, 3)
    C = axis_curvature(ch, om, u, y)
    assert np.abs(C - _central(lambda x: axis_jacobian(axis_frames(ch, a, x)[3], axis_frames(ch, a, x)[1]).T @ y, q)).max() <= 1e-8
    # the merit's gradient and Hessian as a whole (sign of both curvature terms: h = goal - value)
    fr2 = axis_frames(ch, a, q + 0.2)
    qn, goal, lam, rho, w = q + 0.1, np.concatenate([fr2[0], fr2[1]]), rng.uniform(-1.0, 1.0, 6), 7.0, 1.3

    def value(x):
        fr = axis_frames(ch, a, x)
        return np.concatenate([fr[0], fr[1]])

    def merit(x):
        h = goal - value(x)
        return np.array(w * np.sum((x - qn) ** 2) + lam @ h + 0.5 * rho * h @ h)

    def grad(x):
        return merit_derivatives(ch, w, x, qn, axis_frames(ch, a, x), lam + rho * (goal - value(x)), rho)[0]

    g, H, _ = merit_derivatives(ch, w, q, qn, axis_frames(ch, a, q), lam + rho * (goal - value(q)), rho)
    assert np.abs(g - _central(merit, q)).max() <= 1e-8
    assert np.abs(H - _central(grad, q)).max() <= 1e-8 * max(1.0, np.abs(H).max())
    return Ju


@pytest.mark.parametrize("axis", AXES, ids=("x", "y", "z", "general"))
def test_axis_jacobian_curvature_and_merit_match_central_differences(kuka, axis):
    _, ch = kuka
    a = unit_axis(axis)
    rng = np.random.default_rng(SEED + 301)
    for q in (NOMINAL, NOMINAL + rng.uniform(-0.5, 0.5, 7), rng.uniform(-1.5, 1.5, 7)):
        _check_derivatives(ch, a, q, rng)
    tester = OracleRobot(TESTER_KIN)
    tch = FoldedChain(tester, "eff")
    assert sorted(tch.jtype) == [0, 0, 1]
    Ju = _check_derivatives(tch, a, np.array([0.4, -0.3, 0.5]), rng)
    assert (Ju[:, tch.qidx[tch.jtype.index(1)]] == 0.0).all()  # a prismatic joint does not turn the axis


@pytest.fixture(scope="module")
def port_runs(kuka):
    """The port on 16 KUKA instances of the batch distribution (computed once)."""
    orc, ch = kuka
    a = unit_axis("z")
    nlp = AxisIKNLP(orc, LINK, "z")
    qn, pg, ug = kuka_batch(np.random.default_rng(SEED + 302), ch, a, 16, NOMINAL, nlp.lo, nlp.up)
    return nlp, a, qn, pg, ug, [solve_axis_ik_al(ch, a, qn[b], qn[b], pg[b], ug[b], nlp.lo, nlp.up, max_iter=300) for b in range(16)]


def _slsqp(nlp, x0, p):
    """scipy SLSQP on the problem with the three axis rows of the literal h projected onto the two directions orthogonal to the goal:
    [p_goal - p; t1 . (u_goal - u); t2 . (u_goal - u)] = 0 with the bounds -- five rows of full rank with, near a unit goal, the literal problem's
    feasible set.  Returns (result, violation of the literal six rows at result.x)."""
    from scipy.optimize import minimize

    g = p[nlp.n + 3 :]
    t1 = np.cross(g, [1.0, 0.0, 0.0] if abs(g[0]) < 0.9 else [0.0, 1.0, 0.0])
    t1 /= np.linalg.norm(t1)
    M = np.zeros((5, 6))
    M[:3, :3], M[3, 3:], M[4, 3:] = np.eye(3), t1, np.cross(g, t1)
    r = minimize(lambda x: nlp.f(x, p), x0, jac=lambda x: nlp.df(x, p), method="SLSQP", bounds=list(zip(nlp.lo, nlp.up)),
                 constraints=[{"type": "eq", "fun": lambda x: M @ nlp.h(x, p), "jac": lambda x: M @ nlp.dh(x, p)}], tol=1e-12, options={"maxiter": 200})
    return r, float(np.abs(nlp.h(r.x, p)).max())


def test_port_optima_agree_with_slsqp(kuka, port_runs):
    """16 instances: the port converges with the six literal rows within 1e-9, and SLSQP ends at the same cost to 1e-6 with the literal rows within
    1e-9.  SLSQP is given the rows in the five-row form of `_slsqp`, not the literal six: |u| = 1 makes the literal Jacobian rank five, and SLSQP's
    least-squares subproblem cannot factor it -- on these 16 instances it stops at once with status 6 (singular matrix C in LSQ subproblem, 11
    instances) or 8 (positive directional derivative, 5) and the literal rows still 0.17 ... 0.72 off, so it yields no optimum to compare with.  On
    the five rows it succeeds from q_nominal on 14 of the 16 with |f - f_port| <= 4.8e-9; the other two run into its iteration cap.  An instance on
    which SLSQP fails or ends at another stationary point is started again from the port's answer, as in the pose test, and must then succeed within
    the same bounds; at least half must be graded from q_nominal."""
    nlp, a, qn, pg, ug, runs = port_runs
    worst, reseeded = 0.0, []
    for b, run in enumerate(runs):
        assert run["status"] == 0 and run["feasibility"] <= 1e-9 and run["stationarity"] <= 1e-6, (b, run)
        p = np.concatenate([qn[b], pg[b], ug[b]])
        r, viol = _slsqp(nlp, qn[b], p)
        if not (r.success and viol <= 1e-9 and abs(r.fun - run["f"]) <= 1e-6):
            reseeded.append((b, int(r.status), float(r.fun), viol, run["f"]))
            r, viol = _slsqp(nlp, run["x"], p)
        worst = max(worst, abs(r.fun - run["f"]))
        assert r.success and viol <= 1e-9 and abs(r.fun - run["f"]) <= 1e-6, (b, r.fun, run["f"], viol, r.message)
    print("worst |f - f_port| %.2e; started again from the port's answer (b, SLSQP status, f_slsqp, violation, f_port):" % worst, reseeded)
    assert len(reseeded) <= 8


def test_both_spellings_lower_to_the_ik_family_with_the_axis_goal():
    robot, problem = axis_ik.setup_solver(build_only=True)
    kind, spec = lower(problem)
    assert kind == _lib.OH_PROBLEM_IK and isinstance(spec, IkSpec) and spec.goal == 2 and spec.orientation is False and spec.plain
    assert (spec.qn_name, spec.pg_name, spec.ug_name, spec.link) == ("q_nominal", "p_goal", "axis_goal", axis_ik.END_EFFECTOR)
    assert (spec.axis == [0.0, 0.0, 1.0]).all()
    by_transform = match_ik(_variant(spelling="transform"))
    assert by_transform.goal == 2 and (by_transform.axis == spec.axis).all() and by_transform.link == spec.link
    general = match_ik(_variant(axis=(1.0, 2.0, -2.0)))
    assert np.abs(general.axis - GENERAL).max() <= 1e-16


def test_position_and_pose_problems_lower_as_before():
    kind, spec = lower(example.setup_solver(build_only=True)[1])
    assert kind == _lib.OH_PROBLEM_IK and spec.goal == 0 and spec.orientation is False and spec.qg_name is None and spec.axis is None and spec.plain
    assert (spec.qn_name, spec.pg_name) == ("q_nominal", "p_goal")
    kind, spec = lower(pose_ik.setup_solver(build_only=True)[1])
    assert kind == _lib.OH_PROBLEM_IK and spec.goal == 1 and spec.orientation is True and spec.axis is None and spec.plain
    assert (spec.qn_name, spec.pg_name, spec.qg_name) == ("q_nominal", "p_goal", "quat_goal")


def _variant(order=("position", "axis"), axis_link=None, spelling="axis", axis="z", extra=None, goal_rows=3):
    robot = optas_amd.RobotModel.builtin("kuka_lwr")
    b = OptimizationBuilder(1, robots=robot)
    par = {name: b.add_parameter(name, rows) for name, rows in (("q_nominal", robot.ndof), ("p_goal", 3), ("axis_goal", 3))}
    state = b.get_model_state(robot.get_name(), 0)
    for what in order:
        if what == "position":
            b.add_equality_constraint("end_goal", robot.get_global_link_position(LINK, state), par["p_goal"])
        elif spelling == "transform":
            b.add_equality_constraint("end_axis", robot.get_global_link_transform(axis_link or LINK, state)[:3, "xyz".index(axis)], par["axis_goal"])
        else:
            b.add_equality_constraint("end_axis", robot.get_global_link_axis(axis_link or LINK, state, axis), par["axis_goal"])
    if extra == "third":
        b.add_equality_constraint("end_axis_again", robot.get_global_link_axis(LINK, state, "x"), par["axis_goal"])
    b.add_cost_term("nominal", sumsqr(state - par["q_nominal"]))
    b.enforce_model_limits(robot.get_name())
    problem = b.build()
    if goal_rows == 4:  # a 4-vector against the axis node: the builder itself refuses the shapes, so the built row's goal is widened afterwards
        goal = problem.eq_constraints["end_axis"].a
        goal.m, goal.shape = 4, (4, 1)
    return problem


def test_refused_shapes_raise_from_match_ik():
    assert match_ik(_variant()).goal == 2
    for problem in (_variant(axis_link="lwr_arm_6_link"), _variant(order=("axis", "position")), _variant(extra="third"), _variant(goal_rows=4)):
        with pytest.raises(LoweringError):
            match_ik(problem)
    # what match_ik refuses for its order or its link still runs on the tape family
    assert lower(_variant(order=("axis", "position")))[0] == _lib.OH_PROBLEM_TAPE and lower(_variant(axis_link="lwr_arm_6_link"))[0] == _lib.OH_PROBLEM_TAPE


def test_the_reference_scripts_first_stage_lowers_to_the_ik_family():
    """compute_initial_configuration()'s problem (sphere_collision_avoidance.py:20-43): its three numeric constants land in the kernel's parameter row,
    and the dq and ddq blocks that initial_configuration pins to zero appear in the solution layout."""
    robot = optas_amd.RobotModel.builtin("kuka_lwr", time_derivs=[0, 1, 2])
    z0 = np.array([0.6, 0.0, -0.8])
    problem = axis_ik.initial_configuration_problem(robot, z0)
    kind, spec = lower(problem)
    assert kind == _lib.OH_PROBLEM_IK and spec.goal == 2 and not spec.plain and (spec.axis == [0.0, 0.0, 1.0]).all()
    assert (spec.qn_name, spec.pg_name, spec.ug_name) == (None, None, None)
    assert (spec.consts["qn"] == np.deg2rad(axis_ik.SCRIPT_NOMINAL_DEG)).all() and (spec.consts["pg"] == axis_ik.SCRIPT_START_EFF_POSITION).all() and (spec.consts["ug"] == z0).all()
    name = robot.get_name()
    assert list(problem.decision_variables.keys()) == [f"{name}/q/x", f"{name}/dq/x", f"{name}/ddq/x"] and problem.nx == 21
    assert set(spec.pinned) == {f"{name}/dq/x", f"{name}/ddq/x"} and all((v == 0).all() and v.shape == (7,) for v in spec.pinned.values())
    # an unpinned further block is refused
    b = OptimizationBuilder(1, robots=robot, derivs_align=True)
    q = b.get_model_state(name, 0)
    b.add_equality_constraint("eff_pos", robot.get_global_link_position(LINK, q), [0.5, 0.0, 0.5])
    b.initial_configuration(name, time_deriv=1)
    b.add_cost_term("nominal", sumsqr(q - np.zeros(7)))
    with pytest.raises(LoweringError):
        match_ik(b.build())


def test_the_axis_node_compiles_to_the_tape_of_the_rotation_column():
    """The problem written with the axis node and the one written with get_global_link_rotation(link, q)[:, 2] give the same tape values to 1e-12."""
    robot = optas_amd.RobotModel.builtin("kuka_lwr")

    def problem(node_of):
        b = OptimizationBuilder(1, robots=robot)
        nominal, goal, axis_goal = b.add_parameter("q_nominal", robot.ndof), b.add_parameter("p_goal", 3), b.add_parameter("axis_goal", 3)
        state = b.get_model_state(robot.get_name(), 0)
        b.add_equality_constraint("end_goal", robot.get_global_link_position(LINK, state), goal)
        b.add_equality_constraint("end_axis", node_of(state), axis_goal)
        b.add_cost_term("nominal", sumsqr(state - nominal))
        b.enforce_model_limits(robot.get_name())
        return b.build()

    new = problem(lambda s: robot.get_global_link_axis(LINK, s, "z"))
    old = problem(lambda s: robot.get_global_link_rotation(LINK, s)[:, 2])
    assert isinstance(new.eq_constraints["end_axis"].b, LinkFunction) and new.eq_constraints["end_axis"].b.what == "axis"
    with pytest.raises(LoweringError):
        match_ik(old)
    t_new, t_old = match_tape(new).tape, match_tape(old).tape
    assert (t_new.nx, t_new.np_, t_new.n_eq, t_new.n_ineq) == (t_old.nx, t_old.np_, t_old.n_eq, t_old.n_ineq) == (7, 13, 6, 14)
    rng = np.random.default_rng(SEED + 303)
    orc = OracleRobot(KUKA_KIN)
    ch = FoldedChain(orc, LINK)
    for _ in range(3):
        x, p = rng.uniform(-1.5, 1.5, 7), rng.uniform(-1.0, 1.0, 13)
        v_new, v_old = tape_ref.forward(t_new, x, p), tape_ref.forward(t_old, x, p)
        for t, v in ((t_new, v_new), (t_old, v_old)):
            assert abs(v[t.out_cost] - np.sum((x - p[:7]) ** 2)) <= 1e-12
        rows_new, rows_old = v_new[np.asarray(t_new.out_rows)], v_old[np.asarray(t_old.out_rows)]
        assert np.abs(rows_new - rows_old).max() <= 1e-12
        e, u, _, _ = axis_frames(ch, unit_axis("z"), x)
        assert np.abs(rows_new[-6:] - np.concatenate([p[7:10] - e, p[10:] - u])).max() <= 1e-12
    # the general axis: rows against the port's frames
    gen = problem(lambda s: robot.get_global_link_axis(LINK, s, (1.0, 2.0, -2.0)))
    t_gen = match_tape(gen).tape
    x, p = rng.uniform(-1.5, 1.5, 7), rng.uniform(-1.0, 1.0, 13)
    e, u, _, _ = axis_frames(ch, GENERAL, x)
    assert np.abs(tape_ref.forward(t_gen, x, p)[np.asarray(t_gen.out_rows)][-6:] - np.concatenate([p[7:10] - e, p[10:] - u])).max() <= 1e-12


@pytest.mark.gpu
def test_exact_h_dh_ddh_of_the_axis_problem_against_central_differences(hip_lib):
    """Optimization.h / dh / ddh of the axis problem (the kinematics inside go through the library): dh against central differences of h to 1e-7,
    ddh against central differences of dh to 1e-5, for 'z' through the transform spelling and for the general axis."""
    rng = np.random.default_rng(SEED + 304)
    orc = OracleRobot(KUKA_KIN)
    ch = FoldedChain(orc, LINK)
    for problem, a in ((_variant(spelling="transform"), unit_axis("z")), (_variant(axis=(1.0, 2.0, -2.0)), GENERAL)):
        x, p = NOMINAL + rng.uniform(-0.5, 0.5, 7), rng.uniform(-1.0, 1.0, 13)
        e, u, _, _ = axis_frames(ch, a, x)
        assert np.abs(problem.h(x, p) - np.concatenate([p[7:10] - e, p[10:] - u])).max() <= 1e-12
        dh = problem.dh(x, p)
        assert dh.shape == (6, 7) and np.abs(dh - _central(lambda z: problem.h(z, p), x)).max() <= 1e-7
        ddh = problem.ddh(x, p)
        fd = _central(lambda z: problem.dh(z, p), x)  # (6, 7, 7)
        assert ddh.shape == (6, 7, 7) and np.abs(ddh - fd).max() <= 1e-5 and np.abs(ddh - np.swapaxes(ddh, 1, 2)).max() <= 1e-12
        assert np.abs(ddh[3:]).max() > 1e-2  # the axis rows do carry curvature
