"""Nearest-to-nominal inverse kinematics with a position goal and a goal for one axis of the link frame ("tool tip here, tool z pointing there"), a
5-DoF task: the rotation about the tool axis stays free, so a 7-joint arm keeps two redundant degrees of freedom for the nominal-posture cost.

Two parts.  `axis_ik_problem` is the parameterised batched problem in the style of examples/pose_ik.py: parameters q_nominal, p_goal and axis_goal,
the position equality, then the axis equality.  `compute_initial_configuration` restates the first stage of the reference's
example/sphere_collision_avoidance.py:20-43 call for call: the end-effector transform of a symbolic q taken apart as p = T[:3, 3], z = T[:3, 2],
numeric constants for the nominal configuration and both goals, and a robot with time_derivs=[0, 1, 2] whose dq and ddq blocks
initial_configuration pins to zero.  HIPSolver lowers both to the IK kernel family (k_ik_axis_solve).  The axis goal is literal, like a quaternion
goal: one that is not of unit length is infeasible as posed."""
import numpy as np

import optas_amd
from optas_amd.builder import OptimizationBuilder
from optas_amd.expr import sumsqr
from optas_amd.solver import HIPSolver

END_EFFECTOR = "end_effector_ball"
NOMINAL_DEG = (0, 45, 0, -90, 0, -45, 0)
SHIFT_DEG = (10, -8, 12, 9, -15, 10, 20)
AXIS = "z"
# sphere_collision_avoidance.py:14, :22
SCRIPT_NOMINAL_DEG = (0, -45, 0, 90, 0, 45, 0)
SCRIPT_START_EFF_POSITION = (0.825, -0.35, 0.2)


def axis_ik_problem(robot, link=END_EFFECTOR, axis=AXIS):
    """T = 1 problem: parameters q_nominal (ndof), p_goal (3) and axis_goal (3); the position equality, then the axis equality."""
    b = OptimizationBuilder(1, robots=robot)
    nominal = b.add_parameter("q_nominal", robot.ndof)
    goal = b.add_parameter("p_goal", 3)
    axis_goal = b.add_parameter("axis_goal", 3)
    state = b.get_model_state(robot.get_name(), 0)
    b.add_equality_constraint("end_goal", robot.get_global_link_position(link, state), goal)
    b.add_equality_constraint("end_axis", robot.get_global_link_axis(link, state, axis), axis_goal)
    b.add_cost_term("nominal", sumsqr(state - nominal))
    b.enforce_model_limits(robot.get_name())
    return b.build()


def setup_solver(robot_name="kuka_lwr", solver_options=None, build_only=False):
    robot = optas_amd.RobotModel.builtin(robot_name)
    problem = axis_ik_problem(robot)
    if build_only:
        return robot, problem
    return robot, HIPSolver(problem).setup("hip_sqp", solver_options)


def script_inputs(robot):
    """Nominal configuration and the goal: where the end effector is, and where its z axis points, at the nominal configuration shifted by SHIFT_DEG."""
    q_nominal = optas_amd.deg2rad(NOMINAL_DEG)
    q_there = q_nominal + optas_amd.deg2rad(SHIFT_DEG)
    p_goal = np.asarray(robot.get_global_link_position(END_EFFECTOR, q_there)).reshape(-1)
    axis_goal = np.asarray(robot.get_global_link_axis(END_EFFECTOR, q_there, AXIS)).reshape(-1)
    return q_nominal, p_goal, axis_goal


def initial_configuration_problem(robot_model, z0, qnom=None, start_eff_position=SCRIPT_START_EFF_POSITION, ee_link=END_EFFECTOR):
    """The builder calls of sphere_collision_avoidance.py:23-37, in the script's order.  z0 is the end effector's z axis at qnom (:17-18)."""
    name = robot_model.get_name()
    qnom = optas_amd.deg2rad(SCRIPT_NOMINAL_DEG) if qnom is None else qnom
    start_eff_position = np.asarray(start_eff_position, dtype=np.float64)
    builder = OptimizationBuilder(1, robots=robot_model, derivs_align=True)
    q = builder.get_model_state(name, 0)
    T = robot_model.get_global_link_transform(ee_link, q)
    p = T[:3, 3]
    z = T[:3, 2]

    builder.enforce_model_limits(name)

    builder.add_equality_constraint("eff_pos", p, start_eff_position)
    builder.add_equality_constraint("eff_ori", z, z0)

    builder.initial_configuration(name, time_deriv=1)
    builder.initial_configuration(name, time_deriv=2)

    builder.add_cost_term("nominal", sumsqr(q - qnom))
    return builder.build()


def compute_initial_configuration(robot_name="kuka_lwr", solver_options=None):
    """sphere_collision_avoidance.py:12-43.  Returns (robot, solver, solution dict, z0)."""
    robot_model = optas_amd.RobotModel.builtin(robot_name, time_derivs=[0, 1, 2])
    name = robot_model.get_name()
    qnom = optas_amd.deg2rad(SCRIPT_NOMINAL_DEG)
    T0 = robot_model.get_global_link_transform(END_EFFECTOR, qnom)
    z0 = T0[:3, 2]
    solver = HIPSolver(initial_configuration_problem(robot_model, z0, qnom)).setup("hip_sqp", solver_options)
    solver.reset_initial_seed({f"{name}/q/x": qnom})
    solution = solver.solve()
    return robot_model, solver, solution, z0


def main():
    robot, solver = setup_solver()
    label = robot.get_name() + "/q"
    q_nominal, p_goal, axis_goal = script_inputs(robot)
    solver.reset_parameters({"q_nominal": q_nominal, "p_goal": p_goal, "axis_goal": axis_goal})
    solver.reset_initial_seed({label + "/x": q_nominal})
    answer = solver.solve()
    q = np.asarray(answer[label]).reshape(-1)
    print("did_solve", solver.did_solve(), "evaluations", solver.number_of_iterations(), "f", solver.stats()["f"][0])
    print("q =", q)
    print("position error", np.abs(np.asarray(robot.get_global_link_position(END_EFFECTOR, q)).reshape(-1) - p_goal).max(),
          "axis error", np.abs(np.asarray(robot.get_global_link_axis(END_EFFECTOR, q, AXIS)).reshape(-1) - axis_goal).max())
    robot3, solver3, solution, z0 = compute_initial_configuration()
    q = np.asarray(solution[robot3.get_name() + "/q"]).reshape(-1)
    print("initial configuration: did_solve", solver3.did_solve(), "q =", q)
    print("position", np.asarray(robot3.get_global_link_position(END_EFFECTOR, q)).reshape(-1), "z", np.asarray(robot3.get_global_link_axis(END_EFFECTOR, q, "z")).reshape(-1), "z0", z0)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
