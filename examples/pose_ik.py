"""Nearest-to-nominal inverse kinematics with a full-pose goal for the KUKA LWR: examples/example.py with a second equality on the link quaternion,
written the way the reference's scripts write an orientation goal (get_global_link_quaternion == parameter, figure_eight_plan.py:105-107).  The goal
is the pose of `end_effector_ball` at a configuration shifted from the nominal one, so it is reachable; its quaternion is the one the model returns
there, sign included: the equality is literal, -quat_goal would be a different (and far) goal.  HIPSolver lowers the problem to the IK kernel family."""
import numpy as np

import optas_amd
from optas_amd.builder import OptimizationBuilder
from optas_amd.expr import sumsqr
from optas_amd.solver import HIPSolver

END_EFFECTOR = "end_effector_ball"
NOMINAL_DEG = (0, 45, 0, -90, 0, -45, 0)
SHIFT_DEG = (10, -8, 12, 9, -15, 10, 20)


def pose_ik_problem(robot, link=END_EFFECTOR):
    """T = 1 problem: parameters q_nominal (ndof), p_goal (3) and quat_goal (4, xyzw); the position equality, then the quaternion equality."""
    b = OptimizationBuilder(1, robots=robot)
    nominal = b.add_parameter("q_nominal", robot.ndof)
    goal = b.add_parameter("p_goal", 3)
    quat = b.add_parameter("quat_goal", 4)
    state = b.get_model_state(robot.get_name(), 0)
    b.add_equality_constraint("end_goal", robot.get_global_link_position(link, state), goal)
    b.add_equality_constraint("end_orientation", robot.get_global_link_quaternion(link, state), quat)
    b.add_cost_term("nominal", sumsqr(state - nominal))
    b.enforce_model_limits(robot.get_name())
    return b.build()


def setup_solver(robot_name="kuka_lwr", solver_options=None, build_only=False):
    robot = optas_amd.RobotModel.builtin(robot_name)
    problem = pose_ik_problem(robot)
    if build_only:
        return robot, problem
    return robot, HIPSolver(problem).setup("hip_sqp", solver_options)


def script_inputs(robot):
    """Nominal configuration and the goal pose: where the end effector is at the nominal configuration shifted by SHIFT_DEG."""
    q_nominal = optas_amd.deg2rad(NOMINAL_DEG)
    q_there = q_nominal + optas_amd.deg2rad(SHIFT_DEG)
    p_goal = np.asarray(robot.get_global_link_position(END_EFFECTOR, q_there)).reshape(-1)
    quat_goal = np.asarray(robot.get_global_link_quaternion(END_EFFECTOR, q_there)).reshape(-1)
    return q_nominal, p_goal, quat_goal


def main():
    robot, solver = setup_solver()
    label = robot.get_name() + "/q"
    q_nominal, p_goal, quat_goal = script_inputs(robot)
    solver.reset_parameters({"q_nominal": q_nominal, "p_goal": p_goal, "quat_goal": quat_goal})
    solver.reset_initial_seed({label + "/x": q_nominal})
    answer = solver.solve()
    q = np.asarray(answer[label]).reshape(-1)
    print("did_solve", solver.did_solve(), "evaluations", solver.number_of_iterations(), "f", solver.stats()["f"][0])
    print("q =", q)
    print("position error", np.abs(np.asarray(robot.get_global_link_position(END_EFFECTOR, q)).reshape(-1) - p_goal).max(),
          "quaternion error", np.abs(np.asarray(robot.get_global_link_quaternion(END_EFFECTOR, q)).reshape(-1) - quat_goal).max())
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
