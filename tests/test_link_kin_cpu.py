"""oh_link_kin without a device: the ABI is declared, bound and exported, argument errors come before any device call, the reference the GPU
tests use (tests/link_kin_ref.py) differentiates rpy correctly, and the Python methods fail loudly where there is no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import link_kin_ref as ref
from conftest import KUKA_KIN
from optas_amd import _lib
from optas_amd.models import RobotModel
from oracle.spatialmath import Quaternion

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_SYMBOLS = ("oh_set_link_frames", "oh_link_kin", "oh_link_kin_device")


def test_symbols_struct_and_null_arguments():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "optas_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in optas_hip.h"
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert "typedef struct oh_link_out" in header
    assert C.sizeof(_lib.oh_link_out) == 56  # seven pointers
    out = _lib.oh_link_out()
    assert lib.oh_link_kin(None, 1, None, None, C.byref(out)) == 1 and b"oh_link_kin" in lib.oh_last_error()
    assert lib.oh_link_kin_device(None, 1, None, None, C.byref(out)) == 1 and b"oh_link_kin_device" in lib.oh_last_error()
    assert lib.oh_set_link_frames(None, None, None) == 1 and b"oh_set_link_frames" in lib.oh_last_error()
    assert lib.oh_abi_version() == 8  # no existing struct or entry point changed


@pytest.mark.parametrize("robot_name", sorted(ref.KINS))
def test_reference_rpy_jacobian_matches_central_differences(robot_name):
    """d rpy / d q of the reference helper against central differences (h = 1e-6; their own error floor is ~1e-9) of the oracle's rpy, on
    the inputs of the GPU parity test; roll and yaw differences are wrapped to (-pi, pi]."""
    h = 1e-6
    worst = 0.0
    for index, (robot, link, base) in enumerate(ref.CASES):
        if robot != robot_name:
            continue
        orc = ref.oracle(robot)
        rpy = lambda q: Quaternion.fromvec(orc.get_link_quaternion(link, q, base)).getrpy()
        Q = ref.case_inputs(index)
        assert Q.shape == (ref.N_CONFIGS, orc.ndof) and np.abs(Q).max() <= 3.0
        for q in Q:
            J = ref.rpy_jacobian(orc, link, base, q)
            for j in range(orc.ndof):
                d = np.zeros(orc.ndof)
                d[j] = h
                diff = rpy(q + d) - rpy(q - d)
                diff[0], diff[2] = ref.wrap(diff[0]), ref.wrap(diff[2])
                worst = max(worst, np.abs(diff / (2.0 * h) - J[:, j]).max())
    print(f"reference d rpy / d q against central differences: {worst:.3e}")
    assert worst <= 1e-7


@pytest.mark.skipif(_lib.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_gpu_means_loud_failure_not_fallback():
    with pytest.raises(_lib.OptasHipError):
        RobotModel(urdf_filename=KUKA_KIN).get_link_rpy("end_effector_ball", [0.1] * 7, "lwr_arm_3_link")


def test_axis_argument_is_checked():
    robot = RobotModel(urdf_filename=KUKA_KIN)
    with pytest.raises(ValueError, match="did not recognize input for axis"):
        robot.get_link_axis("end_effector_ball", [0.1] * 7, axis="w", base_link="lwr_arm_3_link")
    with pytest.raises(ValueError, match="did not recognize input for axis"):
        robot.get_global_link_axis("end_effector_ball", [0.1] * 7, [1.0, 0.0])


def test_symbolic_joint_state_is_refused():
    from optas_amd.expr import as_expr

    robot = RobotModel(urdf_filename=KUKA_KIN)
    q = as_expr(np.zeros(7))
    for call in (lambda: robot.get_link_rpy("end_effector_ball", q, "lwr_arm_3_link"), lambda: robot.get_global_link_analytical_jacobian("end_effector_ball", q),
                 lambda: robot.get_link_position_function("end_effector_ball", "lwr_arm_3_link")(q)):
        with pytest.raises(NotImplementedError, match="symbolic"):
            call()
