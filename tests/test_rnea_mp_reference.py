"""The float64 oracle of RobotModel.rnea (oracle/torque.py: rnea_batch, its complex-step Jacobian rnea_jacobian and the complex-step Hessian of
its hand-written adjoint rnea_ctau_hessian) against a 50-digit restatement differenced in mpmath (oracle/rnea_mp.py), on every chain length
1 ... 8 joints and the awkward arm of tests/dyn_robots.py.  The GPU kernels are graded against the float64 oracle at every sample
(tests/test_gpu_rnea_kernels.py); this pins the oracle itself."""
import numpy as np
import pytest

import dyn_robots
from oracle.rnea_mp import rnea_ctau_hessian_mp, rnea_jacobian_mp, rnea_mp
from oracle.robot import OracleRobot
from oracle.torque import RneaTables, rnea_batch, rnea_ctau_hessian, rnea_jacobian

TAGS = ["med1", "med2", "med3", "med4", "med5", "med6", "med7", "med8", "tester2", "awkward5"]


def _rel(a, ref):
    return np.abs(a - ref).max() / max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("tag", TAGS)
def test_float64_oracle_equals_the_mp_reference(tag, tmp_path):
    kin = {t: k for t, k, _ in dyn_robots.robots(tmp_path)}[tag]
    tb = RneaTables(OracleRobot(kin))
    for q, qd, qdd, c, hess in dyn_robots.mp_points(tag, tb.ndof):
        tau = rnea_mp(tb, q, qd, qdd)
        assert _rel(rnea_batch(tb, q, qd, qdd), tau) <= 1e-13, (tag, q)
        J = rnea_jacobian_mp(tb, q, qd, qdd)
        assert _rel(rnea_jacobian(tb, q, qd, qdd), J) <= 1e-12, (tag, q)
        if hess:
            H = rnea_ctau_hessian_mp(tb, q, qd, qdd, c)
            assert _rel(rnea_ctau_hessian(tb, q, qd, qdd, c), H) <= 1e-11, (tag, q)
            assert np.abs(H[2 * tb.ndof:, tb.ndof:]).max() <= 1e-20 * max(1.0, np.abs(H).max())  # tau is affine in qdd


def test_every_robot_is_listed(tmp_path):
    assert sorted(TAGS) == sorted(t for t, _, _ in dyn_robots.robots(tmp_path))
