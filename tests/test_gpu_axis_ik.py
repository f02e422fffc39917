"""Inverse kinematics with a position goal and a link-axis goal (oh_ik_set_axis_goal, k_ik_axis_solve) on the GPU against the numpy port of its state
machine (tests/axis_ik_ref.py) and the literal reference form (AxisIKNLP through kkt_reference_form).  Tolerances are the IK family's own
(tests/test_gpu_pose_ik.py): x and f 1e-7 against the port, evaluations +-2, multipliers 1e-5, equal status; literal form: stationarity 1e-6,
feasibility 1e-9, |f - AxisIKNLP.f| 1e-12."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from axis_ik_ref import AxisIKNLP, axis_frames, kuka_batch, solve_axis_ik_al, unit_axis
from conftest import KUKA_KIN, SEED
from optas_amd import _lib
from optas_amd.backend import IKBackend, tape_backend, tape_default_max_iter
from optas_amd.models import RobotModel
from oracle.robot import OracleRobot
from oracle.solvers import kkt_reference_form
from oracle.structured import FoldedChain
from test_gpu_chain_lengths import _robots

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from examples import axis_ik  # noqa: E402

pytestmark = pytest.mark.gpu
LINK = axis_ik.END_EFFECTOR
NOMINAL = np.deg2rad(axis_ik.NOMINAL_DEG)
EDGES = (1, 63, 64, 65, 257)
GENERAL = np.array([1.0, 2.0, -2.0]) / 3.0
A = unit_axis("z")


@pytest.fixture(scope="module")
def kuka():
    orc = OracleRobot(KUKA_KIN)
    return orc, FoldedChain(orc, LINK), AxisIKNLP(orc, LINK, "z"), RobotModel(urdf_filename=KUKA_KIN).kinematic_chain(LINK)


@pytest.fixture(scope="module")
def edge_reference(kuka):
    """257 instances and the port's answer to each, computed once: the batch of B instances is the first B of them."""
    orc, ch, nlp, _ = kuka
    qn, pg, ug = kuka_batch(np.random.default_rng(SEED + 310), ch, A, max(EDGES), NOMINAL, nlp.lo, nlp.up)
    runs = [solve_axis_ik_al(ch, A, qn[b], qn[b], pg[b], ug[b], nlp.lo, nlp.up) for b in range(max(EDGES))]
    return qn, np.concatenate([qn, pg, ug], 1), runs


def _against_port(res, mult, runs):
    mu, zlo, zup = mult
    for b, r in enumerate(runs):
        assert int(res.status[b]) == r["status"], (b, int(res.status[b]), r["status"])
        assert abs(int(res.iters[b]) - r["iterations"]) <= 2, (b, int(res.iters[b]), r["iterations"])
        assert np.abs(res.x[b] - r["x"]).max() <= 1e-7 and abs(res.f[b] - r["f"]) <= 1e-7, (b, np.abs(res.x[b] - r["x"]).max())
        assert np.abs(mu[b] - r["lam_h"]).max() <= 1e-5 and np.abs(zlo[b] - r["z_lo"]).max() <= 1e-5 and np.abs(zup[b] - r["z_up"]).max() <= 1e-5, b


def _literal_form(nlp, res, mult, p):
    mu, zlo, zup = mult
    for b in range(len(p)):
        lam = np.concatenate([zlo[b], zup[b], np.maximum(mu[b], 0), np.maximum(-mu[b], 0)])
        assert np.abs(nlp.df(res.x[b], p[b]) - nlp.dv(res.x[b], p[b]).T @ lam).max() <= 1e-6, b
        k = kkt_reference_form(nlp, res.x[b], p[b], active_tol=1e-7)
        assert k["stationarity"] <= 1e-6 and k["feasibility"] <= 1e-9, (b, k)
        assert abs(nlp.f(res.x[b], p[b]) - res.f[b]) <= 1e-12


@pytest.mark.parametrize("B", EDGES)
def test_batch_edges_against_port_and_literal_form(hip_lib, kuka, edge_reference, B):
    orc, ch, nlp, chain = kuka
    x0, p, runs = edge_reference
    be = IKBackend(chain, nlp.lo, nlp.up, axis="z")
    assert be.np_ == 13 and be.flag("ik_goal") == 2 and be.flag("ik_orientation") == 0
    res = be.solve(x0[:B], p[:B])
    mult = be.multipliers(B)
    assert mult[0].shape == (B, 6) and mult[1].shape == (B, 7) and mult[2].shape == (B, 7)
    _against_port(res, mult, runs[:B])
    assert res.kkt[:, 0].max() <= 1e-6 and res.kkt[:, 1].max() <= 1e-9 and (res.kkt[:, 2] == 0).all()
    _literal_form(nlp, res, mult, p[:B])
    be.close()


def test_every_chain_length_two_to_eight(hip_lib, tmp_path):
    rng = np.random.default_rng(SEED + 311)
    seen, used = set(), set()
    axes = ["x", "y", "z", GENERAL]
    for i, (tag, kin, link, qn) in enumerate(_robots(tmp_path) + [("kuka7", KUKA_KIN, LINK, NOMINAL)]):  # (_robots has 2, 3, 3, 4, 5, 6 and 8 joints; the arm itself is the 7)
        axis = axes[i % 4]
        a = unit_axis(axis)
        orc = OracleRobot(kin)
        n = orc.ndof
        ch = FoldedChain(orc, link)
        nlp = AxisIKNLP(orc, link, axis)
        lo, up = np.maximum(nlp.lo, -3.0), np.minimum(nlp.up, 3.0)
        be = IKBackend(RobotModel(urdf_filename=kin).kinematic_chain(link), lo, up, max_iter=300, axis=axis)
        B = 64
        q0 = np.clip(qn + rng.uniform(-0.2, 0.2, (B, n)), lo, up)
        qgoal = np.clip(q0 + rng.uniform(-0.3, 0.3, (B, n)), lo, up)  # reachable by construction (chains under five joints are over-determined)
        pg, Re = ch.fk(qgoal)[:2]
        ug = Re @ a
        res = be.solve(q0, np.concatenate([q0, pg, ug], 1))
        runs = [solve_axis_ik_al(ch, a, q0[b], q0[b], pg[b], ug[b], lo, up, max_iter=300) for b in range(B)]
        print(f"axis IK {tag}: {n} joints, axis {axis}, evaluations p50 {int(np.median(res.iters))} max {int(res.iters.max())}, converged {(res.status == 0).mean():.3f}")
        assert [int(s) for s in res.status] == [r["status"] for r in runs], tag
        assert (res.status == 0).all(), (tag, np.bincount(res.status))
        e, Rx = ch.fk(res.x)[:2]
        assert np.abs(e - pg).max() <= 1e-9 and np.abs(Rx @ a - ug).max() <= 1e-9, tag
        assert np.abs(res.x - np.stack([r["x"] for r in runs])).max() <= 1e-7, tag
        seen.add(n)
        used.add(i % 4)
        be.close()
    assert seen == set(range(2, 9)) and used == {0, 1, 2, 3}


def test_active_limits_match_the_port(hip_lib, kuka):
    orc, ch, nlp, chain = kuka
    lo, up = np.maximum(nlp.lo, NOMINAL - 0.45), np.minimum(nlp.up, NOMINAL + 0.45)
    B = 64
    qn, pg, ug = kuka_batch(np.random.default_rng(SEED + 312), ch, A, B, NOMINAL, lo, up)
    qn = np.clip(qn, lo, up)
    be = IKBackend(chain, lo, up, max_iter=300, axis="z")
    res = be.solve(qn, np.concatenate([qn, pg, ug], 1))
    mult = be.multipliers(B)
    runs = [solve_axis_ik_al(ch, A, qn[b], qn[b], pg[b], ug[b], lo, up, max_iter=300) for b in range(B)]
    _against_port(res, mult, runs)
    zlo, zup = mult[1], mult[2]
    assert (zlo >= 0).all() and (zup >= 0).all() and ((zlo > 0) <= (res.x <= lo)).all() and ((zup > 0) <= (res.x >= up)).all()
    n_active = [(int((zlo[b] > 0).sum()), int((zup[b] > 0).sum())) for b in range(B)]
    assert n_active == [(int((r["z_lo"] > 0).sum()), int((r["z_up"] > 0).sum())) for r in runs]
    assert sum(1 for a in n_active if a[0] + a[1] > 0) >= 1
    be.close()


def test_batch_properties(hip_lib, kuka):
    """4096 reachable goals: inside the limits, f = ||x - qn||^2, goals reached to 1e-9 where converged, and the device converges wherever the port
    does (the port is run on the device's failures only).  The port itself leaves 0 of these 4096 instances unconverged (seed SEED + 313, max_iter
    300; the cap is 1 %)."""
    orc, ch, nlp, chain = kuka
    B = 4096
    qn, pg, ug = kuka_batch(np.random.default_rng(SEED + 313), ch, A, B, NOMINAL, nlp.lo, nlp.up)
    be = IKBackend(chain, nlp.lo, nlp.up, max_iter=300, axis="z")
    res = be.solve(qn, np.concatenate([qn, pg, ug], 1))
    ok = res.status == 0
    print("axis IK batch: %.3f ms device for %d instances, evaluations p50 %d max %d, converged %.4f" % (be.solve_ms(), B, np.median(res.iters), res.iters.max(), ok.mean()))
    assert (res.x >= nlp.lo).all() and (res.x <= nlp.up).all()
    assert np.abs(np.sum((res.x - qn) ** 2, 1) - res.f).max() <= 1e-12
    e, Rx = ch.fk(res.x[ok])[:2]
    assert np.abs(e - pg[ok]).max() <= 1e-9 and np.abs(Rx @ A - ug[ok]).max() <= 1e-9 and res.kkt[ok, 0].max() <= 1e-6
    failed = np.flatnonzero(~ok)
    assert len(failed) <= B // 100, len(failed)  # beyond the port's own cap nothing below could pass
    for b in failed:
        r = solve_axis_ik_al(ch, A, qn[b], qn[b], pg[b], ug[b], nlp.lo, nlp.up, max_iter=300)
        print("not converged on the device:", b, "status", int(res.status[b]), "evaluations", int(res.iters[b]), "kkt", res.kkt[b], "| port status", r["status"], "evaluations", r["iterations"])
        assert r["status"] != 0, b
    be.close()


def test_non_finite_inputs_are_reported_as_in_the_siblings(hip_lib, kuka):
    """A non-finite nominal configuration or goal (position or axis part) ends at OH_STATUS_NUMERICAL after the first evaluation.  A non-finite seed
    is projected onto the limits first (fmin / fmax drop a NaN), as in the position kernel; the two kernels agree on the status of such an instance."""
    orc, ch, nlp, chain = kuka
    qn, pg, ug = kuka_batch(np.random.default_rng(SEED + 314), ch, A, 6, NOMINAL, nlp.lo, nlp.up)
    x0, p = qn.copy(), np.concatenate([qn, pg, ug], 1)
    p[1, 3] = np.inf  # nominal configuration
    p[2, 7 + 1] = np.inf  # position goal
    p[3, 7 + 3 + 2] = np.nan  # axis goal
    x0[4, 2], x0[5, 0] = np.nan, np.inf  # seeds
    be = IKBackend(chain, nlp.lo, nlp.up, axis="z")
    res = be.solve(x0, p)
    assert res.status[:4].tolist() == [0, 2, 2, 2] and res.iters[1:4].tolist() == [1, 1, 1]
    pos = IKBackend(chain, nlp.lo, nlp.up)
    rp = pos.solve(x0, p[:, :10])
    assert rp.status[:3].tolist() == [0, 2, 2] and res.status[4:].tolist() == rp.status[4:].tolist()
    assert np.isfinite(res.x[4:]).all() and (res.x[4:] >= nlp.lo).all() and (res.x[4:] <= nlp.up).all()
    be.close()
    pos.close()


def test_a_goal_axis_that_is_not_unit_is_infeasible_as_posed(hip_lib, kuka):
    """The goal is literal: 1.1 times a unit vector cannot be met by a unit u, |1.1 g - u|_2 >= 0.1 with equality at u = g, where the residual is
    0.1 g.  kkt[:, 1] is the largest absolute row, so the instances graded are those whose goal direction has a component of at least 0.95: there the
    best possible residual already has |.|_inf >= 0.095, and 0.09 leaves room for the position rows the penalty trades against."""
    orc, ch, nlp, chain = kuka
    qn, pg, ug = kuka_batch(np.random.default_rng(SEED + 315), ch, A, 64, NOMINAL, nlp.lo, nlp.up)
    sel = np.abs(ug).max(1) >= 0.95
    assert sel.sum() >= 8, int(sel.sum())
    qn, pg, ug = qn[sel], pg[sel], ug[sel]
    be = IKBackend(chain, nlp.lo, nlp.up, axis="z")
    res = be.solve(qn, np.concatenate([qn, pg, 1.1 * ug], 1))
    print("non-unit goal: status", np.bincount(res.status), "feasibility min %.4f max %.4f" % (res.kkt[:, 1].min(), res.kkt[:, 1].max()))
    assert (res.status != 0).all() and (res.kkt[:, 1] >= 0.09).all()
    be.close()


def test_set_axis_goal_error_codes(hip_lib, kuka):
    orc, ch, nlp, chain = kuka
    lib = _lib.load()
    z = (C.c_double * 3)(0.0, 0.0, 1.0)
    pose = IKBackend(chain, nlp.lo, nlp.up, orientation=True)
    assert lib.oh_ik_set_axis_goal(pose._h, z) == _lib.OH_ERR_INVALID and pose.flag("ik_goal") == 1
    pose.close()
    pos = IKBackend(chain, nlp.lo, nlp.up)
    assert pos.flag("ik_goal") == 0
    assert lib.oh_ik_set_axis_goal(pos._h, (C.c_double * 3)(0.0, 0.0, 0.0)) == _lib.OH_ERR_INVALID
    assert lib.oh_ik_set_axis_goal(pos._h, (C.c_double * 3)(0.0, np.nan, 1.0)) == _lib.OH_ERR_INVALID
    assert lib.oh_ik_set_axis_goal(pos._h, None) == _lib.OH_ERR_INVALID and pos.flag("ik_goal") == 0
    qn, pg, _ = kuka_batch(np.random.default_rng(SEED + 316), ch, A, 2, NOMINAL, nlp.lo, nlp.up)
    assert (pos.solve(qn, np.concatenate([qn, pg], 1)).status == 0).all()
    assert lib.oh_ik_set_axis_goal(pos._h, z) == _lib.OH_ERR_STATE and pos.flag("ik_goal") == 0 and pos.np_ == 10
    pos.close()
    # the library normalises the link-frame axis: (0, 0, 2) is 'z'
    a2, az = IKBackend(chain, nlp.lo, nlp.up, axis=(0.0, 0.0, 2.0)), IKBackend(chain, nlp.lo, nlp.up, axis="z")
    qn, pg, ug = kuka_batch(np.random.default_rng(SEED + 316), ch, A, 2, NOMINAL, nlp.lo, nlp.up)
    p = np.concatenate([qn, pg, ug], 1)
    assert (a2.solve(qn, p).x == az.solve(qn, p).x).all()
    a2.close()
    az.close()


def test_example_flow_through_hipsolver(hip_lib, kuka):
    orc, ch, nlp, _ = kuka
    robot, solver = axis_ik.setup_solver()
    name = robot.get_name()
    q_nominal, p_goal, axis_goal = axis_ik.script_inputs(robot)
    solver.reset_parameters({"q_nominal": q_nominal, "p_goal": p_goal, "axis_goal": axis_goal})
    solver.reset_initial_seed({f"{name}/q/x": q_nominal})
    sol = solver.solve()
    assert solver.did_solve() and isinstance(solver._backend, IKBackend) and solver._backend.flag("ik_goal") == 2
    q = np.asarray(sol[f"{name}/q"]).reshape(-1)
    e, u, _, _ = axis_frames(ch, A, q)
    assert np.abs(e - p_goal).max() <= 1e-9 and np.abs(u - axis_goal).max() <= 1e-9
    k = kkt_reference_form(nlp, q, np.concatenate([q_nominal, p_goal, axis_goal]), active_tol=1e-7)
    assert k["stationarity"] <= 1e-6 and k["feasibility"] <= 1e-9 and abs(solver.stats()["f"][0] - nlp.f(q, q_nominal)) <= 1e-12
    # the first stage of the reference's sphere_collision_avoidance.py, call for call
    robot3, solver3, solution, z0 = axis_ik.compute_initial_configuration()
    assert solver3.did_solve() and solver3._backend.flag("ik_goal") == 2
    q = np.asarray(solution[f"{name}/q"]).reshape(-1)
    e, z, _, _ = axis_frames(ch, A, q)
    assert np.abs(e - np.array([0.825, -0.35, 0.2])).max() <= 1e-9 and np.abs(z - np.asarray(z0).reshape(3)).max() <= 1e-9
    assert (q >= nlp.lo).all() and (q <= nlp.up).all()
    assert (np.asarray(solution[f"{name}/dq"]) == 0).all() and (np.asarray(solution[f"{name}/ddq"]) == 0).all()
    assert np.asarray(solution[f"{name}/dq"]).shape == (7, 1) and (solver3._backend.lin_eq_multipliers(1) == 0).all()


def test_same_problem_on_the_tape_family(hip_lib, kuka):
    """The problem written with the axis node, forced onto the generic tape family (the route it takes when match_ik refuses it): same optimum."""
    from optas_amd.lowering import match_tape

    orc, ch, nlp, chain = kuka
    B = 64
    qn, pg, ug = kuka_batch(np.random.default_rng(SEED + 317), ch, A, B, NOMINAL, nlp.lo, nlp.up)
    p = np.concatenate([qn, pg, ug], 1)
    be = IKBackend(chain, nlp.lo, nlp.up, max_iter=300, axis="z")
    rk = be.solve(qn, p)
    be.close()
    tape = match_tape(axis_ik.setup_solver(build_only=True)[1]).tape
    tb = tape_backend(tape, max_iter=tape_default_max_iter(tape.nx), tol=1e-6, tol_feas=1e-9, jit=False)
    rt = tb.solve(qn, p)
    tb.close()
    print("tape against kernel: converged", (rk.status == 0).mean(), (rt.status == 0).mean(), "max |f difference| %.3e" % np.abs(rk.f - rt.f).max())
    assert (rk.status == 0).all() and (rt.status == 0).all()
    assert np.abs(rk.f - rt.f).max() <= 1e-6
