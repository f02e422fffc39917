"""Full-pose inverse kinematics (oh_ik_desc.orientation, k_ik_pose_solve) on the GPU against the numpy port of its state machine
(tests/pose_ik_ref.py) and the literal reference form (PoseIKNLP through kkt_reference_form).  Tolerances are the IK family's own
(tests/test_gpu_ik.py): x and f 1e-7 against the port, evaluations +-2, multipliers 1e-5, equal status; literal form: stationarity 1e-6,
feasibility 1e-9, |f - PoseIKNLP.f| 1e-12.  The position path is held to the bits of the parent's library (tests/golden/ik_parent_bits.npz)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, KUKA_KIN, SEED
from optas_amd.backend import IKBackend
from optas_amd.models import RobotModel
from oracle.robot import OracleRobot
from oracle.solvers import kkt_reference_form
from oracle.structured import FoldedChain
from pose_ik_ref import PoseIKNLP, kuka_batch, solve_pose_ik_al
from test_gpu_chain_lengths import _robots

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from examples import pose_ik  # noqa: E402

pytestmark = pytest.mark.gpu
LINK = pose_ik.END_EFFECTOR
NOMINAL = np.deg2rad(pose_ik.NOMINAL_DEG)
EDGES = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def kuka():
    orc = OracleRobot(KUKA_KIN)
    return orc, FoldedChain(orc, LINK), PoseIKNLP(orc, LINK), RobotModel(urdf_filename=KUKA_KIN).kinematic_chain(LINK)


@pytest.fixture(scope="module")
def edge_reference(kuka):
    """257 instances and the port's answer to each, computed once: the batch of B instances is the first B of them."""
    orc, ch, nlp, _ = kuka
    qn, pg, qg = kuka_batch(np.random.default_rng(SEED + 210), ch, orc, LINK, max(EDGES), NOMINAL, nlp.lo, nlp.up)
    runs = [solve_pose_ik_al(orc, LINK, ch, qn[b], qn[b], pg[b], qg[b], nlp.lo, nlp.up) for b in range(max(EDGES))]
    return qn, np.concatenate([qn, pg, qg], 1), runs


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
    be = IKBackend(chain, nlp.lo, nlp.up, orientation=True)
    assert be.np_ == 14 and be.flag("ik_orientation") == 1
    res = be.solve(x0[:B], p[:B])
    mult = be.multipliers(B)
    assert mult[0].shape == (B, 7) and mult[1].shape == (B, 7) and mult[2].shape == (B, 7)
    _against_port(res, mult, runs[:B])
    assert res.kkt[:, 0].max() <= 1e-6 and res.kkt[:, 1].max() <= 1e-9 and (res.kkt[:, 2] == 0).all()
    _literal_form(nlp, res, mult, p[:B])
    be.close()


def test_every_chain_length_two_to_eight(hip_lib, tmp_path):
    rng = np.random.default_rng(SEED + 211)
    seen = set()
    for tag, kin, link, qn in _robots(tmp_path) + [("kuka7", KUKA_KIN, LINK, NOMINAL)]:  # (_robots has 2, 3, 3, 4, 5, 6 and 8 joints; the arm itself is the 7)
        orc = OracleRobot(kin)
        n = orc.ndof
        ch = FoldedChain(orc, link)
        nlp = PoseIKNLP(orc, link)
        lo, up = np.maximum(nlp.lo, -3.0), np.minimum(nlp.up, 3.0)
        be = IKBackend(RobotModel(urdf_filename=kin).kinematic_chain(link), lo, up, max_iter=300, orientation=True)
        B = 64
        q0 = np.clip(qn + rng.uniform(-0.2, 0.2, (B, n)), lo, up)
        qgoal = np.clip(q0 + rng.uniform(-0.3, 0.3, (B, n)), lo, up)  # reachable by construction (chains under six joints are over-determined)
        pg, qg = ch.fk(qgoal)[0], orc.quaternion_batch(link, qgoal)
        res = be.solve(q0, np.concatenate([q0, pg, qg], 1))
        runs = [solve_pose_ik_al(orc, link, ch, q0[b], q0[b], pg[b], qg[b], lo, up, max_iter=300) for b in range(B)]
        assert [int(s) for s in res.status] == [r["status"] for r in runs], tag
        assert (res.status == 0).all(), (tag, np.bincount(res.status))
        assert np.abs(ch.fk(res.x)[0] - pg).max() <= 1e-9 and np.abs(orc.quaternion_batch(link, res.x) - qg).max() <= 1e-9, tag
        assert np.abs(res.x - np.stack([r["x"] for r in runs])).max() <= 1e-7, tag
        seen.add(n)
        print(f"pose IK {tag}: {n} joints, evaluations p50 {int(np.median(res.iters))} max {int(res.iters.max())}")
        be.close()
    assert seen == set(range(2, 9))


def test_active_limits_match_the_port(hip_lib, kuka):
    orc, ch, nlp, chain = kuka
    lo, up = np.maximum(nlp.lo, NOMINAL - 0.45), np.minimum(nlp.up, NOMINAL + 0.45)
    B = 64
    qn, pg, qg = kuka_batch(np.random.default_rng(SEED + 212), ch, orc, LINK, B, NOMINAL, lo, up)
    qn = np.clip(qn, lo, up)
    be = IKBackend(chain, lo, up, max_iter=300, orientation=True)
    res = be.solve(qn, np.concatenate([qn, pg, qg], 1))
    mult = be.multipliers(B)
    runs = [solve_pose_ik_al(orc, LINK, ch, qn[b], qn[b], pg[b], qg[b], lo, up, max_iter=300) for b in range(B)]
    _against_port(res, mult, runs)
    zlo, zup = mult[1], mult[2]
    assert (zlo >= 0).all() and (zup >= 0).all() and ((zlo > 0) <= (res.x <= lo)).all() and ((zup > 0) <= (res.x >= up)).all()
    n_active = [(int((zlo[b] > 0).sum()), int((zup[b] > 0).sum())) for b in range(B)]
    assert n_active == [(int((r["z_lo"] > 0).sum()), int((r["z_up"] > 0).sum())) for r in runs]
    assert sum(1 for a in n_active if a[0] + a[1] > 0) >= 1
    be.close()


def test_batch_properties(hip_lib, kuka):
    """4096 reachable pose goals: every one converges (the port does on this distribution), reaches the pose to 1e-9 and stays inside the limits."""
    orc, ch, nlp, chain = kuka
    B = 4096
    qn, pg, qg = kuka_batch(np.random.default_rng(SEED + 213), ch, orc, LINK, B, NOMINAL, nlp.lo, nlp.up)
    be = IKBackend(chain, nlp.lo, nlp.up, max_iter=300, orientation=True)
    res = be.solve(qn, np.concatenate([qn, pg, qg], 1))
    ok = res.status == 0
    for b in np.flatnonzero(~ok)[:8]:  # the port's verdict on what the device did not finish
        r = solve_pose_ik_al(orc, LINK, ch, qn[b], qn[b], pg[b], qg[b], nlp.lo, nlp.up, max_iter=300)
        print("not converged on the device:", b, "status", int(res.status[b]), "evaluations", int(res.iters[b]), "kkt", res.kkt[b], "| port status", r["status"], "evaluations", r["iterations"])
    assert (res.x >= nlp.lo).all() and (res.x <= nlp.up).all()
    assert np.abs(ch.fk(res.x[ok])[0] - pg[ok]).max() <= 1e-9 and np.abs(orc.quaternion_batch(LINK, res.x[ok]) - qg[ok]).max() <= 1e-9
    assert np.abs(np.sum((res.x - qn) ** 2, 1) - res.f).max() <= 1e-12 and res.kkt[ok, 0].max() <= 1e-6
    print("pose IK batch: %.3f ms device for %d instances, evaluations p50 %d max %d, converged %.4f" % (be.solve_ms(), B, np.median(res.iters), res.iters.max(), ok.mean()))
    assert ok.mean() == 1.0
    be.close()


def test_example_flow_through_hipsolver(hip_lib, kuka):
    orc, ch, nlp, _ = kuka
    robot, solver = pose_ik.setup_solver()
    name = robot.get_name()
    q_nominal, p_goal, quat_goal = pose_ik.script_inputs(robot)
    solver.reset_parameters({"q_nominal": q_nominal, "p_goal": p_goal, "quat_goal": quat_goal})
    solver.reset_initial_seed({f"{name}/q/x": q_nominal})
    sol = solver.solve()
    assert solver.did_solve() and isinstance(solver._backend, IKBackend) and solver._backend.flag("ik_orientation") == 1
    assert {f"{name}/q", f"{name}/q/x"} <= set(sol) and sol[f"{name}/q"].shape == (7, 1)
    st = solver.stats()
    assert st["success"] and st["return_status"] == ["Solve_Succeeded"] and st["iter_count"] == int(st["iterations"][0]) <= 60
    q = np.asarray(sol[f"{name}/q"]).reshape(-1)
    assert np.abs(orc.get_global_link_position(LINK, q) - p_goal).max() <= 1e-9 and np.abs(orc.get_global_link_quaternion(LINK, q) - quat_goal).max() <= 1e-9
    k = kkt_reference_form(nlp, q, np.concatenate([q_nominal, p_goal, quat_goal]), active_tol=1e-7)
    assert k["stationarity"] <= 1e-6 and k["feasibility"] <= 1e-9 and abs(st["f"][0] - nlp.f(q, q_nominal)) <= 1e-12
    # a position-only handle answers 0
    from examples.example import setup_solver

    assert setup_solver()[1]._backend.flag("ik_orientation") == 0


def test_position_path_is_bit_equal_to_the_parent(hip_lib, kuka):
    """orientation = 0: x, f, evaluations and multipliers of the golden batch of test_gpu_ik.py, bit for bit what the library built from the
    parent commit returned (tests/golden/ik_parent_bits.npz, dumped there through the same IKBackend calls)."""
    _, _, nlp, chain = kuka
    g, ref = np.load(os.path.join(GOLDEN, "ik_golden.npz")), np.load(os.path.join(GOLDEN, "ik_parent_bits.npz"))
    be = IKBackend(chain, nlp.lo, nlp.up)
    assert be.np_ == 10 and be.flag("ik_orientation") == 0
    res = be.solve(g["x0"], g["p"])
    mu, zlo, zup = be.multipliers(len(g["p"]))
    assert mu.shape[1] == 3
    for name, got in (("x", res.x), ("f", res.f), ("kkt", res.kkt), ("mu", mu), ("z_lo", zlo), ("z_up", zup)):
        assert got.shape == ref[name].shape and (np.ascontiguousarray(got).view(np.uint64) == np.ascontiguousarray(ref[name]).view(np.uint64)).all(), name
    assert (res.iters == ref["iters"]).all() and (res.status == ref["status"]).all()
    be.close()


def test_non_finite_inputs_are_reported_as_in_the_position_kernel(hip_lib, kuka):
    """A non-finite nominal configuration or goal (position or quaternion part) ends at OH_STATUS_NUMERICAL after the first evaluation.  A non-finite
    seed is treated as the position kernel treats it: the projection onto the limits comes first (fmin / fmax drop a NaN), so with finite limits
    the solve starts from the bound; the two kernels must agree on the status of such an instance."""
    orc, ch, nlp, chain = kuka
    qn, pg, qg = kuka_batch(np.random.default_rng(SEED + 214), ch, orc, LINK, 6, NOMINAL, nlp.lo, nlp.up)
    x0, p = qn.copy(), np.concatenate([qn, pg, qg], 1)
    p[1, 3] = np.inf  # nominal configuration
    p[2, 7 + 1] = np.inf  # position goal
    p[3, 7 + 3 + 2] = np.nan  # quaternion goal
    x0[4, 2], x0[5, 0] = np.nan, np.inf  # seeds
    be = IKBackend(chain, nlp.lo, nlp.up, orientation=True)
    res = be.solve(x0, p)
    assert res.status[:4].tolist() == [0, 2, 2, 2] and res.iters[1:4].tolist() == [1, 1, 1]
    pos = IKBackend(chain, nlp.lo, nlp.up)
    rp = pos.solve(x0, p[:, :10])
    assert rp.status[:3].tolist() == [0, 2, 2] and res.status[4:].tolist() == rp.status[4:].tolist()
    assert np.isfinite(res.x[4:]).all() and (res.x[4:] >= nlp.lo).all() and (res.x[4:] <= nlp.up).all()
    be.close()
    pos.close()
