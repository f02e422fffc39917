"""The one IK iteration over a rows policy (optas_amd/csrc/oh_ik.hip: ik_rows_solve with IkPositionRows, IkPoseRows, IkAxisRows) held to the bits of the
three texts it replaced.  tests/golden/ik_rows_parent_bits.npz was written on an MI355X by the library of the last commit that had k_ik_solve and
k_ik_pose_solve as texts of their own beside ik_rows_solve, through rows_outputs() below (tools/gpu_ik_ab_dump.py pin): for each goal shape, every chain
length from 2 to 8 on reachable goals, a KUKA batch with narrowed limits (active bounds), the non-finite inputs of the pose and the axis tests and, for
the axis goal, the goal that is not of unit length (the case whose outer passes make no evaluation).  Outputs only; the inputs come from the seeds.
Equality of every array as integers, per goal shape and case."""
import os

import numpy as np
import pytest

import axis_ik_ref
import pose_ik_ref
from conftest import GOLDEN, KUKA_KIN, SEED
from optas_amd.backend import IKBackend
from optas_amd.models import RobotModel
from oracle.problems import IKExampleNLP
from oracle.robot import OracleRobot
from oracle.structured import FoldedChain
from test_gpu_chain_lengths import _robots

LINK = "end_effector_ball"
NOMINAL = np.deg2rad([0, 45, 0, -90, 0, -45, 0])
GOALS = {"position": {}, "pose": {"orientation": True}, "axis": {"axis": "z"}}  # IKBackend's arguments
A = axis_ik_ref.unit_axis("z")
OUT = ("x", "f", "kkt", "iters", "status", "mu", "z_lo", "z_up")
B_KUKA, B_OTHER = 65, 16  # one full block plus one lane on the arm itself


def _goal_rows(orc, link, ch, qgoal):
    """Per goal shape, the goal columns of p at the configurations qgoal: position; position and quaternion; position and link z axis."""
    pg, Re = ch.fk(qgoal)[:2]
    return {"position": pg, "pose": np.concatenate([pg, orc.quaternion_batch(link, qgoal)], 1), "axis": np.concatenate([pg, Re @ A], 1)}


def rows_cases(tmp_path):
    """[(case, goal shape, kinematics file, link, lo, up, max_iter or None for the default, x0, p)]"""
    cases = []
    rng = np.random.default_rng(SEED + 401)
    lengths = set()
    for tag, kin, link, qn in _robots(tmp_path) + [("kuka7", KUKA_KIN, LINK, NOMINAL)]:  # 2, 3, 3, 4, 5, 6, 8 joints and the arm itself
        orc = OracleRobot(kin)
        n, ch, nlp = orc.ndof, FoldedChain(orc, link), IKExampleNLP(orc, link)
        lengths.add(n)
        lo, up = np.maximum(nlp.lo, -3.0), np.minimum(nlp.up, 3.0)
        B = B_KUKA if tag == "kuka7" else B_OTHER
        q0 = np.clip(qn + rng.uniform(-0.2, 0.2, (B, n)), lo, up)  # seeds and reachable goals as test_every_chain_length_two_to_eight draws them
        for goal, g in _goal_rows(orc, link, ch, np.clip(q0 + rng.uniform(-0.3, 0.3, (B, n)), lo, up)).items():
            cases.append(("length_" + tag, goal, kin, link, lo, up, 300, q0, np.concatenate([q0, g], 1)))
    assert lengths == set(range(2, 9))
    orc = OracleRobot(KUKA_KIN)
    ch, nlp = FoldedChain(orc, LINK), IKExampleNLP(orc, LINK)
    # bounds active: the limits narrowed to nominal +- 0.45 (test_active_limits_match_the_port)
    lo, up = np.maximum(nlp.lo, NOMINAL - 0.45), np.minimum(nlp.up, NOMINAL + 0.45)
    qn = np.clip(NOMINAL + rng.uniform(-0.3, 0.3, (B_KUKA, 7)), lo, up)
    for goal, g in _goal_rows(orc, LINK, ch, np.clip(qn + rng.uniform(-0.5, 0.5, (B_KUKA, 7)), lo, up)).items():
        cases.append(("narrow", goal, KUKA_KIN, LINK, lo, up, 300, qn, np.concatenate([qn, g], 1)))
    # the six instances of test_non_finite_inputs_are_reported_as_in_the_position_kernel (position: its first ten columns, as there) / ..._as_in_the_siblings
    qn, pg, qg = pose_ik_ref.kuka_batch(np.random.default_rng(SEED + 214), ch, orc, LINK, 6, NOMINAL, nlp.lo, nlp.up)
    batches = {"pose": (qn, np.concatenate([qn, pg, qg], 1))}
    qn, pg, ug = axis_ik_ref.kuka_batch(np.random.default_rng(SEED + 314), ch, A, 6, NOMINAL, nlp.lo, nlp.up)
    batches["axis"] = (qn, np.concatenate([qn, pg, ug], 1))
    for goal, (qn, p) in batches.items():
        x0, p = qn.copy(), p.copy()
        p[1, 3] = np.inf  # nominal configuration
        p[2, 7 + 1] = np.inf  # position goal
        p[3, 7 + 3 + 2] = np.nan  # quaternion / axis goal
        x0[4, 2], x0[5, 0] = np.nan, np.inf  # seeds
        cases.append(("non_finite", goal, KUKA_KIN, LINK, nlp.lo, nlp.up, None, x0, p))
        if goal == "pose":
            cases.append(("non_finite", "position", KUKA_KIN, LINK, nlp.lo, nlp.up, None, x0, np.ascontiguousarray(p[:, :10])))
    # test_a_goal_axis_that_is_not_unit_is_infeasible_as_posed: every outer pass near the end makes no evaluation
    qn, pg, ug = axis_ik_ref.kuka_batch(np.random.default_rng(SEED + 315), ch, A, 64, NOMINAL, nlp.lo, nlp.up)
    sel = np.abs(ug).max(1) >= 0.95
    cases.append(("non_unit", "axis", KUKA_KIN, LINK, nlp.lo, nlp.up, None, qn[sel], np.concatenate([qn[sel], pg[sel], 1.1 * ug[sel]], 1)))
    return cases


def rows_outputs(cases):
    """{goal/case/output: array} through IKBackend only."""
    out, chains = {}, {}
    for case, goal, kin, link, lo, up, max_iter, x0, p in cases:
        if (kin, link) not in chains:
            chains[kin, link] = RobotModel(urdf_filename=kin).kinematic_chain(link)
        be = IKBackend(chains[kin, link], lo, up, **GOALS[goal], **({} if max_iter is None else {"max_iter": max_iter}))
        try:
            assert be.flag("ik_goal") == list(GOALS).index(goal)
            res = be.solve(x0, p)
            got = (res.x, res.f, res.kkt, res.iters, res.status) + be.multipliers(len(x0))
        finally:
            be.close()
        for name, a in zip(OUT, got):
            out["%s/%s/%s" % (goal, case, name)] = np.ascontiguousarray(a)
    return out


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.gpu
def test_one_iteration_has_the_bits_of_the_three_it_replaced(hip_lib, tmp_path):
    ref = np.load(os.path.join(GOLDEN, "ik_rows_parent_bits.npz"))
    cases = rows_cases(tmp_path)
    got = rows_outputs(cases)
    assert sorted(got) == sorted(ref.files)
    per_goal = {goal: sorted({c[0] for c in cases if c[1] == goal}) for goal in GOALS}
    assert per_goal["axis"] == sorted(per_goal["pose"] + ["non_unit"]) and per_goal["position"] == per_goal["pose"] and len(per_goal["pose"]) == 8 + 2
    # what the cases are there for happens in the pinned runs: bounds active, the non-finite statuses, the evaluation cap of the goal that cannot be met
    for goal in GOALS:
        assert ((ref[goal + "/narrow/z_lo"] > 0) | (ref[goal + "/narrow/z_up"] > 0)).any(), goal
        assert ref[goal + "/non_finite/status"][1:3].tolist() == [2, 2] and ref[goal + "/non_finite/iters"][1:3].tolist() == [1, 1], goal
    assert (ref["axis/non_unit/status"] != 0).all() and (ref["axis/non_unit/status"] == 1).any()
    differ = []
    for key in ref.files:
        if got[key].dtype != ref[key].dtype or got[key].shape != ref[key].shape or not (_bits(got[key]) == _bits(ref[key])).all():
            differ.append(key)
    print("arrays", len(ref.files), "differing", differ)
    assert not differ, differ
