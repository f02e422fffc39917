"""The torque-MPC kernels (optas_amd/csrc/oh_torque.hip: named records, one unit map, k_tq_step as its numbered steps) held to the bits of the texts they
replaced.  tests/golden/torque_parent_bits.npz was written on an MI355X by the library of the last commit whose k_tq_step was one body and whose records were
addressed by numbers, through torque_outputs() below (tools/gpu_tq_ab_dump.py pin).  B = 5 instances of T = 11 knots unless a case says otherwise: 55 units
fill no whole number of wavefronts at any chain length (64 / N = 32, 21, 16, 12, 10, 9 units per wavefront), so the last wavefront is partial and instances
share wavefronts everywhere.  Cases: every chain length from 2 to 7 with effort limits far away and binding, each stopped after 1, 2, 3 and 12 steps and run
to the end (intermediate iterates, not only the fixed point); velocity rows that bind and the dual-number Jacobian on 4 and 7 joints; on 7 joints the curvature
term never stored (tq_curv_lag = 0) and never used (tq_curv_from = 0); the hard-pressed velocity rows (the re-evaluation branch of the barrier update); initial
velocities outside their limits; non-finite seeds; the receding horizon on the device on 5 joints (warm barrier parameter, tq_mu_dec_warm).  Outputs only; the
inputs come from the seeds.  x is pinned where a solve runs to its end, every other array also at the caps (pinned()).  Equality of every array as integers."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, MED7_KIN, SEED
from optas_amd.backend import TorqueBackend
from optas_amd.models import RobotModel
from oracle.problems import TorqueMPCNLP
from oracle.robot import OracleRobot
from oracle.torque import TorqueProblem
from oracle.torque_ipm import solve_torque_ipm
from test_gpu_torque_chain_lengths import W, _binding_limits, _robots

B, T = 5, 11
CAPS = (1, 2, 3, 12, None)  # max_iter; None: the backend's default
MED7 = ("med7", MED7_KIN, "lbr_link_ee", np.deg2rad([0, 45, 0, -90, 0, -45, 0]))
OUT = ("x", "f", "kkt", "iters", "status", "mult")
OUT_ROLLOUT = ("states", "tau0", "f", "iters", "status")


def _batch(orc, link, lim, qn, rng, T=T, B=B):
    """Seeds and goals as test_every_chain_length_equals_the_port_and_is_a_kkt_point_of_the_literal_problem draws them."""
    n = orc.ndof
    prob = TorqueProblem(orc, link, T=T, dt=0.1, tau_lim=lim, **W)
    nlp = TorqueMPCNLP(prob)
    qc = qn + np.concatenate([np.zeros((1, n)), rng.uniform(-0.1, 0.1, (B - 1, n))])
    goal = np.stack([prob.goal_figure_eight(q, scale=0.5) for q in qc])
    return np.stack([nlp.seed(q) for q in qc]), np.stack([nlp.pack_p(qc[b], np.zeros(n), goal[b]) for b in range(len(qc))])


def torque_cases(tmp_path):
    """[(case, kinematics file, link, T, TorqueBackend arguments, options, x0, p)]; for the rollout case x0 is the plants' state and p the goal table."""
    cases = []
    rng = np.random.default_rng(SEED + 40)
    inputs = {}
    for tag, kin, link, qn in _robots(tmp_path) + [MED7]:  # 2 .. 7 joints
        orc = OracleRobot(kin)
        n = orc.ndof
        for lname, lim in (("far", np.full(n, 1e3)), ("binding", _binding_limits(orc, link, qn))):
            x0, p = _batch(orc, link, lim, qn, rng)
            inputs[tag, lname] = (kin, link, lim, x0, p)
            for cap in CAPS:
                kw = dict(tau_lo=-lim, tau_up=lim, **({} if cap is None else {"max_iter": cap}))
                cases.append(("length_%s_%s_%s" % (tag, lname, "end" if cap is None else "cap%d" % cap), kin, link, T, kw, {}, x0, p))
    assert sorted(OracleRobot(k).ndof for (_, l), (k, *_) in inputs.items() if l == "far") == list(range(2, 8))
    for tag in ("med4", "med7"):
        kin, link, lim, x0, p = inputs[tag, "binding"]
        n = OracleRobot(kin).ndof
        # velocity rows that bind (test_dual_number_path_and_velocity_rows_on_a_short_chain): 0.8 of the fastest joint of the plan without them -- the
        # numpy port's plan here, so that the cases do not depend on a device run
        prob = TorqueProblem(OracleRobot(kin), link, T=T, dt=0.1, tau_lim=lim, **W)
        vmax = 0.8 * max(np.abs(solve_torque_ipm(prob, p[b, :n], np.zeros(n), p[b, 2 * n :].reshape(T, 3))["dQ"]).max() for b in range(2))
        cases.append(("velocity_" + tag, kin, link, T, dict(tau_lo=-lim, tau_up=lim, dq_lo=-vmax, dq_up=vmax), {}, x0, p))
        cases.append(("jac_dual_" + tag, kin, link, T, dict(tau_lo=-lim, tau_up=lim), {"tq_jac_dual": 1}, x0, p))
    kin, link, lim, x0, p = inputs["med7", "binding"]
    cases.append(("curv_lag0_med7", kin, link, T, dict(tau_lo=-lim, tau_up=lim), {"tq_curv_lag": 0}, x0, p))
    cases.append(("curv_from0_med7", kin, link, T, dict(tau_lo=-lim, tau_up=lim), {"tq_curv_from": 0}, x0, p))
    # the six instances of test_hard_pressed_velocity_rows_leave_the_relaxed_zone (T = 30, 600 steps: the re-evaluation under a lower barrier parameter)
    orc = OracleRobot(MED7_KIN)
    QC = np.deg2rad([0, 30, 0, -90, 0, -30, 0])
    prob = TorqueProblem(orc, MED7[2], T=30, dt=0.1, tau_lim=58.0, **W)
    qc = QC[None] + np.concatenate([np.zeros((1, 7)), np.random.default_rng(SEED + 9).uniform(-0.05, 0.05, (5, 7))])
    goal = np.stack([prob.goal_figure_eight(q) for q in qc])
    x0 = np.zeros((6, 4 * 7 * 30))
    x0[:, : 7 * 30] = np.tile(qc, (1, 30))
    cases.append(("hard_pressed", MED7_KIN, MED7[2], 30, dict(tau_lo=-58.0, tau_up=58.0, dq_lo=-0.2, dq_up=0.2, max_iter=600), {},
                  x0, np.ascontiguousarray(np.concatenate([qc, np.zeros((6, 7)), goal.reshape(6, -1)], 1))))
    # the six instances of test_initial_velocity_outside_its_limits_is_reported_infeasible
    dqc = np.zeros((6, 7))
    dqc[2, 3], dqc[4, 0] = 0.8, -0.51
    goal = np.stack([TorqueProblem(orc, MED7[2], T=12, dt=0.1, tau_lim=58.0, **W).goal_figure_eight(QC)] * 6)  # (the oracle's goal: the cases need no device)
    cases.append(("infeasible", MED7_KIN, MED7[2], 12, dict(tau_lo=-58.0, tau_up=58.0, dq_lo=-0.5, dq_up=0.5, max_iter=300), {},
                  np.zeros((6, 4 * 7 * 12)), np.concatenate([np.tile(QC, (6, 1)), dqc, goal.reshape(6, -1)], 1)))
    # seeds with a NaN in one instance and an Inf in another, in the ddQ block (the only block of a seed the family reads)
    kin, link, lim, x0, p = inputs["med7", "far"]
    x0 = x0.copy()
    x0[1, 2 * 7 * T + 7 * 3 + 2] = np.nan
    x0[3, 2 * 7 * T + 7 * 9 + 6] = np.inf
    cases.append(("non_finite", kin, link, T, dict(tau_lo=-lim, tau_up=lim), {}, x0, p))
    # oh_tq_rollout on the 5-joint arm: 3 plants, 4 ticks, advance = 1 (goal table as test_closed_loop_on_the_device_equals_the_port_on_a_five_joint_arm)
    kin, link, lim, _, _ = inputs["med5", "binding"]
    prob = TorqueProblem(OracleRobot(kin), link, T=T, dt=0.1, tau_lim=lim, **W)
    q0 = np.deg2rad([0, 45, 0, -90, 0]) + np.array([[0.0] * 5, [0.05, -0.04, 0.03, 0.02, -0.05], [-0.03, 0.02, 0.05, -0.04, 0.01]])
    e, Re, _, _ = prob.chain.fk(q0)
    ts = np.arange(4 + T) * 0.1
    loc = 0.5 * np.stack([0.2 * np.sin(ts * np.pi * 0.5), 0.1 * np.sin(ts * np.pi), np.zeros_like(ts)], 1)
    cases.append(("rollout_med5", kin, link, T, dict(tau_lo=-lim, tau_up=lim), {"ticks": 4, "advance": 1},
                  np.concatenate([q0, np.zeros((3, 5))], 1), np.stack([e[b][None] + loc @ Re[b].T for b in range(3)])))
    return cases


def torque_outputs(cases):
    """{case/output: array} through TorqueBackend only."""
    out, models = {}, {}
    for case, kin, link, T_, kw, options, x0, p in cases:
        if kin not in models:
            robot = RobotModel(urdf_filename=kin, time_derivs=[0, 1, 2])
            models[kin] = (robot.kinematic_chain(link), robot.dynamics_tables())
        be = TorqueBackend(*models[kin], T=T_, dt=0.1, **W, **kw)
        try:
            if case.startswith("rollout"):
                names, got = OUT_ROLLOUT, be.rollout(x0, p, options["ticks"], advance=options["advance"])
            else:
                be.set_options(options)
                res = be.solve(x0, p)
                names, got = OUT, (res.x, res.f, res.kkt, res.iters, res.status, be.multipliers(len(x0)))
        finally:
            be.close()
        for name, a in zip(names, got):
            out["%s/%s" % (case, name)] = np.ascontiguousarray(a)
    return out


def pinned(key):
    """x where the solve ran to its end; every other array at the caps as well (the file stays small)."""
    case, name = key.split("/")
    return name != "x" or "_cap" not in case


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


@pytest.mark.gpu
def test_the_step_functions_and_named_records_have_the_bits_of_the_texts_they_replaced(hip_lib, tmp_path):
    ref = np.load(os.path.join(GOLDEN, "torque_parent_bits.npz"))
    cases = torque_cases(tmp_path)
    got = {k: v for k, v in torque_outputs(cases).items() if pinned(k)}
    assert sorted(got) == sorted(ref.files)
    assert len(cases) == 6 * 2 * len(CAPS) + 4 + 2 + 4
    # what the cases are there for happens in the pinned runs
    ends = [c[0] for c in cases if c[0].startswith("length_") and c[0].endswith("_end")]
    assert any(len(set(ref[c + "/iters"].tolist())) > 1 for c in ends)  # the running list was rebuilt: launches over fewer instances than the batch
    binding = [ref[c + "/mult"] for c in ends if "_binding_" in c]
    # (per case the criterion of test_gpu_torque_chain_lengths.py; in absolute terms the 2-joint robot's largest multiplier is 2.9e-4 -- its torques are a few
    #  N m and the cost pushes with 2 w_tau tau -- and those of the longer chains 0.015 ... 0.22)
    assert len(binding) == 6 and all(lam.max() > 1e3 * np.median(lam) for lam in binding) and sum(lam.max() > 1e-3 for lam in binding) == 5
    for c in [c[0] for c in cases if "_cap" in c[0]]:
        cap = int(c.rsplit("cap", 1)[1])
        assert (ref[c + "/iters"] == np.minimum(cap, ref[c.rsplit("_", 1)[0] + "_end/iters"])).all() and (cap > 3 or ref[c + "/status"].tolist() == [1] * B), c
    for tag, n in (("med4", 4), ("med7", 7)):
        assert ref["velocity_%s/mult" % tag].shape == (B, T, 4 * n) and ref["velocity_%s/mult" % tag][:, :, 2 * n :].max() > 1e-3
    for c, base in (("jac_dual_med4", "length_med4_binding_end"), ("jac_dual_med7", "length_med7_binding_end"), ("curv_lag0_med7", "length_med7_binding_end"),
                    ("curv_from0_med7", "length_med7_binding_end")):
        assert any(not _same(ref[c + "/" + name], ref[base + "/" + name]) for name in OUT), c
    assert (ref["non_finite/status"][[1, 3]] == 2).all() and (ref["non_finite/status"][[0, 2, 4]] == 0).all()
    assert ref["infeasible/status"][[2, 4]].tolist() == [3, 3] and (np.delete(ref["infeasible/status"], [2, 4]) != 3).all()
    assert ref["hard_pressed/mult"][:, :, 14:].max() > 1e-3 and ref["rollout_med5/iters"].shape == (4, 3)
    differ = [key for key in ref.files if not _same(got[key], ref[key])]
    print("arrays", len(ref.files), "differing", differ)
    assert not differ, differ
