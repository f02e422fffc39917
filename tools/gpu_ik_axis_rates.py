#!/usr/bin/env python
"""Device time of inverse kinematics with a position goal and a link-axis goal (oh_ik_set_axis_goal, k_ik_axis_solve) -> profiles/ik_axis_rates.json.
Recorded, nothing asserted.

KUKA LWR, link end_effector_ball, axis 'z', the batch distribution of tests/test_gpu_ik.py::test_large_batch_properties with a link axis: q_nominal =
nominal + U(+-0.3), goal = position and axis at clip(q_nominal + U(+-0.5)), seed q_nominal; B = 4096 and 65 536.  Four legs in one process:

  (a) axis      the axis problem on the IK family (six equality rows);
  (b) position  the position problem on the same q_nominal / position goals (k_ik_solve);
  (c) pose      the full-pose problem on the same configurations' poses (k_ik_pose_solve);
  (d) tape      the same axis problem through the generic tape family with HIPSolver's defaults for it -- the route it takes when match_ik refuses it.

The figure is the device time of the solve's launches between the handle's HIP events (oh_get_timing out[4]); two warm-up solves, then REPEATS
timed ones: median, minimum, maximum.  Evaluations p50 / max and the converged share stand beside each leg, and the code-object facts of the
axis instantiations.  "reroute_default" records the rule the re-route follows: on by default only if (a) is faster than (d) with the two min-max
ranges apart.  Usage: gpu_ik_axis_rates.py [--skip-tape-large]  (the tape leg at B = 65 536 is the long one)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "ik_axis_rates.json")
REPEATS = 7
LINK = "end_effector_ball"


def _timed(be, x0, p, repeats=REPEATS, warmup=2):
    for _ in range(warmup):
        res = be.solve(x0, p)
    ms = []
    for _ in range(repeats):
        res = be.solve(x0, p)
        ms.append(be.solve_ms())
    ok = res.status == 0
    B = len(x0)
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "repeats": repeats,
            "solves_per_s_median": B / (float(np.median(ms)) * 1e-3), "evaluations_p50": int(np.median(res.iters)), "evaluations_max": int(res.iters.max()),
            "converged": float(ok.mean())}, res


def main():
    from examples import axis_ik
    from optas_amd import _lib
    from optas_amd.backend import IKBackend, tape_backend, tape_default_max_iter
    from optas_amd.lowering import match_tape
    from optas_amd.models import RobotModel

    robot = RobotModel.builtin("kuka_lwr")
    chain = robot.kinematic_chain(LINK)
    lo, up = np.asarray(robot.lower_actuated_joint_limits, float).reshape(-1), np.asarray(robot.upper_actuated_joint_limits, float).reshape(-1)
    nominal = np.deg2rad(axis_ik.NOMINAL_DEG)
    tape = match_tape(axis_ik.setup_solver(build_only=True)[1]).tape
    out = {"robot": "kuka_lwr", "link": LINK, "axis": axis_ik.AXIS, "timer": "oh_get_timing out[4] (HIP events around the solve's launches)", "batches": {},
           "kernels": {f"k_ik_axis_solve_{n}": _lib.kernel_info(f"k_ik_axis_solve_{n}") for n in range(2, 9)}}
    for B in (4096, 65536):
        rng = np.random.default_rng(20261020 + B)
        qn = nominal + rng.uniform(-0.3, 0.3, (B, 7))
        qgoal = np.clip(qn + rng.uniform(-0.5, 0.5, (B, 7)), lo, up)
        pose = np.ascontiguousarray(robot._kin(LINK).fk_jac(qgoal, want_jac=False)[0])  # (B, 7): position, quaternion (reference sign)
        ug = np.ascontiguousarray(np.asarray(robot.get_global_link_axis(LINK, qgoal.T, axis_ik.AXIS)).T)  # (B, 3)
        legs = {}
        be = IKBackend(chain, lo, up, max_iter=300, axis=axis_ik.AXIS)
        legs["axis"], ra = _timed(be, qn, np.concatenate([qn, pose[:, :3], ug], 1))
        be.close()
        be = IKBackend(chain, lo, up, max_iter=300)
        legs["position"], _ = _timed(be, qn, np.concatenate([qn, pose[:, :3]], 1))
        be.close()
        be = IKBackend(chain, lo, up, max_iter=300, orientation=True)
        legs["pose"], _ = _timed(be, qn, np.concatenate([qn, pose], 1))
        be.close()
        if not (B > 4096 and "--skip-tape-large" in sys.argv):
            be = tape_backend(tape, max_iter=tape_default_max_iter(tape.nx), tol=1e-6, tol_feas=1e-9, jit=True)
            legs["tape"], rt = _timed(be, qn, np.concatenate([qn, pose[:, :3], ug], 1), repeats=REPEATS if B <= 4096 else 3, warmup=1)
            both = (ra.status == 0) & (rt.status == 0)
            legs["tape"]["max_abs_f_difference_where_both_converged"] = float(np.abs(ra.f - rt.f)[both].max()) if both.any() else None
            be.close()
            legs["axis_over_tape"] = legs["axis"]["median_ms"] / legs["tape"]["median_ms"]
            legs["reroute_default"] = bool(legs["axis"]["max_ms"] < legs["tape"]["min_ms"])  # (a) faster than (d), the min-max ranges apart
        legs["axis_over_position"] = legs["axis"]["median_ms"] / legs["position"]["median_ms"]
        legs["axis_over_pose"] = legs["axis"]["median_ms"] / legs["pose"]["median_ms"]
        out["batches"][str(B)] = legs
        print(B, json.dumps(legs), flush=True)
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
