#!/usr/bin/env python
"""Bits and device times of the inverse-kinematics family for comparing two builds of the library (OPTAS_HIP_LIBRARY selects the other one) after a
change that must alter neither.  One process per library and call:

  pin OUT.npz      every output array of tests/test_gpu_ik_rows_bits.py:rows_outputs on its rows_cases: what that test compares against
                   (tests/golden/ik_rows_parent_bits.npz, written from the parent's library).
  time OUT.json    7 device times (ms, the handle's event timer, after 2 warm-up solves) of the position, the pose and the axis ('z') problem on the
                   KUKA, on the batches of tools/gpu_ik_axis_rates.py at B = 4096 and 65 536; the oh_kernel_info of all 21 IK instantiations.
  report TIMES...  per point, the new library's median against the parent's maximum (TIMES: the json files of `time`, told apart by their "library"
                   entry; several per library are pooled) -> profiles/ik_rows_ab.json with both sets of times and both libraries' kernel facts.
                   Exit status 1 if a point is slower.
"""
import json
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, d)
KERNELS = [f"{k}_{n}" for k in ("k_ik_solve", "k_ik_pose_solve", "k_ik_axis_solve") for n in range(2, 9)]


def pin(path):
    import test_gpu_ik_rows_bits as rb

    with tempfile.TemporaryDirectory() as tmp:
        out = rb.rows_outputs(rb.rows_cases(pathlib.Path(tmp)))
    np.savez_compressed(path, **out)
    print("pinned", len(out), "arrays to", path, os.path.getsize(path), "bytes")


def time_points(path):
    import gpu_ik_axis_rates as ar
    from examples import axis_ik
    from optas_amd import _lib
    from optas_amd.backend import IKBackend
    from optas_amd.models import RobotModel

    robot = RobotModel.builtin("kuka_lwr")
    chain = robot.kinematic_chain(ar.LINK)
    lo, up = np.asarray(robot.lower_actuated_joint_limits, float).reshape(-1), np.asarray(robot.upper_actuated_joint_limits, float).reshape(-1)
    nominal = np.deg2rad(axis_ik.NOMINAL_DEG)
    pts = {}
    for B in (4096, 65536):
        rng = np.random.default_rng(20261020 + B)
        qn = nominal + rng.uniform(-0.3, 0.3, (B, 7))
        qgoal = np.clip(qn + rng.uniform(-0.5, 0.5, (B, 7)), lo, up)
        pose = np.ascontiguousarray(robot._kin(ar.LINK).fk_jac(qgoal, want_jac=False)[0])
        ug = np.ascontiguousarray(np.asarray(robot.get_global_link_axis(ar.LINK, qgoal.T, axis_ik.AXIS)).T)
        for leg, kw, goal in (("position", {}, pose[:, :3]), ("pose", {"orientation": True}, pose), ("axis", {"axis": axis_ik.AXIS}, np.concatenate([pose[:, :3], ug], 1))):
            be = IKBackend(chain, lo, up, max_iter=300, **kw)
            p = np.concatenate([qn, goal], 1)
            for _ in range(2):
                be.solve(qn, p)
            ms = []
            for _ in range(ar.REPEATS):
                res = be.solve(qn, p)
                ms.append(float(be.solve_ms()))
            be.close()
            pts["%s_b%d" % (leg, B)] = {"ms": ms, "evaluations_p50": int(np.median(res.iters)), "evaluations_max": int(res.iters.max()), "converged": float((res.status == 0).mean())}
            print(leg, B, pts["%s_b%d" % (leg, B)], flush=True)
    with open(path, "w") as f:
        json.dump({"library": os.environ.get("OPTAS_HIP_LIBRARY", "in-tree"), "points": pts, "kernels": {k: _lib.kernel_info(k) for k in KERNELS}}, f, indent=1)


def report(files):
    runs = {"parent": {}, "new": {}}
    kernels = {}
    for path in files:
        rec = json.load(open(path))
        side = "new" if rec["library"] == "in-tree" else "parent"
        kernels[side] = rec["kernels"]
        for k, v in rec["points"].items():
            e = runs[side].setdefault(k, {"ms": [], "evaluations_p50": v["evaluations_p50"], "evaluations_max": v["evaluations_max"]})
            assert (e["evaluations_p50"], e["evaluations_max"]) == (v["evaluations_p50"], v["evaluations_max"]), (path, k)
            e["ms"].extend(v["ms"])
    points = {}
    for k, nw in runs["new"].items():
        pa = runs["parent"][k]
        points[k] = {"parent_ms": pa["ms"], "new_ms": nw["ms"], "parent_max_ms": max(pa["ms"]), "new_median_ms": float(np.median(nw["ms"])),
                     "holds": bool(np.median(nw["ms"]) <= max(pa["ms"])), "evaluations_p50": (pa["evaluations_p50"], nw["evaluations_p50"]),
                     "evaluations_max": (pa["evaluations_max"], nw["evaluations_max"])}
    res = {"source": "tools/gpu_ik_ab_dump.py", "robot": "kuka_lwr", "timer": "oh_get_timing out[4] (HIP events around the solve's launches); per process 7 solves after 2 warm-ups",
           "speed_criterion": "per point, the new library's median over its runs <= the parent's maximum over its runs; processes of the two libraries alternated",
           "points": points, "kernels_new": kernels["new"], "kernels_parent": kernels["parent"]}
    with open(os.path.join(ROOT, "profiles", "ik_rows_ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["parent_max_ms"], v["new_median_ms"], v["holds"]) for k, v in points.items()}, indent=1))
    return 0 if all(v["holds"] for v in points.values()) else 1


if __name__ == "__main__":
    if sys.argv[1] == "pin":
        pin(sys.argv[2])
    elif sys.argv[1] == "time":
        time_points(sys.argv[2])
    else:
        sys.exit(report(sys.argv[2:]))
