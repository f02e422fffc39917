#!/usr/bin/env python
"""Bits, device times and kernel facts of the torque-MPC family for comparing two builds of the library (OPTAS_HIP_LIBRARY selects the other one) after a
change that must alter none of them.  One process per library and call:

  pin OUT.npz [all]   the output arrays of tests/test_gpu_torque_bits.py:torque_outputs on its torque_cases that the test compares (pinned()): what
                      tests/golden/torque_parent_bits.npz holds, written from the parent's library.  `all`: every array, x at the caps included.
  time OUT.json LEG   device times (ms, the handle's event timer, 5 solves after 2 warm-ups) of the med7 cold solve of config 5 as tools/bench_configs.py
                      poses it at B = 8192, 1024 and 1, of the same with velocity rows at B = 8192 and of oh_tq_rollout on 1024 plants x 10 ticks; one more
                      solve per point with profiling on gives the evaluation pair's and the step kernel's ms per launch (oh_get_timing [0]/[1], [2]/[3]);
                      the oh_kernel_info of every k_tq_{eval,curv,step}_N the library answers for.  LEG: parent, parent_again or new.
  report TIMES...     per point, the new library's median against the parent's maximum, and the same for the parent_again legs (the criterion's own noise);
                      the kernel facts of both libraries side by side (waves per SIMD, scratch, LDS) -> profiles/tq_steps_ab.json.  Exit status 1 if a
                      point or a kernel fact misses.
"""
import ctypes as C
import json
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, d)
KERNELS = [f"{k}_{n}" for k in ("k_tq_eval", "k_tq_curv", "k_tq_step") for n in range(2, 8)] + ["k_tq_eval", "k_tq_curv", "k_tq_step"]
SEED, REPEATS = 20261020, 5


def pin(path, everything=False):
    import test_gpu_torque_bits as tb

    with tempfile.TemporaryDirectory() as tmp:
        out = tb.torque_outputs(tb.torque_cases(pathlib.Path(tmp)))
    if not everything:
        out = {k: v for k, v in out.items() if tb.pinned(k)}
    np.savez_compressed(path, **out)
    print("pinned", len(out), "arrays to", path, os.path.getsize(path), "bytes")


def _config5(med7, link, B, T, dt, rows):
    """qc, the goal table of `rows` knots and the rest pose of config 5 (tools/bench_configs.py:_torque)."""
    qn = np.deg2rad([0, 30, 0, -90, 0, -30, 0])
    qc = np.atleast_2d(qn + (np.random.default_rng(SEED + B).uniform(-0.1, 0.1, (B, 7)) if B > 1 else 0.0))
    ts = np.arange(rows) * dt
    loc = np.stack([0.2 * np.sin(ts * np.pi * 0.5), 0.1 * np.sin(ts * np.pi), np.zeros(rows)])
    pose, _ = med7._kin(link).fk_jac(qc, want_jac=False)
    x, y, z, w = pose[:, 3], pose[:, 4], pose[:, 5], pose[:, 6]
    Re = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                   np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                   np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)
    return qc, np.ascontiguousarray(pose[:, None, :3] + np.einsum("bij,jt->bti", Re, loc))


def _per_launch(be):
    out = (C.c_double * 14)()
    from optas_amd import _lib

    _lib.check(_lib.load().oh_get_timing(be._h, out), "oh_get_timing")
    return {"eval_pair_ms_per_launch": out[0] / max(out[1], 1.0), "step_ms_per_launch": out[2] / max(out[3], 1.0), "launches": int(out[1])}


def time_points(path, leg):
    from optas_amd import _lib
    from optas_amd.backend import TorqueBackend
    from optas_amd.models import RobotModel

    med7 = RobotModel.builtin("med7")
    link, T, dt = "lbr_link_ee", 30, 0.1
    mk = lambda **kw: TorqueBackend(med7.kinematic_chain(link), med7.dynamics_tables(), T=T, dt=dt, w_path=1000.0, w_vel=0.1, w_tau=1e-4, tau_lo=-58.0, tau_up=58.0, max_iter=600, **kw)
    pts = {}
    for name, B, kw in (("cold_b8192", 8192, {}), ("cold_b1024", 1024, {}), ("cold_b1", 1, {}), ("velocity_b8192", 8192, dict(dq_lo=-0.5, dq_up=0.5))):
        qc, goal = _config5(med7, link, B, T, dt, T)
        p = np.ascontiguousarray(np.concatenate([qc, np.zeros((B, 7)), goal.reshape(B, -1)], 1))
        x0 = np.zeros((B, 4 * 7 * T))
        x0[:, : 7 * T] = np.tile(qc, (1, T))
        be = mk(**kw)
        bufs = [_lib.DeviceBuffer(a.nbytes).upload(a) for a in (x0, p)] + [_lib.DeviceBuffer(n) for n in (x0.nbytes, 8 * B, 24 * B, 4 * B, 4 * B)]
        ms = []
        for k in range(2 + REPEATS):
            be.solve_device(B, *bufs)
            if k >= 2:
                ms.append(float(be.solve_ms()))
        be.set_profiling(True)
        be.solve_device(B, *bufs)
        prof = _per_launch(be)
        be.set_profiling(False)
        it, st = bufs[5].download(np.int32, (B,)), bufs[6].download(np.int32, (B,))
        pts[name] = {"ms": ms, **prof, "steps_sum": int(it.sum()), "steps_max": int(it.max()), "ok": float(_lib.status_ok(st).mean())}
        for b in bufs:
            b.free()
        be.close()
        print(name, pts[name], flush=True)
    B, ticks = 1024, 10
    qc, table = _config5(med7, link, B, T, dt, ticks + T)
    st0 = np.concatenate([qc, np.zeros((B, 7))], 1)
    be = mk()
    ms = []
    for k in range(1 + REPEATS):
        _, _, _, it, st = be.rollout(st0, table, ticks)
        if k >= 1:
            ms.append(float(be.timing()["solve_ms"]))
    pts["rollout_b1024_t10"] = {"ms": ms, "steps_sum": int(it.sum()), "steps_max": int(it.max()), "ok": float(_lib.status_ok(st).mean())}
    be.close()
    print("rollout_b1024_t10", pts["rollout_b1024_t10"], flush=True)
    kernels = {}
    for k in KERNELS:
        try:
            kernels[k] = _lib.kernel_info(k)
        except _lib.OptasHipError:
            pass  # (a library from before the per-chain-length names)
    with open(path, "w") as f:
        json.dump({"leg": leg, "library": os.environ.get("OPTAS_HIP_LIBRARY", "in-tree"), "points": pts, "kernels": kernels}, f, indent=1)


def report(files):
    runs, kernels = {"parent": {}, "parent_again": {}, "new": {}}, {}
    for path in files:
        rec = json.load(open(path))
        assert (rec["leg"] == "new") == (rec["library"] == "in-tree"), path
        kernels["new" if rec["leg"] == "new" else "parent"] = rec["kernels"]
        for k, v in rec["points"].items():
            e = runs[rec["leg"]].setdefault(k, {"ms": [], "eval_pair_ms_per_launch": [], "step_ms_per_launch": [], "steps_sum": v["steps_sum"], "steps_max": v["steps_max"]})
            e["ms"].extend(v["ms"])
            for q in ("eval_pair_ms_per_launch", "step_ms_per_launch"):
                if q in v:
                    e[q].append(v[q])
    points = {}
    for k, pa in runs["parent"].items():
        points[k] = {"parent_ms": pa["ms"], "parent_max_ms": max(pa["ms"])}
        for leg in ("new", "parent_again"):
            r = runs[leg][k]
            points[k].update({leg + "_ms": r["ms"], leg + "_median_ms": float(np.median(r["ms"])), leg + "_holds": bool(np.median(r["ms"]) <= max(pa["ms"])),
                              leg + "_same_steps": (r["steps_sum"], r["steps_max"]) == (pa["steps_sum"], pa["steps_max"])})
        for q in ("eval_pair_ms_per_launch", "step_ms_per_launch"):
            if pa[q]:
                points[k][q] = {leg: float(np.median(runs[leg][k][q])) for leg in runs}
        points[k]["verdict"] = "holds" if points[k]["new_holds"] else ("noise: parent_again misses too" if not points[k]["parent_again_holds"] else "slower")
    facts = {}
    for k, nw in kernels["new"].items():
        pa = kernels["parent"].get(k)
        facts[k] = {"new": nw, "parent": pa}
        if pa is not None:
            facts[k]["holds"] = bool(nw["waves_per_simd"] == pa["waves_per_simd"] and nw["scratch_bytes_per_lane"] <= pa["scratch_bytes_per_lane"]
                                     and nw["lds_bytes_per_block"] == pa["lds_bytes_per_block"])
    res = {"source": "tools/gpu_tq_ab_dump.py", "robot": "med7, T = 30, effort limits 58 N m (config 5 of tools/bench_configs.py)",
           "timer": "oh_get_timing out[4] (HIP events around the solve's launches); per process 5 solves after 2 warm-ups (rollout: 5 after 1)",
           "speed_criterion": "per point, the new library's median over its runs <= the parent's maximum over its runs; processes alternated parent, new, parent_again; "
                              "parent_again is the parent's library once more, held to the same criterion: a point it misses too is noise",
           "kernel_criterion": "per kernel, the parent's waves per SIMD, no more scratch, the same LDS",
           "points": points, "kernels": facts}
    with open(os.path.join(ROOT, "profiles", "tq_steps_ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["parent_max_ms"], v["new_median_ms"], v["parent_again_median_ms"], v["verdict"]) for k, v in points.items()}, indent=1))
    print("kernel facts missing:", [k for k, v in facts.items() if not v.get("holds", True)], "without a parent value:", [k for k, v in facts.items() if v["parent"] is None])
    ok = all(v["verdict"] != "slower" and v["new_same_steps"] for v in points.values()) and all(v.get("holds", True) for v in facts.values())
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "pin":
        pin(sys.argv[2], everything=sys.argv[3:] == ["all"])
    elif sys.argv[1] == "time":
        time_points(sys.argv[2], sys.argv[3])
    else:
        sys.exit(report(sys.argv[2:]))
