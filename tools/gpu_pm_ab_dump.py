#!/usr/bin/env python
"""Bits and device times of the point-mass family for comparing two builds of the library (OPTAS_HIP_LIBRARY selects the other one) after a change
that must alter neither.  One process per library and call, each under a time limit of its own, the chain stopped at the first failure:

  pin OUT.npz      every output array of tests/test_gpu_pm_bits.py:pm_outputs on its pm_cases, after check_pinned: what that test compares against
                   (tests/golden/pm_parent_bits.npz, written from the parent's library).
  time OUT.json    7 device times (ms, the handle's event timer, after 2 warm-up solves) per point: the MPC tick at T = 20 on tools/bench_configs.py's
                   instances at B = 1, 1024, 4096 (wave kernel), 4096 with pm_wave_max 0 and 65 536 (thread kernel); T = 64 and T = 65 at B = 4096;
                   the closed loop of 10 ticks at B = 4096.  Each point with its kernel, iteration counts and converged share.
  report FILES...  per point, the new library's median against the parent's maximum; the iteration counts of the two must be equal.  Files named
                   *.remarks are the compiler's -Rpass-analysis=kernel-resource-usage output for oh_pointmass.hip (hipcc --offload-arch=gfx950 -O3
                   -std=c++17 --cuda-device-only -c, standard error kept), the parent's with "parent" in the file name.
                   -> profiles/pm_one_text_ab.json.  Exit status 1 if a point is slower, a kernel gained scratch or lost occupancy.
  pieces FILES...  the evidence for what a kernel keeps written out: json files of `time` and npz files of `pin` from libraries in which the kernel calls
                   more of oh_pm_rules.h than what ships (file names <label>_<run>.json, <label>.npz; the parent's times parent_<run>.json), with
                   label=what it calls.  Per library the arrays that differ from tests/golden/pm_parent_bits.npz and, per point, its median against the
                   parent's maximum.  -> profiles/pm_one_text_pieces.json
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, d)
from gpu_ab_common import report, timed, write_times  # noqa: E402

TICK_POINTS = [(1, None), (1024, None), (4096, None), (4096, 0.0), (65536, None)]  # (B, pm_wave_max or the default)
EDGE_HORIZONS = (64, 65)
LOOP_B, LOOP_TICKS = 4096, 10
KERNELS = {"k_pm_solve8PmParams": "k_pm_solve", "k_pm_solve_wave8PmParams": "k_pm_solve_wave"}  # in the mangled name


def pin(path):
    import test_gpu_pm_bits as pb

    cases = pb.pm_cases()
    out = pb.pm_outputs(cases)
    pb.check_pinned(out, cases)
    np.savez_compressed(path, **out)
    print("pinned", len(out), "arrays to", path, os.path.getsize(path), "bytes")


def tick_parameters(B, seed):
    """tools/bench_configs.py's instances of config 3: starts in the box outside the obstacle, a goal ramp to (1, 1)"""
    from examples.point_mass_mpc import obstacle_and_goal

    obs, _ = obstacle_and_goal(2.0, np.zeros(2))
    c = np.random.default_rng(seed).uniform(-1.2, 1.2, (2 * B + 64, 2))
    c = c[np.linalg.norm(c - obs[:, 0][None], axis=1) > 0.35][:B]
    goal = np.clip(c[:, None, :] + (1 - c[:, None, :]) * (np.arange(20) / 19.0)[None, :, None], -1.5, 1.5)  # [B][20][2]
    return np.ascontiguousarray(np.concatenate([c, np.zeros((B, 2)), goal.reshape(B, -1), np.tile(obs.T.reshape(-1), (B, 1))], 1))


def time_points(path):
    import pm_edge_cases as pe
    from conftest import SEED
    from optas_amd.backend import PointMassBackend

    pts = {}

    def point(key, be, solve, T, B, **how):
        pts[key] = timed(solve, be.solve_ms, **how)
        pts[key]["path"] = "wave" if T <= 64 and B <= int(be.get_option("pm_wave_max")) else "thread"
        be.close()
        print(key, pts[key], flush=True)

    for B, wave_max in TICK_POINTS:
        be = PointMassBackend()
        if wave_max is not None:
            be.set_options(pm_wave_max=wave_max)
        x0, p = np.zeros((B, 80)), tick_parameters(B, SEED + 3)
        point("tick_T20_b%d%s" % (B, "" if wave_max is None else "_wavemax%d" % wave_max), be, lambda: be.solve(x0, p), 20, B)
    for T in EDGE_HORIZONS:
        o = pe.gen.options("mpc", T)
        be = PointMassBackend(T=T, dt=o["dt"], w_acc=o["w_acc"], max_iter=pe.MAX_ITER, tol=pe.TOL)
        x0, p = pe.filler(T, o["dt"], LOOP_B, seed=3)
        point("tick_T%d_b%d" % (T, LOOP_B), be, lambda: be.solve(x0, p), T, LOOP_B)
    be = PointMassBackend()
    state0 = np.concatenate([tick_parameters(LOOP_B, SEED + 4)[:, 0:2], np.zeros((LOOP_B, 2))], axis=1)
    tab = pe.obstacle_table(LOOP_TICKS * 2 + 20, 0.05)
    point("rollout_T20_b%d_ticks%d" % (LOOP_B, LOOP_TICKS), be, lambda: be.rollout(state0, tab, LOOP_TICKS), 20, LOOP_B, iters=lambda r: r[2], status=lambda r: r[3])
    write_times(path, pts)


def pieces(args):
    import json

    what = dict(a.split("=", 1) for a in args if "=" in a)
    files = [a for a in args if "=" not in a]
    times = {}
    for f in (f for f in files if f.endswith(".json")):
        label = os.path.basename(f).rsplit("_", 1)[0]
        for k, v in json.load(open(f))["points"].items():
            e = times.setdefault(label, {}).setdefault(k, dict(v, ms=[]))
            assert (e["iters_sum"], e["iters_max"]) == (v["iters_sum"], v["iters_max"]), (f, k)
            e["ms"].extend(v["ms"])
    ref = np.load(os.path.join(ROOT, "tests", "golden", "pm_parent_bits.npz"))
    out = {"source": "tools/gpu_pm_ab_dump.py pieces", "criterion": "no array differs from tests/golden/pm_parent_bits.npz; per point the median <= the parent's maximum",
           "parent_max_ms": {k: max(v["ms"]) for k, v in times["parent"].items()}, "libraries": {}}
    for f in (f for f in files if f.endswith(".npz")):
        label = os.path.basename(f)[:-4]
        got = np.load(f)
        differ = sorted(k for k in ref.files if got[k].tobytes() != ref[k].tobytes())
        pts = {k: {"path": v["path"], "median_ms": float(np.median(v["ms"])), "holds": bool(np.median(v["ms"]) <= max(times["parent"][k]["ms"])), "runs": len(v["ms"])}
               for k, v in times.get(label, {}).items()}  # (a library known to move bits need not be timed)
        out["libraries"][label] = {"calls": what.get(label, ""), "arrays_differing": differ, "points": pts,
                                   "points_missed": sorted(k for k, v in pts.items() if not v["holds"])}
        print(label, "differing", len(differ), "missed", out["libraries"][label]["points_missed"])
    with open(os.path.join(ROOT, "profiles", "pm_one_text_pieces.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1] == "pin":
        pin(sys.argv[2])
    elif sys.argv[1] == "time":
        time_points(sys.argv[2])
    elif sys.argv[1] == "pieces":
        pieces(sys.argv[2:])
    else:
        sys.exit(report(sys.argv[2:], KERNELS, "tools/gpu_pm_ab_dump.py", "pm_one_text_ab.json", check_occupancy=True))
