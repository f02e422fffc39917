#!/usr/bin/env python
"""Device time of the dense Lagrangian Hessian through oh_tape_hvp (k_tape_hvp) -> profiles/tape_hvp_rates.json.  Recorded, nothing asserted.

  * the 7-joint IK tape (examples/example.py) at B = 65 536;
  * the joint-space planner's tape as written (examples/simple_joint_space_planner.py, 280 variables) at B = 256.

Next to each, what a user had before the entry existed for the same matrix: 2 nx calls of oh_tape_probe at x +- h e_k (central differences of the
gradient; host wall time, every call ends in a device synchronise and a copy back), and how far the two matrices are apart.  The work-area budget
(option tape_hvp_work_mb) is the default 256 MB, and 4096 MB beside it: the budget decides how many lanes a launch has.

oh_tape_hvp: device time is the handle's event timer around its launches (oh_get_timing out[4]), wall time the host clock around the whole call
(copies in, launches, the copy of [B][nx][nx] back).  Two warm-up calls, then the median of the repeats with min and max.  Every step is a child
process under a time limit of its own; the chain stops at the first step that fails."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "profiles", "tape_hvp_rates.json")
STEPS = [("ik", 240), ("planner", 420)]


def _stats(ms):
    import numpy as np

    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "repeats": len(ms)}


def _workload(name):
    import numpy as np

    from optas_amd.tape import compile_problem

    golden = os.path.join(ROOT, "tests", "golden")
    rng = np.random.default_rng(7)
    if name == "ik":
        from examples.example import setup_solver

        g = np.load(os.path.join(golden, "ik_golden.npz"))
        B = 65536
    else:
        from examples.simple_joint_space_planner import setup_solver

        g = np.load(os.path.join(golden, "planner_golden.npz"))
        B = 256
    tp = compile_problem(setup_solver(build_only=True)[1])
    idx = np.arange(B) % len(g["x"])
    x = g["x"][idx] + rng.uniform(-1e-3, 1e-3, (B, int(tp.nx)))  # around the recorded optima
    p = np.ascontiguousarray(g["p"][idx])
    ni, ne = int(tp.n_ineq), int(tp.n_eq)
    seeds = np.concatenate([np.ones((B, 1)), -rng.uniform(0.0, 1.0, (B, ni)), -rng.uniform(-1.0, 1.0, (B, ne))], axis=1)  # (1, -lam, -mu)
    return tp, B, x, p, seeds


def step(name):
    import numpy as np

    from optas_amd.backend import TapeBackend

    tp, B, x, p, seeds = _workload(name)
    nx = int(tp.nx)
    be = TapeBackend(tp, jit=False, wave=False, metric=False)  # (oh_tape_hvp and oh_tape_probe run the interpreter on the handle's tape whatever its solves use)
    out = {"B": B, "nx": nx, "tape_len": len(tp.op), "n_ineq": int(tp.n_ineq), "n_eq": int(tp.n_eq), "units": B * nx,
           "work_area_mb_default": be.get_option("tape_hvp_work_mb"), "work_doubles_per_unit": 4 * len(tp.op) + 3 * nx}
    for key, mb in (("budget_4096_mb", 4096), ("", 256)):  # the default budget last: its figures are the headline ones, H is its matrix
        be.set_option("tape_hvp_work_mb", mb)
        dev, wall = [], []
        for rep in range(2 + 5):
            t0 = time.perf_counter()
            H = be.hessian(x, p, seeds)
            t1 = time.perf_counter()
            if rep >= 2:
                dev.append(be.solve_ms())
                wall.append(1e3 * (t1 - t0))
        rec = {"launches": be.flag("tape_hvp_launches"), "hvp_device": _stats(dev), "hvp_wall": _stats(wall)}
        if key:
            out[key] = rec
        else:
            out.update(rec)
    out["asymmetry_max"] = float(np.abs(H - H.transpose(0, 2, 1)).max())
    h = 1e-5
    fd_wall = []
    Hfd = np.empty_like(H)
    for rep in range(1 + 3):
        t0 = time.perf_counter()
        for k in range(nx):
            xp, xm = x.copy(), x.copy()
            xp[:, k] += h
            xm[:, k] -= h
            gp = be.probe(xp, p, None, seeds)[2]
            gm = be.probe(xm, p, None, seeds)[2]
            Hfd[:, k, :] = (gp - gm) / (2.0 * h)
        if rep >= 1:
            fd_wall.append(1e3 * (time.perf_counter() - t0))
    out["probe_differences_wall"] = _stats(fd_wall)
    out["probe_calls"] = 2 * nx
    out["difference_max_rel"] = float(np.abs(H - Hfd).max() / max(1.0, np.abs(H).max()))
    out["wall_ratio_differences_over_hvp"] = out["probe_differences_wall"]["median_ms"] / out["hvp_wall"]["median_ms"]
    be.close()
    return out


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        sys.path.insert(0, ROOT)
        print("RESULT " + json.dumps(step(sys.argv[2])))
        return 0
    res = {"source": "tools/gpu_tape_hvp_rates.py",
           "timer": "hvp_device: oh_get_timing out[4], events around the launches of k_tape_hvp; *_wall: host clock around the calls (copies included); "
                    "median after warm-up, min and max beside it", "workloads": {}}
    for name, limit in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {name}: time limit of {limit} s; stopping", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"step {name}: exit {p.returncode}; stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return p.returncode
        val = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        res["workloads"][name] = val
        print(name, json.dumps(val), flush=True)
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
