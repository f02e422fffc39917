#!/usr/bin/env python
"""Device time of the dense Lagrangian Hessian through oh_tape_hvp on the wavefront evaluator (option tape_hvp_wave, k_tape_wave_hvp) beside the
interpreter's lanes (k_tape_hvp) -> profiles/tape_hvp_wave_rates.json.  Recorded, nothing asserted.

  (a) planner          the joint-space planner's tape as written (examples/simple_joint_space_planner.py, 280 variables), B = 256;
  (b) planner_reduced  the same problem with its affine equality rows eliminated (what the solver iterates on), B = 256;
  (c) nx65             tests/tape_cases.py:shape_tapes()["nx65"], 65 variables and a few hundred instructions, B = 4096.

Legs of one workload, all in ONE process on one library: option off (an interpreter handle of the tape, what HIPSolver.lagrangian_hessian() creates
without the option) at the default work-area budget of 256 MB and at 4096 MB; option on with the four register columns in LDS and in global memory
(tape_wave_regs 1 / 0; the global leg at the default budget).  The figure is the device time of the launches, the handle's event timer
(oh_get_timing out[4]); the host clock around the whole call stands beside it.  Two warm-up calls, then the median of five with min and max.
Every workload is a child process under a time limit of its own; the chain stops at the first one that fails."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "profiles", "tape_hvp_wave_rates.json")
STEPS = [("planner", 420), ("planner_reduced", 420), ("nx65", 240)]


def _stats(ms):
    import numpy as np

    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "repeats": len(ms)}


def _workload(name):
    import numpy as np

    rng = np.random.default_rng(7)
    if name == "nx65":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import tape_cases as tc

        tp = tc.shape_tapes()["nx65"]
        B = 4096
        x = rng.uniform(0.2, 0.9, (B, int(tp.nx)))
        p = np.zeros((B, 0))
    else:
        from examples.simple_joint_space_planner import setup_solver
        from optas_amd.tape import compile_problem, eliminate_affine_equalities

        g = np.load(os.path.join(ROOT, "tests", "golden", "planner_golden.npz"))
        B = 256
        tp = compile_problem(setup_solver(build_only=True)[1])
        idx = np.arange(B) % len(g["x"])
        x = g["x"][idx] + rng.uniform(-1e-3, 1e-3, (B, int(tp.nx)))  # around the recorded optima
        p = np.ascontiguousarray(g["p"][idx])
        if name == "planner_reduced":
            el = eliminate_affine_equalities(tp)
            tp, x = el.tape, np.ascontiguousarray(x[:, el.free])
    ni, ne = int(tp.n_ineq), int(tp.n_eq)
    seeds = np.concatenate([np.ones((B, 1)), -rng.uniform(0.0, 1.0, (B, ni)), -rng.uniform(-1.0, 1.0, (B, ne))], axis=1)  # (1, -lam, -mu)
    return tp, B, x, p, seeds


def _leg(be, x, p, seeds):
    dev, wall = [], []
    for rep in range(2 + 5):
        t0 = time.perf_counter()
        H = be.hessian(x, p, seeds)
        t1 = time.perf_counter()
        if rep >= 2:
            dev.append(be.solve_ms())
            wall.append(1e3 * (t1 - t0))
    return H, {"path": be.flag("tape_hvp_path"), "launches": be.flag("tape_hvp_launches"), "work_mb": be.get_option("tape_hvp_work_mb"),
               "hvp_device": _stats(dev), "hvp_wall": _stats(wall)}


def step(name):
    import numpy as np

    from optas_amd import _lib
    from optas_amd.backend import TapeBackend

    tp, B, x, p, seeds = _workload(name)
    nx = int(tp.nx)
    out = {"B": B, "nx": nx, "tape_len": len(tp.op), "n_ineq": int(tp.n_ineq), "n_eq": int(tp.n_eq), "units": B * nx}
    off = TapeBackend(tp, jit=False, wave=False, metric=False)
    off.set_option("tape_hvp_work_mb", 4096)
    _, out["off_4096_mb"] = _leg(off, x, p, seeds)
    off.set_option("tape_hvp_work_mb", 256)
    H_off, out["off_256_mb"] = _leg(off, x, p, seeds)
    off.close()
    on = TapeBackend(tp, jit=False, wave=True, metric=False)
    assert on.flag("tape_wave") >= 1, "the wavefront schedule was not built"
    on.set_option("tape_hvp_wave", 1)
    out.update({"tape_len_wave": len(on.tape.op), "levels": on.flag("tape_levels"), "passes": on.flag("tape_passes"), "kernel": _lib.kernel_info("k_tape_wave_hvp")})
    for key, regs in (("on_global", 0), ("on_lds", 1)):
        on.set_option("tape_wave_regs", regs)  # (rebuilds the schedule with the placement forced)
        on.set_option("tape_hvp_wave", 1)
        H_on, out[key] = _leg(on, x, p, seeds)
        assert out[key]["path"] == (1 if regs else 2), (key, out[key]["path"])
        out[key]["against_off_max_rel"] = float(np.abs(H_on - H_off).max() / max(1.0, np.abs(H_off).max()))
        out[key]["asymmetry_max"] = float(np.abs(H_on - H_on.transpose(0, 2, 1)).max())
    on.set_option("tape_wave_regs", -1)
    on.set_option("tape_hvp_wave", 1)
    _, out["on_default"] = _leg(on, x, p, seeds)
    on.close()
    best = min(out["on_lds"]["hvp_device"]["median_ms"], out["on_global"]["hvp_device"]["median_ms"])
    out["off_256_over_on_default"] = out["off_256_mb"]["hvp_device"]["median_ms"] / out["on_default"]["hvp_device"]["median_ms"]
    out["off_4096_over_on_best"] = out["off_4096_mb"]["hvp_device"]["median_ms"] / best
    return out


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        sys.path.insert(0, ROOT)
        print("RESULT " + json.dumps(step(sys.argv[2])))
        return 0
    res = {"source": "tools/gpu_tape_hvp_wave_rates.py",
           "timer": "hvp_device: oh_get_timing out[4], events around the launches of one oh_tape_hvp (V = NULL: the dense Hessian); hvp_wall: host clock around "
                    "the call (copies included); 2 warm-up calls, median of 5 with min and max; the legs of a workload run in one process", "workloads": {}}
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
