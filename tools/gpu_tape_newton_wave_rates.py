#!/usr/bin/env python
"""Truncated Newton-CG on the wavefront evaluator (options tape_newton + tape_newton_wave: k_tape_wave_newton) against Newton-CG on the interpreter
(tape_newton alone: k_tape_solve_newton) and against the default quasi-Newton solve on the wavefront evaluator (k_tape_wave), all legs on one library in one
process -> profiles/tape_newton_wave_rates.json.  Recorded; the one criterion (the new path's median below the interpreter leg's minimum on the eliminated
planner at B = 256) is reported as "time_criterion_met", nothing is asserted.

  * the joint-space planner (examples/simple_joint_space_planner.py) on the eliminated backend with the cost metric at B = 256 and B = 4096 -- there also
    the new path with its register columns forced into LDS and into global memory (tape_wave_regs 1 / 0): the numbers behind oh_tape_wave_newton_place;
  * the same planner as written (280 variables, every row kept) at B = 256;
  * the 65-variable shape tape (tests/tape_cases.py: nx65) at B = 4096.

Per workload and leg: the device time of a solve (the handle's event timer, oh_get_timing out[4]) -- one warm-up solve, then six, the median with min and
max --, median and maximum over the batch of evaluations, accepted steps and Hessian-vector products (iters = evaluations + products), the share of
instances that converged, the largest |f - f_default| over the instances both legs converged on, and what flag("tape_newton_path") reported.  The run is
one child process under a time limit; the file is rewritten after every leg."""
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "profiles", "tape_newton_wave_rates.json")
RUNS = 6
LIMIT = 1100
NEWTON, WAVE = {"tape_newton": 1}, {"tape_newton": 1, "tape_newton_wave": 1}
LEGS = [("default", None), ("newton_interpreter", NEWTON), ("newton_wave", WAVE)]
PLACEMENT_LEGS = [("newton_wave_regs_lds", dict(WAVE, tape_wave_regs=1)), ("newton_wave_regs_global", dict(WAVE, tape_wave_regs=0))]


def _stats(ms):
    import numpy as np

    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "runs": len(ms)}


def _counts(v):
    import numpy as np

    return {"median": float(np.median(v)), "max": int(np.max(v))}


def _planner(B, eliminate):
    import numpy as np

    from examples.simple_joint_space_planner import setup_solver
    from optas_amd.backend import tape_backend
    from optas_amd.tape import compile_problem

    rng = np.random.default_rng(20260927)  # tools/gpu_tape_newton_rates.py's batch, tiled
    g = np.load(os.path.join(ROOT, "tests", "golden", "planner_golden.npz"))
    tp = compile_problem(setup_solver(build_only=True)[1])
    P = g["p"][np.arange(B) % len(g["p"])].copy()
    P[4:, :14] += rng.uniform(-0.05, 0.05, (B - 4, 14))
    P[4:, 14:17] += rng.uniform(-0.02, 0.02, (B - 4, 3))
    x0 = np.zeros((B, int(tp.nx)))
    x0[:, :140] = np.tile(g["q0"].reshape(-1, 1), (1, 20)).reshape(-1)[None, :]
    # (as written the default leg needs the evaluations solver.py gives a trajectory-sized tape; Newton-CG is capped where the eliminated legs are)
    make = lambda opts: tape_backend(tp, eliminate=eliminate, max_iter=3000 if (eliminate or opts) else 400000, options=opts)
    return make, x0, np.ascontiguousarray(P)


def _nx65(B):
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tape_cases as tc
    from optas_amd.backend import TapeBackend

    tp = tc.shape_tapes()["nx65"]
    x, p = tc.shape_point(tp, 11)[:2]
    rng = np.random.default_rng(65)
    x0 = x[None] * rng.uniform(0.9, 1.1, (B, 1)) + rng.uniform(-0.01, 0.01, (B, int(tp.nx)))
    return (lambda opts: TapeBackend(tp, jit=False, wave=True, max_iter=600, options=opts)), x0, np.tile(p, (B, 1))


WORKLOADS = [("planner_eliminated_B256", lambda: _planner(256, True), True), ("planner_eliminated_B4096", lambda: _planner(4096, True), True),
             ("planner_as_written_B256", lambda: _planner(256, False), False), ("nx65_B4096", lambda: _nx65(4096), False)]


def run():
    import numpy as np

    res = {"source": "tools/gpu_tape_newton_wave_rates.py",
           "timer": "device: oh_get_timing out[4], events around the solve's launch; one warm-up solve, then %d, median with min and max; every leg on the same "
                    "library in the same process" % RUNS,
           "counts": "per instance over the batch: evaluations of the merit, accepted line-search steps, Hessian-vector products (iters = evaluations + products)",
           "workloads": {}}
    for name, build, placement in WORKLOADS:
        make, x0, p = build()
        B = len(x0)
        out = {"B": B, "nx": int(x0.shape[1]), "legs": {}}
        f_default = ok_default = None
        for leg, opts in LEGS + (PLACEMENT_LEGS if placement else []):
            be = make(opts)
            ms = []
            for r in range(1 + RUNS):
                sol = be.solve(x0, p)
                if r:
                    ms.append(be.solve_ms())
            rec = {"options": opts or {}, "flag_tape_wave": be.flag("tape_wave"), "flag_tape_newton": be.flag("tape_newton"), "flag_tape_newton_path": be.flag("tape_newton_path"),
                   "tape_passes": be.flag("tape_passes"), "tape_levels": be.flag("tape_levels"), "converged_share": float((sol.status == 0).mean()), "device": _stats(ms)}
            if opts:
                steps, hvps = be.newton_stats(B)
                rec.update({"evaluations": _counts(sol.iters - hvps), "steps": _counts(steps), "products": _counts(hvps)})
            else:
                rec["evaluations"] = _counts(sol.iters)
            if leg == "default":
                f_default, ok_default = sol.f.copy(), sol.status == 0
            both = ok_default & (sol.status == 0)
            rec["both_converged"] = int(both.sum())
            rec["max_abs_f_minus_f_default"] = float(np.abs(sol.f - f_default)[both].max()) if both.any() else None
            be.close()
            out["legs"][leg] = rec
            res["workloads"][name] = out
            print(name, leg, json.dumps(rec), flush=True)
            with open(OUT, "w") as f:
                json.dump(res, f, indent=1)
        L = out["legs"]
        out["newton_wave_over_default"] = L["newton_wave"]["device"]["median_ms"] / L["default"]["device"]["median_ms"]
        out["newton_interpreter_over_newton_wave"] = L["newton_interpreter"]["device"]["median_ms"] / L["newton_wave"]["device"]["median_ms"]
        if name == "planner_eliminated_B256":
            res["time_criterion"] = "planner_eliminated_B256: median of newton_wave below the minimum of newton_interpreter in the same run"
            res["time_criterion_met"] = bool(L["newton_wave"]["device"]["median_ms"] < L["newton_interpreter"]["device"]["min_ms"])
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)
    return 0


def main():
    if len(sys.argv) == 2 and sys.argv[1] == "--run":
        sys.path.insert(0, ROOT)
        return run()
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--run"], timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"time limit of {LIMIT} s; what was measured until then is in {OUT}", file=sys.stderr)
        return 124
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
