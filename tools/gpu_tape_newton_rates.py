#!/usr/bin/env python
"""Truncated Newton-CG (option tape_newton = 1) against the quasi-Newton path (tape_newton = 0: the default handle, generated code or the wavefront
evaluator) on the same library in the same run -> profiles/tape_newton_rates.json.  Recorded, nothing asserted.

  * the 7-joint IK tape (examples/example.py) at B = 65 536, reachable goals around the nominal posture;
  * planar IK (examples/planar_ik.py) at B = 4096, starts around [pi / 2, 0, 0];
  * the joint-space planner (examples/simple_joint_space_planner.py) on the eliminated backend with the cost metric (the preconditioner of CG) at B = 256.

Per workload and leg: median, 99th percentile and maximum over the batch of evaluations, and for Newton-CG of accepted steps and Hessian-vector products (iters is their
sum with the evaluations), how many instances converged, how far the two legs' optima are apart, and the device time of a solve (the handle's event timer,
oh_get_timing out[4]): one warm-up solve, then six, the median with min and max.  Beside them the numpy port's counts (tests/tape_newton_ref.py,
oracle/tape_ref.py) on the first instances of the batch.  Every step is a child process under a time limit of its own; the chain stops at the first
step that fails."""
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "profiles", "tape_newton_rates.json")
STEPS = [("ik", 300), ("planar", 240), ("planner", 420)]
RUNS = 6
PORT_SAMPLE = {"ik": 8, "planar": 4, "planner": 2}


def _stats(ms):
    import numpy as np

    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "runs": len(ms)}


def _counts(v):
    import numpy as np

    return {"median": float(np.median(v)), "p99": float(np.percentile(v, 99)), "max": int(np.max(v))}


def _workload(name):
    """(backend factory(newton), x0, p, port arguments)"""
    import numpy as np

    from optas_amd.backend import TapeBackend, tape_backend
    from optas_amd.tape import compile_problem

    golden = os.path.join(ROOT, "tests", "golden")
    rng = np.random.default_rng(20260927)
    if name == "ik":
        from examples.example import setup_solver
        from optas_amd.models import RobotModel

        tp = compile_problem(setup_solver(build_only=True)[1])
        B = 65536
        qn = np.deg2rad([0, 45, 0, -90, 0, -45, 0]) + rng.uniform(-0.3, 0.3, (B, 7))
        kuka = RobotModel.builtin("kuka_lwr")  # goals the arm can reach: the positions of perturbed configurations (tools/gpu_tape_rates.py)
        qg = np.clip(qn + rng.uniform(-0.5, 0.5, (B, 7)), kuka.lower_actuated_joint_limits, kuka.upper_actuated_joint_limits)
        p = np.ascontiguousarray(np.concatenate([qn, np.asarray(kuka.get_global_link_position("end_effector_ball", qg.T)).T], 1))
        make = lambda newton: TapeBackend(tp, options={"tape_newton": 1} if newton else None)
        return make, qn, p, {"tape": tp, "h0": None, "rho0": 10.0, "max_iter": 2000, "free": None}
    if name == "planar":
        from examples.planar_ik import setup_solver
        from optas_amd.lowering import lower

        tp = lower(setup_solver(build_only=True)[1])[1].tape
        B = 4096
        x0 = np.array([np.pi / 2, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, (B, 3))
        x0[0] = [np.pi / 2, 0.0, 0.0]
        make = lambda newton: TapeBackend(tp, options={"tape_newton": 1} if newton else None)
        return make, x0, np.zeros((B, 0)), {"tape": tp, "h0": None, "rho0": 10.0, "max_iter": 2000, "free": None}
    from examples.simple_joint_space_planner import setup_solver

    g = np.load(os.path.join(golden, "planner_golden.npz"))
    tp = compile_problem(setup_solver(build_only=True)[1])
    B = 256
    idx = np.arange(B) % len(g["p"])
    P = g["p"][idx].copy()
    P[4:, :14] += rng.uniform(-0.05, 0.05, (B - 4, 14))
    P[4:, 14:17] += rng.uniform(-0.02, 0.02, (B - 4, 3))
    x0 = np.zeros((B, int(tp.nx)))
    x0[:, :140] = np.tile(g["q0"].reshape(-1, 1), (1, 20)).reshape(-1)[None, :]
    make = lambda newton: tape_backend(tp, max_iter=3000, options={"tape_newton": 1} if newton else None)
    probe = make(False)  # the reduced tape, its metric and penalty, for the port
    arg = {"tape": probe.elim.tape, "h0": probe.inner._h0, "rho0": 1e4, "max_iter": 3000, "free": probe.elim.free}
    probe.close()
    return make, x0, np.ascontiguousarray(P), arg


def step(name):
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tape_newton_ref as N
    from oracle import tape_ref

    make, x0, p, arg = _workload(name)
    B = len(x0)
    out = {"B": B, "nx": int(x0.shape[1]), "tape_len": len(arg["tape"].op), "n_ineq": int(arg["tape"].n_ineq), "n_eq": int(arg["tape"].n_eq)}
    sol = {}
    for newton in (1, 0):
        be = make(bool(newton))
        ms = []
        for run in range(1 + RUNS):
            res = be.solve(x0, p)
            if run:
                ms.append(be.solve_ms())
        rec = {"evaluator": "interpreter" if newton else ("wavefront" if be.flag("tape_wave") else ("generated code" if be.jit else "interpreter")),
               "flag_tape_newton": be.flag("tape_newton"), "converged": int((res.status == 0).sum()), "device": _stats(ms)}
        if newton:
            steps, hvps = be.newton_stats(B)
            rec.update({"evaluations": _counts(res.iters - hvps), "steps": _counts(steps), "products": _counts(hvps), "iters": _counts(res.iters),
                        "slowest_instance": int(np.argmax(res.iters)), "slowest_status": int(res.status[np.argmax(res.iters)])})
        else:
            rec["evaluations"] = _counts(res.iters)
        out["tape_newton_%d" % newton] = rec
        sol[newton] = res
        be.close()
    both = (sol[1].status == 0) & (sol[0].status == 0)
    out["same_optimum"] = int((both & (np.abs(sol[1].f - sol[0].f) <= 1e-6 * np.maximum(1.0, np.abs(sol[0].f)))).sum())
    out["newton_f_lower"] = int((both & (sol[1].f < sol[0].f - 1e-6 * np.maximum(1.0, np.abs(sol[0].f)))).sum())
    out["newton_f_higher"] = int((both & (sol[1].f > sol[0].f + 1e-6 * np.maximum(1.0, np.abs(sol[0].f)))).sum())
    out["device_time_ratio_newton_over_default"] = out["tape_newton_1"]["device"]["median_ms"] / out["tape_newton_0"]["device"]["median_ms"]
    # the ports on the first instances
    n = PORT_SAMPLE[name]
    pe, ps, ph, be_ = [], [], [], []
    for b in range(n):
        xs = x0[b] if arg["free"] is None else x0[b][arg["free"]]
        r = N.solve_tape_newton(arg["tape"], xs, p[b], rho0=arg["rho0"], h0=arg["h0"], max_iter=arg["max_iter"])
        pe.append(r["evals"]), ps.append(r["steps"]), ph.append(r["hvps"])
        if name != "planner":  # (the quasi-Newton port of the 133-variable planner takes minutes)
            be_.append(tape_ref.solve_tape_al(arg["tape"], xs, p[b], rho0=arg["rho0"], max_iter=arg["max_iter"])["evals"])
    out["port"] = {"instances": n, "newton_evaluations": _counts(pe), "newton_steps": _counts(ps), "newton_products": _counts(ph)}
    if be_:
        out["port"]["default_evaluations"] = _counts(be_)
    return out


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        sys.path.insert(0, ROOT)
        print("RESULT " + json.dumps(step(sys.argv[2])))
        return 0
    res = {"source": "tools/gpu_tape_newton_rates.py",
           "timer": "device: oh_get_timing out[4], events around the solve's launch; one warm-up solve, then %d, median with min and max; both legs on the same "
                    "library in the same process, tape_newton = 1 first" % RUNS,
           "counts": "per instance over the batch: evaluations of the merit, accepted line-search steps, Hessian-vector products (iters = evaluations + products)",
           "workloads": {}}
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
