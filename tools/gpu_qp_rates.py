#!/usr/bin/env python
"""Device time of the workgroup-per-instance dense QP kernel (k_qp_solve_block) -> profiles/qp_block_rates.json.  Recorded, nothing asserted.

  * packed rows resident: the planted classes n64, n96, n128_max (tests/qp_planted_large.py) at B = 1, 256, 4096;
  * the 72-variable linear MPC at B = 256 through HIPSolver's option dense_qp (device assembly + solve), against the same problem on the
    default path (generic tape family), in the same job on the same GPU.

Device time is the handle's event timer (oh_get_timing) after warm-up: median of the repeats, with min and max.  Every step is a child process
under a time limit of its own; the chain stops at the first step that fails."""
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "profiles", "qp_block_rates.json")
STEPS = [("rows", "n64", 120), ("rows", "n96", 180), ("rows", "n128_max", 300), ("mpc", "256", 300)]


def _stats(ms):
    import numpy as np

    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "repeats": len(ms)}


def step_rows(name):
    import numpy as np

    import qp_planted_large as L
    from optas_amd.backend import QPBackend

    a = L.CLASSES[name]
    n, m, me = a["n"], a["m"], a["me"]
    packed = np.stack([L.pack(qp) for qp in L.planted_instances(name)])
    be = QPBackend(n, m, me)
    out = {"n": n, "m": m, "me": me, "batches": {}}
    for B in (1, 256, 4096):
        rows = packed[np.arange(B) % L.N_INST]
        x0 = np.zeros((B, n))
        ms = []
        for rep in range(2 + (3 if B == 4096 else 7)):
            r = be.solve(x0, rows)
            if rep >= 2:
                ms.append(be.solve_ms())
        st = _stats(ms)
        st.update(converged=int((r.status == 0).sum()), iters_mean=float(r.iters.mean()), iters_max=int(r.iters.max()))
        st["us_per_iteration_per_round_of_256_blocks"] = 1e3 * st["median_ms"] / max(1.0, float(r.iters.max())) / max(1.0, np.ceil(B / 256.0))
        out["batches"][str(B)] = st
    be.close()
    return out


def step_mpc(B):
    import numpy as np

    import qp_planted_large as L
    from optas_amd.solver import HIPSolver

    B = int(B)
    o = L.mpc_problem()
    pv = L.mpc_parameters(np.random.default_rng(50000), B)
    x0 = np.zeros((B, o.nx))
    out = {"B": B, "nx": o.nx, "nk": o.nk, "na": o.na}
    for key, opts in (("dense_qp", {"dense_qp": True}), ("tape_family", {})):
        s = HIPSolver(o).setup("hip_sqp", opts)
        ms = []
        for rep in range(7):
            r = s.solve_batch_arrays(x0, pv)
            if rep >= 2:
                ms.append(s.backend.solve_ms())
        st = _stats(ms)
        st.update(converged=int((r.status == 0).sum()), iters_mean=float(r.iters.mean()), f_mean=float(r.f.mean()))
        out[key] = st
        s.backend.close()
    out["tape_over_dense_qp"] = out["tape_family"]["median_ms"] / out["dense_qp"]["median_ms"]
    return out


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--step":
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        print("RESULT " + json.dumps({"rows": step_rows, "mpc": step_mpc}[sys.argv[2]](sys.argv[3])))
        return 0
    res = {"source": "tools/gpu_qp_rates.py", "timer": "oh_get_timing: device time of the whole solve, median after 2 warm-up solves", "rows": {}, "mpc": None}
    for kind, arg, limit in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, arg], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {kind} {arg}: time limit of {limit} s; stopping", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"step {kind} {arg}: exit {p.returncode}; stopping\n{p.stderr[-2000:]}", file=sys.stderr)
            return p.returncode
        val = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        if kind == "rows":
            res["rows"][arg] = val
        else:
            res["mpc"] = val
        print(kind, arg, json.dumps(val), flush=True)
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
