#!/usr/bin/env python
"""Bits and device times of everything that reads the tape vocabulary (csrc/oh_tape_ops.h), for comparing two builds of the library (OPTAS_HIP_LIBRARY
selects the other one) after a change that must not alter either.  One process per library and call:

  dump OUT.npz     every output array of: oh_tape_phi on the opcode table, the shape tapes and the random tapes on all six evaluator variants
                   (tests/test_gpu_tape_evaluators.py's handles); oh_tape_hvp with its gradient and the dense Hessian on tape_hvp_ref's composite
                   cases; oh_tape_probe's values, adjoints and gradient on the opcode table; solves of the 7-joint IK goldens with and without
                   generated code; a QP handle fed by an opcode-rich tape (cost |x|^2 / 2 + sum_j op_j(p_2j, p_2j+1) x_(j mod n), rows x_i + 2 >= 0)
                   at n = 2 (B = 32: a lane per probe, B = 256: a lane per instance) and n = 40 (block assembly): x, f, multipliers;
                   the wavefront evaluator's sweeps (tests/test_gpu_tape_wave_bits.py:wave_outputs) on the opcode table, every composite case, a tape
                   with a row of each kind and one without rows, at one wavefront and at four, registers in LDS and in global memory: oh_tape_phi,
                   oh_tape_hvp with tape_hvp_wave (given V and the unit directions, with the gradient), oh_tape_phi_hvp with tape_newton_wave; one
                   Newton-CG solve on the wavefront evaluator (nx65, B = 32): x, f, kkt, multipliers, counts, oh_tape_newton_stats.
  pin OUT.npz      the part of `dump` that tests/test_gpu_tape_wave_bits.py compares against (tests/golden/tape_wave_parent_bits.npz).
  time OUT.json N  N device times (ms, the handle's event timer, after one warm-up call) of: the 7-joint IK tape at B = 65 536 on the interpreter and
                   on generated code; the perturbed planner batches B = 256 and 1024 of tools/gpu_tape_rates.py (wavefront evaluator); both points
                   of tools/gpu_tape_hvp_rates.py at the default budget; the dense_qp leg of tools/gpu_qp_rates.py (72 variables, B = 256); the
                   planner's dense Hessian on the wavefront evaluator (tools/gpu_tape_hvp_wave_rates.py: planner, default placement); the Newton-CG
                   solve of the eliminated planner on it at B = 256 (tools/gpu_tape_newton_wave_rates.py); one oh_tape_phi of the eliminated planner
                   at B = 1024 (no event timer in that call: the host clock around it, copies included).
  report PARENT.npz NEW.npz OUT.json TIMES...   arrays compared byte for byte; per point the new library's median against the parent's maximum
                   (TIMES: the json files of `time`, told apart by their "library" entry).  Exit status 1 if an array differs or a point is slower.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, d)
GOLDEN = os.path.join(ROOT, "tests", "golden")


class Env:  # what conftest.oh_debug needs of pytest's monkeypatch
    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=False):
        os.environ.pop(k, None)


def _ik():
    from examples.example import setup_solver
    from optas_amd.tape import compile_problem

    return compile_problem(setup_solver(build_only=True)[1]), np.load(os.path.join(GOLDEN, "ik_golden.npz"))


def qp_tape(n):
    import tape_cases as tc

    t = tc.B()
    xs = [t.x(i) for i in range(n)]
    cost = None
    for i in range(n):
        h = t.emit(5, t.const(0.5), t.emit(12, xs[i]))
        cost = h if cost is None else t.emit(3, cost, h)
    for j, o in enumerate(range(3, 27)):
        coef = t.emit(o, t.p(2 * j), t.p(2 * j + 1) if o in tc.BINARY else 0)
        cost = t.emit(3, cost, t.emit(5, coef, xs[j % n]))
    rows = [t.emit(3, xs[i], t.const(2.0)) for i in range(n)]
    return t.tape(cost, rows, n, 0, n, 48)


def dump(path):
    import tape_cases as tc
    import tape_hvp_ref as R
    import test_gpu_tape_evaluators as ev
    from optas_amd.backend import QPBackend, TapeBackend

    env, out = Env(), {}

    def put(prefix, d):
        print(prefix, len(d), flush=True)
        for k, v in d.items():
            out[prefix + "/" + k] = np.asarray(v)

    X, P, operands = tc.opcode_table_lines()
    lam, mu = tc.table_multipliers(operands), np.zeros((len(X), 24))
    for v, r in ev._table_all(env, X, P, lam, mu, cover=False).items():
        put("phi/table/" + v, r)
    shapes = tc.shape_tapes()
    for k, name in enumerate(sorted(shapes)):
        h = ev.Handles(env, shapes[name])
        pts = [tc.shape_point(h.tape, 100 + k + 1 + 1000 * j) for j in range(3)]
        args = [np.array([pt[i] for pt in pts]).reshape(3, -1) for i in range(4)]
        for v, r in h.phi(*args, pts[0][4], cover=False).items():
            put("phi/shape_%s/%s" % (name, v), r)
        h.close()
    for spec in tc.RANDOM_SPECS:
        tp0, x, p, la, m_, rho = tc.random_tape(*spec)
        h = ev.Handles(env, tp0)
        for v, r in h.phi(x[None], p[None], la[None], m_[None], rho, cover=False).items():
            put("phi/random%d/%s" % (spec[0], v), r)
        h.close()
    ev._clear(env)
    os.environ["OH_DEBUG_OPTIONS"] = "tape_wave=0.0"
    for name, tp, x, p, seeds, v in R.composite_cases():
        be = TapeBackend(tp, jit=False, wave=False)
        HV, g = be.hvp(x[None], p[None], seeds[None], v[None, None])
        put("hvp/" + name, {"HV": HV, "grad": g, "H": be.hessian(x[None], p[None], seeds[None])})
        be.close()
    tp = tc.opcode_table_tape(range(3, 27))
    be = TapeBackend(tp, jit=False, wave=False)
    seeds = np.random.default_rng(3).uniform(-1.0, 1.0, (len(X), 49))
    val, adj, g = be.probe(X, P, np.arange(len(tp.op)), seeds)
    put("probe/table", {"val": val, "adj": adj, "grad": g})
    be.close()
    tp, gold = _ik()
    for jit in (True, False):
        be = TapeBackend(tp, jit=jit)
        r = be.solve(gold["x0"], gold["p"])
        la, m_ = be.multipliers(len(gold["p"]))
        put("solve/ik_jit%d" % jit, {"x": r.x, "f": r.f, "iters": r.iters, "status": r.status, "kkt": r.kkt, "lam": la, "mu": m_})
        be.close()
    os.environ.pop("OH_DEBUG_OPTIONS")
    for n, B in ((2, 32), (2, 256), (40, 48)):
        be = QPBackend(n, n, 0, tape=qp_tape(n))
        pv = np.random.default_rng(100 * n + B).uniform(0.2, 0.9, (B, 48))
        r = be.solve(np.zeros((B, n)), pv)
        put("qp/n%d_B%d" % (n, B), {"x": r.x, "f": r.f, "iters": r.iters, "status": r.status, "lam": be.multipliers(B)[0], "block": be.flag("qp_block")})
        be.close()
    import test_gpu_tape_wave_bits as wb

    cases = wb.pin_cases(composites=[c[0] for c in R.composite_cases()])
    tp = shapes["rows_none"]
    cases.setdefault("rows_none", wb._batch("rows_none", tp, *tc.shape_point(tp, 11)[:2], 3))
    put("wave", wb.wave_outputs(env, cases, tuple(wb.WAVE_OPTS), dense_max_nx=1 << 30))
    tp = shapes["nx65"]
    x, p = tc.shape_point(tp, 11)[:2]
    rng = np.random.default_rng(65)
    x0 = x[None] * rng.uniform(0.9, 1.1, (32, 1)) + rng.uniform(-0.01, 0.01, (32, int(tp.nx)))
    be = TapeBackend(tp, jit=False, wave=True, max_iter=600, options={"tape_newton": 1, "tape_newton_wave": 1})
    r = be.solve(x0, np.tile(p, (32, 1)))
    steps, hvps = be.newton_stats(32)
    la, m_ = be.multipliers(32)
    put("solve/newton_wave_nx65", {"x": r.x, "f": r.f, "iters": r.iters, "status": r.status, "kkt": r.kkt, "lam": la, "mu": m_, "steps": steps, "products": hvps,
                                   "path": be.flag("tape_newton_path")})
    be.close()
    np.savez(path, **out)
    print("dumped", len(out), "arrays to", path)


def pin(path):
    import test_gpu_tape_wave_bits as wb

    out = wb.wave_outputs(Env(), wb.pin_cases(), wb.PIN_VARIANTS)
    np.savez_compressed(path, **out)
    print("pinned", len(out), "arrays to", path)


def time_points(path, reps):
    import time

    import gpu_tape_hvp_rates as hv
    import gpu_tape_hvp_wave_rates as hvw
    import gpu_tape_newton_wave_rates as nw
    import qp_planted_large as L
    from examples.simple_joint_space_planner import setup_solver as planner_setup
    from optas_amd.backend import TapeBackend
    from optas_amd.models import RobotModel
    from optas_amd.solver import HIPSolver

    pts = {}

    def run(name, call, ms):
        call()
        pts[name] = []
        for _ in range(reps):
            call()
            pts[name].append(float(ms()))
        print(name, pts[name], flush=True)

    tp, _ = _ik()
    rng = np.random.default_rng(20260927)
    B = 65536
    qn = np.deg2rad([0, 45, 0, -90, 0, -45, 0]) + rng.uniform(-0.3, 0.3, (B, 7))
    kuka = RobotModel.builtin("kuka_lwr")  # (goals the arm can reach: the positions of perturbed configurations, as tools/gpu_tape_rates.py draws them)
    qg = np.clip(qn + rng.uniform(-0.5, 0.5, (B, 7)), kuka.lower_actuated_joint_limits, kuka.upper_actuated_joint_limits)
    p = np.ascontiguousarray(np.concatenate([qn, np.asarray(kuka.get_global_link_position("end_effector_ball", qg.T)).T], 1))
    for jit in (False, True):
        be = TapeBackend(tp, jit=jit, wave=False)
        run("ik_b65536_" + ("jit" if jit else "interp"), lambda: be.solve(qn, p), be.solve_ms)
        be.close()
    g = np.load(os.path.join(GOLDEN, "planner_golden.npz"))
    robot, solver = planner_setup(solver_options={"max_iter": 400000})
    P, nb = g["p"], len(g["p"])
    solver.reset_parameters_batch({"nominal_joint_state": P[:, :7], "current_joint_state": P[:, 7:14], "position_goal": P[:, 14:17], "orientation_goal": P[:, 17:]})
    solver.reset_initial_seed_batch({f"{robot.get_name()}/q/x": np.stack([np.tile(g["q0"].reshape(-1, 1), (1, 20))] * nb)})
    solver.solve_batch()
    be = solver.backend
    assert be.flag("tape_wave") >= 1
    x0 = np.zeros((nb, solver.opt.nx))
    x0[:, :140] = np.tile(g["q0"].reshape(-1, 1), (1, 20)).reshape(-1)[None, :]
    for Bn in (256, 1024):
        idx = np.arange(Bn) % nb
        Pn = P[idx].copy()
        Pn[:, :14] += rng.uniform(-0.05, 0.05, (Bn, 14))
        Pn[:, 14:17] += rng.uniform(-0.02, 0.02, (Bn, 3))
        xs, Pn = np.ascontiguousarray(x0[idx]), np.ascontiguousarray(Pn)
        run("planner_wave_b%d" % Bn, lambda: be.solve(xs, Pn), be.solve_ms)
    be.close()
    for name in ("ik", "planner"):
        tp, B, x, p, seeds = hv._workload(name)
        be = TapeBackend(tp, jit=False, wave=False, metric=False)
        run("hvp_" + name, lambda: be.hessian(x, p, seeds), be.solve_ms)
        be.close()
    o = L.mpc_problem()
    pv, x0 = L.mpc_parameters(np.random.default_rng(50000), 256), np.zeros((256, o.nx))
    s = HIPSolver(o).setup("hip_sqp", {"dense_qp": True})
    run("qp_dense_mpc_b256", lambda: s.solve_batch_arrays(x0, pv), s.backend.solve_ms)
    s.backend.close()
    tp, B, x, p, seeds = hvw._workload("planner")
    be = TapeBackend(tp, jit=False, wave=True, metric=False)
    be.set_option("tape_hvp_wave", 1)
    run("hvp_wave_planner", lambda: be.hessian(x, p, seeds), be.solve_ms)
    assert be.flag("tape_hvp_path") >= 1
    be.close()
    make, x0, p = nw._planner(256, True)
    be = make(nw.WAVE)
    run("newton_wave_planner_b256", lambda: be.solve(x0, p), be.solve_ms)
    assert be.flag("tape_newton_path") >= 1
    be.close()
    make, x0, p = nw._planner(1024, True)
    be = make(None)
    inner = be.inner
    xi = np.random.default_rng(1024).uniform(-0.1, 0.1, (1024, inner.nx))
    lam, mu = np.zeros((1024, int(inner.tape.n_ineq))), np.zeros((1024, int(inner.tape.n_eq)))
    wall = [0.0]

    def phi_call():
        t0 = time.perf_counter()
        inner.phi(xi, p, lam, mu, 10.0)
        wall[0] = 1e3 * (time.perf_counter() - t0)

    run("planner_phi_b1024_wall", phi_call, lambda: wall[0])
    assert inner.flag("tape_wave") >= 1
    be.close()
    with open(path, "w") as f:
        json.dump({"library": os.environ.get("OPTAS_HIP_LIBRARY", "in-tree"), "points_ms": pts}, f, indent=1)


def report(parent, new, path, times):
    a, b = np.load(parent), np.load(new)
    differ = [k for k in a.files if k not in b.files or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    differ += [k for k in b.files if k not in a.files]
    runs = {"parent": {}, "new": {}}
    for t in times:
        rec = json.load(open(t))
        side = runs["new" if rec["library"] == "in-tree" else "parent"]
        for k, ms in rec["points_ms"].items():
            side.setdefault(k, []).extend(ms)
    points = {}
    for k in runs["new"]:
        pm, nm = runs["parent"][k], runs["new"][k]
        points[k] = {"parent_ms": pm, "new_ms": nm, "parent_max_ms": max(pm), "new_median_ms": float(np.median(nm)), "holds": bool(np.median(nm) <= max(pm))}
    res = {"source": "tools/gpu_tape_ab_dump.py", "arrays": len(a.files), "arrays_differing": differ, "bit_identical": not differ,
           "speed_criterion": "per point, the new library's median over its runs <= the parent's maximum over its runs; processes of the two libraries alternated",
           "points": points}
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: (v["parent_max_ms"], v["new_median_ms"], v["holds"]) for k, v in points.items()}, indent=1))
    print("arrays", len(a.files), "differing", differ)
    return 0 if not differ and all(v["holds"] for v in points.values()) else 1


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif sys.argv[1] == "pin":
        pin(sys.argv[2])
    elif sys.argv[1] == "time":
        time_points(sys.argv[2], int(sys.argv[3]))
    else:
        sys.exit(report(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5:]))
