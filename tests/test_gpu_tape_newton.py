"""Truncated Newton-CG inner solver of the tape family on the device (option tape_newton: optas_amd/csrc/oh_tape_newton.h, InterpEval::hess_vec and
k_tape_solve_newton of oh_tape.hip), up to HIPSolver.

References: tests/tape_newton_ref.py -- the merit's generalised Hessian by second differences of the 60-digit interpreter plus rho grad row grad row^T with
the rows' gradients by mp differences (no derivative rule shared with the device), and the numpy restatement of the state machine.  The product is graded
with tape_hvp_ref.within(.., DEVICE_TOL) = 1e-12 max(1, |H|_inf), solves with the tolerances tests/test_tape.py and tests/test_planner.py use on the same
goldens.  Every figure is printed before it is asserted; no test asserts a time."""
import ctypes as C
import os

import numpy as np
import pytest

import tape_cases as tc
import tape_hvp_ref as R
import tape_newton_ref as N
from conftest import GOLDEN, oh_debug
from optas_amd import _lib
from optas_amd.backend import EliminatedTapeBackend, TapeBackend
from oracle import tape_ref

pytestmark = pytest.mark.gpu

TOL = R.DEVICE_TOL


def _clear(monkeypatch):
    oh_debug(monkeypatch, tape_wave=None, tape_lbfgs=None, tape_wave_nt=None, tape_wave_regs=None, tape_lds_max=None, tape_hvp_work_mb=None, tape_newton=None,
             tape_newton_cg=None)


def _interp(monkeypatch, tp, **kw):
    _clear(monkeypatch)
    be = TapeBackend(tp, jit=False, wave=False, **kw)
    assert be.flag("tape_wave") == 0 and not be.jit and be.tape is tp
    return be


def _newton(monkeypatch, tp, **kw):
    _clear(monkeypatch)
    be = TapeBackend(tp, options={"tape_newton": 1}, **kw)
    assert be.newton and not be.jit and not be.wave and be.tape is tp and be.get_option("tape_newton") == 1
    return be


def _ik_tape():
    from examples.example import setup_solver as ik
    from optas_amd.tape import compile_problem

    return compile_problem(ik(build_only=True)[1])


# ---- 1. the merit's Hessian-vector product ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.composite_cases()])
def test_merit_hvp_composite_tapes_against_mp(hip_lib, monkeypatch, name):
    kept, dropped = N.kept_merit_cases()
    assert len(dropped) <= 2
    cases = [c for c in kept if c[0] == name]
    assert cases or name in [d[0] for d in dropped]
    for _, tp, x, p, lam, mu, rho in cases:
        H, margin = N.merit_reference(name, rho)
        be = _interp(monkeypatch, tp)
        try:
            nx = int(tp.nx)
            HV, g = be.phi_hvp(x[None], p[None], lam[None], mu[None], rho, np.eye(nx)[None])
            g_phi = be.phi(x[None], p[None], lam[None], mu[None], rho)["grad"]
        finally:
            be.close()
        ok, err = R.within(HV[0], H, TOL)
        asym = float(np.abs(HV[0] - HV[0].T).max()) / max(1.0, float(np.abs(H).max()))
        print(name, "rho", rho, "nx", nx, "active", int((margin > 0).sum()), "inactive", int((margin < 0).sum()), "|H|", float(np.abs(H).max()), "error", err,
              "asymmetry", asym)
        assert ok, (name, rho, err)
        assert asym <= TOL
        assert tc.same(g, g_phi).all()  # the evaluation in front of the products is oh_tape_phi's, bit for bit


@pytest.mark.parametrize("o", sorted(tc.DIFF_OPS), ids=lambda o: tc.OP_NAME[o])
def test_merit_hvp_every_differentiable_opcode_as_a_row(hip_lib, monkeypatch, o):
    """tape_cases.row_tape(o): the opcode on two variables as the one >= row, cost 0.  Every line active (lam - rho g = 0.5) and, where a multiplier >= 0
    allows it with the margin, inactive (then the product is exactly zero)."""
    tp, rho = tc.row_tape(o), tc.TABLE_RHO
    X, LAM = [], []
    for x in R.single_op_lines(o):
        g = float(tape_ref.forward(tp, x, np.zeros(0))[2])
        X.append(x), LAM.append(max(0.0, rho * g) + 0.5)
        if rho * g >= N.MARGIN:
            X.append(x), LAM.append(max(0.0, rho * g - 0.5))
    X, LAM = np.array(X), np.array(LAM).reshape(-1, 1)
    be = _interp(monkeypatch, tp)
    try:
        HV, _ = be.phi_hvp(X, np.zeros((len(X), 0)), LAM, None, rho, np.tile(np.eye(2)[None], (len(X), 1, 1)))
    finally:
        be.close()
    n_act = n_inact = 0
    for x, lam, got in zip(X, LAM, HV):
        H, margin = N.merit_hessian_mp(tp, x, np.zeros(0), lam, np.zeros(0), rho)
        assert abs(margin[0]) >= N.MARGIN
        ok, err = R.within(got, H, TOL)
        print(tc.OP_NAME[o], x, "margin", margin[0], "|H|", float(np.abs(H).max()), "error", err)
        assert ok, (tc.OP_NAME[o], x, lam, got, H, err)
        if margin[0] > 0:
            n_act += 1
        else:
            n_inact += 1
            assert not got.any()
    assert n_act >= 1 and n_inact >= 1


@pytest.mark.parametrize("B", [63, 64, 65])
def test_merit_hvp_block_edges_alone_and_at_any_position(hip_lib, monkeypatch, B):
    """The one-variable tape (one >= row, one = row) in batches one lane short of a block, on its edge and one lane into the next."""
    _, tp, x, p, lam, mu, rho = next(c for c in N.merit_cases() if c[0] == "random1" and c[6] == 1.0)
    rng = np.random.default_rng(B)
    X = x[None] + rng.uniform(-0.05, 0.05, (B, 1))
    P = np.tile(p, (B, 1))
    LAM = np.tile(lam, (B, 1)) * rng.uniform(0.0, 2.0, (B, 1))  # rows on either side of lam - rho g = 0
    MU = np.tile(mu, (B, 1)) * rng.uniform(0.5, 1.5, (B, 1))
    V = rng.uniform(-1.0, 1.0, (B, 2, 1))
    be = _interp(monkeypatch, tp)
    try:
        hv, g = be.phi_hvp(X, P, LAM, MU, rho, V)
        assert np.isfinite(hv).all() and np.isfinite(g).all()
        assert tc.same(g, be.phi(X, P, LAM, MU, rho)["grad"]).all()  # its phi is oh_tape_phi's, bit for bit
        for b in (0, 31, 62, B - 1):  # alone
            h1, g1 = be.phi_hvp(X[b : b + 1], P[b : b + 1], LAM[b : b + 1], MU[b : b + 1], rho, V[b : b + 1])
            assert tc.same(h1[0], hv[b]).all() and tc.same(g1[0], g[b]).all(), b
        perm = rng.permutation(B)  # at any position
        hp, gp = be.phi_hvp(X[perm], P[perm], LAM[perm], MU[perm], rho, V[perm])
        assert tc.same(hp, hv[perm]).all() and tc.same(gp, g[perm]).all()
        want = N.merit_hvp_port(tp, X[B - 1], P[B - 1], LAM[B - 1], MU[B - 1], rho, V[B - 1, 1])
        assert R.within(hv[B - 1, 1], want, TOL)[0]
    finally:
        be.close()


# ---- 2. solves against the port and the goldens ------------------------------------------------------------------------------------------------------------
def test_ik_batch_against_the_goldens_and_the_port(hip_lib, monkeypatch):
    g = np.load(os.path.join(GOLDEN, "ik_golden.npz"))
    tp = _ik_tape()
    B, max_iter, cap = len(g["p"]), 2000, min(int(tp.nx), 50)
    be = _newton(monkeypatch, tp, max_iter=max_iter)
    try:
        res = be.solve(g["x0"], g["p"])
        assert be.flag("tape_newton") == 1 and be.flag("tape_wave") == 0
        lam, mu = be.multipliers(B)
        steps, hvps = be.newton_stats(B)
    finally:
        be.close()
    evals = res.iters - hvps
    print("IK, %d instances: evaluations p50 %d max %d, steps p50 %d max %d, products p50 %d max %d" % (B, np.median(evals), evals.max(), np.median(steps), steps.max(),
                                                                                                       np.median(hvps), hvps.max()))
    assert (res.status == 0).all() and np.abs(res.f - g["f"]).max() < 1e-7 and np.abs(res.x - g["x"]).max() < 1e-4 and res.kkt[:, 1].max() < 1e-9
    assert (hvps <= steps * cap).all() and (evals >= 1).all() and (res.iters <= max_iter).all()
    for i in (0, 5, 17):
        r = N.solve_tape_newton(tp, g["x0"][i], g["p"][i], max_iter=max_iter)
        print("instance", i, "device evaluations / steps / products", int(evals[i]), int(steps[i]), int(hvps[i]), "port", r["evals"], r["steps"], r["hvps"])
        assert np.abs(res.x[i] - r["x"]).max() < 1e-7
        assert np.abs(lam[i] - r["lam"]).max() < 1e-4 and np.abs(mu[i] - r["mu"]).max() < 1e-4
        assert abs(int(steps[i]) - r["steps"]) <= 2
        assert int(res.iters[i]) == int(evals[i]) + int(hvps[i])
    assert int((lam > 0).sum(axis=1).max()) >= 1 and (lam >= 0).all()


def test_three_tiny_problems_reach_the_ports_end_points(hip_lib, monkeypatch):
    for name, (tp, x0) in N.tiny_problems().items():
        r = N.solve_tape_newton(tp, x0, np.zeros(0))
        be = _newton(monkeypatch, tp)
        try:
            res = be.solve(x0[None], np.zeros((1, 0)))
            steps, hvps = be.newton_stats(1)
        finally:
            be.close()
        print(name, "x", res.x[0], "status", int(res.status[0]), "iters", int(res.iters[0]), "steps", int(steps[0]), "products", int(hvps[0]), "port", r["x"], r["status"],
              r["evals"] + r["hvps"])
        assert int(res.status[0]) != 2  # never NUMERICAL
        if name == "cos":  # negative curvature at the start
            assert int(res.status[0]) == 0 and abs(abs(res.x[0, 0]) - np.pi) < 1e-5 and abs(res.x[0, 1]) < 1e-5
        elif name == "rosenbrock":
            assert int(res.status[0]) == 0 and np.abs(res.x[0] - 1.0).max() < 1e-5
        else:  # singular Hessian at the optimum: converged or at the cap
            assert int(res.status[0]) in (0, 1) and abs(res.x[0, 0] - 1.0) < 2e-2
        assert int(res.status[0]) == r["status"] and np.abs(res.x[0] - r["x"]).max() < 1e-6


# ---- 3. a handle beyond 48 variables ------------------------------------------------------------------------------------------------------------------------
RANDOM60 = (15, 300, 60, 1, 1)  # tape_cases.random_tape: 60 variables, one >= and one = row; the port converges from the tape's own point and around it


def test_sixty_variables_agree_with_the_port(hip_lib, monkeypatch):
    tp, x, p = tc.random_tape(*RANDOM60)[:3]
    rng = np.random.default_rng(60)
    X0 = np.stack([x, x + rng.uniform(-0.01, 0.01, 60), x + rng.uniform(-0.01, 0.01, 60)])  # (the port converges from each within 25 evaluations)
    P = np.tile(p, (3, 1))
    be = _newton(monkeypatch, tp, max_iter=600)
    try:
        res = be.solve(X0, P)
        assert be.flag("tape_newton") == 1 and be.flag("tape_wave") == 0
        steps, hvps = be.newton_stats(3)
    finally:
        be.close()
    for b in range(3):
        r = N.solve_tape_newton(tp, X0[b], p, max_iter=600)
        print("instance", b, "device", int(res.status[b]), int(res.iters[b]), int(steps[b]), int(hvps[b]), "port", r["status"], r["evals"] + r["hvps"], r["steps"], r["hvps"],
              "difference", float(np.abs(res.x[b] - r["x"]).max()))
        assert r["status"] == 0 and int(res.status[b]) == 0
        assert np.abs(res.x[b] - r["x"]).max() < 1e-7


def test_planner_on_the_eliminated_backend_with_its_metric_as_preconditioner(hip_lib, monkeypatch):
    """tests/test_planner.py's tolerances for the eliminated path with the cost metric: f within 1e-5 of the interior-point golden, x within 2e-3, the literal rows."""
    from conftest import MED7_KIN
    from examples.simple_joint_space_planner import setup_solver
    from oracle.problems import JointSpacePlannerNLP
    from oracle.robot import OracleRobot

    _clear(monkeypatch)
    g = np.load(os.path.join(GOLDEN, "planner_golden.npz"))
    nlp = JointSpacePlannerNLP(OracleRobot(MED7_KIN))
    B = 2
    P = g["p"][:B]
    robot, solver = setup_solver(solver_options={"max_iter": 5000, "options": {"tape_newton": 1}})
    try:
        name = robot.get_name()
        solver.reset_parameters_batch({"nominal_joint_state": P[:, :7], "current_joint_state": P[:, 7:14], "position_goal": P[:, 14:17], "orientation_goal": P[:, 17:]})
        solver.reset_initial_seed_batch({f"{name}/q/x": np.stack([np.tile(g["q0"].reshape(-1, 1), (1, 20))] * B)})
        sols = solver.solve_batch()
        st = solver.stats()
        be = solver.backend
        assert isinstance(be, EliminatedTapeBackend) and be.inner.newton and not be.wave and not be.jit
        assert be.flag("tape_newton") == 1 and be.flag("tape_wave") == 0 and be.flag("tape_metric") == 1
        steps, hvps = be.newton_stats(B)
        print("planner: iters", st["iterations"].tolist(), "steps", steps.tolist(), "products", hvps.tolist(), "f", st["f"].tolist(), "golden", g["f"][:B].tolist(),
              "device ms", be.solve_ms())
        assert st["success"], st["status"]
        for b in range(B):
            x = solver.opt.decision_variables.dict2vec(sols[b])
            assert abs(st["f"][b] - g["f"][b]) <= 1e-5 * g["f"][b]
            assert abs(nlp.f(x, P[b]) - st["f"][b]) <= 1e-10 and np.abs(nlp.a(x, P[b])).max() <= 1e-12 and np.abs(nlp.h(x, P[b])).max() <= 1e-8 and nlp.g(x, P[b]).min() >= -1e-9
            assert np.abs(x - g["x"][b]).max() <= 2e-3
    finally:
        solver.backend.close()


# ---- 4. nothing else moves -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["interp", "jit", "wave"])
def test_option_off_is_the_path_that_never_heard_of_it(hip_lib, monkeypatch, path):
    _clear(monkeypatch)
    if path == "wave":
        tp = tc.shape_tapes()["nx65"]
        x, p = tc.shape_point(tp, 11)[:2]
        X0, P = np.stack([x, 0.9 * x, 1.1 * x]), np.tile(p, (3, 1))
        oh_debug(monkeypatch, tape_lbfgs=4, tape_wave_nt=64, tape_wave_regs="lds")
        kw = dict(jit=False, wave=True, max_iter=300)
    else:
        g = np.load(os.path.join(GOLDEN, "ik_golden.npz"))
        tp, X0, P = _ik_tape(), g["x0"][:20], g["p"][:20]
        kw = dict(jit=path == "jit", wave=False)
    plain = TapeBackend(tp, **kw)
    off = TapeBackend(tp, options={"tape_newton": 0}, **kw)
    try:
        assert (plain.flag("tape_wave") >= 1) == (path == "wave") == (off.flag("tape_wave") >= 1) and plain.jit == off.jit == (path == "jit")
        a, b = plain.solve(X0, P), off.solve(X0, P)
        assert off.flag("tape_newton") == 0 and plain.flag("tape_newton") == 0
        assert tc.same(a.x, b.x).all() and tc.same(a.f, b.f).all() and np.array_equal(a.iters, b.iters) and np.array_equal(a.status, b.status)
        off.set_option("tape_newton", 1)  # and back: the evaluator is rebuilt, the bits are those again
        off.set_option("tape_newton", 0)
        c = off.solve(X0, P)
        assert tc.same(a.x, c.x).all() and np.array_equal(a.iters, c.iters)
    finally:
        plain.close()
        off.close()


def test_generated_source_has_no_text_of_the_new_header(hip_lib):
    src, _ = TapeBackend.generated_source(_ik_tape())
    for word in ("tape_newton", "hess_vec", "TapeNewtonWork", "OH_TAPE_NEWTON_H"):
        assert word not in src
    assert "tape_solve_instance" in src


def test_refusals_before_any_device_call(hip_lib, monkeypatch):
    from optas_amd.backend import PointMassBackend

    _, tp, x, p, lam, mu, rho = next(c for c in N.merit_cases() if c[0] == "random2" and c[6] == 1.0)
    nx = int(tp.nx)
    ptr = _lib._ptr
    x, p, lam, mu = (np.ascontiguousarray(a[None]) for a in (x, p, lam, mu))
    V, HV, g = np.ascontiguousarray(np.eye(nx)[None]), np.empty((1, nx, nx)), np.empty((1, nx))
    steps, hvps = np.zeros(1, np.int32), np.zeros(1, np.int32)
    pm = PointMassBackend()
    be = _interp(monkeypatch, tp)
    try:
        assert hip_lib.oh_set_option(pm._h, b"tape_newton", C.c_double(1.0)) == 1 and b"OH_PROBLEM_TAPE" in hip_lib.oh_last_error()
        assert hip_lib.oh_set_option(be._h, b"tape_newton_cg", C.c_double(-1.0)) == 1 and b"tape_newton_cg" in hip_lib.oh_last_error()
        assert be.get_option("tape_newton_cg") == -1 and be.get_option("tape_newton") == 0  # the defaults
        f = hip_lib.oh_tape_phi_hvp
        assert f(be._h, 1, ptr(x), ptr(p), ptr(lam), ptr(mu), rho, nx, ptr(V), ptr(HV), ptr(g)) == 0
        assert f(be._h, 1, ptr(x), ptr(p), ptr(lam), ptr(mu), rho, nx, ptr(V), ptr(HV), None) == 0  # grad is optional
        for args in ((None, 1, ptr(x), ptr(p), ptr(lam), ptr(mu), rho, nx, ptr(V), ptr(HV), ptr(g)), (be._h, 1, None, ptr(p), ptr(lam), ptr(mu), rho, nx, ptr(V), ptr(HV), ptr(g)),
                     (be._h, 1, ptr(x), ptr(p), ptr(lam), ptr(mu), rho, nx, None, ptr(HV), ptr(g)), (be._h, 1, ptr(x), ptr(p), ptr(lam), ptr(mu), rho, nx, ptr(V), None, ptr(g))):
            assert f(*args) == 1 and b"oh_tape_phi_hvp" in hip_lib.oh_last_error() and b"null" in hip_lib.oh_last_error()
        assert f(be._h, 1, ptr(x), ptr(p), None, ptr(mu), rho, nx, ptr(V), ptr(HV), ptr(g)) == 1 and b"bad sizes" in hip_lib.oh_last_error()  # the tape has >= rows
        assert f(be._h, 0, ptr(x), ptr(p), ptr(lam), ptr(mu), rho, nx, ptr(V), ptr(HV), ptr(g)) == 1
        assert f(be._h, 1, ptr(x), ptr(p), ptr(lam), ptr(mu), rho, 0, ptr(V), ptr(HV), ptr(g)) == 1
        assert f(be._h, 1, ptr(x), ptr(p), ptr(lam), ptr(mu), 0.0, nx, ptr(V), ptr(HV), ptr(g)) == 1 and b"penalty" in hip_lib.oh_last_error()
        assert f(pm._h, 1, ptr(x), ptr(p), ptr(lam), ptr(mu), rho, nx, ptr(V), ptr(HV), ptr(g)) == 3  # OH_ERR_STATE
        s = hip_lib.oh_tape_newton_stats
        for args in ((None, 1, ptr(steps), ptr(hvps)), (be._h, 1, None, ptr(hvps)), (be._h, 1, ptr(steps), None)):
            assert s(*args) == 1 and b"oh_tape_newton_stats" in hip_lib.oh_last_error() and b"null" in hip_lib.oh_last_error()
        assert s(be._h, 1, ptr(steps), ptr(hvps)) == 3 and s(pm._h, 1, ptr(steps), ptr(hvps)) == 3  # no Newton-CG solve yet; not a tape handle
    finally:
        be.close()
        pm.close()


# ---- 5. through HIPSolver ---------------------------------------------------------------------------------------------------------------------------------------
def test_planar_ik_through_hipsolver(hip_lib, monkeypatch):
    """examples/planar_ik.py with solver_options={"tape_newton": 1}: the assertions tests/test_tape.py makes for the BFGS path, against this solver's port."""
    from examples.planar_ik import setup_solver as planar

    _clear(monkeypatch)
    robot, solver = planar(solver_options={"tape_newton": 1})
    try:
        solver.reset_initial_seed({f"{robot.get_name()}/q/x": [np.pi / 2.0, 0.0, 0.0]})
        sol = solver.solve()
        be = solver.backend
        assert isinstance(be, TapeBackend) and be.newton and be.flag("tape_newton") == 1 and not be.jit and not be.wave
        q = np.asarray(sol[f"{robot.get_name()}/q"]).reshape(-1)
        r = N.solve_tape_newton(solver._spec.tape, np.array([np.pi / 2, 0.0, 0.0]), np.zeros(0))
        steps, hvps = be.newton_stats(1)
        print("planar IK: q", q, "port", r["x"], "iters", solver.stats()["iterations"], "steps", steps, "products", hvps, "port", r["evals"] + r["hvps"], r["steps"], r["hvps"])
        assert solver.did_solve() and np.abs(q - r["x"]).max() < 1e-7 and abs(solver.stats()["f"][0] - r["f"]) < 1e-9
        assert np.abs(np.asarray(robot.get_global_link_position("end", q)).reshape(-1)[:2] - [1.2, 0.2]).max() < 1e-8
        o = solver.opt
        x = o.decision_variables.dict2vec(sol)
        assert o.k(x, np.zeros(0)).min() > -1e-9 and o.g(x, np.zeros(0)).min() > -1e-9 and np.abs(o.h(x, np.zeros(0))).max() < 1e-8
    finally:
        solver.backend.close()
