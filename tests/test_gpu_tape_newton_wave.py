"""Truncated Newton-CG on the wavefront evaluator (options tape_newton + tape_newton_wave; optas_amd/csrc/oh_tape_wave.hip: WaveEval::hvp, k_tape_wave_newton,
k_tape_wave_merit_hvp): one block per instance runs the state machine of oh_tape_newton.h on the handle's level schedule, every CG iteration one self-contained
forward-over-reverse sweep of the merit with seed tangents; oh_tape_phi_hvp on such a handle runs that sweep, one block per (instance, direction).

Variants, confirmed through flag("tape_newton_path") after every call: wave64 (one wavefront, LDS), wave256_lds, wave256_global; the handles are created the
way tests/test_gpu_tape_hvp_wave.py:_wave creates them.  References: tests/tape_newton_ref.py -- the 60-digit merit Hessian where the composite cases have
one, the float64 port run on be.tape (the tape the handle holds, re-associated beyond 48 variables) everywhere, and the numpy state machine.  Tolerance
wherever a reference is involved: tape_hvp_ref.DEVICE_TOL, |got - ref|_inf <= 1e-12 max(1, |ref|_inf); bit claims use tape_cases.same.  Solves: |x - x_port|_inf
< 1e-7, tests/test_gpu_tape_newton.py's figure.  Every figure is printed before it is asserted; no test asserts a time.  Every test sets tape_newton_wave or
reads the flag "tape_newton_path": a library without the feature refuses both."""
import ctypes as C
import os

import numpy as np
import pytest

import tape_cases as tc
import tape_hvp_ref as R
import tape_newton_ref as N
from conftest import GOLDEN, oh_debug
from optas_amd.backend import EliminatedTapeBackend, TapeBackend
from oracle import tape_ref

pytestmark = pytest.mark.gpu

TOL = R.DEVICE_TOL
WAVE_OPTS = {"wave64": dict(tape_wave_nt=64, tape_wave_regs="lds"), "wave256_lds": dict(tape_wave_nt=256, tape_wave_regs="lds"),
             "wave256_global": dict(tape_wave_nt=256, tape_wave_regs="global")}
PATH = {"wave64": 1, "wave256_lds": 1, "wave256_global": 2}
VARIANTS = tuple(WAVE_OPTS)
ON_ALL_VARIANTS = ("random8", "mixed_level", "same_operand", "many_loads", "dead")  # tests/test_gpu_tape_hvp_wave.py's
BRANCH_NAMES = ([f"fanout{k}" for k in (0, 1, 3, 4, 64)] + [f"width{w}" for w in (63, 64, 65, 255, 256, 257)] + [f"depth{d}" for d in range(1, 8)] +
                [f"nx{n}" for n in (1, 63, 64, 257)] + ["direct_p_cost", "direct_const_cost", "rows300"])
NEWTON = {"tape_newton": 1, "tape_newton_wave": 1}
RANDOM60 = (15, 300, 60, 1, 1)  # tests/test_gpu_tape_newton.py's 60-variable case


def _clear(monkeypatch):
    oh_debug(monkeypatch, tape_wave=None, tape_lbfgs=None, tape_wave_nt=None, tape_wave_regs=None, tape_lds_max=None, tape_hvp_work_mb=None, tape_newton=None,
             tape_newton_cg=None, tape_newton_wave=None, tape_hvp_wave=None)


def _wave(monkeypatch, tp, v, options=NEWTON, **kw):
    """A wavefront handle of the variant (tests/test_gpu_tape_hvp_wave.py:_wave) with the Newton-CG options set at creation."""
    _clear(monkeypatch)
    oh_debug(monkeypatch, tape_lbfgs=4, **WAVE_OPTS[v])
    be = TapeBackend(tp, jit=False, wave=True, options=options, **kw)
    _clear(monkeypatch)
    assert be.flag("tape_wave") >= 1, v
    for k, val in (options or {}).items():
        assert be.get_option(k) == val
    return be


def _interp_newton(monkeypatch, tp, **kw):
    _clear(monkeypatch)
    be = TapeBackend(tp, jit=False, wave=False, options={"tape_newton": 1}, **kw)
    assert be.flag("tape_wave") == 0 and be.tape is tp
    return be


def _same(a, b, what):
    ok = tc.same(a, b)
    assert ok.all(), (what, np.argwhere(~ok)[:5].tolist(), np.asarray(a)[~ok][:5], np.asarray(b)[~ok][:5])


def _asym(H, scale):
    return float(np.abs(H - H.T).max()) / max(1.0, float(np.abs(scale).max()))


def _ik_tape():
    from examples.example import setup_solver as ik
    from optas_amd.tape import compile_problem

    return compile_problem(ik(build_only=True)[1])


@pytest.fixture(scope="module")
def shapes():
    return tc.shape_tapes()


# ---- 1. the product on the composite tapes, against mp and against the port on the handle's tape -----------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.composite_cases()])
def test_merit_hvp_composite_tapes_against_mp_and_the_port(hip_lib, monkeypatch, name):
    kept, dropped = N.kept_merit_cases()
    print("dropped by the reference itself", dropped)
    assert len(dropped) <= 2
    cases = [c for c in kept if c[0] == name]
    assert cases or name in [d[0] for d in dropped]
    for _, tp, x, p, lam, mu, rho in cases:
        H, margin = N.merit_reference(name, rho)
        nx = int(tp.nx)
        for var in (VARIANTS if name in ON_ALL_VARIANTS else ("wave256_lds",)):
            be = _wave(monkeypatch, tp, var)
            try:
                HV, g = be.phi_hvp(x[None], p[None], lam[None], mu[None], rho, np.eye(nx)[None])
                assert be.flag("tape_newton_path") == PATH[var], var
                g_phi = be.phi(x[None], p[None], lam[None], mu[None], rho)["grad"]
                assert be.flag("tape_newton_path") == PATH[var], var
                H_port = N.merit_hessian_port(be.tape, x, p, lam, mu, rho)
            finally:
                be.close()
            ok, err = R.within(HV[0], H, TOL)
            ok_p, err_p = R.within(HV[0], H_port, TOL)
            asym = _asym(HV[0], H)
            print(var, name, "rho", rho, "nx", nx, "active", int((margin > 0).sum()), "inactive", int((margin < 0).sum()), "|H|", float(np.abs(H).max()), "error", err,
                  "against the port", err_p, "asymmetry", asym)
            assert ok, (var, name, rho, err)
            assert ok_p, (var, name, rho, err_p)
            assert asym <= TOL, (var, name, rho, asym)
            _same(g, g_phi, (var, name, rho, "gradient against phi"))


# ---- 2. every differentiable opcode as a row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", sorted(tc.DIFF_OPS), ids=lambda o: tc.OP_NAME[o])
def test_merit_hvp_every_differentiable_opcode_as_a_row(hip_lib, monkeypatch, o):
    """tape_cases.row_tape(o), active (lam - rho g = 0.5) and inactive as tests/test_gpu_tape_newton.py has them; and at an exact tie lam = rho g (rho = 2: the
    product is exact, contracted or not) the product is the inactive one's (lam = 0, g > 0), bit for bit."""
    tp, rho = tc.row_tape(o), tc.TABLE_RHO
    assert rho == 2.0
    X, LAM = [], []
    for x in R.single_op_lines(o):
        g = float(tape_ref.forward(tp, x, np.zeros(0))[2])
        X.append(x), LAM.append(max(0.0, rho * g) + 0.5)
        if rho * g >= N.MARGIN:
            X.append(x), LAM.append(max(0.0, rho * g - 0.5))
    X, LAM = np.array(X), np.array(LAM).reshape(-1, 1)
    P0, V = np.zeros((len(X), 0)), np.tile(np.eye(2)[None], (len(X), 1, 1))
    refs = [N.merit_hessian_mp(tp, x, np.zeros(0), lam, np.zeros(0), rho) for x, lam in zip(X, LAM)]
    for var in VARIANTS:
        be = _wave(monkeypatch, tp, var)
        try:
            HV, _ = be.phi_hvp(X, P0, LAM, None, rho, V)
            assert be.flag("tape_newton_path") == PATH[var], var
            g_dev = be.phi(X, P0, LAM, None, rho)["rows"][:, 0]
            pos = np.isfinite(g_dev) & (g_dev > 0.0)
            tie = inact = None
            if pos.any():
                tie, _ = be.phi_hvp(X[pos], P0[pos], (rho * g_dev[pos]).reshape(-1, 1), None, rho, V[pos])
                assert be.flag("tape_newton_path") == PATH[var], var
                inact, _ = be.phi_hvp(X[pos], P0[pos], np.zeros((int(pos.sum()), 1)), None, rho, V[pos])
        finally:
            be.close()
        n_act = n_inact = 0
        for x, lam, got, (H, margin) in zip(X, LAM, HV, refs):
            assert abs(margin[0]) >= N.MARGIN
            ok, err = R.within(got, H, TOL)
            print(var, tc.OP_NAME[o], x, "margin", margin[0], "|H|", float(np.abs(H).max()), "error", err)
            assert ok, (var, tc.OP_NAME[o], x, lam, got, H, err)
            if margin[0] > 0:
                n_act += 1
            else:
                n_inact += 1
                assert not got.any()
        assert n_act >= 1 and n_inact >= 1
        print(var, tc.OP_NAME[o], "ties", int(pos.sum()))
        assert pos.any()
        _same(tie, inact, (var, tc.OP_NAME[o], "tie against inactive"))


# ---- 3. schedule shapes against the port ----------------------------------------------------------------------------------------------------------------
def _half_active(tp, x, p, rho):
    """Multipliers of the >= rows: even rows active (lam - rho g = 0.5), odd rows inactive by at least the margin where a multiplier >= 0 allows it."""
    ni = int(tp.n_ineq)
    with np.errstate(all="ignore"):
        g = tape_ref.forward(tp, x, p)[np.asarray(tp.out_rows, int)[:ni]] if ni else np.zeros(0)
    return np.array([max(0.0, rho * g[i]) + 0.5 if (i % 2 == 0 or rho * g[i] < N.MARGIN) else max(0.0, rho * g[i] - 0.5) for i in range(ni)])


@pytest.mark.parametrize("name", BRANCH_NAMES)
def test_merit_hvp_schedule_shapes_against_the_port(hip_lib, monkeypatch, shapes, name):
    tp = shapes[name]
    nx = int(tp.nx)
    x, p, _, mu, rho = tc.shape_point(tp, 11)
    v = np.random.default_rng(29).uniform(-1.0, 1.0, nx)
    want = {}
    for var in VARIANTS:
        be = _wave(monkeypatch, tp, var)
        try:
            if not want:
                lam = _half_active(be.tape, x, p, rho)
                want["hv"] = N.merit_hvp_port(be.tape, x, p, lam, mu, rho, v)
                want["g"] = N.MeritEval(be.tape, p).phi(x, lam, mu, rho)[1]
                want["op"] = np.asarray(be.tape.op).copy()
                margins = lam - rho * tape_ref.forward(be.tape, x, p)[np.asarray(be.tape.out_rows, int)[: len(lam)]] if len(lam) else np.zeros(0)
                print(name, "nx", nx, "rho", rho, "active", int((margins > 0).sum()), "inactive", int((margins < 0).sum()))
                assert (np.abs(margins) >= N.MARGIN).all()
            assert np.array_equal(want["op"], be.tape.op), var
            hv, g = be.phi_hvp(x[None], p[None], lam[None], mu[None], rho, v[None, None])
            assert be.flag("tape_newton_path") == PATH[var], var
        finally:
            be.close()
        ok_v, e_v = R.within(hv[0, 0], want["hv"], TOL)
        ok_g, e_g = R.within(g[0], want["g"], TOL)
        print(var, name, "H v error", e_v, "gradient error", e_g, "|H v|", float(np.abs(want["hv"]).max()))
        assert ok_v, (var, name, e_v)
        assert ok_g, (var, name, e_g)


# ---- 4. bits ------------------------------------------------------------------------------------------------------------------------------------------
def _rowless():
    out = [(c[0], c[1], c[2], c[3]) for c in R.composite_cases() if int(c[1].n_ineq) + int(c[1].n_eq) == 0]
    tp = tc.shape_tapes()["rows_none"]
    return out + [("rows_none", tp) + tuple(tc.shape_point(tp, 11)[:2])]


@pytest.mark.parametrize("var", VARIANTS)
def test_without_rows_the_product_is_k_tape_wave_hvps(hip_lib, monkeypatch, var):
    """No row, no seed tangent: the sweep is k_tape_wave_hvp's with the cost's seed 1, bit for bit, on the same handle."""
    cases = _rowless()
    print("tapes without rows", [c[0] for c in cases])
    assert cases
    for name, tp, x, p in cases:
        nx = int(tp.nx)
        rng = np.random.default_rng(5)
        X = x[None] + rng.uniform(-0.02, 0.02, (3, nx))
        P, V = np.tile(p, (3, 1)), rng.uniform(-1.0, 1.0, (3, 2, nx))
        be = _wave(monkeypatch, tp, var)
        try:
            be.set_option("tape_hvp_wave", 1)
            hv, g = be.phi_hvp(X, P, None, None, 10.0, V)
            assert be.flag("tape_newton_path") == PATH[var]
            hv2, g2 = be.hvp(X, P, np.ones((3, 1)), V)
            assert be.flag("tape_hvp_path") == PATH[var]
        finally:
            be.close()
        assert np.isfinite(hv).all()
        _same(hv, hv2, (var, name, "H v"))
        _same(g, g2, (var, name, "gradient"))


def _unit_batch(seed=41):
    _, tp, x, p, lam, mu, rho = next(c for c in N.merit_cases() if c[0] == "random8" and c[6] == 1.0)
    rng = np.random.default_rng(seed)
    B, nx = 5, int(tp.nx)
    X = x[None] + rng.uniform(-0.02, 0.02, (B, nx))
    LAM = np.tile(lam, (B, 1)) * rng.uniform(0.0, 2.0, (B, len(lam)))  # rows on either side of lam - rho g = 0
    MU = np.tile(mu, (B, 1)) * rng.uniform(0.5, 1.5, (B, len(mu)))
    return tp, X, np.tile(p, (B, 1)), LAM, MU, rho, rng.uniform(-1.0, 1.0, (B, 2, nx))


def test_a_units_bits_alone_at_any_position_placement_and_width(hip_lib, monkeypatch):
    tp, X, P, LAM, MU, rho, V = _unit_batch()
    out = {}
    for var in VARIANTS:
        be = _wave(monkeypatch, tp, var)
        try:
            hv, g = be.phi_hvp(X, P, LAM, MU, rho, V)
            assert be.flag("tape_newton_path") == PATH[var] and np.isfinite(hv).all() and np.isfinite(g).all()
            for b in range(5):
                h1, g1 = be.phi_hvp(X[b : b + 1], P[b : b + 1], LAM[b : b + 1], MU[b : b + 1], rho, V[b : b + 1])
                _same(h1[0], hv[b], (var, "alone", b))
                _same(g1[0], g[b], (var, "alone, gradient", b))
                h0, _ = be.phi_hvp(X[b : b + 1], P[b : b + 1], LAM[b : b + 1], MU[b : b + 1], rho, V[b : b + 1, 1:2])
                _same(h0[0, 0], hv[b, 1], (var, "one direction", b))
            perm = np.random.default_rng(2).permutation(5)
            hp, gp = be.phi_hvp(X[perm], P[perm], LAM[perm], MU[perm], rho, V[perm])
            assert be.flag("tape_newton_path") == PATH[var]
            _same(hp, hv[perm], (var, "permuted"))
            _same(gp, g[perm], (var, "permuted, gradient"))
            ok, err = R.within(hv[4, 1], N.merit_hvp_port(be.tape, X[4], P[4], LAM[4], MU[4], rho, V[4, 1]), TOL)
            print(var, "unit (4, 1) against the port", err)
            assert ok
            out[var] = (hv, g)
        finally:
            be.close()
    for var in ("wave256_global", "wave64"):
        _same(out[var][0], out["wave256_lds"][0], (var, "H v across placement / width"))
        _same(out[var][1], out["wave256_lds"][1], (var, "gradient across placement / width"))


def _solve_all(be, X0, P, B):
    res = be.solve(X0, P)
    steps, hvps = be.newton_stats(B)
    return res, steps, hvps


def test_a_solves_bits_alone_at_any_position_and_placement(hip_lib, monkeypatch):
    """One instance of the 60-variable tape alone, at every position of a batch of 5, LDS against global memory at 256 threads.  (Across widths Red associates
    differently: not claimed.)"""
    tp, x, p = tc.random_tape(*RANDOM60)[:3]
    rng = np.random.default_rng(60)
    X0 = np.stack([x] + [x + rng.uniform(-0.01, 0.01, 60) for _ in range(4)])
    P = np.tile(p, (5, 1))
    out = {}
    for var in VARIANTS:
        be = _wave(monkeypatch, tp, var, max_iter=600)
        try:
            res, steps, hvps = _solve_all(be, X0, P, 5)
            assert be.flag("tape_newton_path") == PATH[var] and be.flag("tape_newton") == 1
            print(var, "status", res.status.tolist(), "iters", res.iters.tolist(), "steps", steps.tolist(), "products", hvps.tolist())
            for b in range(5):
                r1, s1, h1 = _solve_all(be, X0[b : b + 1], P[b : b + 1], 1)
                assert be.flag("tape_newton_path") == PATH[var]
                _same(r1.x[0], res.x[b], (var, "alone, x", b))
                _same(r1.f[0], res.f[b], (var, "alone, f", b))
                assert int(r1.iters[0]) == int(res.iters[b]) and int(r1.status[0]) == int(res.status[b]) and int(s1[0]) == int(steps[b]) and int(h1[0]) == int(hvps[b])
            perm = np.random.default_rng(3).permutation(5)
            rp, sp, hp = _solve_all(be, X0[perm], P[perm], 5)
            _same(rp.x, res.x[perm], (var, "permuted, x"))
            _same(rp.f, res.f[perm], (var, "permuted, f"))
            assert np.array_equal(rp.iters, res.iters[perm]) and np.array_equal(rp.status, res.status[perm]) and np.array_equal(sp, steps[perm]) and np.array_equal(hp, hvps[perm])
            out[var] = (res, steps, hvps)
        finally:
            be.close()
    a, b = out["wave256_lds"], out["wave256_global"]
    _same(a[0].x, b[0].x, "LDS against global, x")
    _same(a[0].f, b[0].f, "LDS against global, f")
    assert np.array_equal(a[0].iters, b[0].iters) and np.array_equal(a[0].status, b[0].status) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- 5. solves against the port ---------------------------------------------------------------------------------------------------------------------------
def _against_the_port(monkeypatch, label, tp, X0, P, max_iter):
    """Device against the port on be.tape, and beside them the interpreter's Newton-CG kernel on the same tape.  Counts are printed, not asserted: the block
    reductions sum in another order than the port, so a count may move where a decision falls on a rounding.  Observed on an MI355X: none moved -- evaluations /
    steps / products equal the port's and the interpreter kernel's on every instance and all three variants (cos 10 / 8 / 8, Rosenbrock 93 / 64 / 111, quartic
    17 / 15 / 15, the 60-variable tape 20 / 12 / 25, 25 / 17 / 40, 21 / 12 / 26, nx65 23 / 10 / 12, 21 / 8 / 11, 22 / 9 / 11), |x - x_port| <= 9e-16."""
    interp = _interp_newton(monkeypatch, tp, max_iter=max_iter)
    try:
        tape = None
        for var in VARIANTS:
            be = _wave(monkeypatch, tp, var, max_iter=max_iter)
            try:
                tape = be.tape
                res, steps, hvps = _solve_all(be, X0, P, len(X0))
                assert be.flag("tape_newton_path") == PATH[var] and be.flag("tape_newton") == 1
            finally:
                be.close()
            ri = interp.solve(X0, P)
            si, hi = interp.newton_stats(len(X0))
            assert interp.flag("tape_newton_path") == 0
            for b in range(len(X0)):
                r = N.solve_tape_newton(tape, X0[b], P[b] if P.shape[1] else np.zeros(0), max_iter=max_iter)
                print(label, var, "instance", b, "device status / evaluations / steps / products", int(res.status[b]), int(res.iters[b]) - int(hvps[b]), int(steps[b]), int(hvps[b]),
                      "port", r["status"], r["evals"], r["steps"], r["hvps"], "interpreter kernel", int(ri.status[b]), int(ri.iters[b]) - int(hi[b]), int(si[b]), int(hi[b]),
                      "|x - x_port|", float(np.abs(res.x[b] - r["x"]).max()))
                assert r["status"] == 0 and int(res.status[b]) == 0
                assert np.abs(res.x[b] - r["x"]).max() < 1e-7
                assert int(res.iters[b]) >= int(hvps[b]) + 1 and int(res.iters[b]) <= max_iter
    finally:
        interp.close()


def test_three_tiny_problems_agree_with_the_port(hip_lib, monkeypatch):
    """cos (negative curvature at the start), Rosenbrock, the quartic with a singular Hessian at its optimum."""
    for name, (tp, x0) in N.tiny_problems().items():
        _against_the_port(monkeypatch, name, tp, x0[None], np.zeros((1, 0)), 2000)


def test_sixty_variables_agree_with_the_port(hip_lib, monkeypatch):
    tp, x, p = tc.random_tape(*RANDOM60)[:3]
    rng = np.random.default_rng(60)
    X0 = np.stack([x, x + rng.uniform(-0.01, 0.01, 60), x + rng.uniform(-0.01, 0.01, 60)])  # tests/test_gpu_tape_newton.py's three starts
    _against_the_port(monkeypatch, "random60", tp, X0, np.tile(p, (3, 1)), 600)


def test_sixty_five_variables_agree_with_the_port(hip_lib, monkeypatch, shapes):
    tp = shapes["nx65"]
    x, p = tc.shape_point(tp, 11)[:2]
    _against_the_port(monkeypatch, "nx65", tp, np.stack([x, 0.9 * x, 1.1 * x]), np.tile(p, (3, 1)), 600)


# ---- 6. the planner through HIPSolver -------------------------------------------------------------------------------------------------------------------
def test_planner_through_hipsolver(hip_lib, monkeypatch):
    """What test_planner_on_the_eliminated_backend_with_its_metric_as_preconditioner asserts, on the wavefront Newton-CG kernel."""
    from conftest import MED7_KIN
    from examples.simple_joint_space_planner import setup_solver
    from oracle.problems import JointSpacePlannerNLP
    from oracle.robot import OracleRobot

    _clear(monkeypatch)
    g = np.load(os.path.join(GOLDEN, "planner_golden.npz"))
    nlp = JointSpacePlannerNLP(OracleRobot(MED7_KIN))
    B = 2
    P = g["p"][:B]
    robot, solver = setup_solver(solver_options={"max_iter": 5000, "tape_newton": 1, "tape_newton_wave": 1})
    try:
        name = robot.get_name()
        solver.reset_parameters_batch({"nominal_joint_state": P[:, :7], "current_joint_state": P[:, 7:14], "position_goal": P[:, 14:17], "orientation_goal": P[:, 17:]})
        solver.reset_initial_seed_batch({f"{name}/q/x": np.stack([np.tile(g["q0"].reshape(-1, 1), (1, 20))] * B)})
        sols = solver.solve_batch()
        st = solver.stats()
        be = solver.backend
        assert isinstance(be, EliminatedTapeBackend) and be.inner.newton and be.wave and not be.jit
        steps, hvps = be.newton_stats(B)
        print("planner: path", be.flag("tape_newton_path"), "iters", st["iterations"].tolist(), "steps", steps.tolist(), "products", hvps.tolist(), "f", st["f"].tolist(),
              "golden", g["f"][:B].tolist(), "device ms", be.solve_ms())
        assert be.flag("tape_newton") == 1 and be.flag("tape_newton_path") >= 1 and be.flag("tape_wave") >= 1 and be.flag("tape_metric") == 1
        assert st["success"], st["status"]
        for b in range(B):
            x = solver.opt.decision_variables.dict2vec(sols[b])
            assert abs(st["f"][b] - g["f"][b]) <= 1e-5 * g["f"][b]
            assert abs(nlp.f(x, P[b]) - st["f"][b]) <= 1e-10 and np.abs(nlp.a(x, P[b])).max() <= 1e-12 and np.abs(nlp.h(x, P[b])).max() <= 1e-8 and nlp.g(x, P[b]).min() >= -1e-9
            assert np.abs(x - g["x"][b]).max() <= 2e-3
    finally:
        solver.backend.close()


# ---- 7. fallback, refusals, option off ------------------------------------------------------------------------------------------------------------------
def test_seven_joint_ik_stays_on_the_interpreter(hip_lib, monkeypatch):
    """nx <= 48 and no forced schedule: both options set, the solve is k_tape_solve_newton's, bit for bit."""
    _clear(monkeypatch)
    g = np.load(os.path.join(GOLDEN, "ik_golden.npz"))
    tp, X0, P = _ik_tape(), g["x0"][:20], g["p"][:20]
    both = TapeBackend(tp, options=NEWTON)
    one = TapeBackend(tp, options={"tape_newton": 1})
    try:
        assert both.flag("tape_wave") == 0 and both.tape is tp and not both.jit
        a, b = both.solve(X0, P), one.solve(X0, P)
        assert both.flag("tape_newton_path") == 0 and both.flag("tape_newton") == 1 and one.flag("tape_newton_path") == 0
        sa, sb = both.newton_stats(20), one.newton_stats(20)
        print("IK: status", a.status.tolist(), "iters", a.iters.tolist())
        assert (a.status == 0).all()
        _same(a.x, b.x, "x")
        _same(a.f, b.f, "f")
        assert np.array_equal(a.iters, b.iters) and np.array_equal(a.status, b.status) and np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    finally:
        both.close()
        one.close()


def test_refused_on_a_point_mass_handle(hip_lib):
    from optas_amd.backend import PointMassBackend

    pm = PointMassBackend()
    try:
        assert hip_lib.oh_set_option(pm._h, b"tape_newton_wave", C.c_double(1.0)) == 1 and b"OH_PROBLEM_TAPE" in hip_lib.oh_last_error()
        assert hip_lib.oh_set_option(pm._h, b"tape_newton_wave", C.c_double(0.0)) == 0
    finally:
        pm.close()


@pytest.mark.parametrize("path", ["interp", "jit", "wave"])
def test_without_tape_newton_the_option_changes_nothing(hip_lib, monkeypatch, path):
    """The set-up of tests/test_gpu_tape_newton.py:test_option_off_is_the_path_that_never_heard_of_it."""
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
    on = TapeBackend(tp, options={"tape_newton_wave": 1}, **kw)
    try:
        assert on.get_option("tape_newton_wave") == 1 and on.get_option("tape_newton") == 0
        assert (plain.flag("tape_wave") >= 1) == (path == "wave") == (on.flag("tape_wave") >= 1) and plain.jit == on.jit == (path == "jit")
        a, b = plain.solve(X0, P), on.solve(X0, P)
        assert on.flag("tape_newton") == 0 and on.flag("tape_newton_path") == 0 and plain.flag("tape_newton") == 0
        _same(a.x, b.x, (path, "x"))
        _same(a.f, b.f, (path, "f"))
        assert np.array_equal(a.iters, b.iters) and np.array_equal(a.status, b.status)
        on.set_option("tape_newton", 1)  # Newton-CG on, a solve, and off again: the evaluator is rebuilt, the bits are those again
        c = on.solve(X0, P)
        print(path, "with tape_newton: path", on.flag("tape_newton_path"), "status", c.status.tolist())
        assert on.flag("tape_newton") == 1 and on.flag("tape_newton_path") == (1 if path == "wave" else 0)
        on.set_option("tape_newton", 0)
        on.set_option("tape_newton_wave", 0)
        d = on.solve(X0, P)
        assert on.flag("tape_newton") == 0
        _same(a.x, d.x, (path, "x, switched back"))
        assert np.array_equal(a.iters, d.iters) and np.array_equal(a.status, d.status)
    finally:
        plain.close()
        on.close()


def test_generated_source_still_has_no_text_of_the_newton_solver(hip_lib):
    src, _ = TapeBackend.generated_source(_ik_tape())
    for word in ("tape_newton", "hess_vec", "TapeNewtonWork", "OH_TAPE_NEWTON_H", "tape_newton_wave"):
        assert word not in src
    assert "tape_solve_instance" in src
    be = TapeBackend(_ik_tape(), jit=False, wave=False)
    try:
        assert be.flag("tape_newton_path") == 0
    finally:
        be.close()


# ---- 8. caps ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", VARIANTS)
def test_caps(hip_lib, monkeypatch, var):
    tp, x, p = tc.random_tape(*RANDOM60)[:3]
    be = _wave(monkeypatch, tp, var, max_iter=7)
    try:
        res, steps, hvps = _solve_all(be, x[None], p[None], 1)
        print(var, "max_iter 7: iters", int(res.iters[0]), "status", int(res.status[0]), "steps", int(steps[0]), "products", int(hvps[0]))
        assert be.flag("tape_newton_path") == PATH[var]
        assert int(res.iters[0]) <= 7 and int(res.status[0]) == 1  # OH_STATUS_MAX_ITER
    finally:
        be.close()
    be = _wave(monkeypatch, tp, var, options=dict(NEWTON, tape_newton_cg=1), max_iter=600)
    try:
        res, steps, hvps = _solve_all(be, x[None], p[None], 1)
        evals = int(res.iters[0]) - int(hvps[0])
        # one product per CG-started step, and every such step goes on to at least one trial evaluation: CG-started steps <= evaluations - 1 (the first is the start's)
        print(var, "tape_newton_cg 1: status", int(res.status[0]), "evaluations", evals, "steps", int(steps[0]), "products", int(hvps[0]))
        assert be.flag("tape_newton_path") == PATH[var]
        assert int(hvps[0]) >= 1 and int(hvps[0]) <= evals - 1 and int(res.iters[0]) <= 600
    finally:
        be.close()


# ---- 9. the kernel's code-object facts --------------------------------------------------------------------------------------------------------------------
def test_kernel_info(hip_lib):
    """k_tape_wave_newton<256, LDS>: no scratch memory; 256 VGPRs and about forty AGPRs, so one wavefront per SIMD -- one block of four per CU."""
    from optas_amd import _lib

    info = _lib.kernel_info("k_tape_wave_newton")
    print(info)
    assert info["block"] == 256 and info["scratch_bytes_per_lane"] == 0 and info["registers_per_lane"] >= 256 and info["blocks_per_cu"] == 1
