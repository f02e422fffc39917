"""oh_tape_hvp on the device (optas_amd/csrc/oh_tape.hip:k_tape_hvp): exact Hessian-vector products and dense Hessians of a tape by forward-over-reverse
on the interpreter, up to HIPSolver.lagrangian_hessian.

Reference: tests/tape_hvp_ref.py -- second differences of the 60-digit interpreter with the base point's selections held (no derivative rule shared with the
device); the 300-variable tape against the float64 port only (its mp reference is 20 s per direction).  Tolerance everywhere a reference is involved:
|got - ref|_inf <= 1e-12 max(1, |ref|_inf) per instance, GRAD_TOL of tests/test_gpu_tape_evaluators.py for composite tapes (the port, on the CPU, is within a
quarter of it: tests/test_tape_hvp_cpu.py).  Symmetry is held to the same form, 1e-12 max(1, |H|_inf): an entry of magnitude |H| carries roundings of
2e-16 |H|.  The bit-level properties use tape_cases.same.  Every figure is printed before it is asserted; no test asserts a time."""
import numpy as np
import pytest

import tape_cases as tc
import tape_hvp_ref as R
from conftest import oh_debug
from optas_amd.backend import EliminatedTapeBackend, TapeBackend

pytestmark = pytest.mark.gpu

TOL = R.DEVICE_TOL


def _clear(monkeypatch):
    oh_debug(monkeypatch, tape_wave=None, tape_lbfgs=None, tape_wave_nt=None, tape_wave_regs=None, tape_lds_max=None, tape_hvp_work_mb=None)


def _interp(monkeypatch, tp):
    """An interpreter handle of the tape as it is (no generated code to compile, no wavefront schedule)."""
    _clear(monkeypatch)
    oh_debug(monkeypatch, tape_wave=0)
    be = TapeBackend(tp, jit=False, wave=False)
    assert be.flag("tape_wave") == 0 and not be.jit and be.tape is tp
    return be


def _case(name):
    return next(c for c in R.composite_cases() if c[0] == name)


def _asym(H):
    return float(np.abs(H - H.T).max()) / max(1.0, float(np.abs(H).max()))


# ---- 1. every differentiable opcode alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", sorted(tc.DIFF_OPS), ids=lambda o: tc.OP_NAME[o])
def test_every_differentiable_opcode_alone(hip_lib, monkeypatch, o):
    tp = tc.single_op_tape(o)
    X, ref = R.single_op_lines(o), R.single_op_reference(o)
    be = _interp(monkeypatch, tp)
    try:
        H = be.hessian(X, np.zeros((len(X), 0)), np.ones((len(X), 1)))  # all lines of the opcode in one batch
    finally:
        be.close()
    assert H.shape == (len(X), 2, 2)
    for x, got, want in zip(X, H, ref):
        ok, err = R.within(got, want, TOL)
        print(tc.OP_NAME[o], x, "error", err, "asymmetry", _asym(got))
        assert ok, (tc.OP_NAME[o], x, got, want, err)
        assert _asym(got) <= TOL


# ---- 2. composite tapes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.composite_cases()])
def test_composite_tapes_against_mp(hip_lib, monkeypatch, name):
    _, tp, x, p, seeds, v = _case(name)
    ref = R.composite_reference(name)
    be = _interp(monkeypatch, tp)
    try:
        hv, g = be.hvp(x[None], p[None], seeds[None], v[None, None])
        H = be.hessian(x[None], p[None], seeds[None])[0]
        _, _, g_probe = be.probe(x[None], p[None], None, seeds[None])
    finally:
        be.close()
    ok_v, e_v = R.within(hv[0, 0], ref["hv"], TOL)
    ok_h, e_h = R.within(H, ref["H"], TOL)
    asym = float(np.abs(H - H.T).max()) / max(1.0, float(np.abs(ref["H"]).max()))
    print(name, "len", len(tp.op), "nx", int(tp.nx), "H v error", e_v, "dense error", e_h, "asymmetry", asym, "|H|", float(np.abs(ref["H"]).max()))
    assert ok_v, (name, e_v)
    assert ok_h, (name, e_h)
    assert asym <= TOL, (name, asym)
    assert tc.same(g, g_probe).all()  # the first-order part is oh_tape_probe's, bit for bit


def test_three_hundred_variables_against_the_port(hip_lib, monkeypatch):
    tp, x, p = tc.random_tape(*R.BIG_SPEC)[:3]
    seeds = R.seed_vector(tp)
    V = np.random.default_rng(23).uniform(-1.0, 1.0, (1, 3, int(tp.nx)))
    be = _interp(monkeypatch, tp)
    try:
        hv, g = be.hvp(x[None], p[None], seeds[None], V)
        _, _, g_probe = be.probe(x[None], p[None], None, seeds[None])
    finally:
        be.close()
    for d in range(3):
        want, g_port = R.hvp_port(tp, x, p, seeds, V[0, d])
        ok, err = R.within(hv[0, d], want, TOL)
        print("direction", d, "error against the port", err, "|H v|", float(np.abs(want).max()))
        assert ok, (d, err)
    assert tc.same(g, g_probe).all()
    assert R.within(g[0], g_port, TOL)[0]  # (the port's gradient is the host math library's: close, not the same bits)


# ---- 3. bit-level properties --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random3", "random8", "mixed_level", "same_operand"])
def test_dense_columns_scaling_and_gradient_bits(hip_lib, monkeypatch, name):
    _, tp, x, p, seeds, v = _case(name)
    nx = int(tp.nx)
    be = _interp(monkeypatch, tp)
    try:
        Hd, gd = be._hvp(x[None], p[None], seeds[None], nx, None)
        _, _, g_probe = be.probe(x[None], p[None], None, seeds[None])
        assert tc.same(gd, g_probe).all()  # V = NULL: the gradient too
        for d in range(nx):  # column d of the dense Hessian is the product with e_d, nv = 1
            col, g1 = be.hvp(x[None], p[None], seeds[None], np.eye(nx)[d][None, None])
            assert tc.same(col[0, 0], Hd[0, d]).all(), (name, d)
            assert tc.same(g1, g_probe).all()
        V = np.random.default_rng(3).uniform(-1.0, 1.0, (1, 4, nx))
        h1, _ = be.hvp(x[None], p[None], seeds[None], V)
        h2, _ = be.hvp(x[None], p[None], seeds[None], 2.0 * V)
        assert tc.same(h2, 2.0 * h1).all()
    finally:
        be.close()


@pytest.mark.parametrize("units", [63, 64, 65])
def test_one_variable_tape_block_edges(hip_lib, monkeypatch, units):
    """nv = 1 on the one-variable tape: batches that end one lane short of a block, on its edge and one lane into the next."""
    _, tp, x, p, seeds, _ = _case("random1")
    rng = np.random.default_rng(units)
    X = x[None] + rng.uniform(-0.05, 0.05, (units, 1))
    P = np.tile(p, (units, 1))
    S = np.tile(seeds, (units, 1)) * rng.uniform(0.5, 1.5, (units, 1))
    V = rng.uniform(-1.0, 1.0, (units, 1, 1))
    be = _interp(monkeypatch, tp)
    try:
        hv, g = be.hvp(X, P, S, V)
        assert be.flag("tape_hvp_launches") == 1
        assert np.isfinite(hv).all() and np.isfinite(g).all()
        for b in (0, 31, 62, units - 1):  # alone
            h1, g1 = be.hvp(X[b : b + 1], P[b : b + 1], S[b : b + 1], V[b : b + 1])
            assert tc.same(h1[0], hv[b]).all() and tc.same(g1[0], g[b]).all(), b
        perm = rng.permutation(units)  # at any position
        hp, gp = be.hvp(X[perm], P[perm], S[perm], V[perm])
        assert tc.same(hp, hv[perm]).all() and tc.same(gp, g[perm]).all()
        want = R.hvp_port(tp, X[units - 1], P[units - 1], S[units - 1], V[units - 1, 0])[0]
        assert R.within(hv[units - 1, 0], want, TOL)[0]
    finally:
        be.close()


def _spec8_batch(B, nv, seed):
    _, tp, x, p, seeds, _ = _case("random8")
    rng = np.random.default_rng(seed)
    X = x[None] + rng.uniform(-0.02, 0.02, (B, int(tp.nx)))
    P = np.tile(p, (B, 1))
    S = np.tile(seeds, (B, 1))
    S[:, 1:] *= rng.uniform(0.5, 1.5, (B, S.shape[1] - 1))
    V = rng.uniform(-1.0, 1.0, (B, nv, int(tp.nx)))
    return tp, X, P, S, V


def test_instances_alone_and_at_any_position(hip_lib, monkeypatch):
    """B = 13, nv = 5 on the tape with every opcode: 65 units, the last instance's last direction alone in the second block."""
    tp, X, P, S, V = _spec8_batch(13, 5, 41)
    be = _interp(monkeypatch, tp)
    try:
        hv, g = be.hvp(X, P, S, V)
        assert np.isfinite(hv).all()
        for b in range(13):
            h1, g1 = be.hvp(X[b : b + 1], P[b : b + 1], S[b : b + 1], V[b : b + 1])
            assert tc.same(h1[0], hv[b]).all() and tc.same(g1[0], g[b]).all(), b
            h0, _ = be.hvp(X[b : b + 1], P[b : b + 1], S[b : b + 1], V[b : b + 1, 3:4])  # one of its directions without the others
            assert tc.same(h0[0, 0], hv[b, 3]).all(), b
        perm = np.random.default_rng(2).permutation(13)
        hp, gp = be.hvp(X[perm], P[perm], S[perm], V[perm])
        assert tc.same(hp, hv[perm]).all() and tc.same(gp, g[perm]).all()
        want = R.hvp_port(tp, X[12], P[12], S[12], V[12, 4])[0]
        ok, err = R.within(hv[12, 4], want, TOL)
        print("unit 64 against the port", err)
        assert ok
    finally:
        be.close()


def test_chunked_launches_give_the_same_bits(hip_lib, monkeypatch):
    """B = 26, nv = 5: 130 units.  With the work-area budget at one block of 64 units the call takes three launches, and the boundary between the
    first two falls inside instance 12 (units 60 .. 64)."""
    tp, X, P, S, V = _spec8_batch(26, 5, 43)
    per_unit = 8 * (4 * len(tp.op) + 3 * int(tp.nx))
    be = _interp(monkeypatch, tp)
    try:
        hv, g = be.hvp(X, P, S, V)
        assert be.flag("tape_hvp_launches") == 1 and be.get_option("tape_hvp_work_mb") == 256
        be.set_option("tape_hvp_work_mb", 100.0 * per_unit / 2.0 ** 20)  # room for 100 units: one whole block
        hc, gc = be.hvp(X, P, S, V)
        assert be.flag("tape_hvp_launches") == 3
        assert tc.same(hc, hv).all() and tc.same(gc, g).all()
        Hc = be.hessian(X, P, S)  # V = NULL across the same boundaries
        be.set_option("tape_hvp_work_mb", 256)
        assert tc.same(Hc, be.hessian(X, P, S)).all() and be.flag("tape_hvp_launches") == 1
        assert np.isfinite(hv).all()
    finally:
        be.close()


def test_wave_handle_runs_its_reassociated_tape(hip_lib, monkeypatch):
    """A handle on the wavefront path holds the tape with its sums re-associated: oh_tape_hvp runs on that tape, with the bits of an interpreter handle
    created from it."""
    tp = tc.shape_tapes()["nx65"]
    x, p = tc.shape_point(tp, 11)[:2]
    seeds = R.seed_vector(tp)
    _clear(monkeypatch)
    oh_debug(monkeypatch, tape_lbfgs=4, tape_wave_nt=64, tape_wave_regs="lds")
    wave = TapeBackend(tp, jit=False, wave=True)
    try:
        assert wave.flag("tape_wave") >= 1 and wave.tape is not tp
        be = _interp(monkeypatch, wave.tape)
        try:
            V = np.random.default_rng(9).uniform(-1.0, 1.0, (1, 3, int(tp.nx)))
            hw, gw = wave.hvp(x[None], p[None], seeds[None], V)
            hi, gi = be.hvp(x[None], p[None], seeds[None], V)
            assert tc.same(hw, hi).all() and tc.same(gw, gi).all()
            want = R.hvp_port(wave.tape, x, p, seeds, V[0, 0])[0]
            assert R.within(hw[0, 0], want, TOL)[0]
        finally:
            be.close()
    finally:
        wave.close()


def test_argument_checks(hip_lib, monkeypatch):
    import ctypes as C

    from optas_amd import _lib
    from optas_amd.backend import PointMassBackend

    _, tp, x, p, seeds, v = _case("random2")
    nx = int(tp.nx)
    ptr = _lib._ptr
    x, p, seeds, V = np.ascontiguousarray(x[None]), np.ascontiguousarray(p[None]), np.ascontiguousarray(seeds[None]), np.ascontiguousarray(v[None, None])
    HV, g = np.empty((1, nx, nx)), np.empty((1, nx))
    be = _interp(monkeypatch, tp)
    try:
        f = hip_lib.oh_tape_hvp
        assert f(be._h, 1, ptr(x), ptr(p), ptr(seeds), 1, ptr(V), ptr(HV), ptr(g)) == 0
        assert f(be._h, 1, ptr(x), ptr(p), ptr(seeds), 1, ptr(V), ptr(HV), None) == 0  # grad is optional
        assert f(be._h, 1, ptr(x), ptr(p), ptr(seeds), nx, None, ptr(HV), ptr(g)) == 0
        for args in ((None, 1, ptr(x), ptr(p), ptr(seeds), 1, ptr(V), ptr(HV), ptr(g)), (be._h, 1, None, ptr(p), ptr(seeds), 1, ptr(V), ptr(HV), ptr(g)),
                     (be._h, 1, ptr(x), ptr(p), None, 1, ptr(V), ptr(HV), ptr(g)), (be._h, 1, ptr(x), ptr(p), ptr(seeds), 1, ptr(V), None, ptr(g))):
            assert f(*args) == 1 and b"oh_tape_hvp" in hip_lib.oh_last_error() and b"null" in hip_lib.oh_last_error()
        assert f(be._h, 0, ptr(x), ptr(p), ptr(seeds), 1, ptr(V), ptr(HV), ptr(g)) == 1 and b"bad sizes" in hip_lib.oh_last_error()
        assert f(be._h, 1, ptr(x), ptr(p), ptr(seeds), 0, ptr(V), ptr(HV), ptr(g)) == 1 and b"bad sizes" in hip_lib.oh_last_error()
        assert f(be._h, 1, ptr(x), None, ptr(seeds), 1, ptr(V), ptr(HV), ptr(g)) == 1  # the tape has parameters
        assert f(be._h, 1, ptr(x), ptr(p), ptr(seeds), nx - 1, None, ptr(HV), ptr(g)) == 1 and b"nv == nx" in hip_lib.oh_last_error()
        pm = PointMassBackend()
        try:
            assert f(pm._h, 1, ptr(x), ptr(p), ptr(seeds), 1, ptr(V), ptr(HV), ptr(g)) == 3 and b"not an OH_PROBLEM_TAPE" in hip_lib.oh_last_error()  # OH_ERR_STATE
        finally:
            pm.close()
    finally:
        be.close()


# ---- 4. through the front door ------------------------------------------------------------------------------------------------------------------------
def _check_front_door(solver, as_written, x, p, columns):
    """lagrangian_hessian() of the last solve: symmetric, and equal to central differences (h = 1e-5) of the as-written tape's probe gradient of the same
    Lagrangian within 1e-6 max(1, |H|_inf) (truncation ~ 1e-10, rounding ~ 1e-11: a wrong rule is an error of order one)."""
    B, nx = x.shape
    tp = as_written.tape
    ni, ne = int(tp.n_ineq), int(tp.n_eq)
    lam, mu = solver.backend.multipliers(B)
    H = solver.lagrangian_hessian()
    assert H.shape == (B, nx, nx) and np.isfinite(H).all()
    seeds = np.concatenate([np.ones((B, 1)), -lam.reshape(B, ni), -mu.reshape(B, ne)], axis=1)
    h = 1e-5
    for b in range(B):
        scale = max(1.0, float(np.abs(H[b]).max()))
        asym = float(np.abs(H[b] - H[b].T).max()) / scale
        pts = np.repeat(x[b][None], 2 * len(columns), axis=0)
        for i, k in enumerate(columns):
            pts[2 * i, k] += h
            pts[2 * i + 1, k] -= h
        _, _, g = as_written.probe(pts, np.repeat(p[b][None], len(pts), axis=0), None, np.repeat(seeds[b][None], len(pts), axis=0))
        fd = (g[0::2] - g[1::2]) / (2.0 * h)  # row i: d grad / d x_k = H e_k
        err = float(np.abs(H[b][columns] - fd).max()) / scale
        print("instance", b, "|H|", scale, "asymmetry", asym, "against differences of the gradient", err)
        assert asym <= 1e-12
        assert err <= 1e-6
    # explicit arguments: the same matrix
    assert tc.same(solver.lagrangian_hessian(x, lam, mu), H).all()
    return H


def test_planar_ik_through_hipsolver(hip_lib, monkeypatch):
    from examples.planar_ik import setup_solver

    _clear(monkeypatch)
    robot, solver = setup_solver()
    try:
        with pytest.raises(ValueError):
            solver.lagrangian_hessian()  # before a solve x, lam and mu must all be given
        H0 = solver.lagrangian_hessian(np.array([[1.0, 0.3, -0.2]]), np.zeros((1, solver._spec.tape.n_ineq)), np.zeros((1, solver._spec.tape.n_eq)))
        assert np.abs(H0[0] - 2.0 * np.eye(3)).max() <= 1e-12  # no multipliers: the Hessian of sumsqr(q - q0)
        solver.reset_initial_seed({f"{robot.get_name()}/q/x": [np.pi / 2.0, 0.0, 0.0]})
        sol = solver.solve()
        assert solver.did_solve() and isinstance(solver.backend, TapeBackend)
        x = solver.opt.decision_variables.dict2vec(sol).reshape(1, -1)
        H = _check_front_door(solver, solver.backend, x, np.zeros((1, 0)), [0, 1, 2])
        assert np.abs(H[0] - 2.0 * np.eye(3)).max() > 1e-3  # the rows' curvature is in it (the FK row's multiplier is not zero)
    finally:
        solver.backend.close()


def test_planner_through_hipsolver_on_the_eliminated_path(hip_lib, monkeypatch):
    import os

    from conftest import GOLDEN
    from examples.simple_joint_space_planner import setup_solver

    _clear(monkeypatch)
    g = np.load(os.path.join(GOLDEN, "planner_golden.npz"))
    robot, solver = setup_solver(solver_options={"max_iter": 400000})
    try:
        name, B = robot.get_name(), 2
        P = g["p"][:B]
        solver.reset_parameters_batch({"nominal_joint_state": P[:, :7], "current_joint_state": P[:, 7:14], "position_goal": P[:, 14:17], "orientation_goal": P[:, 17:]})
        solver.reset_initial_seed_batch({f"{name}/q/x": np.stack([np.tile(g["q0"].reshape(-1, 1), (1, 20))] * B)})
        solver.solve_batch()
        assert solver.stats()["success"] and isinstance(solver.backend, EliminatedTapeBackend) and solver.opt.nx == 280
        x = solver.stats()["solution"].x
        columns = sorted(np.random.default_rng(12).choice(280, 8, replace=False).tolist())
        _check_front_door(solver, solver.backend._as_written(), x, solver._p_batch, columns)
    finally:
        solver.backend.close()


def test_other_families_say_so(hip_lib):
    from examples.figure_eight_plan import setup_solver

    _, solver = setup_solver(T=12, Tmax=10.0 * 11 / 49.0, solver_options={"max_iter": 10})
    try:
        with pytest.raises(NotImplementedError, match="figure-eight"):
            solver.lagrangian_hessian()
    finally:
        solver.backend.close()
