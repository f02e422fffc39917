"""oh_tape_hvp on the wavefront evaluator (option tape_hvp_wave; optas_amd/csrc/oh_tape_wave.hip:k_tape_wave_hvp): one block per (instance, direction) runs the
handle's level schedule forward with tangents and backward with the adjoints' directional derivatives, registers in LDS or in global memory.

Variants, each confirmed through the handle's flags after every call: wave64 (one wavefront, LDS), wave256_lds, wave256_global; handles are created the way
tests/test_gpu_tape_evaluators.py:Handles creates them.  References (tests/tape_hvp_ref.py): second differences of the 60-digit interpreter where a cached
one exists, otherwise the float64 port, which tests/test_tape_hvp_cpu.py holds to mp at a quarter of the tolerance.  The port is always run on be.tape, the
tape the handle holds; the cached mp references belong to the tape as written, and where the handle holds it re-associated (nx65, the only composite case
beyond 48 variables) that is the same function to all 60 digits.  Tolerance wherever a reference is involved: R.DEVICE_TOL, |got - ref|_inf <= 1e-12
max(1, |ref|_inf) per instance; symmetry in the same form.  Bit-level claims use tape_cases.same.  Every figure is printed before it is asserted; no test
asserts a time.  Every test sets the option or reads the flag "tape_hvp_path", which a library without the feature refuses."""
import numpy as np
import pytest

import tape_cases as tc
import tape_hvp_ref as R
from conftest import oh_debug
from optas_amd.backend import EliminatedTapeBackend, TapeBackend

pytestmark = pytest.mark.gpu

TOL = R.DEVICE_TOL
WAVE_OPTS = {"wave64": dict(tape_wave_nt=64, tape_wave_regs="lds"), "wave256_lds": dict(tape_wave_nt=256, tape_wave_regs="lds"),
             "wave256_global": dict(tape_wave_nt=256, tape_wave_regs="global")}
PATH = {"wave64": 1, "wave256_lds": 1, "wave256_global": 2}
VARIANTS = tuple(WAVE_OPTS)
ON_ALL_VARIANTS = ("random8", "mixed_level", "same_operand", "many_loads", "dead")
BRANCH_NAMES = ([f"fanout{k}" for k in (0, 1, 3, 4, 64)] + [f"width{w}" for w in (63, 64, 65, 255, 256, 257)] + [f"depth{d}" for d in range(1, 8)] +
                [f"nx{n}" for n in (1, 63, 64, 257)] + ["direct_p_cost", "direct_const_cost", "rows300"])


def _clear(monkeypatch):
    oh_debug(monkeypatch, tape_wave=None, tape_lbfgs=None, tape_wave_nt=None, tape_wave_regs=None, tape_lds_max=None, tape_hvp_work_mb=None)


def _wave(monkeypatch, tp, v, option=1):
    """A wavefront handle of the variant; option None: a handle that never hears of tape_hvp_wave."""
    _clear(monkeypatch)
    oh_debug(monkeypatch, tape_lbfgs=4, **WAVE_OPTS[v])
    be = TapeBackend(tp, jit=False, wave=True)
    _clear(monkeypatch)
    assert be.flag("tape_wave") >= 1, v
    if option is not None:
        be.set_option("tape_hvp_wave", option)
        assert be.get_option("tape_hvp_wave") == option
    return be


def _interp(monkeypatch, tp):
    _clear(monkeypatch)
    oh_debug(monkeypatch, tape_wave=0)
    be = TapeBackend(tp, jit=False, wave=False)
    _clear(monkeypatch)
    assert be.flag("tape_wave") == 0 and not be.jit and be.tape is tp
    return be


def _case(name):
    return next(c for c in R.composite_cases() if c[0] == name)


def _asym(H, scale=None):
    return float(np.abs(H - H.T).max()) / max(1.0, float(np.abs(H if scale is None else scale).max()))


def _same(a, b, what):
    ok = tc.same(a, b)
    assert ok.all(), (what, np.argwhere(~ok)[:5].tolist(), np.asarray(a)[~ok][:5], np.asarray(b)[~ok][:5])


# ---- 1. every differentiable opcode alone -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", sorted(tc.DIFF_OPS), ids=lambda o: tc.OP_NAME[o])
def test_every_differentiable_opcode_alone(hip_lib, monkeypatch, o):
    tp = tc.single_op_tape(o)
    X, ref = R.single_op_lines(o), R.single_op_reference(o)
    for v in VARIANTS:
        be = _wave(monkeypatch, tp, v)
        try:
            assert be.tape is tp
            H = be.hessian(X, np.zeros((len(X), 0)), np.ones((len(X), 1)))  # all lines of the opcode in one batch
            assert be.flag("tape_hvp_path") == PATH[v], v
        finally:
            be.close()
        assert H.shape == (len(X), 2, 2)
        for x, got, want in zip(X, H, ref):
            ok, err = R.within(got, want, TOL)
            print(v, tc.OP_NAME[o], x, "error", err, "asymmetry", _asym(got))
            assert ok, (v, tc.OP_NAME[o], x, got, want, err)
            assert _asym(got) <= TOL


# ---- 2. composite tapes against mp (5. the gradient against the port) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.composite_cases()])
def test_composite_tapes_against_mp(hip_lib, monkeypatch, name):
    _, tp, x, p, seeds, v = _case(name)
    ref = R.composite_reference(name)
    for var in (VARIANTS if name in ON_ALL_VARIANTS else ("wave256_lds",)):
        be = _wave(monkeypatch, tp, var)
        try:
            hv, g = be.hvp(x[None], p[None], seeds[None], v[None, None])
            assert be.flag("tape_hvp_path") == PATH[var], var
            H = be.hessian(x[None], p[None], seeds[None])[0]
            assert be.flag("tape_hvp_path") == PATH[var], var
            g_port = R.hvp_port(be.tape, x, p, seeds, v)[1]
        finally:
            be.close()
        ok_v, e_v = R.within(hv[0, 0], ref["hv"], TOL)
        ok_h, e_h = R.within(H, ref["H"], TOL)
        ok_g, e_g = R.within(g[0], g_port, TOL)
        asym = _asym(H, ref["H"])
        print(var, name, "len", len(tp.op), "nx", int(tp.nx), "H v error", e_v, "dense error", e_h, "asymmetry", asym, "gradient error", e_g,
              "|H|", float(np.abs(ref["H"]).max()))
        assert ok_v, (var, name, e_v)
        assert ok_h, (var, name, e_h)  # (dead: a non-finite dead instruction would show here)
        assert asym <= TOL, (var, name, asym)
        assert ok_g, (var, name, e_g)


# ---- 3. schedule branches, against the port ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes():
    return tc.shape_tapes()


@pytest.mark.parametrize("name", BRANCH_NAMES)
def test_schedule_branches_against_the_port(hip_lib, monkeypatch, shapes, name):
    tp = shapes[name]
    nx = int(tp.nx)
    x, p = tc.shape_point(tp, 11)[:2]
    seeds = R.seed_vector(tp)
    v = np.random.default_rng(29).uniform(-1.0, 1.0, nx)
    want = {}
    for var in VARIANTS:
        be = _wave(monkeypatch, tp, var)
        try:
            if not want:  # (beyond 48 variables the handle holds the tape re-associated: every variant the same one)
                want["hv"], want["g"] = R.hvp_port(be.tape, x, p, seeds, v)
                if nx <= 8:
                    want["H"] = R.hessian_port(be.tape, x, p, seeds)
                want["op"] = np.asarray(be.tape.op).copy()
            assert np.array_equal(want["op"], be.tape.op), var
            hv, g = be.hvp(x[None], p[None], seeds[None], v[None, None])
            assert be.flag("tape_hvp_path") == PATH[var], var
            H = be.hessian(x[None], p[None], seeds[None])[0] if nx <= 8 else None
            assert be.flag("tape_hvp_path") == PATH[var], var
        finally:
            be.close()
        ok_v, e_v = R.within(hv[0, 0], want["hv"], TOL)
        ok_g, e_g = R.within(g[0], want["g"], TOL)
        print(var, name, "nx", nx, "H v error", e_v, "gradient error", e_g, "|H v|", float(np.abs(want["hv"]).max()))
        assert ok_v, (var, name, e_v)
        assert ok_g, (var, name, e_g)
        if H is not None:
            ok_h, e_h = R.within(H, want["H"], TOL)
            print(var, name, "dense error", e_h, "asymmetry", _asym(H, want["H"]))
            assert ok_h, (var, name, e_h)
            assert _asym(H, want["H"]) <= TOL


# ---- 4. bits ------------------------------------------------------------------------------------------------------------------------------------------
def _spec8_batch(B, nv, seed):
    _, tp, x, p, seeds, _ = _case("random8")
    rng = np.random.default_rng(seed)
    X = x[None] + rng.uniform(-0.02, 0.02, (B, int(tp.nx)))
    P = np.tile(p, (B, 1))
    S = np.tile(seeds, (B, 1))
    S[:, 1:] *= rng.uniform(0.5, 1.5, (B, S.shape[1] - 1))
    V = rng.uniform(-1.0, 1.0, (B, nv, int(tp.nx)))
    return tp, X, P, S, V


@pytest.mark.parametrize("var", VARIANTS)
def test_units_alone_and_at_any_position(hip_lib, monkeypatch, var):
    """B = 13, nv = 5 on the tape with every opcode: every instance alone, one of its directions without the others, a permuted batch."""
    tp, X, P, S, V = _spec8_batch(13, 5, 41)
    be = _wave(monkeypatch, tp, var)
    try:
        hv, g = be.hvp(X, P, S, V)
        assert be.flag("tape_hvp_path") == PATH[var] and np.isfinite(hv).all()
        for b in range(13):
            h1, g1 = be.hvp(X[b : b + 1], P[b : b + 1], S[b : b + 1], V[b : b + 1])
            _same(h1[0], hv[b], (var, "alone", b))
            _same(g1[0], g[b], (var, "alone, gradient", b))
            h0, g0 = be.hvp(X[b : b + 1], P[b : b + 1], S[b : b + 1], V[b : b + 1, 3:4])  # one of its directions without the others
            _same(h0[0, 0], hv[b, 3], (var, "one direction", b))
            _same(g0[0], g[b], (var, "one direction, gradient", b))
        perm = np.random.default_rng(2).permutation(13)
        hp, gp = be.hvp(X[perm], P[perm], S[perm], V[perm])
        assert be.flag("tape_hvp_path") == PATH[var]
        _same(hp, hv[perm], (var, "permuted"))
        _same(gp, g[perm], (var, "permuted, gradient"))
        ok, err = R.within(hv[12, 4], R.hvp_port(be.tape, X[12], P[12], S[12], V[12, 4])[0], TOL)
        print(var, "unit 64 against the port", err)
        assert ok
    finally:
        be.close()


@pytest.mark.parametrize("var", VARIANTS)
def test_dense_columns_are_unit_products(hip_lib, monkeypatch, var):
    """Column d of V = NULL is the product with e_d at nv = 1, bit for bit."""
    _, tp, x, p, seeds, _ = _case("random8")
    nx = int(tp.nx)
    be = _wave(monkeypatch, tp, var)
    try:
        Hd, gd = be._hvp(x[None], p[None], seeds[None], nx, None)
        assert be.flag("tape_hvp_path") == PATH[var]
        for d in range(nx):
            col, g1 = be.hvp(x[None], p[None], seeds[None], np.eye(nx)[d][None, None])
            assert be.flag("tape_hvp_path") == PATH[var]
            _same(col[0, 0], Hd[0, d], (var, d))
            _same(g1, gd, (var, d, "gradient"))
    finally:
        be.close()


def _batch_of(name, shapes, B, nv, seed):
    if name in shapes:
        tp = shapes[name]
        x, p = tc.shape_point(tp, 11)[:2]
        seeds = R.seed_vector(tp)
    else:
        _, tp, x, p, seeds, _ = _case(name)
    rng = np.random.default_rng(seed)
    X = x[None] + rng.uniform(-0.02, 0.02, (B, int(tp.nx)))
    return tp, X, np.tile(p, (B, 1)), np.tile(seeds, (B, 1)), rng.uniform(-1.0, 1.0, (B, nv, int(tp.nx)))


@pytest.mark.parametrize("name", ["random8", "mixed_level", "nx65"])
def test_block_width_and_placement_give_the_same_bits(hip_lib, monkeypatch, shapes, name):
    tp, X, P, S, V = _batch_of(name, shapes, 3, 2, 7)
    out = {}
    for var in VARIANTS:
        be = _wave(monkeypatch, tp, var)
        try:
            hv, g = be.hvp(X, P, S, V)
            assert be.flag("tape_hvp_path") == PATH[var]
            H = be.hessian(X, P, S) if int(tp.nx) <= 8 else None
            assert be.flag("tape_hvp_path") == PATH[var]
            out[var] = (hv, g, H)
        finally:
            be.close()
    assert np.isfinite(out["wave256_lds"][0]).all()
    for var in ("wave256_global", "wave64"):
        _same(out[var][0], out["wave256_lds"][0], (name, var, "H v"))
        _same(out[var][1], out["wave256_lds"][1], (name, var, "gradient"))
        if out[var][2] is not None:
            _same(out[var][2], out["wave256_lds"][2], (name, var, "dense"))


def _n_reg(tp):
    """Registers of the wave schedule (oh_tape_wave_build): zero, trash, one per variable, one per live instruction that is not a load, -1 where a live NEG needs it."""
    live, op = R._live(tp), np.asarray(tp.op)
    return 2 + int(tp.nx) + int((live & (op != 1)).sum()) + int((live & (op == 7)).any())


def test_chunked_launches_give_the_same_bits(hip_lib, monkeypatch):
    """Registers in global memory, B = 3, nv = 5: with the work area's budget at two units a launch the 15 units take 8 launches (one unit in the last),
    the boundaries fall inside instances, and every bit stays."""
    tp, X, P, S, V = _spec8_batch(3, 5, 43)
    per_unit = 8 * 4 * _n_reg(tp)
    be = _wave(monkeypatch, tp, "wave256_global")
    try:
        hv, g = be.hvp(X, P, S, V)
        assert be.flag("tape_hvp_path") == 2 and be.flag("tape_hvp_launches") == 1 and be.get_option("tape_hvp_work_mb") == 256
        be.set_option("tape_hvp_work_mb", 2.5 * per_unit / 2.0 ** 20)
        hc, gc = be.hvp(X, P, S, V)
        print("launches", be.flag("tape_hvp_launches"), "bytes per unit", per_unit)
        assert be.flag("tape_hvp_path") == 2 and be.flag("tape_hvp_launches") == 8
        _same(hc, hv, "chunked H v")
        _same(gc, g, "chunked gradient")
        Hc = be.hessian(X, P, S)  # V = NULL across the same boundaries
        assert be.flag("tape_hvp_launches") == 8
        be.set_option("tape_hvp_work_mb", 1e-9)  # at least one unit goes per launch
        h1, _ = be.hvp(X, P, S, V)
        assert be.flag("tape_hvp_launches") == 15
        _same(h1, hv, "one unit a launch")
        be.set_option("tape_hvp_work_mb", 256)
        _same(Hc, be.hessian(X, P, S), "chunked dense")
        assert be.flag("tape_hvp_launches") == 1 and be.flag("tape_hvp_path") == 2
    finally:
        be.close()


# ---- 5. the gradient is phi's sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", VARIANTS)
def test_gradient_has_the_bits_of_phi(hip_lib, monkeypatch, shapes, var):
    tp, X, P, _, V = _batch_of("rows_none", shapes, 5, 2, 19)
    be = _wave(monkeypatch, tp, var)
    try:
        _, g = be.hvp(X, P, np.ones((5, 1)), V)
        assert be.flag("tape_hvp_path") == PATH[var]
        g_phi = be.phi(X, P, None, None, 10.0)["grad"]
        assert be.flag("tape_regs_lds") == (0 if var == "wave256_global" else 1)
    finally:
        be.close()
    _same(g, g_phi, (var, "gradient against phi"))
    ok, err = R.within(g[0], R.hvp_port(tp, X[0], P[0], np.ones(1), V[0, 0])[1], TOL)
    print(var, "gradient against the port", err)
    assert ok


# ---- 6. option off is untouched ---------------------------------------------------------------------------------------------------------------------
def test_option_off_is_untouched(hip_lib, monkeypatch, shapes):
    tp, X, P, S, V = _batch_of("nx65", shapes, 3, 2, 7)
    never = _wave(monkeypatch, tp, "wave256_lds", option=None)
    off = _wave(monkeypatch, tp, "wave256_lds", option=0)
    on = _wave(monkeypatch, tp, "wave256_lds", option=1)
    try:
        h_never, g_never = never.hvp(X, P, S, V)
        assert never.flag("tape_hvp_path") == 0
        h_off, g_off = off.hvp(X, P, S, V)
        assert off.flag("tape_hvp_path") == 0 and off.flag("tape_hvp_launches") == 1
        _same(h_off, h_never, "option 0 set explicitly")
        _same(g_off, g_never, "option 0 set explicitly, gradient")
        h_on, _ = on.hvp(X, P, S, V)
        assert on.flag("tape_hvp_path") == 1
        on.set_option("tape_hvp_wave", 0)  # and back: the option is read per call, the schedule is not rebuilt
        h_back, _ = on.hvp(X, P, S, V)
        assert on.flag("tape_hvp_path") == 0 and on.flag("tape_wave") >= 1
        _same(h_back, h_never, "option switched back")
        for b in range(3):
            ok, err = R.within(h_on[b], h_never[b], TOL)  # both exact products of the same tape: the interpreter's order against the gather's
            print("instance", b, "wavefront against interpreter lanes", err)
            assert ok
        be = _interp(monkeypatch, never.tape)
        try:
            h_i0, g_i0 = be.hvp(X, P, S, V)
            assert be.flag("tape_hvp_path") == 0
            be.set_option("tape_hvp_wave", 1)  # no schedule on this handle: silently the interpreter
            h_i1, g_i1 = be.hvp(X, P, S, V)
            assert be.flag("tape_hvp_path") == 0 and be.flag("tape_wave") == 0
            _same(h_i1, h_i0, "interpreter handle with the option")
            _same(g_i1, g_i0, "interpreter handle with the option, gradient")
            _same(h_i0, h_never, "wave handle, option off, against the interpreter handle")
        finally:
            be.close()
    finally:
        for b in (never, off, on):
            b.close()


def test_one_wavefront_whose_four_columns_do_not_fit_stays_on_the_interpreter(hip_lib, monkeypatch):
    """1500 terms sin(c_i x) summed by a balanced tree: about 6000 registers.  Two columns (96 KB) fit the LDS, so the one-wavefront schedule is built; four (192 KB)
    do not, and that block width has no global placement: the product runs on the interpreter's lanes."""
    t = tc.B()
    xs = [t.x(k) for k in range(4)]
    lvl = [t.emit(8, t.emit(5, xs[i % 4], t.const(0.1 + 0.0004 * i))) for i in range(1500)]
    while len(lvl) > 1:
        lvl = [t.emit(3, lvl[i], lvl[i + 1]) if i + 1 < len(lvl) else lvl[i] for i in range(0, len(lvl), 2)]
    tp = t.tape(lvl[0], [], 0, 0, 4, 0)
    assert 8 * 2 * _n_reg(tp) < 120 * 1024 and 8 * 4 * _n_reg(tp) > 160 * 1024
    x = np.random.default_rng(3).uniform(0.2, 0.9, (1, 4))
    be = _wave(monkeypatch, tp, "wave64")
    ref = _interp(monkeypatch, tp)
    try:
        H = be.hessian(x, np.zeros((1, 0)), np.ones((1, 1)))
        assert be.flag("tape_hvp_path") == 0 and be.flag("tape_hvp_launches") == 1
        _same(H, ref.hessian(x, np.zeros((1, 0)), np.ones((1, 1))), "the interpreter's bits")
    finally:
        be.close()
        ref.close()
    big = _wave(monkeypatch, tp, "wave256_lds")  # four wavefronts: the same tape goes to global memory whatever tape_wave_regs asks for
    try:
        Hb = big.hessian(x, np.zeros((1, 0)), np.ones((1, 1)))
        assert big.flag("tape_hvp_path") == 2
    finally:
        big.close()
    ok, err = R.within(Hb[0], H[0], TOL)
    print("four wavefronts, global registers, against the interpreter", err)
    assert ok


# ---- 7. through the front door ------------------------------------------------------------------------------------------------------------------------
def test_planner_through_hipsolver(hip_lib, monkeypatch):
    import os

    from conftest import GOLDEN
    from examples.simple_joint_space_planner import setup_solver

    _clear(monkeypatch)
    g = np.load(os.path.join(GOLDEN, "planner_golden.npz"))
    B = 2
    P = g["p"][:B]
    params = {"nominal_joint_state": P[:, :7], "current_joint_state": P[:, 7:14], "position_goal": P[:, 14:17], "orientation_goal": P[:, 17:]}
    robot, solver = setup_solver(solver_options={"max_iter": 400000, "tape_hvp_wave": 1})
    _, plain = setup_solver(solver_options={"max_iter": 400000})  # never solved: its Hessian at the other solver's point and multipliers
    try:
        name = robot.get_name()
        solver.reset_parameters_batch(params)
        plain.reset_parameters_batch(params)
        solver.reset_initial_seed_batch({f"{name}/q/x": np.stack([np.tile(g["q0"].reshape(-1, 1), (1, 20))] * B)})
        solver.solve_batch()
        be = solver.backend
        assert solver.stats()["success"] and isinstance(be, EliminatedTapeBackend) and solver.opt.nx == 280
        x = solver.stats()["solution"].x
        lam, mu = be.multipliers(B)
        H = solver.lagrangian_hessian()
        assert be.flag("tape_hvp_path") in (1, 2) and be._as_written().flag("tape_wave") >= 1
        assert H.shape == (B, 280, 280) and np.isfinite(H).all()
        H_plain = plain.lagrangian_hessian(x, lam, mu)
        assert plain.backend.flag("tape_hvp_path") == 0 and plain.backend._as_written().flag("tape_wave") == 0
        columns = sorted(np.random.default_rng(12).choice(280, 8, replace=False).tolist())
        for b in range(B):
            asym = _asym(H[b])
            ok, err = R.within(H[b][columns], H_plain[b][columns], TOL)
            print("instance", b, "path", be.flag("tape_hvp_path"), "|H|", float(np.abs(H[b]).max()), "asymmetry", asym, "against the option off", err)
            assert asym <= 1e-12
            assert ok, (b, err)
        # the multipliers do not feel the option: the same call on the handle of the problem as written that a solver without it creates
        wave_handle, be._orig = be._orig, plain.backend._as_written()
        try:
            lam_plain, mu_plain = be.multipliers(B)
        finally:
            be._orig = wave_handle
        _same(lam, lam_plain, "inequality multipliers")
        _same(mu, mu_plain, "equality multipliers")
    finally:
        solver.backend.close()
        plain.backend.close()
