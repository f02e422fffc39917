"""The float64 tape oracle (oracle/tape_ref.py: the grader of every tape test) and the composed elementary functions of optas_amd/tape.py against
mpmath (oracle/tape_mp.py, 60 digits; derivatives by differences in that precision, conventions at the kinks from its table).  CPU only.

Measures (the ones tests/test_gpu_tape_evaluators.py holds the device evaluators to):
  single instructions: IEEE operations (+ - * / sqrt, NEG, FABS, FMIN, FMAX, comparisons, logic, IFZ) within half an ulp of the exact result; the host
    math library (numpy) within 1 ulp (glibc documents its double-precision sin cos atan2 asin exp log below one ulp; measured here on the table: 0.53);
  composite tapes: values 1e-13, gradients 1e-12, relative to max(1, |reference|_max) -- as tests/test_rnea_mp_reference.py; the ORACLE must be within a
    QUARTER of those on every tape and point the generators emit, so that a failure of a device evaluator at the full threshold is the device's.
"""
import math

import mpmath
import numpy as np
import pytest

import tape_cases as tc
from optas_amd.tape import TapeBuilder
from oracle import tape_mp, tape_ref

VAL_TOL, GRAD_TOL = 1e-13, 1e-12


def test_hand_written_ieee_expectations_hold_for_the_float64_oracle():
    for o, a, b, want in tc.HAND:
        got = tc.ieee_value(o, a, b)
        assert tc.same(got, want), (tc.OP_NAME[o], a, b, got, want)
    assert set(o for o, *_ in tc.HAND) == set(range(3, 27))


def test_opcode_table_oracle_against_mp():
    _, _, operands = tc.opcode_table_lines()
    ref = tc.table_reference(operands, tc.table_multipliers(operands))
    worst, n_val, n_grad, fw, rv = {}, 0, 0, set(), set()
    for ln, line in enumerate(ref):
        for o, e in line.items():
            if e["mp"] is not None and np.isfinite(e["ieee"]):
                u = tape_mp.ulp_error(e["ieee"], e["mp"])
                worst[o] = max(worst.get(o, 0.0), u)
                assert u <= (1.0 if o in tc.LIBM_OPS else 0.5), (tc.OP_NAME[o], operands[ln][o], e["ieee"], u)
                n_val += 1
                fw.add(o)
            elif e["mp"] is not None:  # overflow: the exact value is beyond the largest double
                assert abs(e["mp"]) > 1.79e308 and np.isinf(e["ieee"]) and (e["ieee"] > 0) == (e["mp"] > 0)
            if e["grad_mp"] is not None:
                for k in range(2):
                    want, got = e["grad_mp"][k], e["grad_ref"][k]
                    if np.isfinite(want):
                        assert abs(got - want) <= 0.25 * GRAD_TOL * max(1.0, abs(want)), (tc.OP_NAME[o], operands[ln][o], got, want)
                    else:
                        assert tc.same(got, want), (tc.OP_NAME[o], operands[ln][o], got, want)
                    n_grad += 1
                if o in tc.DIFF_OPS:
                    rv.add(o)
    print("largest error of the float64 oracle in ulp per opcode:", {tc.OP_NAME[o]: round(u, 3) for o, u in sorted(worst.items())}, n_val, "values", n_grad, "slopes")
    assert fw == tc.ALL_OPS and rv == tc.DIFF_OPS and n_val > 800 and n_grad > 1200


def _check_composite(tp, x, p, lam, mu, rho, frac, what):
    r, m = tc.ref_phi(tp, x, p, lam, mu, rho), tape_mp.phi_mp(tp, x, p, lam, mu, rho)
    for k in ("merit", "f", "cmax", "meas"):
        assert abs(r[k] - m[k]) <= frac * VAL_TOL * max(1.0, abs(m[k])), (what, k, r[k], m[k])
    if len(m["rows"]):
        assert np.abs(r["rows"] - m["rows"]).max() <= frac * VAL_TOL * max(1.0, np.abs(m["rows"]).max()), what
    err = np.abs(r["grad"] - m["grad"]).max() / max(1.0, np.abs(m["grad"]).max())
    assert err <= frac * GRAD_TOL, (what, err)
    return np.abs(m["grad"]).max()


@pytest.mark.parametrize("spec", tc.RANDOM_SPECS, ids=lambda s: f"seed{s[0]}_{s[1]}ins_{s[2]}x")
def test_random_tapes_oracle_within_a_quarter_of_the_thresholds(spec):
    tp, x, p, lam, mu, rho = tc.random_tape(*spec)
    gmax = _check_composite(tp, x, p, lam, mu, rho, 0.25, spec)
    assert gmax > 1e-2  # gradients of order one, not squashed to nothing
    v = tape_ref.forward(tp, x, p)
    assert np.isfinite(v).all() and np.abs(v).max() <= 8.0  # domain-safe, magnitudes bounded


def test_random_tapes_cover_every_opcode_and_both_sides_of_the_inequality_seed():
    fw, rv, on, off = set(), set(), 0, 0
    for spec in tc.RANDOM_SPECS:
        tp, x, p, lam, mu, rho = tc.random_tape(*spec)
        f, r = tc.ops_used(tp)
        fw |= f
        rv |= r
        g = tape_ref.forward(tp, x, p)[tp.out_rows[: tp.n_ineq]]
        on += int((lam - rho * g > 0).sum())
        off += int((lam - rho * g < 0).sum())
    assert fw == tc.ALL_OPS and rv == tc.DIFF_OPS and on > 10 and off > 10


def test_schedule_shape_tapes_oracle_against_mp():
    for i, (name, tp) in enumerate(tc.shape_tapes().items()):
        _check_composite(tp, *tc.shape_point(tp, 100 + i), 0.25, name)
    tp = tc.huge_fanout_tape()
    _check_composite(tp, *tc.shape_point(tp, 7), 0.25, "huge fan-out")


def test_conventions_at_the_kinks():
    """The table of oracle/tape_mp.py, the float64 oracle and the header's text say the same at exact ties."""
    for o, a, b, want in [(15, 1.0, 1.0, (1.0, 0.0)), (16, 1.0, 1.0, (1.0, 0.0)), (15, 0.0, -0.0, (1.0, 0.0)), (16, -0.0, 0.0, (1.0, 0.0)), (15, 2.0, 1.0, (0.0, 1.0)),
                          (16, 2.0, 1.0, (1.0, 0.0)), (14, 0.0, 0.0, (0.0, 0.0)), (14, -2.0, 0.0, (-1.0, 0.0)), (24, 0.0, 3.0, (0.0, 0.0)), (24, 2.0, 3.0, (0.0, 1.0)),
                          (17, 1.0, 1.0, (0.0, 0.0)), (19, 1.0, 1.0, (0.0, 0.0)), (21, 0.0, 0.0, (0.0, 0.0)), (22, 1.0, 1.0, (0.0, 0.0))]:
        tp = tc.single_op_tape(o)
        x = np.array([a, b])
        g_ref = tape_ref.reverse(tp, tape_ref.forward(tp, x, np.zeros(0)), {2: 1.0})
        g_mp = tape_mp.phi_mp(tp, x, np.zeros(0), [], [], 1.0)["grad"]
        assert tuple(g_ref) == want and tuple(g_mp) == want, (tc.OP_NAME[o], a, b, g_ref, g_mp)


def test_reverse_sweep_multiplies_a_zero_adjoint_through():
    """include/optas_hip.h (oh_tape_phi): 0 times a non-finite partial derivative is NaN, in the oracle as on the device; IFZ cuts the path only to the
    operand it does not pass its adjoint to.  (The oracle used to skip instructions whose adjoint was exactly 0 and returned finite gradients here.)"""
    t = tc.B()
    x0 = t.x(0)
    r = t.emit(24, t.emit(17, t.const(0.0), x0), t.emit(11, x0))  # ifz(x > 0, sqrt(x))
    tp = t.tape(r, [], 0, 0, 1, 0)
    for xv, want in ((4.0, 0.25), (0.0, NAN := float("nan")), (-1.0, NAN)):
        with np.errstate(all="ignore"):
            g = tape_ref.reverse(tp, tape_ref.forward(tp, np.array([xv]), np.zeros(0)), {int(r): 1.0})
        assert tc.same(g[0], want), (xv, g)
    t = tc.B()
    s = t.emit(11, t.x(0))
    tp = t.tape(t.emit(12, t.x(1)), [s], 1, 0, 2, 0)  # sqrt(x0) >= 0 as a row whose seed is exactly 0 at lam = 0
    g = tc.ref_phi(tp, np.array([0.0, 1.0]), np.zeros(0), np.zeros(1), np.zeros(0), 1.0)["grad"]
    assert np.isnan(g[0]) and g[1] == 2.0


# ---- the composed functions of optas_amd/tape.py ----------------------------------------------------------------------------------------------
def _composed(fn, xs):
    """(values, derivatives) of a TapeBuilder composition of one variable at the points xs, by the float64 oracle."""
    tb = TapeBuilder()
    r = fn(tb, tb.x(0))
    tp = tc.make(tb.op, tb.a, tb.b, tb.c, r, [], 0, 0, 1, 0)
    val, der = [], []
    with np.errstate(all="ignore"):
        for xv in xs:
            v = tape_ref.forward(tp, np.array([xv]), np.zeros(0))
            val.append(v[r])
            der.append(tape_ref.reverse(tp, v, {int(r): 1.0})[0])
    return np.array(val), np.array(der)


def _logspace(lo, hi, n):
    return [float(v) for v in np.logspace(lo, hi, n)]


_SMALL = _logspace(-12, 0, 25)
_BOTH = lambda pts: sorted(set([-v for v in pts] + list(pts)))
COMPOSED = {  # name: (builder, mpmath function, points over the domain, ends where the composition loses digits included)
    "tanh": (lambda tb, a: tb.tanh(a), mpmath.tanh, _BOTH(_SMALL + [2.0, 10.0, 19.0, 40.0, 354.0, 355.0, 400.0, 709.0, 710.0, 1e4, 1e300])),
    "sinh": (lambda tb, a: tb.sinh(a), mpmath.sinh, _BOTH(_SMALL + [2.0, 10.0, 100.0, 700.0])),
    "cosh": (lambda tb, a: tb.cosh(a), mpmath.cosh, _BOTH(_SMALL + [2.0, 10.0, 100.0, 700.0])),
    "acos": (lambda tb, a: tb.acos(a), mpmath.acos, _BOTH([0.0, 0.3, 0.9, 1.0 - 1e-6, 1.0 - 1e-10]) + [1.0 - 1e-14]),
    "atan": (lambda tb, a: tb.atan(a), mpmath.atan, _BOTH(_SMALL + [3.0, 1e3, 1e8, 1e16, 1e100, 1e300])),
    "asinh": (lambda tb, a: tb.asinh(a), mpmath.asinh, _BOTH(_SMALL + [0.0, 3.0, 3e4, 1e9, 1e12, 1e15, 1e100, 1e150])),
    "acosh": (lambda tb, a: tb.acosh(a), mpmath.acosh, [1.0 + 1e-6, 1.0 + 1e-3, 1.5, 3.0, 1e3, 1e9, 1e15, 1e100, 1e150]),
    "atanh": (lambda tb, a: tb.atanh(a), mpmath.atanh, _BOTH(_SMALL[:-1] + [0.5, 0.9, 1.0 - 1e-6, 1.0 - 1e-10])),
    "log1p": (lambda tb, a: tb.log1p(a), mpmath.log1p, _BOTH(_SMALL[:-1]) + [-0.5, -1.0 + 1e-6, 1.0, 1e3, 1e15, 1e300]),
    "expm1": (lambda tb, a: tb.expm1(a), mpmath.expm1, _BOTH(_SMALL + [5.0, 30.0, 100.0, 700.0]) + [-745.0, -1e4]),
    "pow3": (lambda tb, a: tb.pow(a, tb.const(3.0)), lambda v: v ** 3, _BOTH(_SMALL + [7.0, 1e10, 1e100])),
    "pow-2": (lambda tb, a: tb.pow(a, tb.const(-2.0)), lambda v: v ** -2, _BOTH([1e-10, 1e-3, 0.5, 1.0, 7.0, 1e10, 1e100])),
    "pow9": (lambda tb, a: tb.pow(a, tb.const(9.0)), lambda v: v ** 9, _BOTH([1e-10, 0.5, 1.0, 1.7, 30.0, 1e30])),
    "pow64": (lambda tb, a: tb.pow(a, tb.const(64.0)), lambda v: v ** 64, _BOTH([0.5, 1.0, 1.1, 3.0, 50.0])),
    "pow0.5": (lambda tb, a: tb.pow(a, tb.const(0.5)), mpmath.sqrt, [1e-300, 1e-10, 0.5, 2.0, 1e10, 1e300]),
    "pow2.5": (lambda tb, a: tb.pow(a, tb.const(2.5)), lambda v: v ** mpmath.mpf(2.5), [1e-100, 1e-10, 1e-3, 0.5, 1.0, 2.0, 30.0, 1e10, 1e100]),
    "pow-1.3": (lambda tb, a: tb.pow(a, tb.const(-1.3)), lambda v: v ** mpmath.mpf(-1.3), [1e-100, 1e-3, 0.5, 1.0, 2.0, 30.0, 1e10, 1e100]),
    "clip": (lambda tb, a: tb.fmin(tb.fmax(a, tb.const(-0.5)), tb.const(1.5)), lambda v: min(max(v, mpmath.mpf(-0.5)), mpmath.mpf(1.5)), [-1e300, -3.0, -0.5 - 1e-9, -0.2, 0.0, 1.0, 1.5 - 1e-9, 1.6, 1e300]),
}


@pytest.mark.parametrize("name", sorted(COMPOSED))
def test_composed_functions_against_mpmath(name):
    build, fn, pts = COMPOSED[name]
    val, der = _composed(build, pts)
    with mpmath.workdps(400):  # (room for 1e300 + h)
        for xv, v, d in zip(pts, val, der):
            x = mpmath.mpf(xv)
            want = fn(x)
            h = mpmath.mpf("1e-30") * (abs(x) if x != 0 else 1)
            dwant = (fn(x + h) - fn(x - h)) / (2 * h)
            if abs(want) > 1.79e308:
                assert np.isinf(v) and (v > 0) == (want > 0), (name, xv, v)
            else:
                assert abs(mpmath.mpf(float(v)) - want) <= VAL_TOL * max(1, abs(want)), (name, xv, v, float(want))
            if abs(dwant) > 1.79e308 or abs(want) > 1.79e308:
                assert not np.isfinite(d) or abs(d) > 1e300, (name, xv, d)
            else:
                assert abs(mpmath.mpf(float(d)) - dwant) <= GRAD_TOL * max(1, abs(dwant)), (name, xv, d, float(dwant))


def test_sign_and_its_zero_derivative():
    val, der = _composed(lambda tb, a: tb.sign(a), [-1e300, -2.0, -5e-324, -0.0, 0.0, 5e-324, 3.0, 1e300])
    assert val.tolist() == [-1.0, -1.0, -1.0, 0.0, 0.0, 1.0, 1.0, 1.0] and not der.any()


def test_asinh_of_negative_arguments():
    """log(x + sqrt(x^2 + 1)) cancelled for x < 0: asinh(-3e4) 1.2e-7 off in the derivative, asinh(-1e9) = -inf with a NaN gradient."""
    pts = [-1e15, -1e12, -1e9, -3e4, -100.0, -1.0, -1e-9, 0.0, 1e-9, 3e4, 1e15]
    val, der = _composed(lambda tb, a: tb.asinh(a), pts)
    for xv, v, d in zip(pts, val, der):
        assert abs(v - math.asinh(xv)) <= 4e-16 * max(1.0, abs(math.asinh(xv))), (xv, v)
        assert abs(d - 1.0 / math.hypot(1.0, xv)) <= 1e-15, (xv, d)
