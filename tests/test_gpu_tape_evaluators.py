"""Every tape opcode, every convention and every branch of the wave schedule on every device evaluator of the generic tape family, ONE evaluation at a
time (oh_tape_phi: exactly one E::phi per instance by the evaluator oh_solve would launch), against oracle/tape_mp.py (mpmath, 60 digits).

Evaluator variants (each confirmed through the handle's flags, not assumed):
  interp          InterpEval, csrc/oh_tape.hip                       jit_global / jit_lds   generated code, work set in global memory / in LDS
  wave64          WaveEval<64, registers in LDS>                     wave256_lds / wave256_global   WaveEval<256, registers in LDS / in global memory>

Tolerances and what they rest on:
  * among evaluators: interpreter = generated code bit for bit in every output (their claim); block width and register placement of the wave evaluator bit
    for bit (its claim); wave = interpreter bit for bit in f, rows, cmax, meas and the gradient -- the gather adds in the serial sweep's order -- on every
    tape that loads each variable once.  (A tape with several X instructions of one variable: the wave schedule merges them into one register whose
    consumers it adds in ONE descending sequence, the serial sweep adds per load and then the loads: another association of the same sum; there the
    gradient is held to the mp bound.)  The merit is a reduction over rows in another order on the wave path: mp bound only.
  * against mp, single instructions: IEEE operations at most half an ulp of the result (subnormal results included).  Math-library opcodes (sin cos atan2
    asin exp log): no accuracy table of the device library is installed with the toolkit documentation on the development machines, so the bound is
    max(2 ulp, twice what the host library shows on the same table) = 2 ulp -- tests/test_tape_mp_reference.py measures the host side at 0.53 ulp and
    asserts it below 1.  Measured on the MI355X, the same on all six variants (largest error over the table, in ulp): SIN 0.503, COS 0.521, ATAN2 0.686,
    ASIN 0.483, EXP 0.501, LOG 0.409.  Results that are zero or non-finite must be the float64 of IEEE 754 / C Annex F exactly: same kind, same sign
    (tape_cases.HAND is written by hand; the rest of the table by numpy, which the CPU test pins to HAND).
  * against mp, composite tapes: relative to max(1, |reference|_max), 1e-13 for values, 1e-12 for gradients (tests/test_rnea_mp_reference.py's
    thresholds); the float64 oracle is within a quarter of them on the same tapes (CPU test), so a failure here is the device's.
"""
import ctypes as C

import numpy as np
import pytest

import tape_cases as tc
from conftest import oh_debug
from optas_amd.backend import TapeBackend
from oracle import tape_mp

pytestmark = pytest.mark.gpu

VAL_TOL, GRAD_TOL, LIBM_ULP = 1e-13, 1e-12, 2.0
JIT_MAX_LEN, JIT_MAX_LIBM = 2500, 250  # instructions / math-library calls among them (each is inlined eight times over into the solve kernels a handle is created
# with): hiprtc time of the generated evaluator stays in seconds per tape.  Larger tapes go to the interpreter and the wave evaluator only.
VARIANTS = ("interp", "jit_global", "jit_lds", "wave64", "wave256_lds", "wave256_global")
WAVE_OPTS = {"wave64": dict(tape_wave_nt=64, tape_wave_regs="lds"), "wave256_lds": dict(tape_wave_nt=256, tape_wave_regs="lds"),
             "wave256_global": dict(tape_wave_nt=256, tape_wave_regs="global")}
COVERAGE = {v: [set(), set()] for v in VARIANTS}  # opcodes each variant evaluated forward / differentiated, from the tapes actually sent (4a - 4c)
OUT = ("merit", "f", "rows", "grad", "cmax", "meas")


def _jit_ok(tp):
    return len(tp.op) <= JIT_MAX_LEN and int(np.isin(np.asarray(tp.op), sorted(tc.LIBM_OPS)).sum()) <= JIT_MAX_LIBM


def _clear(monkeypatch):
    oh_debug(monkeypatch, tape_wave=None, tape_lbfgs=None, tape_wave_nt=None, tape_wave_regs=None, tape_lds_max=None)


class Handles:
    """The evaluators of one tape: wave handles first (the backend hands trajectory-sized tapes over with their sums re-associated: THAT tape is then
    the tape of every variant and of the reference), then the interpreter and the generated code."""

    def __init__(self, monkeypatch, tp, variants=VARIANTS, expect_wave=True):
        self.be, self.tape = {}, tp
        for v in [w for w in WAVE_OPTS if w in variants]:
            _clear(monkeypatch)
            oh_debug(monkeypatch, tape_lbfgs=4, **WAVE_OPTS[v])
            be = TapeBackend(tp, jit=False, wave=True)
            if expect_wave:
                assert be.flag("tape_wave") >= 1, v
                if be.tape is not tp:
                    if self.tape is tp:
                        self.tape = be.tape
                    assert np.array_equal(self.tape.op, be.tape.op) and np.array_equal(self.tape.a, be.tape.a) and np.array_equal(self.tape.b, be.tape.b)
            self.be[v] = be
        _clear(monkeypatch)
        oh_debug(monkeypatch, tape_wave=0)
        if "interp" in variants:
            self.be["interp"] = TapeBackend(self.tape, jit=False, wave=False)
            assert self.be["interp"].flag("tape_wave") == 0 and not self.be["interp"].jit
        if ("jit_global" in variants or "jit_lds" in variants) and _jit_ok(self.tape):
            oh_debug(monkeypatch, tape_lbfgs=1)  # (one pair: the smallest work set, so that the LDS entry is in reach of as many tapes as possible)
            self.be["jit"] = TapeBackend(self.tape, jit=True, wave=False)
            assert self.be["jit"].flag("tape_wave") == 0 and self.be["jit"].jit
        _clear(monkeypatch)

    def phi(self, X, P, LAM, MU, rho, cover=True):
        """{variant: outputs} of one batch; the variant names say what actually ran."""
        out = {}
        B = len(X)
        for v, be in self.be.items():
            if v == "jit":
                be.set_option("tape_lds_max", 0)
                out["jit_global"] = be.phi(X, P, LAM, MU, rho)
                assert be.flag("tape_jit_lds") == 0
                be.set_option("tape_lds_max", 1 << 30)
                r = be.phi(X, P, LAM, MU, rho)
                if be.flag("tape_jit_lds") == 1:
                    out["jit_lds"] = r
            else:
                out[v] = be.phi(X, P, LAM, MU, rho)
                if v in WAVE_OPTS and be.flag("tape_wave") >= 1:
                    assert be.flag("tape_regs_lds") == (0 if v == "wave256_global" else 1), v
        if cover:
            fw, rv = tc.ops_used(self.tape)
            for v in out:
                if not (v in WAVE_OPTS and self.be[v].flag("tape_wave") == 0):
                    COVERAGE[v][0] |= fw
                    COVERAGE[v][1] |= rv
        return out

    def close(self):
        for be in self.be.values():
            be.close()


def _unique_loads(tp):
    loads = np.asarray(tp.a)[np.asarray(tp.op) == 1]
    return len(set(loads.tolist())) == len(loads)


def _assert_same(a, b, keys, what):
    for k in keys:
        ok = tc.same(a[k], b[k])
        assert ok.all(), (what, k, np.argwhere(~ok)[:5].tolist(), np.asarray(a[k])[~ok][:5], np.asarray(b[k])[~ok][:5])


def _among(out, tp, what):
    """The bit-for-bit claims among the evaluators."""
    if "interp" in out:
        for v in ("jit_global", "jit_lds"):
            if v in out:
                _assert_same(out[v], out["interp"], OUT, (what, v, "interp"))
    waves = [v for v in WAVE_OPTS if v in out]
    for v in waves[1:]:  # (the merit's row terms are summed per thread and then across threads: another order at another block width, like the interpreter's)
        _assert_same(out[v], out[waves[0]], [k for k in OUT if k != "merit"], (what, v, waves[0]))
    if "wave256_lds" in out and "wave256_global" in out:
        _assert_same(out["wave256_global"], out["wave256_lds"], OUT, (what, "register placement"))
    if waves and "interp" in out:
        keys = ("f", "rows", "cmax", "meas") + (("grad",) if _unique_loads(tp) else ())
        _assert_same(out[waves[0]], out["interp"], keys, (what, waves[0], "interp"))


def _against_mp(out, tp, X, P, LAM, MU, rho, what, instances=None):
    for b in (range(len(X)) if instances is None else instances):
        m = tape_mp.phi_mp(tp, X[b], P[b], LAM[b], MU[b], rho)
        gs = max(1.0, np.abs(m["grad"]).max())
        for v, r in out.items():
            for k in ("merit", "f", "cmax", "meas"):
                assert abs(r[k][b] - m[k]) <= VAL_TOL * max(1.0, abs(m[k])), (what, v, b, k, r[k][b], m[k])
            if len(m["rows"]):
                assert np.abs(r["rows"][b] - m["rows"]).max() <= VAL_TOL * max(1.0, np.abs(m["rows"]).max()), (what, v, b)
            err = np.abs(r["grad"][b] - m["grad"]).max() / gs
            assert err <= GRAD_TOL, (what, v, b, err, int(np.abs(r["grad"][b] - m["grad"]).argmax()))


def test_phi_refuses_bad_arguments_before_any_device_call(hip_lib):
    from optas_amd.backend import PointMassBackend

    tp = tc.row_tape(3)
    be = TapeBackend(tp, jit=False)
    x, lam, o = np.zeros((1, 2)), np.zeros((1, 1)), [np.zeros(2) for _ in range(6)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    good = (ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(o[4]), ptr(o[5]))
    assert hip_lib.oh_tape_phi(be._h, 1, ptr(x), None, ptr(lam), None, 1.0, *good) == 0
    assert hip_lib.oh_tape_phi(None, 1, ptr(x), None, ptr(lam), None, 1.0, *good) == 1 and b"null" in hip_lib.oh_last_error()
    assert hip_lib.oh_tape_phi(be._h, 1, None, None, ptr(lam), None, 1.0, *good) == 1
    assert hip_lib.oh_tape_phi(be._h, 0, ptr(x), None, ptr(lam), None, 1.0, *good) == 1 and b"bad sizes" in hip_lib.oh_last_error()
    assert hip_lib.oh_tape_phi(be._h, 1, ptr(x), None, None, None, 1.0, *good) == 1  # a >= row and no multipliers
    assert hip_lib.oh_tape_phi(be._h, 1, ptr(x), None, ptr(lam), None, 0.0, *good) == 1 and b"penalty" in hip_lib.oh_last_error()
    assert hip_lib.oh_tape_phi(be._h, 1, ptr(x), None, ptr(lam), None, 1.0, good[0], good[1], None, *good[3:]) == 1  # rows asked for, no buffer
    pm = PointMassBackend()
    assert hip_lib.oh_tape_phi(pm._h, 1, ptr(x), None, ptr(lam), None, 1.0, *good) == 3 and b"not an OH_PROBLEM_TAPE" in hip_lib.oh_last_error()  # OH_ERR_STATE
    pm.close()
    be.close()


# ---- (a) the opcode table --------------------------------------------------------------------------------------------------------------------------
def _table_run(monkeypatch, ops, variants, X, P, lam, mu, cover=True):
    tp = tc.opcode_table_tape(ops)
    h = Handles(monkeypatch, tp, variants)
    cols = np.concatenate([[2 * (o - 3), 2 * (o - 3) + 1] for o in ops])
    rows = np.array([o - 3 for o in ops])
    out = h.phi(X[:, cols], P[:, cols], lam[:, rows], mu[:, rows], tc.TABLE_RHO, cover)
    h.close()
    return out


def _table_all(monkeypatch, X, P, lam, mu, cover=True):
    """Every variant on the whole table.  The generated code's LDS entry takes work sets of at most 3 KB an instance: it gets the table in two halves."""
    ops = list(range(3, 27))
    out = _table_run(monkeypatch, ops, [v for v in VARIANTS if v != "jit_lds"], X, P, lam, mu, cover)
    out.pop("jit_lds", None)
    halves = [_table_run(monkeypatch, ops[:12], ["jit_lds"], X, P, lam, mu, cover), _table_run(monkeypatch, ops[12:], ["jit_lds"], X, P, lam, mu, cover)]
    assert all("jit_lds" in hf for hf in halves), "the generated code's LDS entry did not take the half tables"
    a, b = halves[0]["jit_lds"], halves[1]["jit_lds"]
    g = np.zeros_like(out["interp"]["grad"])
    g[:, :24], g[:, 24:] = a["grad"], b["grad"]
    out["jit_lds"] = {"rows": np.concatenate([a["rows"][:, :12], b["rows"][:, :12], a["rows"][:, 12:], b["rows"][:, 12:]], axis=1), "grad": g, "f": a["f"]}
    return out


def test_opcode_table_values_and_slopes_on_every_evaluator(hip_lib, monkeypatch):
    """Values of every row and the slopes of every row's own variables, per evaluator; prints the largest error against mp in ulp per math-library opcode
    (the figures of the MI355X are in the module's docstring)."""
    X, P, operands = tc.opcode_table_lines()
    lam, mu = tc.table_multipliers(operands), np.zeros((len(X), 24))
    ref = tc.table_reference(operands, lam)
    out = _table_all(monkeypatch, X, P, lam, mu)
    assert set(out) == set(VARIANTS)
    worst, bad = {v: {} for v in out}, []
    for v, r in out.items():
        for ln, line in enumerate(ref):
            for o, e in line.items():
                j, (a, b) = o - 3, operands[ln][o]
                for col in (j, 24 + j):  # the row fed from the variables and the one fed from the parameters
                    got = r["rows"][ln, col]
                    if e["mp"] is not None and np.isfinite(e["ieee"]) and e["ieee"] != 0.0:
                        u = tape_mp.ulp_error(got, e["mp"])
                        worst[v][o] = max(worst[v].get(o, 0.0), u)
                        if not u <= (LIBM_ULP if o in tc.LIBM_OPS else 0.5):
                            bad.append((v, "value", tc.OP_NAME[o], (a, b), got, e["ieee"], u))
                    elif o in (15, 16) and a == 0.0 and b == 0.0:
                        if got != 0.0:  # fmin / fmax of +0 and -0: C leaves the sign of the result open (Annex F.10.9.2, footnote); numpy and the device differ
                            bad.append((v, "value", tc.OP_NAME[o], (a, b), got, e["ieee"]))
                    elif not tc.same(got, e["ieee"]):
                        bad.append((v, "value", tc.OP_NAME[o], (a, b), got, e["ieee"]))
                got = r["grad"][ln, 2 * j: 2 * j + 2]
                if e["grad_mp"] is not None:
                    for k in range(2):
                        want = e["grad_mp"][k]
                        if not (abs(got[k] - want) <= GRAD_TOL * max(1.0, abs(want)) if np.isfinite(want) else tc.same(got[k], want)):
                            bad.append((v, "slope", tc.OP_NAME[o], (a, b), got, e["grad_mp"]))
                elif o == 12 and abs(a) > 8.9e307 and v in WAVE_OPTS:
                    # SQR where 2 a overflows: the interpreter forms (w 2) a, the wave evaluator w (a + a) -- the same number until a + a is inf, where a
                    # seed of 0 gives 0 there and NaN here.  The slope 2 a is beyond float64 either way; not worth an instruction in every pass.
                    if not (tc.same(got, e["grad_ref"]) | np.isnan(got)).all():
                        bad.append((v, "slope", tc.OP_NAME[o], (a, b), got, e["grad_ref"]))
                elif o not in tc.LIBM_OPS or not np.isfinite(e["grad_ref"]).all():
                    # no smooth finite merit here: the float64 arithmetic of the rule (math-library slopes that are finite may differ in the last places)
                    if not tc.same(got, e["grad_ref"]).all():
                        bad.append((v, "slope", tc.OP_NAME[o], (a, b), got, e["grad_ref"]))
                if o not in tc.BINARY and not (got[1] == 0.0 and not np.signbit(got[1])):  # a variable no instruction reads
                    bad.append((v, "unread variable", tc.OP_NAME[o], (a, b), got))
    for v in out:
        print(v, "largest error in ulp:", {tc.OP_NAME[o]: round(u, 3) for o, u in sorted(worst[v].items()) if o in tc.LIBM_OPS})
    for key in ("rows", "grad"):
        for v in out:
            ok = tc.same(out[v][key], out["interp"][key])
            for ln, c in np.argwhere(~ok):
                o = 3 + (c % 24 if key == "rows" else c // 2)
                if not (key == "grad" and o == 12 and abs(operands[ln][o][0]) > 8.9e307 and v in WAVE_OPTS):  # (SQR beyond the overflow of 2 a: above)
                    bad.append((v, key, "differs from the interpreter", tc.OP_NAME[o], operands[ln][o], out[v][key][ln, c], out["interp"][key][ln, c]))
    for item in bad[:60]:
        print("MISMATCH", item)
    assert not bad, (len(bad), bad[:5])
    # a line with non-finite entries leaves the other instances of its batch alone: the finite lines evaluated by themselves give the same bits
    fin = np.isfinite(X).all(axis=1)
    alone = _table_all(monkeypatch, X[fin], P[fin], lam[fin], mu[fin], cover=False)
    for v in out:
        for key in ("rows", "grad"):
            assert tc.same(alone[v][key], out[v][key][fin]).all(), (v, key)


def test_opcode_table_with_seeds_that_are_exactly_zero(hip_lib, monkeypatch):
    """lam = 0: a row with g >= 0 (or NaN: fmax(0, NaN) = 0) seeds its opcode with -0.  The sweep multiplies through (include/optas_hip.h): the slope is 0
    where the partial derivative is finite and NaN where it is not (sqrt and log at 0, division by 0) -- on every evaluator, and in the float64 oracle."""
    X, P, operands = tc.opcode_table_lines()
    lam, mu = tc.table_multipliers(operands, zero_seed=True), np.zeros((len(X), 24))
    ref = tc.table_reference(operands, lam)
    out = _table_all(monkeypatch, X, P, lam, mu)
    n_nan, bad = 0, []
    for v, r in out.items():
        for ln, line in enumerate(ref):
            for o, e in line.items():
                g = e["ieee"]
                if g >= 0.0 or np.isnan(g):
                    got = r["grad"][ln, 2 * (o - 3): 2 * (o - 3) + 2]
                    if not (np.isnan(got) | (got == 0.0)).all():
                        bad.append((v, tc.OP_NAME[o], operands[ln][o], got))
                    if not (np.isnan(got) == np.isnan(e["grad_ref"])).all() and not (o == 12 and abs(operands[ln][o][0]) > 8.9e307 and v in WAVE_OPTS):  # (SQR: see the test above)
                        bad.append((v, tc.OP_NAME[o], operands[ln][o], got, e["grad_ref"]))
                    n_nan += int(np.isnan(got).sum())
    for item in bad[:60]:
        print("MISMATCH", item)
    assert not bad and n_nan > 50, (len(bad), bad[:5], n_nan)
    l0, l1 = operands.index(next(row for row in operands if row[11] == (0.0, 0.0))), operands.index(next(row for row in operands if row[6] == (1.0, 0.0)))
    for v, r in out.items():
        assert np.isnan(r["grad"][l0, 2 * (11 - 3)]) and np.isnan(r["grad"][l1, 2 * (6 - 3)]), v  # sqrt(0): -0 * 0.5 / 0;  1 / 0 = inf >= 0: -0 / 0


def test_negation_keeps_the_sign_of_zero_on_every_evaluator(hip_lib, monkeypatch):
    """The wave evaluator computed NEG as (-a) + 0, which is +0 for a = +0: atan2(-x, c < 0) came out 2 pi away and 1 / (-x) with the other sign at x = 0."""
    t = tc.B()
    n = t.emit(7, t.x(0))
    rows = [t.emit(10, n, t.const(-1.0)), t.emit(6, t.const(1.0), n), n]
    tp = t.tape(t.emit(12, t.x(1)), rows, 0, 3, 2, 0)
    h = Handles(monkeypatch, tp)
    X = np.array([[0.0, 1.0], [-0.0, 1.0], [0.5, 1.0]])
    out = h.phi(X, np.zeros((3, 0)), np.zeros((3, 0)), np.zeros((3, 3)), 1.0, cover=False)
    h.close()
    want = np.array([[-np.pi, -np.inf, -0.0], [np.pi, np.inf, 0.0], [np.arctan2(-0.5, -1.0), -2.0, -0.5]])
    for v, r in out.items():
        assert tc.same(r["rows"], want).all(), (v, r["rows"])


def test_non_finite_constants_compile_and_evaluate(hip_lib, monkeypatch):
    """fmin(x, inf) is a legal graph; the generator used to print the constant as `inf`, which is no C++ literal: the handle could not be created."""
    t = tc.B()
    x0 = t.x(0)
    rows = [t.emit(15, x0, t.const(np.inf)), t.emit(16, x0, t.const(-np.inf)), t.emit(15, x0, t.const(np.nan)), t.emit(3, x0, t.const(-0.0))]
    tp = t.tape(t.emit(12, x0), rows, 2, 2, 1, 0)
    h = Handles(monkeypatch, tp)
    out = h.phi(np.array([[0.75], [-0.0]]), np.zeros((2, 0)), np.ones((2, 2)), np.zeros((2, 2)), 1.0, cover=False)
    h.close()
    assert "jit_global" in out and "jit_lds" in out
    for v, r in out.items():
        assert tc.same(r["rows"], np.array([[0.75] * 4, [-0.0] * 4])).all(), (v, r["rows"])
    _among(out, tp, "non-finite constants")


# ---- (b) schedule shapes ------------------------------------------------------------------------------------------------------------------------------
SHAPES = tc.shape_tapes()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_schedule_shapes(hip_lib, monkeypatch, name):
    tp0 = SHAPES[name]
    h = Handles(monkeypatch, tp0)
    tp = h.tape
    pts = [tc.shape_point(tp, 100 + sorted(SHAPES).index(name) + 1000 * k) for k in range(3)]
    X, P, LAM, MU = (np.array([pt[i] for pt in pts]).reshape(3, -1) for i in range(4))
    rho = pts[0][4]
    out = h.phi(X, P, LAM, MU, rho)
    assert {"interp", "wave64", "wave256_lds", "wave256_global"} <= set(out), set(out)
    assert ("jit_global" in out) == _jit_ok(tp)
    _among(out, tp, name)
    _against_mp(out, tp, X, P, LAM, MU, rho, name, instances=[0])
    if name == "nx1000":  # variables no instruction reads: exactly zero
        for r in out.values():
            assert not r["grad"][:, 1:-1:2].any()
    h.close()


def test_fan_out_beyond_the_schedule_s_consumer_count_falls_back_to_the_thread_path(hip_lib, monkeypatch):
    tp = tc.huge_fanout_tape()
    h = Handles(monkeypatch, tp, variants=("wave256_lds", "interp"), expect_wave=False)
    assert h.be["wave256_lds"].flag("tape_wave") == 0  # declined: 66 000 consumers of one register
    pt = tc.shape_point(tp, 7)
    args = (pt[0][None], np.zeros((1, 0)), np.zeros((1, 0)), pt[3][None], pt[4])
    out = h.phi(*args, cover=False)
    _assert_same(out["wave256_lds"], out["interp"], OUT, "fallback")
    _against_mp({"interp": out["interp"]}, tp, *args, "huge fan-out")
    h.close()


# ---- (c) random tapes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", tc.RANDOM_SPECS, ids=lambda s: f"seed{s[0]}_{s[1]}ins_{s[2]}x")
def test_random_tapes(hip_lib, monkeypatch, spec):
    tp0, x, p, lam, mu, rho = tc.random_tape(*spec)
    h = Handles(monkeypatch, tp0)
    out = h.phi(x[None], p[None], lam[None], mu[None], rho)
    _among(out, h.tape, spec)
    _against_mp(out, h.tape, x[None], p[None], lam[None], mu[None], rho, spec)
    h.close()


# ---- (d) batch placement ------------------------------------------------------------------------------------------------------------------------------
def test_an_instance_is_the_same_wherever_it_sits_in_a_batch(hip_lib, monkeypatch):
    tp, x, p, lam, mu, rho = tc.random_tape(*tc.RANDOM_SPECS[2])
    rng = np.random.default_rng(11)
    N = 1100
    X, P = x + 1e-3 * rng.standard_normal((N, tp.nx)), p + 1e-3 * rng.standard_normal((N, tp.np_))
    LAM, MU = np.tile(lam, (N, 1)), np.tile(mu, (N, 1))
    h = Handles(monkeypatch, tp, variants=("interp", "jit_global", "jit_lds", "wave64"))
    _clear(monkeypatch)
    oh_debug(monkeypatch, tape_lbfgs=4)
    h.be["wave_auto"] = TapeBackend(tp, jit=False, wave=True)
    _clear(monkeypatch)
    assert h.be["wave_auto"].flag("tape_wave") >= 1
    alone = {}
    for B in (1, 63, 513, 64, 65, N, 2):  # growing and shrinking on the same handles: buffers are reused and regrown
        res = {}
        for v, be in h.be.items():
            if v == "jit":
                for name, cap in (("jit_global", 0), ("jit_lds", 1 << 30)):
                    be.set_option("tape_lds_max", cap)
                    res[name] = be.phi(X[:B], P[:B], LAM[:B], MU[:B], rho)
            else:
                res[v] = be.phi(X[:B], P[:B], LAM[:B], MU[:B], rho)
        assert h.be["wave_auto"].flag("tape_regs_lds") == (1 if B <= 512 else 0)  # beyond 512 instances the registers move to global memory
        for v, r in res.items():
            if B == 1:
                alone[v] = r
            _assert_same({k: r[k][:1] for k in OUT}, alone[v], OUT, (v, B, "first instance"))
            if B == N:
                for i in (62, 63, 64, 512, 513, N - 1):
                    if v.startswith("jit"):
                        h.be["jit"].set_option("tape_lds_max", 0 if v == "jit_global" else 1 << 30)
                    one = (h.be["jit"] if v.startswith("jit") else h.be[v]).phi(X[i: i + 1], P[i: i + 1], LAM[i: i + 1], MU[i: i + 1], rho)
                    _assert_same({k: r[k][i: i + 1] for k in OUT}, one, OUT, (v, B, i))
    h.close()


def test_every_variant_evaluated_and_differentiated_every_opcode():
    """Computed from the tapes the tests above actually sent (4a - 4c), so that a later edit of the tables cannot silently drop an opcode.  Runs last in the file."""
    for v in VARIANTS:
        assert COVERAGE[v][0] == tc.ALL_OPS, (v, "forward", sorted(tc.ALL_OPS - COVERAGE[v][0]))
        assert COVERAGE[v][1] == tc.DIFF_OPS, (v, "reverse", sorted(tc.DIFF_OPS - COVERAGE[v][1]))
