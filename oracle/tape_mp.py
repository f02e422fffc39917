"""ORACLE (test infrastructure, not product code) -- the instruction set of include/optas_hip.h (oh_tape_desc: 27 opcodes) and the
augmented-Lagrangian merit of csrc/oh_tape_solver.h (tape_al_ineq / tape_al_eq) restated in mpmath at 60 significant digits.  It grades the
numpy restatement oracle/tape_ref.py and, through oh_tape_phi, the three device evaluators.

Values: every register from the exact binary images of the float64 inputs and constants.

Gradient of the merit with respect to x: NOT a reverse sweep -- central differences of the mp merit, h = 1e-25 min(1, |x_k|) (1e-25 at x_k = 0;
truncation ~ h^2 = 1e-50 of the third derivative, rounding ~ 1e-60 / h = 1e-35; the working precision grows with the magnitude of the inputs, so
that x + h and the argument reduction of sin(1e22) keep 60 digits behind the point), so nothing here shares a derivative rule with the evaluators.  Where the merit is not smooth the
derivative is a convention, and a difference across the kink would not reproduce it; the conventions are this table, written from the header's text
and casadi's rules as the project states them (casadi/core/calculus.hpp), and the perturbed evaluations hold the selections of the base point:

    FMIN a b    passes to a where a <= b, else to b              (d fmin = (x <= y, !(x <= y)): a tie goes to a)
    FMAX a b    passes to a where a >= b, else to b              (a tie goes to a)
    FABS a      slope +1 for a > 0, -1 for a < 0, 0 at a = 0
    LT LE EQ NE NOT AND OR    constants (zero derivative)
    IFZ a b     b where a != 0, else the constant 0; nothing passes to the condition a
    max(0, lam - rho g) of an inequality row: the branch of the base point (at lam = rho g both sides give the seed 0)

Away from the kinks holding the selection changes nothing (h is far below the distance to any tie of float64 inputs that is not exact).
Non-finite values and signed zeros are outside mpmath (no NaN arithmetic, no -0): forward_mp raises NonFinite there, and the tests write the
expected IEEE 754 / C Annex F results of those table entries down by hand.  A register without a finite value that neither the cost nor a row
depends on (a dead instruction) is nobody's business.

Only ``tests/`` may import it.
"""
import mpmath
import numpy as np

DPS = 60
H = "1e-25"

_BINARY = frozenset([3, 4, 5, 6, 10, 15, 16, 17, 18, 19, 20, 22, 23, 24])


class NonFinite(ArithmeticError):
    """The instruction has no finite real value at this point (division by zero, sqrt / log / asin outside the domain)."""


def _dps(*arrays):
    big = max([1.0] + [abs(float(t)) for a in arrays for t in np.asarray(a, float).reshape(-1) if np.isfinite(t)])
    return DPS + int(np.ceil(np.log10(big)))


def _exact(v):
    v = float(v)
    if not np.isfinite(v):
        raise NonFinite("non-finite input")
    return mpmath.mpf(v)


def _run(tape, x, p, sel, base=None, var=-1):
    """All registers at mp inputs x, p.  sel None: decide every selection here and return them; a list: hold those.
    base, var: the registers of a run that differs from this one in variable `var` alone -- whatever does not depend on it is taken from there."""
    mp = mpmath.mp
    L = len(tape.op)
    v = [None] * L
    out = [None] * L if sel is None else sel
    decide = sel is None
    one, zero = mp.mpf(1), mp.mpf(0)
    ops, aa, bb = [int(t) for t in tape.op], [int(t) for t in tape.a], [int(t) for t in tape.b]
    dirty = [False] * L
    for i in range(L):
        o, a, b = ops[i], aa[i], bb[i]
        if base is not None:
            d = (o == 1 and a == var) or (o >= 3 and (dirty[a] or (o in _BINARY and dirty[b])))
            if not d:
                v[i] = base[i]
                continue
            dirty[i] = True
        if o == 0:
            r = _exact(tape.c[i])
        elif o == 1:
            r = x[a]
        elif o == 2:
            r = p[a]
        else:
            va = v[a]
            vb = v[b] if o in _BINARY else None
            if va is None or (o in _BINARY and vb is None):  # an operand without a finite value: so is this register; it counts once the cost or a row reads it
                v[i] = None
                continue
            if o == 3:
                r = va + vb
            elif o == 4:
                r = va - vb
            elif o == 5:
                r = va * vb
            elif o == 6:
                r = None if vb == 0 else va / vb  # (no finite value)
            elif o == 7:
                r = -va
            elif o == 8:
                r = mp.sin(va)
            elif o == 9:
                r = mp.cos(va)
            elif o == 10:
                r = None if (va == 0 and vb <= 0) else mp.atan2(va, vb)  # ATAN2(0, b <= 0): the branch cut, decided by the sign of a zero
            elif o == 11:
                r = None if va < 0 else mp.sqrt(va)
            elif o == 12:
                r = va * va
            elif o == 13:
                r = None if abs(va) > 1 else mp.asin(va)
            elif o == 14:
                if decide:
                    out[i] = 1 if va > 0 else (-1 if va < 0 else 0)
                r = out[i] * va
            elif o == 15:
                if decide:
                    out[i] = bool(va <= vb)
                r = va if out[i] else vb
            elif o == 16:
                if decide:
                    out[i] = bool(va >= vb)
                r = va if out[i] else vb
            elif 17 <= o <= 23:
                if decide:
                    t = (va < vb if o == 17 else va <= vb if o == 18 else va == vb if o == 19 else va != vb if o == 20 else va == 0 if o == 21
                         else (va != 0 and vb != 0) if o == 22 else (va != 0 or vb != 0))
                    out[i] = one if t else zero
                r = out[i]
            elif o == 24:
                if decide:
                    out[i] = bool(va != 0)
                r = vb if out[i] else zero
            elif o == 25:
                r = mp.exp(va)
            elif o == 26:
                r = None if va <= 0 else mp.log(va)
            else:
                raise ValueError(f"opcode {o}")
        v[i] = r
    return v, out


def forward_mp(tape, x, p):
    """Every register (list of mpf) at the float64 point x, p."""
    with mpmath.workdps(_dps(x, p, tape.c)):
        return _run(tape, [_exact(t) for t in x], [_exact(t) for t in p], None)[0]


def _merit(tape, v, lam, mu, rho, active):
    """tape_al_ineq / tape_al_eq summed over the rows.  active None: decide the branch of max(0, lam - rho g) per row here; a list: hold it."""
    mp = mpmath.mp
    ni, ne = int(tape.n_ineq), int(tape.n_eq)
    rows = [v[int(r)] for r in tape.out_rows]
    f = v[int(tape.out_cost)]
    if f is None or any(r is None for r in rows):
        raise NonFinite("the cost or a row has no finite value at this point (division by zero, sqrt / log / asin outside the domain, atan2 on its cut)")
    val, cm, ms = f, mp.mpf(0), mp.mpf(0)
    act = [None] * ni if active is None else active
    for i in range(ni):
        g = rows[i]
        t = lam[i] - rho * g
        if active is None:
            act[i] = bool(t > 0)
        s = t if act[i] else mp.mpf(0)
        val += (s * s - lam[i] * lam[i]) / (2 * rho)
        cm = max(cm, -g)
        ms = max(ms, abs(min(g, lam[i] / rho)))
    for j in range(ne):
        c = rows[ni + j]
        val += -mu[j] * c + rho * c * c / 2
        cm = max(cm, abs(c))
        ms = max(ms, abs(c))
    return {"merit": val, "f": f, "rows": rows, "cmax": cm, "meas": ms}, act


def merit_mp(tape, x, p, lam, mu, rho):
    """merit, f, rows, cmax, meas (mpf) of one instance."""
    with mpmath.workdps(_dps(x, p, tape.c)):
        v, _ = _run(tape, [_exact(t) for t in x], [_exact(t) for t in p], None)
        return _merit(tape, v, [_exact(t) for t in lam], [_exact(t) for t in mu], _exact(rho), None)[0]


def phi_mp(tape, x, p, lam, mu, rho, grad=True):
    """What oh_tape_phi returns for one instance, rounded to float64 at the end: dict merit, f, rows, cmax, meas, grad."""
    with mpmath.workdps(_dps(x, p, tape.c)):
        mp = mpmath.mp
        xs, ps = [_exact(t) for t in x], [_exact(t) for t in p]
        lm, mm, rh = [_exact(t) for t in lam], [_exact(t) for t in mu], _exact(rho)
        v, sel = _run(tape, xs, ps, None)
        m, act = _merit(tape, v, lm, mm, rh, None)
        out = {"merit": float(m["merit"]), "f": float(m["f"]), "rows": np.array([float(r) for r in m["rows"]]), "cmax": float(m["cmax"]), "meas": float(m["meas"]),
               "merit_mp": m["merit"], "rows_mp": m["rows"], "f_mp": m["f"]}
        if grad:
            h0 = mp.mpf(H)
            used = set(int(tape.a[i]) for i in range(len(tape.op)) if int(tape.op[i]) == 1)
            g = np.zeros(int(tape.nx))
            for k in sorted(used):
                h = h0 * min(1, abs(xs[k])) if xs[k] != 0 else h0
                xp, xm = list(xs), list(xs)
                xp[k] = xs[k] + h
                xm[k] = xs[k] - h
                fp = _merit(tape, _run(tape, xp, ps, sel, v, k)[0], lm, mm, rh, act)[0]["merit"]
                fm = _merit(tape, _run(tape, xm, ps, sel, v, k)[0], lm, mm, rh, act)[0]["merit"]
                g[k] = float((fp - fm) / (2 * h))
            out["grad"] = g
        return out


def ulp_error(got, want_mp):
    """|got - want| in units of the last place of the float64 nearest to want (subnormal spacing below the smallest normal)."""
    with mpmath.workdps(DPS):
        want = mpmath.mpf(want_mp)
        w = abs(float(want))
        spacing = float(np.spacing(w)) if w > 0 else 5e-324
        return float(abs(mpmath.mpf(float(got)) - want) / mpmath.mpf(spacing))
