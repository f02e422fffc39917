"""Tapes and points shared by tests/test_tape_mp_reference.py (CPU: oracle/tape_ref.py against oracle/tape_mp.py) and
tests/test_gpu_tape_evaluators.py (GPU: the three device evaluators through oh_tape_phi): the per-opcode table with its edge operands, the
hand-written IEEE 754 / C Annex F expectations of the entries mpmath cannot state, the synthetic schedule shapes and the seeded generator of
domain-safe random tapes."""
import math

import numpy as np

from optas_amd.tape import Tape
from oracle import tape_ref

BINARY = frozenset([3, 4, 5, 6, 10, 15, 16, 17, 18, 19, 20, 22, 23, 24])
ALL_OPS = frozenset(range(3, 27))
DIFF_OPS = frozenset([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 24, 25, 26])  # opcodes with a derivative rule (17 .. 23 are piecewise constant)
LIBM_OPS = frozenset([8, 9, 10, 13, 25, 26])  # backed by the math library; the rest are exact or correctly rounded IEEE operations
OP_NAME = "CONST X P ADD SUB MUL DIV NEG SIN COS ATAN2 SQRT SQR ASIN FABS FMIN FMAX LT LE EQ NE NOT AND OR IFZ EXP LOG".split()

INF, NAN = float("inf"), float("nan")
TINY, MINN = 5e-324, 2.2250738585072014e-308  # smallest subnormal, smallest normal


def make(op, a, b, c, cost, rows, n_ineq, n_eq, nx, np_):
    return Tape(np.asarray(op, np.int32), np.asarray(a, np.int32), np.asarray(b, np.int32), np.asarray(c, np.float64), int(cost),
                np.asarray(rows, np.int32).reshape(-1), int(n_ineq), int(n_eq), int(nx), int(np_))


class B:
    """Instruction lists with no folding and no sharing: what is asked for is what the tape holds."""

    def __init__(self):
        self.op, self.a, self.b, self.c = [], [], [], []

    def emit(self, o, a=0, b=0, c=0.0):
        self.op.append(o), self.a.append(a), self.b.append(b), self.c.append(c)
        return len(self.op) - 1

    def const(self, v):
        return self.emit(0, 0, 0, v)

    def x(self, k):
        return self.emit(1, k)

    def p(self, k):
        return self.emit(2, k)

    def tape(self, cost, rows, n_ineq, n_eq, nx, np_):
        return make(self.op, self.a, self.b, self.c, cost, rows, n_ineq, n_eq, nx, np_)


def same(got, want):
    """Elementwise: the same float64 -- NaN for NaN (any payload), otherwise equal with the same sign (so -0 is not +0)."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    return (np.isnan(got) & np.isnan(want)) | ((got == want) & (np.signbit(got) == np.signbit(want)))


def ops_used(tp):
    """(opcodes a forward sweep of the live part executes, opcodes a reverse sweep differentiates) -- live: what the cost and the rows depend on."""
    live = np.zeros(len(tp.op), bool)
    live[tp.out_cost] = True
    live[np.asarray(tp.out_rows, int)] = True
    for i in range(len(tp.op) - 1, -1, -1):
        if live[i] and tp.op[i] >= 3:
            live[tp.a[i]] = True
            if int(tp.op[i]) in BINARY:
                live[tp.b[i]] = True
    ops = set(int(o) for o in np.asarray(tp.op)[live])
    return ops & ALL_OPS, ops & DIFF_OPS


def ref_phi(tp, x, p, lam, mu, rho):
    """InterpEval::phi in float64 numpy (oracle/tape_ref.py's sweeps, the row terms in the order the kernel adds them)."""
    with np.errstate(all="ignore"):
        v = tape_ref.forward(tp, x, p)
        ni, ne = int(tp.n_ineq), int(tp.n_eq)
        rows = v[np.asarray(tp.out_rows, int)] if ni + ne else np.zeros(0)
        val, cm, ms = v[tp.out_cost], 0.0, 0.0
        seeds = {int(tp.out_cost): 1.0}
        for i in range(ni):
            g, r = rows[i], int(tp.out_rows[i])
            s = np.fmax(0.0, lam[i] - rho * g)
            val = val + (s * s - lam[i] * lam[i]) / (2.0 * rho)
            cm = np.fmax(cm, np.fmax(0.0, -g))
            ms = np.fmax(ms, abs(np.fmin(g, lam[i] / rho)))
            seeds[r] = seeds.get(r, 0.0) + (-s)
        for j in range(ne):
            c, r = rows[ni + j], int(tp.out_rows[ni + j])
            val = val + (-mu[j] * c + 0.5 * rho * c * c)
            cm = np.fmax(cm, abs(c))
            ms = np.fmax(ms, abs(c))
            seeds[r] = seeds.get(r, 0.0) + (-mu[j] + rho * c)
        return {"merit": float(val), "f": float(v[tp.out_cost]), "rows": np.array(rows, float), "grad": tape_ref.reverse(tp, v, seeds), "cmax": float(cm),
                "meas": float(ms)}


# ---- (a) the opcode table -----------------------------------------------------------------------------------------------------------------
# One tape: opcode o = 3 .. 26 is row j = o - 3 twice -- as a >= row fed from the variables x[2j], x[2j + 1] (unary opcodes leave x[2j + 1] unread:
# its gradient is exactly 0) and as an = row fed from the parameters p[2j], p[2j + 1] (no adjoint).  The cost is the constant 0.
def opcode_table_tape(ops=tuple(range(3, 27))):
    """ops: the opcodes of the table (all of them; a part of the table for an evaluator whose work set must stay small), variables and rows renumbered."""
    t = B()
    ineq, eq = [], []
    for j, o in enumerate(ops):
        xa, xb = t.x(2 * j), t.x(2 * j + 1)
        ineq.append(t.emit(o, xa, xb if o in BINARY else 0))
    for j, o in enumerate(ops):
        pa, pb = t.p(2 * j), t.p(2 * j + 1)
        eq.append(t.emit(o, pa, pb if o in BINARY else 0))
    cost = t.const(0.0)
    return t.tape(cost, ineq + eq, len(ops), len(ops), 2 * len(ops), 2 * len(ops))


_PI = math.pi
GENERIC = [(0.7, -1.3), (-2.5, 0.4), (1.0, 1.0), (-3.0, -3.0), (2.0, 3.0), (3.0, 2.0), (-0.6, -0.2), (0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0),
           (1.0, 0.0), (1.0, -0.0), (-1.0, 0.0), (-1.0, -0.0), (0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0),
           (INF, 1.0), (-INF, 1.0), (1.0, INF), (1.0, -INF), (INF, INF), (INF, -INF), (-INF, INF), (-INF, -INF), (NAN, 1.0), (1.0, NAN), (NAN, NAN), (NAN, 0.0),
           (0.0, NAN), (INF, NAN), (TINY, 2.0), (2.0, TINY), (1.0, 1e-310), (TINY, 3.0), (MINN, MINN), (1e308, 1e308), (-1e308, 1e308), (1e-200, 1e-200),
           (0.25, 0.25), (0.5, -0.5)]
SPECIFIC = {
    6: [(1.0, 3.0), (1.0, TINY), (-1.0, TINY), (TINY, 3.0), (1e-310, 1e10), (1e308, 0.5), (7.0, -1e-310)],
    8: [(1e-300, 0), (_PI / 2, 0), (_PI, 0), (3 * _PI / 2, 0), (2 * _PI, 0), (-_PI, 0), (1e15, 0), (1e16, 0), (1e18, 0), (1e20, 0), (1e22, 0), (-1e22, 0), (TINY, 0), (1e308, 0)],
    10: [(1.0, 1.0), (1.0, -1.0), (-1.0, -1.0), (-1.0, 1.0), (1e-300, -1e300), (1e300, 1e-300), (TINY, -1.0), (-TINY, -1.0), (3.0, -4.0)],
    11: [(0.0, 0), (-0.0, 0), (MINN, 0), (TINY, 0), (1e-310, 0), (4.0, 0), (2.0, 0), (-1.0, 0), (1e308, 0)],
    13: [(1.0, 0), (-1.0, 0), (1.0 - 2.0 ** -53, 0), (-(1.0 - 2.0 ** -53), 0), (1.0 - 1e-8, 0), (-1.0 + 1e-8, 0), (0.5, 0), (1.0 + 2.0 ** -52, 0), (-2.0, 0), (TINY, 0), (1e-300, 0)],
    25: [(709.78, 0), (-709.78, 0), (745.2, 0), (-745.2, 0), (-745.0, 0), (-740.0, 0), (0.0, 0), (1.0, 0), (-1.0, 0), (1e-300, 0)],
    26: [(0.0, 0), (-0.0, 0), (MINN, 0), (TINY, 0), (1e-310, 0), (1.0, 0), (2.0, 0), (-1.0, 0), (1e308, 0), (1.0 + 2.0 ** -52, 0)],
}
SPECIFIC[9] = SPECIFIC[8]


def opcode_table_lines():
    """(X [n_lines][48], P [n_lines][48], operands[line][opcode] = (a, b)): line l gives opcode o entry l of its own list where that has one, else of the generic list."""
    n = len(GENERIC) + max(len(v) for v in SPECIFIC.values())
    X = np.zeros((n, 48))
    operands = []
    for ln in range(n):
        row = {}
        for o in range(3, 27):
            spec = SPECIFIC.get(o, [])
            a, b = GENERIC[ln] if ln < len(GENERIC) else (spec[ln - len(GENERIC)] if ln - len(GENERIC) < len(spec) else GENERIC[(ln + o) % 7])
            X[ln, 2 * (o - 3)], X[ln, 2 * (o - 3) + 1] = a, b
            row[o] = (float(a), float(b))
        operands.append(row)
    return X, X.copy(), operands


def single_op_tape(o):
    t = B()
    xa, xb = t.x(0), t.x(1)
    r = t.emit(o, xa, xb if o in BINARY else 0)
    return t.tape(r, [], 0, 0, 2, 0)


def ieee_value(o, a, b):
    """The float64 value of one instruction as numpy / the host C library computes it (IEEE 754, C Annex F); pinned by HAND below."""
    with np.errstate(all="ignore"):
        return float(tape_ref.forward(single_op_tape(o), np.array([a, b]), np.zeros(0))[2])


# Written down by hand from IEEE 754-2008 and C11 Annex F (F.10: atan2, asin, exp, log, sqrt, fmin / fmax, F.9.2 signed zeros), not computed:
# (opcode, a, b, expected).  "pi" entries are the correctly rounded multiples C requires for the exact cases of atan2.
HAND = [
    (3, 0.0, -0.0, 0.0), (3, -0.0, -0.0, -0.0), (3, INF, -INF, NAN), (3, INF, 1.0, INF), (3, NAN, 1.0, NAN),
    (4, 0.0, 0.0, 0.0), (4, -0.0, 0.0, -0.0), (4, INF, INF, NAN), (4, 1.0, INF, -INF),
    (5, -0.0, 1.0, -0.0), (5, 0.0, -1.0, -0.0), (5, -0.0, -1.0, 0.0), (5, INF, 0.0, NAN), (5, -INF, INF, -INF), (5, 1e308, 1e308, INF),
    (6, 1.0, 0.0, INF), (6, 1.0, -0.0, -INF), (6, -1.0, 0.0, -INF), (6, 0.0, 0.0, NAN), (6, INF, INF, NAN), (6, 1.0, INF, 0.0), (6, 1.0, -INF, -0.0), (6, 1.0, TINY, INF),
    (6, 0.0, -1.0, -0.0),
    (7, 0.0, 0, -0.0), (7, -0.0, 0, 0.0), (7, INF, 0, -INF), (7, NAN, 0, NAN),
    (8, 0.0, 0, 0.0), (8, -0.0, 0, -0.0), (8, INF, 0, NAN), (8, -INF, 0, NAN), (8, NAN, 0, NAN), (8, TINY, 0, TINY),
    (9, 0.0, 0, 1.0), (9, -0.0, 0, 1.0), (9, INF, 0, NAN), (9, NAN, 0, NAN), (9, TINY, 0, 1.0),
    (10, 0.0, 0.0, 0.0), (10, -0.0, 0.0, -0.0), (10, 0.0, -0.0, _PI), (10, -0.0, -0.0, -_PI), (10, 0.0, 1.0, 0.0), (10, -0.0, 1.0, -0.0), (10, 0.0, -1.0, _PI),
    (10, -0.0, -1.0, -_PI), (10, 1.0, 0.0, _PI / 2), (10, 1.0, -0.0, _PI / 2), (10, -1.0, 0.0, -_PI / 2), (10, 1.0, INF, 0.0), (10, 1.0, -INF, _PI), (10, INF, 1.0, _PI / 2),
    (10, -INF, 1.0, -_PI / 2), (10, INF, INF, _PI / 4), (10, INF, -INF, 3 * _PI / 4), (10, -INF, INF, -_PI / 4), (10, -INF, -INF, -3 * _PI / 4), (10, NAN, 1.0, NAN), (10, 1.0, NAN, NAN),
    (11, 0.0, 0, 0.0), (11, -0.0, 0, -0.0), (11, -1.0, 0, NAN), (11, INF, 0, INF), (11, -INF, 0, NAN), (11, NAN, 0, NAN), (11, 4.0, 0, 2.0),
    (12, -0.0, 0, 0.0), (12, -INF, 0, INF), (12, NAN, 0, NAN), (12, 1e308, 0, INF), (12, 1e-200, 0, 0.0),
    (13, 0.0, 0, 0.0), (13, -0.0, 0, -0.0), (13, 1.0, 0, _PI / 2), (13, -1.0, 0, -_PI / 2), (13, 1.0 + 2.0 ** -52, 0, NAN), (13, -2.0, 0, NAN), (13, INF, 0, NAN), (13, NAN, 0, NAN),
    (14, -0.0, 0, 0.0), (14, 0.0, 0, 0.0), (14, -INF, 0, INF), (14, NAN, 0, NAN), (14, -2.5, 0, 2.5),
    (15, 1.0, NAN, 1.0), (15, NAN, 1.0, 1.0), (15, NAN, NAN, NAN), (15, INF, 1.0, 1.0), (15, -INF, 1.0, -INF), (15, INF, NAN, INF), (15, 2.0, 3.0, 2.0),
    (16, 1.0, NAN, 1.0), (16, NAN, 1.0, 1.0), (16, NAN, NAN, NAN), (16, INF, 1.0, INF), (16, -INF, 1.0, 1.0), (16, 2.0, 3.0, 3.0),
    (17, 0.0, -0.0, 0.0), (17, NAN, 1.0, 0.0), (17, 1.0, NAN, 0.0), (17, -INF, INF, 1.0), (17, 1.0, 1.0, 0.0), (17, 2.0, 3.0, 1.0),
    (18, 0.0, -0.0, 1.0), (18, NAN, NAN, 0.0), (18, 1.0, 1.0, 1.0), (18, INF, INF, 1.0), (18, 3.0, 2.0, 0.0),
    (19, 0.0, -0.0, 1.0), (19, NAN, NAN, 0.0), (19, INF, INF, 1.0), (19, 1.0, 1.0, 1.0), (19, INF, -INF, 0.0),
    (20, 0.0, -0.0, 0.0), (20, NAN, NAN, 1.0), (20, NAN, 1.0, 1.0), (20, 1.0, 1.0, 0.0),
    (21, 0.0, 0, 1.0), (21, -0.0, 0, 1.0), (21, NAN, 0, 0.0), (21, INF, 0, 0.0), (21, 0.7, 0, 0.0),
    (22, NAN, 1.0, 1.0), (22, NAN, 0.0, 0.0), (22, -0.0, 1.0, 0.0), (22, INF, INF, 1.0), (22, 1.0, 1.0, 1.0),
    (23, NAN, 0.0, 1.0), (23, 0.0, -0.0, 0.0), (23, 0.0, NAN, 1.0), (23, 0.0, 1.0, 1.0),
    (24, NAN, 1.0, 1.0), (24, 0.0, NAN, 0.0), (24, -0.0, INF, 0.0), (24, 1.0, NAN, NAN), (24, 1.0, -0.0, -0.0), (24, INF, INF, INF), (24, 0.0, 1.0, 0.0), (24, 0.7, -1.3, -1.3),
    (25, 0.0, 0, 1.0), (25, -0.0, 0, 1.0), (25, INF, 0, INF), (25, -INF, 0, 0.0), (25, NAN, 0, NAN), (25, 709.78, 0, 1.7928227943945155e308), (25, 745.2, 0, INF), (25, -745.2, 0, 0.0),
    (25, -745.0, 0, TINY),
    (26, 0.0, 0, -INF), (26, -0.0, 0, -INF), (26, 1.0, 0, 0.0), (26, -1.0, 0, NAN), (26, INF, 0, INF), (26, -INF, 0, NAN), (26, NAN, 0, NAN),
]


# ---- (b) schedule shapes ------------------------------------------------------------------------------------------------------------------
def shape_tapes():
    """{name: tape}: small synthetic tapes that walk the branches of the wave evaluator's host-built schedule (csrc/oh_tape_wave.hip:oh_tape_wave_build);
    every one is also a plain tape for the other evaluators.  Values stay of order one by construction."""
    out = {}
    # fan-out of one register: c = cos(x0) consumed by k products c * x_j (inline consumer slots up to 3, the overflow list beyond)
    for k in (0, 1, 3, 4, 5, 64, 1000):
        t = B()
        nx = max(k, 1) + 1
        c = t.emit(9, t.x(0))
        terms = [t.emit(5, c, t.x(1 + j % (nx - 1))) for j in range(k)]
        acc = t.emit(12, t.x(1)) if k == 0 else terms[0]  # k = 0: c is read by nobody, it is a row only
        for r in terms[1:]:
            acc = t.emit(3, acc, t.emit(5, r, t.const(1.0 / k)))
        rows = [terms[len(terms) // 2]] if terms else [c]
        out[f"fanout{k}"] = t.tape(acc, rows, 0, 1, nx, 0)
    # one level of w instructions (sin of w variables), then a sum; w around the pass sizes of both block widths
    for w in (1, 63, 64, 65, 255, 256, 257, 1025):
        t = B()
        lv = [t.emit(8, t.x(j)) for j in range(w)]
        acc = lv[0]
        for r in lv[1:]:
            acc = t.emit(3, acc, r)
        out[f"width{w}"] = t.tape(acc, [lv[w // 2], lv[-1]], 1, 1, w, 0)
    # pass counts: d levels of one instruction each (d passes forward; reverse d + the variables' pass): d = 1 .. 8 covers every residue mod 4
    for d in (1, 2, 3, 4, 5, 6, 7, 8):
        t = B()
        r = t.emit(8, t.x(0))
        for _ in range(d - 1):
            r = t.emit(9, r)
        out[f"depth{d}"] = t.tape(r, [r], 1, 0, 1, 0)
    # a dependent chain of several thousand levels
    t = B()
    r, one = t.x(0), t.const(0.999)
    for i in range(3000):
        r = t.emit(8, t.emit(5, r, one)) if i % 2 else t.emit(3, r, t.x(1))
    out["chain3000"] = t.tape(r, [r], 0, 1, 2, 0)
    # nx around and beyond the block sizes; variables nobody reads (odd ones); variables loaded by many X instructions
    for nx in (1, 63, 64, 65, 257, 1000):
        t = B()
        acc = t.emit(12, t.x(0))
        for k in range(0, nx, 2):
            acc = t.emit(3, acc, t.emit(5, t.emit(8, t.x(k)), t.emit(9, t.x(k))))  # two loads of x_k: one register on the wave path
        for _ in range(5):
            acc = t.emit(3, acc, t.emit(5, t.x(0), t.x(nx - 1)))
        out[f"nx{nx}"] = t.tape(acc, [acc], 1, 0, nx, 0)
    # a few variables, each loaded by many X instructions with several consumers each (one register on the wave path)
    t = B()
    acc = t.emit(12, t.x(0))
    for i in range(12):
        xa, xb = t.x(i % 3), t.x((i + 1) % 3)
        acc = t.emit(3, acc, t.emit(5, t.emit(8, xa), t.emit(3, xa, xb)))
    out["many_loads"] = t.tape(acc, [acc], 0, 1, 3, 0)
    # X, P, CONST registers used directly as cost and as rows; the cost also a row; one register as several rows, >= and = mixed
    t = B()
    x0, x1, p0, c0 = t.x(0), t.x(1), t.p(0), t.const(0.75)
    s = t.emit(5, x0, x1)
    out["direct_x_cost"] = t.tape(x0, [x0, x1, p0, c0, s, s, x0, s, p0, c0], 6, 4, 2, 1)
    out["direct_p_cost"] = t.tape(p0, [s, x1], 1, 1, 2, 1)
    out["direct_const_cost"] = t.tape(c0, [s, s], 1, 1, 2, 1)
    out["cost_is_row"] = t.tape(s, [s, s, s], 2, 1, 2, 1)
    # both operands the same register, every binary opcode
    t = B()
    x0 = t.emit(3, t.x(0), t.const(0.25))
    rows = [t.emit(o, x0, x0) for o in sorted(BINARY)]
    acc = rows[0]
    for r in rows[1:]:
        acc = t.emit(3, acc, r)
    out["same_operand"] = t.tape(acc, rows, 7, 7, 1, 0)
    # row counts: none, only >=, only =, and 300 rows (more rows than threads)
    for name, ni, ne in (("rows_none", 0, 0), ("rows_ineq", 3, 0), ("rows_eq", 0, 3), ("rows300", 170, 130)):
        t = B()
        xs = [t.x(k) for k in range(4)]
        rows = [t.emit(4, t.emit(8, t.emit(5, xs[i % 4], t.const(0.1 + 0.01 * i))), t.const(0.3 - 0.002 * i)) for i in range(ni + ne)]
        cost = t.emit(3, t.emit(12, xs[0]), t.emit(5, xs[1], t.emit(9, xs[2])))
        cost = t.emit(3, cost, t.emit(25, xs[3]))
        out[name] = t.tape(cost, rows, ni, ne, 4, 0)
    # dead instructions, some with non-finite values (log of a negative number, division by zero): no evaluator may let them reach the result
    t = B()
    x0, x1 = t.x(0), t.x(1)
    dead = t.emit(26, t.emit(7, t.emit(12, x0)))
    t.emit(6, x1, t.emit(4, x0, x0))
    t.emit(3, dead, x1)
    live = t.emit(5, t.emit(8, x0), x1)
    t.emit(11, t.emit(4, t.const(-1.0), t.emit(12, x1)))
    out["dead"] = t.tape(live, [live], 0, 1, 2, 0)
    # one level that holds every rare opcode (and the common ones) several times over: arrange() deals different bodies to the wavefronts of a block
    t = B()
    xs = [t.emit(3, t.emit(5, t.x(k), t.const(0.2)), t.const(0.3 + 0.05 * k)) for k in range(8)]  # values in (0, 1): inside every domain
    lvl = []
    for rep in range(3):
        for o in range(3, 27):
            lvl.append(t.emit(o, xs[(o + rep) % 8], xs[(o + 3 * rep + 1) % 8] if o in BINARY else 0))
    acc = lvl[0]
    for r in lvl[1:]:
        acc = t.emit(3, acc, t.emit(5, r, t.const(0.125)))
    out["mixed_level"] = t.tape(acc, [lvl[3], lvl[7], lvl[10], lvl[21], lvl[22], lvl[23]], 3, 3, 8, 0)
    return out


def shape_point(tp, seed):
    rng = np.random.default_rng(seed)
    ni, ne = int(tp.n_ineq), int(tp.n_eq)
    return (rng.uniform(0.2, 0.9, tp.nx), rng.uniform(0.2, 0.9, max(tp.np_, 0)), rng.uniform(0.0, 2.0, ni), rng.uniform(-1.0, 1.0, ne), float(10.0 ** rng.uniform(-1, 2)))


def huge_fanout_tape(k=66000):
    """One register with more than 65 535 consumers: the wave schedule's 16-bit consumer count cannot hold it and the builder declines."""
    t = B()
    c = t.emit(9, t.x(0))
    x1 = t.x(1)
    acc = t.emit(5, c, x1)
    for j in range(k | 1):  # + c - c + c ...: the value stays of order one (66 000 additions of the same number would be the sample's rounding, not the evaluator's)
        acc = t.emit(4 if j % 2 else 3, acc, c)
    return t.tape(acc, [acc], 0, 1, 2, 0)


# ---- (c) random tapes ---------------------------------------------------------------------------------------------------------------------
def random_tape(seed, n_ins, nx, n_ineq, n_eq, np_=3):
    """A seeded composition of every differentiable opcode (the piecewise-constant ones ride along as IFZ conditions), domain-safe by construction:
    every value is kept in [-2, 2] (a register that leaves [-1.5, 1.5] is brought back through sin), sqrt / log / divisors see 1.5 + v >= 0.5 only after
    such a fold, asin sees v / 2.  Operands are drawn from the recent registers and the variables, so gradients stay of order one and every variable
    is read.  Returns (tape, x, p, lam, mu, rho)."""
    rng = np.random.default_rng(seed)
    t = B()
    x = rng.uniform(-1.0, 1.0, nx)
    p = rng.uniform(-1.0, 1.0, np_)
    vals = []  # float64 value of every register at (x, p): steers the construction only

    def emit(o, a=0, b=0, c=0.0):
        r = t.emit(o, a, b, c)
        with np.errstate(all="ignore"):
            if o == 0:
                v = c
            elif o == 1:
                v = x[a]
            elif o == 2:
                v = p[a]
            else:
                tp1 = make([0, 0, o], [0, 0, 0], [0, 0, 1], [vals[a], vals[b] if o in BINARY else 0.0, 0.0], 2, [], 0, 0, 1, 0)
                v = float(tape_ref.forward(tp1, np.zeros(1), np.zeros(0))[2])
        vals.append(v)
        return r

    pool = [emit(1, k) for k in range(nx)] + [emit(2, k) for k in range(np_)]
    half, c15 = emit(0, 0, 0, 0.5), emit(0, 0, 0, 1.5)
    smooth_unary = [7, 8, 9, 12, 14, 25]
    n_pool0 = len(pool)

    def bounded(r):
        return r if abs(vals[r]) <= 1.5 else emit(8, r)

    def pick():
        if rng.random() < 0.25:
            return pool[int(rng.integers(0, n_pool0))]
        return pool[int(rng.integers(max(0, len(pool) - 40), len(pool)))]

    while len(t.op) < n_ins:
        kind = int(rng.integers(0, 12))
        a, b = bounded(pick()), bounded(pick())
        if kind <= 2:
            r = emit(int(rng.choice([3, 4, 5])), a, b)
        elif kind == 3:
            r = emit(int(rng.choice(smooth_unary)), a)
        elif kind == 4:
            r = emit(6, a, emit(3, c15, emit(5, half, b)))  # divisor in [0.75, 2.25]
        elif kind == 5:
            r = emit(int(rng.choice([11, 26])), emit(3, c15, emit(5, half, a)))
        elif kind == 6:
            r = emit(13, emit(5, half, a))
        elif kind == 7:
            r = emit(10, a, emit(3, c15, emit(5, half, b)))
        elif kind == 8:
            r = emit(int(rng.choice([15, 16])), a, b)
        elif kind == 9:
            cond = emit(int(rng.choice([17, 18, 19, 20])), a, b)
            if rng.random() < 0.5:
                cond = emit(int(rng.choice([21, 22, 23])), cond, emit(17, b, a))
            r = emit(3, emit(24, cond, a), emit(24, emit(21, cond), b))
        else:
            r = emit(3, a, emit(5, half, b))
        pool.append(bounded(r))
    # every variable reaches the cost: a sum of squares of the variables' sines on top of what was drawn, and the last registers
    acc = bounded(pool[-1])
    for k in range(nx):
        acc = emit(3, acc, emit(5, emit(0, 0, 0, 1.0 / nx), emit(12, emit(8, pool[k]))))
    cand = [r for r in pool[n_pool0:] if t.op[r] not in (0, 2)]
    rows = [cand[int(i)] for i in rng.integers(len(cand) // 2, len(cand), n_ineq + n_eq)]
    tp = t.tape(acc, rows, n_ineq, n_eq, nx, np_)
    rho = float(10.0 ** rng.uniform(-3, 8))
    g = np.array([vals[r] for r in rows[:n_ineq]])
    side = rng.random(n_ineq) < 0.5  # rows on either side of lam - rho g = 0
    lam = np.where(side, np.maximum(0.0, rho * g) + rng.uniform(0.1, 1.0, n_ineq) * max(rho, 1.0), np.maximum(0.0, rho * g - rng.uniform(0.1, 1.0, n_ineq) * max(rho, 1.0)))
    mu = rng.uniform(-2.0, 2.0, n_eq) * max(1.0, rho)
    return tp, x, p, lam, mu, rho


RANDOM_SPECS = [  # (seed, instructions, nx, n_ineq, n_eq): 10 instructions to a few thousand, one variable to a few hundred
    (1, 10, 1, 1, 1), (2, 60, 3, 2, 1), (3, 250, 12, 4, 3), (4, 600, 300, 5, 5), (5, 1500, 60, 20, 10), (6, 3000, 40, 30, 30),
]


# ---- references of the opcode table -------------------------------------------------------------------------------------------------------
def row_tape(o):
    """Opcode o on two variables as the one >= row of a tape whose cost is the constant 0: the opcode table's row, alone."""
    t = B()
    xa, xb = t.x(0), t.x(1)
    r = t.emit(o, xa, xb if o in BINARY else 0)
    return t.tape(t.const(0.0), [r], 1, 0, 2, 0)


TABLE_RHO = 2.0


def table_multipliers(operands, zero_seed=False):
    """lam [n_lines][24] with lam - rho g = 1 on every row whose value is finite (seed -1: of order one); zero_seed: lam = 0, so that rows with
    g >= 0 (and NaN rows: fmax(0, NaN) = 0) get a seed that is exactly zero."""
    lam = np.zeros((len(operands), 24))
    if not zero_seed:
        for ln, row in enumerate(operands):
            for o in range(3, 27):
                g = ieee_value(o, *row[o])
                lam[ln, o - 3] = 1.0 + TABLE_RHO * g if np.isfinite(g) and abs(g) < 1e300 else 1.0
    return lam


def table_reference(operands, lam):
    """Per line and opcode: {"ieee": float64 value by IEEE / Annex F, "mp": mpf value or None where mpmath has none, "grad_ref": float64 oracle gradient (2,),
    "grad_mp": (2,) or None where the merit is not finite and smooth in a neighbourhood}."""
    from oracle import tape_mp

    out = []
    for ln, row in enumerate(operands):
        line = {}
        for o in range(3, 27):
            a, b = row[o]
            tp = row_tape(o)
            e = {"ieee": ieee_value(o, a, b), "mp": None, "grad_mp": None}
            xx, ll = np.array([a, b]), np.array([lam[ln, o - 3]])
            e["grad_ref"] = ref_phi(tp, xx, np.zeros(0), ll, np.zeros(0), TABLE_RHO)["grad"]
            if o not in BINARY:
                xx = np.array([a, 0.0])  # (the operand a unary opcode does not read may be anything)
            try:
                e["mp"] = tape_mp.forward_mp(tp, xx, np.zeros(0))[2]
                if e["mp"] is None:
                    raise tape_mp.NonFinite
                # The gradient is compared with mp where the row's value is finite and every operand is 0 or within 1e-150 .. 1e150: outside, the squares the
                # derivative rules of DIV and ATAN2 form (b b, a a + b b) over- or underflow in float64, the seed lam - rho g with them, and what the
                # evaluators must then agree on is the float64 arithmetic of the rule (grad_ref), not the real derivative.
                if np.isfinite(e["ieee"]) and all(t == 0.0 or 1e-150 <= abs(t) <= 1e150 for t in xx):
                    e["grad_mp"] = tape_mp.phi_mp(tp, xx, np.zeros(0), ll, np.zeros(0), TABLE_RHO)["grad"]
            except tape_mp.NonFinite:
                pass
            line[o] = e
        out.append(line)
    return out
