"""References of oh_tape_hvp (optas_amd/csrc/oh_tape.hip:k_tape_hvp), shared by tests/test_tape_hvp_cpu.py and tests/test_gpu_tape_hvp.py.

(a) hvp_port / hessian_port: the kernel's forward-over-reverse sweep in float64 numpy, rule for rule (same selections at the kinks, dead instructions
    left out of the reverse sweep, every adjoint and tangent multiplied through).

(b) hvp_mp / hessian_mp: the independent reference.  NOT a derivative rule anywhere: second differences of the 60-digit interpreter oracle/tape_mp.py
    with the selections of the base point held,

        (H v)_k = [L(x + h (v + e_k)) - L(x + h (v - e_k)) - L(x - h (v - e_k)) + L(x - h (v + e_k))] / (4 h^2),      h = 1e-15,

    L the seeded combination of tape_mp._run's registers, at tape_mp._dps working precision (>= 60 digits).  Truncation ~ h^2 = 1e-30 of the fourth
    derivative, rounding ~ 1e-60 / h^2 = 1e-30 of L: both twelve orders below the tolerances they serve.  The dense Hessian is the same formula with
    v = e_j for j <= k (it is symmetric by construction; the device's own asymmetry is graded separately), each perturbed run recomputing only the
    registers that depend on x_j or x_k (tape_mp._run's `base`)."""
import mpmath
import numpy as np

from oracle import tape_mp, tape_ref

H_STEP = "1e-15"
DEVICE_TOL = 1e-12  # GRAD_TOL of tests/test_gpu_tape_evaluators.py for composite tapes: |got - ref|_inf <= 1e-12 max(1, |ref|_inf)
PORT_TOL = DEVICE_TOL / 4  # the port against mp: a quarter, so that a GPU failure is the device's

_BINARY = tape_ref._BINARY


def within(got, ref, tol):
    """(ok, error relative to max(1, |ref|_inf)) of one instance's vector or matrix."""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    scale = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
    err = float(np.abs(got - ref).max()) / scale if ref.size else 0.0
    return bool(np.isfinite(got).all()) and err <= tol, err


def seed_vector(tp, seed=5):
    """1 on the cost, U(-2, 2) on the rows from a fixed generator."""
    rng = np.random.default_rng(seed)
    return np.concatenate([[1.0], rng.uniform(-2.0, 2.0, int(tp.n_ineq) + int(tp.n_eq))])


# ---- (a) float64 port -----------------------------------------------------------------------------------------------------------------------
def _live(tp):
    live = np.zeros(len(tp.op), bool)
    live[int(tp.out_cost)] = True
    live[np.asarray(tp.out_rows, int)] = True
    for i in range(len(tp.op) - 1, -1, -1):
        if live[i] and tp.op[i] >= 3:
            live[tp.a[i]] = True
            if int(tp.op[i]) in _BINARY:
                live[tp.b[i]] = True
    return live


def hvp_port(tp, x, p, seeds, v):
    """(H v (nx,), gradient (nx,)) of sum seeds * (cost, rows) at x, p along v: k_tape_hvp for one unit."""
    f8 = np.float64
    L, nx = len(tp.op), int(tp.nx)
    ops, aa, bb = [int(t) for t in tp.op], [int(t) for t in tp.a], [int(t) for t in tp.b]
    x, p, v = np.asarray(x, f8), np.asarray(p, f8), np.asarray(v, f8)
    val, dval = np.zeros(L), np.zeros(L)
    sign = lambda t: 1.0 if t > 0.0 else (-1.0 if t < 0.0 else 0.0)
    with np.errstate(all="ignore"):
        for i in range(L):
            o, a, b = ops[i], aa[i], bb[i]
            if o == 0:
                r, t = f8(tp.c[i]), f8(0.0)
            elif o == 1:
                r, t = x[a], v[a]
            elif o == 2:
                r, t = p[a], f8(0.0)
            else:
                va, ta = val[a], dval[a]
                vb, tb = (val[b], dval[b]) if o in _BINARY else (f8(0.0), f8(0.0))
                if o == 3:
                    r, t = va + vb, ta + tb
                elif o == 4:
                    r, t = va - vb, ta - tb
                elif o == 5:
                    r, t = va * vb, ta * vb + va * tb
                elif o == 6:
                    r = va / vb
                    t = (ta - r * tb) / vb
                elif o == 7:
                    r, t = -va, -ta
                elif o == 8:
                    r, t = np.sin(va), np.cos(va) * ta
                elif o == 9:
                    r, t = np.cos(va), -(np.sin(va) * ta)
                elif o == 10:
                    r, t = np.arctan2(va, vb), (vb * ta - va * tb) / (va * va + vb * vb)
                elif o == 11:
                    r = np.sqrt(va)
                    t = 0.5 / r * ta
                elif o == 12:
                    r, t = va * va, 2.0 * va * ta
                elif o == 13:
                    r, t = np.arcsin(va), ta / np.sqrt((1.0 - va) * (1.0 + va))
                elif o == 14:
                    r, t = abs(va), sign(va) * ta
                elif o == 15:
                    r, t = np.fmin(va, vb), (ta if va <= vb else tb)
                elif o == 16:
                    r, t = np.fmax(va, vb), (ta if va >= vb else tb)
                elif 17 <= o <= 23:
                    c = (va < vb if o == 17 else va <= vb if o == 18 else va == vb if o == 19 else va != vb if o == 20 else va == 0.0 if o == 21
                         else (va != 0.0 and vb != 0.0) if o == 22 else (va != 0.0 or vb != 0.0))
                    r, t = f8(1.0 if c else 0.0), f8(0.0)
                elif o == 24:
                    r, t = (vb, tb) if va != 0.0 else (f8(0.0), f8(0.0))
                elif o == 25:
                    r = np.exp(va)
                    t = r * ta
                else:
                    r, t = np.log(va), ta / va
            val[i], dval[i] = r, t
        adj, dadj = np.zeros(L), np.zeros(L)
        seeds = np.asarray(seeds, f8)
        adj[int(tp.out_cost)] += seeds[0]
        for i, r in enumerate(np.asarray(tp.out_rows, int)):
            adj[r] += seeds[1 + i]
        g, hv = np.zeros(nx), np.zeros(nx)
        live = _live(tp)
        for i in range(L - 1, -1, -1):
            if not live[i]:
                continue
            w, dw = adj[i], dadj[i]
            o, a, b = ops[i], aa[i], bb[i]
            if o in (0, 2) or 17 <= o <= 23:
                continue
            if o == 1:
                g[a] += w
                hv[a] += dw
                continue
            va, ta = val[a], dval[a]
            vb, tb = (val[b], dval[b]) if o in _BINARY else (f8(0.0), f8(0.0))
            if o == 3:
                adj[a] += w; adj[b] += w; dadj[a] += dw; dadj[b] += dw
            elif o == 4:
                adj[a] += w; adj[b] -= w; dadj[a] += dw; dadj[b] -= dw
            elif o == 5:
                adj[a] += w * vb; adj[b] += w * va
                dadj[a] += dw * vb + w * tb; dadj[b] += dw * va + w * ta
            elif o == 6:
                adj[a] += w / vb; adj[b] -= w * va / (vb * vb)
                dadj[a] += (dw - w * tb / vb) / vb
                dadj[b] -= (dw * va + w * ta - 2.0 * (w * va) * tb / vb) / (vb * vb)
            elif o == 7:
                adj[a] -= w; dadj[a] -= dw
            elif o == 8:
                c = np.cos(va)
                adj[a] += w * c
                dadj[a] += dw * c - w * np.sin(va) * ta
            elif o == 9:
                s = np.sin(va)
                adj[a] -= w * s
                dadj[a] -= dw * s + w * np.cos(va) * ta
            elif o == 10:
                d = va * va + vb * vb
                adj[a] += w * vb / d; adj[b] -= w * va / d
                dd = 2.0 * (va * ta + vb * tb)
                dadj[a] += (dw * vb + w * (tb - vb * dd / d)) / d
                dadj[b] -= (dw * va + w * (ta - va * dd / d)) / d
            elif o == 11:
                r = val[i]
                q = 0.5 / r
                adj[a] += w * 0.5 / r
                dadj[a] += dw * q - w * (q * dval[i] / r)
            elif o == 12:
                adj[a] += w * 2.0 * va
                dadj[a] += dw * 2.0 * va + w * 2.0 * ta
            elif o == 13:
                s = (1.0 - va) * (1.0 + va)
                r = np.sqrt(s)
                adj[a] += w / r
                dadj[a] += dw / r + w * (va * ta / (s * r))
            elif o == 14:
                adj[a] += w * sign(va); dadj[a] += dw * sign(va)
            elif o == 15 or o == 16:
                k = a if (va <= vb if o == 15 else va >= vb) else b
                adj[k] += w; dadj[k] += dw
            elif o == 24:
                if va != 0.0:
                    adj[b] += w; dadj[b] += dw
            elif o == 25:
                adj[a] += w * val[i]
                dadj[a] += dw * val[i] + w * dval[i]
            elif o == 26:
                adj[a] += w / va
                dadj[a] += (dw - w * ta / va) / va
    return hv, g


def hessian_port(tp, x, p, seeds):
    nx = int(tp.nx)
    return np.stack([hvp_port(tp, x, p, seeds, np.eye(nx)[d])[0] for d in range(nx)])


# ---- (b) second differences of the 60-digit interpreter ---------------------------------------------------------------------------------------
class _Vars:
    """A set of variable indices that compares equal to each of its members: tape_mp._run's `var` for a run that differs from `base` in several variables."""

    def __init__(self, ks):
        self.ks = frozenset(int(k) for k in ks)

    def __eq__(self, k):
        return k in self.ks

    __hash__ = None


class _Mp:
    """The seeded combination L at mp points around (x, p), selections of the base point held."""

    def __init__(self, tp, x, p, seeds):
        mp = mpmath.mp
        self.tp = tp
        self.xs, self.ps = [tape_mp._exact(t) for t in x], [tape_mp._exact(t) for t in p]
        self.w = [tape_mp._exact(t) for t in seeds]
        self.regs = [int(tp.out_cost)] + [int(r) for r in tp.out_rows]
        self.h = mp.mpf(H_STEP)
        self.base, self.sel = tape_mp._run(tp, self.xs, self.ps, None)
        self.used = sorted(set(int(tp.a[i]) for i in range(len(tp.op)) if int(tp.op[i]) == 1))
        self.L0 = self.combine(self.base)

    def combine(self, v):
        s = mpmath.mp.mpf(0)
        for w, r in zip(self.w, self.regs):
            if v[r] is None:
                raise tape_mp.NonFinite("the cost or a row has no finite value at this point")
            s += w * v[r]
        return s

    def at(self, step, changed=None):
        """L(x + h step); step: {k: mpf multiple of h}.  changed: only these variables differ from the base point (None: any may)."""
        if not step:
            return self.L0
        xs = list(self.xs)
        for k, c in step.items():
            xs[k] = xs[k] + self.h * c
        if changed is None:
            return self.combine(tape_mp._run(self.tp, xs, self.ps, self.sel)[0])
        return self.combine(tape_mp._run(self.tp, xs, self.ps, self.sel, self.base, _Vars(changed))[0])


def _dps(tp, x, p, seeds, v=()):
    return tape_mp._dps(x, p, tp.c, seeds, v)


def hvp_mp(tp, x, p, seeds, v):
    """H v (nx,) float64, rounded at the end."""
    with mpmath.workdps(_dps(tp, x, p, seeds, v)):
        m = _Mp(tp, x, p, seeds)
        vs = {k: tape_mp._exact(t) for k, t in enumerate(v) if float(t) != 0.0}
        out = np.zeros(int(tp.nx))

        def shifted(sign_v, sign_e, k):
            st = {j: sign_v * c for j, c in vs.items()}
            st[k] = st.get(k, 0) + sign_e
            return m.at({j: c for j, c in st.items() if c != 0})

        for k in m.used:  # a variable no X instruction loads has a zero row
            d = shifted(1, 1, k) - shifted(1, -1, k) - shifted(-1, 1, k) + shifted(-1, -1, k)  # x + h (v + e_k), x + h (v - e_k), x - h (v - e_k), x - h (v + e_k)
            out[k] = float(d / (4 * m.h * m.h))
        return out


def hessian_mp(tp, x, p, seeds):
    """The dense Hessian (nx, nx) float64: the formula above with v = e_j, j <= k, mirrored."""
    nx = int(tp.nx)
    with mpmath.workdps(_dps(tp, x, p, seeds)):
        m = _Mp(tp, x, p, seeds)
        H = np.zeros((nx, nx))
        one = {}  # L(x +- 2 h e_j)
        for j in m.used:
            one[j] = (m.at({j: 2}, (j,)), m.at({j: -2}, (j,)))
            H[j, j] = float((one[j][0] - 2 * m.L0 + one[j][1]) / (4 * m.h * m.h))  # v = e_k = e_j: x + 2 h e_j, x, x, x - 2 h e_j
        for a, j in enumerate(m.used):
            for k in m.used[a + 1:]:
                d = m.at({j: 1, k: 1}, (j, k)) - m.at({j: 1, k: -1}, (j, k)) - m.at({j: -1, k: 1}, (j, k)) + m.at({j: -1, k: -1}, (j, k))
                H[j, k] = H[k, j] = float(d / (4 * m.h * m.h))
        return H


# ---- the cases both test files grade ------------------------------------------------------------------------------------------------------------
RANDOM_SPECS = [(1, 10, 1, 1, 1), (2, 60, 3, 2, 1), (3, 250, 12, 4, 3), (7, 400, 6, 3, 2), (8, 800, 5, 2, 2)]  # the last covers all 17 differentiable opcodes
SHAPE_NAMES = ["many_loads", "dead", "same_operand", "direct_x_cost", "cost_is_row", "rows_none", "rows_ineq", "rows_eq", "mixed_level", "fanout5", "width65", "nx65",
               "depth8"]
BIG_SPEC = (4, 600, 300, 5, 5)  # graded against the port only: its mp reference takes 20 s per direction
_cache = {}


def composite_cases():
    """[(name, tape, x, p, seeds, v)]: the random and the shape tapes with their points, seeds and one random direction."""
    if "composite" not in _cache:
        import tape_cases

        out = []
        for spec in RANDOM_SPECS:
            tp, x, p = tape_cases.random_tape(*spec)[:3]
            out.append(("random%d" % spec[0], tp, x, p))
        shapes = tape_cases.shape_tapes()
        for name in SHAPE_NAMES:
            tp = shapes[name]
            x, p = tape_cases.shape_point(tp, 11)[:2]
            out.append((name, tp, x, p))
        rng = np.random.default_rng(17)
        _cache["composite"] = [(n, tp, x, p, seed_vector(tp), rng.uniform(-1.0, 1.0, int(tp.nx))) for n, tp, x, p in out]
    return _cache["composite"]


def composite_reference(name):
    """{"hv": H v along the case's direction, "H": dense Hessian} by mp, computed once per process."""
    key = ("ref", name)
    if key not in _cache:
        _, tp, x, p, seeds, v = next(c for c in composite_cases() if c[0] == name)
        _cache[key] = {"hv": hvp_mp(tp, x, p, seeds, v), "H": hessian_mp(tp, x, p, seeds)}
    return _cache[key]


def single_op_lines(o):
    """The points of opcode o alone on two variables: GENERIC[0:7] and (0.3, 0.8), without those outside the domain (a <= 0 for SQRT and LOG, |a| >= 1
    for ASIN) and the ties of FMIN and FMAX."""
    import tape_cases

    pts = list(tape_cases.GENERIC[0:7]) + [(0.3, 0.8)]
    keep = []
    for a, b in pts:
        if o in (11, 26) and a <= 0.0:
            continue
        if o == 13 and abs(a) >= 1.0:
            continue
        if o in (15, 16) and a == b:
            continue
        keep.append((a, b))
    return np.array(keep)


def single_op_reference(o):
    """[n_lines][2][2] dense Hessians of opcode o alone by mp."""
    key = ("single", o)
    if key not in _cache:
        import tape_cases

        tp = tape_cases.single_op_tape(o)
        _cache[key] = np.stack([hessian_mp(tp, x, np.zeros(0), [1.0]) for x in single_op_lines(o)])
    return _cache[key]
