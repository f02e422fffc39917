"""References of the tape family's truncated Newton-CG inner solver (optas_amd/csrc/oh_tape_newton.h, InterpEval::hess_vec of oh_tape.hip), shared by
tests/test_tape_newton_cpu.py and tests/test_gpu_tape_newton.py.

(a) merit_hvp_port: the generalised Hessian of the augmented-Lagrangian merit times v in float64 numpy -- oracle/tape_ref.py's forward sweep, then the
    tangent sweep, the seeds with their tangents and the reverse sweep with dadj beside adj, rule for rule as the device runs them (the rules are
    tests/tape_hvp_ref.py:hvp_port's; what is new is the seed tangent rho * dval[row] of an active inequality row and of every equality row).

(b) solve_tape_newton: the state machine of oh_tape_newton.h statement for statement (outer loop and Armijo test are oracle/tape_ref.py:solve_tape_al's).

(c) merit_hessian_mp: the independent reference.  tape_hvp_ref.hessian_mp (second differences of the 60-digit interpreter) of the combination
    cost + sum seed_r row_r with the AL seeds -(lam - rho g) / 0 / (-mu + rho c) decided in mp, plus rho sum_active grad row grad row^T with the rows'
    gradients by central differences of oracle/tape_mp.py's registers (h = 1e-25, selections of the base point held).  No derivative rule is shared with (a)."""
import mpmath
import numpy as np

import tape_hvp_ref as R
from oracle import tape_mp, tape_ref

_BINARY = tape_ref._BINARY


# ---- (a) float64 port of InterpEval::phi + hess_vec -------------------------------------------------------------------------------------------------
def _reverse_adj(tp, v, seeds, live):
    """oracle/tape_ref.py:reverse keeping the register adjoints: (gradient, adj) with adj[i] the final adjoint of register i."""
    L = len(tp.op)
    adj = np.zeros(L)
    for r, w in seeds:
        adj[r] += w
    g = np.zeros(int(tp.nx))
    ops, aa, bb = tp.op, tp.a, tp.b
    for i in range(L - 1, -1, -1):
        if not live[i]:
            continue
        w = adj[i]
        o, a, b = int(ops[i]), int(aa[i]), int(bb[i])
        if o == 1:
            g[a] += w
        elif o == 3:
            adj[a] += w; adj[b] += w
        elif o == 4:
            adj[a] += w; adj[b] -= w
        elif o == 5:
            adj[a] += w * v[b]; adj[b] += w * v[a]
        elif o == 6:
            adj[a] += w / v[b]; adj[b] -= w * v[a] / (v[b] * v[b])
        elif o == 7:
            adj[a] -= w
        elif o == 8:
            adj[a] += w * np.cos(v[a])
        elif o == 9:
            adj[a] -= w * np.sin(v[a])
        elif o == 10:
            d = v[a] * v[a] + v[b] * v[b]
            adj[a] += w * v[b] / d; adj[b] -= w * v[a] / d
        elif o == 11:
            adj[a] += w * 0.5 / v[i]
        elif o == 12:
            adj[a] += w * 2.0 * v[a]
        elif o == 13:
            adj[a] += w / np.sqrt((1.0 - v[a]) * (1.0 + v[a]))
        elif o == 14:
            adj[a] += w * (1.0 if v[a] > 0.0 else (-1.0 if v[a] < 0.0 else 0.0))
        elif o == 15:
            adj[a if v[a] <= v[b] else b] += w
        elif o == 16:
            adj[a if v[a] >= v[b] else b] += w
        elif o == 24:
            if v[a] != 0.0:
                adj[b] += w
        elif o == 25:
            adj[a] += w * v[i]
        elif o == 26:
            adj[a] += w / v[a]
    return g, adj


class MeritEval:
    """InterpEval of oh_tape.hip for one instance: phi(x) leaves val and adj behind, hess_vec(v) reads them (the solver's invariant: every hess_vec follows a
    phi at the same point with the same multipliers and penalty)."""

    def __init__(self, tp, p):
        self.tp, self.p = tp, np.asarray(p, float)
        self.live = R._live(tp)
        self.ni, self.ne = int(tp.n_ineq), int(tp.n_eq)
        self.rows = [int(r) for r in tp.out_rows]
        self.ops, self.aa, self.bb = [int(t) for t in tp.op], [int(t) for t in tp.a], [int(t) for t in tp.b]

    def phi(self, x, lam, mu, rho):
        tp, ni, ne = self.tp, self.ni, self.ne
        with np.errstate(all="ignore"):
            v = tape_ref.forward(tp, x, self.p)
            f = v[int(tp.out_cost)]
            val, cm, ms = f, 0.0, 0.0
            seeds = [(int(tp.out_cost), 1.0)]
            rowv = np.zeros(ni + ne)
            for i in range(ni):
                g = v[self.rows[i]]
                s = np.fmax(0.0, lam[i] - rho * g)
                val = val + (s * s - lam[i] * lam[i]) / (2.0 * rho)
                cm = np.fmax(cm, np.fmax(0.0, -g))
                ms = np.fmax(ms, abs(np.fmin(g, lam[i] / rho)))
                seeds.append((self.rows[i], -s))
                rowv[i] = g
            for j in range(ne):
                c = v[self.rows[ni + j]]
                val = val + (-mu[j] * c + 0.5 * rho * c * c)
                cm = np.fmax(cm, abs(c))
                ms = np.fmax(ms, abs(c))
                seeds.append((self.rows[ni + j], -mu[j] + rho * c))
                rowv[ni + j] = c
            grad, adj = _reverse_adj(tp, v, seeds, self.live)
        self.val, self.adj, self.rowv, self.lam, self.rho = v, adj, rowv, np.array(lam, float), float(rho)
        return float(val), grad, float(f), float(cm), float(ms)

    def hess_vec(self, vdir):
        """One tangent forward sweep and one dadj reverse sweep on the val / adj the last phi left."""
        f8 = np.float64
        tp, val, adj, rho = self.tp, self.val, self.adj, self.rho
        L = len(self.ops)
        dval, dadj = np.zeros(L), np.zeros(L)
        sign = lambda t: 1.0 if t > 0.0 else (-1.0 if t < 0.0 else 0.0)
        vdir = np.asarray(vdir, f8)
        out = np.zeros(int(tp.nx))
        with np.errstate(all="ignore"):
            for i in range(L):
                if not self.live[i]:
                    continue
                o, a, b = self.ops[i], self.aa[i], self.bb[i]
                if o == 1:
                    t = vdir[a]
                elif o < 3 or 17 <= o <= 23:
                    t = f8(0.0)
                else:
                    va, ta = val[a], dval[a]
                    vb, tb = (val[b], dval[b]) if o in _BINARY else (f8(0.0), f8(0.0))
                    if o == 3:
                        t = ta + tb
                    elif o == 4:
                        t = ta - tb
                    elif o == 5:
                        t = ta * vb + va * tb
                    elif o == 6:
                        t = (ta - val[i] * tb) / vb
                    elif o == 7:
                        t = -ta
                    elif o == 8:
                        t = np.cos(va) * ta
                    elif o == 9:
                        t = -(np.sin(va) * ta)
                    elif o == 10:
                        t = (vb * ta - va * tb) / (va * va + vb * vb)
                    elif o == 11:
                        t = 0.5 / val[i] * ta
                    elif o == 12:
                        t = 2.0 * va * ta
                    elif o == 13:
                        t = ta / np.sqrt((1.0 - va) * (1.0 + va))
                    elif o == 14:
                        t = sign(va) * ta
                    elif o == 15:
                        t = ta if va <= vb else tb
                    elif o == 16:
                        t = ta if va >= vb else tb
                    elif o == 24:
                        t = tb if va != 0.0 else f8(0.0)
                    elif o == 25:
                        t = val[i] * ta
                    else:
                        t = ta / va
                dval[i] = t
            # seed tangents: an active inequality row (lam - rho g > 0, a tie is inactive) and every equality row: rho * dval[row]
            for i in range(self.ni):
                if np.fmax(0.0, self.lam[i] - rho * self.rowv[i]) > 0.0:
                    dadj[self.rows[i]] += rho * dval[self.rows[i]]
            for j in range(self.ne):
                dadj[self.rows[self.ni + j]] += rho * dval[self.rows[self.ni + j]]
            for i in range(L - 1, -1, -1):
                if not self.live[i]:
                    continue
                w, dw = adj[i], dadj[i]
                o, a, b = self.ops[i], self.aa[i], self.bb[i]
                if o in (0, 2) or 17 <= o <= 23:
                    continue
                if o == 1:
                    out[a] += dw
                    continue
                va, ta = val[a], dval[a]
                vb, tb = (val[b], dval[b]) if o in _BINARY else (f8(0.0), f8(0.0))
                if o == 3:
                    dadj[a] += dw; dadj[b] += dw
                elif o == 4:
                    dadj[a] += dw; dadj[b] -= dw
                elif o == 5:
                    dadj[a] += dw * vb + w * tb; dadj[b] += dw * va + w * ta
                elif o == 6:
                    dadj[a] += (dw - w * tb / vb) / vb
                    dadj[b] -= (dw * va + w * ta - 2.0 * (w * va) * tb / vb) / (vb * vb)
                elif o == 7:
                    dadj[a] -= dw
                elif o == 8:
                    dadj[a] += dw * np.cos(va) - w * np.sin(va) * ta
                elif o == 9:
                    dadj[a] -= dw * np.sin(va) + w * np.cos(va) * ta
                elif o == 10:
                    d = va * va + vb * vb
                    dd = 2.0 * (va * ta + vb * tb)
                    dadj[a] += (dw * vb + w * (tb - vb * dd / d)) / d
                    dadj[b] -= (dw * va + w * (ta - va * dd / d)) / d
                elif o == 11:
                    r = val[i]
                    q = 0.5 / r
                    dadj[a] += dw * q - w * (q * dval[i] / r)
                elif o == 12:
                    dadj[a] += dw * 2.0 * va + w * 2.0 * ta
                elif o == 13:
                    s = (1.0 - va) * (1.0 + va)
                    r = np.sqrt(s)
                    dadj[a] += dw / r + w * (va * ta / (s * r))
                elif o == 14:
                    dadj[a] += dw * sign(va)
                elif o == 15 or o == 16:
                    dadj[a if (va <= vb if o == 15 else va >= vb) else b] += dw
                elif o == 24:
                    if va != 0.0:
                        dadj[b] += dw
                elif o == 25:
                    dadj[a] += dw * val[i] + w * dval[i]
                elif o == 26:
                    dadj[a] += (dw - w * ta / va) / va
        return out


def merit_hvp_port(tape, x, p, lam, mu, rho, v):
    """(generalised Hessian of the merit at x) v, (nx,): one phi, then one hess_vec."""
    ev = MeritEval(tape, p)
    ev.phi(np.asarray(x, float), np.asarray(lam, float), np.asarray(mu, float), float(rho))
    return ev.hess_vec(v)


# ---- (b) the state machine of oh_tape_newton.h ----------------------------------------------------------------------------------------------------------
def solve_tape_newton(tape, x0, p, tol=1e-6, tol_feas=1e-9, max_iter=2000, rho0=10.0, cg_cap=-1, h0=None, trace=None):
    """Port of k_tape_solve_newton: PHR outer loop of solve_tape_al, inner line-search truncated Newton-CG on exact merit curvature.  Returns solve_tape_al's
    keys (evals: phi evaluations) plus steps (accepted Newton-path steps) and hvps (products); the device's iters is evals + hvps."""
    n, ni, ne = int(tape.nx), int(tape.n_ineq), int(tape.n_eq)
    cap = int(cg_cap) if cg_cap > 0 else min(n, 50)
    ev = MeritEval(tape, p)
    lam, mu, rho = np.zeros(ni), np.zeros(ne), float(rho0)
    x = np.array(x0, dtype=float)
    M = (lambda r: h0 @ r) if h0 is not None else (lambda r: r.copy())
    val, grad, fval, cmax, meas = ev.phi(x, lam, mu, rho)
    evals, hvps, steps, status = 1, 0, 0, 1
    omega, meas_prev, msum = max(tol, 1e-2), 1e300, 0.0
    force_sd = False
    while True:
        stat = float(np.abs(grad).max()) if n else 0.0
        if not (np.isfinite(val) and abs(val) < 1e300) or np.isnan(grad).any():
            status = 2
            break
        if stat <= omega:
            if stat <= tol and meas <= tol_feas:
                status = 0
                break
            if evals + hvps >= max_iter:
                break
            mu = mu - rho * ev.rowv[ni:]
            lam = np.fmax(0.0, lam - rho * ev.rowv[:ni])
            msum = float(np.sum(np.abs(mu)) + np.sum(lam))
            if meas > 0.25 * meas_prev:
                rho = min(rho * 10.0, 1e8)
            meas_prev = meas
            omega = max(tol, min(omega, 0.1 * meas))
            val, grad, fval, cmax, meas = ev.phi(x, lam, mu, rho)
            evals += 1
            continue
        if evals + hvps >= max_iter:
            break
        newton = not force_sd
        if newton:
            # truncated CG on H d = -g, preconditioner M (the handle's metric, else the identity)
            z = np.zeros(n)
            r = grad.copy()
            y = M(r)
            pd = -y
            ry = float(r @ y)
            gnorm = float(np.sqrt(grad @ grad))
            eta = min(0.5, float(np.sqrt(gnorm)))
            d, unit = None, False
            for j in range(cap):
                hp = ev.hess_vec(pd)
                hvps += 1
                kappa, pp = float(pd @ hp), float(pd @ pd)
                if not kappa > 1e-12 * pp:  # negative or vanishing curvature, or NaN
                    d = -y if j == 0 else z
                    unit = j == 0  # the (preconditioned) gradient direction carries no Newton scale: unit-length cap below
                    newton = h0 is not None or j > 0  # without a metric it IS steepest descent: a failed search from it ends the instance
                    break
                a = ry / kappa
                z = z + a * pd
                r = r + a * hp
                if float(np.sqrt(r @ r)) <= eta * gnorm:
                    break
                if j + 1 == cap or evals + hvps + 1 >= max_iter:  # the cap; or what is left of the budget is the line search's first trial
                    break
                y = M(r)
                ryn = float(r @ y)
                pd = -y + (ryn / ry) * pd
                ry = ryn
            if d is None:
                d = z
        else:
            d, unit = -grad, True
        slope = float(grad @ d)
        if not slope < 0.0:
            d, unit = -grad, True
            slope = float(grad @ d)
            newton = False
        alpha = 1.0
        if unit:  # steepest descent knows nothing about the scale of the problem: the unit-length cap of the BFGS path's fresh metric
            alpha = min(1.0, 1.0 / float(np.abs(d).max()))
        ok = False
        slack = 4e-16 * (max(1.0, abs(val)) + msum)
        gg = float(grad @ grad)
        for _ in range(40):
            xt = x + alpha * d
            vt, gt, ft, ct, mt = ev.phi(xt, lam, mu, rho)
            evals += 1
            need = -1e-4 * alpha * slope
            fin = vt == vt
            if need > slack:
                if fin and vt <= val - need + slack:
                    ok = True
                    break
            elif fin and vt <= val - slack:
                ok = True
                break
            elif fin and vt <= val + slack:
                ggt = float(gt @ gt)
                if ggt <= (1.0 - 1e-4 * alpha) * gg and ggt < gg:
                    ok = True
                    break
            alpha *= 0.5
            if evals + hvps >= max_iter:
                break
        if not ok:
            if trace is not None:
                trace.append({"evals": evals, "hvps": hvps, "val": val, "stat": stat, "alpha": 0.0, "newton": newton, "rho": rho})
            val, grad, fval, cmax, meas = ev.phi(x, lam, mu, rho)  # val / adj / rowv belong to the rejected trial: back to x (the invariant of hess_vec)
            evals += 1
            if not newton or evals + hvps >= max_iter:
                break  # steepest descent cannot improve: rounding floor
            force_sd = True
            continue
        force_sd = False
        steps += 1
        x, val, grad, fval, cmax, meas = xt, vt, gt, ft, ct, mt
        if trace is not None:
            trace.append({"evals": evals, "hvps": hvps, "val": val, "stat": float(np.abs(grad).max()), "alpha": alpha, "newton": newton, "rho": rho})
    g, c = ev.rowv[:ni], ev.rowv[ni:]
    return {"x": x, "f": float(fval), "lam": lam, "mu": mu, "evals": evals, "status": status, "stat": float(np.abs(grad).max()),
            "feas": float(max(np.abs(c).max() if ne else 0.0, np.maximum(0.0, -g).max() if ni else 0.0)), "steps": steps, "hvps": hvps, "meas": float(meas)}


# ---- (c) the independent reference ------------------------------------------------------------------------------------------------------------------------
def al_seeds_mp(tape, x, p, lam, mu, rho):
    """(seeds (1 + rows,) float64 for tape_hvp_ref, active [rows] bool, margins lam - rho g of the inequality rows as float64), decided at >= 60 digits."""
    ni, ne = int(tape.n_ineq), int(tape.n_eq)
    with mpmath.workdps(tape_mp._dps(x, p, tape.c, lam, mu, [rho])):
        v = tape_mp.forward_mp(tape, x, p)
        rows = [v[int(r)] for r in tape.out_rows]
        if any(r is None for r in rows):
            raise tape_mp.NonFinite("a row has no finite value at this point")
        rh = tape_mp._exact(rho)
        seeds, active, margin = [mpmath.mpf(1)], [], []
        for i in range(ni):
            t = tape_mp._exact(lam[i]) - rh * rows[i]
            active.append(bool(t > 0))
            margin.append(float(t))
            seeds.append(-t if t > 0 else mpmath.mpf(0))
        for j in range(ne):
            active.append(True)
            seeds.append(-tape_mp._exact(mu[j]) + rh * rows[ni + j])
        return seeds, active, np.array(margin)


def row_gradients_mp(tape, x, p):
    """[rows][nx] list of lists of mpf: central differences (h = 1e-25) of oracle/tape_mp.py's registers, selections of the base point held."""
    mp = mpmath.mp
    xs, ps = [tape_mp._exact(t) for t in x], [tape_mp._exact(t) for t in p]
    base, sel = tape_mp._run(tape, xs, ps, None)
    rows = [int(r) for r in tape.out_rows]
    used = sorted(set(int(tape.a[i]) for i in range(len(tape.op)) if int(tape.op[i]) == 1))
    h = mp.mpf(tape_mp.H)
    J = [[mp.mpf(0)] * int(tape.nx) for _ in rows]
    for k in used:
        xp, xm = list(xs), list(xs)
        xp[k], xm[k] = xs[k] + h, xs[k] - h
        vp = tape_mp._run(tape, xp, ps, sel, base, k)[0]
        vm = tape_mp._run(tape, xm, ps, sel, base, k)[0]
        for i, r in enumerate(rows):
            J[i][k] = (vp[r] - vm[r]) / (2 * h)
    return J


def merit_hessian_mp(tape, x, p, lam, mu, rho):
    """The generalised Hessian of the merit (nx, nx) float64, and the inequality rows' margins lam - rho g (float64, decided in mp)."""
    nx = int(tape.nx)
    seeds, active, margin = al_seeds_mp(tape, x, p, lam, mu, rho)
    with mpmath.workdps(tape_mp._dps(x, p, tape.c, lam, mu, [rho]) + 10):
        # tape_hvp_ref._Mp takes the seeds as they are (mpf): second differences of cost + sum seed_r row_r
        m = R._Mp(tape, x, p, [0.0] * len(seeds))
        m.w = list(seeds)
        m.L0 = m.combine(m.base)
        H = [[mpmath.mpf(0)] * nx for _ in range(nx)]
        hh = 4 * m.h * m.h
        for j in m.used:
            H[j][j] = (m.at({j: 2}, (j,)) - 2 * m.L0 + m.at({j: -2}, (j,))) / hh
        for a, j in enumerate(m.used):
            for k in m.used[a + 1:]:
                d = m.at({j: 1, k: 1}, (j, k)) - m.at({j: 1, k: -1}, (j, k)) - m.at({j: -1, k: 1}, (j, k)) + m.at({j: -1, k: -1}, (j, k))
                H[j][k] = H[k][j] = d / hh
        J = row_gradients_mp(tape, x, p)
        rh = tape_mp._exact(rho)
        out = np.zeros((nx, nx))
        for j in range(nx):
            for k in range(nx):
                s = H[j][k]
                for i, act in enumerate(active):
                    if act:
                        s += rh * J[i][j] * J[i][k]
                out[j, k] = float(s)
    return out, margin


# ---- the cases both test files grade ----------------------------------------------------------------------------------------------------------------------
RHOS = (1.0, 100.0)
MARGIN = 1e-3  # |lam - rho g| of every inequality row is at least this: float64 and mp agree on the active set
_cache = {}


def _with_a_row(tp):
    """A tape without rows gets one appended: its cost register as a >= row."""
    if int(tp.n_ineq) + int(tp.n_eq) > 0:
        return tp
    import tape_cases

    return tape_cases.make(tp.op, tp.a, tp.b, tp.c, tp.out_cost, [int(tp.out_cost)], 1, 0, tp.nx, tp.np_)


def merit_cases():
    """[(name, tape, x, p, lam, mu, rho)]: tape_hvp_ref.composite_cases() under both penalties.  Inequality row i is made active (lam = rho g + 0.5, or 0.5 - rho g
    > 0 with lam = 0.5 where that is negative) when i + (index of rho) is even, otherwise inactive (lam = max(0, rho g - 0.5)) where a multiplier >= 0 allows it
    with the margin (rho g >= MARGIN; active like the others where not); mu ~ U(-1, 1) from a fixed generator."""
    if "cases" not in _cache:
        out = []
        rng = np.random.default_rng(29)
        for name, tp0, x, p, _, _ in R.composite_cases():
            tp = _with_a_row(tp0)
            ni, ne = int(tp.n_ineq), int(tp.n_eq)
            with np.errstate(all="ignore"):  # (the "dead" tape holds a log of a negative number nobody reads)
                g = tape_ref.forward(tp, x, p)[np.asarray(tp.out_rows, int)[:ni]] if ni else np.zeros(0)
            mu = rng.uniform(-1.0, 1.0, ne)
            for k, rho in enumerate(RHOS):
                lam = np.array([max(0.0, rho * g[i]) + 0.5 if ((i + k) % 2 == 0 or rho * g[i] < MARGIN) else max(0.0, rho * g[i] - 0.5) for i in range(ni)])
                out.append((name, tp, x, p, lam, mu, rho))
        _cache["cases"] = out
    return _cache["cases"]


def merit_reference(name, rho):
    """(H (nx, nx) by mp, margins lam - rho g by mp) of one case, computed once per process."""
    key = ("ref", name, rho)
    if key not in _cache:
        _, tp, x, p, lam, mu, _ = next(c for c in merit_cases() if c[0] == name and c[6] == rho)
        _cache[key] = merit_hessian_mp(tp, x, p, lam, mu, rho)
    return _cache[key]


def merit_hessian_port(tp, x, p, lam, mu, rho):
    ev = MeritEval(tp, p)
    ev.phi(np.asarray(x, float), np.asarray(lam, float), np.asarray(mu, float), float(rho))
    return np.stack([ev.hess_vec(e) for e in np.eye(int(tp.nx))])


def kept_merit_cases():
    """(the cases on which the port is within DEVICE_TOL of mp, [(name, rho, error)] of those dropped)."""
    if "kept" not in _cache:
        kept, dropped = [], []
        for c in merit_cases():
            H, _ = merit_reference(c[0], c[6])
            ok, err = R.within(merit_hessian_port(*c[1:]), H, R.DEVICE_TOL)
            (kept if ok else dropped).append(c if ok else (c[0], c[6], err))
        _cache["kept"] = (kept, dropped)
    return _cache["kept"]


def tiny_problems():
    """{name: (tape, x0)}: cos(x0) + x1^2 / 2 (negative curvature at the start), Rosenbrock, (x0 - 1)^4 (singular Hessian at the optimum)."""
    import tape_cases

    out = {}
    t = tape_cases.B()
    x0, x1 = t.x(0), t.x(1)
    out["cos"] = (t.tape(t.emit(3, t.emit(9, x0), t.emit(5, t.const(0.5), t.emit(12, x1))), [], 0, 0, 2, 0), np.array([0.1, 1.0]))
    t = tape_cases.B()
    x0, x1 = t.x(0), t.x(1)
    a = t.emit(12, t.emit(4, t.const(1.0), x0))
    bq = t.emit(5, t.const(100.0), t.emit(12, t.emit(4, x1, t.emit(12, x0))))
    out["rosenbrock"] = (t.tape(t.emit(3, a, bq), [], 0, 0, 2, 0), np.array([-1.2, 1.0]))
    t = tape_cases.B()
    out["quartic"] = (t.tape(t.emit(12, t.emit(12, t.emit(4, t.x(0), t.const(1.0)))), [], 0, 0, 1, 0), np.array([3.0]))
    return out
