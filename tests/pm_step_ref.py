"""50-digit reference of the first k iterations of the point-mass interior-point state machine (oracle/pointmass_ipm.py, csrc/oh_pointmass.hip).

What the port and the two kernels share is the Riccati recursion that produces the Newton direction and the adjoint recursion behind the
stationarity figure.  Neither appears here.  The direction is the dense solve of the condensed Newton system: the free controls
(a_0 .. a_{T-2}, or a_0 .. a_{T-3} under fix_final_velocity, whose last control is da_{T-2} = -dv_{T-2} / dt) are the unknowns, the
stacked (dx_1 .. dx_{T-1}, da_0 .. da_{T-2}) are a linear map M of them (the two axes have the same scalar roll-out coefficients), and

    H = M^T blkdiag(Q_1 .. Q_{T-1}, R .. R) M,    g = M^T (q_1 .. q_{T-1}, 2 w a_0 .. 2 w a_{T-2}),    H u = -g

with the port's own Q_t = diag(2 wt, 2 wt, 2 w_vel, 2 w_vel) + J_t^T Sig_t J_t, q_t = gx_t - J_t^T (mu / s - Sig rc), R = 2 w I.  The stationarity
figure is max |M^T (lx_1 .. lx_{T-1}, 2 w a)| over the free controls: the gradient of the Lagrangian through the same map.  The rest (seed, slacks
and multipliers, ds, dlam, the two fraction-to-the-boundary lengths, the updates, the exact roll-out, the sigma ladder, mu) is restated in mp.

Inputs are float64 numbers taken exactly; the literals of the algorithm (0.995, 0.1, 0.3, 0.8, 1e-2) are the float64 values the port and the
kernels use."""
import numpy as np
from mpmath import mp, mpf

DPS = 50
NI = 9


def _f(v):
    return mpf(float(v))


def _cons(x, ob, ylim, vlim, safe_sq):
    """c (9) and the obstacle row's (jx, jy); the box rows' Jacobian entries are +-1 on their own coordinate."""
    dx, dy = x[0] - ob[0], x[1] - ob[1]
    c = [x[0] + ylim, ylim - x[0], x[1] + ylim, ylim - x[1], x[2] + vlim, vlim - x[2], x[3] + vlim, vlim - x[3], dx * dx + dy * dy - safe_sq]
    return c, 2 * dx, 2 * dy


def _JTw(w, jx, jy):
    return [w[0] - w[1] + jx * w[8], w[2] - w[3] + jy * w[8], w[4] - w[5], w[6] - w[7]]


def _Jv(v, jx, jy):
    return [v[0], -v[0], v[1], -v[1], v[2], -v[2], v[3], -v[3], jx * v[0] + jy * v[1]]


def _rollout(T, dt, curr, dcurr, a):
    X = [[curr[0], curr[1], dcurr[0], dcurr[1]]]
    for t in range(T - 1):
        x = X[-1]
        X.append([x[0] + dt * x[2], x[1] + dt * x[3], x[2] + dt * a[t][0], x[3] + dt * a[t][1]])
    return X


def _control_map(T, dt, pinned):
    """Scalar roll-out coefficients of one axis: for every free control s the lists cy[s][t], cv[s][t] (t = 0 .. T-1) of dy_t, dv_t per unit da_s,
    and ca[s] = {t: coefficient of da_t}.  Made by rolling unit controls out, the pinned control as a function of the state."""
    nf = T - 2 if pinned else T - 1
    cy, cv, ca = [], [], []
    for s in range(nf):
        y, v = [mpf(0)], [mpf(0)]
        acts = {}
        for t in range(T - 1):
            if pinned and t == T - 2:
                da = -v[t] / dt
            else:
                da = mpf(1) if t == s else mpf(0)
            if da != 0:
                acts[t] = da
            y.append(y[t] + dt * v[t])
            v.append(v[t] + dt * da)  # (under the pin dv_{T-1} = dv_{T-2} + dt (-dv_{T-2} / dt): zero to the working precision, not by decree)
        cy.append(y), cv.append(v), ca.append(acts)
    return nf, cy, cv, ca


def _cholesky_solve(H, rhs):
    n = len(H)
    L = [[mpf(0)] * n for _ in range(n)]
    for i in range(n):
        Li = L[i]
        for j in range(i):
            Lj = L[j]
            Li[j] = (H[i][j] - mp.fdot(Li[:j], Lj[:j])) / Lj[j]
        d = H[i][i] - mp.fdot(Li[:i], Li[:i])
        if not d > 0:
            raise ArithmeticError("condensed Hessian is not positive definite")
        Li[i] = mp.sqrt(d)
    y = [mpf(0)] * n
    for i in range(n):
        y[i] = (rhs[i] - mp.fdot(L[i][:i], y[:i])) / L[i][i]
    x = [mpf(0)] * n
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - mp.fsum(L[k][i] * x[k] for k in range(i + 1, n))) / L[i][i]
    return x


def pm_steps_mp(T, dt, w, ylim, vlim, safe_sq, curr, dcurr, goal, obs, V0=None, k_max=3, tol=1e-8, track_final_only=False, w_vel=0.0,
                fix_final_velocity=False):
    """The state machine with max_iter = 1 .. k_max at once (the iterates of a shorter run are a prefix of a longer one's).
    goal, obs: (2, T) float64; V0: (2, T) velocity seed or None.
    Returns a list over the evaluations it = 0 .. k_max (as far as the machine runs) of dict(x, f, kkt, status, mp=...) -- entry k is what a solve
    with max_iter = k returns when it neither converged nor was declared infeasible earlier: x (4T,) in the reference layout, f and
    kkt = (stat, feas, compl) at the point after the k-th step, rounded to float64, status 0 / 1 / 3 of that evaluation.  Entry k >= 1 also has the
    step that led to it: ap, ad (mpf), dv_last (|dv_{T-1}| of the Newton direction, mpf) and v_last (|v_{T-1}| after it)."""
    old = mp.dps
    mp.dps = DPS
    try:
        return _steps(int(T), _f(dt), _f(w), _f(ylim), _f(vlim), _f(safe_sq), curr, dcurr, goal, obs, V0, int(k_max), _f(tol), bool(track_final_only),
                      _f(w_vel), bool(fix_final_velocity))
    finally:
        mp.dps = old


def _steps(T, dt, w, ylim, vlim, safe_sq, curr, dcurr, goal, obs, V0, k_max, tol, final_only, w_vel, pinned):
    curr, dcurr = [_f(v) for v in curr], [_f(v) for v in dcurr]
    goal = [[_f(goal[0][t]), _f(goal[1][t])] for t in range(T)]
    obs = [[_f(obs[0][t]), _f(obs[1][t])] for t in range(T)]
    V = [[mpf(0), mpf(0)] for _ in range(T)] if V0 is None else [[_f(V0[0][t]), _f(V0[1][t])] for t in range(T)]
    V[0] = list(dcurr)
    if pinned:
        V[T - 1] = [mpf(0), mpf(0)]
    a = [[(V[t + 1][j] - V[t][j]) / dt for j in range(2)] for t in range(T - 1)]
    wt = [mpf(0) if (final_only and t < T - 1) else mpf(1) for t in range(T)]
    nf, cy, cv, ca = _control_map(T, dt, pinned)
    tau, floor_s, mu = _f(0.995), _f(1e-2), _f(0.1)
    X = _rollout(T, dt, curr, dcurr, a)
    s, lam = [None] * T, [None] * T
    for t in range(T):
        c, _, _ = _cons(X[t], obs[t], ylim, vlim, safe_sq)
        s[t] = [max(ci, floor_s) for ci in c]
        lam[t] = [mu / si for si in s[t]]
    out, step = [], None
    for it in range(k_max + 1):
        cs, jxs, jys, rcs, gxs, lxs = [None] * T, [None] * T, [None] * T, [None] * T, [None] * T, [None] * T
        for t in range(T):
            c, jx, jy = _cons(X[t], obs[t], ylim, vlim, safe_sq)
            cs[t], jxs[t], jys[t] = c, jx, jy
            rcs[t] = [c[i] - s[t][i] for i in range(NI)]
            gxs[t] = [-2 * wt[t] * (goal[t][0] - X[t][0]), -2 * wt[t] * (goal[t][1] - X[t][1]), 2 * w_vel * X[t][2], 2 * w_vel * X[t][3]]
            jl = _JTw(lam[t], jx, jy)
            lxs[t] = [gxs[t][j] - jl[j] for j in range(4)]

        def through_map(rows):
            """M^T (rows_1 .. rows_{T-1}, 2 w a): rows[t] is a 4-vector on x_t"""
            g = []
            for sidx in range(nf):
                for j in range(2):
                    v = mp.fdot(cy[sidx][1:], [rows[t][j] for t in range(1, T)]) + mp.fdot(cv[sidx][1:], [rows[t][2 + j] for t in range(1, T)])
                    v += mp.fsum(coef * 2 * w * a[t][j] for t, coef in ca[sidx].items())
                    g.append(v)
            return g

        gl = through_map(lxs)
        stat = max(abs(v) for v in gl) if gl else mpf(0)
        feas = max(abs(r) for t in range(1, T) for r in rcs[t])
        compl = max(lam[t][i] * s[t][i] for t in range(1, T) for i in range(NI))
        fval = mp.fsum(wt[t] * ((goal[t][0] - X[t][0]) ** 2 + (goal[t][1] - X[t][1]) ** 2) + w_vel * (X[t][2] ** 2 + X[t][3] ** 2) for t in range(T))
        fval += w * mp.fsum(a[t][0] ** 2 + a[t][1] ** 2 for t in range(T - 1))
        status = 1
        if stat <= tol and feas <= tol and compl <= tol:
            status = 0
        elif compl > _f(1e6) and feas > _f(1e3) * tol:
            status = 3
        x = np.array([float(X[t][j]) for t in range(T) for j in range(2)] + [float(X[t][2 + j]) for t in range(T) for j in range(2)])
        rec = {"x": x, "f": float(fval), "kkt": np.array([float(stat), float(feas), float(compl)]), "status": status, "iters": it}
        if step is not None:
            rec.update(step, v_last=max(abs(X[T - 1][2]), abs(X[T - 1][3])))
        out.append(rec)
        if status != 1 or it == k_max:
            break
        # ---- Newton step: dense solve of the condensed system
        sig = [[lam[t][i] / s[t][i] for i in range(NI)] for t in range(T)]
        Q00, Q01, Q11, Qv0, Qv1, q = [mpf(0)] * T, [mpf(0)] * T, [mpf(0)] * T, [mpf(0)] * T, [mpf(0)] * T, [None] * T
        for t in range(1, T):
            sg, jx, jy = sig[t], jxs[t], jys[t]
            Q00[t] = 2 * wt[t] + sg[0] + sg[1] + sg[8] * jx * jx
            Q11[t] = 2 * wt[t] + sg[2] + sg[3] + sg[8] * jy * jy
            Q01[t] = sg[8] * jx * jy
            Qv0[t] = 2 * w_vel + sg[4] + sg[5]
            Qv1[t] = 2 * w_vel + sg[6] + sg[7]
            jq = _JTw([mu / s[t][i] - sg[i] * rcs[t][i] for i in range(NI)], jx, jy)
            q[t] = [gxs[t][j] - jq[j] for j in range(4)]
        q[0] = [mpf(0)] * 4
        g = through_map(q)
        n = 2 * nf
        H = [[mpf(0)] * n for _ in range(n)]
        yQ = {name: [[cy[sidx][t] * Qt[t] for t in range(T)] for sidx in range(nf)] for name, Qt in (("00", Q00), ("01", Q01), ("11", Q11))}
        vQ = {name: [[cv[sidx][t] * Qt[t] for t in range(T)] for sidx in range(nf)] for name, Qt in (("0", Qv0), ("1", Qv1))}
        for s1 in range(nf):
            for s2 in range(s1 + 1):
                lo = s1 + 1  # knots up to the later control do not move with it
                aa = mp.fsum(coef * ca[s2].get(t, 0) for t, coef in ca[s1].items()) * 2 * w  # R
                h00 = mp.fdot(yQ["00"][s1][lo:], cy[s2][lo:]) + mp.fdot(vQ["0"][s1][lo:], cv[s2][lo:]) + aa
                h11 = mp.fdot(yQ["11"][s1][lo:], cy[s2][lo:]) + mp.fdot(vQ["1"][s1][lo:], cv[s2][lo:]) + aa
                h01 = mp.fdot(yQ["01"][s1][lo:], cy[s2][lo:])
                for (j1, j2, v) in ((0, 0, h00), (1, 1, h11), (0, 1, h01), (1, 0, h01)):
                    H[2 * s1 + j1][2 * s2 + j2] = v
                    H[2 * s2 + j2][2 * s1 + j1] = v
        u = _cholesky_solve(H, [-v for v in g])
        dX = [[mpf(0)] * 4 for _ in range(T)]
        for t in range(1, T):
            for j in range(2):
                dX[t][j] = mp.fdot([cy[sidx][t] for sidx in range(nf)], u[j::2])
                dX[t][2 + j] = mp.fdot([cv[sidx][t] for sidx in range(nf)], u[j::2])
        da = [[mpf(0), mpf(0)] for _ in range(T - 1)]
        for sidx in range(nf):
            for t, coef in ca[sidx].items():
                for j in range(2):
                    da[t][j] += coef * u[2 * sidx + j]
        ap, ad = mpf(1), mpf(1)
        ds, dl = [None] * T, [None] * T
        for t in range(1, T):
            d = _Jv(dX[t], jxs[t], jys[t])
            ds[t] = [d[i] + rcs[t][i] for i in range(NI)]
            dl[t] = [(mu / s[t][i] - lam[t][i]) - sig[t][i] * ds[t][i] for i in range(NI)]
            for i in range(NI):
                if ds[t][i] < 0:
                    ap = min(ap, -tau * s[t][i] / ds[t][i])
                if dl[t][i] < 0:
                    ad = min(ad, -tau * lam[t][i] / dl[t][i])
        a = [[a[t][j] + ap * da[t][j] for j in range(2)] for t in range(T - 1)]
        X = _rollout(T, dt, curr, dcurr, a)
        gap = mpf(0)
        for t in range(1, T):
            s[t] = [s[t][i] + ap * ds[t][i] for i in range(NI)]
            lam[t] = [lam[t][i] + ad * dl[t][i] for i in range(NI)]
            gap += mp.fdot(s[t], lam[t])
        gap /= NI * (T - 1)
        am = min(ap, ad)
        sigma = _f(0.1) if am > _f(0.9) else (_f(0.3) if am > _f(0.5) else _f(0.8))
        mu = max(sigma * gap, _f(1e-2) * tol)
        step = {"ap": ap, "ad": ad, "dv_last": max(abs(dX[T - 1][2]), abs(dX[T - 1][3]))}
    return out
