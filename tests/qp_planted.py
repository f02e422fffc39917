"""Planted dense QPs for the QP family (optas_amd/csrc/oh_qp.hip, numpy port oracle/qp_ipm.py):

    min x^T P x + q^T x   s.t.  M x + c >= 0,  A x + b = 0.

The optimum is planted, not solved for: draw P, M, A, x*, lam* >= 0, nu* and slacks sigma >= 0 with lam*_i sigma_i = 0, then set

    q = -(P + P^T) x* + M^T lam* + A^T nu*,      c = sigma - M x*,      b = -A x*,

so x* is a KKT point with multipliers (lam*, nu*), and for the classes below the unique optimum.  All data are small dyadic rationals
(multiples of 1/8 in [-4, 4]; P = G G^T / 2 (+ I / 8), multiples of 1/128): every product and sum above is exact in float64, so q, c, b
and f* = x*^T P x* + q^T x* carry no rounding.  `check_exact` recomputes an instance with fractions.Fraction.

Left out on purpose, because the iteration itself (the port alone, on the CPU) does not converge on all instances there:
  * rank-deficient P with exactly n - rank active-plus-equality rows (the port runs into max_iter on some, x error 2e-6);
  * badly scaled P (1e3 diagonal scaling): the absolute tol = 1e-9 is out of reach, the port ends with status 1.
"""
import functools
from fractions import Fraction

import numpy as np

EPS = float(np.finfo(np.float64).eps)
TOL = 1e-9  # oh_qp_desc.tol / solve_qp_ipm's default
BIG = 1e9   # the bound rows of the reference's Booth test with constraint=True

# name -> arguments of make_qp.  na: active rows (sigma = 0); the others have sigma in [1/8, 4] (or BIG).
CLASSES = {
    "base": dict(n=6, m=10, me=2, na=2),
    "n1": dict(n=1, m=2, me=0, na=1),
    "n1_eq": dict(n=1, m=0, me=1, na=0),
    "m100": dict(n=8, m=100, me=0, na=5),
    "m256": dict(n=8, m=256, me=2, na=4),
    "m65": dict(n=32, m=65, me=8, na=10),
    "me_eq_n": dict(n=5, m=6, me=5, na=0),
    "vertex": dict(n=6, m=20, me=0, na=6),
    "vertex_eq": dict(n=7, m=16, me=3, na=4),
    "rank_def": dict(n=8, m=20, me=2, na=4, rank=3),  # na + me = 6 > n - rank = 5
    "lp": dict(n=6, m=20, me=0, na=6, rank=0),
    "lp_eq": dict(n=6, m=20, me=2, na=4, rank=0),
    "nonsym": dict(n=6, m=10, me=2, na=2, skew=True),  # same draws as "base" plus a skew part: same optimum
    "dup_row": dict(n=6, m=10, me=0, na=3, dup=True),  # row 1 copies row 0: compare x, f and lam_0 + lam_1
    "weak_row": dict(n=6, m=10, me=0, na=3, weak=True),  # one active row with lam* = 0: compare x and f only
    "big_rows": dict(n=6, m=10, me=2, na=2, big=3),
    "max_inactive": dict(n=32, m=256, me=32, na=0),
    "max": dict(n=32, m=256, me=16, na=12),
}
_SEED0 = {name: 7000 + 1000 * i for i, name in enumerate(CLASSES)}
_SEED0["nonsym"] = _SEED0["base"]
_SEED0["weak_row"] = 100  # (seeds on which the port needs at most 40 iterations: without strict complementarity it converges linearly)
N_INST = 24

# Port (oracle/qp_ipm.py) against the planted optimum, 24 instances per class (test_qp_planted_cpu.py prints and re-checks them):
# max |x - x*|, max |f - f*| / max(1, |f*|), max multiplier error.  Measured on the CPU; the GPU bound is 10 times these.
PORT_ERR = {
    "base": (2.053e-09, 3.375e-11, 1.125e-08),  # iters <= 14
    "n1": (1.892e-08, 4.271e-10, 2.766e-07),  # iters <= 12
    "n1_eq": (4.974e-13, 9.006e-13, 6.899e-12),  # iters <= 1
    "m100": (7.164e-09, 1.148e-11, 2.420e-08),  # iters <= 16
    "m256": (4.593e-09, 3.839e-12, 9.350e-08),  # iters <= 17
    "m65": (6.790e-10, 8.548e-13, 1.680e-08),  # iters <= 18
    "me_eq_n": (2.442e-15, 1.967e-15, 3.638e-08),  # iters <= 11
    "vertex": (2.882e-09, 9.822e-11, 3.621e-06),  # iters <= 18
    "vertex_eq": (3.771e-09, 9.953e-12, 9.347e-07),  # iters <= 15
    "rank_def": (1.031e-08, 4.408e-11, 2.657e-08),  # iters <= 17
    "lp": (5.938e-09, 4.920e-10, 7.772e-08),  # iters <= 19
    "lp_eq": (2.132e-08, 2.034e-10, 8.031e-08),  # iters <= 17
    "nonsym": (2.053e-09, 3.375e-11, 1.125e-08),  # iters <= 14
    "dup_row": (5.564e-09, 1.488e-11, 7.253e-09),  # iters <= 15
    "weak_row": (2.436e-06, 1.580e-13, 0.000e+00),  # iters <= 29
    "big_rows": (4.568e-09, 1.220e-11, 5.160e-07),  # iters <= 15
    "max_inactive": (2.212e-13, 3.866e-16, 5.697e-07),  # iters <= 11
    "max": (1.245e-09, 8.018e-13, 1.063e-07),  # iters <= 17
}
MARGIN = 10.0


def bound(name):
    return tuple(MARGIN * v for v in PORT_ERR[name])


def _dy(rng, shape, lo=-4.0, hi=4.0):
    return rng.integers(int(8 * lo), int(8 * hi) + 1, shape) / 8.0


def make_qp(name, seed):
    a = CLASSES[name]
    n, m, me, na = a["n"], a["m"], a["me"], a["na"]
    rank = a.get("rank", n)
    rng = np.random.default_rng(seed)
    G = _dy(rng, (n, rank))
    Ps = 0.5 * (G @ G.T) + (np.eye(n) / 8.0 if rank == n else 0.0)
    M, A = _dy(rng, (m, n)), _dy(rng, (me, n))
    if n == 1:  # a zero coefficient is a row without a variable
        M[M == 0.0] = A[A == 0.0] = 0.125
    xs, nus = _dy(rng, n), _dy(rng, me)
    act = np.arange(na) if a.get("dup") else np.sort(rng.choice(m, na, replace=False))
    if m > 64 and na and act.max() < 64:
        act[-1] = rng.integers(64, m)  # an active row in the second pass of the wavefront kernel's row loops
    lam = np.zeros(m)
    sig = _dy(rng, m, 0.125, 4.0)
    lam[act] = _dy(rng, na, 0.125, 4.0)
    sig[act] = 0.0
    K = np.zeros((n, n))
    if a.get("skew"):  # drawn last: everything else equals the "base" instance of the same seed
        U = np.triu(_dy(rng, (n, n), -2.0, 2.0), 1)
        K = U - U.T
    if a.get("dup"):
        M[1] = M[0]
    if a.get("weak"):
        lam[act[-1]] = 0.0
    if a.get("big"):
        inact = np.setdiff1d(np.arange(m), act)
        sig[inact[: a["big"]]] = BIG
    P = Ps + K
    q = -(P + P.T) @ xs + M.T @ lam + A.T @ nus
    c = sig - M @ xs
    b = -A @ xs
    f = float(xs @ P @ xs + q @ xs)
    return dict(name=name, n=n, m=m, me=me, G=G, K=K, P=P, q=q, M=M, c=c, A=A, b=b, x=xs, lam=lam, nu=nus, sigma=sig, f=f, act=act)


@functools.lru_cache(maxsize=None)
def planted_instances(name):
    """The N_INST instances of a class (fixed seeds), the ones the port's errors are recorded on.  Shared: leave unchanged."""
    return tuple(make_qp(name, _SEED0[name] + i) for i in range(N_INST))


def planted_batch(name, B):
    """A batch of B: instance i of the batch is instance i % N_INST of the class, so every one of them has a recorded port error."""
    qps = planted_instances(name)
    return [qps[i % N_INST] for i in range(B)]


def pack(qp):
    return np.concatenate([np.asarray(qp[k], dtype=np.float64).reshape(-1) for k in ("P", "q", "M", "c", "A", "b")])


def check_exact(qp):
    """The float64 data of an instance equals the same construction in rational arithmetic."""
    F = lambda arr: [[Fraction(float(v)) for v in row] for row in np.atleast_2d(arr)]
    n, m, me = qp["n"], qp["m"], qp["me"]
    G, K, M, A = F(qp["G"]) if qp["G"].size else [[] for _ in range(n)], F(qp["K"]), F(qp["M"]) if m else [], F(qp["A"]) if me else []
    xs, lam, nu, sig = ([Fraction(float(v)) for v in qp[k]] for k in ("x", "lam", "nu", "sigma"))
    full = qp["G"].shape[1] == n
    P = [[sum(G[i][k] * G[j][k] for k in range(len(G[i]))) / 2 + (Fraction(1, 8) if (full and i == j) else 0) + K[i][j] for j in range(n)] for i in range(n)]
    q = [-sum((P[i][j] + P[j][i]) * xs[j] for j in range(n)) + sum(M[k][i] * lam[k] for k in range(m)) + sum(A[k][i] * nu[k] for k in range(me)) for i in range(n)]
    c = [sig[k] - sum(M[k][j] * xs[j] for j in range(n)) for k in range(m)]
    b = [-sum(A[k][j] * xs[j] for j in range(n)) for k in range(me)]
    f = sum(xs[i] * P[i][j] * xs[j] for i in range(n) for j in range(n)) + sum(q[i] * xs[i] for i in range(n))
    same = lambda fr, arr: all(Fraction(float(v)) == w for v, w in zip(np.asarray(arr).reshape(-1), fr))
    assert same([v for row in P for v in row], qp["P"]) and same(q, qp["q"]) and same(c, qp["c"]) and same(b, qp["b"]) and Fraction(qp["f"]) == f
    # the planted point is a KKT point in exact arithmetic: feasible, complementary, stationary (by construction of q; restated from the packed data)
    assert all(sum(M[k][j] * xs[j] for j in range(n)) + Fraction(float(qp["c"][k])) == sig[k] >= 0 for k in range(m))
    assert all(lam[k] >= 0 and lam[k] * sig[k] == 0 for k in range(m))
    assert all(sum(A[k][j] * xs[j] for j in range(n)) + Fraction(float(qp["b"][k])) == 0 for k in range(me))


def errors(qp, x, f, lam, nu):
    """(max |x - x*|, |f - f*| / max(1, |f*|), multiplier error) of a returned point; the multiplier error follows the class's rule."""
    ex = float(np.abs(np.asarray(x) - qp["x"]).max())
    ef = abs(float(f) - qp["f"]) / max(1.0, abs(qp["f"]))
    a = CLASSES[qp["name"]]
    lam, ls = np.array(lam, dtype=float), qp["lam"].copy()
    if a.get("weak"):
        return ex, ef, 0.0
    if a.get("dup"):  # only the sum over the two copies is determined
        lam[0], ls[0] = lam[0] + lam[1], ls[0] + ls[1]
        lam[1] = ls[1] = 0.0
    em = max(float(np.abs(lam - ls).max(initial=0.0)), float(np.abs(np.asarray(nu) - qp["nu"]).max(initial=0.0)))
    return ex, ef, em


def kkt_certificate(qp, x, lam, nu):
    """KKT residuals of (x, lam, nu) for the data P, q, M, c, A, b of `qp`, evaluated with mpmath at 50 digits, and for each row the bound
    (n + m + me + 2) eps sum|terms| on what float64 evaluation of that row can differ by.  Returns a dict of floats:
    stat = max |(P + P^T) x + q - M^T lam - A^T nu|, min_s = min(M x + c), max_eq = max |A x + b|, min_lam, max_comp = max lam_i (M x + c)_i,
    the bounds stat_bound / s_bound / eq_bound (maxima over the rows) and ok_s / ok_eq: every row within TOL plus its own bound."""
    import mpmath as mp

    with mp.workdps(50):
        n = len(x)
        P, M, A = np.atleast_2d(qp["P"]), np.asarray(qp["M"], dtype=float).reshape(-1, n), np.asarray(qp["A"], dtype=float).reshape(-1, n)
        q, c, b = (np.asarray(qp[k], dtype=float).reshape(-1) for k in ("q", "c", "b"))
        m, me = M.shape[0], A.shape[0]
        k = (n + m + me + 2) * EPS
        f = lambda v: mp.mpf(float(v))
        X, L, N = [f(v) for v in x], [f(v) for v in lam], [f(v) for v in nu]
        stat, stat_b = mp.mpf(0), mp.mpf(0)
        for i in range(n):
            terms = [f(q[i])] + [(f(P[i, j]) + f(P[j, i])) * X[j] for j in range(n)] + [-f(M[r, i]) * L[r] for r in range(m)] + [-f(A[r, i]) * N[r] for r in range(me)]
            stat, stat_b = max(stat, abs(mp.fsum(terms))), max(stat_b, k * mp.fsum(abs(t) for t in terms))
        s, s_b = [], []
        for r in range(m):
            terms = [f(c[r])] + [f(M[r, j]) * X[j] for j in range(n)]
            s.append(mp.fsum(terms))
            s_b.append(k * mp.fsum(abs(t) for t in terms))
        e, e_b = [], []
        for r in range(me):
            terms = [f(b[r])] + [f(A[r, j]) * X[j] for j in range(n)]
            e.append(abs(mp.fsum(terms)))
            e_b.append(k * mp.fsum(abs(t) for t in terms))
        return dict(stat=float(stat), stat_bound=float(stat_b), min_s=float(min(s, default=mp.inf)), s_bound=float(max(s_b, default=0)),
                    max_eq=float(max(e, default=0)), eq_bound=float(max(e_b, default=0)), min_lam=float(min(L, default=mp.inf)),
                    max_comp=float(max((L[r] * s[r] for r in range(m)), default=0)),
                    ok_s=all(s[r] >= -(TOL + s_b[r]) for r in range(m)), ok_eq=all(e[r] <= TOL + e_b[r] for r in range(me)))


def assert_certificate(cert, kkt=None):
    """What a point returned with status CONVERGED must satisfy; kkt: the triple the solver reported for it."""
    assert cert["stat"] <= TOL + cert["stat_bound"], cert
    assert cert["ok_s"] and cert["ok_eq"] and cert["min_lam"] >= 0.0, cert
    if kkt is not None:
        assert abs(float(kkt[0]) - cert["stat"]) <= cert["stat_bound"], (kkt, cert)


# ---- which kernel a solve runs: restatement of oh_launch_qp_solve (oh_qp.hip) and of Q.np / Q.nwork (oh_api_qp.hip) -----------------------
def qp_sizes(n, m, me):
    np_ = n * n + n + m * n + m + me * n + me
    nwork = n + 2 * m + me + n * n + 2 * n + 2 * m + me * n + me * me + me + n
    return np_, nwork


def _fit(doubles):
    for c in (64, 32, 16):
        if 8 * doubles * c <= 48 * 1024:
            return c
    return 0


def launch_path(n, m, me, B, qp_mode=-1):
    """("wave", 64) or ("thread", mode, instances per block) for a solve of B instances with option qp_mode."""
    np_, nwork = qp_sizes(n, m, me)
    bs2, bs1 = _fit(nwork + np_), _fit(nwork)
    if qp_mode not in (0, 1, 2) and B <= 64 and 8 * (nwork + np_) <= 48 * 1024:
        return ("wave", 64)
    mode = 2 if bs2 else (1 if bs1 else 0)
    if qp_mode == 0 or (qp_mode == 1 and bs1) or (qp_mode == 2 and bs2):
        mode = qp_mode
    return ("thread", mode, {2: bs2, 1: bs1, 0: 64}[mode])


def forced_fits(n, m, me, qp_mode):
    """The forced mode is the one that runs (a forced mode that does not fit LDS falls back to the automatic choice)."""
    return launch_path(n, m, me, 70, qp_mode)[1] == qp_mode


GPU_BATCHES = (70, 40, 1, 64, 65)  # 70 with qp_mode -1 and every forced mode that fits; the others with qp_mode -1


# ---- inputs of the isolation and device-assembly tests -----------------------------------------------------------------------------------
def bad_instances(qp):
    """Three rows no iteration can solve: contradictory rows x_0 >= 1 and x_0 <= 0, an LP without a bounding row, a nan in q."""
    n, m = qp["n"], qp["m"]
    contra = {k: np.array(qp[k], dtype=float) for k in ("P", "q", "M", "c", "A", "b")}
    contra["M"][0], contra["c"][0] = np.eye(n)[0], -1.0
    contra["M"][1], contra["c"][1] = -np.eye(n)[0], 0.0
    unb = {k: np.array(qp[k], dtype=float) for k in ("P", "q", "M", "c", "A", "b")}
    unb["P"][:], unb["M"][:], unb["c"][:], unb["q"][:] = 0.0, 0.0, 1.0, 1.0
    unb["A"][:], unb["b"][:] = 0.0, 0.0
    unb["A"][0, 0] = unb["A"][1, 1] = 1.0  # x_0 = x_1 = 0; the other four run off along -q
    nan = {k: np.array(qp[k], dtype=float) for k in ("P", "q", "M", "c", "A", "b")}
    nan["q"][2] = np.nan
    return [pack(contra), pack(unb), pack(nan)]


def parametric_qp():
    """n = 12 (91 probe points: two passes of k_qp_assemble_par's probe loop): a sum of squares of linear forms, 10 inequality and 2 equality
    rows, every coefficient a function of the parameters -- through products and atan2, the non-arithmetic node the expression layer has."""
    from conftest import SEED
    from optas_amd.builder import OptimizationBuilder
    from optas_amd.expr import atan2

    rng = np.random.default_rng(SEED + 12)
    n = 12
    builder = OptimizationBuilder(1)
    x = builder.add_decision_variables("x", n)
    p = builder.add_parameter("p", 4)
    g = [p[0], atan2(p[1], p[2]), p[0] * p[3], atan2(p[3], p[0]) * p[2]]

    def form(k):
        co = rng.integers(-8, 9, (n, 2)) / 4.0
        e = None
        for i in range(n):
            t = (g[(k + i) % 4] * float(co[i, 1]) + float(co[i, 0])) * x[i]
            e = t if e is None else e + t
        return e

    for k in range(14):
        builder.add_cost_term(f"form{k}", (form(k) - g[k % 4] * float(rng.integers(1, 9)) / 4.0) ** 2)
    for i in range(n):
        builder.add_cost_term(f"reg{i}", (0.5 * x[i] - 0.25 * g[i % 4]) ** 2)
    for r in range(10):
        builder.add_geq_inequality_constraint(f"row{r}", form(100 + r) * 0.25 + g[r % 4] * 0.125 + 0.25)
    for r in range(2):
        builder.add_equality_constraint(f"eq{r}", form(200 + r) * 0.25, g[(r + 1) % 4] * 0.0625)
    return builder.build()
