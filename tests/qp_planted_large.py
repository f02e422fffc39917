"""Planted dense QPs beyond n = 32, m = 256, me = 32: the sizes k_qp_solve_block (optas_amd/csrc/oh_qp_block.hip) alone serves, up to the
library's limits (128, 1024, 128).  The same dyadic-rational construction as qp_planted.make_qp (every datum exact in float64, the optimum
planted), with a class table, generator and errors() of its own: qp_planted.CLASSES is what the existing GPU test parametrises over and
stays as it is.

The seed of instance k of class number i is 50000 + 1000 i + k; 12 instances per class."""
import functools

import numpy as np

from qp_planted import TOL, _dy, assert_certificate, check_exact, kkt_certificate, pack  # noqa: F401  (re-exported for the tests)

LIMITS = (128, 1024, 128)  # OH_QP_MAX_N / _M / _ME
SMALL = (32, 256, 32)      # up to here the thread / wavefront kernels serve a handle

# name -> n, m, me, na (active rows: sigma = 0, lam* > 0); rank of P's symmetric part (default n); skew: a skew part is added to P
CLASSES = {
    "n33": dict(n=33, m=40, me=4, na=6),                 # first size beyond the old limit
    "n48_m257": dict(n=48, m=257, me=8, na=12),          # first m beyond
    "n64": dict(n=64, m=128, me=16, na=20),
    "n65_me33": dict(n=65, m=130, me=33, na=12),         # crosses 64 in n, first me beyond
    "me_eq_n_40": dict(n=40, m=12, me=40, na=0),         # me = n
    "vertex_48": dict(n=48, m=160, me=0, na=48, x_f_only=True),  # 48 x 48 active set, ill-conditioned: compare x, f and the certificate only
    "lp_eq_40": dict(n=40, m=120, me=8, na=32, rank=0),
    "rank_def_64": dict(n=64, m=160, me=8, na=40, rank=20),
    "nonsym_64": dict(n=64, m=128, me=16, na=20, skew=True),
    "n96": dict(n=96, m=512, me=48, na=30),
    "n128_max": dict(n=128, m=1024, me=64, na=40),
    "n128_me128": dict(n=128, m=64, me=128, na=0),
    "n128_inactive": dict(n=128, m=1024, me=128, na=0),
}
_SEED0 = {name: 50000 + 1000 * i for i, name in enumerate(CLASSES)}
N_INST = 12

# Port (oracle/qp_ipm.py) against the planted optimum on the 12 instances of each class: max |x - x*|, max |f - f*| / max(1, |f*|), max
# multiplier error (0 where the class does not compare multipliers).  Measured on the CPU (test_qp_large_cpu.py prints and re-checks them), not chosen.
PORT_ERR = {
    "n33": (1.627e-09, 3.136e-13, 6.515e-09),  # iters <= 15
    "n48_m257": (1.032e-09, 2.249e-13, 1.076e-08),  # iters <= 17
    "n64": (4.829e-10, 1.981e-13, 1.163e-08),  # iters <= 19
    "n65_me33": (4.707e-10, 1.721e-13, 1.256e-08),  # iters <= 17
    "me_eq_n_40": (5.240e-14, 4.565e-16, 5.384e-08),  # iters <= 11
    "vertex_48": (2.727e-09, 1.914e-12, 0.000e+00),  # iters <= 23
    "lp_eq_40": (3.922e-09, 5.046e-11, 8.103e-09),  # iters <= 29
    "rank_def_64": (2.772e-09, 1.398e-12, 1.613e-08),  # iters <= 29
    "nonsym_64": (4.256e-10, 2.899e-13, 9.408e-09),  # iters <= 19
    "n96": (3.011e-10, 2.066e-13, 3.755e-08),  # iters <= 21
    "n128_max": (3.354e-10, 1.158e-13, 6.977e-08),  # iters <= 21
    "n128_me128": (1.212e-13, 4.031e-16, 3.530e-08),  # iters <= 11
    "n128_inactive": (1.399e-13, 2.926e-16, 5.356e-07),  # iters <= 11
}
# the port's iteration count on each of the 12 instances
PORT_ITERS = {
    "n33": (14, 14, 13, 14, 13, 14, 14, 14, 15, 12, 14, 15),
    "n48_m257": (17, 17, 14, 16, 14, 16, 17, 17, 17, 17, 14, 15),
    "n64": (17, 19, 17, 17, 16, 18, 17, 17, 15, 15, 19, 16),
    "n65_me33": (13, 17, 15, 16, 15, 14, 16, 15, 14, 17, 16, 16),
    "me_eq_n_40": (10, 11, 11, 11, 10, 11, 11, 11, 11, 11, 11, 11),
    "vertex_48": (20, 18, 23, 20, 20, 22, 20, 22, 21, 20, 20, 23),
    "lp_eq_40": (24, 22, 29, 25, 27, 28, 26, 23, 23, 29, 26, 26),
    "rank_def_64": (22, 26, 28, 29, 25, 22, 24, 21, 24, 26, 25, 28),
    "nonsym_64": (19, 18, 16, 18, 17, 17, 18, 16, 19, 18, 16, 17),
    "n96": (21, 17, 17, 17, 18, 17, 16, 19, 18, 19, 17, 17),
    "n128_max": (19, 19, 20, 20, 19, 19, 19, 21, 20, 19, 19, 20),
    "n128_me128": (11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11),
    "n128_inactive": (11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11),
}
MARGIN = 10.0
# A point is accepted at KKT residual <= TOL = 1e-9: errors below that carry no information about the kernel (the equality-only classes sit
# at 1e-14), so the bounds are floored at TOL / 10 for x and f and at 1e-8 for the multipliers.
FLOOR = (TOL / 10.0, TOL / 10.0, 1e-8)


def bound(name):
    return tuple(max(MARGIN * v, fl) for v, fl in zip(PORT_ERR[name], FLOOR))


def is_large(n, m, me):
    return n > SMALL[0] or m > SMALL[1] or me > SMALL[2]


def make_qp(name, seed):
    a = CLASSES[name]
    n, m, me, na = a["n"], a["m"], a["me"], a["na"]
    rank = a.get("rank", n)
    rng = np.random.default_rng(seed)
    G = _dy(rng, (n, rank))
    Ps = 0.5 * (G @ G.T) + (np.eye(n) / 8.0 if rank == n else 0.0)
    M, A = _dy(rng, (m, n)), _dy(rng, (me, n))
    xs, nus = _dy(rng, n), _dy(rng, me)
    act = np.sort(rng.choice(m, na, replace=False))
    lam = np.zeros(m)
    sig = _dy(rng, m, 0.125, 4.0)
    lam[act] = _dy(rng, na, 0.125, 4.0)
    sig[act] = 0.0
    K = np.zeros((n, n))
    if a.get("skew"):
        U = np.triu(_dy(rng, (n, n), -2.0, 2.0), 1)
        K = U - U.T
    P = Ps + K
    q = -(P + P.T) @ xs + M.T @ lam + A.T @ nus
    c = sig - M @ xs
    b = -A @ xs
    f = float(xs @ P @ xs + q @ xs)
    return dict(name=name, n=n, m=m, me=me, G=G, K=K, P=P, q=q, M=M, c=c, A=A, b=b, x=xs, lam=lam, nu=nus, sigma=sig, f=f, act=act)


@functools.lru_cache(maxsize=None)
def planted_instances(name):
    """The N_INST instances of a class (fixed seeds), the ones the port's errors are recorded on.  Shared: leave unchanged."""
    return tuple(make_qp(name, _SEED0[name] + k) for k in range(N_INST))


def planted_batch(name, B):
    """Instance i of the batch is instance i % N_INST of the class."""
    qps = planted_instances(name)
    return [qps[i % N_INST] for i in range(B)]


def errors(qp, x, f, lam, nu):
    """(max |x - x*|, |f - f*| / max(1, |f*|), multiplier error); the multiplier error is 0 for a class that compares x and f only."""
    ex = float(np.abs(np.asarray(x) - qp["x"]).max())
    ef = abs(float(f) - qp["f"]) / max(1.0, abs(qp["f"]))
    if CLASSES[qp["name"]].get("x_f_only"):
        return ex, ef, 0.0
    em = max(float(np.abs(np.asarray(lam) - qp["lam"]).max(initial=0.0)), float(np.abs(np.asarray(nu) - qp["nu"]).max(initial=0.0)))
    return ex, ef, em


@functools.lru_cache(maxsize=None)
def port_results(name):
    """The port on the 12 instances of a class: (worst errors (3,), iteration counts (12,), statuses (12,)).  Shared: leave unchanged."""
    from oracle.qp_ipm import solve_qp_ipm

    worst, its, sts = np.zeros(3), [], []
    for qp in planted_instances(name):
        r = solve_qp_ipm(qp["P"], qp["q"], qp["M"], qp["c"], qp["A"], qp["b"])
        worst = np.maximum(worst, errors(qp, r["x"], r["f"], r["lam"], r["nu"]))
        its.append(int(r["iters"]))
        sts.append(int(r["status"]))
    return worst, tuple(its), tuple(sts)


def mpc_problem():
    """Linear MPC over a horizon of 12 for a 3-D task model with position and velocity states: Euler rows, the position pinned to the parameter
    y0 and the velocity to zero, both states within their limits; cost 10 |y_T - goal|^2 + 0.1 |dY|^2.
    QuadraticCostLinearConstraints with nx = 72, nk = 144, na = 39, parameters [y0 (3) | goal (3)]."""
    import optas_amd as optas
    from optas_amd.builder import OptimizationBuilder
    from optas_amd.expr import sumsqr

    task = optas.TaskModel("mpc", 3, time_derivs=[0, 1], dlim={0: [-2, 2], 1: [-0.5, 0.5]})
    b = OptimizationBuilder(12, tasks=[task], derivs_align=True)
    y0, goal = b.add_parameter("y0", 3), b.add_parameter("goal", 3)
    b.integrate_model_states("mpc", 1, 0.5)
    b.fix_configuration("mpc", y0)
    b.fix_configuration("mpc", np.zeros(3), time_deriv=1)
    b.enforce_model_limits("mpc", time_deriv=0)
    b.enforce_model_limits("mpc", time_deriv=1)
    Y, dY = b.get_model_states("mpc"), b.get_model_states("mpc", time_deriv=1)
    b.add_cost_term("goal", 10.0 * sumsqr(Y[:, -1] - goal))
    b.add_cost_term("vel", 0.1 * sumsqr(dY))
    return b.build()


def mpc_parameters(rng, B):
    """y0 in U(-0.3, 0.3)^3, goal in U(-1, 1)^3 * (3.5, 1, 3.5): the first and third coordinates can ask for more than the velocity limit allows."""
    return np.hstack([rng.uniform(-0.3, 0.3, (B, 3)), rng.uniform(-1.0, 1.0, (B, 3)) * np.array([3.5, 1.0, 3.5])])
