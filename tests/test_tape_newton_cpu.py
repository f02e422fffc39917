"""Truncated Newton-CG on the tape family, CPU side: the float64 port of the merit's Hessian-vector product against the independent 60-digit reference,
and the numpy restatement of the state machine (tests/tape_newton_ref.py) on the IK goldens, planar IK and three tiny problems.  Needs no GPU."""
import os

import numpy as np
from scipy.optimize import minimize

import tape_hvp_ref as R
import tape_newton_ref as N
from conftest import GOLDEN
from oracle import tape_ref


def test_merit_hvp_port_against_the_mp_reference():
    """Dense generalised Hessian of the merit, column by column through hess_vec, on every composite case under rho = 1 and rho = 100, graded with
    tape_hvp_ref.within(.., DEVICE_TOL).  The GPU test grades the device on the cases kept here (36 of 36: none dropped, worst error 1.3e-15)."""
    kept, dropped = N.kept_merit_cases()
    n_act = n_inact = 0
    worst = 0.0
    for name, tp, x, p, lam, mu, rho in N.merit_cases():
        H, margin = N.merit_reference(name, rho)
        assert (np.abs(margin) >= N.MARGIN).all(), (name, rho, margin)  # float64 and mp agree on the active set
        with np.errstate(all="ignore"):
            f64 = lam - rho * tape_ref.forward(tp, x, p)[np.asarray(tp.out_rows, int)[: int(tp.n_ineq)]]
        assert ((f64 > 0) == (margin > 0)).all()
        n_act += int((margin > 0).sum())
        n_inact += int((margin < 0).sum())
        if (name, rho) not in [(d[0], d[1]) for d in dropped]:
            err = R.within(N.merit_hessian_port(tp, x, p, lam, mu, rho), H, R.DEVICE_TOL)[1]
            worst = max(worst, err)
            print(name, "rho", rho, "nx", int(tp.nx), "active", int((margin > 0).sum()), "inactive", int((margin < 0).sum()), "|H|", float(np.abs(H).max()), "error", err)
    print("kept", len(kept), "dropped", dropped, "worst kept error", worst)
    assert len(dropped) <= 2, dropped
    assert n_act >= 1 and n_inact >= 1, (n_act, n_inact)
    # one product along a random direction is the dense matrix times that direction
    name, tp, x, p, lam, mu, rho = next(c for c in kept if c[0] == "random3" and c[6] == 100.0)
    v = np.random.default_rng(4).uniform(-1.0, 1.0, int(tp.nx))
    assert R.within(N.merit_hvp_port(tp, x, p, lam, mu, rho, v), N.merit_reference(name, rho)[0] @ v, R.DEVICE_TOL)[0]


def _ik_tape():
    from examples.example import setup_solver as ik
    from optas_amd.tape import compile_problem

    return compile_problem(ik(build_only=True)[1])


def test_port_solves_the_ik_goldens():
    g = np.load(os.path.join(GOLDEN, "ik_golden.npz"))
    tp = _ik_tape()
    for i in (0, 5, 17):
        r = N.solve_tape_newton(tp, g["x0"][i], g["p"][i])
        b = tape_ref.solve_tape_al(tp, g["x0"][i], g["p"][i])
        print("instance", i, "evaluations", r["evals"], "steps", r["steps"], "products", r["hvps"], "BFGS evaluations", b["evals"])
        assert r["status"] == 0 and abs(r["f"] - g["f"][i]) < 1e-7 and np.abs(r["x"] - g["x"][i]).max() < 1e-4 and r["feas"] < 1e-9
        assert r["hvps"] <= r["steps"] * 7 + 7 and r["evals"] + r["hvps"] <= 2000


def test_port_solves_planar_ik():
    """From [pi / 2, 0, 0] the first full Newton step leaves the basin the BFGS path stays in: the solver ends, status 0, at ANOTHER local optimum of this
    non-convex problem (the other heading bound active, f = 40.47 against 5.96), after 169 evaluations and 183 products against 54 evaluations.  What is
    checked is what tests/test_tape.py checks of the BFGS port's point, less the identity of the active heading row: status, feasibility, and that SLSQP
    started there cannot improve on it."""
    from examples.planar_ik import setup_solver as planar
    from optas_amd.lowering import lower

    tp = lower(planar(build_only=True)[1])[1].tape
    x0, p = np.array([np.pi / 2, 0.0, 0.0]), np.zeros(0)
    r = N.solve_tape_newton(tp, x0, p)
    print("planar IK: evaluations", r["evals"], "steps", r["steps"], "products", r["hvps"], "f", r["f"], "x", r["x"])
    assert r["status"] == 0 and r["feas"] < 1e-9
    fun = lambda x: (lambda v: (v[tp.out_cost], tape_ref.reverse(tp, v, {tp.out_cost: 1.0})))(tape_ref.forward(tp, x, p))
    cons = [{"type": "ineq", "fun": lambda x: tape_ref.forward(tp, x, p)[tp.out_rows[: tp.n_ineq]]},
            {"type": "eq", "fun": lambda x: tape_ref.forward(tp, x, p)[tp.out_rows[tp.n_ineq :]]}]
    s = minimize(fun, r["x"], jac=True, method="SLSQP", constraints=cons, tol=1e-12, options={"maxiter": 200})
    assert s.success and abs(s.fun - r["f"]) < 1e-6 and np.abs(s.x - r["x"]).max() < 1e-4  # a local optimum


def test_port_on_the_three_tiny_problems():
    tiny = N.tiny_problems()
    tp, x0 = tiny["cos"]  # negative curvature at the start: the first direction is the gradient's, within unit length
    r = N.solve_tape_newton(tp, x0, np.zeros(0))
    assert r["status"] == 0 and abs(abs(r["x"][0]) - np.pi) < 1e-5 and abs(r["x"][1]) < 1e-5, r
    tp, x0 = tiny["rosenbrock"]
    r = N.solve_tape_newton(tp, x0, np.zeros(0))
    print("Rosenbrock: evaluations", r["evals"], "steps", r["steps"], "products", r["hvps"])
    assert r["status"] == 0 and np.abs(r["x"] - 1.0).max() < 1e-5, r
    tp, x0 = tiny["quartic"]  # singular Hessian at the optimum: linear convergence, no breakdown
    r = N.solve_tape_newton(tp, x0, np.zeros(0))
    assert r["status"] in (0, 1) and abs(r["x"][0] - 1.0) < 2e-2, r
    r = N.solve_tape_newton(tp, x0, np.zeros(0), max_iter=12)  # at the cap
    assert r["status"] == 1 and r["evals"] + r["hvps"] <= 13
