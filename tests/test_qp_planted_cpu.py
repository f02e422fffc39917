"""Planted QPs (tests/qp_planted.py) on the CPU: the construction is exact, the numpy port (oracle/qp_ipm.py) reaches every planted optimum --
the errors it leaves are the reference errors the GPU bounds of tests/test_gpu_qp_planted.py are set from -- and the chosen sizes reach every
launch path of oh_launch_qp_solve."""
import numpy as np
import pytest

import qp_planted as Q
from oracle.qp_ipm import solve_qp_ipm


@pytest.mark.parametrize("name", list(Q.CLASSES))
def test_planted_data_is_exact(name):
    qps = Q.planted_instances(name)
    Q.check_exact(qps[0])
    a = Q.CLASSES[name]
    for qp in qps:  # the class's properties hold for every instance
        assert (qp["sigma"] == 0).sum() == a["na"] and (qp["lam"] > 0).sum() == a["na"] - (1 if a.get("weak") else 0)
        assert np.linalg.matrix_rank(0.5 * (qp["P"] + qp["P"].T)) == a.get("rank", a["n"])
        assert np.linalg.matrix_rank(qp["A"]) == a["me"] if a["me"] else True
        if a["m"] > 64 and a["na"]:
            assert qp["act"].max() >= 64
    if a.get("skew"):
        base = Q.planted_instances("base")
        assert all(np.abs(qp["K"]).max() > 0 and (qp["K"] == -qp["K"].T).all() and (qp["P"] - qp["K"] == b["P"]).all() and (qp["x"] == b["x"]).all()
                   and (qp["q"] == b["q"]).all() and qp["f"] == b["f"] for qp, b in zip(qps, base))
    if a.get("big"):
        assert all((qp["sigma"] == Q.BIG).sum() == a["big"] for qp in qps)
    if a.get("dup"):
        assert all((qp["M"][0] == qp["M"][1]).all() and qp["c"][0] == qp["c"][1] for qp in qps)


@pytest.mark.parametrize("name", list(Q.CLASSES))
def test_port_reaches_the_planted_optimum(name):
    worst = np.zeros(3)
    for qp in Q.planted_instances(name):
        r = solve_qp_ipm(qp["P"], qp["q"], qp["M"], qp["c"], qp["A"], qp["b"])
        assert r["status"] == 0 and r["iters"] <= 40
        worst = np.maximum(worst, Q.errors(qp, r["x"], r["f"], r["lam"], r["nu"]))
    print(f"{name}: port max |x - x*| {worst[0]:.3e}  rel |f - f*| {worst[1]:.3e}  multipliers {worst[2]:.3e}  (recorded {Q.PORT_ERR[name]})")
    # the recorded figures are this measurement; another BLAS may associate sums differently, so the port is held to what the kernels are held to
    assert (worst <= np.array(Q.bound(name))).all()


def test_port_certificate_and_reported_residuals():
    """kkt_certificate on the port's own output: what the GPU test asserts of the kernels holds for the iteration on the CPU."""
    for name in ("base", "nonsym", "big_rows", "lp_eq"):
        qp = Q.planted_instances(name)[17]
        r = solve_qp_ipm(qp["P"], qp["q"], qp["M"], qp["c"], qp["A"], qp["b"])
        Q.assert_certificate(Q.kkt_certificate(qp, r["x"], r["lam"], r["nu"]), r["kkt"])
    # and it tells a wrong point from a right one
    cert = Q.kkt_certificate(qp, r["x"] + 1e-6, r["lam"], r["nu"])
    with pytest.raises(AssertionError):
        Q.assert_certificate(cert)


def test_asymmetric_p_regression():
    """x^T P x has the gradient (P + P^T) x: with the residual 2 P x + q the iteration stopped, status CONVERGED, up to 1.2 away from x*."""
    bx = Q.bound("base")[0]
    for qp, base in zip(Q.planted_instances("nonsym"), Q.planted_instances("base")):
        r = solve_qp_ipm(qp["P"], qp["q"], qp["M"], qp["c"], qp["A"], qp["b"])
        assert r["status"] == 0 and np.abs(r["x"] - qp["x"]).max() <= bx
        s = solve_qp_ipm(base["P"], base["q"], base["M"], base["c"], base["A"], base["b"])
        assert s["iters"] == r["iters"] and np.abs(s["x"] - r["x"]).max() <= bx  # only the symmetric part of P enters


def test_sizes_reach_every_launch_path():
    seen = set()
    for name, a in Q.CLASSES.items():
        n, m, me = a["n"], a["m"], a["me"]
        for B in Q.GPU_BATCHES:
            p = Q.launch_path(n, m, me, B, -1)
            seen.add(("auto",) + p[:2] + ((m > 64,) if p[0] == "wave" else ()))
        for mode in (0, 1, 2):
            if Q.forced_fits(n, m, me, mode):
                seen.add(("forced", "thread", mode))
    for mode in (0, 1, 2):
        assert ("auto", "thread", mode) in seen and ("forced", "thread", mode) in seen
    assert ("auto", "wave", 64, False) in seen and ("auto", "wave", 64, True) in seen
    # the selection itself, at sizes worked out by hand from oh_launch_qp_solve: 6/10/2 has np = 126, nwork = 120
    assert Q.qp_sizes(6, 10, 2) == (126, 120)
    assert Q.launch_path(6, 10, 2, 70) == ("thread", 2, 16) and Q.launch_path(6, 10, 2, 70, 1) == ("thread", 1, 32)
    assert Q.launch_path(6, 10, 2, 64) == ("wave", 64) and Q.launch_path(6, 10, 2, 65) == ("thread", 2, 16) and Q.launch_path(6, 10, 2, 64, 0) == ("thread", 0, 64)
    assert Q.launch_path(32, 256, 32, 64) == ("thread", 0, 64) and not Q.forced_fits(32, 256, 32, 1)  # 10560 + 3232 doubles: no wavefront, no LDS
    assert Q.launch_path(7, 16, 3, 70) == ("thread", 1, 32)  # 177 + 208 = 385 doubles: one too many for 16 instances with their rows


def test_bad_instances_are_not_solved_by_the_port():
    """(CPU statement of what the isolation test plants: the iteration itself gives these up.)"""
    from oracle.qp_ipm import solve_qp_ipm

    qp = Q.planted_instances("base")[0]
    n, m, me = qp["n"], qp["m"], qp["me"]
    for row in Q.bad_instances(qp):
        o = np.cumsum([0, n * n, n, m * n, m, me * n, me])
        P, q, M, c, A, b = (row[o[i]:o[i + 1]] for i in range(6))
        with np.errstate(all="ignore"):
            assert solve_qp_ipm(P.reshape(n, n), q, M.reshape(m, n), c, A.reshape(me, n), b)["status"] != 0


def test_parametric_qp_is_a_quadratic_program():
    from optas_amd.lowering import lower
    from optas_amd.optimization import QuadraticCostLinearConstraints

    o = Q.parametric_qp()
    assert isinstance(o, QuadraticCostLinearConstraints) and (o.nx, o.np, o.nk, o.na) == (12, 4, 10, 2)
    assert 1 + 2 * o.nx + o.nx * (o.nx - 1) // 2 > 64
    _, spec = lower(o)
    assert (spec.n, spec.m, spec.me) == (12, 10, 2)
    p = np.array([0.75, 1.25, 0.5, 1.0])
    P = o.P(p)
    assert np.abs(P - P.T).max() == 0.0 and np.linalg.eigvalsh(P).min() > 0.2
