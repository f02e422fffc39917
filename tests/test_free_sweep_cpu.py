"""The table of tests/free_sweep_cases.py, checked without a GPU: every linear solve of the numpy port's first three iterations (the first only from
108 free knots on) against oracle/blocktri_mp.py at 50 digits, the recorded errors and sensitivities, and the conditions the GPU test
(test_gpu_free_sweeps.py) relies on:

 1. the port accepts its first step on every instance, so max_iter = 1 returns seed + z;
 2. in every variant some case has a rejected step in iterations 2-3 (mu > 0: the sweeps' damping branch runs);
 3. no acceptance ratio of the first three iterations lies within 1e-3 of the 1e-4 threshold;
 4. no inequality row of the first three evaluations has |lam - rho g| < 1e-6 (an active-set flip between two roundings is another system).

The on_system hook must leave the port's results bit-identical."""
import numpy as np
import pytest

import free_sweep_cases as fc
from oracle.blocktri_mp import solve_mp
from oracle.structured import block_tridiag_solve

_MEASURED = {}


@pytest.fixture(scope="module")
def robots_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("free_sweep_robots")


def _measure(robots_dir, case):
    if case not in _MEASURED:
        _MEASURED[case] = fc.measure(robots_dir, case)
    return _MEASURED[case]


def test_solve_mp_on_a_dense_system():
    """The reference itself: full coupling blocks, a shift, against numpy on the assembled matrix; the residual check refuses a wrong answer's system."""
    rng = np.random.default_rng(5)
    N, m, mu = 5, 4, 0.3
    A = rng.normal(size=(N, m, m))
    D = np.einsum("tij,tkj->tik", A, A) + np.eye(m)
    E = 0.3 * rng.normal(size=(N - 1, m, m))
    rhs = rng.normal(size=(N, m))
    K = np.zeros((N * m, N * m))
    for t in range(N):
        K[t * m : (t + 1) * m, t * m : (t + 1) * m] = D[t] + mu * np.eye(m)
        if t < N - 1:
            K[t * m : (t + 1) * m, (t + 1) * m : (t + 2) * m] = E[t]
            K[(t + 1) * m : (t + 2) * m, t * m : (t + 1) * m] = E[t].T
    z, z_mp, res = solve_mp(D, E, rhs, mu)
    assert res <= 1e-40 and np.abs(z - np.linalg.solve(K, rhs.reshape(-1)).reshape(N, m)).max() <= 1e-13
    zp, ok = block_tridiag_solve(D, E, rhs, mu)
    assert ok and np.abs(z - zp).max() <= 1e-13
    D[2] -= 4.0 * np.eye(m)  # indefinite: the general inverse takes over, the port's Cholesky gives up
    z2 = solve_mp(D, E, rhs, mu)[0]
    K[2 * m : 3 * m, 2 * m : 3 * m] -= 4.0 * np.eye(m)
    assert np.abs(z2 - np.linalg.solve(K, rhs.reshape(-1)).reshape(N, m)).max() <= 1e-12 and not block_tridiag_solve(D, E, rhs, mu)[1]
    z1 = solve_mp(D[:1], E[:0], rhs[:1], mu)[0]  # a single knot
    assert np.abs(z1[0] - np.linalg.solve(D[0] + mu * np.eye(m), rhs[0])).max() <= 1e-13


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_port_steps_against_mp_and_the_conditions_of_the_table(robots_dir, case):
    m = _measure(robots_dir, case)
    c = m["case"]
    rec_err, rec_sens = fc.PORT_STEP_ERR[case], fc.SENS[case]
    print("%s: T %d, port |z - z_mp| %.2e (recorded %.2e), sensitivity %.2e (recorded %.2e), |z| %.3f, bound %.2e, coupling values %d, damped (instance, "
          "iteration, mu) %s, rejected %d" % (fc.case_id(case), c.T, m["port_err"], rec_err, m["sens"], rec_sens, m["z1_inf"], fc.bound(case, m["z1_inf"]),
                                              m["n_coupling"], m["damped"], m["rejected"]))
    assert m["hook_neutral"]
    assert m["first_accepted"] and m["cap1_err"] <= 1e-15, m["cap1_err"]  # (1)
    assert m["ratio_gap"] > 1e-3, m["ratio_gap"]  # (3)
    assert m["rows_gap"] >= 1e-6, m["rows_gap"]  # (4)
    # the recorded numbers are this measurement (the port's error is rounding noise of numpy's factorisation: a factor 2 either way; the sensitivity is
    # an exact solution's answer to a fixed perturbation)
    assert 0.5 * rec_err <= m["port_err"] <= 2.0 * rec_err, (m["port_err"], rec_err)
    assert abs(m["sens"] - rec_sens) <= 0.05 * rec_sens, (m["sens"], rec_sens)
    # the port's own solver is certified: inside the bound the GPU test grants the kernels
    assert m["port_err"] <= fc.bound(case, m["z1_inf"])
    if c.variant == "vel" and c.nK > 1:
        assert m["n_coupling"] >= 2  # the coupling differs between intervals / joints: an off-by-one interval index changes the system


@pytest.mark.parametrize("variant", ["plain", "guarded", "vel"])
def test_every_variant_has_a_case_with_a_rejected_step(robots_dir, variant):
    """(2): the case named in REJECTING has a rejected step in iterations 2-3 and solves with mu > 0 after it."""
    case = fc.REJECTING[variant]
    assert case[1] == variant and case in fc.CASES
    m = _measure(robots_dir, case)
    assert m["rejected"] > 0 and any(it in (1, 2) and mu > 0.0 for _, it, mu in m["damped"]), (m["rejected"], m["damped"])
