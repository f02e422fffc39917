"""The table of tests/locked_step_cases.py, checked without a GPU:

 1. the graded caps of a curvature are k, k + 1, k + 2, k = the first cap by which every instance has accepted a step (FIRST_CAP, re-measured here; 1 on
    most cases, 7 on four and five joints, whose every earlier trial lm_accept refuses): every case grades accepted steps, asserted;
 2. every linear solve that adds a step to a graded cap, under Gauss-Newton and under exact curvature, against oracle/blocktri_mp.py at 50 digits in
    two forms -- the reduced system and the saddle-point form without a null-space basis (beyond 65 free knots: the first graded system, reduced);
 3. the recorded errors and sensitivities (a factor 2), the on_system hook (every field of the result bit-identical with and without it), and the
    decision margins the GPU test relies on up to the last graded cap: no ratio test within 1e-3 of 1e-4, no retraction, convergence or polish test
    near its threshold, no Cholesky pivot within 1e-6 relative of zero, no reduced gradient near the hybrid switch, the port from a seed perturbed by
    a few ulp takes the same decisions, and its full solve ends at the same optimum after as many steps (max(2, 5 %));
 4. the compiled host port (oracle/cpu_port: the product's own eval_unit / couple_unit / step_instance<N, false> built for the host cores) on the
    7 and 6 joint chains at every horizon, by the rules of test_gpu_locked_steps.py (grade below).  A failure there is a finding in the product's state
    machine or in the port; the two found this way are in the port now (lm_accept's convergence test of a trial, eval_unit's polish tolerance).

Measured (2026-10-21), compiled port, largest |Q - Q_ref| / bound over the 19 cases of 7 and 6 joints: 0.36 (kuka7-plain-nK129, second graded cap,
Gauss-Newton); under exact curvature at most 0.03."""
import numpy as np
import pytest

import locked_step_cases as lc

_MEASURED = {}


@pytest.fixture(scope="module")
def robots_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("locked_step_robots")


def _measure(robots_dir, case):
    if case not in _MEASURED:
        _MEASURED[case] = lc.measure(robots_dir, case)
    return _MEASURED[case]


def _within_factor_2(measured, recorded):
    return measured == recorded or 0.5 * recorded <= measured <= 2.0 * recorded


def test_saddle_point_form_equals_the_reduced_form_on_a_small_system(robots_dir):
    """The two mp references against each other, where the step is known: Z z of the reduced system is the saddle-point form's d, and Jc d = 0."""
    c = lc.Case(robots_dir, ("kuka7", "plain", 3))
    _, recs = c.port_systems(0, 2, "exact")
    for r in recs[:2]:
        d_s = lc.saddle_step_mp(r, c.prob.kappa)
        d_r = np.einsum("tia,ta->ti", r["Z"][2:], lc.reduced_step_mp(r))
        assert np.abs(d_s - d_r).max() <= 1e-11 * max(1.0, np.abs(d_r).max())
        assert np.abs(np.einsum("tmi,ti->tm", r["Jc"][2:], d_s)).max() <= 1e-13 * max(1.0, np.abs(d_s).max())


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_port_steps_against_mp_and_the_conditions_of_the_table(robots_dir, case):
    m = _measure(robots_dir, case)
    assert m["ok"], m["why"]
    c = m["case"]
    print("%s: T %d, first caps %s, port |step - step_mp| %.2e (recorded %.2e), sensitivity %s (recorded %s), |step| %.3f, bounds %s, rejected %d, "
          "ratio gap %.1e, retraction %.5f, pivot %.1e, switch %.2f, full (status, steps, f, perturbed ...) %s"
          % (lc.case_id(case), c.T, m["first_cap"], m["port_err"], lc.PORT_STEP_ERR[case], ["%.2e" % s for s in m["sens"]], ["%.2e" % s for s in lc.SENS[case]], m["step_inf"],
             ["%.2e" % lc.bound(case, pos, m["step_inf"]) for pos in range(3)], m["rejected"], m["ratio_gap"], m["retract"], m["pivot"], m["switch"], m["full"]))
    assert m["hook_neutral"]
    assert tuple(m["first_cap"][h] for h in c.curvatures) == lc.FIRST_CAP[case]
    assert m["ratio_gap"] > lc.RATIO_GAP and m["retract"] >= lc.RETRACT_FACTOR and m["pivot"] >= lc.PIVOT_GAP and m["switch"] >= lc.SWITCH_FACTOR
    assert m["rows"] >= lc.ROWS_GAP, m["rows"]  # (vel: no velocity row within 1e-6 of changing sides; inf without rows)
    if c.variant == "vel" and c.nK > 1:
        assert m["wnext_values"] >= 2  # the coupling differs between intervals / joints: an off-by-one interval index changes the system
    assert _within_factor_2(m["port_err"], lc.PORT_STEP_ERR[case]), (m["port_err"], lc.PORT_STEP_ERR[case])
    for pos in range(3):
        assert _within_factor_2(m["sens"][pos], lc.SENS[case][pos]), (pos, m["sens"], lc.SENS[case])
        # the port's own solver is certified: inside the bound the tests grant the compiled port and the kernels
        assert m["port_err"] <= lc.bound(case, pos, m["step_inf"])


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_every_case_grades_an_accepted_step(robots_dir, case):
    """At the first graded cap of either curvature every instance has left the retracted seed: a sweep's step is in what is graded."""
    c = lc.Case(robots_dir, case)
    for h in c.curvatures:
        k = c.caps(h)[0]
        for i in range(lc.N_INST):
            r, seed = c.port(i, k, h), c.port(i, 0, h)["Q"]
            assert np.abs(r["Q"] - seed).max() > 1e-6  # (the count may pass k by a zero step: a polish is counted even at the cap), (lc.case_id(case), h, i, r["iters"], r["rejected"])
        if k > 1:  # ... and no earlier cap would do: some instance still sits on its seed
            assert any(np.abs(c.port(i, k - 1, h)["Q"] - c.port(i, 0, h)["Q"]).max() <= 1e-9 for i in range(lc.N_INST)), (lc.case_id(case), h)


@pytest.mark.parametrize("variant", ["plain", "vel"])
def test_a_case_has_a_rejected_step_inside_its_graded_caps(robots_dir, variant):
    case = lc.REJECTING[variant]
    assert case in lc.CASES and case[1] == variant
    assert _measure(robots_dir, case)["rejected"] > 0


@pytest.mark.parametrize("case", [k for k in lc.CASES if k[0] in ("kuka7", "kuka6") and k[1] == "plain"], ids=lc.case_id)
def test_compiled_port_at_every_horizon(robots_dir, case):
    import optas_amd
    from oracle import cpu_port

    cpu_port.build()
    c = lc.Case(robots_dir, case)
    refs = c.references()
    chain = optas_amd.RobotModel(urdf_filename=c.kin).kinematic_chain(c.link)
    x0 = np.concatenate([c.Q0.reshape(lc.N_INST, -1), np.zeros((lc.N_INST, c.n * (c.T - 1)))], 1)
    worst = {}
    for cap, curvature, mode in [(k, h, m) for h, m in (("gauss_newton", 0), ("exact", 1)) for k in c.caps(h)] + [("full", "hybrid", 2)]:
        x, f, kkt, iters, status = cpu_port.solve(chain, c.T, c.dt, c.prob.local_path, x0, c.qc, hessian=mode, tol=lc.TOL, tol_feas=lc.TOL_FEAS,
                                                  max_iter=c.max_iter_full if cap == "full" else cap, threads=1)
        tag = (lc.case_id(case), cap, curvature)
        for b in range(lc.N_INST):
            assert c.linear_rows(x[b], c.qc[b]) <= 1e-12, tag
        w = lc.grade(c, refs, cap, curvature, x[:, : c.n * c.T].reshape(lc.N_INST, c.T, c.n), f, iters, status, tag)
        if w is not None:
            worst[(cap, curvature)] = w
    print("%s: compiled port, |Q - Q_ref| / bound %s" % (lc.case_id(case), {k: "%.3f" % v for k, v in worst.items()}))
