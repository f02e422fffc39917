"""The rules of the point-mass iteration (optas_amd/csrc/oh_pm_rules.h, called by k_pm_solve and k_pm_solve_wave of oh_pointmass.hip) held to the bits
of the two kernel texts of the commit before (profiles/pm_one_text_pieces.json: what moved them, and stays written out).  tests/golden/pm_parent_bits.npz was written on an MI355X by the library of the last commit in which each
kernel spelled the iteration out by itself, through pm_outputs() below (tools/gpu_pm_ab_dump.py pin).  Outputs only; the inputs come from the seeds
and from tests/golden/pm_steps_mp.npz.  Equality of every array as integers.

The option max_iter = 0 of the handle selects the default of 100 (oh_create_pointmass), so the evaluation-only exit of the kernels cannot be reached
through PointMassBackend: the cap cell runs at 0 (the default) and at 1, the shortest capped solve."""
import os

import numpy as np
import pytest

import pm_edge_cases as pe
from conftest import GOLDEN

gen = pe.gen
PATHS = (("thread", 0.0), ("wave", 20480.0))
OUT = ("x", "f", "kkt", "iters", "status")
ROLL_OUT = ("states", "f", "iters", "status")
CONVERGED, MAX_ITER, NUMERICAL, INFEASIBLE = 0, 1, 2, 3  # OH_STATUS_*
T_BENCH, B_BENCH = 20, 70  # the benchmark's horizon; a block of 64 threads and a partly filled second one
# position in the batch of 70 -> what is wrong with the instance
NAN_GOAL, NAN_OBSTACLE, OBSTACLE_LANDS, START_INSIDE = 3, 40, 64, 69
CAP_CELL = ("mpc", 5)
LOOP = dict(T=20, B=65, n_ticks=3, advance=2, ramp=0.032)


def _bench_batch():
    x0, p = pe.filler(T_BENCH, gen.options("mpc", T_BENCH)["dt"], B_BENCH, seed=2)
    T = T_BENCH
    p[NAN_GOAL, 4 + 2 * 1 + 1] = np.nan
    p[NAN_OBSTACLE, 4 + 2 * T + 2 * (T - 1)] = np.nan
    # test_obstacle_landing_on_the_mass_at_a_later_knot_is_reported_infeasible: the obstacle far away, except at knot 3, where it sits on the start
    p[OBSTACLE_LANDS, 2:4] = 0.0
    p[OBSTACLE_LANDS, 4 + 2 * T :] = 5.0
    p[OBSTACLE_LANDS, 4 + 2 * T + 2 * 3 : 4 + 2 * T + 2 * 3 + 2] = p[OBSTACLE_LANDS, 0:2]
    p[START_INSIDE, 4 + 2 * T : 4 + 2 * T + 2] = p[START_INSIDE, 0:2]
    return x0, p


def pm_cases():
    """[(key, "solve", variant, T, max_iter, pm_wave_max, x0, p)] and [(key, "rollout", T, pm_wave_max, state0, obstacle table)]"""
    fixture = np.load(os.path.join(GOLDEN, "pm_steps_mp.npz"))
    cases = []
    for variant, T in gen.cells():
        ids = [gen.case_id(variant, T, s) for s in range(gen.N_SLOTS)]
        x0, p = (np.stack([fixture[i + "_" + k] for i in ids]) for k in ("x0", "p"))
        # the iteration cap: 1 is the smallest the handle takes (one step, then the evaluation that ends at the cap); 0 selects the default of 100
        for max_iter in (2, pe.MAX_ITER) + ((0, 1) if (variant, T) == CAP_CELL else ()):
            for path, wave_max in PATHS:
                cases.append(("%s/T%d/it%d/%s" % (variant, T, max_iter, path), "solve", variant, T, max_iter, wave_max, x0, p))
    x0, p = _bench_batch()
    for path, wave_max in PATHS:
        cases.append(("bench/T%d/B%d/%s" % (T_BENCH, B_BENCH, path), "solve", "mpc", T_BENCH, pe.MAX_ITER, wave_max, x0, p))
    tab = pe.obstacle_table(LOOP["n_ticks"] * LOOP["advance"] + LOOP["T"], gen.options("mpc", LOOP["T"])["dt"])
    for path, wave_max in PATHS:
        cases.append(("loop/T%d/B%d/%s" % (LOOP["T"], LOOP["B"], path), "rollout", LOOP["T"], wave_max, pe.rollout_starts(LOOP["B"]), tab))
    return cases


def pm_outputs(cases):
    """{key/output: array} through PointMassBackend only."""
    from optas_amd.backend import PointMassBackend

    out = {}
    for case in cases:
        key, kind = case[:2]
        variant, T, max_iter, wave_max = (case[2:6]) if kind == "solve" else ("mpc", case[2], pe.MAX_ITER, case[3])
        o = gen.options(variant, T)
        be = PointMassBackend(T=T, dt=o["dt"], w_acc=o["w_acc"], ylim=gen.YLIM, vlim=gen.VLIM, safe=gen.SAFE, max_iter=max_iter, tol=gen.TOL,
                              track_final_only=o["track_final_only"], w_vel=o["w_vel"], fix_final_velocity=o["fix_final_velocity"])
        try:
            be.set_options(pm_wave_max=wave_max)
            if kind == "solve":
                r = be.solve(case[6], case[7])
                got = {k: getattr(r, k) for k in OUT}
            else:
                got = dict(zip(ROLL_OUT, be.rollout(case[4], case[5], LOOP["n_ticks"], LOOP["advance"], LOOP["ramp"])))
        finally:
            be.close()
        for name, a in got.items():
            out["%s/%s" % (key, name)] = np.ascontiguousarray(a)
    return out


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def check_pinned(ref, cases):
    """What the cases are there for happens in the pinned runs: both kernels, every exit of the iteration, a pinned stage and a free one."""
    keys = {c[0] for c in cases}
    differ_on_lanes = False
    for variant, T in gen.cells():
        for max_iter in (2, pe.MAX_ITER):
            xt, xw = (_bits(ref["%s/T%d/it%d/%s/x" % (variant, T, max_iter, path)]) for path, _ in PATHS)
            if T > 64:
                assert (xt == xw).all(), (variant, T, max_iter)  # no lane per knot beyond 64: both settings run k_pm_solve
            else:
                differ_on_lanes = differ_on_lanes or bool((xt != xw).any())
    assert differ_on_lanes  # the two kernels place their fused multiply-adds differently: equal bits everywhere would mean one kernel ran twice
    seen = set()
    for k in keys:
        seen |= set(ref[k + "/status"].reshape(-1).tolist())
    assert {CONVERGED, MAX_ITER, NUMERICAL, INFEASIBLE} <= seen, seen
    fixes = {bool(gen.VARIANTS[c[2]][4]) for c in cases if c[1] == "solve" and c[3] >= 3}
    assert fixes == {True, False}
    clean = np.delete(np.arange(B_BENCH), [NAN_GOAL, NAN_OBSTACLE, OBSTACLE_LANDS, START_INSIDE])
    for path, _ in PATHS:
        st = ref["bench/T%d/B%d/%s/status" % (T_BENCH, B_BENCH, path)]
        assert (st[clean] == CONVERGED).all(), (path, st)
        assert (st[[NAN_GOAL, NAN_OBSTACLE]] == NUMERICAL).all() and (st[[OBSTACLE_LANDS, START_INSIDE]] == INFEASIBLE).all(), (path, st)
        cap = "%s/T%d/it%%d/%s" % (CAP_CELL + (path,))
        assert (ref[cap % 1 + "/iters"] == 1).all() and (ref[cap % 1 + "/status"] == MAX_ITER).all()
        assert (ref[cap % 0 + "/iters"] > 2).all() and (ref[cap % 0 + "/status"] == CONVERGED).all()  # (oh_create_pointmass: max_iter <= 0 is the default)
        assert (ref["loop/T%d/B%d/%s/status" % (LOOP["T"], LOOP["B"], path)] == CONVERGED).mean() >= 0.9


@pytest.mark.gpu
def test_shared_rules_have_the_bits_of_the_texts_they_replaced(hip_lib):
    ref = np.load(os.path.join(GOLDEN, "pm_parent_bits.npz"))
    cases = pm_cases()
    check_pinned(ref, cases)
    got = pm_outputs(cases)
    assert sorted(got) == sorted(ref.files)
    differ = []
    for key in ref.files:
        if got[key].dtype != ref[key].dtype or got[key].shape != ref[key].shape or not (_bits(got[key]) == _bits(ref[key])).all():
            differ.append(key)
    print("arrays", len(ref.files), "differing", differ)
    assert not differ, differ
