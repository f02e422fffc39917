"""Both kernels of the point-mass family (csrc/oh_pointmass.hip: k_pm_solve, one thread per plant; k_pm_solve_wave, one wavefront per plant and one lane
per knot) at the horizon edges T = 2, 3, 4, 5, 63, 64, 65, in four variants: the MPC tick, the planner (track_final_only, w_vel, fix_final_velocity),
and the two crossed settings.  Every solve goes through PointMassBackend; option pm_wave_max = 0 selects the thread kernel, 20480 the wave kernel where
T <= 64, and at T = 65 both settings must give the thread kernel's answer bit for bit.

(a) Truncated iterations (max_iter = 1, 2, 3) against tests/golden/pm_steps_mp.npz: the state machine at 50 digits with Newton directions from a dense
    solve of the condensed system (tests/pm_step_ref.py), no Riccati recursion.  The tolerance per case and quantity is measured, not chosen: 64 times
    the numpy port's recorded distance from mp, floored at 1e-13 max(1, |reference|_inf).  Port and kernels are three float64 executions of one
    recursion in different rounding orders (Cholesky with divisions there, rsqrt and compiler-placed FMAs here); their errors scale alike with the
    condition number of the condensed Hessian (up to 2e5 at T = 63 .. 65); 64 is room for a rounding order, not for a wrong term.  Knot 0 of x equals
    (curr, dcurr) exactly, the Euler rows hold to 1e-13.
    Largest observed ratios, device distance over max(port distance, floor / 64), limit 64:  thread kernel 3.9 (stat, fix_final_velocity alone,
    T = 63, k = 3),  wave kernel 6.3 (compl, MPC, T = 64, k = 3); at T <= 5 both stay below 1.2.
    Largest device distance from mp in x:  5.4e-14 on either kernel (planner, T = 65, where both run k_pm_solve); the port's: 7.8e-14.
(b) Full solves (tol 1e-8, max_iter 200), 8 instances per cell, against the port: equal status and iteration counts, f to 1e-8 relative (the other
    point-mass modules' figure), kkt <= tol, wave against thread 1e-10 in x and kkt and 1e-11 relative in f (the T = 20 test's figures), and for the MPC
    and planner variants the reference-form KKT check on PointMassMPCNLP(T) / PointMassPlannerNLP(T) at test_gpu_pointmass.py's thresholds.  The
    instances (tests/pm_edge_cases.py) keep the port's last evaluation at <= 0.5 tol and the one before at >= 2 tol; asserted here from the port's run.
(c) Batch placement: an instance's x, f, kkt, iters and status are the same bits at positions 0, 62, 63, 64, B - 1 of batches of 1, 63, 64, 65, 129 (thread
    kernel, rows [row][b] of stride Bp) and of 1, 65 (wave kernel), on one handle that grows to 129 and comes back to 63.
(d) Non-finite inputs in a batch of 6 with finite neighbours, T = 3 and 64: NaN in curr, in a goal entry of knot 1 and of knot T - 1, in an obstacle entry
    of knot T - 1 or of knot 0, inf in a goal entry end at OH_STATUS_NUMERICAL with the same iteration count on both paths; NaNs where no kernel reads
    (the Y block of x0, its dY block at knot 0, and at knot T - 1 under fix_final_velocity) change no bit.  Neighbours keep their bits.
    (The thread kernel used to find a NaN obstacle entry one evaluation late, after a step with a NaN direction: its maxima drop NaNs.)
(e) oh_pm_rollout with B = 65, 3 ticks, the largest advance (T = 3: 2, T = 64: 63) against a host loop of solves: states 1e-9, f 1e-10 (the rollout test's
    figures), equal statuses and iteration counts."""
import os

import numpy as np
import pytest

import pm_edge_cases as pe
from conftest import GOLDEN
from optas_amd import _lib
from optas_amd.backend import PointMassBackend
from oracle.problems import PointMassMPCNLP, PointMassPlannerNLP
from oracle.solvers import kkt_reference_form

gen = pe.gen
pytestmark = pytest.mark.gpu

PATHS = (("thread", 0.0), ("wave", 20480.0))
FACTOR, FLOOR = 64.0, 1e-13


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "pm_steps_mp.npz"))


def _backend(variant, T, max_iter, wave_max):
    o = gen.options(variant, T)
    be = PointMassBackend(T=T, dt=o["dt"], w_acc=o["w_acc"], ylim=gen.YLIM, vlim=gen.VLIM, safe=gen.SAFE, max_iter=max_iter, tol=gen.TOL,
                          track_final_only=o["track_final_only"], w_vel=o["w_vel"], fix_final_velocity=o["fix_final_velocity"])
    return be.set_options(pm_wave_max=wave_max)


def _solve(variant, T, max_iter, wave_max, x0, p):
    be = _backend(variant, T, max_iter, wave_max)
    r = be.solve(x0, p)
    be.close()
    return r


def _cell(fixture, variant, T):
    ids = [gen.case_id(variant, T, s) for s in range(gen.N_SLOTS)]
    return {k: np.stack([fixture[i + "_" + k] for i in ids]) for k in ("x0", "p", "x", "f", "kkt", "dist")}


def _same_bits(a, b):
    return all(getattr(a, k).shape == getattr(b, k).shape and getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ("x", "f", "kkt", "iters", "status"))


def _linear_rows(T, dt, x, p):
    Y, V = x[:, : 2 * T].reshape(-1, T, 2), x[:, 2 * T :].reshape(-1, T, 2)
    assert np.array_equal(Y[:, 0], p[:, 0:2]) and np.array_equal(V[:, 0], p[:, 2:4])
    assert np.abs(Y[:, 1:] - (Y[:, :-1] + dt * V[:, :-1])).max() <= 1e-13


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,T", gen.cells(), ids=lambda v: str(v))
def test_truncated_iterations_against_mp(hip_lib, fixture, variant, T):
    c = _cell(fixture, variant, T)
    dt = gen.options(variant, T)["dt"]
    worst = {name: [0.0, 0.0, None] for name, _ in PATHS}  # ratio, |x - x_mp|, where
    failures = []
    for n, k in enumerate(gen.KS):
        got = {name: _solve(variant, T, k, wave_max, c["x0"], c["p"]) for name, wave_max in PATHS}
        if T > 64:
            assert _same_bits(got["thread"], got["wave"])  # no lane per knot beyond 64: both settings run k_pm_solve
        for name, r in got.items():
            assert (r.status == _lib.OH_STATUS_MAX_ITER).all() and (r.iters == k).all(), (name, k, r.status, r.iters)
            _linear_rows(T, dt, r.x, c["p"])
            for s in range(gen.N_SLOTS):
                dev = [np.abs(r.x[s] - c["x"][s, n]).max(), abs(r.f[s] - c["f"][s, n])] + list(np.abs(r.kkt[s] - c["kkt"][s, n]))
                scale = [np.abs(c["x"][s, n]).max(), abs(c["f"][s, n])] + list(np.abs(c["kkt"][s, n]))
                for q, d, rec, sc in zip(("x", "f", "stat", "feas", "compl"), dev, c["dist"][s, n], scale):
                    ratio = d / max(rec, FLOOR * max(1.0, sc) / FACTOR)
                    if ratio > worst[name][0]:
                        worst[name][0], worst[name][2] = ratio, (s, k, q, float(d), float(rec))
                    if not ratio <= FACTOR:
                        failures.append((name, s, k, q, float(d), float(rec)))
                worst[name][1] = max(worst[name][1], dev[0])
    for name, (ratio, dx, where) in worst.items():
        print(f"PM_STEPS {variant} T {T} {name}: largest ratio {ratio:.3g} at (slot, k, quantity, device distance, port distance) {where}; |x - x_mp| <= {dx:.3e}")
    assert not failures, failures


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,T", gen.cells(), ids=lambda v: str(v))
def test_full_solves_against_the_port(hip_lib, variant, T):
    opt = gen.options(variant, T)
    x0, p = (np.stack(a) for a in zip(*(pe.full_instance(variant, T, i) for i in pe.FULL_SEEDS[(variant, T)])))
    assert len(p) == pe.N_FULL
    ref = [gen.port(opt, x0[b], p[b], pe.MAX_ITER) for b in range(len(p))]
    for r in ref:
        last, before = pe.margins(r)
        assert r["status"] == 0 and last <= 0.5 * pe.TOL and before >= 2.0 * pe.TOL, (last, before)
    got = {name: _solve(variant, T, pe.MAX_ITER, wave_max, x0, p) for name, wave_max in PATHS}
    for name, r in got.items():
        assert np.array_equal(r.status, [q["status"] for q in ref]) and np.array_equal(r.iters, [q["iters"] for q in ref]), (name, r.status, r.iters)
        assert (r.kkt <= pe.TOL).all(), (name, r.kkt.max())
        _linear_rows(T, opt["dt"], r.x, p)
        for b, q in enumerate(ref):
            assert abs(r.f[b] - q["f"]) <= 1e-8 * max(1.0, abs(q["f"])), (name, b, r.f[b], q["f"])
            if variant in ("mpc", "planner"):
                if variant == "mpc":
                    k = kkt_reference_form(PointMassMPCNLP(T=T), r.x[b], p[b], active_tol=1e-3)
                    assert k["stationarity"] <= 1e-5 and k["feasibility"] <= 1e-9, (name, b, k["stationarity"], k["feasibility"])
                else:  # p = [init; goal], the obstacle at the origin and the start at rest are part of the problem
                    k = kkt_reference_form(PointMassPlannerNLP(T=T), r.x[b], np.concatenate([p[b, 0:2], p[b, 4:6]]), active_tol=1e-3)
                    assert k["stationarity"] < 1e-6 and k["feasibility"] < 1e-9, (name, b, k["stationarity"], k["feasibility"])
    rt, rw = got["thread"], got["wave"]
    if T > 64:
        assert _same_bits(rt, rw)
    assert np.abs(rt.x - rw.x).max() <= 1e-10 and np.abs(rt.kkt - rw.kkt).max() <= 1e-10
    assert np.abs(rt.f - rw.f).max() <= 1e-11 * max(1.0, np.abs(rt.f).max())


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["mpc", "planner"])
@pytest.mark.parametrize("path,sizes", [("thread", (1, 63, 64, 65, 129, 63)), ("wave", (1, 65, 1))], ids=["thread", "wave"])
def test_an_instance_keeps_its_bits_wherever_it_sits(hip_lib, fixture, variant, path, sizes):
    T = 64
    c = _cell(fixture, variant, T)
    fx, fp = pe.filler(T, gen.options(variant, T)["dt"], max(sizes), seed=1)
    be = _backend(variant, T, pe.MAX_ITER, dict(PATHS)[path])  # one handle: its pool grows to the largest batch and is used again for a smaller one
    alone = None
    for B in sizes:
        pos = sorted({q for q in (0, 62, 63, 64, B - 1) if q < B})
        for shift in range(gen.N_SLOTS):
            x0, p = fx[:B].copy(), fp[:B].copy()
            who = {q: (i + shift) % gen.N_SLOTS for i, q in enumerate(pos)}
            for q, s in who.items():
                x0[q], p[q] = c["x0"][s], c["p"][s]
            r = be.solve(x0, p)
            if alone is None:
                alone = {}
            for q, s in who.items():
                bits = tuple(getattr(r, k)[q].tobytes() for k in ("x", "f", "kkt", "iters", "status"))
                if B == 1 and s not in alone:
                    alone[s] = bits  # the first four solves: every instance by itself
                assert bits == alone[s], (variant, path, B, q, s)
            assert (r.status == _lib.OH_STATUS_CONVERGED).mean() >= 0.9  # (what is compared are real solves, the fillers included)
    be.close()
    assert sorted(alone) == list(range(gen.N_SLOTS))


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------------
def _poisons(T):
    """name -> (array, index, value, ends at OH_STATUS_NUMERICAL, needs fix_final_velocity)"""
    nan = float("nan")
    return {
        "NaN in curr": ("p", 1, nan, True, False),
        "NaN in a goal entry of knot 1": ("p", 4 + 2 * 1 + 1, nan, True, False),
        "NaN in a goal entry of knot T-1": ("p", 4 + 2 * (T - 1), nan, True, False),
        "NaN in an obstacle entry of knot T-1": ("p", 4 + 2 * T + 2 * (T - 1), nan, True, False),
        "inf in a goal entry": ("p", 4 + 2 * (T // 2), float("inf"), True, False),
        # (not a row of the iteration but a row of the problem, the one k_pm_infeasible judges: both kernels carry the NaNs of every knot's rows)
        "NaN in an obstacle entry of knot 0": ("p", 4 + 2 * T + 1, nan, True, False),
        "NaN in the Y block of x0": ("x0", 2 * (T // 2) + 1, nan, False, False),
        "NaN in the dY block of x0 at knot 0": ("x0", 2 * T, nan, False, False),
        "NaN in the dY block of x0 at knot T-1 under fix_final_velocity": ("x0", 2 * T + 2 * (T - 1) + 1, nan, False, True),
    }


@pytest.mark.parametrize("T", [3, 64])
@pytest.mark.parametrize("variant", ["mpc", "planner"])
def test_non_finite_inputs(hip_lib, fixture, variant, T):
    c = _cell(fixture, variant, T)
    order = [0, 0, 1, 2, 1, 3]  # slots 1 and 4 of the batch are the poisoned copies of instances 0 and 1
    bad, src = [1, 4], [0, 1]
    good = [0, 2, 3, 5]
    fix = gen.VARIANTS[variant][4]
    clean = {name: _solve(variant, T, pe.MAX_ITER, wave_max, c["x0"], c["p"]) for name, wave_max in PATHS}
    for what, (arr, idx, value, numerical, needs_fix) in _poisons(T).items():
        if needs_fix and not fix:
            continue
        if numerical and variant != "mpc":
            continue  # (under track_final_only the goals of the knots before the last carry weight 0: the MPC tick's cost reads every listed entry)
        x0, p = c["x0"][order].copy(), c["p"][order].copy()
        (p if arr == "p" else x0)[bad, idx] = value
        got = {name: _solve(variant, T, pe.MAX_ITER, wave_max, x0, p) for name, wave_max in PATHS}
        for name, r in got.items():
            for k in ("x", "f", "kkt", "iters", "status"):  # the finite neighbours: the bits of the batch without the poisoned instances
                assert getattr(r, k)[good].tobytes() == getattr(clean[name], k).tobytes(), (what, name, k)
            if numerical:
                assert (r.status[bad] == _lib.OH_STATUS_NUMERICAL).all(), (what, name, r.status)
            else:
                for k in ("x", "f", "kkt", "iters", "status"):
                    assert getattr(r, k)[bad].tobytes() == getattr(clean[name], k)[src].tobytes(), (what, name, k)
        if numerical:  # identically on both paths: the evaluation that finds the value is the same one
            assert np.array_equal(got["thread"].iters[bad], got["wave"].iters[bad]), (what, got["thread"].iters[bad], got["wave"].iters[bad])


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,advance,ramp", [(3, 2, 0.032), (64, 63, 0.004)], ids=["T3", "T64"])
@pytest.mark.parametrize("path", ["thread", "wave"])
def test_closed_loop_at_the_largest_advance(hip_lib, path, T, advance, ramp):
    B, n_ticks, dt = 65, 3, 0.05
    tab = pe.obstacle_table(n_ticks * advance + T, dt)
    state0 = pe.rollout_starts(B)
    be = _backend("mpc", T, pe.MAX_ITER, dict(PATHS)[path])
    states, f, iters, status = be.rollout(state0, tab, n_ticks, advance, ramp)
    assert np.array_equal(states[0], state0) and (status == _lib.OH_STATUS_CONVERGED).mean() >= 0.9
    st, x = state0.copy(), np.zeros((B, 4 * T))
    for k in range(n_ticks):
        goal = st[:, None, 0:2] + ramp * np.arange(T)[None, :, None]  # (B, T, 2)
        obs = np.tile(tab[k * advance : k * advance + T].reshape(-1), (B, 1))
        r = be.solve(x, np.concatenate([st, goal.reshape(B, -1), obs], axis=1))
        assert np.array_equal(r.status, status[k]) and np.array_equal(r.iters, iters[k]), (k, np.flatnonzero(r.iters != iters[k]))
        assert np.abs(r.f - f[k]).max() < 1e-10
        x = r.x
        st = np.concatenate([x[:, 2 * advance : 2 * advance + 2], x[:, 2 * T + 2 * advance : 2 * T + 2 * advance + 2]], axis=1)
        assert np.abs(st - states[k + 1]).max() < 1e-9
    be.close()
