"""tests/golden/pm_steps_mp.npz without a GPU: the numpy port of the point-mass interior-point solver (oracle/pointmass_ipm.py), on which every
other point-mass test leans, against the 50-digit state machine of tests/pm_step_ref.py, whose Newton directions come from a dense solve of the
condensed system and whose stationarity figure comes from the same control-to-state map -- neither uses the Riccati or the adjoint recursion.

 1. The port's answers after 1, 2 and 3 iterations lie at the recorded distance from the mp ones on every case of the fixture.  The recorded distance
    is rounding noise of numpy's small products and factorisations, which another BLAS may order differently: a factor 2 is granted, over a floor of
    1e-13 max(1, |reference|) (the floor of the GPU test's tolerance).
 2. The fixture is what tools/make_pm_steps_golden.py writes: every cell of T <= 5 is drawn and computed again, and so is one T = 64 case from its
    stored inputs; inputs and mp results agree bit for bit.
 3. The pinned branch is exercised: under fix_final_velocity the mp Newton direction has dv_{T-1} = 0 and the iterate v_{T-1} = 0 after every step
    (to the 50 digits: below 1e-45), while without the flag both are far from zero."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_pm_steps_golden as gen  # noqa: E402

FLOOR = 1e-13
MP_ARRAYS = ("desc", "x0", "p", "x", "f", "kkt", "step", "pinned")  # everything but the port's distance, which depends on numpy's build


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "pm_steps_mp.npz"))


def _case(fixture, variant, T, slot):
    cid = gen.case_id(variant, T, slot)
    return {k: fixture[cid + "_" + k] for k in MP_ARRAYS + ("dist",)}


def test_fixture_holds_the_grid(fixture):
    want = {gen.case_id(v, T, s) + "_" + k for v, T in gen.cells() for s in range(gen.N_SLOTS) for k in MP_ARRAYS + ("dist",)}
    assert set(fixture.files) == want and len(gen.cells()) == 26
    for v, T in gen.cells():
        cs = [_case(fixture, v, T, s) for s in range(gen.N_SLOTS)]
        assert all(np.abs(c["p"][2:4]).min() > 0.0 for c in cs)  # start velocities non-zero
        assert sum(bool(np.abs(c["x0"][2 * T :]).max() > 0.0) for c in cs) >= 2  # a velocity seed in at least two
        if T >= 5:  # a first step cut by the fraction-to-the-boundary rule, wherever the generator's search found one
            assert any(c["step"][0, 0] < 1.0 for c in cs) == ((v, T) not in gen.NO_CUT_CELLS), (v, T)
        for c in cs:
            am = c["step"].min(axis=1)
            assert (np.abs(am - 0.9) > 1e-6).all() and (np.abs(am - 0.5) > 1e-6).all()
            opt = gen.options(v, T)
            assert np.array_equal(c["desc"], [T, opt["dt"], opt["w_acc"], opt["w_vel"], opt["track_final_only"], opt["fix_final_velocity"], gen.YLIM, gen.VLIM,
                                              gen.SAFE, gen.TOL])


@pytest.mark.parametrize("variant,T", gen.cells(), ids=lambda v: str(v))
def test_port_against_mp_at_the_recorded_distance(fixture, variant, T):
    opt = gen.options(variant, T)
    for slot in range(gen.N_SLOTS):
        c = _case(fixture, variant, T, slot)
        for n, k in enumerate(gen.KS):
            r = gen.port(opt, c["x0"], c["p"], k)
            assert r["status"] == 1 and r["iters"] == k
            got = [np.abs(gen.port_x(r) - c["x"][n]).max(), abs(r["f"] - c["f"][n])] + list(np.abs(np.array(r["kkt"]) - c["kkt"][n]))
            scale = [np.abs(c["x"][n]).max(), abs(c["f"][n])] + list(np.abs(c["kkt"][n]))
            for name, d, rec, sc in zip(("x", "f", "stat", "feas", "compl"), got, c["dist"][n], scale):
                assert d <= max(2.0 * rec, FLOOR * max(1.0, sc)), (variant, T, slot, k, name, d, rec)


def test_small_horizon_cells_regenerate_bit_for_bit(fixture):
    small = [(v, T) for v, T in gen.cells() if T <= 5]
    arrays, draws, rejected = gen.generate(small, verbose=False)
    assert 4 * rejected <= draws
    n = 0
    for key, v in arrays.items():
        if key.rsplit("_", 1)[1] in MP_ARRAYS:
            assert fixture[key].shape == v.shape and fixture[key].tobytes() == v.tobytes(), key
            n += 1
    assert n == len(small) * gen.N_SLOTS * len(MP_ARRAYS)


def test_one_T64_case_regenerates_bit_for_bit(fixture):
    variant, T, slot = "planner", 64, 1
    c = _case(fixture, variant, T, slot)
    e = gen.evaluate(gen.options(variant, T), c["x0"], c["p"])
    assert e is not None
    for k in MP_ARRAYS:
        assert e[k].shape == c[k].shape and e[k].tobytes() == c[k].tobytes(), k


def test_pinned_branch_is_exercised(fixture):
    for v, T in gen.cells():
        for slot in range(gen.N_SLOTS):
            c = _case(fixture, v, T, slot)
            if gen.VARIANTS[v][4]:
                assert (c["pinned"] <= 1e-45).all(), (v, T, slot, c["pinned"])
                assert (np.abs(c["x"][:, 2 * T + 2 * (T - 1) :]) <= 1e-45).all()
            else:
                assert (c["pinned"] > 1e-6).all(), (v, T, slot, c["pinned"])
