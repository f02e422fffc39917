"""compact_fused = 2, the lean carried compaction: the moving retraction leaves the accepted knot behind and moves the Lagrangian gradient only on the
lanes whose evaluation reads it; an instance whose trial the sweep after the compaction rejects is fetched from the old layout through a device-side
list (k_sweep_lists), and the list-driven copies behind a sweep are launched only when their list is not empty.  Only data movement and launches change,
so every bit of every output equals the round-7 sequence (compact_fused = 1) and the gather (compact_fused = 0): no tolerance.

4096 KUKA instances, T = 12, start configurations perturbed by +-0.5 rad so that trials are rejected (at bench.py's +-0.1 almost none is); the kernels
compiled for the chain always (specialize = 1), hand-over to the persistent kernel at 256 survivors, a compaction whenever a tenth of the batch has
finished.  Seed 20261019.  Instances that went through the rescue list, measured on an MI355X: hybrid 209, exact 60, hybrid_max_iter_6 9,
exact_max_iter_6 4, hybrid_check_every_2 26, exact_check_every_2 44 (of 6587 / 5341 / 3393 / 948 / 4649 / 3737 survivors moved by 4 / 4 / 1 / 1 / 3 / 3 carried
compactions; the hybrid cases moved the gradient of 87, 91 and 86 % of them).  lean_count = 1 switches the counter of the gradient-moving lanes on."""
import numpy as np
import pytest

from conftest import KUKA_KIN
from optas_amd import _lib
from optas_amd.backend import FigureEightBackend
from optas_amd.models import RobotModel

pytestmark = pytest.mark.gpu
LINK = "end_effector_ball"
B, T, SEED = 4096, 12, 20261019
QC0_DEG = [0, 30, 0, -90, 0, -30, 0]
OPTS = {"specialize": 1, "tail_threshold": 256, "compact_frac": 0.9, "lean_count": 1}


def _problem():
    tmax = 10.0 * (T - 1) / 49.0  # the knot spacing of the T = 50 headline
    t = np.linspace(0.0, tmax, T)
    lp = np.zeros((T, 3))
    lp[:, 0] = 0.2 * np.sin(t * np.pi * 0.5)
    lp[:, 1] = 0.1 * np.sin(t * np.pi)
    rng = np.random.default_rng(SEED)
    qc = np.deg2rad(QC0_DEG)[None, :] + rng.uniform(-0.5, 0.5, (B, 7))
    x0 = np.concatenate([np.repeat(qc, T, axis=0).reshape(B, 7 * T), np.zeros((B, 7 * (T - 1)))], axis=1)
    return float(t[1] - t[0]), lp, x0, qc


@pytest.fixture(scope="module")
def problem():
    return _problem()


def _solve(problem, hessian, max_iter, fused, extra):
    dt, lp, x0, qc = problem
    chain = RobotModel(urdf_filename=KUKA_KIN).kinematic_chain(LINK)
    be = FigureEightBackend(chain, T, dt, lp, max_iter=max_iter, tol=1e-8, hessian=hessian)
    be.set_options(dict(OPTS, compact_fused=fused, **extra))
    assert be.get_option("compact_fused") == fused
    r = be.solve(x0, qc)
    assert be.flag("specialized")
    out = {"x": r.x, "f": r.f, "kkt": r.kkt, "iters": r.iters, "status": r.status, "multipliers": be.multipliers(B), "timing": be.timing()}
    be.close()
    return out


# (hessian, max_iter, further options, carried compactions asked for).  max_iter = 6: instances end MAX_ITER inside compacting iterations;
# check_every = 2: the host looks at the counters after every second sweep only, and launches the two list-driven copies unconditionally after the others.
CASES = {
    "hybrid": (_lib.OH_HESSIAN_HYBRID, 300, {}, 4),
    "exact": (_lib.OH_HESSIAN_EXACT, 300, {}, 4),
    "hybrid_max_iter_6": (_lib.OH_HESSIAN_HYBRID, 6, {}, 1),
    "exact_max_iter_6": (_lib.OH_HESSIAN_EXACT, 6, {}, 1),
    "hybrid_check_every_2": (_lib.OH_HESSIAN_HYBRID, 300, {"check_every": 2}, 1),
    "exact_check_every_2": (_lib.OH_HESSIAN_EXACT, 300, {"check_every": 2}, 1),
}


@pytest.mark.parametrize("case", list(CASES))
def test_lean_compaction_is_bit_identical_to_both_earlier_sequences(hip_lib, monkeypatch, problem, case):
    monkeypatch.delenv("OH_DEBUG_OPTIONS", raising=False)
    hessian, max_iter, extra, min_compactions = CASES[case]
    lean, fused, gather = (_solve(problem, hessian, max_iter, v, extra) for v in (2, 1, 0))
    tm = lean["timing"]
    print(case, {k: (tm[k], fused["timing"][k], gather["timing"][k]) for k in ("compactions", "rejected_steps", "tail_iterations", "iterations_launched")},
          {k: tm[k] for k in ("rescued_instances", "gradient_lanes_moved", "lanes_moved")}, "status counts", np.unique(lean["status"], return_counts=True))
    for other in (fused, gather):
        for k in ("x", "f", "kkt", "iters", "status", "multipliers"):
            assert np.array_equal(lean[k], other[k]), (case, k)
        assert tm["compactions"] == other["timing"]["compactions"]
        assert other["timing"]["rescued_instances"] == 0  # the list belongs to the lean sequence alone
    # (compactions counts the hand-over to the persistent kernel too: one of them is not carried)
    assert tm["compactions"] - 1 >= min_compactions, tm
    assert tm["lanes_moved"] > 0 and tm["rescued_instances"] >= 1, tm  # without a rescued instance the run says nothing about the knots left behind
    assert 0 <= tm["gradient_lanes_moved"] <= tm["lanes_moved"]
    if hessian == _lib.OH_HESSIAN_EXACT:
        assert tm["gradient_lanes_moved"] == tm["lanes_moved"]  # exact curvature reads the gradient on every lane
    if max_iter == 6:
        assert (lean["status"] == _lib.OH_STATUS_MAX_ITER).any()
