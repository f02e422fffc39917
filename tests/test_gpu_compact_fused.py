"""compact_fused: before a carried compaction the retraction compiled for the chain lays the knots down at their new index itself
(oh_spec_retract_move) and k_carry_gather moves only the pinned knots and the per-instance scalars.  Only data movement changes, so a solve with the
option on equals the solve with it off (k_retract, then the whole k_carry_gather) in every bit of every output: no tolerance."""
import numpy as np
import pytest

import bench
from conftest import KUKA_KIN
from optas_amd.backend import FigureEightBackend
from optas_amd.models import RobotModel

pytestmark = pytest.mark.gpu
LINK = "end_effector_ball"


def _backend(**opts):
    dt, lp = bench.local_path()
    chain = RobotModel(urdf_filename=KUKA_KIN).kinematic_chain(LINK)
    be = FigureEightBackend(chain, bench.T, dt, lp, max_iter=300, tol=1e-8, hessian=2)  # bench.py's headline: tol 1e-8, hybrid Hessian
    return be.set_options(opts) if opts else be


def _solve(B, x0, qc, **opts):
    be = _backend(**opts)
    assert be.get_option("compact_fused") == opts.get("compact_fused", 1)
    r = be.solve(x0, qc)
    assert be.flag("specialized")  # the kernels compiled for the chain ran (every batch of at least 4096 instances): the option selects a path
    out = {"x": r.x, "f": r.f, "kkt": r.kkt, "iters": r.iters, "status": r.status, "multipliers": be.multipliers(B), "timing": be.timing()}
    be.close()
    return out


# B = 24 576 on one stream: batched launches and compactions above the hand-over to the persistent kernel; B = 65 536 at the default options: two
# parts on two streams, the peer inherits the option; compact_sort = 0: the survivors keep their order, another pattern of new indices.
# (At the default hand-over, 16 384 survivors, a batch of 24 576 is compacted twice -- once carried, once for the hand-over; measured on the GPU, both
# settings of the option bit-identical -- which is fewer than the three this test asks for.  The one-stream cases therefore hand over at 4096
# survivors: same batch, same stream count, more carried compactions.)
ONE_STREAM = {"streams": 1, "tail_threshold": 4096}


@pytest.mark.parametrize("B, opts", [(24576, ONE_STREAM), (65536, {}), (24576, dict(ONE_STREAM, compact_sort=0))], ids=["one_stream", "two_parts", "unsorted"])
def test_fused_compaction_is_bit_identical_to_the_gather(hip_lib, monkeypatch, B, opts):
    monkeypatch.delenv("OH_DEBUG_OPTIONS", raising=False)
    x0, qc = bench.make_inputs(B, 0)
    on = _solve(B, x0, qc, compact_fused=1, **opts)
    off = _solve(B, x0, qc, compact_fused=0, **opts)
    print({k: (on["timing"][k], off["timing"][k]) for k in ("compactions", "tail_iterations", "iterations_launched")})
    for k in ("x", "f", "kkt", "iters", "status", "multipliers"):
        assert np.array_equal(on[k], off[k]), k
    assert on["timing"]["compactions"] == off["timing"]["compactions"] and on["timing"]["compactions"] >= 3
    assert on["timing"]["tail_iterations"] > 0 and off["timing"]["tail_iterations"] > 0
    assert (on["status"] == 0).all() and (off["status"] == 0).all()
