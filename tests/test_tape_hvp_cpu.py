"""oh_tape_hvp without a GPU: the float64 port of the kernel's forward-over-reverse sweep (tests/tape_hvp_ref.py:hvp_port) against second differences
of the 60-digit interpreter (hvp_mp / hessian_mp) on every case tests/test_gpu_tape_hvp.py grades the device on, and the C entry's argument checks.

Tolerance: |port - mp|_inf <= 2.5e-13 max(1, |mp|_inf), a quarter of the device's 1e-12 (GRAD_TOL of tests/test_gpu_tape_evaluators.py), so that a
failure on the GPU is the device's.  Measured: <= 2.3e-16 over all cases (finite, smooth points; the selections at the kinks held)."""
import os
import re

import numpy as np
import pytest

import tape_cases as tc
import tape_hvp_ref as R
from optas_amd import _lib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.mark.parametrize("o", sorted(tc.DIFF_OPS), ids=lambda o: tc.OP_NAME[o])
def test_port_matches_mp_on_every_differentiable_opcode_alone(o):
    tp = tc.single_op_tape(o)
    lines, ref = R.single_op_lines(o), R.single_op_reference(o)
    assert len(lines) >= 3
    for x, Href in zip(lines, ref):
        H = R.hessian_port(tp, x, np.zeros(0), [1.0])
        ok, err = R.within(H, Href, R.PORT_TOL)
        print(tc.OP_NAME[o], x, "error", err)
        assert ok, (tc.OP_NAME[o], x, H, Href, err)
    if o in tc.BINARY and o in (5, 6, 10):  # the cross term is exercised: it is not zero
        assert np.abs(ref[:, 0, 1]).max() > 1e-3


@pytest.mark.parametrize("name", [c[0] for c in R.composite_cases()])
def test_port_matches_mp_on_composite_tapes(name):
    _, tp, x, p, seeds, v = next(c for c in R.composite_cases() if c[0] == name)
    ref = R.composite_reference(name)
    hv, g = R.hvp_port(tp, x, p, seeds, v)
    H = R.hessian_port(tp, x, p, seeds)
    ok_v, e_v = R.within(hv, ref["hv"], R.PORT_TOL)
    ok_h, e_h = R.within(H, ref["H"], R.PORT_TOL)
    print(name, "H v error", e_v, "dense error", e_h, "|H|", np.abs(ref["H"]).max())
    assert ok_v and ok_h, (name, e_v, e_h)
    assert R.within(ref["H"] @ v, ref["hv"], R.PORT_TOL)[0]  # the two mp references agree with each other
    # the port's gradient is the first-order oracle's, bit for bit (same operations in the same order)
    from oracle import tape_ref

    with np.errstate(all="ignore"):
        val = tape_ref.forward(tp, x, p)
        sd = {}
        for w, r in zip(seeds, [int(tp.out_cost)] + [int(t) for t in tp.out_rows]):
            sd[r] = sd.get(r, 0.0) + w
        assert tc.same(g, tape_ref.reverse(tp, val, sd)).all()


def test_the_last_random_tape_covers_every_differentiable_opcode():
    tp = next(c for c in R.composite_cases() if c[0] == "random8")[1]
    assert tc.ops_used(tp)[1] == tc.DIFF_OPS


def test_null_handle_is_rejected_and_named():
    lib = _lib.load()
    assert lib.oh_tape_hvp(None, 1, None, None, None, 1, None, None, None) == 1
    assert b"oh_tape_hvp" in lib.oh_last_error()


def test_entry_is_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "optas_hip.h")).read()
    assert re.search(r"\bint oh_tape_hvp\(oh_handle\* h, int B, const double\* x, const double\* p, const double\* seeds,\s*int nv, const double\* V, double\* HV, double\* grad\);", txt)
    assert "oh_tape_hvp" in _lib.SYMBOLS
    assert _lib.load().oh_abi_version() == 8  # no struct changed
