"""The wavefront evaluator's one level-schedule sweep (optas_amd/csrc/oh_tape_wave.hip: WaveEval::sweep) held to the bits of the three sweeps it replaced.
tests/golden/tape_wave_parent_bits.npz was written on an MI355X by the library of the last commit that had WaveEval::phi, k_tape_wave_hvp and WaveSweep::hvp
as three texts, through wave_outputs() below (tools/gpu_tape_ab_dump.py pin): oh_tape_phi, oh_tape_hvp (option tape_hvp_wave) and oh_tape_phi_hvp (options
tape_newton + tape_newton_wave) on the opcode table, two composite tapes and a tape with an active, an inactive and an equality row, at one wavefront with the
registers in LDS and at four with the registers in global memory.  Byte equality, NaN payloads included."""
import os

import numpy as np
import pytest

import tape_cases as tc
import tape_hvp_ref as R
from conftest import GOLDEN, oh_debug
from optas_amd.backend import TapeBackend

WAVE_OPTS = {"wave64": dict(tape_wave_nt=64, tape_wave_regs="lds"), "wave256_lds": dict(tape_wave_nt=256, tape_wave_regs="lds"),
             "wave256_global": dict(tape_wave_nt=256, tape_wave_regs="global")}  # tests/test_gpu_tape_hvp_wave.py's
PATH = {"wave64": 1, "wave256_lds": 1, "wave256_global": 2}
PIN_VARIANTS = ("wave64", "wave256_global")
PIN_COMPOSITES = ("random8", "mixed_level")
PHI_OUT = ("merit", "f", "rows", "grad", "cmax", "meas")


def rows_tape():
    """cost x0^2 + x1^2 + exp(x2); rows x0 x1 - 0.1 >= 0 (active at the point below), sin(x2) + 2 >= 0 (inactive), x0 + x1 x2 - 1 = 0."""
    t = tc.B()
    x0, x1, x2 = t.x(0), t.x(1), t.x(2)
    cost = t.emit(3, t.emit(3, t.emit(12, x0), t.emit(12, x1)), t.emit(25, x2))
    g0 = t.emit(4, t.emit(5, x0, x1), t.const(0.1))
    g1 = t.emit(3, t.emit(8, x2), t.const(2.0))
    h0 = t.emit(4, t.emit(3, x0, t.emit(5, x1, x2)), t.const(1.0))
    return t.tape(cost, [g0, g1, h0], 2, 1, 3, 0)


def _batch(name, tp, x, p, B):
    """Points around x, multipliers on either side of lam = rho g, weights and one direction per instance, all from a generator seeded by the name."""
    rng = np.random.default_rng(sum(name.encode()))
    nx, ni, ne = int(tp.nx), int(tp.n_ineq), int(tp.n_eq)
    X = x[None] + rng.uniform(-0.02, 0.02, (B, nx))
    return dict(tape=tp, X=X, P=np.tile(p, (B, 1)), LAM=rng.uniform(0.0, 1.0, (B, ni)), MU=rng.uniform(-1.0, 1.0, (B, ne)), rho=1.0,
                S=np.concatenate([np.ones((B, 1)), rng.uniform(-2.0, 2.0, (B, ni + ne))], axis=1), V=rng.uniform(-1.0, 1.0, (B, 1, nx)))


def pin_cases(composites=PIN_COMPOSITES):
    """{name: tape, X, P, LAM, MU, rho, S (oh_tape_hvp's weights), V}: the opcode table (every line, special values included), composite tapes of
    tape_hvp_ref, the tape with one row of each kind."""
    X, P, operands = tc.opcode_table_lines()
    rng = np.random.default_rng(3)
    cases = {"table": dict(tape=tc.opcode_table_tape(), X=X, P=P, LAM=tc.table_multipliers(operands), MU=np.zeros((len(X), 24)), rho=tc.TABLE_RHO,
                           S=rng.uniform(-1.0, 1.0, (len(X), 49)), V=rng.uniform(-1.0, 1.0, (len(X), 1, 48)))}
    for name, tp, x, p, _, _ in R.composite_cases():
        if name in composites:
            cases[name] = _batch(name, tp, x, p, 3)
    cases["rows"] = _batch("rows", rows_tape(), np.array([0.9, 0.8, 0.3]), np.zeros(0), 2)
    cases["rows"]["LAM"][:] = [1.0, 0.0]  # g0 ~ 0.62 < lam / rho: active; g1 > 0 = lam: inactive
    return cases


def wave_outputs(monkeypatch, cases, variants, dense_max_nx=8):
    """{case/variant/output: array} of oh_tape_phi, oh_tape_hvp on the wavefront evaluator (given V; the unit directions up to dense_max_nx variables) and
    oh_tape_phi_hvp on it, one handle per case and variant; hvp_path / newton_path: what the handle's flags said ran."""
    clear = dict(tape_wave=None, tape_lbfgs=None, tape_wave_nt=None, tape_wave_regs=None, tape_lds_max=None, tape_hvp_work_mb=None, tape_newton=None,
                 tape_newton_cg=None, tape_newton_wave=None, tape_hvp_wave=None)
    out = {}
    for name, c in cases.items():
        for v in variants:
            oh_debug(monkeypatch, **clear)
            oh_debug(monkeypatch, tape_lbfgs=4, **WAVE_OPTS[v])
            be = TapeBackend(c["tape"], jit=False, wave=True, options={"tape_newton": 1, "tape_newton_wave": 1})
            oh_debug(monkeypatch, **clear)
            try:
                assert be.flag("tape_wave") >= 1, (name, v)
                be.set_option("tape_hvp_wave", 1)
                key = "%s/%s/" % (name, v)
                for k, a in be.phi(c["X"], c["P"], c["LAM"], c["MU"], c["rho"]).items():
                    out[key + "phi_" + k] = a
                assert be.flag("tape_regs_lds") == (0 if v == "wave256_global" else 1), (name, v)
                out[key + "hvp_HV"], out[key + "hvp_grad"] = be.hvp(c["X"], c["P"], c["S"], c["V"])
                if int(c["tape"].nx) <= dense_max_nx:
                    out[key + "hvp_H"] = be.hessian(c["X"], c["P"], c["S"])
                out[key + "hvp_path"] = np.array(be.flag("tape_hvp_path"))
                out[key + "phi_hvp_HV"], out[key + "phi_hvp_grad"] = be.phi_hvp(c["X"], c["P"], c["LAM"], c["MU"], c["rho"], c["V"])
                out[key + "newton_path"] = np.array(be.flag("tape_newton_path"))
            finally:
                be.close()
    return {k: np.ascontiguousarray(a) for k, a in out.items()}


@pytest.mark.gpu
def test_one_sweep_has_the_bits_of_the_three_it_replaced(hip_lib, monkeypatch):
    ref = np.load(os.path.join(GOLDEN, "tape_wave_parent_bits.npz"))
    cases = pin_cases()
    assert set(cases) == {"table", "rows"} | set(PIN_COMPOSITES)
    got = wave_outputs(monkeypatch, cases, PIN_VARIANTS)
    assert sorted(got) == sorted(ref.files)
    for name in cases:
        for v in PIN_VARIANTS:
            key = "%s/%s/" % (name, v)
            assert int(got[key + "hvp_path"][0]) == PATH[v] and int(got[key + "newton_path"][0]) == PATH[v], key
            for k in ["phi_" + o for o in PHI_OUT] + ["hvp_HV", "hvp_grad", "phi_hvp_HV", "phi_hvp_grad"]:
                assert key + k in got, key + k
    rows = got["rows/wave64/phi_rows"]
    lam = cases["rows"]["LAM"]
    assert (lam[:, 0] - rows[:, 0] > 0).all() and (lam[:, 1] - rows[:, 1] < 0).all() and rows.shape[1] == 3  # active, inactive, the equality row
    differ = [k for k in ref.files if got[k].dtype != ref[k].dtype or got[k].shape != ref[k].shape or got[k].tobytes() != ref[k].tobytes()]
    print("arrays", len(ref.files), "differing", differ)
    assert not differ, differ
