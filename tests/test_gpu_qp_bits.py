"""The one interior-point text over a team (optas_amd/csrc/oh_qp.hip: qp_ipm with QpThread and QpWave), the rules of oh_qp_rules.h in
k_qp_solve_block and k_qp_assemble_block in the place of k_qp_assemble_par, held to the bits of the texts they replaced.
tests/golden/qp_parent_bits.npz was written on an MI355X by the library of the last commit that had k_qp_solve, k_qp_solve_wave and
k_qp_assemble_par as texts of their own, through qp_outputs() below (tools/gpu_qp_ab_dump.py pin).  Outputs only; the inputs come from the
seeds.  Equality of every array as integers."""
import os

import numpy as np
import pytest

import qp_planted as Q
import qp_planted_large as L
from conftest import GOLDEN, SEED

OUT = ("x", "f", "kkt", "iters", "status")
B_CLASS = 12       # partly filled blocks of 64, 32 and 16; with qp_mode -1 a wavefront per instance
BAD_POS = (0, 37, 63)  # test_bad_instances_leave_their_batch_alone
BAD_RUNS = ((70, -1), (70, 0), (64, -1))


def _rows(module, name, B):
    return np.stack([module.pack(qp) for qp in module.planted_batch(name, B)])


def qp_cases():
    """[(key, "rows", (n, m, me), qp_mode, rows, multipliers wanted)] and [(key, "solver", problem, options, parameters)]"""
    cases = []
    for name, a in Q.CLASSES.items():
        dims = (a["n"], a["m"], a["me"])
        rows = _rows(Q, name, B_CLASS)
        for mode in (0, 1, 2, -1):
            if mode < 0 or mode == 0 or Q.forced_fits(*dims, mode):
                cases.append(("%s/B%d/mode%d" % (name, B_CLASS, mode), "rows", dims, mode, rows, mode <= 0))
    for name in ("base", "vertex_eq"):  # the automatic thread choice across a block boundary; a wavefront alone
        a = Q.CLASSES[name]
        for B in (70, 1):
            cases.append(("%s/B%d/mode-1" % (name, B), "rows", (a["n"], a["m"], a["me"]), -1, _rows(Q, name, B), False))
    a = Q.CLASSES["base"]
    bad = Q.bad_instances(Q.planted_instances("base")[0])
    for B, mode in BAD_RUNS:
        rows = _rows(Q, "base", B)
        for k, p in enumerate(BAD_POS):
            rows[p] = bad[k]
        cases.append(("bad/B%d/mode%d" % (B, mode), "rows", (a["n"], a["m"], a["me"]), mode, rows, False))
    for module, name in ((Q, "base"), (Q, "rank_def"), (Q, "me_eq_n"), (L, "n33")):  # k_qp_solve_block: the rules header
        a = module.CLASSES[name]
        cases.append(("%s/B3/mode3" % name, "rows", (a["n"], a["m"], a["me"]), 3, _rows(module, name, 3), False))
    # device assembly: a block per instance with two passes of the probe loop (B <= 64), a thread per instance (70), the large handle's kernel
    rng = np.random.default_rng(SEED + 13)
    for B in (3, 64, 70):
        cases.append(("parametric/B%d" % B, "solver", "parametric", {}, rng.uniform(0.5, 1.5, (B, 4))))
    cases.append(("mpc/B3", "solver", "mpc", {"dense_qp": True}, L.mpc_parameters(np.random.default_rng(SEED + 14), 3)))
    return cases


def case_path(case):
    """launch_path of a "rows" case that runs a thread or a wavefront kernel, else None"""
    if case[1] != "rows" or case[3] == 3 or L.is_large(*case[2]):
        return None
    return Q.launch_path(*case[2], len(case[4]), case[3])


def qp_outputs(cases):
    """{key/output: array} through QPBackend and HIPSolver only."""
    from optas_amd.backend import QPBackend
    from optas_amd.solver import HIPSolver

    out, problems = {}, {}
    for case in cases:
        key, kind = case[:2]
        if kind == "rows":
            (n, m, me), mode, rows, want_mult = case[2:]
            be = QPBackend(n, m, me)
            try:
                be.set_option("qp_mode", mode)
                r = be.solve(np.zeros((len(rows), n)), rows)
                assert be.flag("qp_block") == (1 if mode == 3 or L.is_large(n, m, me) else 0)
                got = dict(zip(OUT, (r.x, r.f, r.kkt, r.iters, r.status)))
                if want_mult:
                    got["lam"], got["nu"] = be.multipliers(len(rows))
            finally:
                be.close()
        else:
            which, options, pv = case[2:]
            if which not in problems:
                problems[which] = Q.parametric_qp() if which == "parametric" else L.mpc_problem()
            o = problems[which]
            dev = HIPSolver(o).setup("hip_sqp", options)
            try:
                assert dev.backend.be.tape is not None
                r = dev.solve_batch_arrays(np.zeros((len(pv), o.nx)), pv)
                got = dict(zip(OUT, (r.x, r.f, r.kkt, r.iters, r.status)))
            finally:
                dev.backend.close()
        for name, a in got.items():
            out["%s/%s" % (key, name)] = np.ascontiguousarray(a)
    return out


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def check_pinned(ref, cases):
    """What the cases are there for happens in the pinned runs: every launch path, the exits of the bad instances beside clean lanes."""
    paths = {case_path(c) for c in cases} - {None}
    assert ("wave", 64) in paths and {p[1] for p in paths if p[0] == "thread"} == {0, 1, 2}, paths
    assert {p[2] for p in paths if p[0] == "thread"} == {64, 32, 16}, paths
    for B, mode in BAD_RUNS:
        st = ref["bad/B%d/mode%d/status" % (B, mode)]
        assert (st[list(BAD_POS)] != 0).all() and (np.delete(st, BAD_POS) == 0).all(), (B, mode, st)
    assert {1, 2} <= set(ref["bad/B70/mode0/status"].tolist())  # MAX_ITER and NUMERICAL
    for c in cases:
        if not c[0].startswith("bad/"):
            assert (ref[c[0] + "/status"] == 0).all(), c[0]


@pytest.mark.gpu
def test_one_text_has_the_bits_of_the_texts_it_replaced(hip_lib):
    ref = np.load(os.path.join(GOLDEN, "qp_parent_bits.npz"))
    cases = qp_cases()
    check_pinned(ref, cases)
    got = qp_outputs(cases)
    assert sorted(got) == sorted(ref.files)
    differ = []
    for key in ref.files:
        if got[key].dtype != ref[key].dtype or got[key].shape != ref[key].shape or not (_bits(got[key]) == _bits(ref[key])).all():
            differ.append(key)
    print("arrays", len(ref.files), "differing", differ)
    assert not differ, differ
