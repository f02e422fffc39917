"""Every sweep of the position-tracking family (csrc/oh_free.hip) at the horizon edges, on 7, 6 and 2 joints, plain / with limit and sphere rows /
with velocity rows (tests/free_sweep_cases.py), selected per solve with oh_set_option and confirmed with oh_get_flag "free_sweep":

  max_iter = 1     the returned knots minus the seed are the Newton step of the first system: against oracle/blocktri_mp.py (50 digits) within
                   bound(case) on every path, instance and knot; the copies of an instance in the batch are bit-identical; the seed itself is refused;
  max_iter = 2, 3  the returned knots are the numpy port's at the same cap to 1e-9, step and rejection counts equal;
  full solve       status 0, f the port's to 1e-9 relative, steps within max(2, 5 %) of the port's, multipliers by the rules of
                   test_gpu_guarded.py / test_gpu_dual_arm_velocity.py (between paths 1e-6, velocity rows 1e-3; 1e-3 against the port)."""
import os
import re

import numpy as np
import pytest

import free_sweep_cases as fc
from conftest import ROOT
from oracle.blocktri_mp import solve_mp
from oracle.robot import OracleRobot
from test_gpu_chain_lengths import _robots as chain_robots

pytestmark = pytest.mark.gpu
SERIAL, PCR, CP, BB, PERSIST = range(5)  # FreeSweep, csrc/oh_kernels.h
NAMES = ("k_step_free", "k_step_free_pcr", "k_step_free_cp", "k_step_free_bb", "k_free_persist")
# path -> options of the solve (free_pcr_max = 0: no block-per-instance sweep at any batch)
PATHS = {
    "serial": dict(free_pcr_max=0, free_cp_max=512, free_bb=1, free_persist=-1),
    "pcr": dict(free_pcr_max=4096, free_cp_max=0, free_bb=0, free_persist=-1),
    "cp": dict(free_pcr_max=4096, free_cp_max=512, free_bb=0, free_persist=-1),
    "bb_pair": dict(free_pcr_max=4096, free_cp_max=512, free_bb=1, free_persist=0),
    "auto": dict(free_pcr_max=4096, free_cp_max=512, free_bb=1, free_persist=-1),
    "persist": dict(free_pcr_max=4096, free_cp_max=512, free_bb=1, free_persist=1),
}


def expected_sweep(case, path):
    """The kernel a path must run, documented fall-backs included (oh_api.hip: free_sweep)."""
    robot, variant, nK = case
    n = fc.NDOF[robot]
    if path == "serial" or n not in (6, 7) or nK > 128:
        return SERIAL
    if path == "pcr":
        return PCR
    if path == "cp" or n == 6:  # (6 joints have no twisted factorisation: free_bb = 1 leaves the cyclic-reduction kernels)
        return CP if nK <= 64 else PCR
    if path == "bb_pair" or variant != "guarded":  # (velocity rows and plain handles never run the persistent kernel)
        return BB
    return PERSIST if (path == "persist" or nK <= 64) else BB


def paths_of(case):
    robot, variant, nK = case
    if fc.NDOF[robot] == 2:
        return ("serial", "auto")
    return tuple(PATHS) if variant == "guarded" else ("serial", "pcr", "cp", "bb_pair", "auto")


@pytest.fixture(scope="module")
def robots_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("free_sweep_robots")


def _knots(c, res):
    return res.x[:, : c.n * c.T].reshape(fc.BATCH, c.T, c.n)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_every_sweep_against_mp_and_the_port(hip_lib, robots_dir, case):
    c = fc.Case(robots_dir, case)
    x0, p = c.batch()
    idx = np.arange(fc.BATCH) % fc.N_INST
    tag = fc.case_id(case)
    # references, once per case: the first system of every instance in mpmath, the port at every cap
    z_mp = []
    for i in range(fc.N_INST):
        _, recs = c.port_systems(i, 1)
        r = recs[0]
        z_mp.append(solve_mp(r["D"], r["Er"], r["rhs"], r["mu"])[0])
    port = {cap: [c.port(i, cap) for i in range(fc.N_INST)] for cap in (1, 2, 3, c.max_iter_full)}
    z_inf = max(float(np.abs(z).max()) for z in z_mp)
    bnd = fc.bound(case, z_inf)
    for cap in (1, 2, 3, c.max_iter_full):
        be = c.backend(cap)
        ref_lam = None
        for path in paths_of(case):
            be.set_options(PATHS[path])
            res = be.solve(x0, p)
            flag, used = be.flag("free_sweep"), be.flag("free_sweeps_used")
            want = expected_sweep(case, path)
            assert flag == want and used == 1 << want, (tag, cap, path, NAMES[flag], NAMES[want], used)
            X = _knots(c, res)
            assert np.isfinite(res.x).all() and np.array_equal(X[:, : c.t0], np.broadcast_to(c.qc[idx][:, None], (fc.BATCH, c.t0, c.n)))
            for b in range(fc.N_INST, fc.BATCH):  # the copies of an instance
                assert np.array_equal(res.x[b], res.x[b % fc.N_INST]) and res.f[b] == res.f[b % fc.N_INST] and res.iters[b] == res.iters[b % fc.N_INST], (tag, cap, path, b)
            pr = port[cap]
            steps, rej = res.iters[: fc.N_INST].tolist(), be.timing()["rejected_steps"]
            if cap == 1:
                z = X[:, c.t0 :] - c.Q0[idx][:, c.t0 :]
                err = max(float(np.abs(z[b] - z_mp[b % fc.N_INST]).max()) for b in range(fc.BATCH))
                print("%s cap 1 %-8s %-16s |z - z_mp| %.2e (bound %.2e, |z| %.3f) steps %s port %s" % (tag, path, NAMES[flag], err, bnd, z_inf, steps, [r["iters"] for r in pr]))
                assert min(float(np.abs(z[b]).max()) for b in range(fc.BATCH)) > 0.0, (tag, path, "the seed came back")
                assert err <= bnd, (tag, path, NAMES[flag], err, bnd)
                assert steps == [r["iters"] for r in pr]
            elif cap <= 3:
                err = max(float(np.abs(X[b] - pr[b % fc.N_INST]["Q"]).max()) for b in range(fc.BATCH))
                print("%s cap %d %-8s %-16s |Q - Q_port| %.2e steps %s port %s rejected %d port %d"
                      % (tag, cap, path, NAMES[flag], err, steps, [r["iters"] for r in pr], rej, 3 * sum(r["rejected"] for r in pr)))
                assert err <= 1e-9, (tag, cap, path, NAMES[flag], err)
                assert steps == [r["iters"] for r in pr] and rej == 3 * sum(r["rejected"] for r in pr), (tag, cap, path)
            else:
                print("%s full  %-8s %-16s status %s f %s steps %s port %s" % (tag, path, NAMES[flag], res.status[: fc.N_INST].tolist(),
                                                                              res.f[: fc.N_INST].tolist(), steps, [r["iters"] for r in pr]))
                assert (res.status == 0).all(), (tag, path, res.status)
                for i in range(fc.N_INST):
                    assert pr[i]["status"] == 0 and abs(res.f[i] - pr[i]["f"]) <= 1e-9 * max(1.0, abs(pr[i]["f"])), (tag, path, i, res.f[i], pr[i]["f"])
                    assert abs(int(res.iters[i]) - pr[i]["iters"]) <= max(2, pr[i]["iters"] // 20), (tag, path, i, int(res.iters[i]), pr[i]["iters"])
                if c.variant != "plain":
                    lam = be.multipliers(fc.BATCH)
                    assert lam.min() >= 0.0
                    if ref_lam is None:
                        ref_lam = lam
                    # between paths: 1e-6 (test_cyclic_reduction_step_equals_the_serial_sweep); velocity rows 1e-3 (test_velocity_limited_arms_batch_both_
                    # sweeps_and_compaction: two elimination orders, each stopped at a reduced gradient of 1e-6)
                    assert np.abs(lam - ref_lam).max() <= (1e-6 if c.variant == "guarded" else 1e-3) * max(1.0, np.abs(ref_lam).max()), (tag, path)
                    for i in range(fc.N_INST):
                        if c.variant == "guarded":
                            lp = pr[i]["lam"]
                        else:
                            lp = np.zeros((c.T, 2 * c.n))
                            lp[: c.T - 1] = pr[i]["lam_v"]  # the velocity rows of knot t are those of dq_t
                        assert np.abs(lam[i] - lp).max() <= 1e-3 * max(1.0, lp.max()), (tag, path, i)
        be.close()


def test_every_chain_length_and_block_instantiation_has_a_case(robots_dir):
    """The chain lengths the family's kernels are instantiated for (OH_FREE_DISPATCH_N) and the block launchers' branches, read off oh_free.hip: each
    chain length is solved by a test of the suite, each block instantiation by a case of the table whose path runs it."""
    src = open(os.path.join(ROOT, "optas_amd", "csrc", "oh_free.hip")).read()
    macro = src[src.index("#define OH_FREE_DISPATCH_N") :]
    macro = macro[: macro.index("default:")]
    lengths = sorted(int(v) for v in re.findall(r"case (\d+):", macro))
    assert lengths == list(range(2, 9))
    covered = set(fc.NDOF.values()) | {OracleRobot(kin).ndof for _, kin, _, _ in chain_robots(robots_dir)}  # test_gpu_chain_lengths.py solves these
    assert covered >= set(lengths), (sorted(covered), lengths)
    block = sorted({int(v) for v in re.findall(r"if \(n == (\d+)\) launch_step_free_block<\1, false>", src)}
                   | {int(v) for v in re.findall(r"else if \(n == (\d+)\) launch_step_free_block<\1, false>", src)})
    guarded = re.search(r"if constexpr \(N == (\d+) \|\| N == (\d+)\)", src)
    assert block == [6, 7] and sorted(int(v) for v in guarded.groups()) == block
    assert re.search(r"if \(n != 7 \|\| nK > 128\) return false;", src) and "static_assert(N == 7" in src  # k_free_persist / k_step_free_bb: 7 joints
    ran = {}
    for case in fc.CASES:
        for path in paths_of(case):
            ran.setdefault((fc.NDOF[case[0]], case[1], expected_sweep(case, path), case[2] <= 64), []).append(case)
    for n in block:
        for variant in ("plain", "guarded", "vel"):  # <N, GUARD, VEL>
            assert (n, variant, CP, True) in ran, (n, variant, "k_step_free_cp")
            assert (n, variant, PCR, True) in ran and (n, variant, PCR, False) in ran, (n, variant, "k_step_free_pcr<64 | 128>")
            if n == 7:
                assert (n, variant, BB, True) in ran and (n, variant, BB, False) in ran, (variant, "k_step_free_bb")
    assert (7, "guarded", PERSIST, True) in ran and (7, "guarded", PERSIST, False) in ran
    for n in lengths:  # the serial sweep k_step_free<N, GUARD, VEL> of the table's robots
        if n in fc.NDOF.values():
            assert any(k[0] == n and k[2] == SERIAL for k in ran)
