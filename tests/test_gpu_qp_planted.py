"""Dense QP kernels (optas_amd/csrc/oh_qp.hip) against planted optima (tests/qp_planted.py): every class on every launch path -- k_qp_solve<0>,
<1>, <2> forced and chosen automatically, k_qp_solve_wave with m <= 64 and m > 64 -- held to 10 times the error the numpy port leaves on the
same instances (measured on the CPU, tests/test_qp_planted_cpu.py); the returned (x, lam, nu) and the reported kkt triple against a 50-digit
KKT certificate; instances that cannot be solved leave the rest of their batch alone; device assembly with two passes of the probe loop."""
import numpy as np
import pytest

import qp_planted as Q
from conftest import SEED


def _solve(be, rows, n, mode=-1):
    be.set_option("qp_mode", mode)
    B = rows.shape[0]
    r = be.solve(np.zeros((B, n)), rows)
    lam, nu = be.multipliers(B)
    return r, lam.copy(), nu.copy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(Q.CLASSES))
def test_planted_optimum_on_every_path(hip_lib, name):
    from optas_amd.backend import QPBackend

    a = Q.CLASSES[name]
    n, m, me = a["n"], a["m"], a["me"]
    qps = Q.planted_batch(name, 70)
    rows = np.stack([Q.pack(qp) for qp in qps])
    bx, bf, bm = Q.bound(name)
    be = QPBackend(n, m, me)
    runs = [(70, mode) for mode in (-1, 0, 1, 2) if mode < 0 or Q.forced_fits(n, m, me, mode)] + [(B, -1) for B in Q.GPU_BATCHES[1:]]
    thread, wave = [], []
    for B, mode in runs:
        r, lam, nu = _solve(be, rows[:B], n, mode)
        path = Q.launch_path(n, m, me, B, mode)
        worst = np.max([Q.errors(qps[i], r.x[i], r.f[i], lam[i], nu[i]) for i in range(B)], axis=0)
        print(f"{name} B={B} qp_mode={mode} {path}: iters <= {r.iters.max()}  |x - x*| {worst[0]:.3e} / {bx:.3e}  rel |f - f*| {worst[1]:.3e} / {bf:.3e}"
              f"  multipliers {worst[2]:.3e} / {bm:.3e}")
        assert (r.status == 0).all(), (B, mode, np.flatnonzero(r.status).tolist())
        assert worst[0] <= bx and worst[1] <= bf and worst[2] <= bm, (B, mode, path)
        (wave if path[0] == "wave" else thread).append((B, mode, r, lam, nu))
        # the returned point and the reported residuals against the 50-digit certificate
        for i in sorted({0, 17, 69} & set(range(B))) if (B, mode) in ((70, -1), (40, -1)) else ():
            Q.assert_certificate(Q.kkt_certificate(qps[i], r.x[i], lam[i], nu[i]), r.kkt[i])
    # the thread paths differ only in where the work set lives: the same bits
    _, _, r0, lam0, nu0 = thread[0]
    for B, mode, r, lam, nu in thread[1:]:
        assert (r.x == r0.x[:B]).all() and (r.f == r0.f[:B]).all() and (r.iters == r0.iters[:B]).all(), (B, mode)
    # the wavefront path associates its sums differently: the tolerances of test_qp.test_dense_qp_kernel_matches_port
    for B, mode, r, lam, nu in wave:
        assert (r.iters == r0.iters[:B]).all()
        assert np.abs(r.x - r0.x[:B]).max() < 1e-9 and np.abs(r.f - r0.f[:B]).max() < 1e-9 * max(1.0, np.abs(r0.f).max())
        assert np.abs(lam - lam0[:B]).max(initial=0.0) < 1e-7 and np.abs(nu - nu0[:B]).max(initial=0.0) < 1e-7
    be.close()


@pytest.mark.gpu
def test_bad_instances_leave_their_batch_alone(hip_lib):
    from optas_amd.backend import QPBackend

    n, m, me = (Q.CLASSES["base"][k] for k in ("n", "m", "me"))
    be = QPBackend(n, m, me)
    bad = Q.bad_instances(Q.planted_instances("base")[0])
    for B, mode in ((70, -1), (70, 0), (70, 1), (64, -1)):  # 16, 64, 32 instances per block; a wavefront per instance
        path = Q.launch_path(n, m, me, B, mode)
        assert path == {(70, -1): ("thread", 2, 16), (70, 0): ("thread", 0, 64), (70, 1): ("thread", 1, 32), (64, -1): ("wave", 64)}[(B, mode)]
        clean = np.stack([Q.pack(qp) for qp in Q.planted_batch("base", B)])
        rc, lc, nc = _solve(be, clean, n, mode)
        assert (rc.status == 0).all()
        pos = (0, 37, 63)  # first lane of the first block, a lane inside a block, last lane of a block (at 16, 32 and 64 per block alike)
        for rot in range(3):
            rows = clean.copy()
            for k, p in enumerate(pos):
                rows[p] = bad[(k + rot) % 3]
            r, lam, nu = _solve(be, rows, n, mode)
            assert (r.status[list(pos)] != 0).all(), (B, mode, rot, r.status[list(pos)])
            keep = np.setdiff1d(np.arange(B), pos)
            for got, ref in ((r.x, rc.x), (r.f, rc.f), (r.kkt, rc.kkt), (r.iters, rc.iters), (r.status, rc.status), (lam, lc), (nu, nc)):
                assert (got[keep] == ref[keep]).all(), (B, mode, rot)
    be.close()


@pytest.mark.gpu
def test_device_assembly_with_two_probe_passes(hip_lib):
    from optas_amd.solver import HIPSolver

    o = Q.parametric_qp()
    dev = HIPSolver(o).setup("hip_sqp")
    host = HIPSolver(o).setup("hip_sqp", {"device_assembly": False})
    assert dev.backend.be.tape is not None and host.backend.be.tape is None
    assert 10 in list(dev.backend.be.tape.op)  # ATAN2 is on the tape
    rng = np.random.default_rng(SEED + 13)
    active = 0
    for B in (3, 64, 70):  # k_qp_assemble_par (a block per instance, 91 probes in two passes) for B <= 64, k_qp_assemble beyond
        pv = rng.uniform(0.5, 1.5, (B, 4))
        x0 = np.zeros((B, o.nx))
        rd, rh = dev.solve_batch_arrays(x0, pv), host.solve_batch_arrays(x0, pv)
        (lam_d, nu_d), (lam_h, nu_h) = dev.backend.be.multipliers(B), host.backend.be.multipliers(B)
        assert (rd.status == 0).all() and (rh.status == 0).all()
        assert np.abs(rd.x - rh.x).max() < 1e-9 and np.abs(rd.f - rh.f).max() < 1e-9 * np.abs(rh.f).max()
        active += int((lam_h > 1e-6).sum())
        for b in sorted({0, 1, B - 1}):
            qp = dict(P=o.P(pv[b]), q=o.q(pv[b]), M=o.M(pv[b]), c=o.c(pv[b]), A=o.A(pv[b]), b=o.b(pv[b]))
            Q.assert_certificate(Q.kkt_certificate(qp, rd.x[b], lam_d[b], nu_d[b]), rd.kkt[b])
            Q.assert_certificate(Q.kkt_certificate(qp, rh.x[b], lam_h[b], nu_h[b]), rh.kkt[b])
            assert abs(rd.f[b] - o.f(rd.x[b], pv[b])) < 1e-9 * max(1.0, abs(rd.f[b]))  # the constant term f(0, p) included
    assert active > 0  # some inequality rows bind
    dev.backend.close()
    host.backend.close()
