"""k_qp_solve_block (optas_amd/csrc/oh_qp_block.hip), one workgroup per instance of a dense QP: planted optima beyond the old limits
(tests/qp_planted_large.py) held to 10 times the error the numpy port leaves on the same instances and to its iteration counts; the kernel
forced (qp_mode 3) on the small classes of tests/qp_planted.py against the automatic path; bad instances beside good ones; a handle reused at
several batch sizes; a 72-variable linear MPC through HIPSolver's option dense_qp with device assembly (k_qp_assemble_block); the code object."""
import numpy as np
import pytest

import qp_planted as Q
import qp_planted_large as L

CERTIFIED = {"n128_max": (0,), "n33": (0, 7), "n65_me33": (0, 7), "vertex_48": (0, 7)}


def _solve(be, rows, n, mode=-1):
    be.set_option("qp_mode", mode)
    B = rows.shape[0]
    r = be.solve(np.zeros((B, n)), rows)
    lam, nu = be.multipliers(B)
    return r, lam.copy(), nu.copy()


def _same_bits(a, b, keep=slice(None)):
    (ra, la, na), (rb, lb, nb) = a, b
    return all((x[keep] == y[keep]).all() for x, y in ((ra.x, rb.x), (ra.f, rb.f), (ra.kkt, rb.kkt), (ra.iters, rb.iters), (ra.status, rb.status), (la, lb), (na, nb)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(L.CLASSES))
def test_planted_optimum_on_every_large_class(hip_lib, name):
    from optas_amd.backend import QPBackend

    a = L.CLASSES[name]
    n, m, me = a["n"], a["m"], a["me"]
    qps = L.planted_instances(name)
    packed = np.stack([L.pack(qp) for qp in qps])
    bx, bf, bm = L.bound(name)
    be = QPBackend(n, m, me)
    for B in (70, 1, 3):
        idx = np.arange(B) % L.N_INST
        r, lam, nu = _solve(be, packed[idx], n, {70: -1, 1: 0, 3: 2}[B])  # a forced 0 / 1 / 2 does not fit a large handle and falls back to the block kernel
        assert be.flag("qp_block") == 1
        worst = np.max([L.errors(qps[idx[i]], r.x[i], r.f[i], lam[i], nu[i]) for i in range(B)], axis=0)
        dit = np.abs(r.iters - np.array(L.PORT_ITERS[name])[idx]).max()
        print(f"{name} B={B}: iters <= {r.iters.max()} (port's +- {dit})  |x - x*| {worst[0]:.3e} / {bx:.3e}  rel |f - f*| {worst[1]:.3e} / {bf:.3e}"
              f"  multipliers {worst[2]:.3e} / {bm:.3e}")
        assert (r.status == 0).all(), (B, np.flatnonzero(r.status).tolist())
        assert worst[0] <= bx and worst[1] <= bf and worst[2] <= bm, B
        assert dit <= 2, (B, r.iters.tolist())  # the same iteration: counts differ only where a stopping test sits within rounding of the tolerance
        if B == 70:  # the returned point and the reported residuals against the 50-digit certificate
            for i in CERTIFIED.get(name, ()):
                L.assert_certificate(L.kkt_certificate(qps[i], r.x[i], lam[i], nu[i]), r.kkt[i])
    be.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["base", "n1", "n1_eq", "m256", "m65", "me_eq_n", "lp", "rank_def", "nonsym", "max"])
def test_block_kernel_forced_on_the_small_classes(hip_lib, name):
    from optas_amd.backend import QPBackend

    a = Q.CLASSES[name]
    n, m, me = a["n"], a["m"], a["me"]
    qps = Q.planted_batch(name, 70)
    rows = np.stack([Q.pack(qp) for qp in qps])
    bx, bf, bm = Q.bound(name)
    be = QPBackend(n, m, me)
    ra, _, _ = _solve(be, rows, n, -1)
    assert be.flag("qp_block") == 0  # the automatic choice of a handle within the old limits is a thread or a wavefront per instance
    r, lam, nu = _solve(be, rows, n, 3)
    assert be.flag("qp_block") == 1
    worst = np.max([Q.errors(qps[i], r.x[i], r.f[i], lam[i], nu[i]) for i in range(70)], axis=0)
    dit = np.abs(r.iters - ra.iters).max()
    print(f"{name} qp_mode=3: iters <= {r.iters.max()} (automatic path's +- {dit})  |x - x*| {worst[0]:.3e} / {bx:.3e}  rel |f - f*| {worst[1]:.3e} / {bf:.3e}"
          f"  multipliers {worst[2]:.3e} / {bm:.3e}")
    assert (ra.status == 0).all() and (r.status == 0).all()
    assert worst[0] <= bx and worst[1] <= bf and worst[2] <= bm
    assert dit <= 2
    be.close()


@pytest.mark.gpu
def test_bad_instances_leave_their_batch_alone(hip_lib):
    from optas_amd.backend import QPBackend

    n, m, me = (L.CLASSES["n33"][k] for k in ("n", "m", "me"))
    be = QPBackend(n, m, me)
    clean = np.stack([L.pack(qp) for qp in L.planted_batch("n33", 70)])
    ref = _solve(be, clean, n)
    assert (ref[0].status == 0).all()
    pos = (0, 37, 69)
    rows = clean.copy()
    for p, bad in zip(pos, Q.bad_instances(L.planted_instances("n33")[0])):  # contradictory rows, unbounded, a nan
        rows[p] = bad
    got = _solve(be, rows, n)
    assert (got[0].status[list(pos)] != 0).all(), got[0].status[list(pos)]
    assert _same_bits(got, ref, np.setdiff1d(np.arange(70), pos))
    be.close()


@pytest.mark.gpu
def test_capacity_and_two_handles(hip_lib):
    from optas_amd.backend import QPBackend

    a = L.CLASSES["n65_me33"]
    n, m, me = a["n"], a["m"], a["me"]
    rows = np.stack([L.pack(qp) for qp in L.planted_batch("n65_me33", 70)])
    be = QPBackend(n, m, me)
    first = _solve(be, rows[:3], n)
    other = QPBackend(33, 40, 4)  # a second large handle alive beside the first
    rows33 = np.stack([L.pack(qp) for qp in L.planted_batch("n33", 5)])
    r33 = _solve(other, rows33, 33)
    grown = _solve(be, rows, n)
    again = _solve(be, rows[:3], n)
    r33b = _solve(other, rows33, 33)
    assert (grown[0].status == 0).all() and (r33[0].status == 0).all()
    assert _same_bits(first, again) and _same_bits(first, grown, slice(0, 3)) and _same_bits(r33, r33b)
    bx = L.bound("n33")[0]
    assert max(np.abs(r33[0].x[i] - L.planted_instances("n33")[i]["x"]).max() for i in range(5)) <= bx
    be.close()
    other.close()


@pytest.mark.gpu
def test_linear_mpc_through_hipsolver(hip_lib):
    from optas_amd.backend import EliminatedTapeBackend, QPBackend, TapeBackend
    from optas_amd.solver import HIPSolver

    o = L.mpc_problem()
    dev = HIPSolver(o).setup("hip_sqp", {"dense_qp": True})
    host = HIPSolver(o).setup("hip_sqp", {"dense_qp": True, "device_assembly": False})
    tape = HIPSolver(o).setup("hip_sqp")
    assert isinstance(dev.backend.be, QPBackend) and isinstance(host.backend.be, QPBackend) and isinstance(tape.backend, (TapeBackend, EliminatedTapeBackend))
    assert dev.backend.be.tape is not None and host.backend.be.tape is None
    assert (dev.backend.be.n, dev.backend.be.m, dev.backend.be.me) == (72, 144, 39)
    rng = np.random.default_rng(50000)
    pv = L.mpc_parameters(rng, 70)
    x0 = np.zeros((70, o.nx))
    rd, rh = dev.solve_batch_arrays(x0[:3], pv[:3]), host.solve_batch_arrays(x0[:3], pv[:3])
    lam_d, nu_d = (v.copy() for v in dev.backend.be.multipliers(3))
    assert (rd.status == 0).all() and (rh.status == 0).all()
    assert np.abs(rd.x - rh.x).max() < 1e-9 and np.abs(rd.f - rh.f).max() < 1e-9 * max(1.0, np.abs(rh.f).max())
    for b in range(3):
        qp = dict(P=o.P(pv[b]), q=o.q(pv[b]), M=o.M(pv[b]), c=o.c(pv[b]), A=o.A(pv[b]), b=o.b(pv[b]))
        L.assert_certificate(L.kkt_certificate(qp, rd.x[b], lam_d[b], nu_d[b]), rd.kkt[b])
        assert abs(rd.f[b] - o.f(rd.x[b], pv[b])) < 1e-9 * max(1.0, abs(rd.f[b]))  # the constant term f(0, p) included
    # the same problem on the default path (tape family): its tolerance, with slack for its 1e-6 stopping rule
    rt = tape.solve_batch_arrays(x0[:3], pv[:3])
    print("f dense_qp", rd.f, "tape family", rt.f, "iters", rd.iters, rt.iters)
    assert (np.abs(rt.f - rd.f) <= 1e-5 * np.abs(rd.f)).all()
    # B = 70: device assembly alone, the first three instances as before
    r70 = dev.solve_batch_arrays(x0, pv)
    lam70, _ = dev.backend.be.multipliers(70)
    assert (r70.status == 0).all(), np.flatnonzero(r70.status).tolist()
    assert np.abs(r70.x[:3] - rh.x).max() < 1e-9 and np.abs(r70.f[:3] - rh.f).max() < 1e-9 * max(1.0, np.abs(rh.f).max())
    assert (lam70 > 1e-6).any()  # some row binds
    for s in (dev, host, tape):
        s.backend.close()


@pytest.mark.gpu
def test_kernel_info(hip_lib):
    from optas_amd import _lib

    info = _lib.kernel_info("k_qp_solve_block")
    print(info)
    assert 0 < info["lds_bytes_per_block"] <= 160 * 1024 and info["block"] == 256  # LDS at the largest sizes
