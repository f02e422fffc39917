"""Large planted QPs (tests/qp_planted_large.py) on the CPU: the construction is exact, the numpy port (oracle/qp_ipm.py) reaches every planted
optimum with the recorded errors and iteration counts -- the figures the GPU bounds of tests/test_gpu_qp_block.py are set from -- the library
accepts sizes up to (128, 1024, 128), and the lowering hands such problems to the dense QP family only when asked to."""
import ctypes as C

import numpy as np
import pytest

import qp_planted_large as L


@pytest.mark.parametrize("name", list(L.CLASSES))
def test_port_reaches_the_planted_optimum(name):
    a = L.CLASSES[name]
    assert L.is_large(a["n"], a["m"], a["me"]) and a["n"] <= L.LIMITS[0] and a["m"] <= L.LIMITS[1] and a["me"] <= min(L.LIMITS[2], a["n"])
    worst, its, sts = L.port_results(name)
    print(f"{name}: port max |x - x*| {worst[0]:.3e}  rel |f - f*| {worst[1]:.3e}  multipliers {worst[2]:.3e}  (recorded {L.PORT_ERR[name]})  iters {its}")
    assert set(sts) == {0} and max(its) <= 29
    # the recorded figures are this measurement; another BLAS may associate sums differently, so the port is held to what the kernel is held to:
    # the bounds, and counts that differ only where a stopping test sits within rounding of the tolerance
    assert (worst <= np.array(L.bound(name))).all()
    assert np.abs(np.array(its) - np.array(L.PORT_ITERS[name])).max() <= 2
    for qp in L.planted_instances(name):  # the class's properties hold for every instance
        assert (qp["sigma"] == 0).sum() == a["na"] and (qp["lam"] > 0).sum() == a["na"]
        assert np.linalg.matrix_rank(0.5 * (qp["P"] + qp["P"].T)) == a.get("rank", a["n"])
        assert np.linalg.matrix_rank(qp["A"]) == a["me"] if a["me"] else True
        assert (np.abs(qp["K"]).max() > 0 and (qp["K"] == -qp["K"].T).all()) == bool(a.get("skew"))


@pytest.mark.parametrize("name", list(L.CLASSES))
def test_planted_data_is_exact(name):
    L.check_exact(L.planted_instances(name)[0])


def test_class_table_and_seeds():
    assert list(L.CLASSES) == ["n33", "n48_m257", "n64", "n65_me33", "me_eq_n_40", "vertex_48", "lp_eq_40", "rank_def_64", "nonsym_64", "n96", "n128_max",
                               "n128_me128", "n128_inactive"]
    assert L._SEED0["n33"] == 50000 and L._SEED0["n128_inactive"] == 62000 and L.N_INST == 12
    assert set(L.PORT_ERR) == set(L.CLASSES) == set(L.PORT_ITERS) and all(len(v) == 12 for v in L.PORT_ITERS.values())
    assert L.bound("me_eq_n_40")[:2] == (1e-10, 1e-10) and L.bound("n33")[2] == pytest.approx(6.515e-8) and L.bound("vertex_48")[2] == 1e-8
    import qp_planted as Q

    assert not set(L.CLASSES) & set(Q.CLASSES)  # the existing table is what the existing GPU test parametrises over


def _create(n, m, me):
    from optas_amd import _lib

    lib = _lib.load()
    desc = _lib.oh_qp_desc(n=n, m=m, me=me, max_iter=100, tol=1e-9)
    h = C.c_void_p()
    rc = lib.oh_create_qp(C.byref(desc), C.byref(h))
    if rc == _lib.OH_OK:
        lib.oh_destroy(h)
    return rc


def test_create_qp_accepts_the_new_limits():
    from optas_amd import _lib

    for n, m, me in ((128, 1024, 128), (33, 0, 0), (1, 257, 0), (40, 0, 40)):
        assert _create(n, m, me) in (_lib.OH_OK, _lib.OH_ERR_HIP), (n, m, me)  # OH_ERR_HIP: no device here; never OH_ERR_INVALID


def test_create_qp_refuses_beyond_the_limits():
    from optas_amd import _lib

    for n, m, me in ((129, 0, 0), (128, 1025, 0), (128, 0, 129), (40, 0, 41), (0, 0, 0)):
        assert _create(n, m, me) == _lib.OH_ERR_INVALID, (n, m, me)
    assert "128" in _lib.load().oh_last_error().decode() and "1024" in _lib.load().oh_last_error().decode()


def test_mpc_problem_lowers_to_the_qp_family_only_on_request():
    from optas_amd import _lib
    from optas_amd.lowering import QP_LIMITS, QP_LIMITS_LARGE, QpSpec, lower
    from optas_amd.optimization import QuadraticCostLinearConstraints

    o = L.mpc_problem()
    assert isinstance(o, QuadraticCostLinearConstraints) and (o.nx, o.nk, o.na, o.np) == (72, 144, 39, 6)
    assert QP_LIMITS == L.SMALL and QP_LIMITS_LARGE == L.LIMITS
    assert lower(o)[0] == _lib.OH_PROBLEM_TAPE
    kind, spec = lower(o, QP_LIMITS_LARGE)
    assert kind == _lib.OH_PROBLEM_QP and isinstance(spec, QpSpec) and (spec.n, spec.m, spec.me) == (72, 144, 39)
    kind, spec = lower(o, (72, 144, 39))
    assert kind == _lib.OH_PROBLEM_QP
    assert lower(o, (71, 144, 39))[0] == lower(o, (72, 143, 39))[0] == lower(o, (72, 144, 38))[0] == _lib.OH_PROBLEM_TAPE


def test_default_lowering_of_a_63_variable_qp_is_unchanged():
    """The velocity-limit problem of test_guarded_cpu.py: QuadraticCostLinearConstraints with nx = 63, nk = 56, na = 0 -- the tape family by default."""
    import optas_amd
    from optas_amd import _lib
    from optas_amd.builder import OptimizationBuilder
    from optas_amd.lowering import QP_LIMITS_LARGE, lower
    from optas_amd.optimization import QuadraticCostLinearConstraints

    r = optas_amd.RobotModel.builtin("kuka_lwr", time_derivs=[0, 1])
    b = OptimizationBuilder(T=5, robots=[r])
    b.enforce_model_limits(r.get_name(), time_deriv=1)
    o = b.build()
    assert isinstance(o, QuadraticCostLinearConstraints) and (o.nx, o.nk, o.na) == (63, 56, 0)
    assert lower(o)[0] == _lib.OH_PROBLEM_TAPE
    assert lower(o, QP_LIMITS_LARGE)[0] == _lib.OH_PROBLEM_QP


def test_mpc_problem_on_the_port():
    """The port converges on six draws of the MPC problem's parameters within max_iter = 100, with a row binding in some of them."""
    from oracle.qp_ipm import solve_qp_ipm

    o = L.mpc_problem()
    pv = L.mpc_parameters(np.random.default_rng(50000), 6)
    binding = 0
    for p in pv:
        r = solve_qp_ipm(o.P(p), o.q(p), o.M(p), o.c(p), o.A(p), o.b(p), max_iter=100)
        assert r["status"] == 0
        binding += int((r["lam"] > 1e-6).any())
    assert binding > 0
