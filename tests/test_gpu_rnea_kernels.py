"""oh_rnea (k_rnea<NB>), oh_rnea_jac (k_rnea_jac<N>), oh_rnea_hess (k_rnea_hess<N>) and oh_rnea_device at every chain length the library
instantiates (1 ... 8 joints) and on an arm that is no rigid-body chain (tests/dyn_robots.py).  The three kernels pack a wave differently -- one
sample per lane in 256-thread blocks, 64 / (3 N) samples of 3 N direction lanes, 64 / N samples of N joint lanes staged in LDS -- so the batch
sizes straddle each kernel's own wave (UPW samples) and block.  Every sample is graded against the float64 oracle (oracle/torque.py), and the
oracle's points against the 50-digit reference (oracle/rnea_mp.py).  Bit-for-bit checks catch what tolerances hide: a sample's result does not
depend on its position in the batch, on its neighbours' values (NaN / inf next door), or on what an earlier call left in the staging buffer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dyn_robots
from conftest import ROOT, SEED
from optas_amd import _lib
from optas_amd.models import RobotModel
from oracle.rnea_mp import rnea_ctau_hessian_mp, rnea_jacobian_mp, rnea_mp
from oracle.robot import OracleRobot
from oracle.torque import RneaTables, rnea_batch, rnea_ctau_hessian, rnea_jacobian

pytestmark = pytest.mark.gpu
TAGS = ["med1", "med2", "med3", "med4", "med5", "med6", "med7", "med8", "tester2", "awkward5"]
# the instantiations of the three kernels and the robot that runs each: k_rnea<NB> takes the body count (joints + 1)
INSTANTIATIONS = {f"k_rnea<{nd + 1}>": tag for nd, tag in enumerate(["med1", "med2", "med3", "med4", "med5", "med6", "med7", "med8"], 1)}
INSTANTIATIONS.update({f"k_rnea_jac<{nd}>": tag for nd, tag in enumerate(["med1", "tester2", "med3", "med4", "awkward5", "med6", "med7", "med8"], 1)})
INSTANTIATIONS.update({f"k_rnea_hess<{nd}>": tag for nd, tag in enumerate(["med1", "med2", "med3", "med4", "med5", "med6", "med7", "med8"], 1)})
RNEA_BLOCK = 256


def upw(kernel, nd):
    """Samples per 64-lane wave."""
    return {"rnea": 64, "jac": 64 // (3 * nd), "hess": 64 // nd}[kernel]


def sizes(kernel, nd):
    u = upw(kernel, nd)
    out = sorted({1, u - 1, u, u + 1, 2 * u + 1, 255, 256, 257, 4097})
    return out + [65537] if kernel == "rnea" else out


class Dyn:
    """One library handle with the robot's dynamics tables; samples are rows: q, qd, qdd, c (n, nd)."""

    def __init__(self, kin):
        self.lib = _lib.load()
        dyn = RobotModel(urdf_filename=kin).dynamics_tables()
        self.nd = dyn.ndof
        desc = _lib.oh_problem_desc(kind=_lib.OH_PROBLEM_KINEMATICS, ndof=max(1, min(dyn.ndof, _lib.OH_MAX_CHAIN)))
        self.h = C.c_void_p()
        _lib.check(self.lib.oh_create(C.byref(desc), C.byref(self.h)), "oh_create")
        _lib.check(self.lib.oh_set_dynamics(self.h, C.byref(dyn)), "oh_set_dynamics")

    def _args(self, *a):
        return [np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.nd) for x in a]

    def rnea(self, q, qd, qdd):
        A = self._args(q, qd, qdd)
        out = np.empty((A[0].shape[0], self.nd))
        _lib.check(self.lib.oh_rnea(self.h, out.shape[0], *map(_lib._ptr, A), _lib._ptr(out)), "oh_rnea")
        return out

    def jac(self, q, qd, qdd):
        A = self._args(q, qd, qdd)
        out = np.empty((A[0].shape[0], self.nd, 3 * self.nd))
        _lib.check(self.lib.oh_rnea_jac(self.h, out.shape[0], *map(_lib._ptr, A), _lib._ptr(out)), "oh_rnea_jac")
        return out

    def hess(self, q, qd, qdd, c):
        A = self._args(q, qd, qdd, c)
        out = np.empty((A[0].shape[0], 3 * self.nd, 3 * self.nd))
        _lib.check(self.lib.oh_rnea_hess(self.h, out.shape[0], *map(_lib._ptr, A), _lib._ptr(out)), "oh_rnea_hess")
        return out

    def call(self, kernel, q, qd, qdd, c):
        return self.rnea(q, qd, qdd) if kernel == "rnea" else self.jac(q, qd, qdd) if kernel == "jac" else self.hess(q, qd, qdd, c)

    def close(self):
        if self.h:
            self.lib.oh_destroy(self.h)
            self.h = None


@pytest.fixture(scope="module")
def kins(tmp_path_factory):
    return {tag: (kin, rigid) for tag, kin, rigid in dyn_robots.robots(tmp_path_factory.mktemp("robots"))}


@pytest.fixture
def robot(kins, request, hip_lib):
    kin, rigid = kins[request.param]
    d = Dyn(kin)
    yield request.param, d, RneaTables(OracleRobot(kin)), rigid
    d.close()


def _inputs(rng, n, nd, qs=2.0, qds=2.0, qdds=2.0):
    return rng.uniform(-qs, qs, (n, nd)), rng.uniform(-qds, qds, (n, nd)), rng.uniform(-qdds, qdds, (n, nd)), rng.normal(size=(n, nd))


def _per_sample(a, ref, tol, what):
    """|a - ref| <= tol max(1, |ref|) sample by sample (leading axis)."""
    a, ref = a.reshape(len(a), -1), ref.reshape(len(ref), -1)
    err = np.abs(a - ref).max(1) / np.maximum(1.0, np.abs(ref).max(1))
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, (what, "samples", bad[:16], err.max())


def _oracle(kernel, tb, q, qd, qdd, c):
    return {"rnea": lambda: rnea_batch(tb, q, qd, qdd), "jac": lambda: rnea_jacobian(tb, q, qd, qdd),
            "hess": lambda: rnea_ctau_hessian(tb, q, qd, qdd, c)}[kernel]()


TOL = {"rnea": 1e-12, "jac": 1e-10, "hess": 1e-10}


def _check_against_oracle(kernel, d, tb, q, qd, qdd, c, what):
    _per_sample(d.call(kernel, q, qd, qdd, c), _oracle(kernel, tb, q, qd, qdd, c), TOL[kernel], what)


@pytest.mark.parametrize("robot", TAGS, indirect=True)
def test_every_sample_of_every_batch_size_equals_the_oracle(robot):
    tag, d, tb, _ = robot
    rng = np.random.default_rng(SEED + 70)
    for kernel in ("rnea", "jac", "hess"):
        for n in sizes(kernel, d.nd):
            _check_against_oracle(kernel, d, tb, *_inputs(rng, n, d.nd), (tag, kernel, n))


@pytest.mark.parametrize("robot", TAGS, indirect=True)
def test_kernels_equal_the_mp_reference(robot):
    tag, d, tb, _ = robot
    for q, qd, qdd, c, hess in dyn_robots.mp_points(tag, d.nd):
        _per_sample(d.rnea(q, qd, qdd), rnea_mp(tb, q, qd, qdd)[None], TOL["rnea"], (tag, "rnea"))
        _per_sample(d.jac(q, qd, qdd), rnea_jacobian_mp(tb, q, qd, qdd)[None], TOL["jac"], (tag, "jac"))
        if hess:
            _per_sample(d.hess(q, qd, qdd, c), rnea_ctau_hessian_mp(tb, q, qd, qdd, c)[None], TOL["hess"], (tag, "hess"))


@pytest.mark.parametrize("robot", TAGS, indirect=True)
def test_results_do_not_depend_on_the_position_in_the_batch(robot):
    """A permuted batch of 2 UPW + 1 samples comes back permuted bit for bit, and every sample equals its own n = 1 call: no lane, LDS slot or
    grid index is shared between samples."""
    tag, d, tb, _ = robot
    rng = np.random.default_rng(SEED + 71)
    for kernel in ("rnea", "jac", "hess"):
        n = 2 * upw(kernel, d.nd) + 1
        A = _inputs(rng, n, d.nd)
        out = d.call(kernel, *A)
        perm = rng.permutation(n)
        assert np.array_equal(d.call(kernel, *(a[perm] for a in A)), out[perm]), (tag, kernel)
        for s in range(n):
            assert np.array_equal(d.call(kernel, *(a[s:s + 1] for a in A))[0], out[s]), (tag, kernel, s)


@pytest.mark.parametrize("robot", TAGS, indirect=True)
def test_a_nan_or_inf_sample_leaves_its_neighbours_alone(robot):
    tag, d, tb, _ = robot
    rng = np.random.default_rng(SEED + 72)
    for kernel in ("rnea", "jac", "hess"):
        u = upw(kernel, d.nd)
        n = 2 * u + 1
        A = _inputs(rng, n, d.nd)
        clean = d.call(kernel, *A)
        bad = [a.copy() for a in A]
        i, k = u // 2, min(u // 2 + 1, n - 1)  # two neighbours in the same wave
        bad[0][i, d.nd - 1] = np.nan
        bad[1][k, 0] = np.inf
        out = d.call(kernel, *bad)
        keep = np.setdiff1d(np.arange(n), [i, k])
        assert np.array_equal(out[keep], clean[keep]), (tag, kernel)
        assert not np.isfinite(out[i]).all() and not np.isfinite(out[k]).all(), (tag, kernel)


@pytest.mark.parametrize("robot", TAGS, indirect=True)
def test_structure_of_the_derivatives(robot):
    tag, d, tb, rigid = robot
    nd = d.nd
    rng = np.random.default_rng(SEED + 73)
    n = 2 * upw("hess", nd) + 1
    q, qd, qdd, c1 = _inputs(rng, n, nd)
    c2 = rng.normal(size=(n, nd))
    H1, H2 = d.hess(q, qd, qdd, c1), d.hess(q, qd, qdd, c2)
    scale = np.maximum(1.0, np.abs(H1).max((1, 2)))[:, None, None]
    assert np.all(np.abs(H1 - np.swapaxes(H1, 1, 2)) <= 1e-12 * scale), tag
    Q, D, A = slice(0, nd), slice(nd, 2 * nd), slice(2 * nd, 3 * nd)
    for H in (H1, H2):  # the kernel writes these entries as constants / copies
        assert not H[:, A, A].any() and not H[:, D, A].any() and not H[:, A, D].any(), tag
        assert np.array_equal(H[:, A, Q], np.swapaxes(H[:, Q, A], 1, 2)), tag
    a, b = 0.7, -1.3
    H12 = d.hess(q, qd, qdd, a * c1 + b * c2)
    lin = a * H1 + b * H2
    scale = np.maximum(1.0, np.maximum(np.abs(a * H1).max((1, 2)), np.abs(b * H2).max((1, 2))))[:, None, None]
    assert np.all(np.abs(H12 - lin) <= 1e-12 * scale), tag
    # the qdd block of J is the mass matrix: oh_rnea's differences in qdd (tau is affine in qdd)
    J = d.jac(q, qd, qdd)
    t0 = d.rnea(q, qd, np.zeros_like(qdd))
    M = np.stack([d.rnea(q, qd, np.tile(np.eye(nd)[j], (n, 1))) - t0 for j in range(nd)], 2)  # (n, nd, nd): column j
    _per_sample(J[:, :, A], M, 1e-12, (tag, "mass matrix"))
    if rigid:
        Ms = J[:, :, A]
        assert np.abs(Ms - np.swapaxes(Ms, 1, 2)).max() <= 1e-12 * max(1.0, np.abs(Ms).max()), tag
        assert np.linalg.eigvalsh(0.5 * (Ms + np.swapaxes(Ms, 1, 2))).min() > 0.0, tag


@pytest.mark.parametrize("robot", TAGS, indirect=True)
def test_extreme_inputs(robot):
    """q up to 1e3 rad (the kernels' own argument reduction against numpy's), qd up to 50 rad/s, qdd up to 500."""
    tag, d, tb, _ = robot
    rng = np.random.default_rng(SEED + 74)
    for kernel in ("rnea", "jac", "hess"):
        n = 257
        A = _inputs(rng, n, d.nd, 1e3, 50.0, 500.0)
        A[0][:8] = np.array([1e3, -1e3, 999.99, -777.5, 0.5 * np.pi * 601, -np.pi * 300, 1e3 - 1e-9, 2.0 ** 9])[:, None]
        _check_against_oracle(kernel, d, tb, *A, (tag, kernel, "extreme"))


@pytest.mark.parametrize("robot", TAGS, indirect=True)
def test_staging_buffer_reuse(robot, kins):
    """4097, then 5, then 4097 fresh samples on one handle: each answer is the fresh handle's bit for bit (nothing of an earlier, larger or
    smaller, call reaches the output)."""
    tag, d, tb, _ = robot
    rng = np.random.default_rng(SEED + 75)
    fresh = Dyn(kins[tag][0])
    try:
        for kernel in ("rnea", "jac", "hess"):
            for n in (4097, 5, 4097):
                A = _inputs(rng, n, d.nd)
                assert np.array_equal(d.call(kernel, *A), fresh.call(kernel, *A)), (tag, kernel, n)
                fresh.close()
                fresh = Dyn(kins[tag][0])
    finally:
        fresh.close()


@pytest.mark.parametrize("robot", TAGS, indirect=True)
def test_rnea_device_inside_nan_guards(robot):
    """oh_rnea_device on caller-owned device buffers, each padded front and back with a NaN guard of one block: tau equals oh_rnea bit for bit,
    the guards are untouched, and the guard NaNs never reach the result."""
    tag, d, tb, _ = robot
    nd = d.nd
    rng = np.random.default_rng(SEED + 76)
    g = RNEA_BLOCK * nd  # guard doubles on each side
    for n in (1, 257, 4097):
        A = _inputs(rng, n, nd)[:3]
        bufs = []
        for a in A + (np.full((n, nd), np.nan),):
            padded = np.concatenate([np.full(g, np.nan), a.reshape(-1), np.full(g, np.nan)])
            bufs.append((_lib.DeviceBuffer(padded.nbytes).upload(padded), padded))
        try:
            base = [b.ptr.value + 8 * g for b, _ in bufs]
            _lib.check(d.lib.oh_rnea_device(d.h, n, *[C.c_void_p(p) for p in base]), "oh_rnea_device")
            back = [b.download(np.float64, p.shape) for b, p in bufs]
            tau = back[3][g:g + n * nd].reshape(n, nd)
            assert np.array_equal(tau, d.rnea(*A)), (tag, n)
            for (b, p), r in zip(bufs, back):
                assert np.isnan(r[:g]).all() and np.isnan(r[g + n * nd:]).all(), (tag, n)
                if b is not bufs[3][0]:
                    assert np.array_equal(r, p, equal_nan=True), (tag, n)
        finally:
            for b, _ in bufs:
                b.free()


def test_every_launcher_instantiation_is_run(kins):
    """The launchers' instantiations, read from the sources, are exactly INSTANTIATIONS, and each one's robot has the chain length it needs: a new
    instantiation without a robot here fails."""
    src = open(os.path.join(ROOT, "optas_amd", "csrc", "oh_rnea.hip")).read()
    macro = src[src.index("#define OH_RNEA_DISPATCH("):]
    macro = macro[: macro.index("default: return false;")]
    cases = [(int(nb), int(nj)) for nb, nj in re.findall(r"case (\d+): C\((\d+)\); break;", macro)]
    assert cases and all(nb == nj + 1 for nb, nj in cases), cases
    found = set()
    for name in ("rnea", "rnea_jac", "rnea_hess"):
        launcher = src[src.index(f"bool oh_launch_{name}("):]
        launcher = launcher[: launcher.index("\n}\n")]
        kernel, extra = re.search(r"#define C\(NN\) hipLaunchKernelGGL\((k_\w+)<NN( \+ 1)?>", launcher).groups()
        assert kernel == f"k_{name}" and "OH_RNEA_DISPATCH(nbodies, C)" in launcher, launcher
        found |= {f"{kernel}<{nj + (1 if extra else 0)}>" for _, nj in cases}
    assert found == set(INSTANTIATIONS), sorted(found ^ set(INSTANTIATIONS))
    for name, tag in INSTANTIATIONS.items():
        assert tag in TAGS
        nd = RneaTables(OracleRobot(kins[tag][0])).ndof
        want = int(re.search(r"<(\d+)>", name).group(1)) - (1 if name.startswith("k_rnea<") else 0)
        assert nd == want, (name, tag, nd)
