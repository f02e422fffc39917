"""k_link_kin (oh_link_kin*) through the C ABI and through RobotModel against the literal oracle (tests/link_kin_ref.py): kinematics of a link in
the frame of a base link -- position, rotation, quaternion, rpy, geometric and analytical Jacobian, axis.  Tolerances: 1e-12 absolute (the
project's FK tolerance), roll and yaw modulo 2 pi, and 1e-11 on d rpy / d q, whose partial derivatives amplify a quaternion error by at most
1 / cos^2(pitch) ~ 10 at the |sinp| <= 0.95 the inputs are drawn with."""
import ctypes as C

import numpy as np
import pytest

import link_kin_ref as ref
from conftest import KUKA_KIN, MED7_KIN, SEED
from optas_amd import _lib
from optas_amd.models import LinkFrameHandle, RobotModel

pytestmark = pytest.mark.gpu
NAMES = ("pos", "rot", "quat", "rpy", "axis", "Jg", "Ja")
SENTINEL = -7.25e300
PAD = 64


def components(ndof):
    return {"pos": 3, "rot": 9, "quat": 4, "rpy": 3, "axis": 3, "Jg": 6 * ndof, "Ja": 6 * ndof}


def shaped(flat: dict, n: int, ndof: int) -> dict:
    """n-by-components arrays -> the shapes of the reference (rot n x 3 x 3, Jacobians n x 6 x ndof)."""
    shp = {"rot": (n, 3, 3), "Jg": (n, 6, ndof), "Ja": (n, 6, ndof)}
    return {k: a.reshape(shp.get(k, a.shape)) for k, a in flat.items()}


def host_call(handle, Q, names, axis3=ref.AXIS3):
    """oh_link_kin with the outputs `names`, each host buffer followed by PAD sentinel doubles that must survive.  -> n-by-components arrays."""
    n, ndof = Q.shape
    comp = components(ndof)
    bufs = {k: np.full(n * comp[k] + PAD, SENTINEL) for k in names}
    out = _lib.oh_link_out(**{k: _lib._ptr(a) for k, a in bufs.items()})
    a3 = np.ascontiguousarray(axis3, dtype=np.float64) if "axis" in names else None
    _lib.check(_lib.load().oh_link_kin(handle._h, n, _lib._ptr(np.ascontiguousarray(Q)), _lib._ptr(a3), C.byref(out)), "oh_link_kin")
    for k, a in bufs.items():
        assert np.all(a[n * comp[k]:] == SENTINEL), f"oh_link_kin wrote past the end of {k}"
        assert not np.any(a[: n * comp[k]] == SENTINEL), f"oh_link_kin left part of {k} unwritten"
    return {k: a[: n * comp[k]].reshape(n, comp[k]) for k, a in bufs.items()}


def device_call(handle, Q, names, axis3=ref.AXIS3):
    """oh_link_kin_device (structure of arrays) with padded, sentinel-filled device buffers.  -> n-by-components arrays."""
    n, ndof = Q.shape
    comp = components(ndof)
    dq = _lib.DeviceBuffer(Q.nbytes).upload(np.ascontiguousarray(Q.T))
    dev = {k: _lib.DeviceBuffer((n * comp[k] + PAD) * 8).upload(np.full(n * comp[k] + PAD, SENTINEL)) for k in names}
    out = _lib.oh_link_out(**{k: b.ptr for k, b in dev.items()})
    a3 = np.ascontiguousarray(axis3, dtype=np.float64) if "axis" in names else None
    try:
        _lib.check(_lib.load().oh_link_kin_device(handle._h, n, dq.ptr, _lib._ptr(a3), C.byref(out)), "oh_link_kin_device")
        res = {}
        for k, b in dev.items():
            a = b.download(np.float64, (n * comp[k] + PAD,))
            assert np.all(a[n * comp[k]:] == SENTINEL), f"oh_link_kin_device wrote past the end of {k}"
            assert not np.any(a[: n * comp[k]] == SENTINEL), f"oh_link_kin_device left part of {k} unwritten"
            res[k] = np.ascontiguousarray(a[: n * comp[k]].reshape(comp[k], n).T)
        return res
    finally:
        for b in [dq] + list(dev.values()):
            b.free()


@pytest.fixture(scope="module")
def robots(hip_lib):
    return {name: RobotModel(urdf_filename=kin) for name, kin in ref.KINS.items()}


@pytest.mark.parametrize("index", range(len(ref.CASES)), ids=["-".join(c) for c in ref.CASES])
def test_parity_with_oracle_on_every_output(hip_lib, robots, index):
    """One call per (link, base) pair with all seven outputs; every kept unit is compared."""
    robot, link, base = ref.CASES[index]
    Q = ref.case_inputs(index)
    n, ndof = Q.shape
    got = shaped(host_call(robots[robot]._frames(link, base), Q, NAMES), n, ndof)
    want = ref.case_reference(index)
    ref.assert_outputs_match(got, want, f"{robot} {link} in {base}:")
    assert np.array_equal(got["Ja"][:, :3], got["Jg"][:, :3])
    if (robot, link, base) in (("tester", "eff", "link2"), ("tester", "link2", "eff")):
        assert not got["Ja"][:, 3:].any()  # only the prismatic joint lies between the two: the relative rotation is constant, d rpy / d q exactly zero


def stacked(v):
    """What a RobotModel method returns (vector, 3-by-n / 4-by-n array, matrix or list of matrices) with the configurations along axis 0."""
    if isinstance(v, list):
        return np.stack(v)
    return v.T if v.ndim == 2 and v.shape[0] in (3, 4) and v.shape[1] == 5 else v


@pytest.mark.parametrize("index", [i for i, c in enumerate(ref.CASES) if c[0] == "kuka"], ids=lambda i: "-".join(ref.CASES[i]))
def test_python_layer_matches_references(hip_lib, robots, index):
    """Every new and every rerouted RobotModel method, and its *_function form, for a 1-D q and a 7-by-5 q: values and shapes."""
    _, link, base = ref.CASES[index]
    rm = robots["kuka"]
    root = rm.get_root_link()
    want = ref.case_reference(index)
    T = np.zeros((ref.N_CONFIGS, 4, 4))
    T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = want["rot"], want["pos"], 1.0
    a3 = ref.AXIS3
    # (method, arguments after q -- also those of the *_function form after the link --, reference, key of the tolerance, shape for a 1-D q)
    table = [
        ("get_link_transform", (base,), T, "pos", (4, 4)),
        ("get_link_position", (base,), want["pos"], "pos", (3,)),
        ("get_link_rotation", (base,), want["rot"], "rot", (3, 3)),
        ("get_link_quaternion", (base,), want["quat"], "quat", (4,)),
        ("get_link_rpy", (base,), want["rpy"], "rpy", (3,)),
        ("get_link_geometric_jacobian", (base,), want["Jg"], "Jg", (6, 7)),
        ("get_link_linear_jacobian", (base,), want["Jg"][:, :3], "Jg", (3, 7)),
        ("get_link_angular_geometric_jacobian", (base,), want["Jg"][:, 3:], "Jg", (3, 7)),
        ("get_link_analytical_jacobian", (base,), want["Ja"], "Ja", (6, 7)),
        ("get_link_angular_analytical_jacobian", (base,), want["Ja"][:, 3:], "Ja3", (3, 7)),
        ("get_link_axis", (a3, base), want["axis"], "axis", (3,)),
        ("get_link_axis", ("x", base), want["rot"][:, :, 0], "axis", (3,)),
        ("get_link_axis", ("y", base), want["rot"][:, :, 1], "axis", (3,)),
        ("get_link_axis", ("z", base), want["rot"][:, :, 2], "axis", (3,)),
    ]
    Q = ref.case_inputs(index)
    for name, args, expect, key, shape1 in table:
        for single in (True, False):
            q = Q[0] if single else Q[:5].T
            exp = expect[0] if single else expect[:5]
            for form, value in (("method", getattr(rm, name)(link, q, *args)), ("function", getattr(rm, name + "_function")(link, *args, n=1 if single else 5)(q))):
                what = f"{name} {form} {'1-D' if single else '7x5'}"
                if single:
                    assert isinstance(value, np.ndarray) and value.shape == shape1, what
                elif len(shape1) == 2:
                    assert isinstance(value, list) and len(value) == 5 and all(m.shape == shape1 for m in value), what
                else:
                    assert isinstance(value, np.ndarray) and value.shape == shape1 + (5,), what
                got = stacked(value)
                if key == "Ja3":  # rows 3-5 alone: pad to the six rows the comparison splits
                    ref.assert_outputs_match({"Ja": np.concatenate([np.zeros_like(got), got], axis=-2)}, {"Ja": np.concatenate([np.zeros_like(exp), exp], axis=-2)}, what)
                elif key == "Ja":
                    ref.assert_outputs_match({"Ja": got}, {"Ja": exp}, what)
                elif key == "rpy":
                    ref.assert_outputs_match({"rpy": got}, {"rpy": exp}, what)
                else:
                    ref.assert_outputs_match({key: got}, {key: exp}, what)
    # the get_global_* variants are the base-frame ones with the root as base (models.py:1528, 1710), bit for bit
    for q in (Q[0], Q[:5].T):
        for gname, bname, extra in (("get_global_link_rpy", "get_link_rpy", ()), ("get_global_link_analytical_jacobian", "get_link_analytical_jacobian", ()),
                                    ("get_global_link_angular_analytical_jacobian", "get_link_angular_analytical_jacobian", ()), ("get_global_link_axis", "get_link_axis", (a3,)),
                                    ("get_global_link_axis", "get_link_axis", ("y",))):
            a, b = getattr(rm, gname)(link, q, *extra), getattr(rm, bname)(link, q, *extra, root)
            assert np.array_equal(np.asarray(a), np.asarray(b)), gname
            f = getattr(rm, gname + "_function")(link, *extra, n=q.shape[-1] if q.ndim == 2 else 1)(q)
            assert np.array_equal(np.asarray(f), np.asarray(a)), gname + "_function"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_ragged_sizes_layouts_and_subsets(hip_lib, robots, n):
    link, base = "end_effector_ball", "lwr_arm_3_link"
    handle = robots["kuka"]._frames(link, base)
    rng = np.random.default_rng(SEED + 77 + n)
    Q = rng.uniform(-2.9, 2.9, (n, 7))
    full = host_call(handle, Q, NAMES)
    # the structure-of-arrays device call is the same kernel: the same bits, and nothing written outside the buffers
    soa = device_call(handle, Q, NAMES)
    for k in NAMES:
        assert np.array_equal(soa[k], full[k]), f"SoA and reference layout differ in {k}"
    # any subset of the outputs gives the bits of the full call
    for subset in (("rpy",), ("Ja",), ("pos", "axis")):
        part = host_call(handle, Q, subset)
        for k in subset:
            assert np.array_equal(part[k], full[k]), f"subset {subset} differs in {k}"
    # up to 16 sampled units away from the pitch singularity (the oracle decides which) against the reference
    orc = ref.oracle("kuka")
    picked = [i for i in rng.permutation(n) if abs(ref.sinp_of(orc.get_link_quaternion(link, Q[i], base))) <= ref.SINP_MAX][:16]
    if picked:
        got = shaped({k: a[picked] for k, a in full.items()}, len(picked), 7)
        ref.assert_outputs_match(got, ref.reference_batch("kuka", link, base, Q[picked]), f"n={n}:")
    assert len(picked) == 16 or n < 63


def test_pitch_branch_and_errors(hip_lib, robots):
    lib = hip_lib
    rm, orc = robots["kuka"], ref.oracle("kuka")
    link, root = "end_effector_ball", rm.get_root_link()
    # q = +-(pi/2) e_2: the oracle's sinp is +-1 there and its pitch +pi/2 both times (the branch that loses the sign)
    Q = np.zeros((2, 7))
    Q[0, 1], Q[1, 1] = np.pi / 2, -np.pi / 2
    want = ref.reference_batch("kuka", link, root, Q)
    assert np.all(want["rpy"][:, 1] == np.pi / 2)
    got = shaped(host_call(rm._frames(link, root), Q, NAMES), 2, 7)
    assert np.all(np.isfinite(got["rpy"]))
    print("pitch at the singularity:", got["rpy"][:, 1])
    assert np.all(np.abs(np.abs(got["rpy"][:, 1]) - np.pi / 2) <= 1e-7)
    ref.assert_outputs_match({k: got[k] for k in ("pos", "rot", "quat", "Jg")}, want, "singular pitch:")

    # errors: every argument check comes before any device work
    d = _lib.oh_problem_desc(kind=_lib.OH_PROBLEM_KINEMATICS, ndof=7)
    h = C.c_void_p()
    _lib.check(lib.oh_create(C.byref(d), C.byref(h)), "create")
    q = np.zeros((1, 7))
    pos, axis = np.zeros(3), np.zeros(3)
    out = _lib.oh_link_out(pos=_lib._ptr(pos))
    assert lib.oh_link_kin(h, 1, _lib._ptr(q), None, C.byref(out)) == 3 and b"oh_set_link_frames" in lib.oh_last_error()  # OH_ERR_STATE
    chain = rm.kinematic_chain(link)
    short = RobotModel(urdf_filename=MED7_KIN).kinematic_chain("lbr_link_4")
    short.ndof = 6
    assert lib.oh_set_link_frames(h, C.byref(chain), C.byref(short)) == 1 and b"ndof" in lib.oh_last_error()
    bad = rm.kinematic_chain(link)
    bad.jtype[2] = 5
    assert lib.oh_set_link_frames(h, C.byref(bad), None) == 1 and b"joint type" in lib.oh_last_error()
    assert lib.oh_link_kin(h, 1, _lib._ptr(q), None, C.byref(out)) == 3  # still no frames
    _lib.check(lib.oh_set_link_frames(h, C.byref(chain), None), "oh_set_link_frames")  # base NULL: the root frame
    assert lib.oh_link_kin(h, 0, _lib._ptr(q), None, C.byref(out)) == 1
    assert lib.oh_link_kin(h, 1, _lib._ptr(q), None, None) == 1 and b"oh_link_kin" in lib.oh_last_error()
    with_axis = _lib.oh_link_out(axis=_lib._ptr(axis))
    assert lib.oh_link_kin(h, 1, _lib._ptr(q), None, C.byref(with_axis)) == 1 and b"axis3" in lib.oh_last_error()
    assert lib.oh_link_kin(h, 1, _lib._ptr(q), _lib._ptr(np.zeros(3)), C.byref(with_axis)) == 1 and b"axis3" in lib.oh_last_error()
    assert lib.oh_link_kin(h, 1, _lib._ptr(q), None, C.byref(out)) == 0
    assert np.abs(pos - orc.get_global_link_position(link, q[0])).max() <= ref.TOL  # base NULL is the root frame
    lib.oh_destroy(h)

    # two chains without joints (med7: lbr_link_0 is rigidly attached to the root): the constant transform for every unit
    med, n = RobotModel(urdf_filename=MED7_KIN), 70
    Qm = np.random.default_rng(SEED).uniform(-2.0, 2.0, (n, 7))
    handle = LinkFrameHandle(med.kinematic_chain("lbr_link_0"), med.kinematic_chain("world"))
    assert handle.ndof == 7 and med.kinematic_chain("lbr_link_0").n_chain == 0
    got = shaped(host_call(handle, Qm, NAMES), n, 7)
    one = ref.reference("med7", "lbr_link_0", "world", Qm[0])
    ref.assert_outputs_match(got, {k: np.broadcast_to(v, (n,) + v.shape) for k, v in one.items()}, "no joints:")
    assert not got["Jg"].any() and not got["Ja"].any()
