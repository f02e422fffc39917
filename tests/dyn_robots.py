"""Robot tables for the inverse-dynamics tests: every chain length oh_set_dynamics accepts (2 ... 9 bodies = 1 ... 8 joints) and one arm built
to be awkward.  Each builder writes a .kin.json file into a directory and returns its path (plain helpers, no fixtures)."""
import copy
import json
import os

from conftest import GOLDEN, MED7_KIN

TESTER_REV_KIN = os.path.join(GOLDEN, "tester_robot_revolute.kin.json")


def _write(tmp_path, d):
    path = os.path.join(str(tmp_path), f"{d['name']}.kin.json")
    with open(path, "w") as f:
        json.dump(d, f)
    return path


def med7_cut(tmp_path, n):
    """med7.kin.json with n actuated joints: cut after joint n, a tool (0.4 kg) on a fixed joint behind it -- every body RobotModel.rnea counts carries <inertial>."""
    d = json.load(open(MED7_KIN))
    joints = {j["name"]: j for j in d["joints"]}
    links = {l["name"]: l for l in d["links"]}
    out = copy.deepcopy(d)
    out["name"] = f"med{n}"
    keep = ["world_lbr_joint"] + [f"lbr_joint_{i}" for i in range(n)]
    out["joints"] = [joints[k] for k in keep] + [{"name": "tool_joint", "type": "fixed", "parent": joints[keep[-1]]["child"], "child": "tool", "xyz": [0.0, 0.0, 0.12],
                                                 "rpy": [0.0, 0.0, 0.0]}]
    out["links"] = [links[k] for k in ["world"] + [joints[k]["child"] for k in keep]] + [
        {"name": "tool", "inertial": {"mass": 0.4, "xyz": [0.0, 0.0, 0.03], "rpy": [0.0, 0.0, 0.0], "inertia": [0.001, 0.0, 0.0, 0.001, 0.0, 0.0008]}}]
    return _write(tmp_path, out)


def med8(tmp_path):
    """med7 with an 8th revolute wrist joint (about x) and a body of its own between the flange and the end-effector link: 9 bodies."""
    d = copy.deepcopy(json.load(open(MED7_KIN)))
    d["name"] = "med8"
    ee = next(j for j in d["joints"] if j["name"] == "lbr_joint_ee")
    ee["parent"] = "lbr_link_8"
    i = d["joints"].index(ee)
    d["joints"].insert(i, {"name": "lbr_joint_7", "type": "revolute", "parent": "lbr_link_7", "child": "lbr_link_8", "xyz": [0.0, 0.0, 0.04],
                           "rpy": [0.0, 0.0, 0.0], "axis": [1.0, 0.0, 0.0], "limit": {"lower": -2.0, "upper": 2.0, "velocity": 10.0, "effort": 20.0}})
    k = [l["name"] for l in d["links"]].index("lbr_link_ee")
    d["links"].insert(k, {"name": "lbr_link_8", "inertial": {"mass": 0.6, "xyz": [0.01, -0.005, 0.02], "rpy": [0.0, 0.0, 0.0],
                                                              "inertia": [0.0009, 0.00002, -0.00001, 0.0011, 0.00003, 0.0007]}})
    return _write(tmp_path, d)


def awkward5(tmp_path):
    """A synthetic 5-joint arm that is no rigid-body chain on purpose:
    - joint-origin rpy everywhere, and on a2 a rotation that moves the joint's axis (R0^T axis != axis: the reference's recursion adds the angular
      velocity iRp @ axis, models.py:1821-1823, which is then not the axis the joint turns about);
    - a non-coordinate unit axis [0.6, 0, 0.8] (a3) and a negative axis (a1), a `continuous` joint (a4);
    - full off-diagonal inertia tensors, one massless body with zero inertia (l3), an inertial origin with nonzero rpy (l2: the reference ignores
      it, so do the oracle and the product -- they are compared with each other, not with physics)."""
    lim = {"lower": -3.0, "upper": 3.0, "velocity": 10.0, "effort": 50.0}
    J = lambda name, typ, parent, child, xyz, rpy, axis=None: {k: v for k, v in dict(
        name=name, type=typ, parent=parent, child=child, xyz=xyz, rpy=rpy, axis=axis, limit=lim if typ == "revolute" else None).items() if v is not None}
    L = lambda name, m, xyz, inertia, rpy=(0.0, 0.0, 0.0): {"name": name, "inertial": {"mass": m, "xyz": xyz, "rpy": list(rpy), "inertia": inertia}}
    d = {"format": "optas_amd.kin/1", "name": "awkward5", "source": "synthetic",
         "joints": [J("base_joint", "fixed", "world", "base", [0.0, 0.0, 0.05], [0.0, 0.0, 0.3]),
                    J("a0", "revolute", "base", "l1", [0.0, 0.0, 0.2], [0.0, 0.0, 0.4], [0.0, 0.0, 1.0]),
                    J("a1", "revolute", "l1", "l2", [0.05, -0.02, 0.25], [0.0, -0.7, 0.0], [0.0, -1.0, 0.0]),
                    J("a2", "revolute", "l2", "l3", [0.3, 0.01, 0.02], [0.3, -0.2, 0.1], [0.0, 0.0, 1.0]),
                    J("a3", "revolute", "l3", "l4", [0.0, 0.04, 0.22], [0.0, 0.0, 0.0], [0.6, 0.0, 0.8]),
                    J("a4", "continuous", "l4", "l5", [0.02, 0.0, 0.18], [0.0, 0.0, 0.25], [0.0, 0.0, 1.0]),
                    J("tool_joint", "fixed", "l5", "tool", [0.0, 0.03, 0.1], [0.2, 0.0, 0.0])],
         "links": [{"name": "world"},
                   L("base", 5.0, [0.0, 0.0, 0.05], [0.05, 0.0, 0.0, 0.05, 0.0, 0.06]),
                   L("l1", 4.2, [0.01, -0.03, 0.11], [0.031, 0.0021, -0.0013, 0.027, 0.0042, 0.012]),
                   L("l2", 3.1, [0.12, 0.02, 0.01], [0.012, -0.0017, 0.0022, 0.034, 0.0011, 0.029], rpy=(0.4, -0.3, 0.9)),
                   L("l3", 0.0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]),
                   L("l4", 1.9, [-0.02, 0.01, 0.09], [0.009, 0.0006, -0.0008, 0.011, -0.0014, 0.005]),
                   L("l5", 1.1, [0.0, 0.015, 0.04], [0.0032, -0.0004, 0.0003, 0.0028, 0.0005, 0.0019]),
                   L("tool", 0.7, [0.03, 0.0, 0.05], [0.0011, 0.0001, -0.0002, 0.0014, 0.00015, 0.0009])]}
    return _write(tmp_path, d)


def robots(tmp_path):
    """(tag, kin file, rigid) for every chain length 1 ... 8 joints plus the awkward arm; rigid: the tables describe a rigid-body chain
    (every joint-origin rotation leaves its axis in place), so the mass matrix is symmetric positive definite."""
    out = [(f"med{n}", med7_cut(tmp_path, n), True) for n in range(1, 7)]
    out += [("med7", MED7_KIN, True), ("med8", med8(tmp_path), True), ("tester2", TESTER_REV_KIN, True), ("awkward5", awkward5(tmp_path), False)]
    return out


def mp_points(tag, nd):
    """The points the high-precision reference (oracle/rnea_mp.py) is evaluated at, shared by the CPU and GPU tests: a moderate one and an
    extreme one (q up to 1e3 rad, qd up to 50 rad/s, qdd up to 500).  -> [(q, qd, qdd, c, with_hessian)]; the Hessian costs ~(3 nd)^2 / 2
    evaluations of the recursion, so the long chains take it at the first point only."""
    import zlib

    import numpy as np

    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    mod = (rng.uniform(-2, 2, nd), rng.uniform(-2, 2, nd), rng.uniform(-2, 2, nd), rng.normal(size=nd), True)
    ext = (rng.uniform(-1e3, 1e3, nd), rng.uniform(-50, 50, nd), rng.uniform(-500, 500, nd), rng.normal(size=nd), nd <= 5)
    return [mod, ext]
