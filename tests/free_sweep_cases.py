"""Cases for the sweeps of the position-tracking family (csrc/oh_free.hip: k_step_free, k_step_free_pcr<64 | 128>, k_step_free_cp, k_step_free_bb,
k_free_persist), shared by test_free_sweep_cpu.py (no GPU) and test_gpu_free_sweeps.py.

A case is (robot, variant, free knots nK).  Robots: the KUKA LWR (7 joints), the KUKA cut after its 6th joint, the med7 cut after its 2nd.  Variants:
plain (dual_arm.py per arm), guarded (joint limits + sphere clearances), vel (joint-velocity rows only, +-0.06 rad/s).  The horizons sit on every edge
of the sweeps' index arithmetic: one free knot (the twisted factorisation's first wavefront owns none), odd / even, 63 / 64 / 65 (limit of k_step_free_cp
and of the automatic k_free_persist, switch from pcr<64> to pcr<128>), 108 / 109 (first dynamic LDS size beyond 64 KB), 127 / 128 / 129 (last block
horizons, 64 knots per wavefront, first horizon of the serial fall-back).  dt = 10 / (T - 1).

Every case has three instances, tiled to a batch of nine.  The seed of an instance is NOT the constant trajectory: q_t = qc + cumsum(U(-0.12, 0.12) dt),
so about half of the velocity rows are violated at the first evaluation and the coupling blocks of the first system differ from interval to interval
and from joint to joint -- with the plain coupling 2 kappa an off-by-one in a sweep's interval index is invisible.

The reference of a step is oracle/blocktri_mp.py (50 digits) on the system the numpy port hands its own solver (on_system hook).  SEEDS, PORT_STEP_ERR
and SENS below were found / measured on the CPU by `python tests/free_sweep_cases.py` and are re-checked by test_free_sweep_cpu.py; they are not chosen.
"""
import copy
import json
import os
import sys
import zlib

import numpy as np

from conftest import KUKA_KIN
from oracle.guarded import Guards, guard_values, solve_free_al
from oracle.robot import OracleRobot
from oracle.structured import FoldedChain, solve_free_lm

N_INST, BATCH = 3, 9
W_PATH, W_VEL, RHO0 = 1.0, 0.01, 10.0
VMAX = 0.06          # rad/s, the velocity rows of the vel variant
WALK = 0.12          # rad/s, the seed's random walk: twice VMAX
LINK_RADIUS, OBS_RADIUS = 0.15, 0.1
TOL = 1e-6
MARGIN = 10.0        # qp_planted_large.MARGIN's role: a different summation order, not a wrong coefficient
FLOOR = 1e-13

HORIZONS = {
    "kuka7": (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 108, 109, 127, 128, 129),
    "kuka6": (2, 5, 63, 64, 65, 128, 129),
    "med2": (2, 33),
}
VARIANTS = {"kuka7": ("plain", "guarded", "vel"), "kuka6": ("plain", "guarded", "vel"), "med2": ("plain",)}
CASES = [(r, v, nk) for r in HORIZONS for v in VARIANTS[r] for nk in HORIZONS[r]]
NDOF = {"kuka7": 7, "kuka6": 6, "med2": 2}
MP_ALL_ITERATIONS_BELOW = 108  # from this horizon on the CPU test certifies the first solve only (1.3 s a solve at 128 knots)


def case_id(case):
    return "%s-%s-nK%d" % case


def kuka_variant(tmp_path, n):
    """kuka_lwr.kin.json with n actuated joints: cut after joint n (a 10 cm tool on the last link), or -- n = 8 -- a wrist joint added behind the flange."""
    d = json.load(open(KUKA_KIN))
    joints = {j["name"]: j for j in d["joints"]}
    out = copy.deepcopy(d)
    out["name"] = f"kuka{n}"
    if n < 7:
        keep = [f"lwr_arm_{i}_joint" for i in range(n)]
        last = joints[keep[-1]]["child"]
        out["joints"] = [joints[k] for k in keep] + [{"name": "tool_joint", "type": "fixed", "parent": last, "child": "tool", "xyz": [0.0, 0.0, 0.1], "rpy": [0.0, 0.0, 0.0]}]
        names = {"lwr_arm_0_link", "tool"} | {joints[k]["child"] for k in keep}
        out["links"] = [l for l in d["links"] if l["name"] in names] + [{"name": "tool"}]
    else:
        js = []
        for j in d["joints"]:
            if j["name"] == "lwr_arm_7_joint":  # the fixed flange joint: a wrist roll about y takes its place, the flange follows
                js.append({"name": "wrist_extra_joint", "type": "revolute", "parent": "lwr_arm_7_link", "child": "wrist_extra_link", "xyz": [0.0, 0.0, 0.05],
                           "rpy": [0.0, 0.0, 0.0], "axis": [0.0, 1.0, 0.0], "limit": {"lower": -2.0, "upper": 2.0, "velocity": 2.0, "effort": 50.0}})
                js.append({**j, "parent": "wrist_extra_link"})
            else:
                js.append(j)
        out["joints"] = js
        out["links"] = d["links"] + [{"name": "wrist_extra_link"}]
    path = os.path.join(str(tmp_path), f"kuka{n}.kin.json")
    json.dump(out, open(path, "w"))
    return path, ("tool" if n < 7 else "end_effector_ball")


QN7 = np.deg2rad([0, -30, 0, 90, 0, 30, 0])  # dual_arm.py:185
# the obstacle column of the synthetic config 4 as the left arm of dual_arm.py sees it (its base stands at y = -0.25)
OBSTACLES = np.array([[0.55, 0.25, 0.1 * (i + 1)] for i in range(6)])


def robot(tmp_path, name):
    """-> (kin file, tracked link, nominal configuration, sphere links the chain has)"""
    if name == "kuka7":
        return KUKA_KIN, "end_effector_ball", QN7, ["end_effector_ball", "lwr_arm_7_link", "lwr_arm_5_link", "lwr_arm_6_link"]
    if name == "kuka6":
        kin, link = kuka_variant(tmp_path, 6)
        return kin, link, QN7[:6], ["tool", "lwr_arm_5_link", "lwr_arm_6_link"]
    import dyn_robots

    return dyn_robots.med7_cut(tmp_path, 2), "tool", np.array([0.4, 0.7]), []


class Case:
    """The three instances of a case: everything the port and the library need."""

    def __init__(self, tmp_path, case, seed=None):
        self.case = case
        self.robot, self.variant, self.nK = case
        self.kin, self.link, qn, self.sphere_links = robot(tmp_path, self.robot)
        self.orc = OracleRobot(self.kin)
        self.chain = FoldedChain(self.orc, self.link)
        self.n = n = self.orc.ndof
        self.fix_dq0 = self.nK == 1
        self.t0 = 2 if self.fix_dq0 else 1
        self.T = T = self.nK + self.t0
        self.dt = 10.0 / (T - 1)
        ts = np.linspace(0.0, 1.0, T)
        self.offs = 0.1 * np.stack([np.sin(np.pi * ts) * 0.8, ts, -0.5 * ts], 1)
        self.seed = SEEDS[case] if seed is None else seed
        rng = np.random.default_rng(self.seed)
        self.guards = Guards()
        self.vlimits = None
        if self.variant == "guarded":
            self.guards = Guards(lo=self.orc.lower_actuated_joint_limits, up=self.orc.upper_actuated_joint_limits, links=self.sphere_links,
                                 link_radii=np.full(len(self.sphere_links), LINK_RADIUS), obs_pos=OBSTACLES, obs_radii=np.full(len(OBSTACLES), OBS_RADIUS))
            # by rejection, the rule of examples/dual_arm.py:draw_feasible_configurations on this chain's rows: q_0 = qc is pinned, its rows are constants
            qc = np.empty((0, n))
            while len(qc) < N_INST:
                cand = qn + rng.uniform(-0.1, 0.1, (64, n))
                qc = np.concatenate([qc, cand[np.array([guard_values(self.chain, c[None], self.guards)[0].min() > 0.0 for c in cand])]])
            self.qc = np.ascontiguousarray(qc[:N_INST])
        else:
            self.qc = qn + rng.uniform(-0.1, 0.1, (N_INST, n))
        if self.variant == "vel":
            self.vlimits = (np.full(n, -VMAX), np.full(n, VMAX))
        steps = rng.uniform(-WALK, WALK, (N_INST, T - 1, n)) * self.dt
        steps[:, : self.t0 - 1] = 0.0  # (fix_dq0: knot 1 is pinned to qc as well)
        self.Q0 = self.qc[:, None, :] + np.concatenate([np.zeros((N_INST, 1, n)), np.cumsum(steps, 1)], 1)
        self.max_iter_full = 600 if self.variant == "vel" else 400

    # ---- the numpy port ----
    def port(self, i, max_iter, on_system=None):
        kw = dict(Q0=self.Q0[i], w_path=W_PATH, w_vel=W_VEL, fix_dq0=self.fix_dq0, max_iter=max_iter, tol=TOL, on_system=on_system)
        if self.variant == "plain":
            return solve_free_lm(self.chain, self.T, self.dt, self.offs, self.qc[i], **kw)
        return solve_free_al(self.chain, self.T, self.dt, self.offs, self.qc[i], self.guards, rho0=RHO0, exact=False, vlimits=self.vlimits, **kw)

    def port_systems(self, i, max_iter=3):
        """The port at the cap and every linear solve it did: [dict(iteration, D, Er, rhs, mu, z, ratio, accept, rows)].  ratio / accept: the ratio
        test that preceded the solve (None for the first evaluation); rows: min |lam - rho g| over the inequality rows of the evaluation before it,
        for the velocity rows in the units of the other rows, |lam_v / vscale - rho g_v| (their own penalty is rho vscale, vscale = dt^2 / 40: taken
        literally it would ask 1e-6 of numbers that are 1e-3 at most).
        The hook's arguments are the system; the rest is read off the port's frame as it stands at the call, so nothing is recomputed here."""
        recs = []

        def hook(it, D, Er, rhs, mu, z):
            loc = sys._getframe(1).f_locals
            first = not recs
            ratio = None if first else loc.get("ratio", loc.get("rho") if self.variant == "plain" else None)
            rec = dict(iteration=it, D=D.copy(), Er=Er.copy(), rhs=rhs.copy(), mu=float(mu), z=None if z is None else z.copy(), ratio=ratio,
                       accept=True if first else bool(loc["accept"]), rows=np.inf)
            if self.variant != "plain":
                Q, lam, rho = loc["Qt"], loc["lam"], loc["rho"]
                m = np.inf
                if lam.shape[1]:
                    m = min(m, np.abs(lam - rho * loc["gv"])[self.t0 :].min())
                if self.vlimits is not None:
                    v = (Q[1:] - Q[:-1]) / self.dt
                    gv = np.concatenate([v - self.vlimits[0][None], self.vlimits[1][None] - v], 1)
                    m = min(m, np.abs(loc["lam_v"] / loc["vscale"] - rho * gv)[self.t0 - 1 :].min())
                rec["rows"] = float(m)
            recs.append(rec)

        return self.port(i, max_iter, on_system=hook), recs

    # ---- the library ----
    def backend(self, max_iter):
        from optas_amd import _lib
        from optas_amd.backend import FigureEightBackend
        from optas_amd.models import RobotModel

        model = RobotModel(urdf_filename=self.kin)
        g = None
        if self.variant != "plain":
            g = _lib.oh_guards()
            if self.variant == "guarded":
                g.limits = 1
                for j in range(self.n):
                    g.q_lo[j], g.q_up[j] = float(self.guards.lo[j]), float(self.guards.up[j])
                g.n_links, g.n_obstacles = len(self.sphere_links), len(OBSTACLES)
                for l, (k, off) in enumerate(model.link_attachments(self.link, self.sphere_links)):
                    g.link_joint[l] = k
                    for a in range(3):
                        g.link_offset[l][a] = float(off[a])
            else:
                g.vel_limits = 1
                for j in range(self.n):
                    g.dq_lo[j], g.dq_up[j] = -VMAX, VMAX
        return FigureEightBackend(model.kinematic_chain(self.link), self.T, self.dt, self.offs, w_path=W_PATH, w_vel=W_VEL, max_iter=max_iter, tol=TOL,
                                  hessian=_lib.OH_HESSIAN_GAUSS_NEWTON, lock_orientation=False, fix_dq0=self.fix_dq0, path_in_frame=False, guards=g)

    def batch(self):
        """x0 (9, nx) and p (9, np): instance b of the batch is instance b % 3 of the case."""
        idx = np.arange(BATCH) % N_INST
        Q = self.Q0[idx].reshape(BATCH, -1)
        x0 = np.concatenate([Q, np.zeros((BATCH, self.n * (self.T - 1)))], 1)
        p = self.qc[idx]
        if self.variant == "guarded":
            obs = np.concatenate([np.append(o, OBS_RADIUS) for o in OBSTACLES])
            p = np.concatenate([p, np.full((BATCH, len(self.sphere_links)), LINK_RADIUS), np.tile(obs, (BATCH, 1))], 1)
        return x0, np.ascontiguousarray(p)


def sensitivity(case, D, Er, rhs, mu, z_mp):
    """max |dz| of the exact solution when every entry of D and rhs is multiplied by 1 + 4 * 2^-53 u, u ~ U(-1, 1): inputs that differ by a few ulp,
    which is what the kernel's own FK and Jacobians are against numpy's."""
    from oracle.blocktri_mp import solve_mp

    rng = np.random.default_rng(zlib.crc32(case_id(case).encode()))
    Dp = D * (1.0 + 4.0 * 2.0**-53 * rng.uniform(-1, 1, D.shape))
    Dp = 0.5 * (Dp + np.swapaxes(Dp, 1, 2))
    rp = rhs * (1.0 + 4.0 * 2.0**-53 * rng.uniform(-1, 1, rhs.shape))
    return float(np.abs(solve_mp(Dp, Er, rp, mu)[0] - z_mp).max())


def bound(case, z_inf):
    return max(MARGIN * max(PORT_STEP_ERR[case], SENS[case]), FLOOR) * max(1.0, z_inf)


def measure(tmp_path, case, seed=None):
    """Everything the CPU test asserts about a case -> dict; the instances' first systems and their mp solutions ride along."""
    from oracle.blocktri_mp import solve_mp

    c = Case(tmp_path, case, seed)
    out = dict(case=c, port_err=0.0, damped=[], first_accepted=True, ratio_gap=np.inf, rows_gap=np.inf, rejected=0, z1=[], z1_inf=0.0,
               hook_neutral=True, cap1_err=0.0, n_coupling=0)
    for i in range(N_INST):
        res, recs = c.port_systems(i, 3)
        plain = c.port(i, 3)
        out["hook_neutral"] &= all(np.array_equal(np.asarray(res[k]), np.asarray(plain[k])) for k in res)
        for r in recs:
            if r["iteration"] > 2:
                continue  # (the solve after the evaluation that closes the third iteration: nobody takes that step)
            if r["ratio"] is not None:
                out["ratio_gap"] = min(out["ratio_gap"], abs(r["ratio"] - 1e-4))
            out["rows_gap"] = min(out["rows_gap"], r["rows"])
            if r["iteration"] >= 1 and not r["accept"]:
                out["rejected"] += 1
            if r["z"] is None:
                continue
            if r["mu"] > 0.0:
                out["damped"].append((i, r["iteration"], r["mu"]))
            if r["iteration"] == 0 or c.nK < MP_ALL_ITERATIONS_BELOW:
                z_mp = solve_mp(r["D"], r["Er"], r["rhs"], r["mu"])[0]
                out["port_err"] = max(out["port_err"], float(np.abs(r["z"] - z_mp).max()))
                if r["iteration"] == 0 and len(out["z1"]) == i:
                    out["z1"].append(z_mp)
                    out["z1_inf"] = max(out["z1_inf"], float(np.abs(z_mp).max()))
                    if i == 0:
                        out["sens"] = sensitivity(case, r["D"], r["Er"], r["rhs"], r["mu"], z_mp)
                        out["n_coupling"] = len(np.unique(np.round(np.einsum("tjj->tj", r["Er"]), 12))) if len(r["Er"]) else 0
        r1 = c.port(i, 1)
        out["first_accepted"] &= bool(np.abs(r1["Q"] - c.Q0[i]).max() > 0.0)
        out["cap1_err"] = max(out["cap1_err"], float(np.abs(r1["Q"][c.t0 :] - c.Q0[i][c.t0 :] - recs[0]["z"]).max()))  # max_iter = 1 returns Q0 + z
    return out


# ---- found / measured by `python tests/free_sweep_cases.py` ----
# 2026-10-18, numpy 2.2.6, mpmath 1.3.0
SEEDS = {
    ('kuka7', 'plain', 1): 14244,
    ('kuka7', 'plain', 2): 85726,
    ('kuka7', 'plain', 3): 78408,
    ('kuka7', 'plain', 4): 41099,
    ('kuka7', 'plain', 5): 35901,
    ('kuka7', 'plain', 31): 12851,
    ('kuka7', 'plain', 32): 79945,
    ('kuka7', 'plain', 33): 96959,
    ('kuka7', 'plain', 63): 7866,
    ('kuka7', 'plain', 64): 47129,
    ('kuka7', 'plain', 65): 33391,
    ('kuka7', 'plain', 108): 1781,
    ('kuka7', 'plain', 109): 22531,
    ('kuka7', 'plain', 127): 32710,
    ('kuka7', 'plain', 128): 93463,
    ('kuka7', 'plain', 129): 5601,
    ('kuka7', 'guarded', 1): 63083,
    ('kuka7', 'guarded', 2): 21316,
    ('kuka7', 'guarded', 3): 20781,
    ('kuka7', 'guarded', 4): 70156,
    ('kuka7', 'guarded', 5): 89022,
    ('kuka7', 'guarded', 31): 48776,
    ('kuka7', 'guarded', 32): 55730,
    ('kuka7', 'guarded', 33): 60196,
    ('kuka7', 'guarded', 63): 34209,
    ('kuka7', 'guarded', 64): 93154,
    ('kuka7', 'guarded', 65): 25108,
    ('kuka7', 'guarded', 108): 3862,
    ('kuka7', 'guarded', 109): 28416,
    ('kuka7', 'guarded', 127): 54917,
    ('kuka7', 'guarded', 128): 51956,
    ('kuka7', 'guarded', 129): 51426,
    ('kuka7', 'vel', 1): 69085,
    ('kuka7', 'vel', 2): 86449,
    ('kuka7', 'vel', 3): 44628,
    ('kuka7', 'vel', 4): 36563,
    ('kuka7', 'vel', 5): 65029,
    ('kuka7', 'vel', 31): 42213,
    ('kuka7', 'vel', 32): 61503,
    ('kuka7', 'vel', 33): 41,
    ('kuka7', 'vel', 63): 58892,
    ('kuka7', 'vel', 64): 15535,
    ('kuka7', 'vel', 65): 49369,
    ('kuka7', 'vel', 108): 41268,
    ('kuka7', 'vel', 109): 35330,
    ('kuka7', 'vel', 127): 1831,
    ('kuka7', 'vel', 128): 8630,
    ('kuka7', 'vel', 129): 93216,
    ('kuka6', 'plain', 2): 84638,
    ('kuka6', 'plain', 5): 36253,
    ('kuka6', 'plain', 63): 11253,
    ('kuka6', 'plain', 64): 44022,
    ('kuka6', 'plain', 65): 11712,
    ('kuka6', 'plain', 128): 7090,
    ('kuka6', 'plain', 129): 98148,
    ('kuka6', 'guarded', 2): 73181,
    ('kuka6', 'guarded', 5): 11579,
    ('kuka6', 'guarded', 63): 22679,
    ('kuka6', 'guarded', 64): 55060,
    ('kuka6', 'guarded', 65): 82210,
    ('kuka6', 'guarded', 128): 40924,
    ('kuka6', 'guarded', 129): 92330,
    ('kuka6', 'vel', 2): 40221,
    ('kuka6', 'vel', 5): 4454,
    ('kuka6', 'vel', 63): 5330,
    ('kuka6', 'vel', 64): 78161,
    ('kuka6', 'vel', 65): 88135,
    ('kuka6', 'vel', 128): 16022,
    ('kuka6', 'vel', 129): 84032,
    ('med2', 'plain', 2): 21403,
    ('med2', 'plain', 33): 89244,
}
PORT_STEP_ERR = {
    ('kuka7', 'plain', 1): 5.124e-14,
    ('kuka7', 'plain', 2): 2.621e-13,
    ('kuka7', 'plain', 3): 8.948e-14,
    ('kuka7', 'plain', 4): 1.695e-13,
    ('kuka7', 'plain', 5): 3.347e-14,
    ('kuka7', 'plain', 31): 1.540e-14,
    ('kuka7', 'plain', 32): 1.250e-14,
    ('kuka7', 'plain', 33): 1.004e-14,
    ('kuka7', 'plain', 63): 1.427e-14,
    ('kuka7', 'plain', 64): 1.757e-14,
    ('kuka7', 'plain', 65): 1.296e-14,
    ('kuka7', 'plain', 108): 4.842e-14,
    ('kuka7', 'plain', 109): 1.023e-14,
    ('kuka7', 'plain', 127): 9.666e-15,
    ('kuka7', 'plain', 128): 1.554e-14,
    ('kuka7', 'plain', 129): 2.426e-14,
    ('kuka7', 'guarded', 1): 2.145e-13,
    ('kuka7', 'guarded', 2): 1.544e-13,
    ('kuka7', 'guarded', 3): 1.488e-13,
    ('kuka7', 'guarded', 4): 1.580e-13,
    ('kuka7', 'guarded', 5): 1.102e-13,
    ('kuka7', 'guarded', 31): 9.295e-14,
    ('kuka7', 'guarded', 32): 1.514e-14,
    ('kuka7', 'guarded', 33): 2.578e-14,
    ('kuka7', 'guarded', 63): 1.108e-14,
    ('kuka7', 'guarded', 64): 1.316e-14,
    ('kuka7', 'guarded', 65): 2.084e-14,
    ('kuka7', 'guarded', 108): 1.493e-14,
    ('kuka7', 'guarded', 109): 3.889e-14,
    ('kuka7', 'guarded', 127): 3.292e-14,
    ('kuka7', 'guarded', 128): 1.025e-13,
    ('kuka7', 'guarded', 129): 4.707e-14,
    ('kuka7', 'vel', 1): 1.460e-14,
    ('kuka7', 'vel', 2): 9.345e-14,
    ('kuka7', 'vel', 3): 7.977e-14,
    ('kuka7', 'vel', 4): 5.212e-14,
    ('kuka7', 'vel', 5): 3.803e-14,
    ('kuka7', 'vel', 31): 1.005e-14,
    ('kuka7', 'vel', 32): 1.169e-14,
    ('kuka7', 'vel', 33): 2.331e-14,
    ('kuka7', 'vel', 63): 1.664e-14,
    ('kuka7', 'vel', 64): 1.195e-14,
    ('kuka7', 'vel', 65): 7.480e-15,
    ('kuka7', 'vel', 108): 4.656e-14,
    ('kuka7', 'vel', 109): 2.762e-14,
    ('kuka7', 'vel', 127): 2.198e-14,
    ('kuka7', 'vel', 128): 1.221e-14,
    ('kuka7', 'vel', 129): 2.527e-14,
    ('kuka6', 'plain', 2): 4.019e-14,
    ('kuka6', 'plain', 5): 5.263e-14,
    ('kuka6', 'plain', 63): 8.965e-15,
    ('kuka6', 'plain', 64): 6.706e-15,
    ('kuka6', 'plain', 65): 2.118e-14,
    ('kuka6', 'plain', 128): 1.051e-14,
    ('kuka6', 'plain', 129): 2.187e-14,
    ('kuka6', 'guarded', 2): 1.477e-13,
    ('kuka6', 'guarded', 5): 3.852e-14,
    ('kuka6', 'guarded', 63): 5.906e-14,
    ('kuka6', 'guarded', 64): 2.290e-14,
    ('kuka6', 'guarded', 65): 8.260e-14,
    ('kuka6', 'guarded', 128): 3.933e-14,
    ('kuka6', 'guarded', 129): 2.962e-14,
    ('kuka6', 'vel', 2): 3.042e-14,
    ('kuka6', 'vel', 5): 2.776e-14,
    ('kuka6', 'vel', 63): 1.985e-14,
    ('kuka6', 'vel', 64): 9.354e-15,
    ('kuka6', 'vel', 65): 1.385e-14,
    ('kuka6', 'vel', 128): 2.156e-14,
    ('kuka6', 'vel', 129): 7.092e-15,
    ('med2', 'plain', 2): 2.220e-16,
    ('med2', 'plain', 33): 1.332e-15,
}
SENS = {
    ('kuka7', 'plain', 1): 3.420e-13,
    ('kuka7', 'plain', 2): 1.933e-13,
    ('kuka7', 'plain', 3): 3.915e-13,
    ('kuka7', 'plain', 4): 1.132e-13,
    ('kuka7', 'plain', 5): 1.389e-13,
    ('kuka7', 'plain', 31): 1.943e-14,
    ('kuka7', 'plain', 32): 4.478e-14,
    ('kuka7', 'plain', 33): 4.602e-14,
    ('kuka7', 'plain', 63): 3.217e-14,
    ('kuka7', 'plain', 64): 3.536e-14,
    ('kuka7', 'plain', 65): 1.249e-14,
    ('kuka7', 'plain', 108): 5.781e-14,
    ('kuka7', 'plain', 109): 8.134e-14,
    ('kuka7', 'plain', 127): 9.943e-15,
    ('kuka7', 'plain', 128): 1.817e-14,
    ('kuka7', 'plain', 129): 5.440e-14,
    ('kuka7', 'guarded', 1): 2.055e-13,
    ('kuka7', 'guarded', 2): 5.148e-13,
    ('kuka7', 'guarded', 3): 2.842e-14,
    ('kuka7', 'guarded', 4): 3.378e-14,
    ('kuka7', 'guarded', 5): 1.737e-13,
    ('kuka7', 'guarded', 31): 2.205e-14,
    ('kuka7', 'guarded', 32): 2.176e-14,
    ('kuka7', 'guarded', 33): 5.009e-14,
    ('kuka7', 'guarded', 63): 6.259e-15,
    ('kuka7', 'guarded', 64): 2.848e-14,
    ('kuka7', 'guarded', 65): 1.774e-14,
    ('kuka7', 'guarded', 108): 2.471e-14,
    ('kuka7', 'guarded', 109): 3.021e-14,
    ('kuka7', 'guarded', 127): 6.722e-14,
    ('kuka7', 'guarded', 128): 1.164e-13,
    ('kuka7', 'guarded', 129): 8.143e-14,
    ('kuka7', 'vel', 1): 1.554e-15,
    ('kuka7', 'vel', 2): 1.929e-14,
    ('kuka7', 'vel', 3): 3.292e-14,
    ('kuka7', 'vel', 4): 1.572e-13,
    ('kuka7', 'vel', 5): 7.294e-14,
    ('kuka7', 'vel', 31): 1.576e-14,
    ('kuka7', 'vel', 32): 7.627e-14,
    ('kuka7', 'vel', 33): 1.030e-14,
    ('kuka7', 'vel', 63): 8.467e-15,
    ('kuka7', 'vel', 64): 2.071e-14,
    ('kuka7', 'vel', 65): 2.382e-14,
    ('kuka7', 'vel', 108): 1.173e-14,
    ('kuka7', 'vel', 109): 6.017e-14,
    ('kuka7', 'vel', 127): 3.469e-14,
    ('kuka7', 'vel', 128): 9.827e-15,
    ('kuka7', 'vel', 129): 7.599e-14,
    ('kuka6', 'plain', 2): 1.740e-13,
    ('kuka6', 'plain', 5): 5.293e-14,
    ('kuka6', 'plain', 63): 2.701e-14,
    ('kuka6', 'plain', 64): 1.509e-14,
    ('kuka6', 'plain', 65): 2.869e-14,
    ('kuka6', 'plain', 128): 4.285e-14,
    ('kuka6', 'plain', 129): 4.115e-14,
    ('kuka6', 'guarded', 2): 3.231e-13,
    ('kuka6', 'guarded', 5): 4.902e-14,
    ('kuka6', 'guarded', 63): 6.978e-14,
    ('kuka6', 'guarded', 64): 1.197e-13,
    ('kuka6', 'guarded', 65): 8.660e-14,
    ('kuka6', 'guarded', 128): 3.288e-14,
    ('kuka6', 'guarded', 129): 5.246e-14,
    ('kuka6', 'vel', 2): 8.238e-14,
    ('kuka6', 'vel', 5): 1.990e-14,
    ('kuka6', 'vel', 63): 2.302e-14,
    ('kuka6', 'vel', 64): 1.896e-14,
    ('kuka6', 'vel', 65): 2.962e-14,
    ('kuka6', 'vel', 128): 9.348e-14,
    ('kuka6', 'vel', 129): 3.719e-14,
    ('med2', 'plain', 2): 1.665e-16,
    ('med2', 'plain', 33): 1.887e-15,
}

# (2) a case per variant whose iterations 2-3 hold a rejected step (the listing above: "rejected" > 0)
REJECTING = {"plain": ("kuka7", "plain", 3), "guarded": ("kuka7", "guarded", 128), "vel": ("kuka6", "vel", 2)}


def _search(tmp_path, case, tries=40):
    base = zlib.crc32(case_id(case).encode()) % 100000
    for k in range(tries):
        m = measure(tmp_path, case, seed=base + k)
        ok = m["first_accepted"] and m["ratio_gap"] > 1e-3 and m["rows_gap"] >= 1e-6 and m["cap1_err"] <= 1e-15
        if ok:
            return base + k, m
    raise RuntimeError(f"no seed for {case_id(case)}")


if __name__ == "__main__":
    import tempfile
    import time

    only = sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        rows = []
        for case in CASES:
            if only and not any(o in case_id(case) for o in only):
                continue
            t = time.time()
            seed, m = _search(tmp, case)
            rows.append((case, seed, m))
            print("# %-22s seed %6d port %.2e sens %.2e |z| %.3f coupling values %d rejected %d damped %s (%.1f s)"
                  % (case_id(case), seed, m["port_err"], m["sens"], m["z1_inf"], m["n_coupling"], m["rejected"], sorted({d[1] for d in m["damped"]}), time.time() - t), flush=True)
        print("SEEDS = {")
        for case, seed, m in rows:
            print("    %r: %d," % (case, seed))
        print("}\nPORT_STEP_ERR = {")
        for case, seed, m in rows:
            print("    %r: %.3e," % (case, m["port_err"]))
        print("}\nSENS = {")
        for case, seed, m in rows:
            print("    %r: %.3e," % (case, m["sens"]))
        print("}")
