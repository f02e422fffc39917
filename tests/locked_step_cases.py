"""Cases for the sweeps of the orientation-locked figure-eight family (csrc/oh_figure8_units.h, oh_figure8.h, oh_figure8_kernels.h, oh_kernels.hip:
k_tail, k_retract / k_evalb_zc / k_step_zc, k_evalb / k_couple / k_step and their run-time specialised twins), shared by test_locked_steps_cpu.py (no
GPU) and test_gpu_locked_steps.py.

A case is (robot, variant = plain | vel, free knots nK), T = nK + 2 (q_0 = q_1 = qc are pinned).  Robots: the KUKA LWR (7 joints), the KUKA cut after its 6th, 5th
and 4th joint, the KUKA with an 8th joint (free_sweep_cases.kuka_variant); the 4, 5 and 8 joint chains follow the short path of
test_gpu_chain_lengths.py.  The horizons sit on the edges of the sweeps' index arithmetic: nK = 1 and 2 (fewer knots than the two-slot prefetch ring of
step_instance_zc), odd / even (the ring's two-fold unrolled loop and its remainder), 16 / 17 and 32 / 33 (steps of the persistent kernel's cyclic
reduction), 63 / 64 / 65 (every lane of k_tail's wavefront owns a knot; first horizon that must fall back to the batched kernels), 129, 254 (T = 256 =
OH_MAX_T).  The path keeps the headline's knot spacing: Tmax = 10 (T - 1) / 49.

Every case has three instances, tiled to a batch of 67 (instance b of the batch is instance b % 3: the copies straddle a wavefront).  The seed of an
instance is NOT the constant trajectory: q_t = qc + cumsum(U(-0.12, 0.12) dt) on the free knots -- with the constant seed every Z_t is the same matrix
and an off-by-one in a sweep's interval index is invisible.

References.  The Newton step of a system is solved at 50 digits (oracle/blocktri_mp.py) in two forms: the reduced system the numpy port hands its own
solver (Z^T D Z, -2 kappa Z_t^T Z_{t+1}), and the saddle-point form [[D_t + mu I, Jc_t^T], [Jc_t, 0]] with the coupling diag(-(2 kappa + w_next), 0, 0, 0)
and the right side [-G_t; 0], which needs no null-space basis.  Beyond the first step the reference is the numpy port (oracle/structured.py:
solve_structured_lm), whose every step is certified against both forms here.

Graded caps.  lm_accept refuses a trial whose retraction did not converge.  On four and five joints (one or two degrees of freedom a knot against the six
rows of a trial's retraction) every trial is refused until the damping has shortened the step, whatever the seed -- also from the constant one -- and
under exact curvature six joints with 64 free knots refuse their first trials too: at max_iter = 1, 2, 3 such a solve returns its retracted seed and
grades no sweep.  So each curvature of a case is graded at the caps k, k + 1, k + 2, k = the first cap by which every instance has accepted a step
(FIRST_CAP, measured: 1 on most cases, 2 under Gauss-Newton on three long horizons, 4 and 7 under exact curvature on kuka6 at 64 and 65 knots, 7 on
kuka4 / kuka5).  Where k = 1 the first graded cap is the
first system's step and is graded against mp through the retraction; otherwise the three caps are graded against the port, whose systems of those
iterations are certified in mp.  test_locked_steps_cpu.py asserts that every case grades an accepted step.

SEEDS, FIRST_CAP, PORT_STEP_ERR and SENS below were found / measured on the CPU by `python tests/locked_step_cases.py` and are re-checked by
test_locked_steps_cpu.py; they are not chosen.  A seed is refused unless no discrete decision up to the last graded cap is near flipping (margins
below) and the port run from a seed perturbed by a few ulp takes the same decisions.

The vel variant (kuka7, kuka6) adds joint-velocity rows at +-VMAX with the walk at 2 VMAX, so rows are violated at the first evaluation and the
coupling blocks diag(2 kappa + w_next) differ from interval to interval and joint to joint; it runs the port's default (hybrid) curvature at every
cap, and a seed must also keep |lam - rho g| >= 1e-6 on every velocity row of every evaluation up to the last graded cap.
Not covered by this table: a parameterised lead joint (k_eval_lead).
"""
import sys
import zlib

import numpy as np

from conftest import KUKA_KIN
from free_sweep_cases import FLOOR, MARGIN, kuka_variant
from oracle.robot import OracleRobot
from oracle.structured import StructuredFigureEight, retract, retract_tol, solve_structured_lm

N_INST, BATCH = 3, 67
WALK = 0.12          # rad/s, the seed's random walk
QC_SPREAD = 0.05     # rad, the instances' qc around the nominal configuration (test_gpu_chain_lengths.py)
TOL, TOL_FEAS = 1e-6, 1e-9
VMAX = 0.06          # rad/s, the velocity rows of the vel variant: half the walk, so rows are violated at the first evaluation (free_sweep_cases.py)
ROWS_GAP = 1e-6      # |lam - rho g| of every velocity row of every evaluation up to the last graded cap (free_sweep_cases.py)
FIRST_CAP_MAX = 24  # a seed is refused unless every instance accepts a step within this many
CURVATURES = ("gauss_newton", "exact")  # plain: the graded caps; the full solve runs hybrid
VEL_CURVATURES = ("hybrid",)  # vel: the port's default throughout


def curvatures(case):
    return VEL_CURVATURES if case[1] == "vel" else CURVATURES


def max_iter_full(case):
    return 1000 if case[1] == "vel" else 300


MP_SADDLE_MAX_NK = 65  # up to here every system of caps 1-3 goes through mp in both forms; beyond, the first system in the reduced form

HORIZONS = {
    "kuka7": (1, 2, 3, 4, 5, 16, 17, 32, 33, 63, 64, 65, 129, 254),
    "kuka6": (1, 2, 5, 64, 65),
    "kuka4": (3, 64, 65),
    "kuka5": (3, 64, 65),
    "kuka8": (3, 64, 65),
}
NDOF = {"kuka7": 7, "kuka6": 6, "kuka4": 4, "kuka5": 5, "kuka8": 8}
VEL_HORIZONS = {"kuka7": (1, 2, 3, 5, 63, 64, 65), "kuka6": (2, 65)}
CASES = [(r, "plain", nk) for r in HORIZONS for nk in HORIZONS[r]] + [(r, "vel", nk) for r in VEL_HORIZONS for nk in VEL_HORIZONS[r]]
QN = np.deg2rad([0, 30, 0, -90, 0, -30, 0, 20])  # test_gpu_chain_lengths.py

# decision margins a seed must keep over the first three iterations (both curvatures)
RATIO_GAP = 1e-3      # |ratio - 1e-4| of every ratio test
RETRACT_FACTOR = 1.001  # every "another correction?" and every settled test of a retraction: value / threshold outside (1 / 1.001, 1.001).
                      # A factor 2 cannot be had: the tolerance of a trial's retraction is tied to the decrease its step predicts (retract_tol), and
                      # the residuals after the second correction land at 0.05 ... 5 times that tolerance on every knot (listing: 60 seeds of
                      # kuka7-plain-nK5 reach 1.01 ... 2.3 on ~80 tests a run; 254 knots have ~15 000 tests).  What two correct implementations can
                      # differ by is far smaller: a residual after a correction is second order in the correction dq (~1e-4), and their dq agree to
                      # bound / |dq| ~ 1e-8 relative, so 1e-3 relative leaves five decades; the perturbed port must take the same decisions besides.
PIVOT_GAP = 1e-6      # every Cholesky pivot of a solve, relative to its diagonal entry
SWITCH_FACTOR = 1.1   # the reduced gradient of every accepted point is this factor away from the hybrid switch 1e-5 w_path, on either side: the
                      # switch also decides the retraction's tolerance (retract_tol), under every curvature, and a horizon of one or two free
                      # knots is past it within three steps whatever the seed -- so "not near" is asked, not "not crossed".  (A factor 2 refuses
                      # every seed of kuka8-plain-nK3, whose Gauss-Newton runs all pass 1.3e-2 ... 1.9e-2; two implementations' reduced gradients
                      # differ by ~1e-8 relative.)


def case_id(case):
    return "%s-%s-nK%d" % case


def robot(tmp_path, name):
    """-> (kin file, tracked link, nominal configuration)"""
    n = NDOF[name]
    if name == "kuka7":
        return KUKA_KIN, "end_effector_ball", QN[:7]
    kin, link = kuka_variant(tmp_path, n)
    return kin, link, QN[:n]


def pivot_margin(D, E, mu):
    """The block Cholesky of blocktridiag(E^T, D + mu I, E), pivot by pivot: min |d_j / S_jj| over every pivot reached (d_j = S_jj - sum_k L_jk^2; the
    factorisation -- and this walk -- stops at the first pivot that is not positive)."""
    N, m = D.shape[0], D.shape[1]
    S = D[0] + mu * np.eye(m)
    worst = np.inf
    for t in range(N):
        L = np.zeros((m, m))
        for j in range(m):
            d = S[j, j] - L[j, :j] @ L[j, :j]
            worst = min(worst, abs(d) / abs(S[j, j]))
            if not d > 0.0:
                return worst
            L[j, j] = np.sqrt(d)
            L[j + 1 :, j] = (S[j + 1 :, j] - L[j + 1 :, :j] @ L[j, :j]) / L[j, j]
        if t < N - 1:
            F = np.linalg.solve(L, E[t]).T
            S = D[t + 1] + mu * np.eye(m) - F @ F.T
    return worst


def _sym(A):
    return 0.5 * (A + np.swapaxes(A, 1, 2))  # (the float64 Dr and Dfull of the port are symmetric to rounding only: solve_mp checks its residual to 1e-40)


def reduced_step_mp(rec):
    """z (nK, n - 3) of the reduced system at 50 digits."""
    from oracle.blocktri_mp import solve_mp

    return solve_mp(_sym(rec["Dr"]), rec["Er"], -rec["gt"], rec["mu"])[0]


def saddle_step_mp(rec, kappa):
    """The step d (nK, n) of the free knots from the saddle-point form at 50 digits: no null-space basis."""
    from oracle.blocktri_mp import solve_mp

    Df, Jc, G, wn = _sym(rec["Dfull"][2:]), rec["Jc"][2:], rec["G"][2:], rec["wnext"][2:]
    nK, n = G.shape
    K = np.zeros((nK, n + 3, n + 3))
    K[:, :n, :n] = Df + rec["mu"] * np.eye(n)[None]
    K[:, :n, n:] = np.swapaxes(Jc, 1, 2)
    K[:, n:, :n] = Jc
    E = np.zeros((nK - 1, n + 3, n + 3))
    for t in range(nK - 1):
        E[t, :n, :n] = np.diag(-(2.0 * kappa + wn[t]))
    rhs = np.concatenate([-G, np.zeros((nK, 3))], 1)
    return solve_mp(K, E, rhs, 0.0)[0][:, :n]


class Case:
    """The three instances of a case: everything the port and the library need."""

    def __init__(self, tmp_path, case, seed=None):
        self.case = case
        self.robot, self.variant, self.nK = case
        self.kin, self.link, qn = robot(tmp_path, self.robot)
        self.orc = OracleRobot(self.kin)
        self.n = n = self.orc.ndof
        self.T = T = self.nK + 2
        self.prob = StructuredFigureEight(self.orc, self.link, T=T, Tmax=10.0 * (T - 1) / 49.0)
        if n not in (6, 7):  # test_gpu_chain_lengths.py: four joints leave ONE degree of freedom per knot: a short path, the tool moved along its local z too
            self.prob.local_path = self.prob.local_path * (0.25 if n < 6 else 1.0)
            self.prob.local_path[:, 2] = 0.6 * self.prob.local_path[:, 0]
        self.dt = self.prob.dt
        self.seed = SEEDS[case] if seed is None else seed
        rng = np.random.default_rng(self.seed)
        self.qc = qn + rng.uniform(-QC_SPREAD, QC_SPREAD, (N_INST, n))
        steps = rng.uniform(-WALK, WALK, (N_INST, self.nK, n)) * self.dt
        self.Q0 = np.repeat(self.qc[:, None, :], T, axis=1)
        self.Q0[:, 2:] += np.cumsum(steps, 1)
        u = np.random.default_rng(zlib.crc32(case_id(case).encode())).uniform(-1.0, 1.0, self.Q0.shape)
        self.Q0_pert = self.Q0.copy()
        self.Q0_pert[:, 2:] *= 1.0 + 4.0 * 2.0**-53 * u[:, 2:]  # free_sweep_cases.sensitivity's perturbation, here on the seed: it goes through the retraction
        self.vlimits = (np.full(n, -VMAX), np.full(n, VMAX)) if self.variant == "vel" else None
        self.curvatures = curvatures(case)
        self.max_iter_full = max_iter_full(case)
        # the instances whose full solve is graded: with velocity rows a long horizon takes 600 ... 900 steps (5 s a solve in the port, and a count that
        # moves by 10 % under a perturbation of a few ulp on most seeds): there the full solve is graded on instance 0 only; no horizon is dropped
        self.full_instances = (0,) if self.variant == "vel" and self.nK >= 63 else tuple(range(N_INST))
        self._refs = None
        self.first_cap = None  # (the search sets what it measured; otherwise FIRST_CAP)

    # ---- the numpy port ----
    def port(self, i, cap, hessian, Q0=None, on_system=None):
        return solve_structured_lm(self.prob, self.qc[i], Q0=self.Q0[i] if Q0 is None else Q0, max_iter=cap, tol=TOL, tol_feas=TOL_FEAS, hessian=hessian,
                                   vlimits=self.vlimits, on_system=on_system)

    def caps(self, curvature):
        """The three graded caps of a curvature: the first cap by which every instance has accepted a step (FIRST_CAP, measured) and the two after it."""
        k = FIRST_CAP[self.case][self.curvatures.index(curvature)] if self.first_cap is None else self.first_cap[curvature]
        return (k, k + 1, k + 2)

    def port_systems(self, i, cap, hessian, Q0=None):
        """The port at the cap and every linear solve it did: [the accepted point's record + dict(iteration, mu, z) + the hook's info (accept, ratio,
        converged, polish_margin, zero_step, stat, hyb_switch, retraction): what decided the evaluation before the solve]."""
        recs = []

        def hook(it, cur, mu, z, info):
            rec = {k: cur[k] for k in ("Q", "Z", "gt", "Dr", "Er", "e", "G", "Dfull", "Jc", "wnext", "f")}
            rec.update(info, iteration=it, mu=float(mu), z=None if z is None else z.copy())
            recs.append(rec)

        return self.port(i, cap, hessian, Q0=Q0, on_system=hook), recs

    def retracted_step(self, rec, d):
        """The point the port's state machine reaches from the accepted point of `rec` with the step d (nK, n) of the free knots: Q_acc + d through
        the retraction with the target e + Jp d, at the port's tolerance for the decrease the port's own step predicts."""
        prob = self.prob
        _, Rc = prob.references(rec["Q"][0])
        gd, z2 = float(np.sum(rec["gt"] * rec["z"])), float(np.sum(rec["z"] * rec["z"]))
        pred = -gd + 0.5 * (gd + rec["mu"] * z2)
        e, _, Jp, _ = prob.chain.jac(rec["Q"])
        Qt, e_tgt = rec["Q"].copy(), e.copy()
        Qt[2:] += d
        e_tgt[2:] += np.einsum("tmi,ti->tm", Jp[2:], d)
        return retract(prob, Qt, Rc, tol=retract_tol(TOL_FEAS, pred, rec["stat"] > rec["hyb_switch"], True), e_tgt=e_tgt)

    def step_mp(self, rec):
        """The Newton step d (nK, n) of a system at 50 digits: the saddle-point form up to MP_SADDLE_MAX_NK free knots, Z z of the reduced system beyond."""
        if self.nK <= MP_SADDLE_MAX_NK:
            return saddle_step_mp(rec, self.prob.kappa)
        return np.einsum("tia,ta->ti", rec["Z"][2:], reduced_step_mp(rec))

    def references(self):
        """What the compiled port and the kernels are graded against, computed once per case: per instance the retracted seed (cap 0), the port at every
        graded cap of each curvature and at the full solve, the first step through mp and the retraction where the first graded cap is 1, the largest
        step of the graded iterations."""
        if self._refs is None:
            out = dict(port={}, cap1={}, seed={}, step_inf=0.0)
            for i in range(N_INST):
                out["seed"][i] = self.port(i, 0, "gauss_newton")["Q"]  # (the seed through the first retraction: what a solve without an accepted step returns)
                for h in self.curvatures:
                    caps = self.caps(h)
                    res, recs = self.port_systems(i, caps[2], h)
                    out["step_inf"] = max([out["step_inf"]] + [float(np.abs(np.einsum("tia,ta->ti", r["Z"][2:], r["z"])).max()) for r in recs
                                                               if r["z"] is not None and caps[0] - 1 <= r["iteration"] < caps[2]])
                    out["port"][(caps[2], h, i)] = res
                    for cap in caps[:2]:
                        out["port"][(cap, h, i)] = self.port(i, cap, h)
                    if caps[0] == 1:  # every instance accepts its first trial: cap 1 is the first system's step, graded against mp
                        first = [r for r in recs if r["iteration"] == 0 and r["z"] is not None][0]  # (the solve whose step is taken: after any raise of the damping)
                        out["cap1"][(h, i)] = self.retracted_step(first, self.step_mp(first))
                if i in self.full_instances:
                    out["port"][("full", "hybrid", i)] = self.port(i, self.max_iter_full, "hybrid")
            self._refs = out
        return self._refs

    # ---- the library ----
    def backend(self, max_iter, hessian):
        from optas_amd import _lib
        from optas_amd.backend import FigureEightBackend
        from optas_amd.models import RobotModel

        mode = {"gauss_newton": _lib.OH_HESSIAN_GAUSS_NEWTON, "exact": _lib.OH_HESSIAN_EXACT, "hybrid": _lib.OH_HESSIAN_HYBRID}[hessian]
        g = None
        if self.variant == "vel":
            g = _lib.oh_guards()
            g.vel_limits = 1
            for j in range(self.n):
                g.dq_lo[j], g.dq_up[j] = -VMAX, VMAX
        return FigureEightBackend(RobotModel(urdf_filename=self.kin).kinematic_chain(self.link), self.T, self.dt, self.prob.local_path, max_iter=max_iter,
                                  tol=TOL, tol_feas=TOL_FEAS, hessian=mode, guards=g)

    def batch(self):
        """x0 (67, nx) and p (67, n): instance b of the batch is instance b % 3 of the case."""
        idx = np.arange(BATCH) % N_INST
        x0 = np.concatenate([self.Q0[idx].reshape(BATCH, -1), np.zeros((BATCH, self.n * (self.T - 1)))], 1)
        return x0, np.ascontiguousarray(self.qc[idx])

    def linear_rows(self, x, qc):
        """a(x) of the literal problem (oracle/problems.py:FigureEightNLP): [qc - q_0; -dq_0; q_{t+1} - q_t - dt dq_t] -> max |.|"""
        Q, dQ = x[: self.n * self.T].reshape(self.T, self.n), x[self.n * self.T :].reshape(self.T - 1, self.n)
        return max(float(np.abs(qc - Q[0]).max()), float(np.abs(dQ[0]).max()), float(np.abs(Q[1:] - Q[:-1] - self.dt * dQ).max()))

    def orientation_rows(self, Q, qc):
        """max |quat(q_t) - quat(qc)| over the knots."""
        quat = self.orc.quaternion_batch(self.link, np.concatenate([qc[None], Q]))
        return float(np.abs(quat[1:] - quat[:1]).max())


def bound(case, pos, step_inf):
    """pos: 0, 1, 2 -- the position of the cap among the three graded caps of its curvature."""
    return max(MARGIN * max(PORT_STEP_ERR[case], SENS[case][pos]), FLOOR) * max(1.0, step_inf)


def grade(c, refs, cap, curvature, X, f, iters, status, tag):
    """The rules of a solve at a cap, for B = len(X) instances (instance b is instance b % 3): shared by test_locked_steps_cpu.py (compiled port) and
    test_gpu_locked_steps.py (every launch path).  X: (B, T, n) knots.  -> the largest |Q - Q_ref| / bound (graded caps) or None."""
    worst = None
    for b in range(len(X)):
        i = b % N_INST
        if cap == "full" and i not in c.full_instances:
            continue
        pr = refs["port"][(cap, curvature, i)]
        assert np.isfinite(X[b]).all(), (tag, b)
        assert np.array_equal(X[b, 0], c.qc[i]) and np.array_equal(X[b, 1], c.qc[i]), (tag, b, "q_0 = q_1 = qc")
        if cap == "full":
            assert status[b] == 0 and pr["status"] == 0, (tag, b, status[b], pr["status"])
            assert abs(f[b] - pr["f"]) <= 1e-9 * max(1.0, abs(pr["f"])), (tag, b, f[b], pr["f"])
            assert abs(int(iters[b]) - pr["iters"]) <= max(2, pr["iters"] // 20), (tag, b, int(iters[b]), pr["iters"])
            assert c.orientation_rows(X[b], c.qc[i]) <= 1e-9, (tag, b)
            continue
        pos = c.caps(curvature).index(cap)
        bnd = bound(c.case, pos, refs["step_inf"])
        # the first system's step at 50 digits through the retraction where the graded caps start at 1, the port otherwise
        ref = refs["cap1"][(curvature, i)] if cap == 1 else pr["Q"]
        err = float(np.abs(X[b] - ref).max())
        worst = max(worst or 0.0, err / bnd)
        assert np.abs(X[b] - refs["seed"][i]).max() > 1e-6, (tag, b, "the seed came back")  # (every graded cap holds an accepted step)
        assert err <= bnd, (tag, b, "|Q - Q_ref| %.3e, bound %.3e" % (err, bnd))
        assert int(iters[b]) == pr["iters"], (tag, b, int(iters[b]), pr["iters"])
    return worst


def first_moving_cap(c, i, h):
    """The first cap at which the port returns something else than the retracted seed (None: not within FIRST_CAP_MAX).  Measured on the returned knots, not
    read off the accept flags: with velocity rows a refused step is followed by shorter trials along it, which count as steps."""
    seed = c.port(i, 0, h)["Q"]
    for cap in range(1, FIRST_CAP_MAX + 1):
        if np.abs(c.port(i, cap, h)["Q"] - seed).max() > 1e-6:
            return cap
    return None


def decisions(recs, cap):
    """The discrete decisions of a port run up to the cap, and how far each is from flipping."""
    out = dict(accepts=[], ratio_gap=np.inf, retract=np.inf, pivot=np.inf, switch=np.inf, rows=np.inf, rejected=0)
    seen = set()
    for r in recs:
        if r["iteration"] > cap:
            continue
        if r["iteration"] not in seen:  # (a raised damping solves again after the same evaluation)
            seen.add(r["iteration"])
            out["accepts"].append(r["accept"])
            out["rows"] = min(out["rows"], r.get("rows", np.inf))
            margins = [v for _, v in r["retraction"]]
            if r["ratio"] is not None:
                out["ratio_gap"] = min(out["ratio_gap"], abs(r["ratio"] - 1e-4))
                margins.append(r["converged"])  # lm_accept: has the trial's retraction converged?
                if not r["accept"]:
                    out["rejected"] += 1
                    margins.append(r["polish_margin"])  # ... and does the accepted point's violation ask for a polish?
            for v in margins:
                out["retract"] = min(out["retract"], np.inf if v == 0.0 else max(v, 1.0 / v))
            v = r["stat"] / r["hyb_switch"]
            out["switch"] = min(out["switch"], max(v, 1.0 / v) if v > 0.0 else np.inf)
        if r["iteration"] < cap:
            out["pivot"] = min(out["pivot"], pivot_margin(r["Dr"], r["Er"], r["mu"]))
    return out


def decisions_ok(d):
    return (d["ratio_gap"] > RATIO_GAP and d["retract"] >= RETRACT_FACTOR and d["pivot"] >= PIVOT_GAP and d["switch"] >= SWITCH_FACTOR
            and d["rows"] >= ROWS_GAP)


def measure(tmp_path, case, seed=None, mp=True):
    """Everything the CPU test asserts about a case -> dict.  mp = False: the decisions only (what the seed search looks at first).
    The graded caps of a curvature are k, k + 1, k + 2 with k the first cap by which every instance has accepted a step: lm_accept refuses a trial whose
    retraction did not converge, and on four and five joints (one or two degrees of freedom a knot against six rows of the trial's retraction) every
    trial is refused until the damping has shortened the step -- at caps 1, 2, 3 such a solve returns the retracted seed and grades no sweep."""
    c = Case(tmp_path, case, seed)
    out = dict(case=c, ok=True, hook_neutral=True, port_err=0.0, sens=[0.0, 0.0, 0.0], rejected=0, ratio_gap=np.inf, retract=np.inf, pivot=np.inf,
               switch=np.inf, rows=np.inf, step_inf=0.0, full=[], why="", first_cap={})
    for h in c.curvatures:
        ks = [first_moving_cap(c, i, h) for i in range(N_INST)]
        if None in ks:
            out["ok"], out["why"] = False, "no accepted step within %d steps under %s: %s" % (FIRST_CAP_MAX, h, ks)
            return out
        out["first_cap"][h] = max(ks)
    c.first_cap = out["first_cap"]
    systems = []
    for i in range(N_INST):
        for h in c.curvatures:
            caps = c.caps(h)
            res, recs = c.port_systems(i, caps[2], h)
            d = decisions(recs, caps[2])
            for k in ("ratio_gap", "retract", "pivot", "switch", "rows"):
                out[k] = min(out[k], d[k])
            out["rejected"] += d["rejected"]
            if not decisions_ok(d):
                out["ok"], out["why"] = False, "decision margins of instance %d, %s: %s" % (i, h, {k: d[k] for k in ("accepts", "ratio_gap", "retract", "pivot", "switch", "rows")})
                return out
            # the perturbed seed: same decisions, and how far the knots move at every cap
            resp, recsp = c.port_systems(i, caps[2], h, Q0=c.Q0_pert[i])
            dp = decisions(recsp, caps[2])
            if dp["accepts"] != d["accepts"] or resp["iters"] != res["iters"] or resp["rejected"] != res["rejected"] or not decisions_ok(dp):
                out["ok"], out["why"] = False, "the perturbed port of instance %d, %s decides otherwise" % (i, h)
                return out
            plain = c.port(i, caps[2], h)
            out["hook_neutral"] &= set(plain) == set(res) and all(np.array_equal(np.asarray(res[k]), np.asarray(plain[k])) for k in res)
            for pos, cap in enumerate(caps):
                a = res if pos == 2 else c.port(i, cap, h)
                b = resp if pos == 2 else c.port(i, cap, h, Q0=c.Q0_pert[i])
                if a["iters"] != b["iters"] or a["rejected"] != b["rejected"]:
                    out["ok"], out["why"] = False, "the perturbed port of instance %d, %s counts otherwise at cap %d" % (i, h, cap)
                    return out
                out["sens"][pos] = max(out["sens"][pos], float(np.abs(a["Q"] - b["Q"]).max()))
            graded = [r for r in recs if r["z"] is not None and caps[0] - 1 <= r["iteration"] < caps[2]]  # the systems whose steps the graded caps add
            systems += [r for r in graded if c.nK <= MP_SADDLE_MAX_NK or (r["iteration"] == caps[0] - 1 and h == c.curvatures[0])]
            out["step_inf"] = max([out["step_inf"]] + [float(np.abs(np.einsum("tia,ta->ti", r["Z"][2:], r["z"])).max()) for r in graded])
            out["wnext_values"] = max(out.get("wnext_values", 0), max(len(np.unique(np.round(r["wnext"][2:-1], 9))) for r in graded))
        # the full solve: not on a watershed
        if i not in c.full_instances:
            continue
        a, b = c.port(i, c.max_iter_full, "hybrid"), c.port(i, c.max_iter_full, "hybrid", Q0=c.Q0_pert[i])
        out["full"].append((a["status"], a["iters"], a["f"], b["status"], b["iters"], b["f"]))
        if not (a["status"] == 0 and b["status"] == 0 and abs(a["f"] - b["f"]) <= 1e-9 * max(1.0, abs(a["f"])) and abs(a["iters"] - b["iters"]) <= max(2, a["iters"] // 20)):
            out["ok"], out["why"] = False, "full solve of instance %d: %s" % (i, out["full"][-1])
            return out
    if mp:
        for r in systems:
            dz = np.einsum("tia,ta->ti", r["Z"][2:], r["z"])
            z_mp = reduced_step_mp(r)
            out["port_err"] = max(out["port_err"], float(np.abs(r["z"] - z_mp).max()))
            if c.nK <= MP_SADDLE_MAX_NK:
                out["port_err"] = max(out["port_err"], float(np.abs(dz - saddle_step_mp(r, c.prob.kappa)).max()))
    return out


# ---- found / measured by `python tests/locked_step_cases.py` ----
# 2026-10-21, numpy 2.2.6, mpmath 1.3.0
# kuka7-plain-nK1    seed  14244 ( 0 refused) first caps [1, 1] port 5.06e-14 sens 3.34e-14 4.77e-15 3.33e-15 |step| 0.422 rejected 0 ratio gap 7.2e-01 retract 1.01411 pivot 3.8e-02 switch 3.46 full [4, 4, 4] (2.5 s)
# kuka7-plain-nK2    seed  85726 ( 0 refused) first caps [1, 1] port 1.81e-13 sens 2.06e-13 5.98e-14 4.54e-15 |step| 0.460 rejected 0 ratio gap 6.5e-01 retract 1.00971 pivot 1.7e-02 switch 2.02 full [4, 4, 4] (3.1 s)
# kuka7-plain-nK3    seed  78408 ( 0 refused) first caps [1, 1] port 1.39e-13 sens 1.87e-13 1.18e-14 1.12e-14 |step| 0.574 rejected 0 ratio gap 4.3e-01 retract 1.01244 pivot 8.6e-03 switch 3.38 full [4, 4, 4] (2.8 s)
# kuka7-plain-nK4    seed  41099 ( 0 refused) first caps [1, 1] port 7.90e-14 sens 1.57e-13 5.09e-14 7.83e-15 |step| 0.594 rejected 0 ratio gap 5.0e-01 retract 1.00994 pivot 5.9e-03 switch 4.17 full [4, 4, 4] (2.4 s)
# kuka7-plain-nK5    seed  35901 ( 0 refused) first caps [1, 1] port 3.34e-13 sens 8.62e-13 2.07e-13 2.19e-14 |step| 0.547 rejected 0 ratio gap 6.5e-01 retract 1.03355 pivot 5.1e-03 switch 2.87 full [4, 4, 4] (2.8 s)
# kuka7-plain-nK16   seed  43634 ( 0 refused) first caps [1, 1] port 1.19e-12 sens 2.00e-12 2.11e-12 9.34e-13 |step| 0.492 rejected 0 ratio gap 8.2e-01 retract 1.01372 pivot 5.1e-03 switch 3.38 full [11, 7, 12] (7.8 s)
# kuka7-plain-nK17   seed  35748 ( 0 refused) first caps [1, 1] port 2.42e-12 sens 4.71e-12 6.72e-12 5.70e-12 |step| 0.518 rejected 0 ratio gap 8.4e-01 retract 1.01164 pivot 1.2e-03 switch 2.43 full [8, 7, 7] (8.3 s)
# kuka7-plain-nK32   seed  79945 ( 0 refused) first caps [1, 1] port 2.41e-12 sens 2.64e-12 3.43e-12 3.64e-12 |step| 0.613 rejected 0 ratio gap 5.3e-01 retract 1.00481 pivot 2.4e-03 switch 5.26 full [7, 14, 24] (12.8 s)
# kuka7-plain-nK33   seed  96960 ( 1 refused) first caps [1, 1] port 6.68e-12 sens 4.66e-12 7.37e-12 8.50e-12 |step| 0.699 rejected 0 ratio gap 7.8e-01 retract 1.00133 pivot 6.5e-03 switch 10.11 full [8, 22, 15] (14.7 s)
# kuka7-plain-nK63   seed   7868 ( 2 refused) first caps [1, 1] port 1.27e-11 sens 1.39e-11 2.46e-11 2.95e-11 |step| 0.868 rejected 0 ratio gap 4.1e-01 retract 1.00748 pivot 2.4e-03 switch 5.43 full [8, 28, 16] (32.8 s)
# kuka7-plain-nK64   seed  47129 ( 0 refused) first caps [1, 1] port 3.32e-11 sens 1.13e-11 1.41e-11 2.12e-11 |step| 2.572 rejected 0 ratio gap 4.9e-01 retract 1.00506 pivot 2.8e-03 switch 16.30 full [9, 21, 8] (26.5 s)
# kuka7-plain-nK65   seed  33391 ( 0 refused) first caps [1, 1] port 1.77e-11 sens 2.10e-11 2.48e-11 3.86e-11 |step| 0.703 rejected 0 ratio gap 7.0e-01 retract 1.00585 pivot 2.5e-03 switch 9.64 full [30, 8, 17] (22.4 s)
# kuka7-plain-nK129  seed   5602 ( 1 refused) first caps [1, 1] port 1.16e-11 sens 4.53e-11 6.25e-11 9.28e-11 |step| 0.979 rejected 0 ratio gap 8.8e-01 retract 1.00183 pivot 6.3e-04 switch 12.32 full [11, 8, 9] (19.2 s)
# kuka7-plain-nK254  seed  19940 ( 2 refused) first caps [2, 1] port 3.19e-12 sens 9.14e-11 8.39e-11 4.85e-11 |step| 0.960 rejected 1 ratio gap 8.4e-01 retract 1.00184 pivot 1.4e-03 switch 7.31 full [27, 26, 9] (55.0 s)
# kuka6-plain-nK1    seed  80708 ( 0 refused) first caps [1, 1] port 9.44e-16 sens 1.44e-15 8.33e-16 5.55e-16 |step| 0.491 rejected 0 ratio gap 2.4e-01 retract 1.73829 pivot 7.2e-01 switch 19.07 full [3, 3, 3] (1.1 s)
# kuka6-plain-nK2    seed  84638 ( 0 refused) first caps [1, 1] port 3.90e-11 sens 2.44e-15 2.44e-15 2.44e-15 |step| 95.937 rejected 0 ratio gap 5.6e-01 retract 1.65107 pivot 1.9e-02 switch 13.82 full [3, 3, 3] (1.3 s)
# kuka6-plain-nK5    seed  36253 ( 0 refused) first caps [1, 1] port 4.33e-15 sens 3.33e-15 8.88e-15 7.11e-15 |step| 1.016 rejected 0 ratio gap 3.7e-01 retract 1.01412 pivot 6.7e-01 switch 18.12 full [3, 3, 3] (1.8 s)
# kuka6-plain-nK64   seed  44024 ( 2 refused) first caps [1, 4] port 3.44e-15 sens 1.61e-15 1.22e-15 1.33e-15 |step| 0.645 rejected 8 ratio gap 2.4e-01 retract 1.00222 pivot 2.0e-02 switch 16.20 full [4, 4, 4] (17.5 s)
# kuka6-plain-nK65   seed  11713 ( 1 refused) first caps [1, 7] port 3.00e-15 sens 5.05e-15 1.78e-15 1.33e-15 |step| 0.812 rejected 10 ratio gap 2.5e-02 retract 1.00271 pivot 4.9e-02 switch 1.60 full [4, 4, 4] (20.2 s)
# kuka4-plain-nK3    seed   4681 ( 0 refused) first caps [7, 7] port 2.08e-17 sens 6.59e-11 5.82e-11 1.49e-10 |step| 0.032 rejected 28 ratio gap 9.9e-01 retract 1.00329 pivot 1.0e+00 switch 1.34 full [16, 16, 6] (1.8 s)
# kuka4-plain-nK64   seed   7147 ( 2 refused) first caps [7, 7] port 5.55e-17 sens 1.16e-10 6.11e-10 7.45e-10 |step| 0.089 rejected 36 ratio gap 9.9e-01 retract 1.00125 pivot 1.0e+00 switch 854.72 full [17, 30, 51] (17.9 s)
# kuka4-plain-nK65   seed  73439 ( 0 refused) first caps [7, 7] port 4.16e-17 sens 7.28e-11 5.53e-10 1.13e-09 |step| 0.074 rejected 36 ratio gap 9.4e-01 retract 1.00286 pivot 1.0e+00 switch 659.88 full [19, 18, 42] (14.5 s)
# kuka5-plain-nK3    seed  11305 ( 0 refused) first caps [7, 7] port 3.47e-17 sens 2.91e-11 3.78e-10 3.10e-10 |step| 0.045 rejected 36 ratio gap 9.8e-01 retract 1.29856 pivot 9.8e-01 switch 452.75 full [16, 42, 18] (3.0 s)
# kuka5-plain-nK64   seed  64582 ( 0 refused) first caps [7, 7] port 4.86e-17 sens 2.62e-10 4.36e-10 2.54e-10 |step| 0.047 rejected 36 ratio gap 9.5e-01 retract 1.00106 pivot 9.5e-01 switch 1581.12 full [43, 45, 45] (18.3 s)
# kuka5-plain-nK65   seed  11568 ( 0 refused) first caps [7, 7] port 5.55e-17 sens 4.07e-10 6.99e-10 8.09e-10 |step| 0.061 rejected 36 ratio gap 9.4e-01 retract 1.00270 pivot 9.6e-01 switch 672.47 full [70, 34, 54] (20.3 s)
# kuka8-plain-nK3    seed   1486 ( 0 refused) first caps [1, 1] port 2.86e-13 sens 1.19e-13 3.71e-13 3.04e-13 |step| 0.545 rejected 0 ratio gap 3.8e-01 retract 1.00265 pivot 8.2e-04 switch 1.19 full [17, 7, 17] (3.3 s)
# kuka8-plain-nK64   seed  12939 ( 3 refused) first caps [2, 1] port 8.42e-12 sens 2.66e-11 2.66e-11 2.66e-11 |step| 0.759 rejected 1 ratio gap 6.3e-01 retract 1.00185 pivot 8.2e-05 switch 6.08 full [26, 28, 26] (36.8 s)
# kuka8-plain-nK65   seed  45182 ( 0 refused) first caps [2, 1] port 1.31e-11 sens 3.05e-11 3.10e-11 3.10e-11 |step| 0.803 rejected 1 ratio gap 7.0e-01 retract 1.00103 pivot 7.7e-05 switch 2.58 full [26, 25, 27] (26.4 s)
# kuka7-vel-nK1      seed  69084 ( 0 refused) first caps [4] port 1.45e-16 sens 3.33e-16 5.55e-16 4.44e-16 |step| 0.034 rejected 0 ratio gap 7.5e-01 retract 1.06387 pivot 3.3e-01 switch 1.24 rows 8.3e+01 full [52, 32, 46] (2.3 s)
# kuka7-vel-nK2      seed  86439 ( 1 refused) first caps [1] port 1.36e-14 sens 2.82e-14 1.14e-15 6.66e-16 |step| 0.383 rejected 0 ratio gap 5.7e-01 retract 1.06450 pivot 2.1e-01 switch 31.20 rows 2.2e+01 full [30, 30, 48] (2.0 s)
# kuka7-vel-nK3      seed  44655 (31 refused) first caps [4] port 2.11e-14 sens 8.47e-16 6.66e-16 6.66e-16 |step| 0.639 rejected 4 ratio gap 1.2e-01 retract 1.01888 pivot 4.4e-02 switch 2.96 rows 7.4e+00 full [56, 70, 72] (38.1 s)
# kuka7-vel-nK5      seed  65029 ( 0 refused) first caps [1] port 9.11e-13 sens 1.70e-12 4.92e-13 1.94e-14 |step| 0.754 rejected 0 ratio gap 4.5e-01 retract 1.06566 pivot 3.7e-02 switch 83.42 rows 9.6e-01 full [54, 96, 66] (2.8 s)
# kuka7-vel-nK63     seed  58893 ( 1 refused) first caps [4] port 4.37e-14 sens 2.70e-11 2.49e-11 2.74e-11 |step| 0.414 rejected 1 ratio gap 5.1e-01 retract 1.00161 pivot 6.6e-03 switch 348.34 rows 1.4e-02 full [664] (26.7 s)
# kuka7-vel-nK64     seed  15536 ( 1 refused) first caps [2] port 6.39e-14 sens 1.17e-11 9.05e-12 1.36e-11 |step| 1.155 rejected 0 ratio gap 3.7e-01 retract 1.00668 pivot 8.3e-03 switch 929.16 rows 2.8e-02 full [700] (57.0 s)
# kuka7-vel-nK65     seed  49370 ( 1 refused) first caps [3] port 6.54e-14 sens 3.92e-12 5.34e-12 5.40e-12 |step| 1.050 rejected 0 ratio gap 3.7e-01 retract 1.00295 pivot 1.9e-02 switch 350.60 rows 1.2e-01 full [857] (49.4 s)
# kuka6-vel-nK2      seed  40197 ( 0 refused) first caps [1] port 2.61e-15 sens 5.55e-16 8.88e-16 4.44e-16 |step| 0.524 rejected 0 ratio gap 1.8e-01 retract 1.01259 pivot 8.2e-01 switch 214.19 rows 8.1e+00 full [33, 32, 30] (3.1 s)
# kuka6-vel-nK65     seed  88136 ( 1 refused) first caps [1] port 2.78e-15 sens 2.72e-15 3.16e-15 1.33e-15 |step| 0.684 rejected 0 ratio gap 3.4e-01 retract 1.00103 pivot 6.3e-01 switch 1079.03 rows 2.2e+00 full [125] (16.7 s)
SEEDS = {
    ('kuka7', 'plain', 1): 14244,
    ('kuka7', 'plain', 2): 85726,
    ('kuka7', 'plain', 3): 78408,
    ('kuka7', 'plain', 4): 41099,
    ('kuka7', 'plain', 5): 35901,
    ('kuka7', 'plain', 16): 43634,
    ('kuka7', 'plain', 17): 35748,
    ('kuka7', 'plain', 32): 79945,
    ('kuka7', 'plain', 33): 96960,
    ('kuka7', 'plain', 63): 7868,
    ('kuka7', 'plain', 64): 47129,
    ('kuka7', 'plain', 65): 33391,
    ('kuka7', 'plain', 129): 5602,
    ('kuka7', 'plain', 254): 19940,
    ('kuka6', 'plain', 1): 80708,
    ('kuka6', 'plain', 2): 84638,
    ('kuka6', 'plain', 5): 36253,
    ('kuka6', 'plain', 64): 44024,
    ('kuka6', 'plain', 65): 11713,
    ('kuka4', 'plain', 3): 4681,
    ('kuka4', 'plain', 64): 7147,
    ('kuka4', 'plain', 65): 73439,
    ('kuka5', 'plain', 3): 11305,
    ('kuka5', 'plain', 64): 64582,
    ('kuka5', 'plain', 65): 11568,
    ('kuka8', 'plain', 3): 1486,
    ('kuka8', 'plain', 64): 12939,
    ('kuka8', 'plain', 65): 45182,
    ('kuka7', 'vel', 1): 69084,
    ('kuka7', 'vel', 2): 86439,
    ('kuka7', 'vel', 3): 44655,
    ('kuka7', 'vel', 5): 65029,
    ('kuka7', 'vel', 63): 58893,
    ('kuka7', 'vel', 64): 15536,
    ('kuka7', 'vel', 65): 49370,
    ('kuka6', 'vel', 2): 40197,
    ('kuka6', 'vel', 65): 88136,
}
FIRST_CAP = {  # (gauss_newton, exact)
    ('kuka7', 'plain', 1): (1, 1),
    ('kuka7', 'plain', 2): (1, 1),
    ('kuka7', 'plain', 3): (1, 1),
    ('kuka7', 'plain', 4): (1, 1),
    ('kuka7', 'plain', 5): (1, 1),
    ('kuka7', 'plain', 16): (1, 1),
    ('kuka7', 'plain', 17): (1, 1),
    ('kuka7', 'plain', 32): (1, 1),
    ('kuka7', 'plain', 33): (1, 1),
    ('kuka7', 'plain', 63): (1, 1),
    ('kuka7', 'plain', 64): (1, 1),
    ('kuka7', 'plain', 65): (1, 1),
    ('kuka7', 'plain', 129): (1, 1),
    ('kuka7', 'plain', 254): (2, 1),
    ('kuka6', 'plain', 1): (1, 1),
    ('kuka6', 'plain', 2): (1, 1),
    ('kuka6', 'plain', 5): (1, 1),
    ('kuka6', 'plain', 64): (1, 4),
    ('kuka6', 'plain', 65): (1, 7),
    ('kuka4', 'plain', 3): (7, 7),
    ('kuka4', 'plain', 64): (7, 7),
    ('kuka4', 'plain', 65): (7, 7),
    ('kuka5', 'plain', 3): (7, 7),
    ('kuka5', 'plain', 64): (7, 7),
    ('kuka5', 'plain', 65): (7, 7),
    ('kuka8', 'plain', 3): (1, 1),
    ('kuka8', 'plain', 64): (2, 1),
    ('kuka8', 'plain', 65): (2, 1),
    ('kuka7', 'vel', 1): (4,),
    ('kuka7', 'vel', 2): (1,),
    ('kuka7', 'vel', 3): (4,),
    ('kuka7', 'vel', 5): (1,),
    ('kuka7', 'vel', 63): (4,),
    ('kuka7', 'vel', 64): (2,),
    ('kuka7', 'vel', 65): (3,),
    ('kuka6', 'vel', 2): (1,),
    ('kuka6', 'vel', 65): (1,),
}
PORT_STEP_ERR = {
    ('kuka7', 'plain', 1): 5.061e-14,
    ('kuka7', 'plain', 2): 1.813e-13,
    ('kuka7', 'plain', 3): 1.391e-13,
    ('kuka7', 'plain', 4): 7.898e-14,
    ('kuka7', 'plain', 5): 3.342e-13,
    ('kuka7', 'plain', 16): 1.191e-12,
    ('kuka7', 'plain', 17): 2.418e-12,
    ('kuka7', 'plain', 32): 2.407e-12,
    ('kuka7', 'plain', 33): 6.678e-12,
    ('kuka7', 'plain', 63): 1.273e-11,
    ('kuka7', 'plain', 64): 3.320e-11,
    ('kuka7', 'plain', 65): 1.768e-11,
    ('kuka7', 'plain', 129): 1.164e-11,
    ('kuka7', 'plain', 254): 3.186e-12,
    ('kuka6', 'plain', 1): 9.437e-16,
    ('kuka6', 'plain', 2): 3.901e-11,
    ('kuka6', 'plain', 5): 4.330e-15,
    ('kuka6', 'plain', 64): 3.442e-15,
    ('kuka6', 'plain', 65): 2.998e-15,
    ('kuka4', 'plain', 3): 2.082e-17,
    ('kuka4', 'plain', 64): 5.551e-17,
    ('kuka4', 'plain', 65): 4.163e-17,
    ('kuka5', 'plain', 3): 3.469e-17,
    ('kuka5', 'plain', 64): 4.857e-17,
    ('kuka5', 'plain', 65): 5.551e-17,
    ('kuka8', 'plain', 3): 2.857e-13,
    ('kuka8', 'plain', 64): 8.422e-12,
    ('kuka8', 'plain', 65): 1.315e-11,
    ('kuka7', 'vel', 1): 1.45e-16,
    ('kuka7', 'vel', 2): 1.36e-14,
    ('kuka7', 'vel', 3): 2.11e-14,
    ('kuka7', 'vel', 5): 9.11e-13,
    ('kuka7', 'vel', 63): 4.37e-14,
    ('kuka7', 'vel', 64): 6.39e-14,
    ('kuka7', 'vel', 65): 6.54e-14,
    ('kuka6', 'vel', 2): 2.61e-15,
    ('kuka6', 'vel', 65): 2.78e-15,
}
SENS = {
    ('kuka7', 'plain', 1): (3.342e-14, 4.765e-15, 3.331e-15),
    ('kuka7', 'plain', 2): (2.057e-13, 5.983e-14, 4.538e-15),
    ('kuka7', 'plain', 3): (1.867e-13, 1.176e-14, 1.116e-14),
    ('kuka7', 'plain', 4): (1.566e-13, 5.090e-14, 7.827e-15),
    ('kuka7', 'plain', 5): (8.622e-13, 2.068e-13, 2.185e-14),
    ('kuka7', 'plain', 16): (1.998e-12, 2.109e-12, 9.343e-13),
    ('kuka7', 'plain', 17): (4.707e-12, 6.718e-12, 5.702e-12),
    ('kuka7', 'plain', 32): (2.637e-12, 3.434e-12, 3.640e-12),
    ('kuka7', 'plain', 33): (4.663e-12, 7.370e-12, 8.498e-12),
    ('kuka7', 'plain', 63): (1.389e-11, 2.461e-11, 2.955e-11),
    ('kuka7', 'plain', 64): (1.130e-11, 1.415e-11, 2.125e-11),
    ('kuka7', 'plain', 65): (2.105e-11, 2.482e-11, 3.865e-11),
    ('kuka7', 'plain', 129): (4.529e-11, 6.252e-11, 9.282e-11),
    ('kuka7', 'plain', 254): (9.143e-11, 8.389e-11, 4.847e-11),
    ('kuka6', 'plain', 1): (1.443e-15, 8.327e-16, 5.551e-16),
    ('kuka6', 'plain', 2): (2.442e-15, 2.442e-15, 2.442e-15),
    ('kuka6', 'plain', 5): (3.331e-15, 8.882e-15, 7.105e-15),
    ('kuka6', 'plain', 64): (1.610e-15, 1.221e-15, 1.332e-15),
    ('kuka6', 'plain', 65): (5.052e-15, 1.776e-15, 1.332e-15),
    ('kuka4', 'plain', 3): (6.594e-11, 5.821e-11, 1.488e-10),
    ('kuka4', 'plain', 64): (1.164e-10, 6.110e-10, 7.446e-10),
    ('kuka4', 'plain', 65): (7.276e-11, 5.533e-10, 1.128e-09),
    ('kuka5', 'plain', 3): (2.910e-11, 3.782e-10, 3.103e-10),
    ('kuka5', 'plain', 64): (2.619e-10, 4.365e-10, 2.539e-10),
    ('kuka5', 'plain', 65): (4.075e-10, 6.985e-10, 8.091e-10),
    ('kuka8', 'plain', 3): (1.193e-13, 3.708e-13, 3.040e-13),
    ('kuka8', 'plain', 64): (2.661e-11, 2.661e-11, 2.661e-11),
    ('kuka8', 'plain', 65): (3.046e-11, 3.103e-11, 3.103e-11),
    ('kuka7', 'vel', 1): (3.33e-16, 5.55e-16, 4.44e-16),
    ('kuka7', 'vel', 2): (2.82e-14, 1.14e-15, 6.66e-16),
    ('kuka7', 'vel', 3): (8.47e-16, 6.66e-16, 6.66e-16),
    ('kuka7', 'vel', 5): (1.70e-12, 4.92e-13, 1.94e-14),
    ('kuka7', 'vel', 63): (2.70e-11, 2.49e-11, 2.74e-11),
    ('kuka7', 'vel', 64): (1.17e-11, 9.05e-12, 1.36e-11),
    ('kuka7', 'vel', 65): (3.92e-12, 5.34e-12, 5.40e-12),
    ('kuka6', 'vel', 2): (5.55e-16, 8.88e-16, 4.44e-16),
    ('kuka6', 'vel', 65): (2.72e-15, 3.16e-15, 1.33e-15),
}
# a case whose graded caps hold rejected steps (the listing above: "rejected" > 0)
# With velocity rows the first seed that keeps the margins has no rejected step inside its graded caps on any of the nine cases (hybrid curvature is
# Gauss-Newton that early): of this case the search asks for one besides (31 seeds that keep the margins pass before it)
REJECT_SOUGHT = {("kuka7", "vel", 3)}
REJECTING = {"plain": ("kuka6", "plain", 64), "vel": ("kuka7", "vel", 3)}  # (exact curvature: the first trials are refused, the damped fourth is accepted)


def _search(tmp_path, case, tries=60):
    base = zlib.crc32(case_id(case).encode()) % 100000
    why = []
    for k in range(tries):
        m = measure(tmp_path, case, seed=base + k, mp=False)
        if m["ok"] and case in REJECT_SOUGHT and m["rejected"] == 0:
            m["ok"], m["why"] = False, "no rejected step inside the graded caps (asked of this case: REJECT_SOUGHT)"
        if m["ok"]:
            return base + k, measure(tmp_path, case, seed=base + k), k
        why.append(m["why"])
    raise RuntimeError("no seed for %s: %s" % (case_id(case), why[-3:]))


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
            seed, m, k = _search(tmp, case)
            rows.append((case, seed, m))
            print("# %-18s seed %6d (%2d refused) first caps %s port %.2e sens %.2e %.2e %.2e |step| %.3f rejected %d ratio gap %.1e retract %.5f pivot %.1e "
                  "switch %.2f rows %.1e full %s (%.1f s)" % (case_id(case), seed, k, [m["first_cap"][h] for h in curvatures(case)], m["port_err"], *m["sens"], m["step_inf"], m["rejected"],
                                                    m["ratio_gap"], m["retract"], m["pivot"], m["switch"], m["rows"], [f[1] for f in m["full"]], time.time() - t), flush=True)
        print("SEEDS = {")
        for case, seed, m in rows:
            print("    %r: %d," % (case, seed))
        print("}\nFIRST_CAP = {  # per curvature of curvatures(case)")
        for case, seed, m in rows:
            print("    %r: %r," % (case, tuple(m["first_cap"][h] for h in curvatures(case))))
        print("}\nPORT_STEP_ERR = {")
        for case, seed, m in rows:
            print("    %r: %.3e," % (case, m["port_err"]))
        print("}\nSENS = {")
        for case, seed, m in rows:
            print("    %r: (%.3e, %.3e, %.3e)," % (case, *m["sens"]))
        print("}")
