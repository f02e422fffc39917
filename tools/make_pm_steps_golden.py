"""Writes tests/golden/pm_steps_mp.npz: the first three iterations of the point-mass interior-point state machine at 50 digits (tests/pm_step_ref.py,
Newton directions by a dense solve of the condensed system, no Riccati recursion) on a grid of variants x horizons x four instances, rounded to float64,
with the inputs and with the numpy port's (oracle/pointmass_ipm.py) distance from them.  CPU only; minutes of mpmath.

    python tools/make_pm_steps_golden.py            # writes the fixture, prints the rejection count
    python tools/make_pm_steps_golden.py --check    # regenerates everything and compares it with the committed fixture, array by array, bit for bit

Per case "<variant>_T<T>_i<slot>" the file holds  _desc (T, dt, w_acc, w_vel, track_final_only, fix_final_velocity, ylim, vlim, safe, tol),
_x0 (4T), _p (4 + 4T), _x (3, 4T), _f (3), _kkt (3, 3) for max_iter = 1, 2, 3, _dist (3, 5): the port's |x - x_mp|_inf, |f - f_mp|, |kkt - kkt_mp|
(3), and _step (3, 2): the step lengths (ap, ad).

An instance is rejected, and the next one drawn, when at any of its three steps min(ap, ad) lies within 1e-6 of 0.9 or 0.5 (the sigma ladder would
branch differently in float64), when it converges or is declared infeasible within three steps, or when the port's status differs from the mp
machine's.  These are conditions on the inputs.  A cell of T >= 5 whose four accepted instances all take a full first step keeps drawing for its
last slot until one is cut by the fraction-to-the-boundary rule (ap < 1); the instances passed over for that are counted apart."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

from oracle.pointmass_ipm import solve_pointmass_ipm  # noqa: E402
from pm_step_ref import pm_steps_mp  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "pm_steps_mp.npz")
SEED = 20261020
YLIM, VLIM, SAFE, TOL = 1.5, 1.0, 0.3, 1e-8
# name: dt, w_acc * T, w_vel * T, track_final_only, fix_final_velocity
VARIANTS = {
    "mpc": (0.05, 0.0025, 0.0, False, False),          # examples/point_mass_mpc.py
    "planner": (0.1, 0.005, 0.01, True, True),         # examples/point_mass_planner.py
    "final_free": (0.1, 0.005, 0.01, True, False),     # the planner's cost, final velocity free
    "fix_only": (0.05, 0.0025, 0.0, False, True),      # the MPC tick's cost, final velocity pinned
}
HORIZONS = (2, 3, 4, 5, 63, 64, 65)
KS = (1, 2, 3)
N_SLOTS = 4
MAX_EXTRA = 60
NO_CUT_CELLS = (("fix_only", 5),)  # cells of T >= 5 in which MAX_EXTRA further draws found no cut first step either


def cells():
    return [(v, T) for v in VARIANTS for T in HORIZONS if not (VARIANTS[v][4] and T < 3)]


def options(variant, T):
    dt, w_acc, w_vel, final_only, fix = VARIANTS[variant]
    return dict(T=T, dt=dt, w_acc=w_acc / T, w_vel=w_vel / T, track_final_only=final_only, fix_final_velocity=fix)


def case_id(variant, T, slot):
    return f"{variant}_T{T}_i{slot}"


def draw(rng, T, dt, seeded):
    """One instance in the style of the buffer-regrow test's parameters: a goal ramp from the start to (1, 1), the moving obstacle table; a moving start,
    and for `seeded` a velocity seed in x0's dY block (its Y block, which no solver reads, is noise)."""
    curr = np.array([-0.9, 0.4]) + rng.uniform(-0.3, 0.3, 2)
    dcurr = rng.uniform(-0.3, 0.3, 2)
    ob = np.array([[0.15 * np.sin(np.pi * (dt * t) - np.pi), 0.15 * np.cos(np.pi * (dt * t) - np.pi) + 0.15] for t in range(T)])  # (T, 2)
    ramp = np.arange(T) / (T - 1.0)
    goal = np.clip(curr[None, :] + (1 - curr[None, :]) * ramp[:, None], -1.5, 1.5)  # (T, 2)
    x0 = np.zeros(4 * T)
    if seeded:
        x0[: 2 * T] = rng.uniform(-1.0, 1.0, 2 * T)
        x0[2 * T :] = rng.uniform(-0.2, 0.2, 2 * T)
    return x0, np.concatenate([curr, dcurr, goal.reshape(-1), ob.reshape(-1)])


def split(T, x0, p):
    return p[0:2], p[2:4], p[4 : 4 + 2 * T].reshape(T, 2).T, p[4 + 2 * T :].reshape(T, 2).T, x0[2 * T :].reshape(T, 2).T


def port(opt, x0, p, max_iter):
    T = opt["T"]
    curr, dcurr, goal, obs, V0 = split(T, x0, p)
    return solve_pointmass_ipm(T, opt["dt"], opt["w_acc"], YLIM, VLIM, SAFE * SAFE, curr, dcurr, goal, obs, V0=V0, tol=TOL, max_iter=max_iter,
                               track_final_only=opt["track_final_only"], w_vel=opt["w_vel"], fix_final_velocity=opt["fix_final_velocity"])


def port_x(r):
    return np.concatenate([r["Y"].T.reshape(-1), r["V"].T.reshape(-1)])


def reference(opt, x0, p):
    T = opt["T"]
    curr, dcurr, goal, obs, V0 = split(T, x0, p)
    return pm_steps_mp(T, opt["dt"], opt["w_acc"], YLIM, VLIM, SAFE * SAFE, curr, dcurr, goal, obs, V0=V0, k_max=KS[-1], tol=TOL,
                       track_final_only=opt["track_final_only"], w_vel=opt["w_vel"], fix_final_velocity=opt["fix_final_velocity"])


def port_distance(opt, x0, p, ref):
    """(3, 5) distances of the port's max_iter = k answers from the mp ones, and whether every status agrees"""
    dist, same = np.zeros((len(KS), 5)), True
    for n, k in enumerate(KS):
        r = port(opt, x0, p, k)
        same = same and r["status"] == ref[k]["status"] and r["iters"] == k
        dist[n, 0] = np.abs(port_x(r) - ref[k]["x"]).max()
        dist[n, 1] = abs(r["f"] - ref[k]["f"])
        dist[n, 2:] = np.abs(np.array(r["kkt"]) - ref[k]["kkt"])
    return dist, same


def evaluate(opt, x0, p):
    """None when a rule rejects the instance, else its arrays"""
    ref = reference(opt, x0, p)
    if len(ref) != KS[-1] + 1 or any(r["status"] != 1 for r in ref):
        return None  # converged or declared infeasible within three steps
    steps = np.array([[float(ref[k]["ap"]), float(ref[k]["ad"])] for k in KS])
    for k in KS:
        am = min(ref[k]["ap"], ref[k]["ad"])
        if abs(am - 0.9) <= 1e-6 or abs(am - 0.5) <= 1e-6:
            return None
    dist, same = port_distance(opt, x0, p, ref)
    if not same:
        return None
    T = opt["T"]
    desc = np.array([T, opt["dt"], opt["w_acc"], opt["w_vel"], float(opt["track_final_only"]), float(opt["fix_final_velocity"]), YLIM, VLIM, SAFE, TOL])
    return {"desc": desc, "x0": x0, "p": p, "x": np.stack([ref[k]["x"] for k in KS]), "f": np.array([ref[k]["f"] for k in KS]),
            "kkt": np.stack([ref[k]["kkt"] for k in KS]), "dist": dist, "step": steps,
            "pinned": np.array([[float(ref[k]["dv_last"]), float(ref[k]["v_last"])] for k in KS])}


def make_cell(variant, T):
    """The four instances of a cell: (list of array dicts, draws, rejected, passed over)"""
    opt = options(variant, T)
    rng = np.random.default_rng(SEED + 1000 * list(VARIANTS).index(variant) + T)
    got, draws, rejected, passed = [], 0, 0, 0
    while len(got) < N_SLOTS:
        x0, p = draw(rng, T, opt["dt"], seeded=len(got) < 2)
        draws += 1
        e = evaluate(opt, x0, p)
        if e is None:
            rejected += 1
        else:
            got.append(e)
    if T >= 5 and not any(e["step"][0, 0] < 1.0 for e in got):
        for _ in range(MAX_EXTRA):
            x0, p = draw(rng, T, opt["dt"], seeded=False)
            draws += 1
            e = evaluate(opt, x0, p)
            if e is None:
                rejected += 1
            elif e["step"][0, 0] < 1.0:
                got[-1] = e
                break
            else:
                passed += 1
        else:
            assert (variant, T) in NO_CUT_CELLS, (variant, T)
    return got, draws, rejected, passed


def generate(which=None, verbose=True):
    arrays, draws, rejected, passed = {}, 0, 0, 0
    for variant, T in which or cells():
        got, d, r, s = make_cell(variant, T)
        draws, rejected, passed = draws + d, rejected + r, passed + s
        for slot, e in enumerate(got):
            for name, v in e.items():
                arrays[case_id(variant, T, slot) + "_" + name] = v
        if verbose:
            worst = np.max([e["dist"][:, 0].max() for e in got])
            cut = [bool(e["step"][0, 0] < 1.0) for e in got]
            print(f"{variant:10s} T {T:2d}: draws {d}, rejected {r}, passed over {s}, first step cut {cut}, port |x - x_mp| <= {worst:.2e}", flush=True)
    if verbose:
        print(f"draws {draws}, rejected by the rules {rejected} ({100.0 * rejected / draws:.1f} %), passed over for a cut first step {passed}")
    return arrays, draws, rejected


def main():
    arrays, draws, rejected = generate()
    assert 4 * rejected <= draws, "more than a quarter of the draws rejected: the distribution is wrong"
    if "--check" in sys.argv:
        have = np.load(FIXTURE)
        assert sorted(have.files) == sorted(arrays), "the fixture holds other cases"
        bad = [k for k in arrays if not (have[k].shape == arrays[k].shape and have[k].tobytes() == arrays[k].tobytes())]
        assert not bad, bad
        print("fixture reproduced bit for bit:", len(arrays), "arrays")
    else:
        np.savez_compressed(FIXTURE, **arrays)
        print("wrote", os.path.relpath(FIXTURE, ROOT), os.path.getsize(FIXTURE), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
