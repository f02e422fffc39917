"""Instances of the point-mass family's horizon-edge tests (test_gpu_pm_horizons.py) beyond the fixture of tools/make_pm_steps_golden.py: the full
solves of every (variant, horizon) cell, fillers for the batch-placement test, and the closed-loop starts.

Full solves compare iteration counts, which means something only away from the stopping threshold: FULL_SEEDS lists, per cell, eight candidate numbers
whose numpy-port run (tol 1e-8, max_iter 200) converges with max(stat, feas, compl) <= 0.5 tol at its last evaluation and >= 2 tol at the one before.
They were chosen on the CPU by walking the candidates 0, 1, 2, ... of each cell (select_full_seeds below); the GPU test asserts the margins again from
the port's own run."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_pm_steps_golden as gen  # noqa: E402

TOL, MAX_ITER = 1e-8, 200
N_FULL = 8
SEED = 20261021


def full_instance(variant, T, i):
    """Candidate i of a cell: (x0, p).  Variants that track every knot get the fixture's kind of instance (goal ramp, moving obstacle, moving start); the two
    that track the last knot only get the planner's: a start at rest, a constant goal across the obstacle, which stands at the origin -- the instance
    PointMassPlannerNLP states."""
    rng = np.random.default_rng(SEED + 100000 * list(gen.VARIANTS).index(variant) + 1000 * T + i)
    dt, final_only = gen.VARIANTS[variant][0], gen.VARIANTS[variant][3]
    if not final_only:
        x0, p = gen.draw(rng, T, dt, seeded=False)
        if i % 4 >= 2:
            # a goal ramp the mass can follow inside its velocity box: few rows active at the optimum.  (With the velocity rows active to the end the
            # complementarity shrinks by a factor just under 4 per step, and no run can lie a factor 2 off the tolerance on both sides.)
            vel = rng.uniform(-0.6, 0.6, 2)
            p[4 : 4 + 2 * T] = (p[None, 0:2] + (dt * np.arange(T))[:, None] * vel[None, :]).reshape(-1)
    else:
        init, goal = rng.uniform(-1.3, -0.5, 2), rng.uniform(0.5, 1.3, 2)
        x0, p = np.zeros(4 * T), np.concatenate([init, np.zeros(2), np.tile(goal, T), np.zeros(2 * T)])
    if i % 2:
        # a velocity seed that leaves the box here and there: slacks start off their rows, steps are cut, and the barrier parameter leaves the ladder
        # 0.1, 0.01, ... on which an unconstrained short horizon lands exactly on the tolerance
        x0[2 * T :] = rng.uniform(-1.2, 1.2, 2 * T)
    return x0, p


def margins(r):
    """(last, one before last) of max(stat, feas, compl) over the port's evaluations"""
    h = r["kkt_history"]
    return max(h[-1]), (max(h[-2]) if len(h) > 1 else np.inf)


def well_separated(r):
    last, before = margins(r)
    return r["status"] == 0 and last <= 0.5 * TOL and before >= 2.0 * TOL


def select_full_seeds(variant, T, n_max=4000):
    opt, out = gen.options(variant, T), []
    for i in range(n_max):
        x0, p = full_instance(variant, T, i)
        if well_separated(gen.port(opt, x0, p, MAX_ITER)):
            out.append(i)
            if len(out) == N_FULL:
                return out
    raise RuntimeError(f"{variant} T = {T}: only {len(out)} of {n_max} candidates qualify")


FULL_SEEDS = {
    ('mpc', 2): [3, 5, 7, 9, 11, 17, 21, 23],
    ('mpc', 3): [7, 11, 13, 15, 17, 21, 23, 27],
    ('mpc', 4): [19, 27, 35, 39, 51, 63, 75, 79],
    ('mpc', 5): [11, 15, 19, 23, 47, 59, 71, 83],
    ('mpc', 63): [1, 3, 7, 17, 18, 20, 21, 23],
    ('mpc', 64): [0, 1, 3, 5, 6, 7, 9, 11],
    ('mpc', 65): [1, 2, 7, 12, 23, 26, 27, 28],
    ('planner', 3): [3, 5, 9, 11, 15, 21, 25, 31],
    ('planner', 4): [1, 5, 7, 19, 21, 22, 28, 30],
    ('planner', 5): [2, 6, 13, 14, 15, 17, 18, 20],
    ('planner', 63): [0, 1, 2, 6, 9, 11, 13, 15],
    ('planner', 64): [10, 16, 23, 24, 27, 28, 30, 34],
    ('planner', 65): [0, 8, 10, 14, 17, 20, 22, 25],
    ('final_free', 2): [5, 11, 19, 21, 25, 29, 33, 39],
    ('final_free', 3): [3, 12, 15, 19, 21, 22, 23, 27],
    ('final_free', 4): [3, 14, 15, 17, 19, 23, 31, 35],
    ('final_free', 5): [5, 11, 13, 15, 21, 27, 29, 31],
    ('final_free', 63): [1, 4, 13, 15, 19, 26, 29, 30],
    ('final_free', 64): [0, 4, 10, 14, 19, 20, 30, 34],
    ('final_free', 65): [7, 13, 14, 16, 22, 26, 29, 35],
    ('fix_only', 3): [1, 3, 7, 9, 15, 17, 19, 29],
    ('fix_only', 4): [3, 7, 9, 13, 17, 29, 33, 35],
    ('fix_only', 5): [1, 4, 8, 13, 15, 16, 24, 25],
    ('fix_only', 63): [0, 1, 2, 5, 7, 11, 13, 15],
    ('fix_only', 64): [4, 10, 18, 19, 20, 22, 23, 30],
    ('fix_only', 65): [0, 1, 2, 3, 4, 5, 7, 10],
}


def filler(T, dt, n, seed):
    """n feasible instances unlike the fixture's (another stream), for the slots around the instances under test"""
    rng = np.random.default_rng(SEED + 7919 * seed + T)
    xs, ps = zip(*(gen.draw(rng, T, dt, seeded=bool(k % 2)) for k in range(n)))
    return np.stack(xs), np.stack(ps)


def obstacle_table(rows, dt, t0=2.0):
    return np.array([[0.15 * np.sin((t0 + dt * j) * np.pi - np.pi), 0.15 * np.cos((t0 + dt * j) * np.pi - np.pi) + 0.15] for j in range(rows)])


def rollout_starts(B):
    rng = np.random.default_rng(SEED + 31)
    return np.concatenate([np.array([-0.9, 0.4]) + rng.uniform(-0.2, 0.2, (B, 2)), rng.uniform(-0.2, 0.2, (B, 2))], axis=1)
