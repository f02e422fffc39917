"""Every launch path of the orientation-locked figure-eight family at the horizon edges, on 4 ... 8 joints (tests/locked_step_cases.py), selected per
solve with oh_set_option and confirmed after the solve with oh_get_flag / oh_get_timing:

  path       options                                                         kernels                                  confirmed by
  tail       specialize=0                                                    k_tail<N>                                tail_iterations > 0, no batched iteration
  tail_spec  specialize=1 + oh_specialize                                    the tail compiled for the chain          ... and flag "specialized" = 1
  zc         specialize=0, tail_threshold=0, compaction=0                    k_retract + k_evalb_zc + k_step_zc       flag "fuse_couple" = 1, tail_iterations = 0
  zc_spec    as zc, specialize=1 + oh_specialize                             the same, compiled for the chain         ... and flag "specialized" = 1
  couple     as zc, fuse_couple=0                                            k_evalb / k_couple / k_step              flag "fuse_couple" = 0, tail_iterations = 0

  vel variant (joint-velocity rows at +-0.06 rad/s, the port's default curvature throughout):
  tail       specialize=0 (tail_vel=1)                                       k_tail_vel<N>                            tail_iterations > 0, no batched iteration
  tail_spec  specialize=1 + oh_specialize                                    k_tail_vel compiled for the chain        ... and flag "specialized" = 1
  lg_split   tail_vel=0, compaction=0, lg_split=1                            k_retract + k_evalb_lg / k_couple_vel / k_step_lg   options read back, tail_iterations = 0
  lg_fused   tail_vel=0, compaction=0, lg_split=0                            k_eval_lg / k_couple_vel / k_step_lg     options read back, tail_iterations = 0
  (flag "fuse_couple" = 0 on all four: handles with inequality rows never fold the coupling; with tail_vel = 0 nothing compiled for the chain is used, so
  there is no specialised batched path to select.)  Full solve: |dq| <= 0.06 + 1e-8, multipliers >= 0, the port's and between paths to 1e-3 max(1, |lam|)
  (the rules of test_gpu_velocity_limits.py at tol 1e-6).

Documented fall-backs, stated in expected(): beyond 64 free knots (T - 2 > 64, oh_api.hip:locked_loop) the tail paths run the batched launches of zc /
zc_spec.  A handle keeps the kernels compiled for its chain once they are loaded, so the specialised paths have a handle of their own; the
three-kernel path is run on the generic handle only (the run-time module is built around the folded coupling).

Per solve, at every cap: the copies of an instance in the batch of 67 are bit-identical in x, f, kkt, iters, status and multipliers; q_0 = q_1 = qc bit
for bit; a(x) to 1e-12.  The graded caps of a curvature are k, k + 1, k + 2 with k the first cap by which every instance has accepted a step
(locked_step_cases.FIRST_CAP: 1 on most cases; 7 on four and five joints, where lm_accept refuses every earlier trial and a solve returns its seed):
  max_iter = k      where k = 1 (Gauss-Newton and exact curvature): the returned knots against the 50-digit Newton step of the first system taken
                    through the port's retraction, within bound(case, 0) on every instance and knot; where k > 1: against the numpy port at that cap;
                    the retracted seed itself coming back is refused at every graded cap; step and rejection counts the port's;
  k + 1, k + 2      the returned knots are the numpy port's at the same cap within bound(case, 1 | 2); step and rejection counts equal;
  full solve        (hybrid, tol 1e-6) status 0, f the port's to 1e-9 relative, steps within max(2, 5 %), f between any two paths to 1e-9 relative,
                    orientation rows of the returned knots <= 1e-9 through OracleRobot.quaternion_batch.
The bounds are measured on the CPU (locked_step_cases.PORT_STEP_ERR, SENS), never chosen; the rules are locked_step_cases.grade, which the compiled
host port passes at every plain 7 and 6 joint horizon without a GPU.  Where k > 1 beyond 65 free knots (kuka7-plain-nK254 under Gauss-Newton, k = 2) no
graded cap is compared with mp through the retraction: the reference is the port, whose first graded system is certified in mp in the reduced form.

Measured on the MI355X (2026-10-21), largest |Q - Q_ref| / bound over the graded caps and all 28 cases: tail 0.34, tail_spec 0.33, zc 0.34, zc_spec 0.33,
couple 0.35 -- each at kuka7-plain-nK129, cap 2, Gauss-Newton (k_step_zc / k_step: beyond 64 free knots the tail paths are the batched kernels).  On four
and five joints, graded at caps 7, 8, 9: tail 0.21, tail_spec 0.20, zc 0.24, zc_spec 0.20, couple 0.24 (kuka5-plain-nK3, cap 7, exact curvature, for
k_tail<5>, k_step_zc<5> and k_step<5>).

With velocity rows (9 cases): tail 0.17 (k_tail_vel, kuka7-vel-nK2, cap 1), tail_spec 0.10 (kuka7-vel-nK65, cap 3: batched launches with the compiled
retraction), lg_split 0.09 (kuka7-vel-nK64, cap 2), lg_fused 0.17 (kuka7-vel-nK2, cap 1).

Found by this test: under exact curvature a seed whose first sweep does not factorise is deferred by k_step_zc and evaluated again; k_defer_copy put
"the older Lagrangian gradient" of that seed where the evaluation reads it, but a seed has none (it was evaluated fresh, lam = 0) and the other slot holds
what the handle's previous solve left behind: the second batched solve on a handle returned knots 3e-3 ... 0.3 rad off (kuka6 / kuka7, 65 free knots,
path zc after the tail path's fall-back).  k_defer_copy and k_sweep_lists now write zeros for an instance that has counted no step."""
import os
import re

import numpy as np
import pytest

import locked_step_cases as lc
from conftest import ROOT

pytestmark = pytest.mark.gpu
BATCHED = dict(tail_threshold=0, compaction=0)
DEFAULTS = dict(tail_threshold=16384, compaction=1, fuse_couple=1, tail_vel=1, lg_split=1)  # csrc/oh_handle.h: Sched
# path -> (handle, options on top of DEFAULTS)
PATHS = {
    "tail": ("generic", {}),
    "tail_spec": ("spec", {}),
    "zc": ("generic", BATCHED),
    "zc_spec": ("spec", BATCHED),
    "couple": ("generic", dict(BATCHED, fuse_couple=0)),
}
# vel: the persistent kernel k_tail_vel (generic, and out of the module compiled for the chain), and the batched launches k_retract + k_evalb_lg (lg_split = 1)
# or the fused k_eval_lg (lg_split = 0), each with k_couple_vel and k_step_lg.  The batched launches with tail_vel = 0 use nothing compiled for the chain
# (oh_api.hip: spec_tail_vel_applies asks for tail_vel), so there is no specialised batched path to select; beyond 64 free knots tail_spec runs the batched
# launches with the retraction compiled for the chain.
PATHS_VEL = {
    "tail": ("generic", {}),
    "tail_spec": ("spec", {}),
    "lg_split": ("generic", dict(BATCHED, tail_vel=0, lg_split=1)),
    "lg_fused": ("generic", dict(BATCHED, tail_vel=0, lg_split=0)),
}
TAIL_MAX_NK = 64  # T - P.t0 <= 64 (oh_api.hip: locked_loop)


def expected(case, path):
    """What a path must report after the solve, documented fall-backs included -> dict(tail, fuse_couple, specialized)."""
    handle, opts = paths_of(case)[path]
    tail = path.startswith("tail") and case[2] <= TAIL_MAX_NK  # beyond: the batched launches (plain: with the folded coupling)
    if case[1] == "vel":  # (handles with inequality rows never fold the coupling: k_couple_vel)
        return dict(tail=tail, fuse_couple=0, specialized=int(handle == "spec"), lg_split=int(opts.get("lg_split", 1)), tail_vel=int(opts.get("tail_vel", 1)))
    return dict(tail=tail, fuse_couple=int(opts.get("fuse_couple", 1)), specialized=int(handle == "spec"))


def paths_of(case):
    return PATHS_VEL if case[1] == "vel" else PATHS


@pytest.fixture(scope="module")
def robots_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("locked_step_robots")


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_every_path_against_mp_and_the_port(hip_lib, robots_dir, case):
    c = lc.Case(robots_dir, case)
    refs = c.references()
    x0, p = c.batch()
    idx = np.arange(lc.BATCH) % lc.N_INST
    tag = lc.case_id(case)
    worst = {}
    for cap, curvature in [(k, h) for h in c.curvatures for k in c.caps(h)] + [("full", "hybrid")]:
        handles = {}
        for name in ("generic", "spec"):
            be = c.backend(c.max_iter_full if cap == "full" else cap, curvature)
            be.set_options(specialize=1 if name == "spec" else 0)
            if name == "spec":
                assert be.specialize()["loaded"], (tag, "oh_specialize")
            handles[name] = be
        f_paths, lam_paths = {}, {}
        for path, (handle, opts) in paths_of(case).items():
            be = handles[handle]
            be.set_options(dict(DEFAULTS, **opts))
            res = be.solve(x0, p)
            want, tm = expected(case, path), be.timing()
            got = dict(tail=tm["tail_iterations"] > 0, fuse_couple=be.flag("fuse_couple"), specialized=be.flag("specialized"))
            if c.variant == "vel":
                got.update(lg_split=int(be.get_option("lg_split")), tail_vel=int(be.get_option("tail_vel")))
            assert got == want and (tm["iterations_launched"] == 0) == want["tail"], (tag, cap, curvature, path, got, want, tm)
            lam = be.multipliers(lc.BATCH)
            for b in range(lc.N_INST, lc.BATCH):  # the copies of an instance
                i = b % lc.N_INST
                assert (np.array_equal(res.x[b], res.x[i]) and res.f[b] == res.f[i] and np.array_equal(res.kkt[b], res.kkt[i]) and res.iters[b] == res.iters[i]
                        and res.status[b] == res.status[i] and np.array_equal(lam[b], lam[i])), (tag, cap, curvature, path, b)
            for b in range(lc.BATCH):
                assert c.linear_rows(res.x[b], c.qc[idx[b]]) <= 1e-12, (tag, cap, curvature, path, b)
            X = res.x[:, : c.n * c.T].reshape(lc.BATCH, c.T, c.n)
            w = lc.grade(c, refs, cap, curvature, X, res.f, res.iters, res.status, (tag, cap, curvature, path))
            steps = res.iters[: lc.N_INST].tolist()
            graded = c.full_instances if cap == "full" else range(lc.N_INST)
            pr = {i: refs["port"][(cap, curvature, i)] for i in graded}
            if cap == "full":
                f_paths[path] = res.f[list(graded)].copy()
                if c.variant == "vel":  # rows to 1e-8; multipliers by the rules of test_gpu_velocity_limits.py (>= 0; the port's and between paths: 1e-3 at tol 1e-6)
                    dq = np.abs(res.x[np.isin(idx, list(graded)), c.n * c.T :]).max()  # (the instances whose full solve is graded: Case.full_instances)
                    assert dq <= lc.VMAX + 1e-8, (tag, path, dq)
                    assert lam.shape == (lc.BATCH, c.T, 2 * c.n) and lam.min() >= 0.0 and lam.max() > 0.0, (tag, path)
                    lam_paths[path] = lam[list(graded)]
                    for i in graded:
                        lp = np.zeros((c.T, 2 * c.n))
                        lp[: c.T - 1] = pr[i]["lam_v"]  # the velocity rows of knot t are those of dq_t
                        assert np.abs(lam[i] - lp).max() <= 1e-3 * max(1.0, lp.max()), (tag, path, i, np.abs(lam[i] - lp).max(), lp.max())
                print("%s full %-9s status %s steps %s port %s" % (tag, path, res.status[: lc.N_INST].tolist(), steps, [pr[i]["iters"] for i in graded]))
            else:
                worst[path] = max(worst.get(path, (0.0,)), (w, cap, curvature))
                pos = c.caps(curvature).index(cap)
                rej, rej_port = tm["rejected_steps"], sum(pr[i]["rejected"] for i in idx)
                print("%s cap %d %-12s %-9s |Q - Q_ref| / bound %.3f (bound %.2e) steps %s port %s rejected %d port %d"
                      % (tag, cap, curvature, path, w, lc.bound(case, pos, refs["step_inf"]), steps, [pr[i]["iters"] for i in graded], rej, rej_port))
                assert rej == rej_port, (tag, cap, curvature, path, rej, rej_port)
        for a in f_paths:
            for b in f_paths:
                assert np.abs(f_paths[a] - f_paths[b]).max() <= 1e-9 * max(1.0, np.abs(f_paths[a]).max()), (tag, a, b)
        for a in lam_paths:
            for b in lam_paths:
                assert np.abs(lam_paths[a] - lam_paths[b]).max() <= 1e-3 * max(1.0, np.abs(lam_paths[a]).max()), (tag, a, b)
        for be in handles.values():
            be.close()
    print("%s: largest |Q - Q_ref| / bound per path (ratio, cap, curvature) %s" % (tag, worst))


def test_every_chain_length_and_every_path_has_its_cases():
    """The chain lengths the locked family is instantiated for, read off oh_kernels.hip's dispatch: each has a case on a tail path and on a batched
    path; every path of the table runs at an odd nK, an even nK and nK < 2 (fewer knots than the prefetch ring of step_instance_zc)."""
    src = open(os.path.join(ROOT, "optas_amd", "csrc", "oh_api.hip")).read()
    assert re.search(r"h->desc\.T - P\.t0 <= 64", src)  # TAIL_MAX_NK
    units = open(os.path.join(ROOT, "optas_amd", "csrc", "oh_figure8_units.h")).read()
    assert re.search(r"#define OH_STEP_ZC_PF 2\b", units)
    kern = open(os.path.join(ROOT, "optas_amd", "csrc", "oh_kernels.hip")).read()
    macro = kern[kern.index("#define OH_DISPATCH_N(n, call)") :]
    macro = macro[: macro.index("default:")]
    lengths = {int(v) for v in re.findall(r"case (\d+):", macro)}
    assert lengths == {4, 5, 6, 7, 8}, lengths
    ran = {}
    for case in lc.CASES:
        for path in paths_of(case):
            e = expected(case, path)
            if case[1] == "plain":
                ran.setdefault((lc.NDOF[case[0]], "tail" if e["tail"] else "batched"), set()).add(path)
            ran.setdefault((case[1], path), set()).add(case[2])
            ran.setdefault((case[1], lc.NDOF[case[0]], "tail" if e["tail"] else "batched"), set()).add(path)
    for n in lengths:
        assert ran.get((n, "tail")) and ran.get((n, "batched")), n
    for variant, paths in (("plain", PATHS), ("vel", PATHS_VEL)):
        for path in paths:
            nks = ran[(variant, path)] if not path.startswith("tail") else {k for k in ran[(variant, path)] if k <= TAIL_MAX_NK}
            assert any(k % 2 for k in nks if k >= 2) and any(k % 2 == 0 for k in nks) and any(k < 2 for k in nks), (variant, path, sorted(nks))
    for n in (6, 7):  # the velocity rows: k_tail_vel and the batched launches on both chains of the table
        assert ran.get(("vel", n, "tail")) and {"lg_split", "lg_fused"} <= ran.get(("vel", n, "batched"), set()), n
