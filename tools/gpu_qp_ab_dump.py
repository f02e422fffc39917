#!/usr/bin/env python
"""Bits and device times of the dense QP family for comparing two builds of the library (OPTAS_HIP_LIBRARY selects the other one) after a change
that must alter neither.  One process per library and call, each under a time limit of its own, the chain stopped at the first failure:

  pin OUT.npz      every output array of tests/test_gpu_qp_bits.py:qp_outputs on its qp_cases, after check_pinned: what that test compares against
                   (tests/golden/qp_parent_bits.npz, written from the parent's library).
  time OUT.json    7 device times (ms, the handle's event timer, after 2 warm-up solves) per point.  Solve only: the planted class vertex_eq (the
                   velocity-IK shape) at B = 1, 64, 4096, 65 536, base at 4096 with qp_mode -1 / 0 / 1 / 2, max at 64 and 4096, base at 256 with
                   qp_mode 3.  Assembly and solve: qp_planted.parametric_qp through HIPSolver at B = 1, 64, 4096.  Each point with its launch path,
                   iteration counts and converged share.
  report FILES...  per point, the new library's median against the parent's maximum (the json files of `time`, told apart by their "library"
                   entry; several per library are pooled); the iteration counts of the two must be equal.  Files named *.remarks are the compiler's
                   -Rpass-analysis=kernel-resource-usage output for oh_qp.hip and oh_qp_block.hip (hipcc --offload-arch=gfx950 -O3
                   --cuda-device-only -c, standard error kept), the parent's with "parent" in the file name.  -> profiles/qp_one_text_ab.json with
                   both sets of times and both resource tables.  Exit status 1 if a point is slower or a kernel gained scratch.
"""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for d in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
REPEATS, WARMUP = 7, 2
SOLVE_POINTS = [("vertex_eq", B, -1) for B in (1, 64, 4096, 65536)] + [("base", 4096, mode) for mode in (-1, 0, 1, 2)] + [("max", 64, -1), ("max", 4096, -1), ("base", 256, 3)]
ASSEMBLY_POINTS = (1, 64, 4096)
KERNELS = {"k_qp_solveILi0E": "k_qp_solve<0>", "k_qp_solveILi1E": "k_qp_solve<1>", "k_qp_solveILi2E": "k_qp_solve<2>", "k_qp_solve_waveE": "k_qp_solve_wave",
           "k_qp_solve_blockE": "k_qp_solve_block", "k_qp_assembleE": "k_qp_assemble", "k_qp_assemble_blockE": "k_qp_assemble_block"}  # in the mangled name


def pin(path):
    import test_gpu_qp_bits as qb

    cases = qb.qp_cases()
    out = qb.qp_outputs(cases)
    qb.check_pinned(out, cases)
    np.savez_compressed(path, **out)
    print("pinned", len(out), "arrays to", path, os.path.getsize(path), "bytes")


def _timed(solve, ms):
    for _ in range(WARMUP):
        solve()
    times = []
    for _ in range(REPEATS):
        res = solve()
        times.append(float(ms()))
    return {"ms": times, "iters_sum": int(res.iters.sum()), "iters_max": int(res.iters.max()), "converged": float((res.status == 0).mean())}


def time_points(path):
    import qp_planted as Q
    from conftest import SEED
    from optas_amd.backend import QPBackend
    from optas_amd.solver import HIPSolver

    pts = {}
    for name, B, mode in SOLVE_POINTS:
        a = Q.CLASSES[name]
        n, m, me = a["n"], a["m"], a["me"]
        one = np.stack([Q.pack(qp) for qp in Q.planted_instances(name)])
        rows, x0 = np.ascontiguousarray(one[np.arange(B) % Q.N_INST]), np.zeros((B, n))
        be = QPBackend(n, m, me)
        be.set_option("qp_mode", mode)
        key = "%s_b%d_mode%d" % (name, B, mode)
        pts[key] = _timed(lambda: be.solve(x0, rows), be.solve_ms)
        pts[key]["path"] = ["block", 256] if mode == 3 else list(Q.launch_path(n, m, me, B, mode))
        be.close()
        print(key, pts[key], flush=True)
    o = Q.parametric_qp()
    dev = HIPSolver(o).setup("hip_sqp")
    assert dev.backend.be.tape is not None
    for B in ASSEMBLY_POINTS:
        pv, x0 = np.random.default_rng(SEED + 15).uniform(0.5, 1.5, (B, 4)), np.zeros((B, o.nx))
        key = "parametric_assembly_b%d" % B
        pts[key] = _timed(lambda: dev.solve_batch_arrays(x0, pv), dev.backend.be.solve_ms)
        pts[key]["path"] = ["assemble_block" if B <= 64 else "assemble"] + list(Q.launch_path(dev.backend.be.n, dev.backend.be.m, dev.backend.be.me, B))
        print(key, pts[key], flush=True)
    dev.backend.close()
    with open(path, "w") as f:
        json.dump({"library": os.environ.get("OPTAS_HIP_LIBRARY", "in-tree"), "points": pts}, f, indent=1)


def resource_usage(path):
    """{kernel: {vgprs, sgprs, scratch_bytes, occupancy}} of the QP kernels in one file of resource-usage remarks"""
    table, name = {}, None
    fields = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes", "Occupancy [waves/SIMD]": "occupancy"}
    for line in open(path):
        hit = re.search(r"remark: +([A-Za-z \[\]/]+): (\S+) \[-Rpass-analysis", line)
        if not hit:
            continue
        if hit.group(1) == "Function Name":
            name = next((pretty for mangled, pretty in KERNELS.items() if mangled in hit.group(2)), None)
        elif name and hit.group(1) in fields:
            table.setdefault(name, {})[fields[hit.group(1)]] = int(hit.group(2))
    return table


def report(files):
    runs, usage = {"parent": {}, "new": {}}, {"parent": {}, "new": {}}
    for path in files:
        if path.endswith(".remarks"):
            usage["parent" if "parent" in os.path.basename(path) else "new"].update(resource_usage(path))
            continue
        rec = json.load(open(path))
        side = "new" if rec["library"] == "in-tree" else "parent"
        for k, v in rec["points"].items():
            e = runs[side].setdefault(k, dict(v, ms=[]))
            assert (e["iters_sum"], e["iters_max"], e["path"]) == (v["iters_sum"], v["iters_max"], v["path"]), (path, k)
            e["ms"].extend(v["ms"])
    points = {}
    for k, nw in runs["new"].items():
        pa = runs["parent"][k]
        assert (pa["iters_sum"], pa["iters_max"]) == (nw["iters_sum"], nw["iters_max"]), (k, pa, nw)  # the same iteration on both sides
        points[k] = {"path": nw["path"], "parent_ms": pa["ms"], "new_ms": nw["ms"], "parent_max_ms": max(pa["ms"]), "new_median_ms": float(np.median(nw["ms"])),
                     "holds": bool(np.median(nw["ms"]) <= max(pa["ms"])), "iters_sum": nw["iters_sum"], "iters_max": nw["iters_max"],
                     "converged": (pa["converged"], nw["converged"])}
    scratch_gained = [k for k, v in usage["new"].items() if v["scratch_bytes"] > usage["parent"][k]["scratch_bytes"]]
    res = {"source": "tools/gpu_qp_ab_dump.py", "timer": "oh_get_timing out[4] (HIP events around the solve's launches); per process %d solves after %d warm-ups" % (REPEATS, WARMUP),
           "speed_criterion": "per point, the new library's median over its runs <= the parent's maximum over its runs; processes of the two libraries alternated",
           "points": points, "resource_usage_new": usage["new"], "resource_usage_parent": usage["parent"], "scratch_gained": scratch_gained}
    with open(os.path.join(ROOT, "profiles", "qp_one_text_ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["parent_max_ms"], v["new_median_ms"], v["holds"]) for k, v in points.items()}, indent=1))
    return 0 if all(v["holds"] for v in points.values()) and not scratch_gained else 1


if __name__ == "__main__":
    if sys.argv[1] == "pin":
        pin(sys.argv[2])
    elif sys.argv[1] == "time":
        time_points(sys.argv[2])
    else:
        sys.exit(report(sys.argv[2:]))
