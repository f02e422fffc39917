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
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, d)
from gpu_ab_common import report, timed as _timed, write_times  # noqa: E402

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
    write_times(path, pts)


if __name__ == "__main__":
    if sys.argv[1] == "pin":
        pin(sys.argv[2])
    elif sys.argv[1] == "time":
        time_points(sys.argv[2])
    else:
        sys.exit(report(sys.argv[2:], KERNELS, "tools/gpu_qp_ab_dump.py", "qp_one_text_ab.json"))
