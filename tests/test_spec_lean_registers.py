"""The lean carried compaction (compact_fused = 2) predicates the moving retraction's gradient copy per lane and drops its store of the accepted knot
(eval_unit<.., MOVE>, D.lean); the evaluation behind it is the same oh_spec_evalb_zc.  Conditions on the code object compiled for the chain, not
measurements: both kernels are built for two waves per SIMD (__launch_bounds__(256, 2): at most 256 registers per lane) and must not touch scratch."""
import glob
import os

import optas_amd
from optas_amd import _lib
from test_spec_retract_move import LINK, READELF, _kernel_notes


def test_moving_retraction_and_evaluation_keep_two_waves_without_scratch(tmp_path, monkeypatch):
    assert os.path.exists(READELF), "llvm-readelf comes with the ROCm toolchain the library is built with"
    monkeypatch.setenv("OPTAS_HIP_CACHE", str(tmp_path / "cache"))
    chain = optas_amd.RobotModel.builtin("kuka_lwr").kinematic_chain(LINK)
    _lib.specialize_compile(chain)
    notes = {}
    for path in glob.glob(str(tmp_path / "cache" / "spec_*.hsaco")):
        notes.update(_kernel_notes(path))
    for name in ("oh_spec_retract_move", "oh_spec_evalb_zc"):
        assert name in notes, sorted(notes)
        k = notes[name]
        print(name, k)
        assert k["vgpr_count"] <= 256, name
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, name
