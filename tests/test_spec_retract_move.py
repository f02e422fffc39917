"""The retraction that lays the knots of a carried compaction down at their new index (oh_spec_retract_move, compact_fused) exists only in the
kernels compiled for a chain, because the generic k_retract spills with it.  These are conditions on its code object, not measurements: a kernel
that spills, or that no longer fits two waves per SIMD, must not reach the GPU as the default path."""
import glob
import os
import re
import subprocess

import pytest

import optas_amd
from optas_amd import _lib

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
LINK = "end_effector_ball"


def _kernel_notes(path):
    """{kernel name: {metadata key: int}} of one code object (AMDGPU metadata note)."""
    txt = subprocess.run([READELF, "--notes", path], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in txt.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        vals = {"agpr_count": int(blk.split()[0])}
        for key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            m = re.search(r"\.%s:\s+(\d+)" % key, blk)
            assert m, (name.group(1), key)
            vals[key] = int(m.group(1))
        out[name.group(1)] = vals
    return out


def _waves_per_simd(vgprs):
    """gfx950: 512 registers per lane and SIMD, handed out in blocks of 8, at most 8 waves."""
    return min(8, 512 // (8 * ((vgprs + 7) // 8)))


def test_moving_retraction_neither_spills_nor_loses_a_wave(tmp_path, monkeypatch):
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not installed")
    monkeypatch.setenv("OPTAS_HIP_CACHE", str(tmp_path / "cache"))
    chain = optas_amd.RobotModel.builtin("kuka_lwr").kinematic_chain(LINK)
    _lib.specialize_compile(chain)
    notes = {}
    for path in glob.glob(str(tmp_path / "cache" / "spec_*.hsaco")):
        notes.update(_kernel_notes(path))
    assert "oh_spec_retract_move" in notes and "oh_spec_retract" in notes, sorted(notes)
    move, plain = notes["oh_spec_retract_move"], notes["oh_spec_retract"]
    print("oh_spec_retract_move", move)
    print("oh_spec_retract     ", plain)
    assert move["private_segment_fixed_size"] == 0 and move["vgpr_spill_count"] == 0
    assert move["vgpr_count"] <= 256  # the cap for two waves per SIMD (__launch_bounds__(256, 2))
    # the plain retraction, which serves the launches without a compaction, is no worse off than the moving one: no more scratch, no more spills,
    # and no fewer waves per SIMD.  (Its raw register count is not compared: the compiler gives the moving kernel 224 registers and the plain one,
    # before and after the flag was added, 226 -- both two waves of the 512-register file, which is allocated in blocks of 8.)
    for key in ("private_segment_fixed_size", "vgpr_spill_count"):
        assert plain[key] <= move[key], key
    assert plain["vgpr_count"] <= 256 and _waves_per_simd(plain["vgpr_count"]) >= _waves_per_simd(move["vgpr_count"]) >= 2
