"""The layout lists of optas_amd/csrc/oh_carve.h (device pools, staging of oh_solve) against tests/golden/pool_layouts.json, which was recorded
once from the hand-written carving statements these lists replaced: every pointer's byte offset and every total.  tests/pool_layout.hip is a
host program (no GPU call), built with the recipe of oracle/cpu_port; it also checks that measuring and carving agree and that no two arrays overlap."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_pool_and_stage_layouts_match_the_recorded_offsets(tmp_path):
    exe = str(tmp_path / "pool_layout")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "optas_amd", "csrc"), "-o", exe, os.path.join(HERE, "pool_layout.hip")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got = json.loads(run.stdout)
    with open(os.path.join(HERE, "golden", "pool_layouts.json")) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for case in want:
        assert got[case] == want[case], case
