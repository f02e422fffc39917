"""optas_amd/build.py:needs_build() sees an edit to any source or header of csrc/, oh_carve.h (the pool layouts) included: the dependency set is
read off the directory, not kept by hand."""
import os

from optas_amd import build

CARVE = os.path.join(build.CSRC, "oh_carve.h")


def test_an_edit_to_the_pool_layouts_asks_for_a_build(tmp_path, monkeypatch):
    out = tmp_path / "liboptas_hip.so"
    out.write_bytes(b"")
    newest = max(os.path.getmtime(d) for d in build.dependencies())
    os.utime(out, (newest + 1, newest + 1))  # a library built after the last edit
    monkeypatch.setattr(build, "OUT", str(out))
    assert CARVE in build.dependencies()
    assert not build.needs_build()
    st = os.stat(CARVE)
    try:
        os.utime(CARVE, (newest + 2, newest + 2))  # touch
        assert build.needs_build()
    finally:
        os.utime(CARVE, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert not build.needs_build()
