"""CPU: the build's source list and csrc/ agree -- a HIP source that is not listed would be
missing from the library (found at link or load time at best), a listed one that does not exist
fails the build."""
import os

from quantized_spectrum_cartography_amd import _build


def test_every_hip_source_is_listed_and_exists():
    on_disk = sorted(f for f in os.listdir(_build.CSRC) if f.endswith(".hip"))
    assert sorted(_build.SOURCES) == on_disk
    assert len(set(_build.SOURCES)) == len(_build.SOURCES)
    # the fused passes' files are all built with the passes' flags
    assert set(_build.PASS_SOURCES) <= set(_build.SOURCES)
    assert all(_build.FILE_FLAGS[s] == _build.PASS_FLAGS for s in _build.PASS_SOURCES)
