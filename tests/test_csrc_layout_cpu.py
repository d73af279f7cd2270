"""The build's file lists (prodsearch_amd/build.py) against what lies in csrc/: a source missing from SOURCES is never
compiled, a header missing from HEADERS leaves stale objects behind after an edit.  No compiler, no device."""
import glob
import os

from prodsearch_amd import build


def _on_disk(pattern):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(build.CSRC, pattern)))


def test_every_hip_source_is_built():
    assert sorted(build.SOURCES) == _on_disk('*.hip')
    assert len(set(build.SOURCES)) == len(build.SOURCES)


def test_every_header_is_a_dependency():
    assert all(os.path.isfile(os.path.join(build.CSRC, h)) for h in build.HEADERS)
    in_csrc = [h for h in build.HEADERS if os.path.dirname(h) == '']
    assert sorted(in_csrc) == _on_disk('*.h')
    assert len(set(build.HEADERS)) == len(build.HEADERS)
