"""ops/build.py needs_build(): the library is stale when any source or any
header of csrc/ is newer. Runs on a temporary directory."""
import os

import pytest

from crawler_amd.ops import build as B


@pytest.fixture
def csrc(tmp_path, monkeypatch):
    """A csrc/ of empty sources and headers, all older than the library."""
    for name in B.SOURCES + ["common.h", "other.h"]:
        p = tmp_path / name
        p.write_text("")
        os.utime(p, (1000, 1000))
    out = tmp_path / "libcrawlhip.so"
    out.write_text("")
    os.utime(out, (2000, 2000))
    monkeypatch.setattr(B, "CSRC", str(tmp_path))
    monkeypatch.setattr(B, "OUT", str(out))
    return tmp_path


def test_fresh_library_needs_no_build(csrc):
    assert not B.needs_build()


def test_missing_library_needs_build(csrc):
    os.remove(B.OUT)
    assert B.needs_build()


@pytest.mark.parametrize("name", ["common.h", "other.h", B.SOURCES[0]])
def test_newer_header_or_source_needs_build(csrc, name):
    """Every *.h counts, listed anywhere or not."""
    os.utime(csrc / name, (3000, 3000))
    assert B.needs_build()
