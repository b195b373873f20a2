"""The ctypes signature table of ops/gpu.py against the ``extern "C"``
definitions in ops/csrc/*.hip, read as text: the same names, the same
argument counts. Nothing is loaded or launched."""
import glob
import os
import re

from crawler_amd.ops import gpu

CSRC = os.path.join(os.path.dirname(gpu.__file__), "csrc")


def _c_entry_points():
    """{name: parameter count} of every ``int crawl_*(...)`` definition
    inside an ``extern "C"`` block."""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        text = open(path).read()
        start = text.find('extern "C" {')
        if start < 0:
            continue
        for m in re.finditer(r"^int (crawl_\w+)\(([^)]*)\)", text[start:],
                             re.M):
            name, params = m.group(1), m.group(2).strip()
            assert name not in found, f"{name} defined twice"
            found[name] = params.count(",") + 1 if params else 0
    return found


def test_table_names_equal_the_c_entry_points():
    assert set(gpu._SIGNATURES) == set(_c_entry_points())


def test_table_argument_counts_equal_the_c_definitions():
    c = _c_entry_points()
    assert c, "no entry point found"
    got = {name: len(args) for name, args in gpu._SIGNATURES.items()}
    assert got == {name: c.get(name) for name in got}
