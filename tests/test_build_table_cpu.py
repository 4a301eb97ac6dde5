"""The build table of srgd_amd/build.py (one row per library) against the built libraries and their Python bindings, and the one
copy of Pillow's tables (srgd_amd/csrc/pillow_coeffs.hpp) seen from outside: the x4 vectors that three libraries export are rows of
the resize library's general table.  No GPU: every call here is host-only."""
import fnmatch
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from srgd_amd import _lib  # noqa: E402
from srgd_amd import backproject as BP  # noqa: E402
from srgd_amd import build as B  # noqa: E402
from srgd_amd import consistency as CS  # noqa: E402
from srgd_amd import guidance as GD  # noqa: E402
from srgd_amd import resize as RZ  # noqa: E402
from tests.lib_exports import exports  # noqa: E402


def test_every_row_of_the_build_table_is_a_built_library_with_the_exports_of_its_binding():
    names = [name for name, _, _, _ in B.LIBRARIES]
    assert names[0] == "hip" and len(names) == len(set(names)) == 11 and B.LIBRARIES[0][1:3] == (B.LIB, B.SOURCES)
    bindings = {name: _lib if name == "hip" else importlib.import_module("srgd_amd." + name) for name in names}
    for name, lib, sources, pattern in B.LIBRARIES:
        mod = bindings[name]
        assert lib == mod.LIB_PATH and os.path.exists(lib), "build the library first (python -m srgd_amd.build)"
        assert exports(lib) == set(mod.PROTOTYPES), name
        assert all(fnmatch.fnmatchcase(n, pattern) for n in mod.PROTOTYPES), name
        if name != "hip":           # the engine's pattern is the prefix of the whole project; an extension's pattern is its own
            for other in names:
                if other != name:
                    assert not any(fnmatch.fnmatchcase(n, pattern) for n in bindings[other].PROTOTYPES), (name, other)
    listed = [src for _, _, sources, _ in B.LIBRARIES for src in sources]
    on_disk = sorted(f for f in os.listdir(B.CSRC) if f.endswith(".hip"))
    assert sorted(listed) == on_disk and len(listed) == len(set(listed))          # every source in exactly one row
    assert set(B.EXTRA_FLAGS) <= set(listed)


def _on_frame(first, taps, start, n):
    """``taps`` (the window from input ``first``) laid on the frame [start, start + n): zeros elsewhere."""
    out = [0] * n
    for t, k in enumerate(taps):
        assert 0 <= first + t - start < n or k == 0
        if k != 0:
            out[first + t - start] = k
    return out


def test_the_x4_vectors_of_three_libraries_are_rows_of_the_resize_table():
    unit = 2.0 ** 22
    g_down, g_up = GD.coeffs()
    # reduction 256 -> 64: rows 0, 1, 10, 62, 63, frame [4i - 6, 4i + 10)
    bounds, kk = RZ.coeffs(256, 64, "bicubic")
    assert kk.shape == (64, 17)
    for v, i in enumerate((0, 1, 10, 62, 63)):
        first, count = (int(b) for b in bounds[i])
        assert count <= 16 and not kk[i, count:].any()
        assert CS.coeffs()[v] == kk[i, :16].tolist(), i
        assert [k * unit for k in g_down[v]] == _on_frame(first, kk[i, :count].tolist(), 4 * i - 6, 16), i
    # enlargement 64 -> 256: outputs 0 .. 9 and 250 .. 255, frame [floor((j - 6) / 4), + 4)
    bounds, kk = RZ.coeffs(64, 256, "bicubic")
    assert kk.shape == (256, 5)
    for v, j in enumerate(list(range(10)) + list(range(250, 256))):
        first, count = (int(b) for b in bounds[j])
        assert count <= 4 and not kk[j, count:].any()
        assert BP.coeffs()[v] == kk[j, :4].tolist(), j
        assert [k * unit for k in g_up[v]] == _on_frame(first, kk[j, :count].tolist(), (j - 6) // 4, 4), j
    assert np.abs(kk).max() < 2 ** 23                                              # so the factor 2^-22 is exact in fp32
