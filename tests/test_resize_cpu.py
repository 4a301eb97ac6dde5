"""srgd_amd.resize without a GPU: the numpy restatement of tests/resize_cases.py against Pillow itself, the library's host-only
tables against the restatement, the size rule and the command line of --outscale, the C ABI (header, prototypes, export tables of
all eight libraries), the refusals of the device call (decided on the host before anything is launched) and the compiler's resource
table of the two kernels.

One case of the shared table, (16,16)->(1,1), is 16 : 1 on both axes and so outside the geometry the library accepts (8 : 1, 49
taps): Pillow and the restatement are compared on it like on every other case, and the library is required to refuse it."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from srgd_amd import _lib  # noqa: E402
from srgd_amd import backproject as BP  # noqa: E402
from srgd_amd import consistency as CS  # noqa: E402
from srgd_amd import ensemble as EN  # noqa: E402
from srgd_amd import guidance as GD  # noqa: E402
from srgd_amd import metrics as MX  # noqa: E402
from srgd_amd import resize as RZ  # noqa: E402
from srgd_amd import solver as SV  # noqa: E402
from srgd_amd.inference import parse_args  # noqa: E402
from tests import resize_cases as RC  # noqa: E402
from tests.lib_exports import exports as _exports  # noqa: E402
from tools.kernel_resources import kernel_table  # noqa: E402

ENTRIES = {"srgd_resize_last_error", "srgd_resize_ksize", "srgd_resize_coeffs", "srgd_resize_u8_images"}


# ------------------------------------------------------------------------------------------- (a) the restatement is Pillow's resize
@pytest.mark.parametrize("filter", list(RC.FILTERS))
def test_the_restatement_is_pillows_resize_bit_for_bit(filter):
    assert RZ.FILTERS == RC.FILTERS == {"bicubic": Image.Resampling.BICUBIC, "bilinear": Image.Resampling.BILINEAR,
                                        "lanczos": Image.Resampling.LANCZOS}
    for in_size, out_size in RC.CASES:
        for name in RC.PATTERNS:
            img = RC.pattern(name, *in_size)
            want = np.asarray(Image.fromarray(img, "RGB").resize((out_size[1], out_size[0]), Image.Resampling(RC.FILTERS[filter])))
            got = RC.expected(name, in_size, out_size, filter)
            assert got.shape == want.shape == (out_size[0], out_size[1], 3) and got.dtype == np.uint8
            assert np.array_equal(got, want), (in_size, out_size, filter, name)
    # the checkerboard reaches both ends of clip8 through the negative lobes of the two filters that have them
    if filter != "bilinear":
        up = RC.expected("checker", (8, 6), (64, 48), filter)
        assert up.min() == 0 and up.max() == 255


# ------------------------------------------------------------------------------------------- (b) the library's tables
@pytest.mark.parametrize("filter", list(RC.FILTERS))
def test_the_librarys_tables_are_the_restatements(filter):
    pairs = RC.axis_pairs()
    assert len(pairs) > 1400 and (48, 6) in pairs and (1, 8) in pairs and (200, 25) in pairs
    widest = 0
    for in_size, out_size in pairs:
        bounds, kk = RZ.coeffs(in_size, out_size, filter)
        want_bounds, want_kk = RC.table(in_size, out_size, filter)
        assert RZ.ksize(in_size, out_size, filter) == RC.ksize(in_size, out_size, filter) == kk.shape[1], (in_size, out_size)
        assert bounds.dtype == kk.dtype == np.int32
        assert np.array_equal(bounds, want_bounds), (in_size, out_size)
        assert np.array_equal(kk, want_kk), (in_size, out_size)
        widest = max(widest, kk.shape[1])
    assert widest == {"bicubic": 33, "bilinear": 17, "lanczos": RZ.MAX_TAPS}[filter]      # 8 : 1 is among the pairs


def test_the_host_functions_refuse_what_the_header_says():
    lib = RZ.lib()
    buf = (C.c_int32 * 4096)()
    at = C.cast(buf, C.c_void_p)
    for in_size, out_size, filter, phrase in ((0, 4, 3, "bad size"), (4, 0, 3, "bad size"), (-1, 4, 3, "bad size"), (16385, 16385, 3, "bad size"),
                                              (17, 2, 3, "ratio"), (2, 17, 3, "ratio"), (16, 1, 1, "ratio"), (8, 8, 0, "unknown filter"),
                                              (8, 8, 4, "unknown filter")):
        assert lib.srgd_resize_ksize(in_size, out_size, filter) == -1
        assert phrase in lib.srgd_resize_last_error().decode(), (in_size, out_size, filter)
        assert lib.srgd_resize_coeffs(in_size, out_size, filter, at, at) == -1
        assert phrase in lib.srgd_resize_last_error().decode(), (in_size, out_size, filter)
    assert lib.srgd_resize_coeffs(8, 8, 3, None, at) == -1 and "null" in lib.srgd_resize_last_error().decode()
    assert lib.srgd_resize_coeffs(8, 8, 3, at, None) == -1 and "null" in lib.srgd_resize_last_error().decode()
    assert not any(buf)                                                       # a refused call writes nothing
    assert lib.srgd_resize_ksize(16384, 2048, 1) == RZ.MAX_TAPS and lib.srgd_resize_ksize(8, 8, 2) == 3
    for in_size, out_size in RC.REFUSED_CASES:                                # 16 : 1
        with pytest.raises(ValueError, match="ratio"):
            RZ.coeffs(in_size[0], out_size[0], "lanczos")
        with pytest.raises(ValueError, match="ratio"):
            RZ.check_sizes([in_size + out_size])


def test_table_buffer_layout():
    sizes = [(40, 52, 20, 26), (33, 65, 33, 31), (6, 8, 6, 8), (65, 33, 31, 33), (40, 52, 20, 26)]
    tab, offsets = RZ.build_tables(sizes, "lanczos")
    assert tab.dtype == np.int32 and all(off % 16 == 0 for off in offsets) and offsets[0] == offsets[4] == 0      # shared by geometry
    assert offsets[2] == offsets[3]                                           # the copy has no table: the next image's begin where its would
    for (h_in, w_in, h_out, w_out), off in zip(sizes, offsets):
        at = off // 4
        for a, b in ((w_in, w_out), (h_in, h_out)):
            if a == b:
                continue
            bounds, kk = RC.table(a, b, "lanczos")
            assert np.array_equal(tab[at:at + 2 * b].reshape(b, 2), bounds)
            at += 2 * b
            assert np.array_equal(tab[at:at + kk.size].reshape(kk.shape), kk)
            at += kk.size
    assert RZ.scratch_bytes(sizes) == sum((3 * s[0] * s[3] + 15) // 16 * 16 for s in sizes)


# ------------------------------------------------------------------------------------------- (c) the size rule and the command line
def test_outscale_size():
    assert RZ.outscale_size(10, 13, 2) == (20, 26) and RZ.outscale_size(10, 13, 3) == (30, 39)      # exact multiples
    assert RZ.outscale_size(10, 13, 4.0) == (40, 52) and RZ.outscale_size(24, 20, 2) == (48, 40)
    assert RZ.outscale_size(5, 3, 0.5) == (3, 2)                              # 2.5 and 1.5: halves go up
    assert RZ.outscale_size(3, 7, 1.5) == (5, 11)                             # 4.5 -> 5, 10.5 -> 11
    assert RZ.outscale_size(10, 13, 1.24) == (12, 16) and RZ.outscale_size(10, 13, 1.26) == (13, 16)
    assert RZ.outscale_size(1, 1, 0.5) == (1, 1) and RZ.outscale_size(1, 2, 0.6) == (1, 1)          # 0.5 -> 1 by the half-way rule, floor of 1
    assert RZ.outscale_size(1, 3, 32) == (32, 96) and RZ.outscale_size(1, 2, 0.125) == (1, 1)      # floor(0.625) = 0 -> 1
    for n in range(1, 300):                                                   # every output stays within the kernels' ratio of the x4 image
        for s in (0.5, 0.51, 1, 1.5, 31.9, 32):
            out = RZ.outscale_size(n, n, s)[0]
            assert 4 * n <= 8 * out and out <= 8 * 4 * n, (n, s)
    assert RZ.check_outscale(None) is None and RZ.check_outscale(4) is None and RZ.check_outscale(4.0) is None
    assert RZ.check_outscale(2) == 2.0 and RZ.check_outscale(0.5) == 0.5 and RZ.check_outscale(32) == 32.0
    for bad in (0.49, 32.01, float("nan"), float("inf"), -2, "2", True):
        with pytest.raises(ValueError):
            RZ.check_outscale(bad)
    assert RZ.check_filter(None) == "bicubic" and [RZ.check_filter(f) for f in RZ.FILTERS] == list(RZ.FILTERS)
    for bad in ("box", "BICUBIC", 3):
        with pytest.raises(ValueError):
            RZ.check_filter(bad)


def test_argument_parsing():
    base = ["-c", "conf.yaml", "-m", "ckpt.pth", "--input_dir", "in", "--output_dir", "out"]
    plain = parse_args(base)
    assert plain.outscale is None and plain.outscale_filter == "bicubic"
    off = parse_args(base + ["--outscale", "4"])
    assert off.outscale is None and vars(off) == vars(plain)                   # --outscale 4 parses to "off"
    two = parse_args(base + ["--outscale", "2"])
    assert two.outscale == 2.0 and two.outscale_filter == "bicubic"
    three = parse_args(base + ["--outscale", "3", "--outscale_filter", "lanczos", "--samples", "3", "--consistency", "--back_project", "2"])
    assert three.outscale == 3.0 and three.outscale_filter == "lanczos"
    assert parse_args(base + ["--outscale", "0.5"]).outscale == 0.5 and parse_args(base + ["--outscale", "32"]).outscale == 32.0
    for extra in (["--outscale", "0.49"], ["--outscale", "32.5"], ["--outscale", "nan"], ["--outscale", "inf"], ["--outscale", "-inf"],
                  ["--outscale", "-2"], ["--outscale", "0"], ["--outscale_filter", "lanczos"],
                  ["--outscale", "4", "--outscale_filter", "bilinear"], ["--outscale", "2", "--outscale_filter", "box"],
                  ["--ensemble", "--samples", "2", "--outscale", "2"], ["--ensemble", "--samples", "2", "--outscale", "3.5"]):
        with pytest.raises(SystemExit) as err:
            parse_args(base + extra)
        assert err.value.code not in (0, None), extra
    assert parse_args(base + ["--ensemble", "--samples", "2", "--outscale", "4"]).ensemble      # the default scale keeps --ensemble


# ------------------------------------------------------------------------------------------- (d) C ABI, refusals, resources
def test_entries_are_declared_prototyped_and_exported_by_a_library_of_their_own():
    header = open(os.path.join(ROOT, "include", "srgd_resize.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(srgd_[a-z0-9_]+)\s*\(", flat))
    assert declared == ENTRIES == set(RZ.PROTOTYPES)
    for name, (_, argtypes) in RZ.PROTOTYPES.items():
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", flat).group(1).strip()
        assert (0 if params == "void" else len(params.split(","))) == len(argtypes), name
    fields = re.search(r"typedef struct srgd_resize_image \{(.*?)\}", flat, flags=re.S).group(1)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert names == [f[0] for f in RZ.ResizeImage._fields_] and C.sizeof(RZ.ResizeImage) == 40
    for const, value in (("SRGD_RESIZE_MAX_TAPS", RZ.MAX_TAPS), ("SRGD_RESIZE_MAX_RATIO", RZ.MAX_RATIO), ("SRGD_RESIZE_MAX_SIDE", RZ.MAX_SIDE),
                         ("SRGD_RESIZE_LANCZOS", 1), ("SRGD_RESIZE_BILINEAR", 2), ("SRGD_RESIZE_BICUBIC", 3)):
        assert re.search(r"#define " + const + r" +" + str(value) + r"\b", header), const
    assert RZ.MAX_TAPS == 49 == 2 * 3 * RZ.MAX_RATIO + 1
    assert os.path.exists(RZ.LIB_PATH), "build the library first (python -m srgd_amd.build)"
    assert _exports(RZ.LIB_PATH) == ENTRIES
    assert RZ.lib().srgd_resize_last_error() is not None                       # binds every prototype
    for mod in (_lib, MX, EN, CS, BP, GD, SV):           # the seven other libraries keep their export tables
        assert _exports(mod.LIB_PATH) == set(mod.PROTOTYPES), mod.__name__
        assert not any(n.startswith("srgd_resize") for n in _exports(mod.LIB_PATH)), mod.__name__
        assert not set(RZ.PROTOTYPES) & set(mod.PROTOTYPES)
    for phrase in ("bit for bit", "A pass whose in == out is skipped; when both are skipped the image is copied",
                   "identical to the call on that image alone", "nothing is launched, nothing is written",
                   "Asynchronous on `stream`; no allocation, no synchronisation"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", header), phrase


def test_refusals_need_no_gpu():
    # every refusal is decided on the host before anything is launched, so it can be checked here: -1 and a message
    lib = RZ.lib()
    src, dst, tables, scratch = 1 << 30, 2 << 30, 3 << 30, 4 << 30            # never dereferenced: a refused call launches nothing
    big = 1 << 40

    def rec(**kw):
        return RZ.ResizeImage(**dict(dict(src_off=0, dst_off=0, tab_off=0, h_in=40, w_in=52, h_out=20, w_out=26), **kw))

    def call(images=None, n=None, **kw):
        images = [rec()] if images is None else images
        a = dict(dict(src=src, dst=dst, filter=3, tables=tables, tables_bytes=big, scratch=scratch, scratch_bytes=big), **kw)
        arr = (RZ.ResizeImage * len(images))(*images) if images != "null" else None
        rc = lib.srgd_resize_u8_images(a["src"], a["dst"], arr, len(images) if n is None else n, a["filter"], a["tables"],
                                       a["tables_bytes"], a["scratch"], a["scratch_bytes"], None)
        return rc, lib.srgd_resize_last_error().decode()
    good = rec(src_off=16 * 400, dst_off=16 * 100, tab_off=16 * 3)
    cases = {"null": [dict(src=None), dict(dst=None), dict(tables=None), dict(scratch=None), dict(images="null", n=1)],
             "n_images": [dict(n=0), dict(n=-1)],
             "bad size": [dict(images=[rec(h_in=0)]), dict(images=[rec(w_out=0)]), dict(images=[rec(h_out=-3)]),
                          dict(images=[rec(w_in=16385, w_out=16385)]), dict(images=[good, rec(w_in=0)])],
             "ratio": [dict(images=[rec(h_in=161)]), dict(images=[rec(w_in=3)]), dict(images=[rec(h_in=16, w_in=16, h_out=1, w_out=1)]),
                       dict(images=[good, good, rec(h_out=4)])],
             "multiple of 16": [dict(images=[rec(src_off=8)]), dict(images=[rec(dst_off=17)]), dict(images=[rec(tab_off=4)]),
                                dict(images=[good, rec(dst_off=24)])],
             "outside [0, 2^36)": [dict(images=[rec(src_off=-16)]), dict(images=[rec(dst_off=1 << 36)]), dict(images=[rec(tab_off=-16)])],
             "unknown filter": [dict(filter=0), dict(filter=4), dict(filter=-1)],
             "scratch must be 16-byte aligned": [dict(scratch=scratch + 8)],
             "tables must be 16-byte aligned": [dict(tables=tables + 4)],
             "tables_bytes": [dict(tables_bytes=4 * (26 * (2 + 9) + 20 * (2 + 9)) - 1), dict(images=[rec(tab_off=64)], tables_bytes=64)],
             "scratch_bytes": [dict(scratch_bytes=3 * 40 * 26 - 1), dict(images=[good, rec()], scratch_bytes=2 * 3 * 40 * 26 - 16)],
             "overlap": [dict(dst=src), dict(dst=src + 16 * 100), dict(images=[rec(src_off=1 << 30)])]}
    for phrase, calls in cases.items():
        for kw in calls:
            rc, msg = call(**kw)
            assert rc == -1 and phrase in msg, (phrase, kw, msg)


@pytest.fixture(scope="module")
def table_of_resources():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    return kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "resize.hip"))


def test_the_kernels_do_not_spill(table_of_resources):
    rows = {r["name"]: r for r in table_of_resources}
    assert set(rows) == {"resize_horizontal_kernel", "resize_vertical_kernel"}
    for name, r in rows.items():
        assert r["spill"] == 0 and r["scratch"] == 0, f"{name} spills ({r['spill']} VGPRs, {r['scratch']} B scratch)"
        assert 0 < r["vgpr"] + max(r["agpr"], 0) <= 64, f"{name} uses {r['vgpr']} + {r['agpr']} registers"      # 8 waves per SIMD
    assert rows["resize_horizontal_kernel"]["lds"] == 16 * 916 + 4 * 32 * 49 + 4 * 64 + 16 * 96
    assert rows["resize_vertical_kernel"]["lds"] == 4 * 16 * 49 + 4 * 32
