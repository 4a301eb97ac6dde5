"""srgd_amd.selfens without a GPU: the dihedral operations and the merge of tests/selfens_cases.py against their definition, the
command line of --self_ensemble, the C ABI (header, prototypes, structure layout, export tables of all eleven libraries), the refusals
of both device calls (decided on the host before anything is launched), the compiler's resource table of the two kernels, and the
folder driver on stubs: order, sizes, seeds and labels of the variants, the merge of variant sets that straddle flush() calls,
skip-if-exists, what is measured, and that self_ensemble=1 changes nothing."""
import ctypes as C
import json
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from srgd_amd import _lib  # noqa: E402
from srgd_amd import alpha as AL  # noqa: E402
from srgd_amd import backproject as BP  # noqa: E402
from srgd_amd import consistency as CS  # noqa: E402
from srgd_amd import ensemble as EN  # noqa: E402
from srgd_amd import guidance as GD  # noqa: E402
from srgd_amd import metrics as MX  # noqa: E402
from srgd_amd import resize as RZ  # noqa: E402
from srgd_amd import selfens as SE  # noqa: E402
from srgd_amd import solver as SV  # noqa: E402
from srgd_amd import threshold as TH  # noqa: E402
from srgd_amd import inference as INF  # noqa: E402
from srgd_amd.inference import parse_args  # noqa: E402
from srgd_amd.lockstep import even_step_tiles  # noqa: E402
from tests import selfens_cases as SC  # noqa: E402
from tests.lib_exports import exports as _exports  # noqa: E402
from tools.kernel_resources import kernel_table  # noqa: E402

ENTRIES = {"srgd_selfens_last_error", "srgd_selfens_transform", "srgd_selfens_merge"}


# ------------------------------------------------------------------------------------------- (a) the operations and the merge
def test_the_eight_operations_form_the_dihedral_group():
    x = np.arange(5 * 6 * 3, dtype=np.uint8).reshape(5, 6, 3)                  # distinct bytes
    images = [SC.apply(x, op) for op in range(8)]
    for op, y in enumerate(images):
        assert y.shape == ((6, 5, 3) if op >= 4 else (5, 6, 3)) and y.flags.c_contiguous
        assert np.array_equal(SC.apply(y, SC.inverse(op)), x), op
        assert SC.inverse(op) == SE.inverse(op) == (6 if op == 5 else 5 if op == 6 else op)
        assert SE.out_size(5, 6, op) == y.shape[:2]
    assert all(not (a.shape == b.shape and np.array_equal(a, b)) for i, a in enumerate(images) for b in images[i + 1:])    # eight different images
    for a in range(8):                                                         # closed under composition
        for b in range(8):
            c = SC.compose(a, b)
            assert np.array_equal(SC.apply(SC.apply(x, a), b), SC.apply(x, c))
        assert SC.compose(a, SC.inverse(a)) == 0
    assert np.array_equal(images[0], x) and np.array_equal(images[1], x[:, ::-1]) and np.array_equal(images[2], x[::-1])
    assert np.array_equal(images[3], x[::-1, ::-1])
    assert np.array_equal(images[4], np.transpose(x, (1, 0, 2)))
    # op 4 then op 1 is op 5: the transpose with its columns reversed, a quarter turn CLOCKWISE - np.rot90(x, k=-1) (k=1, numpy's
    # default direction, is counterclockwise and is op 6)
    assert SC.compose(4, 1) == 5 and np.array_equal(images[5], np.rot90(x, k=-1)) and np.array_equal(images[6], np.rot90(x, k=1))
    assert np.array_equal(images[3], np.rot90(x, k=2)) and np.array_equal(images[7], np.rot90(x, k=2).swapaxes(0, 1))
    assert SE.OPS == SC.OPS == {1: (0,), 2: (0, 1), 4: (0, 1, 2, 3), 8: (0, 1, 2, 3, 4, 5, 6, 7)}
    for bad in (-1, 8, 1.0, True, "1", None):
        with pytest.raises(ValueError):
            SE.inverse(bad)


def test_a_hand_computed_merge_and_the_rounding_cases():
    x0 = np.array([[[0, 1, 2], [3, 4, 5], [6, 7, 8]], [[10, 20, 30], [40, 50, 60], [70, 80, 255]]], np.uint8)      # [2, 3, 3]
    x1 = np.array([[[1, 1, 3], [3, 5, 5], [9, 7, 8]], [[11, 22, 30], [40, 53, 61], [70, 81, 255]]], np.uint8)
    # halves go up: (0 + 1) / 2 -> 1, (2 + 3) / 2 -> 3, (6 + 9) / 2 -> 8, (20 + 22) / 2 = 21 exactly, (50 + 53) / 2 -> 52
    want = np.array([[[1, 1, 3], [3, 5, 5], [8, 7, 8]], [[11, 21, 30], [40, 52, 61], [70, 81, 255]]], np.uint8)
    assert np.array_equal(SC.merge([x0, x1], (0, 0)), want)
    mirrored = x1[:, ::-1].copy()                                              # source 1 as the driver holds it: apply(x1, 1)
    assert np.array_equal(mirrored[0, 0], [9, 7, 8]) and np.array_equal(SC.merge([x0, mirrored], (0, 1)), want)
    assert np.array_equal(SC.merge([SC.apply(x0, 5), SC.apply(x1, 6)], (5, 6)), want)
    assert np.array_equal(SC.merge([x0], (0,)), x0) and np.array_equal(SC.merge([SC.apply(x0, 7)], (7,)), x0)
    m01 = SC.mean01(want)
    assert m01.shape == (3, 2, 3) and m01.dtype == np.float32 and m01[2, 1, 2] == np.float32(1.0) and m01[0, 0, 0] == np.float32(1) / np.float32(255)
    for n in (2, 4, 8):                                                        # S mod n == n / 2 goes up, n / 2 - 1 goes down
        ops = SC.OPS[n]
        srcs = SC.sources(5, 6, ops, "halves")
        total = sum(SC.apply(s, SC.inverse(op)).astype(np.int64) for s, op in zip(srcs, ops)).reshape(-1)
        assert (total[0::2] % n == n // 2).all() and (total[1::2] % n == n // 2 - 1).all()
        got = SC.merge(srcs, ops)
        assert np.array_equal(got, SC.halves_expected(5, 6, n))
        assert np.array_equal(got.reshape(-1)[0::2].astype(np.int64), total[0::2] // n + 1) and np.array_equal(got.reshape(-1)[1::2], total[1::2] // n)
    ones = SC.merge(SC.sources(7, 1, SC.OPS[8], "ones"), SC.OPS[8])
    assert ones.shape == (7, 1, 3) and (ones == 255).all()
    assert len(SC.SIZES) == 10 and {(3 * w) % 16 for _, w in SC.SIZES} >= {0, 2, 3, 5, 9, 13, 15}
    for h, w in ((63, 65), (65, 63), (129, 67), (16, 341)):                    # rows start at every byte phase modulo 16
        assert {(3 * w * y) % 16 for y in range(h)} == set(range(16)), (h, w)
    assert sorted(SC.OP_LISTS) == [1, 2, 3, 4, 5, 8] and all(len(v) == k for k, v in SC.OP_LISTS.items()) and len(set(SC.REPEATED)) < len(SC.REPEATED)


# ------------------------------------------------------------------------------------------- (b) the command line
def test_argument_parsing_and_the_refusals(tmp_path, monkeypatch):
    base = ["-c", "conf.yaml", "-m", "ckpt.pth", "--input_dir", "in", "--output_dir", "out"]
    plain = parse_args(base)
    assert plain.self_ensemble == 1 and vars(parse_args(base + ["--self_ensemble", "1"])) == vars(plain)
    for n in (2, 4, 8):
        assert parse_args(base + ["--self_ensemble", str(n)]).self_ensemble == n
    both = parse_args(base + ["--self_ensemble", "8", "--samples", "2", "--ensemble", "--consistency", "--lockstep_tiles", "16"])
    assert both.self_ensemble == 8 and both.samples == 2 and both.ensemble
    for extra in (["--self_ensemble", "3"], ["--self_ensemble", "0"], ["--self_ensemble", "16"], ["--self_ensemble", "-2"],
                  ["--self_ensemble", "2.0"], ["--self_ensemble", "eight"]):
        with pytest.raises(SystemExit) as err:
            parse_args(base + extra)
        assert err.value.code not in (0, None), extra
    assert [SE.check_self_ensemble(n) for n in (None, 1, 2, 4, 8)] == [1, 1, 2, 4, 8]
    for bad in (0, 3, 5, 6, 7, 16, -8, 2.0, True, "8"):
        with pytest.raises(ValueError):
            SE.check_self_ensemble(bad)
        with pytest.raises(ValueError):                                       # before a file is listed or the model is touched
            INF.batch_sr_target_images(str(tmp_path / "no_such_folder"), str(tmp_path / "out"), None, self_ensemble=bad)
    assert not os.path.exists(tmp_path / "out")
    # an EDM config: refused from the configuration file, before the model is built
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    assert "model: conditional_continuous" in conf_src
    edm = tmp_path / "edm.yaml"
    edm.write_text(conf_src.replace("model: conditional_continuous", "model: conditional_elucidated"))

    def no_model(*a, **kw):
        raise AssertionError("the model must not be built")
    monkeypatch.setattr(INF, "get_model", no_model)
    argv = ["-c", str(edm), "-m", "ckpt.pth", "--input_dir", str(tmp_path / "in"), "--output_dir", str(tmp_path / "out")]
    with pytest.raises(SystemExit) as err:
        INF.main(argv + ["--self_ensemble", "2"])
    assert "--self_ensemble" in str(err.value) and "EDM" in str(err.value) and not os.path.exists(tmp_path / "out")
    with pytest.raises(AssertionError, match="must not be built"):            # without the flag the same command goes on to the model
        INF.main(argv)
    from srgd_amd.model import ConditionalElucidatedDiffusionSR
    with pytest.raises(ValueError, match="EDM"):
        INF.batch_sr_target_images(str(tmp_path / "in"), str(tmp_path / "out"), object.__new__(ConditionalElucidatedDiffusionSR), self_ensemble=4)
    assert not os.path.exists(tmp_path / "out")
    assert INF.dihedral_on_device is SE.dihedral_on_device and INF.self_ensemble_on_device is SE.self_ensemble_on_device


# ------------------------------------------------------------------------------------------- (c) C ABI, refusals, resources
def test_entries_are_declared_prototyped_and_exported_by_a_library_of_their_own():
    header = open(os.path.join(ROOT, "include", "srgd_selfens.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(srgd_[a-z0-9_]+)\s*\(", flat))
    assert declared == ENTRIES == set(SE.PROTOTYPES)
    for name, (_, argtypes) in SE.PROTOTYPES.items():
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", flat).group(1).strip()
        assert (0 if params == "void" else len(params.split(","))) == len(argtypes), name
    for struct, cls, size in (("srgd_selfens_record", SE.SelfensRecord, 32), ("srgd_selfens_image", SE.SelfensImage, 128)):
        fields = re.search(r"typedef struct " + struct + r" \{(.*?)\}", flat, flags=re.S).group(1)
        names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
        assert [n.replace("[8]", "") for n in names] == [f[0] for f in cls._fields_] and C.sizeof(cls) == size, struct
        assert [n for n in names if n.endswith("[8]")] == [f[0] + "[8]" for f in cls._fields_ if hasattr(f[1], "_length_")]
    assert [(f[0], getattr(SE.SelfensImage, f[0]).offset) for f in SE.SelfensImage._fields_] == \
        [("dst_off", 0), ("mean01_off", 8), ("H", 16), ("W", 20), ("n_src", 24), ("pad", 28), ("src_off", 32), ("op", 96)]
    assert [getattr(SE.SelfensRecord, f[0]).offset for f in SE.SelfensRecord._fields_] == [0, 8, 16, 20, 24, 28]
    for const, value in (("SRGD_SELFENS_MAX_SOURCES", SE.MAX_SOURCES), ("SRGD_SELFENS_MAX_IMAGES", SE.MAX_IMAGES), ("SRGD_SELFENS_TILE", SE.TILE),
                         ("SRGD_SELFENS_LDS_TRANSFORM", SE.LDS_TRANSFORM), ("SRGD_SELFENS_LDS_MERGE", SE.LDS_MERGE)):
        assert re.search(r"#define " + const + r" +" + str(value) + r"\b", header), const
    assert SE.MAX_IMAGES == SC.MAX_IMAGES == 32 and SE.MAX_SOURCES == SC.MAX_SOURCES == 8 and SE.TILE == SC.TILE
    assert os.path.exists(SE.LIB_PATH), "build the library first (python -m srgd_amd.build)"
    assert _exports(SE.LIB_PATH) == ENTRIES
    assert SE.lib().srgd_selfens_last_error() is not None                      # binds every prototype
    others = (_lib, MX, EN, CS, BP, GD, SV, RZ, AL, TH)
    assert len({mod.LIB_PATH for mod in others} | {SE.LIB_PATH}) == 11
    for mod in others:                                   # the ten other libraries keep their export tables
        assert _exports(mod.LIB_PATH) == set(mod.PROTOTYPES), mod.__name__
        assert not any(n.startswith("srgd_selfens") for n in _exports(mod.LIB_PATH)), mod.__name__
        assert not set(SE.PROTOTYPES) & set(mod.PROTOTYPES)
    for phrase in ("m = (2*S + n) div (2*n)", "identical to the call on that image alone", "nothing is launched, nothing is written",
                   "Asynchronous on `stream`; no allocation, no synchronisation", "Every source byte is read once, every output byte written once",
                   "inverse(5) = 6", "3*h*w < 2^31"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", header), phrase
    from srgd_amd import build as B
    row = {name: (lib, sources) for name, lib, sources, _ in B.LIBRARIES}["selfens"]
    assert row[1] == ["selfens.hip"] and "selfens.hip" not in B.SOURCES and row[0] == SE.LIB_PATH


def test_an_unbuilt_library_is_an_error_not_a_fallback(monkeypatch, tmp_path):
    monkeypatch.setattr(SE, "_handle", None)
    monkeypatch.setattr(SE, "LIB_PATH", str(tmp_path / "libsrgd_selfens.so"))
    with pytest.raises(_lib.SrgdHipError, match="srgd_amd.build"):
        SE.lib()


def test_refusals_need_no_gpu():
    # every refusal is decided on the host before anything is launched, so it can be checked here: -1 and a message
    lib = SE.lib()
    src, dst, m01 = 1 << 30, 2 << 30, 3 << 30                                  # never dereferenced: a refused call launches nothing

    def record(**kw):
        return SE.SelfensRecord(**dict(dict(src_off=0, dst_off=0, h=7, w=5, op=5, pad=0), **kw))

    def transform(records=None, n=None, **kw):
        records = [record()] if records is None else records
        a = dict(dict(src=src, dst=dst), **kw)
        arr = (SE.SelfensRecord * len(records))(*records) if records != "null" else None
        rc = lib.srgd_selfens_transform(a["src"], a["dst"], arr, len(records) if n is None else n, None)
        return rc, lib.srgd_selfens_last_error().decode()
    good = record(src_off=16 * 40, dst_off=16 * 90)
    side = 26755                                                               # 3 * 26755^2 >= 2^31 > 3 * 26754^2
    assert 3 * side * side >= 2 ** 31 > 3 * (side - 1) * (side - 1)
    cases = {"null": [dict(src=None), dict(dst=None), dict(records="null", n=1)],
             "n must be": [dict(n=0), dict(n=-1)],
             "bad size": [dict(records=[record(h=0)]), dict(records=[record(w=-3)]), dict(records=[record(h=side, w=side)]),
                          dict(records=[record(h=1, w=715827883)]), dict(records=[good, record(w=0)]), dict(records=[record(h=2 ** 31 - 1, w=2 ** 31 - 1)])],
             "op outside": [dict(records=[record(op=8)]), dict(records=[record(op=-1)]), dict(records=[good, good, record(op=9)])],
             "multiple of 16": [dict(records=[record(src_off=8)]), dict(records=[record(dst_off=17)]), dict(records=[good, record(dst_off=24)])],
             "outside [0, 2^36)": [dict(records=[record(src_off=-16)]), dict(records=[record(dst_off=1 << 36)])],
             "16-byte aligned": [dict(src=src + 4), dict(dst=dst + 8)],
             "overlap": [dict(dst=src), dict(dst=src + 96), dict(records=[record(src_off=1 << 30)])]}
    for phrase, calls in cases.items():
        for kw in calls:
            rc, msg = transform(**kw)
            assert rc == -1 and phrase in msg and msg.startswith("srgd_selfens_transform"), (phrase, kw, msg)

    def image(**kw):
        f = dict(dict(dst_off=0, mean01_off=0, H=7, W=5, n_src=2, pad=0, src_off=[0, 112], op=[0, 5]), **kw)
        im = SE.SelfensImage(f["dst_off"], f["mean01_off"], f["H"], f["W"], f["n_src"], f["pad"])
        for j, (off, op) in enumerate(zip(f["src_off"], f["op"])):
            im.src_off[j], im.op[j] = off, op
        return im

    def merge(images=None, n=None, **kw):
        images = [image()] if images is None else images
        a = dict(dict(src=src, dst=dst, m01=m01), **kw)
        arr = (SE.SelfensImage * len(images))(*images) if images != "null" else None
        rc = lib.srgd_selfens_merge(a["src"], a["dst"], a["m01"], arr, len(images) if n is None else n, None)
        return rc, lib.srgd_selfens_last_error().decode()
    cases = {"null": [dict(src=None), dict(dst=None), dict(images="null", n=1), dict(src=None, m01=None)],
             "n_images": [dict(n=0), dict(n=-2)],
             "n_src": [dict(images=[image(n_src=0)]), dict(images=[image(n_src=9)]), dict(images=[image(), image(n_src=-1)])],
             "bad size": [dict(images=[image(H=0)]), dict(images=[image(W=-1)]), dict(images=[image(H=side, W=side)]), dict(images=[image(), image(W=0)])],
             "op outside": [dict(images=[image(op=[0, 8])]), dict(images=[image(op=[-1, 0])]), dict(images=[image(), image(op=[3, 77])])],
             "multiple of 16": [dict(images=[image(dst_off=8)]), dict(images=[image(src_off=[0, 100])]), dict(images=[image(), image(src_off=[4, 112])])],
             "outside [0, 2^36)": [dict(images=[image(dst_off=-16)]), dict(images=[image(src_off=[0, 1 << 36])])],
             "negative mean01": [dict(images=[image(mean01_off=-1)]), dict(images=[image(), image(mean01_off=-4)])],
             "16-byte aligned": [dict(src=src + 4), dict(dst=dst + 8)],
             "4-byte aligned": [dict(m01=m01 + 2)],
             "overlap": [dict(dst=src), dict(dst=src + 208), dict(images=[image(src_off=[0, 1 << 30])])]}
    for phrase, calls in cases.items():
        for kw in calls:
            rc, msg = merge(**kw)
            assert rc == -1 and phrase in msg and msg.startswith("srgd_selfens_merge"), (phrase, kw, msg)
    # ignored fields: the entries j >= n_src of a record, and mean01_off where mean01 is NULL, are not looked at - such calls pass
    # the host checks up to the launch, which this test never reaches


def test_the_list_apis_refuse_bad_arguments_and_need_a_gpu():
    a, b = torch.zeros(4, 5, 3, dtype=torch.uint8), torch.zeros(5, 4, 3, dtype=torch.uint8)
    for bad in (lambda: SE.dihedral_on_device([], []), lambda: SE.dihedral_on_device([a], [0, 1]), lambda: SE.dihedral_on_device([a], [8]),
                lambda: SE.dihedral_on_device([a.float()], [0]), lambda: SE.dihedral_on_device([a[:, :, :2]], [0]), lambda: SE.dihedral_on_device(a, [0]),
                lambda: SE.dihedral_on_device([a[:0]], [0]), lambda: SE.dihedral_on_device([a], [1.0]),
                lambda: SE.self_ensemble_on_device([]), lambda: SE.self_ensemble_on_device([[]]), lambda: SE.self_ensemble_on_device([[(a, 0)] * 9]),
                lambda: SE.self_ensemble_on_device([[(a, 0), (b, 0)]]), lambda: SE.self_ensemble_on_device([[(a, 0), (a, 4)]]),
                lambda: SE.self_ensemble_on_device([[(a, 8)]]), lambda: SE.self_ensemble_on_device([[(a.int(), 0)]]),
                lambda: SE.self_ensemble_on_device([[a]]), lambda: SE.self_ensemble_on_device([(a, 0)])):
        with pytest.raises(ValueError):
            bad()
    if not torch.cuda.is_available():                                         # no CPU fallback
        for call in (lambda: SE.dihedral_on_device([a], [5]), lambda: SE.self_ensemble_on_device([[(a, 0), (b, 4)]]),
                     lambda: SE.self_ensemble_on_device([[(a, 0)]], return_mean01=True)):
            with pytest.raises(_lib.SrgdHipError):
                call()
        flat = torch.zeros(256, dtype=torch.uint8)
        with pytest.raises(_lib.SrgdHipError):
            SE.transform_flat(flat, [0], flat.clone(), [0], [(4, 5)], [1])
        with pytest.raises(_lib.SrgdHipError):
            SE.merge_flat(flat, [[0, 64]], [[0, 4]], flat.clone(), [0], [(4, 5)])


@pytest.fixture(scope="module")
def table_of_resources():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    return kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "selfens.hip"))


def test_the_kernels_do_not_spill(table_of_resources):
    rows = {r["name"]: r for r in table_of_resources}
    assert set(rows) == {"selfens_transform_kernel", "selfens_merge_kernel"}
    for name, r in rows.items():
        assert r["spill"] == 0 and r["scratch"] == 0, f"{name} spills ({r['spill']} VGPRs, {r['scratch']} B scratch)"
        assert 0 < r["vgpr"] + max(r["agpr"], 0) <= 64, f"{name} uses {r['vgpr']} + {r['agpr']} registers"      # 8 waves per SIMD
    assert rows["selfens_transform_kernel"]["lds"] == SE.LDS_TRANSFORM == 32 * 116
    assert rows["selfens_merge_kernel"]["lds"] == SE.LDS_MERGE == 8 * 32 * 116 + 32 * 96


# ------------------------------------------------------------------------------------------- (d) the folder driver on stubs
LABELS = {"b.png": 2}
SIZES = {"a": (24, 24), "b": (22, 24), "c": (24, 24)}                          # (w, h): b is not square


def _stubs(monkeypatch, log):
    def sampler(kind):
        def run(images, *a, **kw):
            ims = images if isinstance(images, list) else [images]
            seeds = list(a[0]) if kind == "seeded" else [kw.get("seed")] * len(ims)
            labels = kw.get("test_label")
            labels = list(labels) if isinstance(labels, (list, tuple)) else [labels] * len(ims)
            assert "reference" not in kw or log.get("plain")
            log["calls"].append((kind, [np.asarray(im).copy() for im in ims], seeds, labels, sorted(k for k in kw if k != "test_label")))
            outs = [Image.fromarray(SC.orientation_stub(np.asarray(im), s), "RGB") for im, s in zip(ims, seeds)]
            ret = outs if isinstance(images, list) else outs[0]
            if "reference" not in kw:
                return ret
            return ret, [{"psnr_y": 20.0, "psnr_rgb": 1.0, "ssim_y": 0.5} for _ in ims]
        return run
    monkeypatch.setattr(INF, "sr_target_image", sampler("solo"))
    monkeypatch.setattr(INF, "sr_target_images", sampler("same"))
    monkeypatch.setattr(INF, "sr_target_images_mixed", sampler("mixed"))
    monkeypatch.setattr(INF, "sr_target_images_seeded", sampler("seeded"))

    def dihedral(images, ops):
        log["dihedral"].append(([t.numpy().copy() for t in images], list(ops)))
        return [torch.from_numpy(SC.apply(t.numpy(), op)) for t, op in zip(images, ops)]

    def merge(groups, return_mean01=False):
        log["merge"].append([[(t.numpy().copy(), op) for t, op in g] for g in groups])
        merged = [SC.merge([t.numpy() for t, _ in g], [op for _, op in g]) for g in groups]
        if not return_mean01:
            return [torch.from_numpy(m) for m in merged]
        return [(torch.from_numpy(m), torch.from_numpy(SC.mean01(m))[None]) for m in merged]

    def metrics(outs, refs, crop_border=4):
        log["metrics"].append(([o.numpy().copy() for o in outs], [r.numpy().copy() for r in refs], crop_border))
        return [{"psnr_y": float(o.sum()), "psnr_rgb": float(len(log["metrics"])), "ssim_y": 0.25} for o in outs]

    def consistency(outputs, inputs, return_down=False):
        log["consistency"].append(([o.numpy().copy() for o in outputs], [i.numpy().copy() for i in inputs]))
        return [{"lr_psnr": float(o.numpy().astype(np.int64).sum() % 1000), "lr_mse": 1.0, "lr_max_abs": 2.0} for o in outputs]
    monkeypatch.setattr(INF, "dihedral_on_device", dihedral)
    monkeypatch.setattr(INF, "self_ensemble_on_device", merge)
    monkeypatch.setattr(INF, "metrics_on_device", metrics)
    monkeypatch.setattr(INF, "consistency_on_device", consistency)


def _new_log(**kw):
    return dict(dict(calls=[], dihedral=[], merge=[], metrics=[], consistency=[]), **kw)


def _inputs(tmp_path):
    indir, gt = tmp_path / "in", tmp_path / "gt"
    indir.mkdir()
    gt.mkdir()
    lows = {}
    for name, (w, h) in SIZES.items():
        lows[f"{name}.png"] = SC.image(h, w, seed=len(lows) + 3)
        Image.fromarray(lows[f"{name}.png"], "RGB").save(indir / f"{name}.png")
        Image.fromarray(SC.image(4 * h, 4 * w, seed=40 + len(lows)), "RGB").save(gt / f"{name}.png")
    return indir, gt, lows


def _png(path):
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _expected(low, k, seed=71, n=8):
    ops = SC.OPS[n]
    return SC.merge([SC.orientation_stub(SC.apply(low, op), seed + k) for op in ops], ops)


def _check_variants(log, lows, names, seed=71, n=8, samples=2):
    """Order, sizes, seeds and labels of every image the samplers were given: per file, per sample, the ops of OPS[n] in order."""
    seen = [(im, s, lab) for _, ims, seeds, labels, _ in log["calls"] for im, s, lab in zip(ims, seeds, labels)]
    want = [(SC.apply(lows[name], op), seed + k, LABELS.get(name, 1)) for name in names for k in range(samples) for op in SC.OPS[n]]
    assert len(seen) == len(want)
    for (im, s, lab), (wim, ws, wlab) in zip(seen, want):
        assert im.shape == wim.shape and np.array_equal(im, wim) and s == ws and lab == wlab
    assert all("reference" not in keys and "crop_border" not in keys for *_, keys in log["calls"])


def test_the_driver_samples_every_orientation_and_saves_the_merge(tmp_path, monkeypatch):
    indir, gt, lows = _inputs(tmp_path)
    names = sorted(lows)
    log = _new_log()
    _stubs(monkeypatch, log)
    run = lambda tag, **kw: INF.batch_sr_target_images(str(indir), str(tmp_path / tag), None, seed=71, test_label=1, labels=LABELS, **kw)  # noqa: E731
    # 1. neither lock-step argument: groups of N * samples = 16, the transposed half of b split off at the size change
    run("auto", self_ensemble=8, samples=2)
    _check_variants(log, lows, names)
    sizes = [[im.shape[:2] for im in ims] for _, ims, *_ in log["calls"]]
    assert sizes == [[(24, 24)] * 16, [(24, 22)] * 4, [(22, 24)] * 4, [(24, 22)] * 4, [(22, 24)] * 4, [(24, 24)] * 16]
    assert [c[0] for c in log["calls"]] == ["seeded", "same", "same", "same", "same", "seeded"]
    assert [(len(ims), ops) for ims, ops in log["dihedral"]] == [(8, list(range(8)))] * 3          # once per opened file
    assert all(np.array_equal(im, lows[name]) for (ims, _), name in zip(log["dihedral"], names) for im in ims)
    assert [[len(g) for g in call] for call in log["merge"]] == [[8, 8], [8], [8], [8, 8]]         # b: s0 after its second flush, s1 after the fourth
    written = sorted(os.listdir(tmp_path / "auto"))
    assert written == sorted(f"{n[0]}_out{s}.png" for n in names for s in ("", "_s1"))
    for name in names:
        for k, s in enumerate(("", "_s1")):
            got = _png(tmp_path / "auto" / f"{name[0]}_out{s}.png")
            assert got.shape == (4 * lows[name].shape[0], 4 * lows[name].shape[1], 3)
            assert np.array_equal(got, _expected(lows[name], k)), (name, k)
    # the stub depends on the orientation: the merge is not what a single run writes
    assert not np.array_equal(_png(tmp_path / "auto" / "a_out.png"), SC.orientation_stub(lows["a.png"], 71))
    # every source of a merge call is the stub's output of its variant, with the variant's op
    first = log["merge"][0][0]
    assert [op for _, op in first] == list(range(8))
    assert all(np.array_equal(t, SC.orientation_stub(SC.apply(lows["a.png"], op), 71)) for t, op in first)

    # 2. a budget of six images' tiles: variant sets straddle flush() calls and are still merged once each
    tiles = [even_step_tiles(4 * h, 4 * w) for h, w in [(24, 24), (24, 22), (22, 24)]]
    assert len(set(tiles)) == 1
    log2 = _new_log()
    _stubs(monkeypatch, log2)
    run("budget", self_ensemble=8, samples=2, lockstep_tiles=6 * tiles[0], consistency=True, reference_dir=str(gt), crop_border=2)
    _check_variants(log2, lows, names)
    assert [len(ims) for _, ims, *_ in log2["calls"]] == [6] * 8 and len(log2["calls"]) == 8       # 48 variants, b's label alone closes no group
    merged_sets = [len(g) for call in log2["merge"] for g in call]
    assert merged_sets == [8] * 6 and len(log2["merge"]) < 8                   # six entries, each merged exactly once, some flushes complete none
    assert [[len(g) for g in call] for call in log2["merge"]] == [[8], [8], [8], [8], [8], [8]]
    for name in names:
        for s in ("", "_s1"):
            assert open(tmp_path / "budget" / f"{name[0]}_out{s}.png", "rb").read() == open(tmp_path / "auto" / f"{name[0]}_out{s}.png", "rb").read()
    # metrics.json and consistency.json: taken of the merged image, against the reference and against the ORIGINAL input
    order = [(name, k) for name in names for k in range(2)]
    assert len(log2["metrics"]) == len(log2["consistency"]) == 6
    for (name, k), (outs, refs, crop), (c_outs, c_ins) in zip(order, log2["metrics"], log2["consistency"]):
        want = _expected(lows[name], k)
        assert crop == 2 and len(outs) == len(refs) == len(c_outs) == len(c_ins) == 1
        assert outs[0].dtype == np.float32 and np.array_equal(outs[0], SC.mean01(want)[None]) and np.array_equal(refs[0], _png(gt / name))
        assert np.array_equal(c_outs[0], want) and np.array_equal(c_ins[0], lows[name])
    doc = json.load(open(tmp_path / "budget" / "metrics.json"))
    assert list(doc["files"]) == [f"{n[0]}_out{s}.png" for n in names for s in ("", "_s1")] and list(doc["images"]) == names
    assert [doc["files"][f]["psnr_rgb"] for f in doc["files"]] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    cdoc = json.load(open(tmp_path / "budget" / "consistency.json"))
    assert list(cdoc) == ["files", "images", "mean"] and list(cdoc["files"]) == list(doc["files"])
    assert cdoc["files"]["c_out.png"]["lr_psnr"] == float(_expected(lows["c.png"], 0).astype(np.int64).sum() % 1000)

    # 3. skip-if-exists per output file: a complete folder samples nothing; a missing sample brings back all N variants of it alone
    log3 = _new_log()
    _stubs(monkeypatch, log3)
    run("auto", self_ensemble=8, samples=2)
    assert log3["calls"] == [] and log3["merge"] == [] and log3["dihedral"] == []
    keep = open(tmp_path / "auto" / "b_out_s1.png", "rb").read()
    os.remove(tmp_path / "auto" / "b_out_s1.png")
    run("auto", self_ensemble=8, samples=2)
    seen = [(im.shape[:2], s, lab) for _, ims, seeds, labels, _ in log3["calls"] for im, s, lab in zip(ims, seeds, labels)]
    assert seen == [((24, 22), 72, 2)] * 4 + [((22, 24), 72, 2)] * 4 and [[len(g) for g in call] for call in log3["merge"]] == [[8]]
    assert open(tmp_path / "auto" / "b_out_s1.png", "rb").read() == keep

    # 4. N = 2 and 4 with --ensemble: the mean image is the ensemble of the merged samples
    log4 = _new_log()
    _stubs(monkeypatch, log4)
    run("four", self_ensemble=4, end_index=2)
    _check_variants(log4, lows, names[:2], n=4, samples=1)
    assert [[im.shape[:2] for im in ims] for _, ims, *_ in log4["calls"]] == [[(24, 24)] * 4, [(24, 22)] * 4]
    assert np.array_equal(_png(tmp_path / "four" / "b_out.png"), _expected(lows["b.png"], 0, n=4))
    run("two", self_ensemble=2, lockstep=3, start_index=1)
    assert np.array_equal(_png(tmp_path / "two" / "c_out.png"), _expected(lows["c.png"], 0, n=2))
    assert np.array_equal(_png(tmp_path / "two" / "b_out.png"), _expected(lows["b.png"], 0, n=2))


def test_self_ensemble_1_is_a_run_without_the_keyword(tmp_path, monkeypatch):
    indir, gt, lows = _inputs(tmp_path)
    logs = {}
    for tag, kw in (("without", {}), ("with", {"self_ensemble": 1}), ("none", {"self_ensemble": None})):
        logs[tag] = _new_log(plain=True)
        _stubs(monkeypatch, logs[tag])
        INF.batch_sr_target_images(str(indir), str(tmp_path / tag), None, seed=71, test_label=1, labels=LABELS, samples=2, lockstep=3,
                                   consistency=True, reference_dir=str(gt), crop_border=2, **kw)
    for tag in ("with", "none"):
        assert logs[tag]["dihedral"] == [] and logs[tag]["merge"] == [] and logs[tag]["metrics"] == []
        assert len(logs[tag]["calls"]) == len(logs["without"]["calls"]) == 3                       # a a | b b | c c
        for (kind, ims, seeds, labels, keys), (kind0, ims0, seeds0, labels0, keys0) in zip(logs[tag]["calls"], logs["without"]["calls"]):
            assert (kind, seeds, labels, keys) == (kind0, seeds0, labels0, keys0) and "reference" in keys
            assert len(ims) == len(ims0) and all(np.array_equal(a, b) for a, b in zip(ims, ims0))
        assert len(logs[tag]["consistency"]) == len(logs["without"]["consistency"])
        for (o, i), (o0, i0) in zip(logs[tag]["consistency"], logs["without"]["consistency"]):
            assert all(np.array_equal(a, b) for a, b in zip(o + i, o0 + i0))
        assert sorted(os.listdir(tmp_path / tag)) == sorted(os.listdir(tmp_path / "without"))
        for name in os.listdir(tmp_path / tag):
            assert open(tmp_path / tag / name, "rb").read() == open(tmp_path / "without" / name, "rb").read(), name
    assert "metrics.json" in os.listdir(tmp_path / "with") and "consistency.json" in os.listdir(tmp_path / "with")
