"""The f16x1 precision (SRGD_PRECISION_F16X1: f16x3 with the halo-kernel 3x3 convolutions contracting the f16 hi halves alone - one
MFMA per product) without a GPU: its public surface, the compiled one-term instances of conv3x3_split_kernel (registers, MFMA and
LDS-DMA counts against their three-term siblings, the hazard lint), and the emulation the GPU tests measure the kernel against."""
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from oracle.split_emulation import halves, split_conv2d, weight_scale
from tests.test_asm_hazards_cpu import CSRC, FLAGS, _kernels, _lint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(CSRC, "conv3x3_split.hip")
# (B, C0, C1, Cout, H, W): one chunk; two sources with the seam at a chunk boundary and two n-tiles; four chunks (both A buffers and
# the steady-state ring); twelve chunks
SHAPES = [(2, 32, 0, 128, 8, 32), (1, 64, 32, 256, 16, 64), (3, 128, 0, 128, 32, 32), (1, 256, 128, 128, 8, 32)]


def seed11_inputs(cfg):
    """the inputs of tests/test_split_gpu.py::test_conv3x3_split_borders_sources_stats"""
    B, c0, c1, cout, H, W = cfg
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(B, c0, H, W, generator=g)
    x1 = torch.randn(B, c1, H, W, generator=g) if c1 else None
    w = torch.randn(cout, c0 + c1, 3, 3, generator=g) / (3 * (c0 + c1) ** 0.5)
    b = torch.randn(cout, generator=g)
    return x0, x1, w, b


def emu1(x, w, b, dtype=torch.float32):
    """The mode's definition: conv(hi(x), hi(w s)) / s + bias, accumulated in `dtype`."""
    s = weight_scale(w, "f16")
    y = F.conv2d(halves(x, "f16")[0].to(dtype), halves(w * s, "f16")[0].to(dtype), None, padding=1) * (1.0 / s)
    return y if b is None else y + b.to(dtype).view(1, -1, 1, 1)


def test_surface():
    from srgd_amd import _lib, build, engine
    from srgd_amd.inference import parse_args
    a = parse_args(["-c", "x", "-m", "w", "--input_dir", "i", "--output_dir", "o", "--precision", "f16x1"])
    assert a.precision == "f16x1"
    assert engine._PRECISIONS["f16x1"] == _lib.PRECISION_F16X1 == 7
    with open(os.path.join(ROOT, "include", "srgd_hip.h")) as f:
        assert re.search(r"^#define SRGD_PRECISION_F16X1 7\b", f.read(), re.M)
    assert len(_lib.PROTOTYPES) == 58
    assert len(build.LIBRARIES) == 11


def _is_one_term(name):
    return re.search(r"conv3x3_split_kernel<(true|false), true, (true|false), 1>", name)


def test_one_term_instances_fit_their_register_budget():
    from tools.kernel_resources import kernel_table
    rows = [r for r in kernel_table(SRC) if _is_one_term(r["name"])]
    assert len(rows) == 4, [r["name"] for r in rows]           # STATS on / off x GNIN on / off
    for r in rows:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        # __launch_bounds__(512, 2): one 512-thread workgroup per CU = two waves per SIMD, 512 / 2 registers each
        assert r["vgpr"] + max(r["agpr"], 0) <= 512 // 2, r


@pytest.fixture(scope="module")
def split_kernels(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path_factory.mktemp("f16x1") / "k.s"
    r = subprocess.run([hipcc, *FLAGS, SRC, "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = _kernels(out.read_text())
    names = subprocess.run(["c++filt"], input="\n".join(kernels), capture_output=True, text=True).stdout.splitlines()
    return {n.replace("srgd::(anonymous namespace)::", ""): ins for n, ins in zip(names, kernels.values())}


def _k_loop(ins):
    """the instructions of the loop that carries the MFMAs: from a label to the backward branch to it (the GNIN instances close
    their loop with an unconditional s_branch and leave it from the middle)"""
    labels = {i[:-1]: n for n, i in enumerate(ins) if i.endswith(":")}
    loops = []
    for n, i in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\S+)", i)
        if m and m.group(1) in labels and labels[m.group(1)] < n:
            body = ins[labels[m.group(1)]:n]
            if sum(b.startswith("v_mfma") for b in body) >= 16:
                loops.append(body)
    assert len(loops) == 1, len(loops)
    return loops[0]


def test_one_term_instances_issue_a_third_of_the_mfmas_and_half_the_weight_copies(split_kernels):
    ones = [n for n in split_kernels if _is_one_term(n)]
    assert len(ones) == 4, list(split_kernels)
    for name in ones:
        sib = next(n for n in split_kernels if n.startswith(name.split("(")[0].replace(", 1>", ", 3>")))
        mf = lambda ins: sum(i.startswith("v_mfma_f32_16x16x32_f16") for i in ins)
        dma = lambda ins: sum(1 for i in ins if i.startswith("buffer_load") and re.search(r"\blds\b", i))
        one, three = split_kernels[name], split_kernels[sib]
        assert mf(three) % 3 == 0 and mf(one) * 3 == mf(three) and mf(one) > 0, (name, mf(one), mf(three))
        assert mf(_k_loop(one)) * 3 == mf(_k_loop(three))
        assert dma(_k_loop(one)) * 2 == dma(_k_loop(three)) and dma(_k_loop(one)) > 0, (name, dma(_k_loop(one)), dma(_k_loop(three)))
        assert _lint(one) == [], (name, _lint(one)[:3])


@pytest.mark.parametrize("cfg", SHAPES, ids=lambda s: "B%d_C%d+%d_Cout%d_%dx%d" % s)
def test_the_yardstick_is_sharp_enough(cfg):
    # the GPU test holds the kernel to 4e-6 * scale of emu1 and demands 10 x that from the three-term arithmetic: emu1 itself must
    # carry less fp32 summation noise than half that bound, and the two arithmetics must differ by far more than it
    x0, x1, w, b = seed11_inputs(cfg)
    x = x0 if x1 is None else torch.cat((x0, x1), 1)
    e1 = emu1(x, w, b)
    scale = max(1.0, float(F.conv2d(x.double(), w.double(), b.double(), padding=1).abs().max()))
    noise = float((e1.double() - emu1(x, w, b, torch.float64)).abs().max())
    gap = float((e1 - split_conv2d(x, w, b, padding=1, terms=3)).abs().max())
    assert noise <= 2e-6 * scale, (noise, scale)
    assert gap >= 40 * 4e-6 * scale, (gap, scale)
