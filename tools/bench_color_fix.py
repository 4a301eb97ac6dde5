"""HIP-event timing of the colour-fix kernels (srgd_image_color_fix / srgd_image_color_fix_images) against the PyTorch restatement
of tests/color_fix_cases.py run in fp32 on the same GPU (F.conv2d depthwise dilated on a replicate-padded image; var):

    python tools/bench_color_fix.py [--out profiles/color_fix_bench.txt] [--note "box / commit"]

Cases, both modes each: one 1024^2 image, one 8192^2 image, and a group of 20 BSD100-shaped x4 outputs (480x320 / 320x480) through the
batched entry against 20 single-image calls.  Every figure is the median over --repeats samples, each sample `inner` back-to-back
calls between two HIP events (so that a sample lasts milliseconds, not one launch), after --warmup untimed calls of the same
shape; scratch and results are allocated outside the timed window.  Gates (exit code 1 when missed): each mode faster than the
restatement on every case, and the 1024^2 case at most 7.1 ms (1 % of the 711 ms the README gives for sampling that image).  The
group's gain over single calls is recorded, not gated.  Needs the MI355X; there is no CPU path."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srgd_amd import _lib                                   # noqa: E402
from srgd_amd.colorfix import MODES, scratch_elements      # noqa: E402
from tests import color_fix_cases as K                      # noqa: E402

BUDGET_1024_MS = 7.1


def timed(fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b) / inner)
    return statistics.median(samples), min(samples), max(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_fix_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--skip_8192", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_color_fix needs the MI355X: no GPU visible and there is no CPU path")
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    lines, ok = [], True

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# colour fix: HIP kernels against the PyTorch restatement (fp32, same GPU), HIP events, median [min, max] ms per call")
    emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.note}")
    emit(f"# warm-up {args.warmup} calls per shape, {args.repeats} samples; sample = `inner` back-to-back calls between two events")
    singles = [("1024x1024", 1024, 1024, 20, 5)] + ([] if args.skip_8192 else [("8192x8192", 8192, 8192, 3, 1)])
    for name, h, w, inner, ref_inner in singles:
        c = torch.rand(3, h, w, device="cuda", generator=g)
        for mode in ("wavelet", "adain"):
            s = torch.rand(3, h, w, device="cuda", generator=g)
            if mode == "adain":
                s = 0.25 + 0.5 * s
            dst = torch.empty_like(c)
            scratch = torch.empty(scratch_elements(mode, [0], [(h, w)]), device="cuda")

            def ours():
                assert L.srgd_image_color_fix(p(c), p(s), h, w, MODES[mode], p(dst), p(scratch), st) == 0, L.srgd_last_error()

            def ref():
                return K.literal(mode, c, s, torch.float32).clamp(0, 1)
            t_ours = timed(ours, args.warmup, args.repeats, inner)
            t_ref = timed(ref, max(1, args.warmup - 1), max(3, args.repeats // 3), ref_inner)
            diff = float((dst - ref()).abs().max())
            passes = 10 if mode == "wavelet" else 3
            traffic = (20 if mode == "wavelet" else 4) * 3 * h * w * 4           # wavelet: ten passes read + write; adain: c twice, s once, dst once
            emit(f"{name:10s} {mode:8s} kernels {t_ours[0]:9.4f} [{t_ours[1]:.4f}, {t_ours[2]:.4f}] ms ({passes} launches, "
                 f"{traffic / t_ours[0] / 1e9:.2f} TB/s of algorithmic traffic)   restatement {t_ref[0]:9.3f} [{t_ref[1]:.3f}, {t_ref[2]:.3f}] ms"
                 f"   x{t_ref[0] / t_ours[0]:.1f}   max|kernels - restatement(fp32)| = {diff:.2e}")
            if t_ours[0] >= t_ref[0]:
                ok = False
                emit(f"# GATE MISSED: {name} {mode} is not faster than the restatement")
            if h == 1024 and t_ours[0] > BUDGET_1024_MS:
                ok = False
                emit(f"# GATE MISSED: {name} {mode} costs more than {BUDGET_1024_MS} ms")
            del s, dst, scratch
        del c
    torch.cuda.empty_cache()
    # 20 BSD100-shaped x4 outputs in the flat per-image layout of a mixed lock-step run
    sizes = [(480, 320), (320, 480)] * 10
    offsets, total = [], 0
    for (h, w) in sizes:
        offsets.append(total)
        total += 3 * h * w
    n = len(sizes)
    offs = (C.c_int64 * n)(*offsets)
    hw = (C.c_int32 * (2 * n))(*[v for sz in sizes for v in sz])
    c = torch.rand(total, device="cuda", generator=g)
    for mode in ("wavelet", "adain"):
        s = torch.rand(total, device="cuda", generator=g)
        if mode == "adain":
            s = 0.25 + 0.5 * s
        dst, dst1 = torch.empty_like(c), torch.empty_like(c)
        scratch = torch.empty(scratch_elements(mode, offsets, sizes), device="cuda")

        def batched():
            assert L.srgd_image_color_fix_images(p(c), p(s), offs, hw, n, MODES[mode], p(dst), p(scratch), st) == 0, L.srgd_last_error()

        def one_by_one():
            for o, (h, w) in zip(offsets, sizes):
                e = c.element_size() * o
                assert L.srgd_image_color_fix(C.c_void_p(c.data_ptr() + e), C.c_void_p(s.data_ptr() + e), h, w, MODES[mode],
                                              C.c_void_p(dst1.data_ptr() + e), p(scratch), st) == 0, L.srgd_last_error()

        def ref():
            return [K.literal(mode, c[o:o + 3 * h * w].view(3, h, w), s[o:o + 3 * h * w].view(3, h, w), torch.float32).clamp(0, 1)
                    for o, (h, w) in zip(offsets, sizes)]
        t_b = timed(batched, args.warmup, args.repeats, 10)
        t_1 = timed(one_by_one, args.warmup, args.repeats, 10)
        t_ref = timed(ref, max(1, args.warmup - 1), max(3, args.repeats // 3), 1)
        torch.cuda.synchronize()
        same = torch.equal(dst, dst1)
        emit(f"{'20xBSD100':10s} {mode:8s} batched {t_b[0]:9.4f} [{t_b[1]:.4f}, {t_b[2]:.4f}] ms   20 single calls {t_1[0]:9.4f} "
             f"[{t_1[1]:.4f}, {t_1[2]:.4f}] ms   gain x{t_1[0] / t_b[0]:.2f} (recorded, not gated)   restatement {t_ref[0]:9.3f} "
             f"[{t_ref[1]:.3f}, {t_ref[2]:.3f}] ms   x{t_ref[0] / t_b[0]:.1f}   batched == single calls bit for bit: {same}")
        if t_b[0] >= t_ref[0] or not same:
            ok = False
            emit(f"# GATE MISSED: 20xBSD100 {mode}")
    emit(f"# gates: every mode faster than the restatement, 1024x1024 <= {BUDGET_1024_MS} ms: {'met' if ok else 'MISSED'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
