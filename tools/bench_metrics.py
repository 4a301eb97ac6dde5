"""HIP-event timing of the metrics kernels (srgd_image_metrics_images) against the same definition written in torch, float64, on the
same GPU (quantisation, BT.601 luma, two separable 11-tap F.conv2d passes over the five quantities, means):

    python tools/bench_metrics.py [--out profiles/metrics_bench.txt] [--note "box / commit"]

Cases: a group of 20 BSD100-shaped x4 outputs (1920x1280) in one batched call, and one 8192^2 output, crop 4.  Every figure is the
median over --repeats samples, each sample `inner` back-to-back calls between two HIP events, after --warmup untimed calls of the same
shape; results and scratch are allocated outside the timed window, and the copy of the numbers to the host is not timed.  The
file also records the kernels' registers, LDS bytes and scratch from the compiler's resource table (tools/kernel_resources.py) and
both results, so that a disagreement between the two sides would show.  Nothing is gated.  Needs the MI355X; there is no CPU path."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from srgd_amd import metrics as MX                          # noqa: E402
from srgd_amd.metrics import scratch_doubles                # noqa: E402


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


def torch_metrics(out01, ref_u8, crop):
    """The definition in torch on the device: [3,h,w] fp32, [h,w,3] uint8 -> [3] float64 (psnr_y, psnr_rgb, ssim_y)."""
    h, w = out01.shape[1:]
    q = (out01 * 255.0).to(torch.int32)[:, crop:h - crop, crop:w - crop].double()
    r = ref_u8.permute(2, 0, 1)[:, crop:h - crop, crop:w - crop].double()
    coef = torch.tensor([65.481, 128.553, 24.966], dtype=torch.float64, device=out01.device).view(3, 1, 1)
    yo, yr = (coef * (q / 255.0)).sum(0) + 16.0, (coef * (r / 255.0)).sum(0) + 16.0
    psnr = lambda a, b: 10.0 * torch.log10(255.0 ** 2 / ((a - b) ** 2).mean())          # noqa: E731
    g = torch.exp(-((torch.arange(11, dtype=torch.float64, device=out01.device) - 5.0) ** 2) / 4.5)
    g = g / g.sum()
    five = torch.stack([yo, yr, yo * yo, yr * yr, yo * yr])[:, None]
    f = F.conv2d(F.conv2d(five, g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1))[:, 0]
    mx, my = f[0], f[1]
    sxx, syy, sxy = f[2] - mx * mx, f[3] - my * my, f[4] - mx * my
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    ssim = (((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))).mean()
    return torch.stack([psnr(yo, yr), psnr(q, r), ssim])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip_8192", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs the MI355X: no GPU visible and there is no CPU path")
    L = MX.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# metrics (Y-PSNR, RGB-PSNR, Y-SSIM, crop 4): HIP kernels against the same definition in torch (float64, same GPU), HIP events, "
         "median [min, max] ms per call")
    emit(f"# command: python tools/bench_metrics.py {' '.join(sys.argv[1:])}")
    emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.note}")
    emit(f"# warm-up {args.warmup} calls per shape, {args.repeats} samples; sample = `inner` back-to-back calls between two events")
    try:
        from kernel_resources import kernel_table
        for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "metrics.hip")):
            if "metrics_" in r["name"]:
                emit(f"# {r['name']}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS per workgroup, {r['spill']} spilled, "
                     f"{r['scratch']} B scratch per lane, occupancy {r['occupancy']} waves per SIMD")
    except Exception as err:                                 # no compiler on this machine: the table is in the CPU suite
        emit(f"# resource table not available here ({type(err).__name__})")
    cases = [("20 x 1280x1920 (one batched call)", 20, 1280, 1920, 5)] + ([] if args.skip_8192 else [("1 x 8192x8192", 1, 8192, 8192, 2)])
    for name, n, h, w, inner in cases:
        crop = 4
        out = torch.rand(n * 3 * h * w, generator=g, device="cuda")
        ref = torch.randint(0, 256, (n * h * w * 3,), generator=g, device="cuda", dtype=torch.uint8)
        offs = (C.c_int64 * n)(*[i * 3 * h * w for i in range(n)])
        hw = (C.c_int32 * (2 * n))(*([h, w] * n))
        res = torch.empty(n, 4, device="cuda", dtype=torch.float64)
        scratch = torch.empty(scratch_doubles([(h, w)] * n, crop), device="cuda", dtype=torch.float64)

        def kernels():
            rc = L.srgd_image_metrics_images(p(out), p(ref), offs, offs, hw, n, crop, p(res), p(scratch), st)
            assert rc == 0, L.srgd_image_metrics_last_error()

        def restatement():
            return [torch_metrics(out[i * 3 * h * w:(i + 1) * 3 * h * w].view(3, h, w), ref[i * 3 * h * w:(i + 1) * 3 * h * w].view(h, w, 3),
                                  crop) for i in range(n)]
        k = timed(kernels, args.warmup, args.repeats, inner)
        t = timed(restatement, 1, max(3, args.repeats // 2), 1)
        want = torch.stack(restatement()).cpu()
        got = res[:, :3].cpu()
        emit(f"{name}: kernels {k[0]:.3f} [{k[1]:.3f}, {k[2]:.3f}] ms; torch float64 {t[0]:.3f} [{t[1]:.3f}, {t[2]:.3f}] ms; "
             f"ratio x{t[0] / k[0]:.1f}; max |kernels - torch| = {float((got - want).abs().max()):.2e}")
        emit(f"  image 0: psnr_y {float(got[0, 0]):.6f} dB, psnr_rgb {float(got[0, 1]):.6f} dB, ssim_y {float(got[0, 2]):.9f}")
        del out, ref, res, scratch
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
