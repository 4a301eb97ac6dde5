"""HIP-event timing of the LR-consistency kernels (srgd_image_consistency_images) against the same definition through Pillow on the
host - ``Image.resize((w, h), BICUBIC)`` and int64 numpy, what a user would otherwise run on the saved PNGs:

    python tools/bench_consistency.py [--out profiles/consistency_bench.txt] [--note "box / commit"]

Cases: a group of 20 BSD100-shaped x4 outputs (1920x1280, inputs 480x320) in one batched call, and one 8192^2 output (input 2048^2),
each with and without the reduced output D stored.  Every kernel figure is the median over --repeats samples, each sample `inner`
back-to-back calls between two HIP events, after --warmup untimed calls of the same shape; buffers and scratch are allocated outside
the timed window, and the copy of the integers to the host is not timed.  The rate is the HR bytes of the outputs (48 hw per image,
each read once by definition; the kernel's tiles read 1.40 x that through their halos, mostly from cache) over the kernels' time,
against the 8 TB/s HBM rate.  The Pillow side is wall-clock time on the host for the same images, arrays already in memory (no PNG
decoding).  The file also records the kernels' registers, LDS bytes and scratch from the compiler's resource table
(tools/kernel_resources.py) and whether the two sides agree, and the two open expectations of DESIGN.md section 5: the share of a
group's sampling time, and whether the kernel is bound by LDS and integer work rather than HBM.  Nothing is gated.  Needs the MI355X;
there is no CPU path."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from srgd_amd import consistency as CS                      # noqa: E402

HBM_TBS = 8.0


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


def pillow_consistency(out, lr):
    """The definition on the host: uint8 [4h,4w,3], [h,w,3] numpy -> (D, [sse_r, sse_g, sse_b, max_abs])."""
    h, w, _ = lr.shape
    down = np.asarray(Image.fromarray(out, "RGB").resize((w, h), Image.BICUBIC))
    e = down.astype(np.int64) - lr.astype(np.int64)
    return down, [int(v) for v in (e * e).sum(axis=(0, 1))] + [int(np.abs(e).max())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip_8192", action="store_true")
    ap.add_argument("--sampling_s", type=float, default=None,
                    help="seconds the group of 20 takes to sample (from a CLI run of the same commit): the kernels' share is reported")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency needs the MI355X: no GPU visible and there is no CPU path")
    L = CS.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# LR consistency (x4 Pillow-bicubic reduction of the output, sse per channel and max |e| against the input): HIP kernels "
         "(HIP events, median [min, max] ms per call) against Pillow + numpy on the host (wall clock)")
    emit(f"# command: python tools/bench_consistency.py {' '.join(sys.argv[1:])}")
    emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; Pillow {Image.__version__}; {args.note}")
    emit(f"# warm-up {args.warmup} calls per shape, {args.repeats} samples; sample = `inner` back-to-back calls between two events")
    try:
        from kernel_resources import kernel_table
        for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "consistency.hip")):
            if "consistency_" in r["name"]:
                emit(f"# {r['name']}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS per workgroup, {r['spill']} spilled, "
                     f"{r['scratch']} B scratch per lane, occupancy {r['occupancy']} waves per SIMD")
    except Exception as err:                                 # no compiler on this machine: the table is in the CPU suite
        emit(f"# resource table not available here ({type(err).__name__})")
    cases = [("20 x 1280x1920 (one batched call)", 20, 320, 480, 5)] + ([] if args.skip_8192 else [("1 x 8192x8192", 1, 2048, 2048, 2)])
    group_ms = None
    for name, n, h, w, inner in cases:
        e = 3 * h * w                                        # a multiple of 16 for both shapes: no padding
        assert e % CS.VEC == 0
        hr = torch.randint(0, 256, (n * 16 * e,), generator=g, device="cuda", dtype=torch.uint8)
        lr = torch.randint(0, 256, (n * e,), generator=g, device="cuda", dtype=torch.uint8)
        h_offs = (C.c_int64 * n)(*[i * 16 * e for i in range(n)])
        l_offs = (C.c_int64 * n)(*[i * e for i in range(n)])
        hw = (C.c_int32 * (2 * n))(*([h, w] * n))
        down = torch.empty(n * e, device="cuda", dtype=torch.uint8)
        stats = torch.empty(n, 4, device="cuda", dtype=torch.int64)
        scratch = torch.empty(CS.scratch_bytes([(h, w)] * n) // 8, device="cuda", dtype=torch.int64)
        hr_host = hr.cpu().numpy().reshape(n, 4 * h, 4 * w, 3)
        lr_host = lr.cpu().numpy().reshape(n, h, w, 3)
        t0 = time.perf_counter()
        host = [pillow_consistency(hr_host[i], lr_host[i]) for i in range(n)]
        host_ms = (time.perf_counter() - t0) * 1e3
        for with_down in (False, True):
            def kernels():
                rc = L.srgd_image_consistency_images(p(hr), h_offs, p(lr), l_offs, hw, n, p(down) if with_down else None,
                                                     l_offs if with_down else None, p(stats), p(scratch), st)
                assert rc == 0, L.srgd_image_consistency_last_error()
            tk = timed(kernels, args.warmup, args.repeats, inner)
            got = stats.cpu().tolist()
            agree = all(got[i] == host[i][1] for i in range(n))
            if with_down:
                got_down = down.cpu().numpy().reshape(n, h, w, 3)
                agree = agree and all(np.array_equal(got_down[i], host[i][0]) for i in range(n))
            nbytes = n * 16 * e
            rate = nbytes / tk[0] / 1e9
            emit(f"{name}, {'with' if with_down else 'without'} D stored: kernels {tk[0]:.3f} [{tk[1]:.3f}, {tk[2]:.3f}] ms = "
                 f"{rate:.2f} TB/s of {nbytes / 1e6:.0f} MB HR bytes ({100 * rate / HBM_TBS:.0f} % of the {HBM_TBS:.0f} TB/s HBM rate); "
                 f"Pillow on the host {host_ms:.0f} ms; ratio x{host_ms / tk[0]:.0f}; results {'agree' if agree else 'DISAGREE'}")
            if n > 1 and not with_down:
                group_ms = tk[0]
        emit(f"  image 0: sse {got[0][:3]}, max_abs {got[0][3]}, lr_psnr {CS.record(*got[0], h, w)['lr_psnr']:.6f} dB")
        del hr, lr, down, stats, scratch
        torch.cuda.empty_cache()
    emit("# expectation 1 (not a gate): the numbers of a group cost far below 1 % of its sampling time - "
         + (f"{group_ms:.3f} ms of {args.sampling_s:.1f} s = {100 * group_ms / 1e3 / args.sampling_s:.4f} %" if args.sampling_s and group_ms
            else "pass --sampling_s with the group's sampling time of a CLI run to fill this in"))
    emit("# expectation 2 (not a gate): the kernel is bound by LDS and integer work rather than HBM - holds where the rate above stays "
         f"well below the {HBM_TBS:.0f} TB/s HBM rate while the kernel reads each HR byte 1.40 x")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
