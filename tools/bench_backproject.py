"""HIP-event timing of the back-projection kernels (srgd_image_backproject_images, include/srgd_backproject.h):

    python tools/bench_backproject.py [--out profiles/backproject_bench.txt] [--note "box / commit"]

Cases: one 1024x1024 output (input 256x256, the sampler's tile) and one 1920x1280 output (input 480x320, BSD100-shaped), each alone
and as a group of 20 in one batched call, for N = 1, 3 and 10 iterations, out of place.  Every figure is the median over --repeats
(>= 20) samples, each sample one call between two HIP events, after --warmup untimed calls of the same shape; buffers and scratch are
allocated outside the timed window.  Beside the time per call and per iteration the file gives the bytes the kernels must move by
definition - begin reads out01 and cond01 (2 x 192 hw) and writes O and C (2 x 48 hw); every iteration's reduce kernel reads O (48 hw)
and writes D (3 hw), its update kernel reads O, C and D (99 hw) and writes O (48 hw); end reads O and out01 (240 hw) and writes dst01
(192 hw) - and the rates they imply: of a whole call, and of one further iteration (the slope between N = 1 and N = 10) against the
198 hw bytes it moves, both against the 8 TB/s HBM rate.  The file also records the kernels' registers, LDS bytes and scratch from the
compiler's resource table (tools/kernel_resources.py) and the share of the sampling time of a 1024x1024 tile (--tile_ms, README: 711 ms
in bf16).  Nothing is gated.  Needs the MI355X; there is no CPU path."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from srgd_amd import backproject as BP                      # noqa: E402

HBM_TBS = 8.0
FIXED_BYTES, ITERATION_BYTES = 2 * 192 + 2 * 48 + 240 + 192, 48 + 3 + 99 + 48      # per LR pixel: begin + end; reduce + update


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b))
    return statistics.median(samples), min(samples), max(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backproject_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--tile_ms", type=float, default=711.0, help="sampling time of one 1024x1024 tile (README: 711 ms in bf16)")
    args = ap.parse_args()
    if args.repeats < 20:
        raise SystemExit("bench_backproject: --repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_backproject needs the MI355X: no GPU visible and there is no CPU path")
    L = BP.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# iterative back-projection (O <- clip(O + C - enlarge(reduce(O))), N times, Pillow-exact 8-bit): HIP kernels, HIP events, "
         "median [min, max] ms per call")
    emit(f"# command: python tools/bench_backproject.py {' '.join(sys.argv[1:])}")
    emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.note}")
    emit(f"# warm-up {args.warmup} calls per shape, {args.repeats} samples; sample = one call (2 + 2 N launches) between two events")
    emit(f"# bytes by definition per LR pixel: begin + end {FIXED_BYTES}, one iteration {ITERATION_BYTES} (reduce 51, update 147)")
    try:
        from kernel_resources import kernel_table
        for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "backproject.hip")):
            if "backproject_" in r["name"]:
                emit(f"# {r['name']}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS per workgroup, {r['spill']} spilled, "
                     f"{r['scratch']} B scratch per lane, occupancy {r['occupancy']} waves per SIMD")
    except Exception as err:                                 # no compiler on this machine: the table is in the CPU suite
        emit(f"# resource table not available here ({type(err).__name__})")
    tile_n3 = None
    for name, n, h, w in (("1 x 1024x1024", 1, 256, 256), ("20 x 1024x1024 (one batched call)", 20, 256, 256),
                          ("1 x 1920x1280", 1, 320, 480), ("20 x 1920x1280 (one batched call)", 20, 320, 480)):
        e = 48 * h * w
        out = torch.rand(n * e, generator=g, device="cuda", dtype=torch.float32)
        cond = torch.rand(n * e, generator=g, device="cuda", dtype=torch.float32)
        dst = torch.empty(n * e, device="cuda", dtype=torch.float32)
        scratch = torch.empty(BP.scratch_bytes([(h, w)] * n), device="cuda", dtype=torch.uint8)
        offs = (C.c_int64 * n)(*[i * e for i in range(n)])
        hw = (C.c_int32 * (2 * n))(*([h, w] * n))
        med = {}
        for iters in (1, 3, 10):
            def kernels():
                rc = L.srgd_image_backproject_images(p(out), p(cond), offs, hw, n, iters, p(dst), p(scratch), st)
                assert rc == 0, L.srgd_image_backproject_last_error()
            tk = timed(kernels, args.warmup, args.repeats)
            med[iters] = tk[0]
            nbytes = n * h * w * (FIXED_BYTES + iters * ITERATION_BYTES)
            rate = nbytes / tk[0] / 1e9
            emit(f"{name}, N = {iters}: {tk[0]:.3f} [{tk[1]:.3f}, {tk[2]:.3f}] ms per call = {tk[0] / iters:.3f} ms per iteration of the "
                 f"call; {nbytes / 1e6:.0f} MB by definition = {rate:.2f} TB/s ({100 * rate / HBM_TBS:.0f} % of the {HBM_TBS:.0f} TB/s HBM rate)")
        slope = (med[10] - med[1]) / 9
        it_bytes = n * h * w * ITERATION_BYTES
        fixed = med[1] - slope
        emit(f"  one further iteration (slope N = 1 .. 10): {slope:.4f} ms for {it_bytes / 1e6:.1f} MB = {it_bytes / slope / 1e9:.2f} TB/s; "
             f"begin + end: {fixed:.4f} ms for {n * h * w * FIXED_BYTES / 1e6:.1f} MB = {n * h * w * FIXED_BYTES / fixed / 1e9:.2f} TB/s")
        if (n, h, w) == (1, 256, 256):
            tile_n3 = med[3]
        del out, cond, dst, scratch
        torch.cuda.empty_cache()
    emit(f"# share of the sampling time: --back_project 3 on one 1024x1024 tile costs {tile_n3:.3f} ms beside {args.tile_ms:.0f} ms of "
         f"sampling = {100 * tile_n3 / args.tile_ms:.3f} %")
    emit("# note: every sample re-reads the same buffers back to back; a single image's buffers (about 40 / 90 MB) fit the 256 MB "
         "Infinity Cache, so its rates are not HBM rates, and its time is mostly that of 2 + 2 N launches; the groups' buffers (0.8 / "
         "1.8 GB) do not fit")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
