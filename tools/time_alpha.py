"""Time of what ``--alpha keep`` adds (``srgd_amd.alpha``) on the MI355X against the same composition in Pillow on the CPU:

    python tools/time_alpha.py [--out profiles/alpha_bench.txt] [--note "box / commit"] [--append]

Attach: ``--images`` (5) RGB outputs of ``--size`` x ``--size`` (2048) pixels, resident on the GPU, and the ``size / 4`` planes of
their inputs -> RGBA: the planes x4 with bicubic, then the pack.  After ``--warmup`` untimed calls, the median of ``--repeats``
``attach_alpha_on_device`` calls, each between two HIP events - tables computed on the host and uploaded, buffers allocated, three
launches, as every ``flush()`` of the folder driver does.  The pack kernel alone (``pack_rgba_flat`` on resident flat buffers) is
timed the same way and its bytes per second - 8 bytes moved per pixel: 3 + 1 read, 4 written - are printed beside the HBM figure of
the box (``--hbm_tbs``, 8 TB/s by specification).  Beside them Pillow on this machine's CPU: ``Image.resize`` of the five planes and
``Image.merge``, one after the other.  Bleed: N = ``--bleed`` (8) passes on five ``size / 4`` RGBA images in one ``bleed_on_device``
call (N + 1 launches).  Every GPU result is compared with Pillow's or with the numpy restatement, byte for byte, before anything is
timed.  Nothing is gated.  Needs the MI355X."""
import argparse
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

from srgd_amd import alpha as AL                            # noqa: E402
from tests import alpha_cases as AC                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alpha_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--images", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--bleed", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--cpu_repeats", type=int, default=3)
    ap.add_argument("--hbm_tbs", type=float, default=8.0, help="the box's HBM bandwidth in TB/s, printed beside the pack's rate")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_alpha needs the MI355X: no GPU visible and there is no CPU path")
    device = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(call):
        samples = []
        for k in range(args.warmup + args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if k >= args.warmup:
                samples.append(a.elapsed_time(b))
        return statistics.median(samples), min(samples), max(samples)

    n, size, low = args.images, args.size, args.size // 4
    emit(f"# alpha (srgd_amd.alpha): {n} x {size}x{size} RGB outputs + {low}x{low} planes -> RGBA per batched call; HIP events, median "
         f"[min, max] ms per call; Pillow {Image.__version__} on this machine's CPU, one image after the other")
    emit(f"# command: python tools/time_alpha.py {' '.join(sys.argv[1:])}")
    emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.note}")
    emit(f"# warm-up {args.warmup} calls, {args.repeats} samples; Pillow: median of {args.cpu_repeats} rounds")
    rng = np.random.default_rng(0)
    rgbs = [rng.integers(0, 256, (size, size, 3), dtype=np.uint8) for _ in range(n)]
    planes = [rng.integers(0, 256, (low, low), dtype=np.uint8) for _ in range(n)]
    cpu = []
    for _ in range(args.cpu_repeats):
        t0 = time.perf_counter()
        want = [Image.merge("RGBA", (*Image.fromarray(c, "RGB").split(), Image.fromarray(p, "L").resize((size, size), Image.Resampling.BICUBIC)))
                for c, p in zip(rgbs, planes)]
        cpu.append(1e3 * (time.perf_counter() - t0))
    d_rgbs = [torch.from_numpy(c).to(device) for c in rgbs]
    d_planes = [torch.from_numpy(p).to(device) for p in planes]
    got = AL.attach_alpha_on_device(d_rgbs, d_planes)
    assert all(np.array_equal(g.cpu().numpy(), np.asarray(w)) for g, w in zip(got, want))
    m, lo, hi = timed(lambda: AL.attach_alpha_on_device(d_rgbs, d_planes))
    c = statistics.median(cpu)
    emit(f"attach, {n} x ({low}x{low} plane -> x4 bicubic -> pack with {size}x{size} RGB): GPU {m:.3f} [{lo:.3f}, {hi:.3f}] ms per call (host "
         f"tables, upload, buffers, copies into flat buffers, 3 launches), equal to Pillow byte for byte; Pillow resize + merge on the CPU "
         f"{c:.1f} [{min(cpu):.1f}, {max(cpu):.1f}] ms; Pillow / GPU = {c / m:.0f} x")
    pixels = size * size
    offs = lambda k: [i * k * pixels for i in range(n)]    # noqa: E731
    rgb = torch.cat([t.reshape(-1) for t in d_rgbs])
    alpha = torch.cat([g[:, :, 3].reshape(-1) for g in got])
    rgba = torch.empty(4 * n * pixels, device=device, dtype=torch.uint8)
    AL.pack_rgba_flat(rgb, offs(3), alpha, offs(1), rgba, offs(4), [(size, size)] * n)
    assert all(np.array_equal(rgba[4 * i * pixels:4 * (i + 1) * pixels].view(size, size, 4).cpu().numpy(), np.asarray(w)) for i, w in enumerate(want))
    m, lo, hi = timed(lambda: AL.pack_rgba_flat(rgb, offs(3), alpha, offs(1), rgba, offs(4), [(size, size)] * n))
    moved = 8 * n * pixels
    emit(f"pack alone, {n} x {size}x{size} on resident flat buffers: {m:.3f} [{lo:.3f}, {hi:.3f}] ms per call, {moved / 1e6:.0f} MB by "
         f"definition (3 + 1 bytes read, 4 written per pixel) = {moved / m / 1e9:.2f} TB/s; HBM of the box: {args.hbm_tbs:g} TB/s "
         f"({100 * moved / m / 1e9 / args.hbm_tbs:.0f} %); the {moved / 1e6:.0f} MB fit the Infinity Cache")
    rgbas = [np.dstack([rng.integers(0, 256, (low, low, 3), dtype=np.uint8), np.where(rng.random((low, low)) < 0.7, 0, 255).astype(np.uint8)])
             for _ in range(n)]
    d_rgbas = [torch.from_numpy(x).to(device) for x in rgbas]
    t0 = time.perf_counter()
    want = [AC.bleed(x, args.bleed) for x in rgbas]
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    got = AL.bleed_on_device(d_rgbas, args.bleed)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    m, lo, hi = timed(lambda: AL.bleed_on_device(d_rgbas, args.bleed))
    emit(f"bleed, N = {args.bleed}, {n} x {low}x{low} RGBA images, about 70 % transparent: GPU {m:.3f} [{lo:.3f}, {hi:.3f}] ms per call "
         f"({args.bleed + 1} launches), equal to the numpy restatement byte for byte (which took {numpy_ms:.0f} ms on this machine's CPU)")
    try:
        from kernel_resources import kernel_table
        for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "alpha.hip")):
            emit(f"# {r['name']}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS per workgroup, {r['spill']} spilled, "
                 f"{r['scratch']} B scratch per lane, occupancy {r['occupancy']} waves per SIMD")
    except Exception as err:                                 # no compiler on this machine: the table is in the CPU suite
        emit(f"# resource table not available here ({type(err).__name__})")
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
