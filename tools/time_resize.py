"""Time of the output resize (``srgd_amd.resize``, ``--outscale S``) on the MI355X against what a user does without it, and its cost
end to end:

    python tools/time_resize.py [--out profiles/resize_bench.txt] [--note "box / commit"] [--append] [--skip_end_to_end]

The kernels: ``--images`` (5) uniform-noise ``--size`` x ``--size`` (2048) uint8 images, resident on the GPU, to size / 2 (S = 2 of a
512 x 512 input) and to 3 size / 4 (S = 3), per filter: after ``--warmup`` untimed calls, the median of ``--repeats`` batched
``resize_flat`` calls, each between two HIP events - tables computed on the host and uploaded, scratch allocated, two launches, as
every call of the folder driver does.  Beside it Pillow's ``Image.resize`` of the same five arrays on this machine's CPU, one after
the other (median of ``--cpu_repeats`` rounds, ``time.perf_counter``): the second pass over the output folder that the flag
replaces.  Every GPU result is compared with Pillow's, byte for byte, before anything is timed.
End to end: the README's example - five 256 x 256 inputs, bf16, dim 128, 50 steps, lock-step 5, device noise - through
``batch_sr_target_images`` into PNG files, with and without ``outscale=2``, interleaved.  Nothing is gated.  Needs the MI355X."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from srgd_amd import resize as RZ                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--images", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--cpu_repeats", type=int, default=3)
    ap.add_argument("--skip_end_to_end", action="store_true")
    ap.add_argument("--ddpm_steps", type=int, default=50)
    ap.add_argument("--e2e_repeats", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_resize needs the MI355X: no GPU visible and there is no CPU path")
    device = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    n, size = args.images, args.size
    emit(f"# output resize (Pillow-exact 8-bit, srgd_amd.resize): {n} x {size}x{size} images per batched call; HIP events, median [min, max] ms "
         f"per call; Pillow {Image.__version__} Image.resize of the same {n} arrays on this machine's CPU, one after the other")
    emit(f"# command: python tools/time_resize.py {' '.join(sys.argv[1:])}")
    emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.note}")
    emit(f"# warm-up {args.warmup} calls, {args.repeats} samples; sample = one resize_flat call (host tables, upload, scratch, 2 launches) "
         f"between two events; Pillow: median of {args.cpu_repeats} rounds")
    rng = np.random.default_rng(0)
    arrays = [rng.integers(0, 256, (size, size, 3), dtype=np.uint8) for _ in range(n)]
    src_offsets = [i * 3 * size * size for i in range(n)]
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays])).to(device)
    for out_size, tag in ((size // 2, "S = 2"), (3 * size // 4, "S = 3")):
        geo = [(size, size, out_size, out_size)] * n
        dst_offsets = [i * 3 * out_size * out_size for i in range(n)]
        dst = torch.empty(n * 3 * out_size * out_size, device=device, dtype=torch.uint8)
        for name in RZ.FILTERS:
            pil = Image.Resampling(RZ.FILTERS[name])
            cpu = []
            for _ in range(args.cpu_repeats):
                t0 = time.perf_counter()
                want = [Image.fromarray(a, "RGB").resize((out_size, out_size), pil) for a in arrays]
                cpu.append(1e3 * (time.perf_counter() - t0))
            samples = []
            for k in range(args.warmup + args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                RZ.resize_flat(src, src_offsets, dst, dst_offsets, geo, name)
                b.record()
                b.synchronize()
                if k == 0:
                    got = dst.cpu().numpy().reshape(n, out_size, out_size, 3)
                    assert all(np.array_equal(got[i], np.asarray(want[i])) for i in range(n)), (name, out_size)
                if k >= args.warmup:
                    samples.append(a.elapsed_time(b))
            m, c = statistics.median(samples), statistics.median(cpu)
            moved = n * 3 * (size * size + 2 * size * out_size + out_size * out_size)
            emit(f"{n} x {size}x{size} -> {out_size}x{out_size} ({tag}), {name}: GPU {m:.3f} [{min(samples):.3f}, {max(samples):.3f}] ms per call "
                 f"({moved / 1e6:.0f} MB by definition = {moved / m / 1e9:.2f} TB/s), equal to Pillow byte for byte; Pillow on the CPU {c:.1f} "
                 f"[{min(cpu):.1f}, {max(cpu):.1f}] ms; Pillow / GPU = {c / m:.0f} x")
    try:
        from kernel_resources import kernel_table
        for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "resize.hip")):
            emit(f"# {r['name']}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS per workgroup, {r['spill']} spilled, "
                 f"{r['scratch']} B scratch per lane, occupancy {r['occupancy']} waves per SIMD")
    except Exception as err:                                 # no compiler on this machine: the table is in the CPU suite
        emit(f"# resource table not available here ({type(err).__name__})")

    if not args.skip_end_to_end:
        import bench
        from srgd_amd.inference import batch_sr_target_images
        sampler, _ = bench.build_sampler(128, device, False, 0)
        sampler.noise_source = "device"
        sampler.precision = "bf16"
        with tempfile.TemporaryDirectory() as td:
            ind = os.path.join(td, "in")
            os.makedirs(ind)
            for i in range(n):
                Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8), "RGB").save(os.path.join(ind, f"im{i:02d}.png"))
            runs = 0

            def folder(outscale):
                nonlocal runs
                runs += 1
                out = os.path.join(td, f"out{runs}")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                batch_sr_target_images(ind, out, sampler, batch_size=125, test_label=0, num_sample_steps=args.ddpm_steps, lockstep=n,
                                       outscale=outscale)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                with Image.open(os.path.join(out, "im00_out.png")) as im:
                    assert im.size == ((512, 512) if outscale else (1024, 1024))
                return dt
            folder(None), folder(2)                         # untimed
            plain, half = [], []
            for _ in range(args.e2e_repeats):
                plain.append(folder(None))
                half.append(folder(2))
            p, h = statistics.median(plain), statistics.median(half)
            emit(f"end to end, {n} x 256x256 inputs -> PNG files, bf16, dim 128, {args.ddpm_steps} steps, lock-step {n}, device noise, "
                 f"{args.e2e_repeats} interleaved pairs after one untimed pair: without --outscale {p:.3f} s "
                 f"[{min(plain):.3f}, {max(plain):.3f}] (1024x1024 files), with --outscale 2 {h:.3f} s [{min(half):.3f}, {max(half):.3f}] "
                 f"(512x512 files): {h - p:+.3f} s = {100 * (h / p - 1):+.2f} % (the resize itself, and PNG files of a quarter of the pixels)")
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
