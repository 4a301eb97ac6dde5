"""Wall-clock cost of LR-consistency guidance (``tiled_sample(consistency_guidance=...)``) on the benchmark's headline configuration:

    python tools/time_guidance.py [--out profiles/guidance_bench.txt] [--note "box / commit"] [--append]

bf16, dim 128, ``--images`` (5) 1024x1024 outputs in lock-step, ``--ddpm_steps`` (50) steps, device noise - what ``bench.py`` times -
with a weight of 1 against a weight of 0, in interleaved runs: after one untimed call of each kind, ``--repeats`` pairs (unguided,
guided), each call between two ``torch.cuda.synchronize()``.  The figures are the medians, the ranges and the ratio of the medians.
The guidance kernels alone (one batched call for the group's canvases, HIP events, median of 21 after 3 untimed calls) and their
registers / LDS from the compiler's resource table are given beside them.  Nothing is gated.  Needs the MI355X."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from srgd_amd import guidance as GD                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--images", type=int, default=5)
    ap.add_argument("--ddpm_steps", type=int, default=50)
    ap.add_argument("--lr_size", type=int, default=256)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_guidance needs the MI355X: no GPU visible and there is no CPU path")
    import bench
    from srgd_amd.synth import synthetic_lr_condition
    device = torch.device("cuda:0")
    sampler, _ = bench.build_sampler(args.dim, device, False, 0)
    sampler.noise_source = "device"
    label = torch.tensor([0], device=device)
    cond = torch.cat([synthetic_lr_condition(i, args.lr_size, args.lr_size).to(device) for i in range(args.images)], 0)
    n_even = ((4 * args.lr_size + 255) // 256 + 1) ** 2 if args.lr_size * 4 > 256 else 1
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def sample(weight):
        sampler.device_noise_seed = 71
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sampler.tiled_sample(batch_size=min(125, n_even * args.images), condition_x=cond, class_label=label,
                                   num_sample_steps=args.ddpm_steps, precision=args.precision, consistency_guidance=weight)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    emit(f"# LR-consistency guidance, weight 1 against weight 0: {args.images} x {4 * args.lr_size}x{4 * args.lr_size} outputs in lock-step, "
         f"{args.ddpm_steps} DDPM steps, {args.precision}, dim {args.dim}, device noise; seconds per tiled_sample call")
    emit(f"# command: python tools/time_guidance.py {' '.join(sys.argv[1:])}")
    emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.note}")
    emit(f"# one untimed call of each kind, then {args.repeats} interleaved pairs (unguided, guided)")
    sample(0.0)
    sample(1.0)
    plain, guided = [], []
    for k in range(args.repeats):
        tp, out_p = sample(0.0)
        tg, out_g = sample(1.0)
        plain.append(tp)
        guided.append(tg)
        emit(f"pair {k}: unguided {tp:.4f} s, guided {tg:.4f} s")
    assert torch.isfinite(out_g).all() and not torch.equal(out_g, out_p)
    mp, mg = statistics.median(plain), statistics.median(guided)
    emit(f"unguided: median {mp:.4f} s [{min(plain):.4f}, {max(plain):.4f}]; guided: median {mg:.4f} s [{min(guided):.4f}, {max(guided):.4f}]")
    emit(f"guided / unguided = {mg / mp:.4f} ({100 * (mg / mp - 1):+.2f} %); per guided step {1e3 * (mg - mp) / args.ddpm_steps:+.3f} ms "
         f"of {1e3 * mp / args.ddpm_steps:.1f} ms")

    # the kernels alone: the group's canvases, one batched call
    h = w = 4 * args.lr_size
    hp = wp = 256 * ((h + 255) // 256 + 1)
    top = left = (hp - h) // 2
    n = args.images
    img = torch.randn(n * 3 * hp * wp, device=device)
    xs = torch.randn(n * 3 * hp * wp, device=device)
    recs, low = GD.records([(b * 3 * hp * wp, b * 3 * h * w, hp, wp, top, left, h, w) for b in range(n)])
    scratch = torch.empty(GD.scratch_bytes(low), device=device, dtype=torch.uint8)
    flat = cond.reshape(-1).contiguous()
    samples = []
    for k in range(24):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        GD.guide_step_flat(img, xs, flat, recs, 0.001, 0.001, scratch)
        b.record()
        b.synchronize()
        if k >= 3:
            samples.append(a.elapsed_time(b))
    moved = n * h * w * 3 * (4 * 1.35 + 0.25 + 12 + 0.36 + 8)
    med = statistics.median(samples)
    emit(f"kernels alone, {n} x {h}x{w} in one call (2 launches): {med:.4f} [{min(samples):.4f}, {max(samples):.4f}] ms; "
         f"{moved / 1e6:.0f} MB by definition = {moved / med / 1e9:.2f} TB/s")
    try:
        from kernel_resources import kernel_table
        for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "guidance.hip")):
            if "guidance_" in r["name"]:
                emit(f"# {r['name']}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS per workgroup, {r['spill']} spilled, "
                     f"{r['scratch']} B scratch per lane, occupancy {r['occupancy']} waves per SIMD")
    except Exception as err:                                 # no compiler on this machine: the table is in the CPU suite
        emit(f"# resource table not available here ({type(err).__name__})")
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
