"""Wall-clock cost and gain of the few-step samplers (``tiled_sample(sampler=..., step_spacing=...)``) on the benchmark's headline
configuration:

    python tools/time_solver.py [--out profiles/solver_bench.txt] [--note "box / commit"] [--append]

bf16, dim 128, ``--images`` (5) 1024x1024 outputs in lock-step, device noise - what ``bench.py`` times - in interleaved runs: after one
untimed call of each kind, ``--repeats`` triples (ddpm at ``--ddpm_steps`` (50) steps, dpmpp2m at the same steps and spacing, dpmpp2m
with logsnr spacing at ``--few_steps`` (20) steps), each call between two ``torch.cuda.synchronize()``.  The figures are the medians,
the ranges and the ratios of the medians: the second against the first is the cost of the extra launch and canvas per step, the third
against the first the wall-time ratio a user gets.  The history kernel alone (one batched call for the group's canvases, HIP events,
median of 21 after 3 untimed calls) and its registers from the compiler's resource table are given beside them.  Nothing is gated, and
nothing here measures image quality.  Needs the MI355X."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from srgd_amd import solver as SV                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--images", type=int, default=5)
    ap.add_argument("--ddpm_steps", type=int, default=50)
    ap.add_argument("--few_steps", type=int, default=20)
    ap.add_argument("--lr_size", type=int, default=256)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_solver needs the MI355X: no GPU visible and there is no CPU path")
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

    kinds = [("ddpm", dict(num_sample_steps=args.ddpm_steps)),
             ("dpmpp2m", dict(num_sample_steps=args.ddpm_steps, sampler="dpmpp2m")),
             (f"dpmpp2m logsnr {args.few_steps}", dict(num_sample_steps=args.few_steps, sampler="dpmpp2m", step_spacing="logsnr"))]

    def sample(kw):
        sampler.device_noise_seed = 71
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sampler.tiled_sample(batch_size=min(125, n_even * args.images), condition_x=cond, class_label=label,
                                   precision=args.precision, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    emit(f"# few-step samplers: {args.images} x {4 * args.lr_size}x{4 * args.lr_size} outputs in lock-step, {args.precision}, dim {args.dim}, "
         f"device noise; seconds per tiled_sample call")
    emit(f"# command: python tools/time_solver.py {' '.join(sys.argv[1:])}")
    emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.note}")
    emit(f"# one untimed call of each kind, then {args.repeats} interleaved triples (ddpm {args.ddpm_steps} steps, dpmpp2m {args.ddpm_steps} "
         f"steps, dpmpp2m logsnr {args.few_steps} steps)")
    for _, kw in kinds:
        sample(kw)
    times = [[] for _ in kinds]
    outs = [None] * len(kinds)
    for k in range(args.repeats):
        for j, (_, kw) in enumerate(kinds):
            t, outs[j] = sample(kw)
            times[j].append(t)
        emit(f"triple {k}: " + ", ".join(f"{name} {ts[-1]:.4f} s" for (name, _), ts in zip(kinds, times)))
    assert all(torch.isfinite(o).all() for o in outs) and not torch.equal(outs[0], outs[1])
    med = [statistics.median(ts) for ts in times]
    for (name, _), ts, m in zip(kinds, times, med):
        emit(f"{name}: median {m:.4f} s [{min(ts):.4f}, {max(ts):.4f}]")
    emit(f"dpmpp2m / ddpm at {args.ddpm_steps} steps = {med[1] / med[0]:.4f} ({100 * (med[1] / med[0] - 1):+.2f} %); per step "
         f"{1e3 * (med[1] - med[0]) / args.ddpm_steps:+.3f} ms of {1e3 * med[0] / args.ddpm_steps:.1f} ms")
    emit(f"ddpm {args.ddpm_steps} steps / dpmpp2m logsnr {args.few_steps} steps = {med[0] / med[2]:.3f} x wall time "
         f"(steps alone: {args.ddpm_steps / args.few_steps:.3f} x)")

    # the kernel alone: the group's canvases, one batched call on the inner boxes
    h = w = 4 * args.lr_size
    hp = wp = 256 * ((h + 255) // 256 + 1)
    n = args.images
    img, xs, xp = (torch.randn(n * 3 * hp * wp, device=device) for _ in range(3))
    recs = SV.records([(b * 3 * hp * wp, hp, wp, 128, 128, hp - 256, wp - 256) for b in range(n)])
    samples = []
    for k in range(24):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        SV.history_step_flat(img, xs, xp, recs, 0.001)
        b.record()
        b.synchronize()
        if k >= 3:
            samples.append(a.elapsed_time(b))
    moved = n * (hp - 256) * (wp - 256) * 3 * 20
    m = statistics.median(samples)
    emit(f"kernel alone, {n} inner boxes of {hp - 256}x{wp - 256} in one call (1 launch): {m:.4f} [{min(samples):.4f}, {max(samples):.4f}] ms; "
         f"{moved / 1e6:.0f} MB by definition = {moved / m / 1e9:.2f} TB/s")
    try:
        from kernel_resources import kernel_table
        for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "solver.hip")):
            if "solver_" in r["name"]:
                emit(f"# {r['name']}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS per workgroup, {r['spill']} spilled, "
                     f"{r['scratch']} B scratch per lane, occupancy {r['occupancy']} waves per SIMD")
    except Exception as err:                                 # no compiler on this machine: the table is in the CPU suite
        emit(f"# resource table not available here ({type(err).__name__})")
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
