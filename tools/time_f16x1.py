"""Wall-clock place of the f16x1 precision (f16x3 with the halo-kernel 3x3 convolutions on the f16 hi halves alone) on the benchmark's
headline configuration:

    python tools/time_f16x1.py [--out profiles/f16x1_bench.txt] [--note "box / commit"] [--repeats 3]

dim 128, ``--images`` (5) 1024x1024 outputs in lock-step, ``--ddpm_steps`` (50) steps, device noise - what ``bench.py`` times (bench.py's
``--precision`` choices do not list the mode, hence this tool).  Three kinds of figure:
  rounds   after one untimed call of each precision, ``--repeats`` interleaved rounds of bf16, f16x3, f16mx2, f16x1, each call between
           two ``torch.cuda.synchronize()``: medians, ranges, HR tiles/s and the ratios of the medians;
  lanes    the same for f16x1 with one and with two step lanes (what SRGD_STEP_LANES=1 / =2 select);
  kernel   the one-term kernel against the three-term kernel alone (tools/bench_conv.py --fp32 --impls 6,16 on the two shapes that
           bound the U-Net: 128->128 @256^2 and 1024->1024 @32^2) and its registers / LDS from the compiler's resource table.
Every GPU step is a child process under a time limit of its own; the first one that fails ends the run (nothing is retried) and the
file holds what was measured until then.  Nothing is gated, and nothing here measures image quality.  Needs the MI355X."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PRECISIONS = ("bf16", "f16x3", "f16mx2", "f16x1")
KERNEL_SHAPES = ("3x3 128->128 @256", "3x3 1024->1024 @32")


def _sampler(args):
    import torch
    import bench
    from srgd_amd.synth import synthetic_lr_condition
    if not torch.cuda.is_available():
        raise SystemExit("time_f16x1 needs the MI355X: no GPU visible and there is no CPU path")
    device = torch.device("cuda:0")
    sampler, _ = bench.build_sampler(args.dim, device, False, 0)
    sampler.noise_source = "device"
    label = torch.tensor([0], device=device)
    cond = torch.cat([synthetic_lr_condition(i, args.lr_size, args.lr_size).to(device) for i in range(args.images)], 0)
    n_even = ((4 * args.lr_size + 255) // 256 + 1) ** 2 if args.lr_size * 4 > 256 else 1

    def sample(precision):
        sampler.device_noise_seed = 71
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sampler.tiled_sample(batch_size=min(125, n_even * args.images), condition_x=cond, class_label=label,
                                   num_sample_steps=args.ddpm_steps, precision=precision)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(out).all(), precision
        return dt

    return sampler, sample, torch.cuda.get_device_name(0), torch.__version__


def _summary(emit, names, times, images):
    med = {n: statistics.median(times[n]) for n in names}
    for n in names:
        ts = times[n]
        emit(f"{n}: median {med[n]:.4f} s [{min(ts):.4f}, {max(ts):.4f}] = {images / med[n]:.4f} HR tiles/s "
             f"[{images / max(ts):.4f}, {images / min(ts):.4f}]")
    return med


def step_rounds(args):
    _, sample, dev, tv = _sampler(args)
    emit = lambda s: print(s, flush=True)
    emit(f"# device: {dev}; torch {tv}")
    emit(f"# one untimed call of each precision, then {args.repeats} interleaved rounds of {', '.join(PRECISIONS)}; seconds per tiled_sample call")
    for p in PRECISIONS:
        sample(p)
    times = {p: [] for p in PRECISIONS}
    for k in range(args.repeats):
        for p in PRECISIONS:
            times[p].append(sample(p))
        emit(f"round {k}: " + ", ".join(f"{p} {times[p][-1]:.4f} s" for p in PRECISIONS))
    med = _summary(emit, PRECISIONS, times, args.images)
    spread = max(max(times[p]) - min(times[p]) for p in ("f16mx2", "f16x1"))
    emit(f"f16x3 / f16x1 = {med['f16x3'] / med['f16x1']:.3f} x (ceiling with the kernel at a third of its time: 1.9 x); "
         f"f16mx2 / f16x1 = {med['f16mx2'] / med['f16x1']:.3f} x; f16x1 / bf16 = {med['f16x1'] / med['bf16']:.3f} x")
    emit(f"f16mx2 median - f16x1 median = {med['f16mx2'] - med['f16x1']:+.4f} s; the larger of the two modes' min-max ranges = {spread:.4f} s: "
         f"f16x1 is {'FASTER than f16mx2 beyond the spread' if med['f16mx2'] - med['f16x1'] > spread else 'NOT faster than f16mx2 beyond the spread'}")


def step_lanes(args):
    sampler, sample, _, _ = _sampler(args)
    emit = lambda s: print(s, flush=True)
    names = ("one lane", "two lanes")
    times = {n: [] for n in names}
    emit(f"# f16x1, step lanes forced (SRGD_STEP_LANES=1 / =2): one untimed call each, then {args.repeats} interleaved pairs")
    for untimed in (True, False):
        for k in range(1 if untimed else args.repeats):
            for n, lanes in zip(names, (1, 2)):
                sampler.step_lanes = lanes
                t = sample("f16x1")
                if not untimed:
                    times[n].append(t)
    med = _summary(emit, names, times, args.images)
    spread = max(max(ts) - min(ts) for ts in times.values())
    emit(f"one lane / two lanes = {med['one lane'] / med['two lanes']:.4f} x; difference {med['one lane'] - med['two lanes']:+.4f} s against a "
         f"largest min-max range of {spread:.4f} s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16x1_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--images", type=int, default=5)
    ap.add_argument("--ddpm_steps", type=int, default=50)
    ap.add_argument("--lr_size", type=int, default=256)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step", choices=["rounds", "lanes"], default=None, help="(internal) run one GPU step in this process")
    args = ap.parse_args()
    if args.step:
        return {"rounds": step_rounds, "lanes": step_lanes}[args.step](args)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def save():
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    emit(f"# f16x1 against bf16, f16x3 and f16mx2: {args.images} x {4 * args.lr_size}x{4 * args.lr_size} outputs in lock-step, {args.ddpm_steps} "
         f"DDPM steps, dim {args.dim}, device noise")
    shown, skip = [], False                                  # (where the file goes is not part of what was measured)
    for a in sys.argv[1:]:
        if skip or a == "--out":
            skip = not skip
            continue
        if not a.startswith("--out="):
            shown.append(a)
    emit(f"# command: python tools/time_f16x1.py {' '.join(shown)}")
    emit(f"# {args.note}")
    own = [sys.executable, os.path.abspath(__file__), "--images", str(args.images), "--ddpm_steps", str(args.ddpm_steps), "--lr_size",
           str(args.lr_size), "--dim", str(args.dim), "--repeats", str(args.repeats)]
    per_call = 40.0 * args.images / 5 * args.ddpm_steps / 50          # generous: the four precisions together, seconds
    steps = [("rounds", own + ["--step", "rounds"], 120 + per_call * (args.repeats + 1) * 2),
             ("lanes", own + ["--step", "lanes"], 120 + per_call * (args.repeats + 1))]
    steps += [(f"kernel {shape}", [sys.executable, os.path.join(ROOT, "tools", "bench_conv.py"), "--fp32", "--impls", "6,16", "--only", shape,
                                   "--iters", "20"], 120) for shape in KERNEL_SHAPES]
    for name, cmd, limit in steps:
        emit(f"## {name}")
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            emit(f"step '{name}' exceeded its {limit:.0f} s limit: stopped, nothing further was run")
            save()
            raise SystemExit(1)
        for ln in r.stdout.splitlines():
            if ln.strip() and "amdgpu.ids" not in ln:
                emit(ln)
        if r.returncode != 0:
            emit(f"step '{name}' failed with status {r.returncode}: nothing further was run\n{r.stderr[-1500:]}")
            save()
            raise SystemExit(1)
    emit("## kernel resources (compiler's table; TFLOP/s above are algorithmic: 2 * 9 * Cin * Cout per output pixel)")
    try:
        from kernel_resources import kernel_table
        for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "conv3x3_split.hip")):
            if "conv3x3_split_kernel<" in r["name"] and ", true, " in r["name"][r["name"].index("<"):]:
                emit(f"# {r['name']}: {r['vgpr']} VGPRs, {r['agpr']} AGPRs, {r['sgpr']} SGPRs, {r['spill']} spilled, {r['scratch']} B scratch per "
                     f"lane, occupancy {r['occupancy']} waves per SIMD by registers")
        emit("## the two-workgroups-per-CU build (-DSRGD_SPLIT1_WAVES=4: __launch_bounds__(512, 4), at most 128 VGPRs), compiled only:")
        for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "conv3x3_split.hip"), ["-DSRGD_SPLIT1_WAVES=4"]):
            if "conv3x3_split_kernel<" in r["name"] and r["name"].rstrip().endswith(", 1>"):
                emit(f"# {r['name']}: {r['vgpr']} VGPRs, {r['spill']} spilled, {r['scratch']} B scratch per lane - compiled only, not timed")
        emit("# LDS per workgroup (dynamic): three terms 147,456 B, one term 73,728 B; both run one 512-thread workgroup per CU")
    except Exception as err:                                 # no compiler on this machine: the table is in the CPU suite
        emit(f"# resource table not available here ({type(err).__name__})")
    save()


if __name__ == "__main__":
    main()
