"""Wall-clock cost of the dynamic threshold (``tiled_sample(dynamic_threshold=P)``) and of the step kernel's new switch:

    python tools/time_threshold.py [--parent DIR] [--out profiles/threshold_bench.txt] [--note "box / commit"] [--append]

(i)   with ``--parent DIR`` (a built checkout of the parent commit): ``bench.py --gpus 1 --steps 5 --warmup 5`` in DIR and in this tree,
      each in a process of its own, in the order parent, this, parent, this - the step kernel reads one more scalar, and the claim to
      check is that the default line stays inside the parent's own run-to-run spread.  Runs before this process touches the GPU.
(ii)  bf16, dim 128, ``--images`` (5) 1024x1024 outputs in lock-step, ``--ddpm_steps`` (50) steps, device noise - what ``bench.py`` times -
      with the percentile against without, in interleaved runs: after one untimed call of each kind, ``--repeats`` pairs (plain,
      thresholded), each call between two ``torch.cuda.synchronize()``.  Medians, ranges and the ratio of the medians.
(iii) the call alone on the group's canvases (one batched call: a clear, three histogram and three scan launches, one apply launch;
      HIP events, median of 21 after 3 untimed calls, x_start restored before every call), in ms and in bytes moved per second, and
      the kernels' registers / LDS from the compiler's resource table.
Nothing is gated.  Needs the MI355X."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from srgd_amd import threshold as TH                        # noqa: E402


def bench_line(tree):
    """The value of ``bench.py``'s default JSON line, run in ``tree`` in a process of its own."""
    done = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "5"], cwd=tree, capture_output=True,
                          text=True, timeout=900)
    if done.returncode != 0:
        raise SystemExit(f"bench.py failed in {tree}:\n{done.stderr[-2000:]}")
    for ln in reversed(done.stdout.splitlines()):
        try:
            doc = json.loads(ln)
        except ValueError:
            continue
        if isinstance(doc, dict) and "value" in doc:
            return float(doc["value"])
    raise SystemExit(f"no JSON result line from bench.py in {tree}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: measurement (i)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "threshold_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--percentile", type=float, default=0.995)
    ap.add_argument("--images", type=int, default=5)
    ap.add_argument("--ddpm_steps", type=int, default=50)
    ap.add_argument("--lr_size", type=int, default=256)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# command: python tools/time_threshold.py {' '.join(sys.argv[1:])}")
    if args.parent is not None:
        emit("# (i) bench.py --gpus 1 --steps 5 --warmup 5 (bf16, five 1024x1024 outputs in lock-step, 50 steps; the keyword is not set: no "
             "x_start, no threshold launch), parent / this / parent / this, a process each")
        runs = {"parent": [], "this commit": []}
        for k in range(2):
            for name, tree in (("parent", args.parent), ("this commit", ROOT)):
                v = bench_line(tree)
                runs[name].append(v)
                emit(f"{name} run {k}: {v:.4f} HR tiles/s ({1e3 / v:.1f} ms per HR tile)")
        mp, mt = statistics.mean(runs["parent"]), statistics.mean(runs["this commit"])
        sp = abs(runs["parent"][0] - runs["parent"][1]) / mp
        st = abs(runs["this commit"][0] - runs["this commit"][1]) / mt
        emit(f"parent: mean {mp:.4f}, its two runs {100 * sp:.2f} % apart; this commit: mean {mt:.4f}, {100 * st:.2f} % apart; "
             f"this / parent = {mt / mp:.4f} ({100 * (mt / mp - 1):+.2f} %)")
        emit("# two runs each: the difference of the means is " + ("smaller" if abs(mt / mp - 1) <= sp else "LARGER")
             + " than the distance between the parent's own two runs.")
    if not torch.cuda.is_available():
        raise SystemExit("time_threshold needs the MI355X: no GPU visible and there is no CPU path")
    import bench
    from srgd_amd.synth import synthetic_lr_condition
    device = torch.device("cuda:0")
    sampler, _ = bench.build_sampler(args.dim, device, False, 0)
    sampler.noise_source = "device"
    label = torch.tensor([0], device=device)
    cond = torch.cat([synthetic_lr_condition(i, args.lr_size, args.lr_size).to(device) for i in range(args.images)], 0)
    n_even = ((4 * args.lr_size + 255) // 256 + 1) ** 2 if args.lr_size * 4 > 256 else 1

    def sample(p):
        sampler.device_noise_seed = 71
        log = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sampler.tiled_sample(batch_size=min(125, n_even * args.images), condition_x=cond, class_label=label,
                                   num_sample_steps=args.ddpm_steps, precision=args.precision, dynamic_threshold=p, threshold_log=log)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out, log

    emit(f"# (ii) dynamic threshold, P = {args.percentile} against off: {args.images} x {4 * args.lr_size}x{4 * args.lr_size} outputs in "
         f"lock-step, {args.ddpm_steps} DDPM steps, {args.precision}, dim {args.dim}, device noise; seconds per tiled_sample call")
    emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.note}")
    emit(f"# one untimed call of each kind, then {args.repeats} interleaved pairs (plain, thresholded)")
    sample(None)
    sample(args.percentile)
    plain, thr = [], []
    for k in range(args.repeats):
        tp, out_p, _ = sample(None)
        tt, out_t, log = sample(args.percentile)
        plain.append(tp)
        thr.append(tt)
        emit(f"pair {k}: plain {tp:.4f} s, thresholded {tt:.4f} s")
    assert torch.isfinite(out_t).all() and not torch.equal(out_t, out_p)
    s = log[0]
    emit(f"# s of image 0 over the run (synthetic weights: no statement about pictures): first {float(s[0, 0]):.3f}, median "
         f"{float(s[:, 0].median()):.3f}, last {float(s[-1, 0]):.3f}; steps with s > 1: {int((s[:, 0] > 1).sum())} of {s.shape[0]}")
    mp, mt = statistics.median(plain), statistics.median(thr)
    emit(f"plain: median {mp:.4f} s [{min(plain):.4f}, {max(plain):.4f}]; thresholded: median {mt:.4f} s [{min(thr):.4f}, {max(thr):.4f}]")
    emit(f"thresholded / plain = {mt / mp:.4f} ({100 * (mt / mp - 1):+.2f} %); per step {1e3 * (mt - mp) / args.ddpm_steps:+.3f} ms "
         f"of {1e3 * mp / args.ddpm_steps:.1f} ms")

    # (iii) the call alone: the group's canvases, one batched call on the even parity (the whole canvas is the update box)
    h = w = 4 * args.lr_size
    hp = wp = 256 * ((h + 255) // 256 + 1)
    top = left = (hp - h) // 2
    n = args.images
    gen = torch.Generator(device=device).manual_seed(5)
    img = torch.randn(n * 3 * hp * wp, device=device, generator=gen)
    pristine = torch.randn(n * 3 * hp * wp, device=device, generator=gen) * 0.6
    xs = pristine.clone()
    recs = TH.records([(b * 3 * hp * wp, hp, wp, top, left, h, w, 0, 0, hp, wp) for b in range(n)])
    scratch = torch.empty(TH.scratch_bytes(n), device=device, dtype=torch.uint8)
    s_out = torch.empty(n, device=device)
    samples = []
    for k in range(24):
        xs.copy_(pristine)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        TH.threshold_step_flat(img, xs, recs, args.percentile, 0.001, s_out, scratch)
        b.record()
        b.synchronize()
        if k >= 3:
            samples.append(a.elapsed_time(b))
    changed = float((xs != pristine).float().mean())
    moved = n * (3 * 3 * h * w * 4 + 3 * hp * wp * (8 + 8 * changed))
    med = statistics.median(samples)
    emit(f"# (iii) the call alone, {n} x {h}x{w} crop boxes in {hp}x{wp} canvases in one call (a clear and 7 launches), s = "
         f"{[round(float(v), 3) for v in s_out]}, {100 * changed:.1f} % of the elements change")
    emit(f"call alone: {med:.4f} [{min(samples):.4f}, {max(samples):.4f}] ms; {moved / 1e6:.0f} MB by definition (three reads of the "
         f"statistics box, x_start read and written, img read and written where it changes) = {moved / med / 1e9:.2f} TB/s")
    try:
        from kernel_resources import kernel_table
        for src, key, flags in (("threshold.hip", "threshold_", ["-ffp-contract=off"]), ("sampler.hip", "final_step_kernel", [])):
            for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", src), flags):
                if key in r["name"]:
                    emit(f"# {r['name'][:60]}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS per workgroup, {r['spill']} spilled, "
                         f"{r['scratch']} B scratch per lane, occupancy {r['occupancy']} waves per SIMD")
    except Exception as err:                                 # no compiler on this machine: the table is in the CPU suite
        emit(f"# resource table not available here ({type(err).__name__})")
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
