"""Wall-clock cost of joint guidance (``tiled_sample(joint_guidance=True)``) and of the step kernel's third instance:

    python tools/time_joint_guidance.py [--parent DIR] [--precisions bf16,f16x3] [--out profiles/joint_guidance_bench.txt] [--append]

(i)  with ``--parent DIR`` (a built checkout of the parent commit): ``bench.py --gpus 1 --steps 5 --warmup 5`` in DIR and in this tree,
     each in a process of its own, in the order parent, this, parent, this.  The workload launches nothing new; the one- and two-pass
     instance of ``final_step_kernel`` is the parent's code, and the claim to check is that the default line stays inside the parent's
     own run-to-run spread.  Runs before this process touches the GPU.
(ii) per precision, dim 128, ``--images`` (5) 1024x1024 outputs in lock-step, ``--ddpm_steps`` (50) steps, device noise - what ``bench.py``
     times - a joint run (cond_scale 1.5, class_cond_scale 2.0) against the class-guided two-pass run (class_cond_scale 2.0) of the same
     arguments: after one untimed call of each kind, ``--repeats`` interleaved pairs, each call between two ``torch.cuda.synchronize()``.
     Medians, ranges, the ratio of the medians, and the launch sizes behind it.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_guidance_bench.txt"))
    ap.add_argument("--note", default="")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--precisions", default="bf16,f16x3", help="comma-separated; empty: measurement (i) only")
    ap.add_argument("--images", type=int, default=5)
    ap.add_argument("--ddpm_steps", type=int, default=50)
    ap.add_argument("--lr_size", type=int, default=256)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--cond_scale", type=float, default=1.5)
    ap.add_argument("--class_cond_scale", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# command: python tools/time_joint_guidance.py {' '.join(sys.argv[1:])}")
    if args.parent is not None:
        emit("# (i) bench.py --gpus 1 --steps 5 --warmup 5 (bf16, five 1024x1024 outputs in lock-step, 50 steps, no guidance: one-pass "
             "steps), parent / this / parent / this, a process each")
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
    precisions = [p for p in args.precisions.split(",") if p]
    if precisions:
        if not torch.cuda.is_available():
            raise SystemExit("time_joint_guidance needs the MI355X: no GPU visible and there is no CPU path")
        import bench
        from srgd_amd.lanes import lanes_wanted
        from srgd_amd.model import _launch_tiles
        from srgd_amd.synth import synthetic_lr_condition
        device = torch.device("cuda:0")
        sampler, _ = bench.build_sampler(args.dim, device, False, 0)
        sampler.noise_source = "device"
        label = torch.tensor([0], device=device)
        cond = torch.cat([synthetic_lr_condition(i, args.lr_size, args.lr_size).to(device) for i in range(args.images)], 0)
        side = (4 * args.lr_size + 255) // 256
        n_even, n_odd = ((side + 1) ** 2, side ** 2) if args.lr_size * 4 > 256 else (1, 1)
        batch = min(125, n_even * args.images)
        emit(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {args.note}")
        for prec in precisions:

            def sample(joint):
                sampler.device_noise_seed = 71
                kw = dict(cond_scale=args.cond_scale, joint_guidance=True) if joint else {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = sampler.tiled_sample(batch_size=batch, condition_x=cond, class_label=label, class_cond_scale=args.class_cond_scale,
                                           num_sample_steps=args.ddpm_steps, precision=prec, **kw)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out

            emit(f"# (ii) {prec}: joint (cond_scale {args.cond_scale}, class_cond_scale {args.class_cond_scale}) against class-guided "
                 f"(class_cond_scale {args.class_cond_scale}): {args.images} x {4 * args.lr_size}x{4 * args.lr_size} outputs in lock-step, "
                 f"{args.ddpm_steps} DDPM steps, dim {args.dim}, batch_size {batch}, device noise; seconds per tiled_sample call")
            for passes, name in ((2, "class-guided"), (3, "joint")):
                t = _launch_tiles(passes, batch)
                for n, grid in ((n_even * args.images, "even"), (n_odd * args.images, "odd")):
                    k = -(-n // min(t, n))
                    emit(f"#   {name}, {grid} step: {n} tiles in {k} launch(es) of at most {-(-n // k)} tiles = {passes * -(-n // k)} U-Net "
                         f"entries, {lanes_wanted(n, passes, t, sampler.step_lanes, prec)} lane(s)")
            emit(f"# one untimed call of each kind, then {args.repeats} interleaved pairs (class-guided, joint)")
            sample(False)
            sample(True)
            two, three = [], []
            for k in range(args.repeats):
                t2, out2 = sample(False)
                t3, out3 = sample(True)
                two.append(t2)
                three.append(t3)
                emit(f"pair {k}: class-guided {t2:.4f} s, joint {t3:.4f} s")
            assert torch.isfinite(out3).all() and not torch.equal(out2, out3)
            m2, m3 = statistics.median(two), statistics.median(three)
            emit(f"{prec}: class-guided median {m2:.4f} s [{min(two):.4f}, {max(two):.4f}]; joint median {m3:.4f} s "
                 f"[{min(three):.4f}, {max(three):.4f}]; joint / class-guided = {m3 / m2:.4f} (three passes for two: 1.5)")
    try:
        from kernel_resources import kernel_table
        for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "sampler.hip")):
            if "final_step_kernel" in r["name"]:
                emit(f"# {r['name'][:70]}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS per workgroup, {r['spill']} spilled, "
                     f"{r['scratch']} B scratch per lane, occupancy {r['occupancy']} waves per SIMD")
    except Exception as err:                                 # no compiler on this machine: the table is in the CPU suite
        emit(f"# resource table not available here ({type(err).__name__})")
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
