"""What each trailing parity step of a precision schedule buys, against the reference's own full-length fixtures:

    python tools/price_precision_schedule.py [--out_dir profiles] [--cases config2,config5] [--heads bf16,f16x1]
                                             [--tails 0,1,2,5,10,15,25,all] [--repeats 3] [--note "box / commit"]

config2 is ``sample_dim128_config2_1024_50steps`` (one 1024x1024 output, 50 DDPM steps), config5 ``sample_dim128_config5_1024_100steps``
(100 steps, class guidance 2.0): host noise after ``torch.manual_seed`` of the fixture's seed, the recipe of ``_full_length_check`` in
tests/test_engine_gpu.py.  For every head and every T the schedule ``HEAD,f16x3:T`` is run (T = 0: the head alone, T = all: f16x3 alone,
run once and listed under every head) and one line goes to ``precision_schedule.jsonl``:
  max_abs, psnr_db        of the final image against the reference's ``image_u16``;
  x0_max_abs_at           max-abs of ``x_start`` at the fixture's traced steps (8x-subsampled planes, as the fixture holds them);
  wall_s                  seconds of ``tiled_sample`` without trajectories: the median of ``--repeats`` calls between two
                          ``torch.cuda.synchronize()``, after the untimed call that made the figures above;
  weighted_sum_s          the step-weighted sum of the two pure runs' medians of this process, what a switch at no cost would take;
  max_memory_allocated    ``torch.cuda.max_memory_allocated()`` since the case began (canvases and noise; the engines' own memory is
                          not torch's) and ``engine_bytes``, the device bytes held by the engines of the schedule.
``precision_schedule.txt`` holds the same as a table.  One process; every engine is packed once, before the first run.  Nothing is
gated: whether any T below the run's length meets the 1e-3 bar is what the files answer.  The caller sets the time limit (about 5
minutes for config2 and 12 for config5 on one MI355X); the lines written until then stay.  Needs the MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAIL = "f16x3"


def _spec(head, tail_steps, steps):
    if tail_steps == 0:
        return head
    if tail_steps == steps:
        return TAIL
    return f"{head},{TAIL}:{tail_steps}"


def price_case(case, trace_steps, heads, tails, repeats, emit):
    import numpy as np
    import torch
    import bench
    from srgd_amd.precision_schedule import executed_names, plan_steps
    from tests.golden import cases as C
    z = np.load(os.path.join(ROOT, "tests", "golden", f"sample_{case['name']}.npz"))
    want = torch.from_numpy(z["image_u16"].astype(np.float32) / 65535.0)
    device = torch.device("cuda:0")
    sampler, _ = bench.build_sampler(case["dim"], device, False, 0)
    sampler.noise_source = "host"
    cond = C.sampler_condition(case).to(device)
    assert abs(cond.double().sum().item() - float(z["cond_sum"])) < 1e-6, "the condition is not the fixture's"
    steps = case["steps"]
    kw = dict(batch_size=case["batch_size"], condition_x=cond, class_label=torch.tensor([case["label"]], device=device),
              num_sample_steps=steps, cond_scale=case["cond_scale"], class_cond_scale=case["class_cond_scale"])
    for name in list(heads) + [TAIL]:                                   # every engine packed once, outside the timed calls
        sampler.model.engine(name)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()

    def measure(spec):
        torch.manual_seed(case["seed"])
        out, _, x0s = sampler.tiled_sample(precision_schedule=spec, with_images=True, with_x0_images=True, **kw)
        out = out.cpu()
        assert torch.isfinite(out).all(), spec
        err = (out - want).abs()
        x0_err = {str(i): float((C.trace_planes(x0s[i + 1]) - torch.from_numpy(z[f"x0_{i}"])).abs().max()) for i in trace_steps}
        del x0s
        times = []
        for _ in range(repeats):
            torch.manual_seed(case["seed"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sampler.tiled_sample(precision_schedule=spec, **kw)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        names = executed_names(plan_steps(spec, steps))
        return dict(schedule=spec, max_abs=float(err.max()), mean_abs=float(err.mean()),
                    psnr_db=float(10 * np.log10(1.0 / max(float((err ** 2).mean()), 1e-20))), x0_max_abs_at=x0_err,
                    wall_s=statistics.median(times), wall_s_all=times, max_memory_allocated=int(torch.cuda.max_memory_allocated()),
                    engine_bytes=int(sum(sampler.model.engine(n).bytes_in_use() for n in names)))

    pure_tail = measure(TAIL)
    for head in heads:
        pure_head, rows = None, []
        for t in sorted(set(min(t, steps) for t in tails)):
            got = dict(pure_tail) if t == steps else measure(_spec(head, t, steps))
            if t == 0:
                pure_head = got
            rows.append(dict(case=case["name"], steps=steps, head=head, tail=TAIL, tail_steps=t, **got))
            if pure_head is not None:
                rows[-1]["weighted_sum_s"] = ((steps - t) * pure_head["wall_s"] + t * pure_tail["wall_s"]) / steps
            emit(rows[-1])


def table(rows):
    lines = []
    for key in sorted(set((r["case"], r["head"]) for r in rows)):
        part = [r for r in rows if (r["case"], r["head"]) == key]
        lines.append(f"## {key[0]}: {part[0]['steps']} steps, head {key[1]}, tail {TAIL}")
        lines.append(f"{'tail steps':>10} {'schedule':<16} {'max-abs':>10} {'PSNR dB':>8} {'x0 max-abs (last traced)':>25} {'wall s':>8} "
                     f"{'weighted s':>10} {'torch peak MiB':>14} {'engines MiB':>11}")
        for r in part:
            last = list(r["x0_max_abs_at"].values())[-1]
            weighted = f"{r['weighted_sum_s']:.3f}" if "weighted_sum_s" in r else "-"
            lines.append(f"{r['tail_steps']:>10} {r['schedule']:<16} {r['max_abs']:>10.3e} {r['psnr_db']:>8.2f} {last:>25.3e} {r['wall_s']:>8.3f} "
                         f"{weighted:>10} {r['max_memory_allocated'] / 2 ** 20:>14.1f} {r['engine_bytes'] / 2 ** 20:>11.1f}")
        within = [r["tail_steps"] for r in part if r["max_abs"] <= 1e-3]
        lines.append(f"# smallest tail within 1e-3 of the reference: {min(within) if within else 'none of those run'}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out_dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="config2,config5")
    ap.add_argument("--heads", default="bf16,f16x1")
    ap.add_argument("--tails", default="0,1,2,5,10,15,25,all")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    import torch
    from tests.golden import cases as C
    if not torch.cuda.is_available():
        raise SystemExit("price_precision_schedule needs the MI355X: no GPU visible and there is no CPU path")
    known = {"config2": (C.FULL_CASES[0], C.FULL_TRACE_STEPS), "config5": (C.FULL5_CASES[0], C.FULL5_TRACE_STEPS)}
    os.makedirs(args.out_dir, exist_ok=True)
    rows = []
    with open(os.path.join(args.out_dir, "precision_schedule.jsonl"), "a") as f:
        def emit(row):
            rows.append(row)
            f.write(json.dumps(row) + "\n")
            f.flush()
            print(f"{row['case']} {row['schedule']}: max-abs {row['max_abs']:.3e}, {row['psnr_db']:.2f} dB, {row['wall_s']:.3f} s", flush=True)
        for name in args.cases.split(","):
            case, trace_steps = known[name]
            tails = [case["steps"] if t == "all" else int(t) for t in args.tails.split(",")]
            price_case(case, trace_steps, args.heads.split(","), tails, args.repeats, emit)
    with open(os.path.join(args.out_dir, "precision_schedule.jsonl")) as f:     # the table of everything the file holds: a case per call adds up
        rows = [json.loads(ln) for ln in f if ln.strip()]
    head = [f"# precision schedules HEAD,{TAIL}:T against the reference's full-length fixtures: host noise, one 1024x1024 output, dim 128",
            "# made by tools/price_precision_schedule.py from precision_schedule.jsonl (one call for all cases, or one per case)",
            f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; wall s: median of {args.repeats} calls after one untimed",
            f"# {args.note}"]
    with open(os.path.join(args.out_dir, "precision_schedule.txt"), "w") as f:
        f.write("\n".join(head + table(rows)) + "\n")


if __name__ == "__main__":
    main()
