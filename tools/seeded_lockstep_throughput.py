"""Per-image noise seeds in lock-step against one image per call, at the engine level (whole tiled_sample calls between
synchronisations): dim-128 seeded weights, 50 steps, device noise, bf16 by default.
    (a) K = 5 samples of ONE 256^2 LR image (1024^2 HR) with seeds s .. s+4
    (b) 20 LR images alternating 120x80 / 80x120 (BSD100 x4 shapes), every image with its own seed, groups of <= 125 tiles
Arms: "solo" = one tiled_sample call per (image, seed) with device_noise_seed set (the only way to K variants without the
keyword), "seeded" = one call per group with seeds=..., "unseeded" = the same groups without the keyword (all images of a canvas
size share their noise: the same tile count, so seeded - unseeded is the cost of the per-stream draws).  Arms alternate,
--repeats rounds each; prints one JSON line per (precision, workload, arm) and the ratios.
    python tools/seeded_lockstep_throughput.py [--repeats 3] [--precisions bf16] [--steps 50]"""
import argparse
import json
import logging
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from srgd_amd.config import load_config  # noqa: E402
from srgd_amd.lockstep import plan_lockstep_groups, plan_mixed_group  # noqa: E402
from srgd_amd.model import get_model  # noqa: E402
from srgd_amd.synth import synth_state_dict  # noqa: E402

WORKLOADS = {
    "a_5_samples_of_1024": [(256, 256)] * 5,
    "b_bsd100_x4_20_seeds": [(120, 80), (80, 120)] * 10,
}
BUDGET = 125

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--precisions", default="bf16")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--workloads", default=",".join(WORKLOADS))
ap.add_argument("--seed", type=int, default=71)
args = ap.parse_args()

schema = {k: tuple(v) for k, v in json.load(open(os.path.join(ROOT, "tests", "golden", "schema_dim128.json"))).items()}
conf = load_config(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml"))
conf.num_sample_steps = args.steps
sampler = get_model(conf, logging.getLogger("seeded")).module
sampler.load_state_dict(synth_state_dict(schema, seed=0), strict=True)
sampler = sampler.eval().to(torch.device("cuda", 0))
sampler.noise_source = "device"
g = torch.Generator().manual_seed(0)
label = torch.tensor([0]).cuda()

for prec in args.precisions.split(","):
    for wl in args.workloads.split(","):
        lr = WORKLOADS[wl]
        hr = [(h * 4, w * 4) for (h, w) in lr]
        if wl.startswith("a_"):                          # K samples of one image
            conds = [torch.rand(1, 3, *hr[0], generator=g).cuda()] * len(hr)
        else:
            conds = [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in hr]
        seeds = [args.seed + i for i in range(len(hr))]
        plans, _ = plan_mixed_group(hr)
        per_step = [len(p.coords0) for p in plans], [len(p.coords1) for p in plans]
        tile_fwd = sum(sum(per_step[i % 2]) for i in range(args.steps))     # U-Net tile evaluations of the whole workload
        groups = plan_lockstep_groups(hr, BUDGET)

        def solo():
            for c, s in zip(conds, seeds):
                sampler.device_noise_seed = s
                sampler.tiled_sample(batch_size=BUDGET, condition_x=c, class_label=label, precision=prec)

        def seeded():
            for grp in groups:
                sampler.tiled_sample(batch_size=BUDGET, condition_x=[conds[i] for i in grp], class_label=label, precision=prec,
                                     seeds=[seeds[i] for i in grp])

        def unseeded():
            sampler.device_noise_seed = args.seed
            for grp in groups:
                sampler.tiled_sample(batch_size=BUDGET, condition_x=[conds[i] for i in grp], class_label=label, precision=prec)
        arms = {"solo": solo, "seeded": seeded, "unseeded": unseeded}
        for fn in arms.values():                         # warm-up: engines, lane engines, graphs, pool
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(args.repeats):
            for k, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
        for k, ts in times.items():
            best, worst = min(ts), max(ts)
            print(json.dumps(dict(precision=prec, workload=wl, arm=k, images=len(lr), calls=len(lr) if k == "solo" else len(groups),
                                  group_sizes=None if k == "solo" else [len(x) for x in groups], steps=args.steps,
                                  tile_forwards=tile_fwd, seconds=[round(t, 3) for t in ts],
                                  images_per_s=round(len(lr) / (sum(ts) / len(ts)), 3),
                                  tile_forwards_per_s=round(tile_fwd / (sum(ts) / len(ts)), 1),
                                  spread_pct=round(100 * (worst - best) / best, 2))), flush=True)
        mean = {k: sum(ts) / len(ts) for k, ts in times.items()}
        print(json.dumps(dict(precision=prec, workload=wl, seeded_over_solo=round(mean["solo"] / mean["seeded"], 3),
                              seeded_vs_unseeded_pct=round(100 * (mean["seeded"] - mean["unseeded"]) / mean["unseeded"], 2))), flush=True)
