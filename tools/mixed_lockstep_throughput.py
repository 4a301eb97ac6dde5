"""Mixed-size lock-step against one image per call, at the engine level (whole tiled_sample calls between synchronisations):
dim-128 seeded weights, 50 steps, device noise, bf16 and f16x3.
    (a) 20 LR images alternating 120x80 / 80x120 (BSD100 x4 shapes: 480x320 / 320x480, 9 / 4 tiles per step each)
    (b) a mixed set of LR sizes 64^2, 96x128, 120x80, 80x120, 256^2, 150x200 (x4: 1 ... 25 tiles per even step)
Arms: "solo" = one tiled_sample call per image (what the command line does with such a folder, --lockstep included: its groups
close at every size change) and "mixed" = plan_lockstep_groups at a budget of 125 tiles, one call per group.  Arms alternate,
--repeats rounds each; prints one JSON line per (precision, workload, arm) with images/s and tile-forwards/s.
--alternating_labels gives image i the class label i % 2 (per-image labels: the solo arm passes each image's own [1] label, the
mixed arm one label per image of the group); without it every image carries label 0.
    python tools/mixed_lockstep_throughput.py [--repeats 3] [--precisions bf16,f16x3] [--steps 50] [--alternating_labels]"""
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
    "a_bsd100_x4": [(120, 80), (80, 120)] * 10,
    "b_mixed": [(64, 64), (96, 128), (120, 80), (80, 120), (256, 256), (150, 200)],
}
BUDGET = 125

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--precisions", default="bf16,f16x3")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--workloads", default=",".join(WORKLOADS))
ap.add_argument("--alternating_labels", action="store_true")
args = ap.parse_args()

schema = {k: tuple(v) for k, v in json.load(open(os.path.join(ROOT, "tests", "golden", "schema_dim128.json"))).items()}
conf = load_config(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml"))
conf.num_sample_steps = args.steps
sampler = get_model(conf, logging.getLogger("mixed")).module
sampler.load_state_dict(synth_state_dict(schema, seed=0), strict=True)
sampler = sampler.eval().to(torch.device("cuda", 0))
sampler.noise_source = "device"
sampler.device_noise_seed = 71
label_of = (lambda i: i % 2) if args.alternating_labels else (lambda i: 0)
g = torch.Generator().manual_seed(0)

for prec in args.precisions.split(","):
    for wl in args.workloads.split(","):
        lr = WORKLOADS[wl]
        hr = [(h * 4, w * 4) for (h, w) in lr]
        conds = [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in hr]
        plans, _ = plan_mixed_group(hr)
        per_step = [len(p.coords0) for p in plans], [len(p.coords1) for p in plans]
        tile_fwd = sum(sum(per_step[i % 2]) for i in range(args.steps))     # U-Net tile evaluations of the whole workload
        groups = plan_lockstep_groups(hr, BUDGET)

        def solo():
            for i, c in enumerate(conds):
                sampler.tiled_sample(batch_size=BUDGET, condition_x=c, class_label=torch.tensor([label_of(i)]).cuda(), precision=prec)

        def mixed():
            for grp in groups:
                labels = torch.tensor([label_of(i) for i in grp] if args.alternating_labels else [0]).cuda()
                sampler.tiled_sample(batch_size=BUDGET, condition_x=[conds[i] for i in grp], class_label=labels, precision=prec)
        arms = {"solo": solo, "mixed": mixed}
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
            print(json.dumps(dict(precision=prec, workload=wl, labels="alternating" if args.alternating_labels else "one", arm=k, images=len(lr), calls=len(lr) if k == "solo" else len(groups),
                                  group_sizes=None if k == "solo" else [len(x) for x in groups], steps=args.steps,
                                  tile_forwards=tile_fwd, seconds=[round(t, 3) for t in ts],
                                  images_per_s=round(len(lr) / (sum(ts) / len(ts)), 3),
                                  tile_forwards_per_s=round(tile_fwd / (sum(ts) / len(ts)), 1),
                                  spread_pct=round(100 * (worst - best) / best, 2))), flush=True)
        s, m = (sum(times[k]) / len(times[k]) for k in ("solo", "mixed"))
        print(json.dumps(dict(precision=prec, workload=wl, mixed_over_solo=round(s / m, 3))), flush=True)
