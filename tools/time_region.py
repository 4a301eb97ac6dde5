"""Region resampling against the whole-image run, at the engine level (whole tiled_sample calls between synchronisations): dim-128
seeded weights, 50 steps, device noise; one 256^2 box across a tile seam of a 1024^2 and of a 4096^2 output, bf16 and f16x3.
Arms, per (precision, size):
    "whole"             the run without the keywords - the code path of the commit before the feature, byte for byte
    "region"            region_known + one box, region_skip_tiles=True: only the tiles that touch the box
    "region_all_tiles"  the same with region_skip_tiles=False: every tile, plus the replacement steps
    "region_no_replace" "region" with the replacement step stubbed out (wrong pictures, right tile count): region - this is the
                        time spent in srgd_sampler_q_start, srgd_randn and the strided copies
Prints one JSON line per arm and writes all lines to profiles/region_bench.txt.
    python tools/time_region.py [--repeats 2] [--precisions bf16,f16x3] [--sizes 1024,4096] [--steps 50]"""
import argparse
import json
import logging
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from srgd_amd import region as RG  # noqa: E402
from srgd_amd.config import load_config  # noqa: E402
from srgd_amd.lockstep import image_plan  # noqa: E402
from srgd_amd.model import get_model  # noqa: E402
from srgd_amd.synth import synth_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--precisions", default="bf16,f16x3")
ap.add_argument("--sizes", default="1024,4096")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--batch_size", type=int, default=125)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_bench.txt"))
args = ap.parse_args()

schema = {k: tuple(v) for k, v in json.load(open(os.path.join(ROOT, "tests", "golden", "schema_dim128.json"))).items()}
conf = load_config(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml"))
conf.num_sample_steps = args.steps
sampler = get_model(conf, logging.getLogger("region")).module
sampler.load_state_dict(synth_state_dict(schema, seed=0), strict=True)
sampler = sampler.eval().to(torch.device("cuda", 0))
sampler.noise_source = "device"
sampler.device_noise_seed = 71
g = torch.Generator().manual_seed(0)
label = torch.tensor([0]).cuda()
lines = []


def emit(rec):
    line = json.dumps(rec)
    lines.append(line)
    print(line, flush=True)


replace = RG._RegionRun.replace
for prec in args.precisions.split(","):
    for size in (int(s) for s in args.sizes.split(",")):
        cond = torch.rand(1, 3, size, size, generator=g).cuda()
        known = torch.rand(1, 3, size, size, generator=g).cuda()
        p = image_plan(size, size)
        seam = 512 - p.box[1]                            # image row / column of the even-grid seam at canvas 512
        box = [(seam - 128, seam - 128, 256, 256)]       # across it on both axes: 4 even tiles
        _, counts = RG.plan_region_steps([(p.coords0, p.coords1, p.box[1], p.box[0], tuple(box))])
        kw = dict(batch_size=args.batch_size, condition_x=cond, class_label=label, precision=prec)
        reg = dict(region_known=known, regions=box)

        def no_replace():
            RG._RegionRun.replace = lambda self, *a, **k: None
            try:
                sampler.tiled_sample(**kw, **reg)
            finally:
                RG._RegionRun.replace = replace
        arms = {"whole": lambda: sampler.tiled_sample(**kw),
                "region": lambda: sampler.tiled_sample(**kw, **reg),
                "region_all_tiles": lambda: sampler.tiled_sample(**kw, **reg, region_skip_tiles=False),
                "region_no_replace": no_replace}
        mean = {}
        for name, fn in arms.items():
            fn()                                         # warm-up: engines, graphs, pool
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            mean[name] = sum(ts) / len(ts)
            tiles = (len(p.coords0), len(p.coords1)) if name in ("whole", "region_all_tiles") else (counts[0][0], counts[1][0])
            emit(dict(precision=prec, output=f"{size}x{size}", arm=name, steps=args.steps, tiles_per_step=list(tiles),
                      tile_forwards=sum(tiles[i % 2] for i in range(args.steps)), seconds=[round(t, 3) for t in ts]))
        emit(dict(precision=prec, output=f"{size}x{size}", whole_over_region=round(mean["whole"] / mean["region"], 2),
                  replacement_seconds=round(mean["region"] - mean["region_no_replace"], 3),
                  replacement_share_of_region=round((mean["region"] - mean["region_no_replace"]) / mean["region"], 3),
                  all_tiles_minus_whole_seconds=round(mean["region_all_tiles"] - mean["whole"], 3)))
        del cond, known
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("# tools/time_region.py: one 256x256 box of a finished output, dim-128 seeded weights, device noise\n")
    f.write("\n".join(lines) + "\n")
