"""Batch driver with the reference ``inference.py`` surface (CLI flags, function names, file naming,
skip-if-exists, per-image reseed) on top of the MI355X engine.

Differences that are deliberate and documented: torchvision/logzero are not needed
(the x4 bicubic resize and the uint8 conversions run as integer kernels on the GPU, bit-identical to what
``T.Resize`` on a PIL image, ``ToTensor`` and ``ToPILImage`` do; ``pil_to_unit_tensor`` / ``unit_tensor_to_pil`` are
the host-side equivalents kept for tests); ``--no_amp`` is accepted and, as upstream (whose sampler ignores ``amp`` and
always computes fp32), changes nothing: the default run reproduces the reference's fp32 numerics.
Engine-only switches: ``--precision {fp32,f16x3,f16x1,bf16,bf16_w8,fp8,fp8_mixed}`` opts into a throughput mode, ``--device_noise`` switches from
the reference-compatible host noise stream to on-device Philox.
"""
from __future__ import annotations

import glob
import json
import logging
import math
import os
import random
from argparse import ArgumentParser
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field, replace
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

from .alpha import MAX_BLEED as ALPHA_BLEED_MAX
from .alpha import alpha_of, check_bleed, check_mode
from .alpha import attach_alpha_on_device, bleed_on_device, resize_planes_on_device  # noqa: F401  (public: srgd_amd.inference.*)
from .backproject import MAX_ITERATIONS as BACK_PROJECT_MAX
from .backproject import back_project_on_device  # noqa: F401  (public: srgd_amd.inference.back_project_on_device)
from .colorfix import color_fix_on_device  # noqa: F401  (public: srgd_amd.inference.color_fix_on_device)
from .config import load_config
from .consistency import KEYS as CONSISTENCY_KEYS
from .consistency import MIN_SIDE as CONSISTENCY_MIN_SIDE
from .consistency import consistency_on_device  # noqa: F401  (public: srgd_amd.inference.consistency_on_device)
from .ensemble import ensemble_on_device  # noqa: F401  (public: srgd_amd.inference.ensemble_on_device)
from .guidance import MIN_SIDE as GUIDANCE_MIN_SIDE
from .lockstep import even_step_tiles, plan_lockstep_groups
from .metrics import KEYS as METRIC_KEYS
from .metrics import metrics_on_device  # noqa: F401  (public: srgd_amd.inference.metrics_on_device)
from .model import ConditionalElucidatedDiffusionSR, get_model
from .precision_schedule import describe_plan, executed_names, plan_steps
from .region import MAX_BOXES as REGION_MAX_BOXES
from .resize import FILTERS as OUTSCALE_FILTERS
from .resize import check_filter, check_outscale, outscale_size
from .selfens import OPS as SELF_ENSEMBLE_OPS
from .selfens import check_self_ensemble
from .selfens import dihedral_on_device, self_ensemble_on_device  # noqa: F401  (public: srgd_amd.inference.*)
from .solver import check_sampler
from .threshold import check_percentile

logger = logging.getLogger("srgd_amd")


def parse_args(argv=None):
    p = ArgumentParser()
    p.add_argument("-c", "--conf", required=True, help="Path to config file")
    p.add_argument("-m", "--ckpt_path", type=str, required=True)
    p.add_argument("--input_dir", type=str, required=True)
    p.add_argument("--output_dir", type=str, required=True)
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--num_sample_steps", type=int, default=250)
    p.add_argument("--interpolation", type=str, default="bicubic")
    p.add_argument("--cond_scale", type=float, default=1.0)
    p.add_argument("--class_cond_scale", type=float, default=1.0)
    p.add_argument("--guidance_start_steps", type=int, default=0)
    p.add_argument("--class_guidance_start_steps", type=int, default=0)
    p.add_argument("--generation_start_steps", type=int, default=0)
    p.add_argument("--start_index", type=int, default=0)
    p.add_argument("--end_index", type=int, default=None)
    p.add_argument("--test_label", type=int, default=None)
    p.add_argument("--no_amp", dest="amp", action="store_false")
    p.add_argument("--no_dpmpp_solver", dest="use_dpmpp_solver", action="store_false")
    p.add_argument("--seed", type=int, default=71)
    p.add_argument("--backend", type=str, default="ddp")
    # engine-only switches (absent upstream)
    p.add_argument("--precision", choices=["fp32", "f16x3", "f16mx2", "f16x1", "bf16", "bf16_w8", "fp8", "fp8_mixed"], default="f16x3",
                   help="f16x3 (default since round 6): fp32 tensors, every convolution product as three f16 MFMAs on (hi, lo) operand "
                        "pairs - within 1e-5 of the reference's CPU path on its fixtures (bar: 1e-3), 3x the speed of fp32; "
                        "fp32: exact-fp32 MFMA (the reference's arithmetic up to summation order); bf16 / bf16_w8 / fp8 / fp8_mixed: "
                        "throughput modes of the MI355X engine (explicit opt-in, not within 1e-3); f16x1: a throughput mode between "
                        "bf16 and f16x3 - f16x3 with the 3x3 convolutions on the f16 hi halves alone, one MFMA per product: "
                        "0.697 HR tiles/s at the headline configuration where f16x3 gives 0.423 and bf16 1.365 (profiles/f16x1_bench.txt); "
                        "77.5 dB / max-abs 3.8e-3 against the reference on its 256^2 fixture where bf16 gives 55.9 dB, random-init weights "
                        "(profiles/f16x1_numerics.jsonl) - NOT within 1e-3, quality on trained weights unmeasured")
    p.add_argument("--device_noise", action="store_true",
                   help="draw DDPM noise on the GPU (Philox) instead of replaying torch's CPU stream")
    group = p.add_mutually_exclusive_group()
    group.add_argument("--lockstep", type=int, default=1,
                       help="sample up to N consecutive same-sized images together (their tiles share U-Net launches, "
                            "--batch_size tiles per image and launch); every image comes out bit-identical to its solo run")
    group.add_argument("--lockstep_tiles", type=int, default=None, metavar="T",
                       help="sample consecutive images of ANY size together, up to T tiles per even step (an image larger "
                            "than T runs alone); every image comes out bit-identical to its solo run (DDPM configs only)")
    p.add_argument("--label_file", type=str, default=None, metavar="PATH",
                   help="text file of `file_name label` lines: the images of --input_dir named there are sampled with that class "
                        "label, the others with --test_label; lock-step groups may mix labels (engine extension)")
    p.add_argument("--samples", type=int, default=1, metavar="K",
                   help="sample every input image K times in lock-step with the noise seeds --seed, --seed+1, ..., --seed+K-1: sample 0 "
                        "goes to <name>_out.png (the file a run without --samples writes), sample k >= 1 to <name>_out_s<k>.png, each "
                        "bit-identical to a solo run with that seed (engine extension, DDPM configs only)")
    p.add_argument("--color_fix", choices=["none", "wavelet", "adain"], default="none",
                   help="colour-correct every output against its x4 bicubic input on the GPU (engine extension): wavelet = the input's "
                        "low frequencies (five a-trous levels) under the output's high frequencies, adain = the input's per-channel "
                        "mean and standard deviation; with --samples every sample is corrected against the same input")
    p.add_argument("--reference_dir", type=str, default=None, metavar="DIR",
                   help="ground truth of the inputs: the reference of IN/NAME.png is DIR/NAME.png, exactly x4 its size.  Y-channel "
                        "PSNR, RGB PSNR and Y-channel SSIM of every written file (as saved, after --color_fix) are computed on the GPU "
                        "and written to OUTPUT_DIR/metrics.json with per-image means over --samples and a mean over all images; with "
                        "--outscale the x4 image is measured, before the resize (engine extension)")
    p.add_argument("--crop_border", type=int, default=4, metavar="N",
                   help="pixels cut from every side of output and reference before the --reference_dir numbers are taken (default 4, "
                        "the scale factor, as the x4 super-resolution literature does)")
    p.add_argument("--ensemble", action="store_true",
                   help="with --samples K >= 2: write the mean image of every input's K samples to <name>_out_mean.png and their "
                        "per-pixel spread (twice the standard deviation, 8-bit) to <name>_out_std.png, both computed on the GPU from the "
                        "samples as saved, and the spread statistics to OUTPUT_DIR/ensemble.json; with --reference_dir the mean "
                        "image's PSNR / SSIM join metrics.json (engine extension)")
    p.add_argument("--consistency", action="store_true",
                   help="LR consistency of every written file: the output as saved (after --color_fix) is reduced x4 on the GPU with the "
                        "operator that made the condition (Pillow's bicubic) and compared with its own input - no ground truth "
                        "needed.  LR-PSNR, LR-MSE and the largest 8-bit error go to OUTPUT_DIR/consistency.json with per-image means "
                        "over --samples and a mean over all images; with --ensemble the mean images are measured too; with "
                        "--outscale the x4 image is measured, before the resize (engine extension)")
    p.add_argument("--back_project", type=int, default=0, metavar="N",
                   help="pull every output back onto its own input on the GPU with N <= 64 steps of iterative back-projection, after "
                        "--color_fix and before the file is saved: the output is reduced x4 and enlarged x4 again with Pillow's bicubic "
                        "and the difference between the x4 input and that image is added, in 8 bits (0, the default: off); raises the "
                        "LR-PSNR --consistency reports; with --samples every sample is corrected against the same input (engine "
                        "extension)")
    p.add_argument("--consistency_guidance", type=float, default=0.0, metavar="G",
                   help="LR-consistency guidance inside the DDPM sampling loop, weight G in [0, 1] (0, the default: off): after every "
                        "step the predicted clean image is reduced x4 and enlarged x4 again on the GPU with the coefficients of "
                        "Pillow's bicubic, and G times the difference between the x4 input and that image is added to the prediction "
                        "and, scaled by the step's weight of the prediction, to the image - the later steps harmonise the correction; "
                        "raises the LR-PSNR --consistency reports; inputs must be at least 5 pixels on a side (engine extension)")
    p.add_argument("--consistency_guidance_start_steps", type=int, default=0, metavar="S",
                   help="with --consistency_guidance: the first guided step (default 0: every step)")
    p.add_argument("--sampler", choices=["ddpm", "ddim", "dpmpp2m"], default="ddpm",
                   help="the step of the tiled DDPM sampling loop: ddpm (default) is the reference's ancestral step; ddim is the DDIM "
                        "family's step with --eta; dpmpp2m is the deterministic second-order multistep solver DPM-Solver++ 2M, which "
                        "with --step_spacing logsnr reaches in 15-20 steps what the first-order steps need 50 and more for - one "
                        "small extra GPU launch per step; the noise draws are those of a ddpm run of the same --num_sample_steps "
                        "(engine extension)")
    p.add_argument("--eta", type=float, default=None, metavar="E",
                   help="with --sampler ddim: the share E in [0, 1] of the ancestral step's noise (default 0: deterministic; 1 is the "
                        "ddpm step up to rounding); dpmpp2m takes 0 only, ddpm none")
    p.add_argument("--step_spacing", choices=["time", "logsnr"], default="time",
                   help="where the --num_sample_steps steps end: time (default) is the reference's uniform grid in t, whose last steps "
                        "jump several units of log-SNR; logsnr is uniform in the log-SNR itself (engine extension)")
    p.add_argument("--dynamic_threshold", type=float, default=0.0, metavar="P",
                   help="dynamic thresholding inside the DDPM sampling loop, percentile P in (0, 1] (0, the default: off; 0.995 is "
                        "Imagen's choice): the steps are taken without the static clamp of the predicted clean image to [-1, 1]; "
                        "after every step the GPU takes per image s = max(1, the exact P-quantile of the prediction's magnitudes), "
                        "clips the prediction to [-s, s] and divides it by s - for guidance scales above 1 (--cond_scale, "
                        "--class_cond_scale), whose overshoot a hard clamp turns into saturated regions; one small batched GPU "
                        "call per step (engine extension)")
    p.add_argument("--joint_guidance", action="store_true",
                   help="allow --cond_scale and --class_cond_scale together in the DDPM sampling loop: every step on which both are "
                        "in force is one three-pass step, eps = e + (s_c - 1)(e - n_c) + (s_l - 1)(e - n_l), with n_c the prediction "
                        "without the condition and n_l the one without the label; about 1.5 times the time of a two-pass step, no "
                        "more memory; without the flag both scales are refused as upstream refuses them; see --dynamic_threshold "
                        "for the overshoot (engine extension)")
    p.add_argument("--outscale", type=float, default=4.0, metavar="S",
                   help="write every file at S times the size of its input instead of 4 times, S in [0.5, 32] (4, the default: off): the "
                        "x4 output as it would have been saved - after --color_fix and --back_project - is resampled on the GPU to "
                        "max(1, floor(in * S + 0.5)) pixels per axis, bit for bit Pillow's Image.resize, immediately before the file "
                        "is encoded; every sample of --samples is resized; not with --ensemble (engine extension)")
    p.add_argument("--outscale_filter", choices=list(OUTSCALE_FILTERS), default=None,
                   help="with --outscale: the filter of the resize (default bicubic, the operator that made the model's conditions)")
    p.add_argument("--alpha", choices=["drop", "keep"], default="drop",
                   help="keep: an input with transparency (modes RGBA, LA, PA, or a tRNS chunk) is written as an RGBA file: its alpha "
                        "plane is enlarged x4 on the GPU with Pillow's bicubic, the operator that makes the model's conditions, and with "
                        "--outscale resized again with --outscale_filter, bit for bit the alpha band of Pillow's Image.resize; the "
                        "colour is the image a run without the flag writes and is not premultiplied; inputs without transparency are "
                        "written as RGB as before; every sample of --samples gets the same alpha; not with --ensemble.  drop (the "
                        "default): the alpha channel is ignored (engine extension)")
    p.add_argument("--alpha_bleed", type=int, default=0, metavar="N",
                   help="with --alpha keep: before anything else sees a transparent input, spread the colours of its visible pixels "
                        "(alpha > 0) N <= 64 pixels into the transparent area on the GPU - every pass gives each unknown pixel the "
                        "rounded mean of its known 8-neighbours - so that the arbitrary colour stored under transparent pixels does "
                        "not leak across the outline as a halo; the bled image is the input of the whole run (condition, --color_fix, "
                        "--back_project, --consistency_guidance, --consistency); the alpha itself is unchanged (0, the default: off)")
    p.add_argument("--self_ensemble", type=int, default=1, metavar="N",
                   help="geometric self-ensemble, N in {1, 2, 4, 8} (1, the default: off): every input is sampled in N orientations - "
                        "2: as it is and mirrored, 4: the four flips, 8: the four flips of the image and of its transpose, the x8 '+' "
                        "variant of the SR literature - in lock-step (--lockstep N*K unless a lock-step flag is given), every output "
                        "is turned back and the N are averaged on the GPU, halves up; --color_fix, --back_project, "
                        "--consistency_guidance and --dynamic_threshold act on every orientation against its own turned input, "
                        "--reference_dir, --consistency, --outscale, --alpha keep and --ensemble on the merged image (engine "
                        "extension, DDPM configs only)")
    p.add_argument("--region_known_dir", type=str, default=None, metavar="DIR",
                   help="resample rectangles of finished outputs: DIR holds an earlier run's output of every input, <name>_out.png "
                        "(with --samples K: <name>_out_s<k>.png, or the one <name>_out.png for every sample - K alternatives of the "
                        "region), exactly x4 of the input - checked before anything is sampled; inside the boxes of --region the "
                        "image is sampled again, coherent with its surroundings, outside them the written file equals the known one "
                        "byte for byte, and only the tiles that touch a box are evaluated; DDPM configs only, not with "
                        "--self_ensemble or --ensemble (engine extension)")
    p.add_argument("--region", action="append", default=None, metavar="T,L,H,W",
                   help="with --region_known_dir: a box top,left,height,width in output pixels to sample again; repeatable up to 16 "
                        "times, boxes may overlap; the same boxes are used for every input, so each must lie inside every output")
    p.add_argument("--precision_schedule", type=str, default=None, metavar="SPEC",
                   help="a precision per step instead of --precision, NAME[:COUNT](,NAME[:COUNT])* over the loop indices of "
                        "--num_sample_steps: bf16:40,f16x3 takes the first 40 steps in bf16 and the rest in f16x3, bf16,f16x3:10 the last "
                        "10 in f16x3; 1 to 4 entries, at most one without a count.  The canvases are fp32 in every precision, so a switch "
                        "converts nothing and every step is the step its precision takes from that canvas; every named engine holds its "
                        "own packed weights.  How far a mixed run lies from the reference is measured by "
                        "tools/price_precision_schedule.py (DDPM configs only, engine extension)")
    args = p.parse_args(argv)
    if args.precision_schedule is not None:
        try:
            args.precision_plan = plan_steps(args.precision_schedule, args.num_sample_steps)
        except ValueError as e:
            raise SystemExit(f"--precision_schedule: {e}")
    try:
        args.self_ensemble = check_self_ensemble(args.self_ensemble)
    except ValueError as e:
        raise SystemExit(f"--self_ensemble: {e}")
    if (args.region_known_dir is None) != (args.region is None):
        raise SystemExit("--region_known_dir and --region go together: the finished outputs and the boxes to sample again")
    if args.region is not None:
        try:
            args.region = [parse_region(text) for text in args.region]
        except ValueError as e:
            raise SystemExit(f"--region: {e}")
        if len(args.region) > REGION_MAX_BOXES:
            raise SystemExit(f"--region: at most {REGION_MAX_BOXES} boxes, got {len(args.region)}")
        if args.self_ensemble > 1:
            raise SystemExit("--region_known_dir: not together with --self_ensemble (a region run keeps one finished image; the "
                             "orientations have none)")
        if args.ensemble:
            raise SystemExit("--region_known_dir: not together with --ensemble (outside the boxes every sample is the known image)")
    if not 0 <= args.alpha_bleed <= ALPHA_BLEED_MAX:
        raise SystemExit(f"--alpha_bleed: N must be in 0 .. {ALPHA_BLEED_MAX}, got {args.alpha_bleed}")
    if args.alpha_bleed and args.alpha != "keep":
        raise SystemExit("--alpha_bleed: needs --alpha keep")
    if args.ensemble and args.alpha == "keep":
        raise SystemExit("--ensemble: not together with --alpha keep (the ensemble reads samples back as RGB; the mean image gets no alpha)")
    try:
        args.outscale = check_outscale(args.outscale)
    except ValueError as e:
        raise SystemExit(f"--outscale: {e}")
    if args.outscale is None and args.outscale_filter is not None:
        raise SystemExit("--outscale_filter: needs --outscale S with S != 4")
    args.outscale_filter = check_filter(args.outscale_filter)
    if args.ensemble and args.outscale is not None:
        raise SystemExit("--ensemble: not together with --outscale (the ensemble reads samples back at x4 of the input and feeds the x4 "
                         "metrics)")
    try:
        check_sampler(args.sampler, args.eta, args.step_spacing)
    except ValueError as e:
        raise SystemExit(f"--sampler / --eta / --step_spacing: {e}")
    if not 0.0 <= args.dynamic_threshold <= 1.0:            # NaN fails both comparisons
        raise SystemExit(f"--dynamic_threshold: P must be in [0, 1], got {args.dynamic_threshold}")
    if not 0.0 <= args.consistency_guidance <= 1.0:         # NaN fails both comparisons
        raise SystemExit(f"--consistency_guidance: G must be in [0, 1], got {args.consistency_guidance}")
    if args.consistency_guidance_start_steps < 0:
        raise SystemExit(f"--consistency_guidance_start_steps: S must be >= 0, got {args.consistency_guidance_start_steps}")
    if not 0 <= args.back_project <= BACK_PROJECT_MAX:
        raise SystemExit(f"--back_project: N must be in 0 .. {BACK_PROJECT_MAX}, got {args.back_project}")
    if args.ensemble and not 2 <= args.samples <= 256:
        raise SystemExit(f"--ensemble: needs --samples K with 2 <= K <= 256, got K = {args.samples}")
    if args.crop_border < 0:
        raise SystemExit(f"--crop_border: N must be >= 0, got {args.crop_border}")
    if args.samples < 1:
        raise SystemExit(f"--samples: K must be >= 1, got {args.samples}")
    if args.seed < 0 and args.samples > 1:
        raise SystemExit("--samples: noise seeds are non-negative, --seed must be >= 0")
    args.labels = None
    if args.label_file is not None:
        args.labels = parse_label_file(args.label_file, args.input_dir, load_config(args.conf).num_classes)
    return args


def parse_label_file(path, input_dir, num_classes):
    """``--label_file``: ``{file name: label}`` from lines of ``file_name label`` (blank lines and ``#`` comments skipped).
    Every name must be a file of ``input_dir`` and every label an integer in ``[0, num_classes)``; anything else ends the
    run here (``SystemExit``), before the model is built."""
    try:
        with open(path) as f:
            lines = f.read().splitlines()
    except OSError as err:
        raise SystemExit(f"--label_file: cannot read {path}: {err}")
    if not num_classes:
        raise SystemExit("--label_file: the configured U-Net has no class embedding (num_classes is not set)")
    present = {os.path.basename(f) for f in glob.glob(f"{input_dir}/*")}
    labels = {}
    for no, line in enumerate(lines, 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        parts = line.rsplit(None, 1)
        if len(parts) != 2:
            raise SystemExit(f"--label_file {path}:{no}: expected `file_name label`")
        name, text = parts[0].strip(), parts[1]
        try:
            label = int(text)
        except ValueError:
            raise SystemExit(f"--label_file {path}:{no}: label {text!r} is not an integer")
        if not 0 <= label < num_classes:
            raise SystemExit(f"--label_file {path}:{no}: label {label} outside [0, {num_classes})")
        if name not in present:
            raise SystemExit(f"--label_file {path}:{no}: {name!r} is not a file of {input_dir}")
        labels[name] = label
    return labels


def _label_tensor(test_label, n_images, device):
    """``test_label``: None, one label for all images (the reference's ``[1]`` tensor) or a sequence of one per image."""
    if test_label is None:
        return None
    if isinstance(test_label, (list, tuple)):
        assert len(test_label) == n_images, "one label per lock-step image"
        ids = list(test_label) if len(set(test_label)) > 1 else [test_label[0]]
    else:
        ids = [test_label]
    return torch.LongTensor(ids).to(device)


def _color_fix_kw(color_fix):
    """``tiled_sample``'s ``color_fix`` keyword for a set mode; nothing for None / "none" (the call a run without the flag makes)."""
    return {} if color_fix in (None, "none") else {"color_fix": color_fix}


def _back_project_kw(back_project):
    """``tiled_sample``'s ``back_project`` keyword for N > 0; nothing for 0 / None (the call a run without the flag makes)."""
    return {"back_project": back_project} if back_project else {}


def _guidance_kw(consistency_guidance, consistency_guidance_start_steps=0):
    """``tiled_sample``'s ``consistency_guidance`` keywords for a weight > 0; nothing for 0 / None (the call a run without the flag
    makes)."""
    if not consistency_guidance:
        return {}
    return {"consistency_guidance": consistency_guidance, "consistency_guidance_start_steps": consistency_guidance_start_steps}


def _threshold_kw(dynamic_threshold):
    """``tiled_sample``'s ``dynamic_threshold`` keyword for a percentile > 0; nothing for 0 / None (the call a run without the flag
    makes)."""
    return {"dynamic_threshold": dynamic_threshold} if dynamic_threshold else {}


def _joint_kw(joint_guidance):
    """``tiled_sample``'s ``joint_guidance`` keyword where it is set; nothing otherwise (the call a run without the flag makes)."""
    return {"joint_guidance": True} if joint_guidance else {}


def _sampler_kw(sampler="ddpm", eta=None, step_spacing="time"):
    """``tiled_sample``'s ``sampler`` / ``eta`` / ``step_spacing`` keywords, each only where it is not the default (nothing for the
    call a run without the flags makes)."""
    kw = {}
    if sampler not in (None, "ddpm"):
        kw["sampler"] = sampler
    if eta is not None:
        kw["eta"] = eta
    if step_spacing not in (None, "time"):
        kw["step_spacing"] = step_spacing
    return kw


def _reference_kw(reference, crop_border):
    """``tiled_sample``'s ``reference`` / ``crop_border`` keywords where a reference is given; nothing otherwise."""
    return {} if reference is None else {"reference": reference, "crop_border": crop_border}


def _split_quality(output, reference):
    """``tiled_sample``'s return value as ``(images, metric dicts or None)``."""
    return output if reference is not None else (output, None)


def _header_size(path):
    """``(width, height)`` from an image file's header, or None where the file cannot be read as an image."""
    try:
        with Image.open(path) as im:
            return im.size
    except (IOError, SyntaxError):
        return None


def reference_problems(file_names, reference_dir, scale=4, crop_border=4):
    """``--reference_dir`` pre-flight: one line per input file whose reference ``reference_dir/<same name>`` is missing, unreadable,
    not exactly ``scale`` times the input's size, or too small for an 11x11 window inside the crop.  Only image headers are read."""
    problems = []
    for f in file_names:
        name = os.path.basename(f)
        ref = os.path.join(reference_dir, name)
        size = _header_size(f)
        if size is None:
            continue                                     # not an image: the sampling loop reports and skips it
        if not os.path.isfile(ref):
            problems.append(f"{name}: reference {ref} is missing")
            continue
        ref_size = _header_size(ref)
        if ref_size is None:
            problems.append(f"{name}: reference {ref} cannot be read as an image")
            continue
        (w, h), (rw, rh) = size, ref_size
        if (rw, rh) != (w * scale, h * scale):
            problems.append(f"{name}: reference is {rw}x{rh}, x{scale} of the {w}x{h} input is {w * scale}x{h * scale}")
        elif min(rw, rh) - 2 * crop_border < 11:
            problems.append(f"{name}: {rw}x{rh} keeps fewer than 11x11 pixels inside a crop of {crop_border}")
    return problems


def check_references(file_names, reference_dir, scale=4, crop_border=4):
    """Ends the run (``SystemExit``, non-zero) with the names ``reference_problems`` lists, before any sampling."""
    problems = reference_problems(file_names, reference_dir, scale, crop_border)
    if problems:
        raise SystemExit("--reference_dir: " + str(len(problems)) + " input(s) without a usable reference:\n  " + "\n  ".join(problems))


def parse_region(text):
    """``--region T,L,H,W`` -> ``(top, left, height, width)``: four integers, the size positive, the corner non-negative
    (``ValueError`` otherwise; whether the box lies inside an output is checked against the known files)."""
    parts = str(text).split(",")
    try:
        box = tuple(int(v) for v in parts)
    except ValueError:
        box = ()
    if len(parts) != 4 or len(box) != 4:
        raise ValueError(f"{text!r} is not top,left,height,width (four integers)")
    if box[0] < 0 or box[1] < 0 or box[2] < 1 or box[3] < 1:
        raise ValueError(f"{text!r}: top and left must be >= 0, height and width >= 1")
    return box


def _region_kw(region_known, regions):
    """``tiled_sample``'s ``region_known`` / ``regions`` keywords where a known image is given; nothing otherwise (the call a run
    without the flags makes)."""
    return {} if region_known is None else {"region_known": region_known, "regions": regions}


def region_known_path(known_dir, file_name, k, samples=1):
    """``--region_known_dir``: the known file of sample k of an input - ``known_dir/<name>_out.png`` (sample k >= 1:
    ``<name>_out_s<k>.png``); under ``--samples`` a file without its own ``_out_s<k>.png`` starts every sample from the one
    ``<name>_out.png``."""
    own = os.path.join(known_dir, sample_output_name(file_name, k))
    if k > 0 and samples > 1 and not os.path.isfile(own):
        return os.path.join(known_dir, sample_output_name(file_name, 0))
    return own


def region_known_problems(file_names, known_dir, regions, scale=4, samples=1):
    """``--region_known_dir`` pre-flight: one line per known file that is missing, unreadable or not exactly ``scale`` times its
    input's size, and per box of ``regions`` that does not lie inside that output.  Only image headers are read."""
    problems = []
    for f in file_names:
        name = os.path.basename(f)
        size = _header_size(f)
        if size is None:
            continue                                     # not an image: the sampling loop reports and skips it
        w, h = size
        for known in sorted({region_known_path(known_dir, f, k, samples) for k in range(samples)}):
            if not os.path.isfile(known):
                problems.append(f"{name}: known output {known} is missing")
                continue
            known_size = _header_size(known)
            if known_size is None:
                problems.append(f"{name}: known output {known} cannot be read as an image")
                continue
            if known_size != (w * scale, h * scale):
                problems.append(f"{name}: known output {os.path.basename(known)} is {known_size[0]}x{known_size[1]}, x{scale} of the {w}x{h} input is "
                                f"{w * scale}x{h * scale}")
        for (t, l, bh, bw) in regions:
            if t + bh > h * scale or l + bw > w * scale:
                problems.append(f"{name}: box {t},{l},{bh},{bw} does not lie inside the {w * scale}x{h * scale} output")
    return problems


def check_region_known(file_names, known_dir, regions, scale=4, samples=1):
    """Ends the run (``SystemExit``, non-zero) with the lines ``region_known_problems`` lists, before any sampling."""
    problems = region_known_problems(file_names, known_dir, regions, scale, samples)
    if problems:
        raise SystemExit("--region_known_dir: " + str(len(problems)) + " problem(s):\n  " + "\n  ".join(problems))


def load_region_known(path):
    """A known output as the fp32 ``[1,3,H,W]`` tensor in [0, 1] ``tiled_sample(region_known=...)`` takes: the file's bytes over
    255, which ``mul(255).byte()`` writes back unchanged."""
    with Image.open(path) as im:
        return pil_to_unit_tensor(im)[None]


def load_reference(path):
    """A ground-truth image as the uint8 ``[H,W,3]`` tensor ``tiled_sample(reference=...)`` takes (decoded on the host)."""
    with Image.open(path) as im:
        return torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy())


def mean_record(records, keys=METRIC_KEYS):
    """Arithmetic mean of metric dicts, key by key of ``keys`` (PSNR averaged in dB, the SR convention); inf and NaN propagate."""
    return {k: sum(r[k] for r in records) / len(records) for k in keys}


def _json_record(record):
    """A metric dict for JSON: finite numbers as they are, the others as the strings "nan", "inf", "-inf"."""
    return {k: (v if math.isfinite(v) else ("nan" if math.isnan(v) else ("inf" if v > 0 else "-inf"))) for k, v in record.items()}


def _records_document(head, file_records, samples, keys, ensemble):
    """The layout ``metrics.json`` and ``consistency.json`` share: ``head``, then ``"files"``, ``"images"`` (with --samples only),
    ``"mean"`` and, for a non-empty ``ensemble``, ``"ensemble"`` / ``"ensemble_mean"``; every mean is taken over ``keys``."""
    per_image = {}
    for name, _, rec in file_records:
        per_image.setdefault(name, []).append(rec)
    image_means = {name: mean_record(recs, keys) for name, recs in per_image.items()}
    doc = dict(head, files={written: _json_record(rec) for _, written, rec in file_records})
    if samples > 1:
        doc["images"] = {name: _json_record(rec) for name, rec in image_means.items()}
    doc["mean"] = _json_record(mean_record(list(image_means.values()), keys))
    if ensemble:
        doc["ensemble"] = {name: _json_record(rec) for name, rec in ensemble}
        doc["ensemble_mean"] = _json_record(mean_record([rec for _, rec in ensemble], keys))
    return doc


def metrics_document(file_records, samples, crop_border, ensemble=None):
    """``metrics.json``: ``file_records`` = ``[(input file name, written file name, metric dict)]`` in run order ->
    ``{"crop_border", "files": {written file: record}, "images": {input file: mean over its samples} (with --samples only),
    "mean": mean over the images}``.  ``ensemble`` (``--ensemble``): ``[(input file name, metric dict of its mean image)]`` adds
    ``"ensemble": {input file: record}`` and ``"ensemble_mean"``, the mean over those; None or empty adds nothing."""
    return _records_document({"crop_border": crop_border}, file_records, samples, METRIC_KEYS, ensemble)


def consistency_document(file_records, samples, ensemble=None):
    """``consistency.json``: ``file_records`` = ``[(input file name, written file name, {"lr_psnr", "lr_mse", "lr_max_abs"})]`` in run
    order -> ``{"files": {written file: record}, "images": {input file: mean over its samples} (with --samples only), "mean": mean
    over the images}``; PSNR is averaged in dB as in ``metrics.json``.  ``ensemble`` (``--ensemble``): ``[(input file name, record of
    its mean image)]`` adds ``"ensemble": {input file: record}`` and ``"ensemble_mean"``, the mean over those; None or empty adds
    nothing.  Non-finite values are written as strings (``_json_record``)."""
    return _records_document({}, file_records, samples, CONSISTENCY_KEYS, ensemble)


def ensemble_output_names(file_name):
    """``--ensemble``: the two file names of an input file's ensemble, ``<name>_out_mean.png`` and ``<name>_out_std.png``."""
    base = os.path.basename(file_name)
    return base.replace(".png", "_out_mean.png"), base.replace(".png", "_out_std.png")


def ensemble_document(records, samples):
    """``ensemble.json``: ``records`` = ``[(input file name, mean file name, std file name, {"mean_std", "max_std"})]`` in run order
    -> ``{"samples": K, "files": {input file: {"mean", "std", "mean_std", "max_std"}}, "mean_std": mean over the files}`` (the
    statistics in 8-bit units)."""
    files = {name: {"mean": mean, "std": std, "mean_std": st["mean_std"], "max_std": st["max_std"]} for name, mean, std, st in records}
    return {"samples": samples, "files": files, "mean_std": sum(st["mean_std"] for *_, st in records) / len(records)}


def pil_to_u8_tensor(image):
    """A PIL image as the uint8 ``[H,W,3]`` tensor it is saved as."""
    return torch.from_numpy(np.asarray(image.convert("RGB"), dtype=np.uint8).copy())


def sample_output_name(file_name, k):
    """``--samples``: output file name of sample k of an input file: sample 0 keeps the reference's ``<name>_out.png``, sample
    k >= 1 is ``<name>_out_s<k>.png``."""
    return os.path.basename(file_name).replace(".png", "_out.png" if k == 0 else f"_out_s{k}.png")


def seed_everything(seed):
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)


def pil_to_unit_tensor(image: Image.Image) -> torch.Tensor:
    """ToTensor: HWC uint8 -> CHW float32 / 255."""
    arr = np.asarray(image.convert("RGB"), dtype=np.uint8)
    return torch.from_numpy(arr.copy()).permute(2, 0, 1).to(torch.float32).div(255.0)


def unit_tensor_to_pil(t: torch.Tensor) -> Image.Image:
    """ToPILImage on a float tensor: mul(255) then byte() (truncation, not rounding)."""
    arr = t.detach().cpu().mul(255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
    return Image.fromarray(arr, "RGB")


def upsample_bicubic_on_device(image: Image.Image, scale: int, device) -> torch.Tensor:
    """``T.Resize((h*scale, w*scale), BICUBIC)`` + ``ToTensor`` of the reference (inference.py:66-73) as integer HIP
    kernels: the LR image goes to the GPU as uint8 HWC, the [1,3,H,W] condition comes out resident in HBM, bit-identical
    to ``pil_to_unit_tensor(image.resize(..., Image.BICUBIC))``."""
    import ctypes as C

    from . import _lib
    arr = np.asarray(image.convert("RGB"), dtype=np.uint8)
    h, w, _ = arr.shape
    src = torch.from_numpy(arr.copy()).to(device)
    dst = torch.empty(1, 3, h * scale, w * scale, device=device, dtype=torch.float32)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().srgd_image_resize_bicubic_u8(C.c_void_p(src.data_ptr()), h, w, h * scale, w * scale,
                                                          C.c_void_p(dst.data_ptr()),
                                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "srgd_image_resize_bicubic_u8")
    return dst


def unit_tensor_to_u8_on_device(t: torch.Tensor) -> torch.Tensor:
    """``mul(255).byte()`` of ``ToPILImage`` (inference.py:93) as a HIP kernel: [3,H,W] fp32 in [0,1] -> [H,W,3] uint8, on the GPU."""
    import ctypes as C

    from . import _lib
    t = t.contiguous()
    _, h, w = t.shape
    out = torch.empty(h, w, 3, device=t.device, dtype=torch.uint8)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().srgd_image_unit_to_u8(C.c_void_p(t.data_ptr()), h, w, C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "srgd_image_unit_to_u8")
    return out


def unit_tensor_to_pil_on_device(t: torch.Tensor) -> Image.Image:
    """``ToPILImage`` on the GPU: only the uint8 HWC image crosses PCIe (1/4 of the bytes)."""
    return Image.fromarray(unit_tensor_to_u8_on_device(t).cpu().numpy(), "RGB")


def _tiled_sample_kw(opts):
    """``tiled_sample``'s keywords out of the arguments of a ``sr_target_image*`` function (its ``locals()``, taken before it binds
    anything else; a function that lacks one of them fails on its first call): the reference's own as they are, an engine extension
    only where it is not at its default - so a run without a flag makes the call it made before the flag existed."""
    own = ("cond_scale", "guidance_start_steps", "class_cond_scale", "class_guidance_start_steps", "generation_start_steps", "num_sample_steps")
    return {**{k: opts[k] for k in own}, "amp": opts["enable_amp"], **_color_fix_kw(opts["color_fix"]),
            **_reference_kw(opts["reference"], opts["crop_border"]), **_back_project_kw(opts["back_project"]),
            **_guidance_kw(opts["consistency_guidance"], opts["consistency_guidance_start_steps"]),
            **_sampler_kw(opts["sampler"], opts["eta"], opts["step_spacing"]), **_threshold_kw(opts["dynamic_threshold"]),
            **_joint_kw(opts["joint_guidance"]), **_region_kw(opts["region_known"], opts["regions"])}


def _sample_group(sr_model, condition_x, sizes, label, batch_size, seeds, opts):
    """The one body of the four ``sr_target_image*`` functions: the reference's per-image reseed, one ``tiled_sample`` call on
    ``condition_x`` (a ``[B,3,H,W]`` tensor or a list of ``[1,3,H,W]`` tensors; ``seeds``: None or one noise seed per image) and the
    outputs as PIL images, each x4 of its entry of ``sizes`` -> ``(images, metric dicts or None)``."""
    seed_everything(opts["seed"])
    sr_model.device_noise_seed = opts["seed"]
    with torch.inference_mode():
        output = sr_model.tiled_sample(batch_size=batch_size, condition_x=condition_x, class_label=label,
                                       **({} if seeds is None else {"seeds": list(seeds)}), **_tiled_sample_kw(opts))
    output, quality = _split_quality(output, opts["reference"])
    outs = [unit_tensor_to_pil_on_device(o[0] if o.dim() == 4 else o) for o in output]
    assert len(outs) == len(sizes) and all(o.size == (w * 4, h * 4) for o, (w, h) in zip(outs, sizes))
    return outs, quality


def sr_target_image(image, sr_model, scale=4, batch_size=8, test_label=2, cond_scale=1.0, guidance_start_steps=0,
                    class_cond_scale=1.0, class_guidance_start_steps=0, generation_start_steps=0,
                    num_sample_steps=250, enable_amp=False, interpolation="bicubic", seed=71, color_fix=None, reference=None,
                    crop_border=4, back_project=0, consistency_guidance=0.0,
                    consistency_guidance_start_steps=0, sampler="ddpm", eta=None, step_spacing="time", dynamic_threshold=None,
                    joint_guidance=False, region_known=None, regions=None):
    """``reference`` (engine extension; here and in the three group forms below): the ground truth as a uint8 ``[H,W,3]`` tensor (a
    list of one per image in the group forms).  The return value is then ``(image(s), metric dicts)``: PSNR / SSIM of every image as
    saved, with ``crop_border`` pixels cut from every side (srgd_amd.metrics).
    ``region_known`` / ``regions`` (engine extension; here and in the three group forms below): the finished output as a fp32
    ``[1,3,4h,4w]`` tensor in [0, 1] (a list of one per image in the group forms) and the boxes to sample again
    (``tiled_sample(region_known=..., regions=...)``); without them the keywords are not passed at all."""
    opts = locals()
    # the reference maps 'lanczos' to bicubic too (inference.py:66-69)
    condition_x = upsample_bicubic_on_device(image, scale, sr_model.device)
    label = torch.LongTensor([test_label]).to(sr_model.device) if test_label is not None else None
    (sr_img,), quality = _sample_group(sr_model, condition_x, [image.size], label, batch_size, None, opts)
    return sr_img if reference is None else (sr_img, quality)


def sr_target_images(images, sr_model, scale=4, batch_size=8, test_label=2, cond_scale=1.0, guidance_start_steps=0,
                     class_cond_scale=1.0, class_guidance_start_steps=0, generation_start_steps=0,
                     num_sample_steps=250, enable_amp=False, interpolation="bicubic", seed=71, color_fix=None, reference=None,
                     crop_border=4, back_project=0, consistency_guidance=0.0,
                     consistency_guidance_start_steps=0, sampler="ddpm", eta=None, step_spacing="time", dynamic_threshold=None,
                     joint_guidance=False, region_known=None, regions=None):
    """``sr_target_image`` for several same-sized images in lock-step (engine extension): one ``tiled_sample`` call on a
    ``[B,3,H,W]`` condition.  Each image is sampled exactly as it would be alone after the reference's per-image
    ``seed_everything(seed)`` (inference.py:73) - bit-identical outputs - while their tiles fill the U-Net launches.
    ``test_label`` may be a sequence of one label per image."""
    opts = locals()
    assert len({im.size for im in images}) == 1, "lock-step images must have the same size"
    condition_x = torch.cat([upsample_bicubic_on_device(im, scale, sr_model.device) for im in images], 0)
    label = _label_tensor(test_label, len(images), sr_model.device)
    outs, quality = _sample_group(sr_model, condition_x, [im.size for im in images], label, batch_size * len(images), None, opts)
    return outs if reference is None else (outs, quality)


def sr_target_images_mixed(images, sr_model, scale=4, batch_size=8, test_label=2, cond_scale=1.0, guidance_start_steps=0,
                           class_cond_scale=1.0, class_guidance_start_steps=0, generation_start_steps=0,
                           num_sample_steps=250, enable_amp=False, interpolation="bicubic", seed=71, color_fix=None, reference=None,
                           crop_border=4, back_project=0, consistency_guidance=0.0,
                           consistency_guidance_start_steps=0, sampler="ddpm", eta=None, step_spacing="time", dynamic_threshold=None,
                           joint_guidance=False, region_known=None, regions=None):
    """``sr_target_image`` for several images of any sizes in lock-step (engine extension): one ``tiled_sample`` call on a list
    of conditions.  Each image comes out bit-identical to its own ``sr_target_image`` run (with its own label where
    ``test_label`` is a sequence of one label per image)."""
    opts = locals()
    conds = [upsample_bicubic_on_device(im, scale, sr_model.device) for im in images]
    label = _label_tensor(test_label, len(images), sr_model.device)
    outs, quality = _sample_group(sr_model, conds, [im.size for im in images], label, batch_size * len(images), None, opts)
    return outs if reference is None else (outs, quality)


def sr_target_images_seeded(images, seeds, sr_model, scale=4, batch_size=8, test_label=2, cond_scale=1.0, guidance_start_steps=0,
                            class_cond_scale=1.0, class_guidance_start_steps=0, generation_start_steps=0,
                            num_sample_steps=250, enable_amp=False, interpolation="bicubic", seed=71, color_fix=None,
                            reference=None, crop_border=4, back_project=0, consistency_guidance=0.0,
                            consistency_guidance_start_steps=0, sampler="ddpm", eta=None, step_spacing="time", dynamic_threshold=None,
                            joint_guidance=False, region_known=None, regions=None):
    """``sr_target_images_mixed`` with one noise seed per image (engine extension, ``tiled_sample(seeds=...)``): image i comes out
    bit-identical to its own ``sr_target_image`` run with ``seed=seeds[i]``; an image may appear several times with different
    seeds (each PIL image is upsampled once).  ``seed`` seeds the process as the other entry points do and is not a noise seed."""
    opts = locals()
    conds = {}
    for im in images:
        if id(im) not in conds:
            conds[id(im)] = upsample_bicubic_on_device(im, scale, sr_model.device)
    label = _label_tensor(test_label, len(images), sr_model.device)
    outs, quality = _sample_group(sr_model, [conds[id(im)] for im in images], [im.size for im in images], label,
                                  batch_size * len(images), seeds, opts)
    return outs if reference is None else (outs, quality)


def plan_sample_entries(file_names, output_dir, samples, seed):
    """``--samples K``: the grouping loop's entries ``(file name, save path, noise seed)`` in order - the K samples of a file are
    consecutive, sample k with seed ``seed + k``; an entry whose output file exists is left out (skip-if-exists per output file,
    so only the missing samples are drawn)."""
    entries = []
    for filename in file_names:
        for k in range(samples):
            save_path = os.path.join(output_dir, sample_output_name(filename, k))
            if os.path.exists(save_path):
                print("skip")
                continue
            entries.append((filename, save_path, seed + k))
    return entries


def try_open_image(image_path):
    try:
        return Image.open(image_path).convert("RGB")
    except (IOError, SyntaxError):
        return None


def try_open_image_with_alpha(image_path):
    """``try_open_image`` for ``--alpha keep``: ``(the RGB image, its alpha plane as uint8 [h,w] or None)`` - ``srgd_amd.alpha.alpha_of``
    of the decoded file - or ``(None, None)`` where the file cannot be opened."""
    try:
        image = Image.open(image_path)
        return image.convert("RGB"), alpha_of(image)
    except (IOError, SyntaxError):
        return None, None


def _u8_to_pil(t, mode="RGB"):
    """A uint8 ``[H,W,C]`` tensor, wherever it lives, as the PIL image that is saved."""
    return Image.fromarray(t.cpu().numpy(), mode)


def _upload_once(run, objects, as_tensor):
    """``objects`` as tensors on the model's device, one upload per distinct object: the K samples of a file share input and plane."""
    placed = {}
    for o in objects:
        if id(o) not in placed:
            placed[id(o)] = run.place(as_tensor(o))
    return [placed[id(o)] for o in objects]


@dataclass
class _Entry:
    """One image of a lock-step group: a sample of an input file or, under ``self_ensemble``, one orientation of it."""
    image: Image.Image                                   # what is sampled: the opened input (after alpha_bleed) or one orientation of it
    save_path: str
    label: object                                        # class label or None
    seed: int                                            # noise seed, the run's seed + k
    k: int                                               # sample index of --samples
    reference: object                                    # --reference_dir: future of the decoded ground truth, or None
    name: str                                            # base name of the input file
    file_name: str                                       # the input file as listed
    plane: object                                        # --alpha keep: the input's alpha plane, uint8 [h,w], or None
    op: int                                              # --self_ensemble: the dihedral op that made `image` of `original`
    original: Image.Image                                # the opened input (after alpha_bleed)
    known: object                                        # --region_known_dir: future of the decoded known output, or None


@dataclass
class _Run:
    """What one ``batch_sr_target_images`` call carries from group to group."""
    sr_model: object
    pool: object                                         # two workers: PNG encoding and decoding overlap the next group's sampling
    opt: SimpleNamespace                                 # the resolved options; kw: the keywords every sr_target_image* call gets
    device: object                                       # of the model; None for the stubs of the CPU tests
    pending: list = field(default_factory=list)          # the entries of the current lock-step group
    saves: list = field(default_factory=list)            # futures of the PNG writers
    file_records: list = field(default_factory=list)     # --reference_dir: (input file name, written file name, metric dict)
    ens_open: dict = field(default_factory=dict)         # --ensemble: input file -> [its K samples (PIL image of this run) or None (on disk), samples still to draw]
    ens_ready: list = field(default_factory=list)        # files whose last sample is handled
    ens_records: list = field(default_factory=list)      # ensemble.json rows
    ens_quality: list = field(default_factory=list)      # metrics.json rows of the mean images
    cons_records: list = field(default_factory=list)     # --consistency: consistency.json rows of the files written
    cons_ensemble: list = field(default_factory=list)    # and of the mean images
    held: dict = field(default_factory=dict)             # --self_ensemble: save path -> [(entry, output)] of the variants sampled so far

    def place(self, t):
        """``t`` on the model's device; as it is where the model has none."""
        return t if self.device is None else t.to(self.device)


def _queue(run, entry):
    """Adds an entry to the pending group and flushes as the grouping asks, in this order: an unlabelled image does not join a
    labelled group; with ``lockstep_tiles`` the image that would push the group over the tile budget (``plan_lockstep_groups``) closes
    it; otherwise a full group or an image of another size closes it, and the group that the entry fills is sampled at once."""
    opt = run.opt
    if run.pending and (entry.label is None) != (run.pending[0].label is None):
        _flush(run)
    if opt.lockstep_tiles is not None:
        hr = [(h * opt.scale, w * opt.scale) for (w, h) in [e.image.size for e in run.pending] + [entry.image.size]]
        if len(plan_lockstep_groups(hr, opt.lockstep_tiles)) > 1:
            _flush(run)
        run.pending.append(entry)
        return
    if run.pending and (len(run.pending) >= max(1, opt.lockstep) or run.pending[0].image.size != entry.image.size):
        _flush(run)
    run.pending.append(entry)
    if len(run.pending) >= max(1, opt.lockstep):
        _flush(run)


def _flush(run):
    """Samples the pending group and takes it through the stages, in this order: ``_sample_entries``, ``_merge_self_ensemble`` (only
    the entries whose last orientation arrived go on), ``_measure_consistency``, ``_outscale``, ``_attach_alpha``, ``_save`` and
    ``_flush_ensembles``."""
    if not run.pending:
        return
    entries = list(run.pending)
    outs = _sample_entries(run, entries)
    run.pending.clear()
    if run.opt.self_ensemble > 1:
        entries, outs = _merge_self_ensemble(run, entries, outs)
        if not entries:
            return
    if run.opt.consistency:                              # the images as saved against the inputs the group was given
        run.cons_records.extend(_measure_consistency(run, [(e.name, os.path.basename(e.save_path)) for e in entries],
                                                     [pil_to_u8_tensor(sr) for sr in outs], [e.image for e in entries]))
    if run.opt.outscale is not None:
        outs = _outscale(run, entries, outs)
    outs = _attach_alpha(run, entries, outs)
    _save(run, entries, outs)
    if run.opt.ensemble:
        _flush_ensembles(run)


def _sample_entries(run, entries):
    """Picks and calls the sampler: one entry is a solo run with its seed (``sr_target_image``: what every image of a group is
    identical to), entries with more than one distinct noise seed go to ``sr_target_images_seeded``, a ``lockstep_tiles`` group to
    ``sr_target_images_mixed``, any other to ``sr_target_images`` - each with ``opt.kw``, in which a keyword at its default is absent.
    ``reference_dir``: the decoded references (one future per input file) are handed on and the numbers of every file join
    ``file_records`` - not under ``self_ensemble``, where the merged image is measured.  ``regions``: the decoded known outputs (one
    future per known file) and the boxes are handed on."""
    opt, sr_model = run.opt, run.sr_model
    images, labels, seeds = [e.image for e in entries], [e.label for e in entries], [e.seed for e in entries]
    if opt.lockstep_tiles is not None:
        tiles = sum(even_step_tiles(h * opt.scale, w * opt.scale) for (w, h) in [im.size for im in images])
        print(f"lock-step group: {len(entries)} images, {tiles} tiles per even step")
    one_label = labels[0] if len(set(labels)) == 1 else labels
    extra = {}
    if opt.reference_dir is not None and opt.self_ensemble == 1:
        extra.update(reference=[e.reference.result() for e in entries], crop_border=opt.crop_border)
    if opt.regions is not None:
        extra.update(region_known=[e.known.result() for e in entries], regions=opt.regions)
    if len(entries) == 1:
        solo = {k: v[0] if k in ("reference", "region_known") else v for k, v in extra.items()}
        outs = sr_target_image(images[0], sr_model, test_label=labels[0], **dict(opt.kw, seed=seeds[0]), **solo)
        outs = ([outs[0]], outs[1]) if "reference" in extra else [outs]
    elif len(set(seeds)) > 1:
        outs = sr_target_images_seeded(images, seeds, sr_model, test_label=one_label, **opt.kw, **extra)
    elif opt.lockstep_tiles is not None:
        outs = sr_target_images_mixed(images, sr_model, test_label=one_label, **dict(opt.kw, seed=seeds[0]), **extra)
    else:
        outs = sr_target_images(images, sr_model, test_label=one_label, **dict(opt.kw, seed=seeds[0]), **extra)
    if "reference" in extra:
        outs, quality = outs
        run.file_records.extend((e.name, os.path.basename(e.save_path), q) for e, q in zip(entries, quality))
    return outs


def _merge_self_ensemble(run, entries, outs):
    """``self_ensemble`` N > 1: the outputs of an entry's orientations are held, across ``_flush`` calls where they straddle them,
    until the N-th arrives; the entries completed in one ``_flush`` are merged in one ``self_ensemble_on_device`` call (every output
    turned back, the N averaged, halves up) and, with ``reference_dir``, measured in one ``metrics_on_device`` call on ``mean01``.
    Returns what every later stage acts on: the completed entries, each with its original input as its image, and the merged images."""
    opt = run.opt
    for e, sr in zip(entries, outs):
        run.held.setdefault(e.save_path, []).append((e, sr))
    complete = [run.held.pop(path) for path in [path for path, parts in run.held.items() if len(parts) == opt.self_ensemble]]
    if not complete:
        return [], []
    merged = self_ensemble_on_device([[(run.place(pil_to_u8_tensor(sr)), e.op) for e, sr in parts] for parts in complete],
                                     return_mean01=opt.reference_dir is not None)
    entries = [replace(parts[0][0], image=parts[0][0].original) for parts in complete]
    if opt.reference_dir is not None:
        quality = metrics_on_device([m[1] for m in merged], [e.reference.result() for e in entries], opt.crop_border)
        run.file_records.extend((e.name, os.path.basename(e.save_path), q) for e, q in zip(entries, quality))
        merged = [m[0] for m in merged]
    return entries, [_u8_to_pil(m) for m in merged]


def _measure_consistency(run, tags, outputs, inputs):
    """One batched ``consistency_on_device`` call (srgd_amd.consistency: the output reduced x4 by Pillow's bicubic against its
    input): ``outputs`` uint8 [4h,4w,3] tensors, ``inputs`` the PIL inputs, ``tags`` a tuple per image that ends in its name ->
    ``[(*tag, record)]`` of the images large enough; a smaller one is reported and left out."""
    keep = []
    for i, im in enumerate(inputs):
        if min(im.size) < CONSISTENCY_MIN_SIDE:
            print(f"consistency: {tags[i][-1]} is {im.size[0]}x{im.size[1]}, smaller than {CONSISTENCY_MIN_SIDE} pixels on a side: "
                  "left out")
        else:
            keep.append(i)
    if not keep:
        return []
    lows = _upload_once(run, [inputs[i] for i in keep], pil_to_u8_tensor)
    recs = consistency_on_device([run.place(outputs[i]) for i in keep], lows)
    return [(*tags[i], rec) for i, rec in zip(keep, recs)]


def _outscale(run, entries, outs):
    """``outscale`` S other than None / 4: the images as they would have been saved, after everything above has been measured on them,
    go through one batched ``resize_on_device`` call (srgd_amd.resize: Pillow's ``Image.resize`` bit for bit) to ``outscale_size``."""
    from .resize import resize_on_device
    resized = resize_on_device([run.place(pil_to_u8_tensor(sr)) for sr in outs],
                               [outscale_size(e.image.size[1], e.image.size[0], run.opt.outscale) for e in entries], run.opt.outscale_filter)
    return [_u8_to_pil(t) for t in resized]


def _attach_alpha(run, entries, outs):
    """``alpha="keep"``: the outputs whose input had an alpha plane get it in one batched ``attach_alpha_on_device`` call
    (srgd_amd.alpha) and leave as RGBA images; the others, and every output of a run without planes, stay as they are."""
    with_alpha = [i for i, e in enumerate(entries) if e.plane is not None]
    if not with_alpha:
        return outs
    planes = _upload_once(run, [entries[i].plane for i in with_alpha], torch.from_numpy)
    rgba = attach_alpha_on_device([run.place(pil_to_u8_tensor(outs[i])) for i in with_alpha], planes, run.opt.scale, run.opt.outscale_filter)
    outs = list(outs)
    for i, t in zip(with_alpha, rgba):
        outs[i] = _u8_to_pil(t, "RGBA")
    return outs


def _save(run, entries, outs):
    """Hands every image to the writer pool and, with ``ensemble``, files it as sample ``k`` of its input; an input whose last sample
    this was is ready for ``_flush_ensembles``."""
    for e, sr in zip(entries, outs):
        run.saves.append(run.pool.submit(sr.save, e.save_path))
        if e.file_name in run.ens_open:
            state = run.ens_open[e.file_name]
            state[0][e.k] = sr
            state[1] -= 1
            if state[1] == 0:
                run.ens_ready.append(e.file_name)


def _plan_ensembles(run, file_names):
    """``ensemble``: what is left to do per input file.  A file whose samples, mean and spread all exist is skipped; one whose samples
    are all on disk - found by the skip-if-exists rule - is ready at once."""
    opt = run.opt
    for filename in file_names:
        paths = [os.path.join(opt.output_dir, sample_output_name(filename, k)) for k in range(opt.samples)]
        missing = sum(not os.path.exists(p) for p in paths)
        if missing == 0 and all(os.path.exists(os.path.join(opt.output_dir, n)) for n in ensemble_output_names(filename)):
            continue
        if missing == 0:
            run.ens_ready.append(filename)
        run.ens_open[filename] = [[None] * opt.samples, missing]


def _flush_ensembles(run):
    """``ensemble``: one batched ``ensemble_on_device`` call (srgd_amd.ensemble) for the files completed since the last one; their mean
    images and spread maps go to ``<name>_out_mean.png`` / ``<name>_out_std.png``.  Samples of this run are the PIL images the samplers
    returned, samples found on disk are decoded on the writer pool (a resumed run writes what an uninterrupted one does); one of another
    size than x``scale`` of the input is reported and that file left out.  ``reference_dir`` and ``consistency`` measure the mean images."""
    opt, pool = run.opt, run.pool
    todo = []                                            # (file name, futures / tensors of its K samples)
    for filename in run.ens_ready:
        drawn = run.ens_open.pop(filename)[0]
        todo.append((filename, [pool.submit(load_reference, os.path.join(opt.output_dir, sample_output_name(filename, k)))
                                if sr is None else pil_to_u8_tensor(sr) for k, sr in enumerate(drawn)]))
    run.ens_ready.clear()
    names, stacks = [], []
    for filename, parts in todo:
        size = _header_size(filename)
        if size is None:
            continue                                     # not an image: the sampling loop has reported it
        want = (size[1] * opt.scale, size[0] * opt.scale, 3)
        try:
            parts = [part if torch.is_tensor(part) else part.result() for part in parts]
        except (IOError, SyntaxError) as err:
            print(f"ensemble: a sample of {os.path.basename(filename)} cannot be read ({err}): no ensemble for this file")
            continue
        wrong = [k for k, part in enumerate(parts) if tuple(part.shape) != want]
        if wrong:
            for k in wrong:
                print(f"ensemble: {sample_output_name(filename, k)} is {parts[k].shape[1]}x{parts[k].shape[0]}, x{opt.scale} of the "
                      f"input is {want[1]}x{want[0]}: no ensemble for {os.path.basename(filename)}")
            continue
        names.append(filename)
        stacks.append(torch.stack(parts))
    if not names:
        return
    results = ensemble_on_device([run.place(st) for st in stacks], return_mean01=opt.reference_dir is not None)
    if opt.reference_dir is not None:
        refs = [pool.submit(load_reference, os.path.join(opt.reference_dir, os.path.basename(f))) for f in names]
        quality = metrics_on_device([r[3] for r in results], [f.result() for f in refs], opt.crop_border)
        run.ens_quality.extend((os.path.basename(f), q) for f, q in zip(names, quality))
    if opt.consistency:                                  # the uint8 mean images against their inputs
        lows = [try_open_image(f) for f in names]
        have = [i for i, im in enumerate(lows) if im is not None]
        run.cons_ensemble.extend(_measure_consistency(run, [(os.path.basename(names[i]),) for i in have], [results[i][0] for i in have],
                                                      [lows[i] for i in have]))
    for filename, res in zip(names, results):
        mean_name, std_name = ensemble_output_names(filename)
        for arr, out_name in ((res[0], mean_name), (res[1], std_name)):
            run.saves.append(pool.submit(_u8_to_pil(arr).save, os.path.join(opt.output_dir, out_name)))
        run.ens_records.append((os.path.basename(filename), mean_name, std_name, res[2]))


def _write_document(path, doc):
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def batch_sr_target_images(input_dir, output_dir, sr_model, scale=4, batch_size=8, test_label=2, cond_scale=1.0,
                           guidance_start_steps=0, class_cond_scale=1.0, class_guidance_start_steps=0,
                           generation_start_steps=0, num_sample_steps=250, start_index=0, end_index=None,
                           enable_amp=False, interpolation="bicubic", seed=71, lockstep=1, lockstep_tiles=None, labels=None,
                           samples=1, color_fix=None, reference_dir=None, crop_border=4, metrics_name="metrics.json", ensemble=False,
                           ensemble_name="ensemble.json", consistency=False, consistency_name="consistency.json", back_project=0,
                           consistency_guidance=0.0, consistency_guidance_start_steps=0, sampler="ddpm", eta=None,
                           step_spacing="time", outscale=None, outscale_filter="bicubic", alpha="drop", alpha_bleed=0,
                           dynamic_threshold=0.0, self_ensemble=1, joint_guidance=False, region_known_dir=None, regions=None):
    """The folder driver.  Every argument is checked first: a bad value or an excluded combination is a ``ValueError``, a missing or
    misshapen ground truth or known output a ``SystemExit`` (``check_references``, ``check_region_known``), before anything is sampled.
    Then every planned entry (``plan_sample_entries``: ``samples`` noise seeds ``seed, seed + 1, ...`` per file, skip-if-exists per
    output file; ``labels``: ``{file name: label}`` for the files that do not take ``test_label``) is opened and queued.  The entries of
    a file share what is made once per opened file: the decoded image, its alpha plane and the bled image (``alpha="keep"``,
    ``alpha_bleed``), the future of its ground truth (``reference_dir``), its N orientations (``self_ensemble``: N consecutive entries
    per sample, the ops of ``srgd_amd.selfens.OPS[N]`` in order) and the future of its known output (``region_known_dir``).
    ``_queue`` decides where a lock-step group ends and ``_flush`` takes the group through the stages, in this order:
    ``_sample_entries``, ``_merge_self_ensemble``, ``_measure_consistency``, ``_outscale``, ``_attach_alpha``, ``_save``,
    ``_flush_ensembles``.  Last, where at least one file was sampled, ``metrics_name`` (``reference_dir``), ``consistency_name``
    (``consistency``) and ``ensemble_name`` (``ensemble``) are written.  A switch at its default loads no library, launches nothing
    and writes nothing; with neither lock-step argument ``samples`` and ``self_ensemble`` group as ``lockstep = self_ensemble * samples``."""
    self_ensemble = check_self_ensemble(self_ensemble)
    if self_ensemble > 1 and isinstance(sr_model, ConditionalElucidatedDiffusionSR):
        raise ValueError("self_ensemble: the orientations of an image are sampled in lock-step with per-image noise seeds, which is "
                         "built for the DDPM sampler only; this model samples with EDM")
    print(f"save images at: {output_dir}")
    os.makedirs(output_dir, exist_ok=True)
    labels = labels or {}
    if self_ensemble > 1 and lockstep_tiles is None and lockstep <= 1:
        lockstep = self_ensemble * samples
    if samples > 1 and lockstep_tiles is None and lockstep <= 1:
        lockstep = samples
    kw = dict(scale=scale, batch_size=batch_size, cond_scale=cond_scale,
              guidance_start_steps=guidance_start_steps, class_cond_scale=class_cond_scale,
              class_guidance_start_steps=class_guidance_start_steps, generation_start_steps=generation_start_steps,
              num_sample_steps=num_sample_steps, enable_amp=enable_amp, interpolation=interpolation, seed=seed,
              color_fix=None if color_fix in (None, "none") else color_fix, **_back_project_kw(back_project),
              **_guidance_kw(consistency_guidance, consistency_guidance_start_steps), **_sampler_kw(sampler, eta, step_spacing),
              **_threshold_kw(dynamic_threshold), **_joint_kw(joint_guidance))
    check_sampler(sampler or "ddpm", eta, step_spacing or "time")
    check_percentile(dynamic_threshold)
    outscale, outscale_filter = check_outscale(outscale), check_filter(outscale_filter)
    if ensemble and outscale is not None:
        raise ValueError("ensemble: not together with outscale")
    alpha, alpha_bleed = check_mode(alpha), check_bleed(alpha_bleed)
    if alpha_bleed and alpha != "keep":
        raise ValueError("alpha_bleed: needs alpha=\"keep\"")
    if ensemble and alpha == "keep":
        raise ValueError("ensemble: not together with alpha=\"keep\"")
    file_names = sorted(glob.glob(f"{input_dir}/*"))[start_index:end_index]
    if consistency_guidance:                             # the guidance kernels take inputs of 5 x 5 pixels and more
        for filename in file_names:
            image = try_open_image(filename)
            if image is not None and min(image.size) < GUIDANCE_MIN_SIDE:
                raise ValueError(f"consistency_guidance: {os.path.basename(filename)} is {image.size[0]}x{image.size[1]}, smaller than "
                                 f"{GUIDANCE_MIN_SIDE} pixels on a side")
    if reference_dir is not None:
        check_references(file_names, reference_dir, scale, crop_border)
    if (region_known_dir is None) != (regions is None):
        raise ValueError("region_known_dir and regions go together")
    if regions is not None:
        if self_ensemble > 1 or ensemble:
            raise ValueError("region_known_dir: not together with self_ensemble or ensemble")
        regions = [parse_region(",".join(str(v) for v in box)) for box in regions]
        if not 1 <= len(regions) <= REGION_MAX_BOXES:
            raise ValueError(f"regions: 1 .. {REGION_MAX_BOXES} boxes, got {len(regions)}")
        check_region_known(file_names, region_known_dir, regions, scale, samples)
    if ensemble and not 2 <= samples <= 256:
        raise ValueError("ensemble: samples must be in 2..256")
    opt = SimpleNamespace(scale=scale, lockstep=lockstep, lockstep_tiles=lockstep_tiles, samples=samples, output_dir=output_dir,
                          reference_dir=reference_dir, crop_border=crop_border, self_ensemble=self_ensemble, regions=regions,
                          consistency=consistency, outscale=outscale, outscale_filter=outscale_filter, ensemble=ensemble, kw=kw)
    with ThreadPoolExecutor(max_workers=2) as pool:      # PNG encoding overlaps the next group's sampling
        run = _Run(sr_model, pool, opt, getattr(sr_model, "device", None))
        if ensemble:
            _plan_ensembles(run, file_names)
        opened, original, plane, ref, variants = None, None, None, None, None      # shared by every entry of the opened file
        known_open = (None, None)                        # --region_known_dir: (the known file last opened, its decoding future)
        for filename, save_path, noise_seed in plan_sample_entries(file_names, output_dir, samples, seed):
            name, k = os.path.basename(filename), noise_seed - seed
            if opened != filename:
                opened, ref = filename, None
                original, plane = try_open_image_with_alpha(filename) if alpha == "keep" else (try_open_image(filename), None)
                if original is None:
                    print("Invalid image or unable to open image:", filename)
                    continue
                if plane is not None and alpha_bleed:    # the bled image is the input from here on
                    rgba = torch.from_numpy(np.dstack([np.asarray(original, dtype=np.uint8), plane]))
                    original = _u8_to_pil(bleed_on_device([run.place(rgba)], alpha_bleed)[0])
                if reference_dir is not None:            # decoded on the pool while the groups before this one sample
                    ref = pool.submit(load_reference, os.path.join(reference_dir, name))
                variants = [original]
                if self_ensemble > 1:                    # the input in every orientation
                    turned = dihedral_on_device([run.place(pil_to_u8_tensor(original))] * self_ensemble, list(SELF_ENSEMBLE_OPS[self_ensemble]))
                    variants = [_u8_to_pil(t) for t in turned]
            elif original is None:
                continue
            known = None
            if regions is not None:                      # decoded on the pool; the samples that start from one file share it
                known_file = region_known_path(region_known_dir, filename, k, samples)
                if known_open[0] != known_file:
                    known_open = (known_file, pool.submit(load_region_known, known_file))
                known = known_open[1]
            for op, image in zip(SELF_ENSEMBLE_OPS[self_ensemble], variants):
                _queue(run, _Entry(image=image, save_path=save_path, label=labels.get(name, test_label), seed=noise_seed, k=k, reference=ref,
                                   name=name, file_name=filename, plane=plane, op=op, original=original, known=known))
        _flush(run)
        if ensemble:
            _flush_ensembles(run)
        for f in run.saves:
            f.result()                                   # surface write errors
    if run.file_records:                                 # --reference_dir, and at least one file was sampled in this run
        _write_document(os.path.join(output_dir, metrics_name),
                        metrics_document(run.file_records, samples, crop_border, **({"ensemble": run.ens_quality} if run.ens_quality else {})))
    if run.cons_records:                                 # --consistency, and at least one file was sampled in this run
        _write_document(os.path.join(output_dir, consistency_name),
                        consistency_document(run.cons_records, samples, **({"ensemble": run.cons_ensemble} if run.cons_ensemble else {})))
    if run.ens_records:                                  # --ensemble, and at least one file's ensemble was taken in this run
        _write_document(os.path.join(output_dir, ensemble_name), ensemble_document(run.ens_records, samples))


def rank_file_range(n_files, start_index, end_index, rank, world):
    """The reference parallelises by hand: one process per GPU with its own ``--start_index/--end_index`` (inference.py:36-37,
    :120).  Under a launcher that sets RANK / WORLD_SIZE (``torchrun --nproc-per-node 8 inference.py ...``) the selected range
    ``[start_index:end_index]`` is cut into ``world`` contiguous slices instead - contiguous, so that ``--lockstep`` groups of
    neighbouring same-sized images survive - and this returns rank's ``(start, end)``.  No collective is involved."""
    lo, hi, _ = slice(start_index, end_index).indices(n_files)
    n = max(0, hi - lo)
    per, rem = divmod(n, world)
    a = lo + rank * per + min(rank, rem)
    return a, a + per + (1 if rank < rem else 0)


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format="[%(levelname)s %(asctime)s] %(message)s")
    args = parse_args(argv)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if args.reference_dir is not None:                   # every rank checks the whole selection, before the model is built
        check_references(sorted(glob.glob(f"{args.input_dir}/*"))[args.start_index:args.end_index], args.reference_dir, 4,
                         args.crop_border)
    if args.region_known_dir is not None:                # likewise: every known output and every box, before the model is built
        check_region_known(sorted(glob.glob(f"{args.input_dir}/*"))[args.start_index:args.end_index], args.region_known_dir,
                           args.region, 4, args.samples)
    conf = load_config(args.conf)
    if args.region_known_dir is not None and conf.model == "conditional_elucidated":
        raise SystemExit("--region_known_dir: region resampling is built for the DDPM sampler (model: conditional_continuous) only; "
                         "this config samples with EDM")
    if args.self_ensemble > 1 and conf.model == "conditional_elucidated":     # before the model is built
        raise SystemExit("--self_ensemble: the orientations of an image are sampled in lock-step with per-image noise seeds, which is "
                         "built for the DDPM sampler (model: conditional_continuous) only; this config samples with EDM - run "
                         "without it")
    if args.precision_schedule is not None and conf.model == "conditional_elucidated":   # before the model is built
        raise SystemExit("--precision_schedule: a precision per step is built for the DDPM sampler (model: conditional_continuous) "
                         "only; this config samples with EDM - use --precision")
    conf.num_sample_steps = args.num_sample_steps
    conf.ckpt_path = args.ckpt_path
    ema_model = get_model(conf, logger)
    if not torch.cuda.is_available():
        raise SystemExit("srgd_amd needs an MI355X: no GPU visible and there is no CPU fallback")
    if world > 1:                                        # one process per GPU, each with its own slice of the input files
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
        n_files = len(glob.glob(f"{args.input_dir}/*"))
        args.start_index, args.end_index = rank_file_range(n_files, args.start_index, args.end_index, rank, world)
        print(f"rank {rank}/{world}: files [{args.start_index}:{args.end_index}] of {n_files}")
    sr_model = ema_model.module.eval().to(torch.device("cuda", torch.cuda.current_device()))
    if args.lockstep_tiles is not None and isinstance(sr_model, ConditionalElucidatedDiffusionSR):
        raise SystemExit("--lockstep_tiles: mixed-size lock-step is built for the DDPM sampler (model: conditional_continuous) only; "
                         "this config samples with EDM - use --lockstep N for same-sized images")
    if args.samples > 1 and isinstance(sr_model, ConditionalElucidatedDiffusionSR):
        raise SystemExit("--samples: per-image noise seeds are built for the DDPM sampler (model: conditional_continuous) only; "
                         "this config samples with EDM - run once per --seed instead")
    sr_model.noise_source = "device" if args.device_noise else "host"
    sr_model.precision = args.precision
    precisions = [args.precision]                        # the engines to pack: with a schedule, those of its executed steps
    if args.precision_schedule is not None:              # --precision is then not used
        sr_model.precision_schedule = args.precision_schedule
        precisions = executed_names(args.precision_plan, args.generation_start_steps)
        print(f"engine precision schedule: {describe_plan(args.precision_plan)} (noise: {sr_model.noise_source})")
    else:
        print(f"engine precision: {args.precision} (noise: {sr_model.noise_source})")
    if args.precision_schedule is None and args.amp and args.precision in ("fp32", "f16x3", "f16mx2"):
        # callers of earlier builds got bf16 from amp=True; upstream's sampler ignores amp and so does this one
        print("note: amp is accepted and ignored as upstream (the sampler computes at fp32 accuracy: f16x3 ~3.4x, fp32 ~10x slower "
              "than the bf16 engine); pass --precision bf16 for the throughput mode")
    import time
    t_pack = time.perf_counter()
    unet = getattr(sr_model, "model", None) or sr_model.net
    from .lanes import AUTO_LANE_PRECISIONS
    for name in precisions:
        unet.engine(name)                               # pack + upload the weights now, not inside the first image
        if (sr_model.step_lanes is None and name in AUTO_LANE_PRECISIONS) or (sr_model.step_lanes or 1) > 1:
            # small steps run as two concurrent halves through a second engine instance (srgd_amd.lanes: a second copy of the packed
            # weights, scratch and graphs): built here, not inside the first image's sampling loop
            unet.engine(name, lane=1)
    torch.cuda.synchronize()
    print(f"engine ready: {len(sr_model.state_dict())} tensors packed and uploaded in {time.perf_counter() - t_pack:.2f} s")
    print(args)
    batch_sr_target_images(args.input_dir, args.output_dir, sr_model, scale=4, batch_size=args.batch_size,
                           test_label=args.test_label, cond_scale=args.cond_scale,
                           guidance_start_steps=args.guidance_start_steps, class_cond_scale=args.class_cond_scale,
                           class_guidance_start_steps=args.class_guidance_start_steps,
                           generation_start_steps=args.generation_start_steps,
                           num_sample_steps=args.num_sample_steps, start_index=args.start_index,
                           end_index=args.end_index, enable_amp=args.amp, interpolation=args.interpolation,
                           seed=args.seed, lockstep=args.lockstep, lockstep_tiles=args.lockstep_tiles, labels=args.labels,
                           samples=args.samples, color_fix=args.color_fix, reference_dir=args.reference_dir,
                           crop_border=args.crop_border, metrics_name="metrics.json" if world == 1 else f"metrics_rank{rank}.json",
                           ensemble=args.ensemble, ensemble_name="ensemble.json" if world == 1 else f"ensemble_rank{rank}.json",
                           consistency=args.consistency, back_project=args.back_project,
                           consistency_guidance=args.consistency_guidance,
                           consistency_guidance_start_steps=args.consistency_guidance_start_steps,
                           sampler=args.sampler, eta=args.eta, step_spacing=args.step_spacing,
                           outscale=args.outscale, outscale_filter=args.outscale_filter, alpha=args.alpha,
                           alpha_bleed=args.alpha_bleed, dynamic_threshold=args.dynamic_threshold,
                           **({"self_ensemble": args.self_ensemble} if args.self_ensemble > 1 else {}),
                           **_joint_kw(args.joint_guidance),
                           **({"region_known_dir": args.region_known_dir, "regions": args.region} if args.region else {}),
                           consistency_name="consistency.json" if world == 1 else f"consistency_rank{rank}.json")


if __name__ == "__main__":
    main()
