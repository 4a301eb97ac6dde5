"""Host-side mirror of the reference's ``model.py`` surface for the ONE shipped sampling path
(``model: conditional_continuous``), backed by the MI355X engine (``libsrgd_hip.so``).

Kept identical to the reference so that callers and checkpoints switch over unchanged:
  * ``get_model(conf, logger)`` (reference model.py:3500-3666) -> object with ``.module``
  * ``ConditionalSRUnet(...)`` constructor signature (model.py:537-556) and ``state_dict`` keys/shapes
     - the published ``.pth`` loads with ``strict=True``
  * ``ConditionalContinuousTimeGaussianDiffusionSR.tiled_sample(...)`` signature, return value and
    error behaviour (model.py:3288-3413)
  * the pure-int tiling helpers ``get_coord_and_pad / get_coords / get_area`` (model.py:116-179)

The modules below hold parameters only; they have no PyTorch implementation of the arithmetic.
All compute runs in hand-written gfx950 kernels; calling this path without a GPU raises.
"""
from __future__ import annotations

import copy
import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._lib import SamplerGeometry, StepScalars
from .backproject import back_project_flat, check_hr_sizes, check_iterations
from .colorfix import check_mode, color_fix_flat
from .metrics import check_sizes, metrics_flat, pack_references
from .engine import HipEngine
from .guidance import check_start_steps, check_weight, guide_step_flat
from .guidance import check_hr_sizes as check_guided_sizes
from .guidance import records as guidance_records
from .guidance import scratch_bytes as guidance_scratch_bytes
from .solver import check_sampler, history_step_flat, history_weights, is_default, step_coefficients
from .solver import records as solver_records
from .threshold import check_percentile, threshold_step_flat
from .threshold import records as threshold_records
from .threshold import scratch_bytes as threshold_scratch_bytes
from .lanes import StepLanes, lanes_setting_from_env, lanes_wanted
from .precision_schedule import executed_names, parse_schedule, plan_steps
from .region import RegionImage, _RegionRun, check_region_args

__all__ = ["get_coord_and_pad", "get_coords", "get_area", "beta_linear_log_snr", "ConditionalSRUnet",
           "ConditionalContinuousTimeGaussianDiffusionSR", "ConditionalElucidatedDiffusionSR", "ModelEma", "get_model"]


# ---------------------------------------------------------------------------------------------
# tiling geometry (pure ints; reference model.py:116-179)
# ---------------------------------------------------------------------------------------------
def _host_randn(generator, *shape):
    """Host-noise draw: ``torch.randn`` on the CPU generator the reference draws from (global unless one is given)."""
    return torch.randn(*shape, generator=generator)


def get_coord_and_pad(height: int, width: int, tile_size: int = 256):
    """Canvas size and placement of an ``height x width`` image: one tile if it fits, otherwise the
    size rounded up to whole tiles plus one extra tile (half a tile of margin per side)."""
    fits = height <= tile_size and width <= tile_size
    canvas_h = tile_size if fits else tile_size * (math.ceil(height / tile_size) + 1)
    canvas_w = tile_size if fits else tile_size * (math.ceil(width / tile_size) + 1)
    left, top = (canvas_w - width) // 2, (canvas_h - height) // 2
    coord = (left, top, left + width, top + height)
    pad = (left, canvas_w - width - left, top, canvas_h - height - top)
    return coord, pad


def _axis_starts(extent: int, tile_size: int, tile_stride: int) -> List[int]:
    starts = list(range(0, extent - tile_size + 1, tile_stride))
    if (extent - tile_size) % tile_stride:
        starts.append(extent - tile_size)      # last tile is pulled back to end at the border
    return starts


def get_coords(h: int, w: int, tile_size: int, tile_stride: int, diff: int = 0):
    """Row-major list of tile boxes ``(hs, he, ws, we)``, each shifted by ``diff``."""
    return [(y + diff, y + diff + tile_size, x + diff, x + diff + tile_size)
            for y in _axis_starts(h, tile_size, tile_stride) for x in _axis_starts(w, tile_size, tile_stride)]


def get_area(coords, height: int, width: int):
    """Bounding box ``(left, top, right, bottom)`` of a tile list and its margins inside the canvas."""
    top = min([height] + [c[0] for c in coords])
    bottom = max([0] + [c[1] for c in coords])
    left = min([width] + [c[2] for c in coords])
    right = max([0] + [c[3] for c in coords])
    return (left, top, right, bottom), (left, width - right, top, height - bottom)


# ---------------------------------------------------------------------------------------------
# schedule scalars: host-side fp32 torch ops in the reference's own order, so the numbers handed
# to the kernels are bit-identical to what the reference computes (model.py:2629-2633, :3127-3134)
# ---------------------------------------------------------------------------------------------
def beta_linear_log_snr(t: torch.Tensor) -> torch.Tensor:
    return -torch.log(torch.special.expm1(1e-4 + 10 * (t ** 2)).clamp(min=1e-20))


def _log_snr_levels(num_steps: int, step_spacing: str = "time") -> List[torch.Tensor]:
    """The N + 1 fp32 log-SNR levels of a run (0-dim tensors): step i goes from level i to level i + 1.  "time": the levels of
    ``linspace(1, 0, N + 1)`` in t, each computed as ``_schedule`` computes it; "logsnr": uniform in the log-SNR itself."""
    if step_spacing == "logsnr":
        levels = torch.linspace(float(beta_linear_log_snr(torch.tensor(1.0))), float(beta_linear_log_snr(torch.tensor(0.0))),
                                num_steps + 1)
        return [levels[i] for i in range(num_steps + 1)]
    times = torch.linspace(1.0, 0.0, num_steps + 1)
    return [beta_linear_log_snr(times[i]) for i in range(num_steps + 1)]


def _schedule(num_steps: int, sampler: str = "ddpm", eta: Optional[float] = None,
              step_spacing: str = "time") -> Tuple[List[StepScalars], List[float]]:
    """The step table and the log-SNR the U-Net is conditioned on at every step.  Called with ``num_steps`` alone: the reference's
    ancestral step on its uniform times.  ``step_spacing="logsnr"`` takes the steps' ends from ``_log_snr_levels``; ``sampler``
    "ddim" (``eta`` in [0, 1]) and "dpmpp2m" (eta 0) replace ``one_minus_c``, ``c`` and ``noise_scale`` - the three scalars the step
    kernel reads independently - by fp32(A alpha / alpha_next), fp32(B / alpha_next) and fp32(S) of srgd_amd.solver's float64
    ``step_coefficients``, so that the kernel's ``alpha_next * (x_t * one_minus_c / alpha + c * x0) + noise_scale * z`` is
    ``A x_t + B x0 + S z``; ``alpha_next * c`` is then B, the weight of x0 the guidance reads.  ``no_clamp`` stays 0 here: the
    clamped step (``_schedule_of`` sets it on every step of a run with the dynamic threshold)."""
    times = torch.linspace(1.0, 0.0, num_steps + 1)
    levels = _log_snr_levels(num_steps, step_spacing) if step_spacing != "time" else None
    scalars, log_snrs = [], []
    for i in range(num_steps):
        ls, ls_next = (beta_linear_log_snr(times[i]), beta_linear_log_snr(times[i + 1])) if levels is None else (levels[i], levels[i + 1])
        c = -torch.special.expm1(ls - ls_next)
        alpha, sigma = ls.sigmoid().sqrt(), (-ls).sigmoid().sqrt()
        alpha_next = ls_next.sigmoid().sqrt()
        var = (-ls_next).sigmoid() * c
        s = StepScalars()
        s.alpha, s.sigma, s.alpha_next, s.c = float(alpha), float(sigma), float(alpha_next), float(c)
        s.one_minus_c = float(1 - c)
        s.noise_scale = float(var.sqrt())
        s.sigma_next = float((-ls_next).sigmoid().sqrt())
        if sampler != "ddpm":
            a_, b_, s_ = step_coefficients(float(ls), float(ls_next), eta or 0.0)
            s.one_minus_c, s.c, s.noise_scale = a_ * s.alpha / s.alpha_next, b_ / s.alpha_next, s_
        scalars.append(s)
        log_snrs.append(float(ls))
    return scalars, log_snrs


# ---------------------------------------------------------------------------------------------
# parameter containers (names/shapes = the reference state_dict; no forward)
# ---------------------------------------------------------------------------------------------
class _Params(nn.Module):
    def forward(self, *a, **k):
        raise RuntimeError("parameter container: the arithmetic of this layer lives in libsrgd_hip.so")


class _Gain(_Params):                                   # RMSNorm.g [1,C,1,1]
    def __init__(self, c):
        super().__init__()
        self.g = nn.Parameter(torch.ones(1, c, 1, 1))


class _FourierFreqs(_Params):                           # RandomOrLearnedSinusoidalPosEmb.weights [half]
    def __init__(self, dim, frozen):
        super().__init__()
        self.weights = nn.Parameter(torch.randn(dim // 2), requires_grad=not frozen)


class _ConvNormAct(_Params):                            # Block: proj + norm
    def __init__(self, cin, cout, groups):
        super().__init__()
        self.proj = nn.Conv2d(cin, cout, 3, padding=1)
        self.norm = nn.GroupNorm(groups, cout)


class _Residual(_Params):                               # ResnetBlock
    def __init__(self, cin, cout, time_dim, groups):
        super().__init__()
        self.mlp = nn.Sequential(nn.SiLU(), nn.Linear(time_dim, cout * 2))
        self.block1 = _ConvNormAct(cin, cout, groups)
        self.block2 = _ConvNormAct(cout, cout, groups)
        self.res_conv = nn.Conv2d(cin, cout, 1) if cin != cout else nn.Identity()


class _LinearAttn(_Params):
    def __init__(self, c, heads, dim_head):
        super().__init__()
        self.norm = _Gain(c)
        self.to_qkv = nn.Conv2d(c, heads * dim_head * 3, 1, bias=False)
        self.to_out = nn.Sequential(nn.Conv2d(heads * dim_head, c, 1), _Gain(c))


class _SoftmaxAttn(_Params):
    def __init__(self, c, heads, dim_head):
        super().__init__()
        self.norm = _Gain(c)
        self.to_qkv = nn.Conv2d(c, heads * dim_head * 3, 1, bias=False)
        self.to_out = nn.Conv2d(heads * dim_head, c, 1)


class _ShuffleUp(_Params):                              # PixelShuffleUpsample: conv1x1 -> SiLU -> PixelShuffle(2)
    def __init__(self, cin, cout):
        super().__init__()
        conv = nn.Conv2d(cin, cout * 4, 1)
        # ICNR-style start: the four sub-pixel filters of each output channel begin identical
        base = torch.empty(cout, cin, 1, 1)
        nn.init.kaiming_uniform_(base)
        with torch.no_grad():
            conv.weight.copy_(base.repeat_interleave(4, dim=0))
            conv.bias.zero_()
        self.net = nn.Sequential(conv, nn.SiLU(), nn.PixelShuffle(2))


def _single_class_id(class_label) -> int:
    """The un-tiled ``sample()`` loops condition every tile on ONE class (the reference passes a ``[1]`` label that
    broadcasts over the batch, model.py:694).  A ``[B]`` label with differing entries (legal for the reference's un-tiled
    ``sample``) is refused there rather than silently collapsed to its first element: un-tiled ``sample()`` is the
    remaining gap.  ``forward`` and the lock-step forms of ``tiled_sample`` take one label per image (``_image_class_ids``)."""
    if class_label is None:
        return -1
    flat = class_label.reshape(-1)
    if flat.numel() > 1 and not bool((flat == flat[0]).all()):
        raise NotImplementedError("per-image class labels: this engine conditions one run on one class "
                                  "(pass a [1] label, or equal labels)")
    return int(flat[0])


def _image_class_ids(class_label, n_images):
    """``class_label`` of a call on ``n_images`` images as one id per image: ``None`` stays ``None``, a ``[1]`` label
    broadcasts (the reference's form), a ``[n_images]`` label gives every image its own; any other count is a ``ValueError``."""
    if class_label is None:
        return None
    flat = [int(v) for v in torch.as_tensor(class_label).reshape(-1).tolist()]
    if len(flat) == 1:
        return flat * n_images
    if len(flat) != n_images:
        raise ValueError(f"class_label holds {len(flat)} labels for {n_images} images (pass one label, or one per image)")
    return flat


def _run_labels(ids):
    """(class_id for the begin entry, per-image ids or None) of a run: labels that differ are set after the begin
    (srgd_sampler_image_labels); equal ones run as the one-label run they are."""
    if ids is None:
        return -1, None
    return ids[0], (ids if len(set(ids)) > 1 else None)


def _noise_seeds(seeds, n_images):
    """``tiled_sample(seeds=...)``: a list of one non-negative int per image (ValueError otherwise)."""
    import operator
    if torch.is_tensor(seeds):
        seeds = seeds.tolist()
    try:
        seeds = list(seeds)
    except TypeError:
        raise ValueError("seeds must be a sequence of one non-negative int per image")
    if len(seeds) != n_images:
        raise ValueError(f"seeds: {len(seeds)} seeds for {n_images} images (one per image)")
    out = []
    for v in seeds:
        try:
            v = operator.index(v)
        except TypeError:
            raise ValueError(f"seeds: {v!r} is not an integer")
        if v < 0 or v >= 2 ** 64:
            raise ValueError(f"seeds: {v} is outside [0, 2**64) (a noise seed is a non-negative integer)")
        out.append(v)
    return out


def _packed_reference(reference, condition_x, crop_border, sampler):
    """``tiled_sample(reference=...)``: the ground truth of every image of ``condition_x`` (a ``[B,3,H,W]`` tensor or a list of
    ``[1,3,H_i,W_i]``) checked against the images' sizes before any sampling and packed into ``(flat uint8 device buffer, byte
    offsets)``.  ValueError: count, dtype or shape do not fit, or an image keeps fewer than 11 x 11 pixels inside the crop."""
    if sampler.canvas_group is not None:
        raise NotImplementedError("reference on a canvas sharded over ranks (canvas_group)")
    sizes = [(int(c.shape[-2]), int(c.shape[-1])) for c in condition_x]
    check_sizes(sizes, crop_border)
    return pack_references(reference, sizes, sampler.device)


def _back_project_steps(back_project, condition_x):
    """``tiled_sample(back_project=N)``: None for 0 / None (nothing is launched), else N with every image of ``condition_x`` (a
    ``[B,3,H,W]`` tensor or a list of ``[1,3,H_i,W_i]``) checked before any sampling.  ValueError: N outside 0 .. 64, a height or
    width that is no multiple of 4 or below 20, 3*H*W >= 2^31 - 256."""
    steps = check_iterations(back_project)
    if steps is not None:
        check_hr_sizes([(int(c.shape[-2]), int(c.shape[-1])) for c in condition_x])
    return steps


def _consistency_guidance(weight, start_steps, condition_x):
    """``tiled_sample(consistency_guidance=w, consistency_guidance_start_steps=s)``: None for a weight of 0 / None (nothing is
    allocated, nothing is launched), else ``(w, s)`` with every image of ``condition_x`` (a ``[B,3,H,W]`` tensor or a list of
    ``[1,3,H,W]`` tensors) checked: multiples of 4 and at least 20 on a side - ``ValueError`` before anything is sampled."""
    weight, start_steps = check_weight(weight), check_start_steps(start_steps)
    if weight is None:
        return None
    conds = condition_x if isinstance(condition_x, (list, tuple)) else [condition_x]
    check_guided_sizes([(int(c.shape[-2]), int(c.shape[-1])) for c in conds])
    return weight, start_steps


class _GuidedRun:
    """The LR-consistency guidance of one DDPM run (srgd_amd.guidance): the record array and the scratch are made once, ``step``
    is one batched call on the run's canvases after step i - x_start += w * g, img += w * fp32(alpha_next_i * c_i) * g inside every
    crop box (the posterior mean is linear in x_start: reference model.py:3164)."""

    def __init__(self, guidance, images, dev):
        self.weight, self.start = guidance
        self.recs, low = guidance_records(images)
        self.scratch = torch.empty(guidance_scratch_bytes(low), device=dev, dtype=torch.uint8)

    def step(self, i, scalars, img, x_start, cond01):
        if i < self.start:
            return
        mean_weight = float(torch.tensor(scalars[i].alpha_next, dtype=torch.float32) * torch.tensor(scalars[i].c, dtype=torch.float32))
        guide_step_flat(img.view(-1), x_start.view(-1), cond01.view(-1), self.recs, self.weight, self.weight * mean_weight,
                        self.scratch)


class _ThresholdRun:
    """The dynamic threshold of one DDPM run (srgd_amd.threshold): the record arrays of both step parities - the statistics box is
    the crop box, the update box what the step wrote: the whole canvas on even steps, the inner box on odd ones - the scratch and the
    [steps, images] array of s are made once; ``step`` is one batched call on the run's canvases after step i, before the guidance and
    the history calls: x_start = clip(x_start, -s, s) / s, img += fp32(alpha_next_i * c_i) * (the change) (the posterior mean is
    linear in x_start: reference model.py:3164)."""

    def __init__(self, q, images, max_steps, dev):
        """``images``: [(canvas_off, Hp, Wp, crop top, crop left, H, W, inner top, inner left, inner height, inner width)]."""
        self.q = q
        self.recs = (threshold_records([m[:7] + (0, 0, m[1], m[2]) for m in images]), threshold_records(images))
        self.scratch = torch.empty(threshold_scratch_bytes(len(images)), device=dev, dtype=torch.uint8)
        self.s = torch.empty(max(max_steps, 1), len(images), device=dev, dtype=torch.float32)
        self.calls = 0

    def step(self, i, scalars, img, x_start):
        mean_weight = float(torch.tensor(scalars[i].alpha_next, dtype=torch.float32) * torch.tensor(scalars[i].c, dtype=torch.float32))
        threshold_step_flat(img.view(-1), x_start.view(-1), self.recs[i % 2], self.q, mean_weight, self.s[self.calls], self.scratch)
        self.calls += 1

    def log(self):
        """[executed steps, images] fp32 on the CPU: every call's s."""
        return self.s[:self.calls].cpu()


def _schedule_of(num_sample_steps, solver, no_clamp=False):
    """The run's step table and log-SNR list: ``_schedule``'s, called as it always was.  ``no_clamp`` sets the field of that name on
    every step: the step kernel then leaves x0 unclamped, for the dynamic threshold's call that follows it."""
    scalars, log_snrs = _schedule(num_sample_steps) if solver is None else _schedule(num_sample_steps, *solver)
    if no_clamp:
        for s in scalars:
            s.no_clamp = 1.0
    return scalars, log_snrs


def _start_log_snr(generation_start_steps, num_sample_steps, step_spacing):
    """The log-SNR level a run that does not start from white noise is forward-diffused to (0-dim fp32): the reference's
    t0 = 1 - g / N under "time"; level g of the run's own list under "logsnr"."""
    if step_spacing != "time":
        return _log_snr_levels(num_sample_steps, step_spacing)[generation_start_steps]
    t0 = (1.0 - torch.tensor(generation_start_steps / num_sample_steps)) if generation_start_steps > 0 \
        else torch.tensor(1.0)
    return beta_linear_log_snr(t0)


class _SolverRun:
    """The history of one dpmpp2m run (srgd_amd.solver): ``x_prev`` - a clone of ``x_start``, so it is finite from the start - and
    the record array of the images' inner boxes are made once; ``step`` is one batched call on the run's canvases after step i (and
    after the step's guidance call, so that the history holds the corrected predictions): img += w_i (x_start - x_prev) inside
    every inner box, x_prev = x_start.  The ring outside the box is re-noised on every odd step: it has no history."""

    def __init__(self, num_sample_steps, step_spacing, first_step, images, x_start):
        self.weights = history_weights(_log_snr_levels(num_sample_steps, step_spacing), first_step)
        self.recs = solver_records(images)
        self.x_prev = x_start.clone()

    def step(self, i, img, x_start):
        history_step_flat(img.view(-1), x_start.view(-1), self.x_prev.view(-1), self.recs, self.weights[i])


def _as_tuple(v, n):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n


class ConditionalSRUnet(nn.Module):
    """Class-conditional SR U-Net (6-channel input: noisy | LR condition; 3-channel eps output)."""

    def __init__(self, dim, init_dim=None, out_dim=None, dim_mults=(1, 2, 4, 8), channels=3,
                 self_condition=True, resnet_block_groups=8, learned_variance=False,
                 learned_sinusoidal_cond=False, random_fourier_features=False, learned_sinusoidal_dim=16,
                 attn_dim_head=32, attn_heads=4, full_attn=(False, False, False, True), flash_attn=False,
                 pixel_shuffle_upsample=True, num_classes=None):
        super().__init__()
        unsupported = []
        if init_dim not in (None, dim): unsupported.append("init_dim != dim")
        if out_dim not in (None, channels): unsupported.append("out_dim != channels")
        if not self_condition: unsupported.append("self_condition=False")
        if learned_variance: unsupported.append("learned_variance=True")
        if not (learned_sinusoidal_cond or random_fourier_features): unsupported.append("fixed sinusoidal time embedding")
        if not pixel_shuffle_upsample: unsupported.append("pixel_shuffle_upsample=False")
        if unsupported:
            raise NotImplementedError("outside the shipped Real-SRGD configuration: " + ", ".join(unsupported))
        n = len(dim_mults)
        heads, dim_heads, full = _as_tuple(attn_heads, n), _as_tuple(attn_dim_head, n), _as_tuple(full_attn, n)
        assert len(full) == n
        if len(set(heads)) != 1 or len(set(dim_heads)) != 1:
            raise NotImplementedError("per-stage attn_heads / attn_dim_head")
        self.dim, self.dim_mults, self.channels = dim, tuple(dim_mults), channels
        self.self_condition = self_condition
        self.num_classes = num_classes
        self.groups, self.heads, self.dim_head = resnet_block_groups, heads[0], dim_heads[0]
        self.full_attn = tuple(bool(f) for f in full)
        self.sinus_dim = learned_sinusoidal_dim
        self.random_or_learned_sinusoidal_cond = True
        self.out_dim = channels
        self.flash_attn = flash_attn          # accepted; attention is a HIP kernel either way
        self.precision = "fp32"               # precision of forward(); the sampler picks its own

        time_dim = dim * 4
        dims = [dim] + [dim * m for m in dim_mults]
        self.init_conv = nn.Conv2d(channels * 2, dim, 7, padding=3)
        self.time_mlp = nn.Sequential(_FourierFreqs(learned_sinusoidal_dim, random_fourier_features),
                                      nn.Linear(learned_sinusoidal_dim + 1, time_dim), nn.GELU(),
                                      nn.Linear(time_dim, time_dim))
        if num_classes is not None:
            self.class_mlp = nn.Sequential(nn.Embedding(num_classes, dim), nn.Linear(dim, time_dim), nn.GELU(),
                                           nn.Linear(time_dim, time_dim))
        mk_res = lambda i, o: _Residual(i, o, time_dim, resnet_block_groups)
        mk_attn = lambda c, f: (_SoftmaxAttn if f else _LinearAttn)(c, self.heads, self.dim_head)
        self.downs, self.ups = nn.ModuleList(), nn.ModuleList()
        for s in range(n):
            cin, cout = dims[s], dims[s + 1]
            down = (nn.Sequential(nn.Identity(), nn.Conv2d(cin * 4, cout, 1)) if s < n - 1     # space-to-depth + 1x1
                    else nn.Conv2d(cin, cout, 3, padding=1))
            self.downs.append(nn.ModuleList([mk_res(cin, cin), mk_res(cin, cin), mk_attn(cin, self.full_attn[s]), down]))
        self.mid_block1 = mk_res(dims[-1], dims[-1])
        self.mid_attn = _SoftmaxAttn(dims[-1], self.heads, self.dim_head)
        self.mid_block2 = mk_res(dims[-1], dims[-1])
        for u in range(n):
            s = n - 1 - u
            cin, cout = dims[s], dims[s + 1]
            up = _ShuffleUp(cout, cin) if u < n - 1 else nn.Conv2d(cout, cin, 3, padding=1)
            self.ups.append(nn.ModuleList([mk_res(cout + cin, cout), mk_res(cout + cin, cout),
                                           mk_attn(cout, self.full_attn[s]), up]))
        self.final_res_block = mk_res(dim * 2, dim)
        self.final_conv = nn.Conv2d(dim, channels, 1)

        self._engines = {}
        self._weights_version = 0
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._invalidate_engines())

    # ---- engine plumbing ---------------------------------------------------------------------
    @property
    def downsample_factor(self) -> int:
        return 2 ** (len(self.dim_mults) - 1)

    def _invalidate_engines(self):
        for eng in self._engines.values():
            eng.close()
        self._engines = {}
        self._weights_version += 1

    def _apply(self, fn, *a, **k):                  # .to()/.cuda()/.float() may move or change the parameters
        out = super()._apply(fn, *a, **k)
        self._invalidate_engines()
        return out

    def __deepcopy__(self, memo):
        engines, self._engines = self._engines, {}
        try:
            cls = self.__class__
            new = cls.__new__(cls)
            memo[id(self)] = new
            for k, v in self.__dict__.items():
                new.__dict__[k] = copy.deepcopy(v, memo)
        finally:
            self._engines = engines
        new._engines = {}
        return new

    def engine(self, precision: str = "fp32", lane: int = 0) -> HipEngine:
        """The C-ABI engine of this U-Net for one precision; ``lane`` > 0: a further instance (srgd_amd.lanes)."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.SrgdHipError("ConditionalSRUnet runs on MI355X only: move the model to the GPU "
                                    "(the CPU restatement under oracle/ is test infrastructure, not a fallback)")
        key = (dev.index if dev.index is not None else torch.cuda.current_device(), precision) + ((lane,) if lane else ())
        if key not in self._engines:
            eng = HipEngine(dim=self.dim, dim_mults=self.dim_mults, full_attn=self.full_attn, channels=self.channels,
                            groups=self.groups, heads=self.heads, dim_head=self.dim_head, sinus_dim=self.sinus_dim,
                            num_classes=self.num_classes, precision=precision, device=torch.device("cuda", key[0]))
            eng.load_state_dict({k: v for k, v in self.state_dict().items()}, strict=True)
            self._engines[key] = eng
        return self._engines[key]

    # ---- reference forward signature (model.py:678) ---------------------------------------------
    def forward(self, x, time, class_label=None, x_self_cond=None):
        f = self.downsample_factor
        assert all(d % f == 0 for d in x.shape[-2:]), \
            f"your input dimensions {x.shape[-2:]} need to be divisible by {f}, given the unet"
        class_id, per_sample = -1, None
        if class_label is not None:
            if class_label.numel() == 1:
                class_id = int(class_label.reshape(-1)[0])
            else:                                   # one label per sample (model.py:692-694 embeds a [B] label row by row)
                per_sample = _image_class_ids(class_label, x.shape[0])
        time = time.reshape(-1)
        if time.numel() == 1 and x.shape[0] > 1:
            time = time.expand(x.shape[0])
        if per_sample is not None:
            return self.engine(self.precision).unet_forward_labels(x, time, per_sample, x_self_cond)
        return self.engine(self.precision).unet_forward(x, time, class_id, x_self_cond)


# ---------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------
_BOTH_SCALES = "Currently, you cannot specify both cond_scale and class_cond_scale at the same time."
_SCHEDULE_SHARDED = "precision_schedule on a canvas sharded over ranks (canvas_group)"


def _step_guidance(i, cond_scale, guidance_start_steps, class_cond_scale, class_guidance_start_steps, joint=False):
    """(passes, guidance_kind, scale) of DDPM step i (model.py:3147-3156).  ``joint``: a step on which both current scales differ
    from 1 is the three-pass joint step, (3, 3, (cond scale, class scale)); every other step is what it is without it."""
    cur_cond_scale = 1.0 if i < guidance_start_steps else cond_scale
    cur_class_scale = 1.0 if i < class_guidance_start_steps else class_cond_scale
    if joint and cur_cond_scale != 1.0 and cur_class_scale != 1.0:
        return 3, 3, (cur_cond_scale, cur_class_scale)
    if cur_cond_scale != 1.0:
        return 2, 2, cur_cond_scale
    if cur_class_scale != 1.0:
        return 2, 1, cur_class_scale
    return 1, 0, 1.0

def _launch_tiles(passes, sub_batch):
    """Tiles per U-Net launch of a step.  A joint step (three passes) is capped at two thirds of the limit: its launches then hold
    at most the 2 x sub_batch entries of a two-pass step, so the memory high-water mark is that of a two-pass run of the same
    command line (results do not depend on the grouping)."""
    return max(1, 2 * sub_batch // 3) if passes == 3 else sub_batch


def _ddpm_step(e_, i, part, img, cond_canvas, x_start, noise_tiles, noise_canvas, passes, kind, scale, sub_batch, seed):
    """One DDPM step on engine ``e_``: the whole grid (``part`` None) or a lane's ``(first, count, ring)``; ``passes`` 3 is the
    joint step with ``scale = (cond scale, class scale)``, everything else today's entries."""
    if passes == 3:
        if part is None:
            e_.sampler_step_joint(i, img, cond_canvas, x_start, noise_tiles, noise_canvas, scale[0], scale[1], sub_batch, seed=seed)
        else:
            e_.sampler_step_joint_tiles(i, part[0], part[1], part[2], img, cond_canvas, x_start, noise_tiles, noise_canvas, scale[0],
                                        scale[1], sub_batch, seed=seed)
    elif part is None:
        e_.sampler_step(i, img, cond_canvas, x_start, noise_tiles, noise_canvas, passes, kind, scale, sub_batch, seed=seed)
    else:
        e_.sampler_step_tiles(i, part[0], part[1], part[2], img, cond_canvas, x_start, noise_tiles, noise_canvas, passes, kind, scale,
                              sub_batch, seed=seed)


def _check_joint(joint_guidance, cond_scale, class_cond_scale, class_label, canvas_group):
    """Both scales at once: refused as upstream does unless ``joint_guidance``; then the refusals of the joint step itself."""
    if cond_scale == 1.0 or class_cond_scale == 1.0:
        return False
    if not joint_guidance:
        raise NotImplementedError(_BOTH_SCALES)
    if class_label is None:
        raise ValueError("joint_guidance needs a class_label (the label-dropped pass would repeat the full one)")
    if canvas_group is not None:
        raise NotImplementedError("joint_guidance on a canvas sharded over ranks (canvas_group)")
    if not (math.isfinite(cond_scale) and math.isfinite(class_cond_scale)):
        raise ValueError("joint_guidance: the scales must be finite")
    return True


class ConditionalContinuousTimeGaussianDiffusionSR(nn.Module):
    def __init__(self, model, *, image_size, channels=3, noise_schedule="linear", num_sample_steps=500,
                 clip_sample_denoised=True, learned_schedule_net_hidden_dim=1024,
                 learned_noise_schedule_frac_gradient=1.0, min_snr_loss_weight=False, min_snr_gamma=5,
                 cond_drop_prob=0.0, class_cond_drop_prob=0.0, loss_type="l2"):
        super().__init__()
        assert model.random_or_learned_sinusoidal_cond
        if noise_schedule != "linear":
            raise NotImplementedError(f"noise_schedule={noise_schedule!r}: only the shipped 'linear' log-SNR schedule is built")
        if not clip_sample_denoised:
            raise NotImplementedError("clip_sample_denoised=False")
        self.model = model
        self.channels, self.image_size = channels, image_size
        self.log_snr = beta_linear_log_snr
        self.num_sample_steps = num_sample_steps
        self.clip_sample_denoised = clip_sample_denoised
        self.min_snr_loss_weight, self.min_snr_gamma = min_snr_loss_weight, min_snr_gamma
        self.cond_drop_prob, self.class_cond_drop_prob = cond_drop_prob, class_cond_drop_prob
        self.loss_type = loss_type
        # engine knobs (not part of the reference surface)
        self.noise_source = "host"     # "host": torch CPU generator in the reference's draw order; "device": Philox
        self.host_generator = None     # host-noise draws: None = torch's global CPU generator (what seed_everything seeds, as the
                                       # reference); a torch.Generator makes a run independent of other threads' draws
        self.device_noise_seed = 0
        self.max_tiles_per_launch = None   # None: use the caller's batch_size as the reference does
        self.step_lanes = lanes_setting_from_env()   # None: automatic - small steps run as two concurrent halves (srgd_amd.lanes)
        # engine precision: "fp32" (default: the reference's numerics - upstream ignores ``amp`` and always computes fp32,
        # SURVEY App. E), "bf16" (throughput mode), "bf16_w8" (bf16 kernels, fp8-e4m3-rounded conv weights),
        # "fp8" (MX-fp8 3x3 convolutions, BASELINE configs[4]), "fp8_mixed" (fp8 below the top resolution only: 53 dB vs
        # bf16 instead of 34 dB).  tiled_sample(precision=...) overrides it per call.
        self.precision = "fp32"
        # None, or a precision schedule (srgd_amd.precision_schedule, e.g. "bf16:40,f16x3"): tiled_sample then takes every step
        # in the precision the schedule plans for it; tiled_sample(precision_schedule=...) or (precision=...) overrides it per call
        self.precision_schedule = None
        # set by srgd_amd.parallel.shard_canvas: a torch.distributed group whose ranks share ONE canvas - each rank
        # runs a contiguous slice of every step's tiles and the updated tiles are all-gathered
        self.canvas_group = None

    def set_seed(self, seed):
        torch.cuda.manual_seed(seed)
        self.device_noise_seed = int(seed)

    @property
    def device(self):
        return next(self.model.parameters()).device

    def _precision_plan(self, precision, schedule, num_sample_steps, generation_start_steps):
        """``(plan, names)`` of a tiled run: the precision of every loop index and the distinct precisions of the executed steps
        in order of first use.  ``schedule``: the call's parsed ``precision_schedule`` or None; without it and without
        ``precision`` the wrapper's ``precision_schedule`` attribute holds, and without any schedule every step has the run's one
        precision."""
        if schedule is None and precision is None and self.precision_schedule is not None:
            schedule = parse_schedule(self.precision_schedule)
        if schedule is None:
            return [precision or self.precision] * num_sample_steps, [precision or self.precision]
        if self.canvas_group is not None:
            raise NotImplementedError(_SCHEDULE_SHARDED)
        plan = plan_steps(schedule, num_sample_steps)
        return plan, executed_names(plan, generation_start_steps)

    @torch.inference_mode()
    def tiled_sample(self, batch_size=4, tile_size=256, tile_stride=256, condition_x=None, class_label=None,
                     cond_scale=1.0, guidance_start_steps=0, class_cond_scale=1.0, class_guidance_start_steps=0,
                     generation_start_steps=0, num_sample_steps=None, with_images=False, with_x0_images=False,
                     start_white_noise=True, amp=False, precision=None, seeds=None, color_fix=None, reference=None,
                     crop_border=4, back_project=0, consistency_guidance=0.0, consistency_guidance_start_steps=0,
                     sampler="ddpm", eta=None, step_spacing="time", dynamic_threshold=None, threshold_log=None,
                     joint_guidance=False, region_known=None, regions=None, region_skip_tiles=True, region_log=None,
                     precision_schedule=None, precision_log=None):
        """Tiled CFG-DDPM sampling (reference model.py:3288-3413).

        ``amp`` is accepted and ignored exactly as in the reference (which always computes fp32); the engine
        precision is ``precision`` (engine-only keyword) or, if None, ``self.precision`` - "fp32" by default, i.e.
        the reference's numerics.  ``condition_x`` is ``[1,3,H,W]`` as in the reference, or
        ``[B,3,H,W]``: B same-sized images sampled in lock-step, each exactly as the reference would
        sample it on its own after ``seed_everything(seed)`` (inference.py:73) - i.e. all B see the
        same noise stream - with every U-Net launch spanning tiles of all images (fills the GPU
        better than 25/16 tiles of one image do).  ``batch_size`` counts tiles across all images.

        ``condition_x`` may also be a list or tuple of ``[1,3,H_i,W_i]`` tensors of different sizes: they are sampled in
        lock-step the same way (mixed-size lock-step, ``_tiled_sample_images``) and a list of ``[1,3,H_i,W_i]`` outputs is
        returned, each bit-identical to a call with that image alone.

        ``seeds`` (engine-only keyword, absent upstream): a sequence of non-negative ints, one noise seed per image of either
        group form.  Image i then comes out bit-identical to a call on that image alone after ``torch.manual_seed(seeds[i])``
        (host noise) or with ``device_noise_seed = seeds[i]`` (device noise), every other argument the same - K copies of one
        image with K seeds are K different samples in one run.  Images that agree in canvas size and seed share one noise
        stream.  In host-noise mode each stream draws from a private ``torch.Generator().manual_seed(seed)`` in the reference's
        draw order, and the caller's generator (``host_generator`` or torch's global one) is neither read nor advanced.  A
        seeded run takes the mixed-size path for both condition forms; ``seeds=None`` is the unseeded call unchanged.  Not
        available together with ``with_images`` / ``with_x0_images`` or a canvas sharded over ranks.

        ``color_fix`` (engine-only keyword, absent upstream): ``None`` / ``"none"`` (default: nothing is launched), ``"wavelet"`` or
        ``"adain"`` - the final [0,1] image of every image of the run is colour-corrected against its own ``condition_x`` on the
        GPU (srgd_amd.colorfix, one batched call per run) and equals ``color_fix_on_device(uncorrected result, condition_x, mode)``
        bit for bit.  Trajectories (``with_images`` / ``with_x0_images``) stay raw; on a canvas sharded over ranks every rank
        corrects its own copy of the whole output.

        ``reference`` (engine-only keyword, absent upstream): ``None`` (default: nothing is launched, the return value is what it
        always was) or the ground truth of the run - a uint8 ``[H,W,3]`` tensor, or a list of them, one per image.  The return
        value then gains a trailing list of ``{"psnr_y", "psnr_rgb", "ssim_y"}`` dicts, one per image: Y-channel PSNR, RGB PSNR and
        Y-channel SSIM of the final image as it would be saved (after the colour fix) with ``crop_border`` pixels cut from every
        side, computed on the GPU (srgd_amd.metrics, one batched call and one copy of 4 doubles per image).  Not available on a
        canvas sharded over ranks.

        ``back_project`` (engine-only keyword, absent upstream): 0 (default: nothing is launched) or the number N <= 64 of
        back-projection steps - after the colour fix and before the metrics, the final image of every image of the run is pulled
        back onto its own ``condition_x`` on the GPU (srgd_amd.backproject, one batched call per run) and equals
        ``back_project_on_device(result without the keyword, condition_x, N)`` bit for bit.  Trajectories stay raw.  The
        condition's height and width must be multiples of 4 and at least 20: ``ValueError`` before anything is sampled.

        ``consistency_guidance`` (engine-only keyword, absent upstream): a weight w in [0, 1]; 0 (default): nothing is allocated,
        nothing is launched, the run is byte for byte what it is without the keyword.  With w > 0, after every step
        i >= max(``consistency_guidance_start_steps``, ``generation_start_steps``) - the last one included - the step's prediction
        of the clean image is pulled towards the input inside every image's crop box, on the GPU in one batched call per step
        (srgd_amd.guidance, include/srgd_guidance.h): g = (2 condition_x - 1) - enlarge(reduce(x_start)), x_start += w g,
        img += w alpha_next_i c_i g - the DDPM posterior mean is linear in x_start, so this is the step taken with the corrected
        prediction (DDNM / ILVR), and the later steps harmonise the correction.  ``with_x0_images`` shows the corrected
        predictions.  Every image of a group is bit-identical to its solo guided run.  The condition's height and width must be
        multiples of 4 and at least 20: ``ValueError`` before anything is sampled.  Not available on a canvas sharded over ranks.

        ``sampler``, ``eta``, ``step_spacing`` (engine-only keywords, absent upstream): the defaults "ddpm", None, "time" are the
        run byte for byte as it is without them.  ``sampler="ddim"`` with ``eta`` in [0, 1] (default 0) is the DDIM family's step
        A x_t + B x0 + S z as a step table (srgd_amd.solver.step_coefficients; eta = 1 is the ancestral step up to rounding);
        ``sampler="dpmpp2m"`` (``eta`` None or 0) is the second-order multistep DPM-Solver++ 2M: the eta = 0 table and, after every
        step but the first executed and the last, img += w_i (x_start_i - x_start_{i-1}) inside every image's inner box on the GPU,
        one batched call per step after the guidance call if there is one (srgd_amd.solver, include/srgd_solver.h).  The noise
        draws of every sampler are those of a ddpm run of the same length (with S = 0 the tile noise is multiplied by zero).
        ``step_spacing="logsnr"`` places the N + 1 step ends uniformly in the log-SNR instead of in t, which is what makes few
        steps worth taking; ``generation_start_steps = g`` then starts from level g of that list.  Bad values: ``ValueError``
        before anything is sampled.  dpmpp2m is not available on a canvas sharded over ranks (its history would have to travel
        with the tile exchange); ddim and ``step_spacing`` only change tables and are.

        ``dynamic_threshold`` (engine-only keyword, absent upstream): a percentile P; None / 0 (default): nothing is loaded,
        allocated or launched, the run is byte for byte what it is without the keyword.  Otherwise P is rounded to fp32 and must lie
        in (0, 1]: the steps are taken without the static clamp of the predicted clean image to [-1, 1], and after every executed step
        - before the guidance and the history calls, whose corrections it completes - one batched call on the GPU (srgd_amd.threshold,
        include/srgd_threshold.h) takes per image s = max(1, the P-quantile of |x_start| inside the crop box), an exact order statistic,
        clips x_start to [-s, s] and divides it by s inside what the step wrote, and adds alpha_next_i c_i times the change to img
        (Imagen's dynamic thresholding: guidance scales above 1 overshoot, and the static clamp saturates whole regions).
        ``with_x0_images`` shows the thresholded predictions.  ``threshold_log``: a list that receives one CPU tensor
        [executed steps, images] of s.  Every image of a group is bit-identical to its solo run.  Combines with every sampler, step
        spacing, ``consistency_guidance``, ``generation_start_steps``, seeds and labels.  Not available on a canvas sharded over
        ranks.  Picture quality on trained weights is not measured.

        ``joint_guidance`` (engine-only keyword, absent upstream): False (default): ``cond_scale`` and ``class_cond_scale`` both
        different from 1 raise ``NotImplementedError`` as upstream does.  True: every step on which both current scales differ from 1
        (after ``guidance_start_steps`` and ``class_guidance_start_steps``) is one three-pass step, eps = e + (s_c - 1)(e - n_c) +
        (s_l - 1)(e - n_l) with n_c the prediction without the condition and n_l the one without the label (include/srgd_hip.h,
        srgd_sampler_step with passes = 3); steps with one active scale are today's two-pass steps byte for byte, steps with none the one-pass
        step.  A joint step launches at most ``max(1, 2 * batch_size // 3)`` tiles at once, so the run needs no more memory than a
        two-pass run of the same arguments.  Works in all three drivers and with every other keyword, which act on the canvases
        after the step.  ``class_label=None``: ``ValueError`` before anything is sampled; not available on a canvas sharded over
        ranks.  Picture quality on trained weights is not measured.

        ``region_known``, ``regions`` (engine-only keywords, absent upstream; srgd_amd.region): without them nothing is allocated or
        launched and the run is byte for byte what it is today.  ``region_known`` is a finished output of this image - fp32
        ``[1,3,H,W]`` in [0, 1], the size of ``condition_x`` - and ``regions`` a list of 1 .. 16 ``(top, left, height, width)`` boxes
        in output pixels, each inside the image; R is their union.  In a lock-step call ``region_known`` is a list with one entry per
        image (``None``: that image is sampled whole, as today) and ``regions`` one box list for all of them or one per image.  With
        k = 2 known - 1 and K(a, s) = ``srgd_sampler_q_start(known, z, a, s)`` on the image's canvas, the *replacement step* at (a, s)
        sets ``img`` outside R to K(a, s) - R of ``img`` is copied into K, K over ``img`` - and, where the run keeps an ``x_start``
        canvas, ``x_start`` outside R to K(1, 0), the padded known image.  It is applied to the start canvas at the start level, and
        after the threshold, guidance and history calls of every step i at (alpha_next_i, sigma_next_i) - the last step at (1, 0)
        without a draw.  z comes from ``srgd_randn`` with the image's noise seed (``seeds[i]``, else ``device_noise_seed``) and
        stream ``(3 << 32) | i``; the start canvas takes index ``num_sample_steps``.  With ``region_skip_tiles`` (default True) step
        i evaluates only the tiles of grid i % 2 that intersect R - each maximal run of consecutive tile indices is one
        ``srgd_sampler_step_tiles`` call without the ring re-noise, which lies outside R and is overwritten - and the result is bit for
        bit that of ``region_skip_tiles=False``, which evaluates all tiles (``dynamic_threshold`` and ``consistency_guidance`` read
        ``x_start`` beyond R: with them the two differ, the skipped tiles showing the known image).  After ``color_fix`` and
        ``back_project`` and before the ``reference`` metrics the output outside R is set to ``region_known`` by copy.
        ``region_log``: a list that receives one row ``[tiles evaluated per image]`` per executed step.  Step lanes are off in a
        region run.  ``ValueError`` before anything is sampled: a box outside the image, no box or more than 16, a ``region_known``
        of another shape or dtype, one keyword without the other; not available on a canvas sharded over ranks or in the EDM
        wrapper (``NotImplementedError``).  Picture quality on trained weights is not measured.

        ``precision_schedule`` (engine-only keyword, absent upstream; srgd_amd.precision_schedule): None (default) is the wrapper's
        ``precision_schedule`` attribute, and with that None too the run is byte for byte what it is today.  Otherwise a schedule
        ``NAME[:COUNT](,NAME[:COUNT])*`` or a sequence of ``(name, count or None)`` pairs - ``"bf16:40,f16x3"``: loop indices 0 .. 39 in
        bf16, the rest in f16x3; ``"bf16,f16x3:10"``: the last 10 in f16x3 - planned over the absolute loop indices of
        ``num_sample_steps``.  Step i runs on the engine of its precision; the canvases are fp32 in every precision and the noise
        draws do not depend on the engine, so nothing is converted at a switch and a step is bit for bit the step a run of that one
        precision takes from the same canvas.  Every precision with an executed step gets its engine begun once before the loop with
        the run's geometry, scalars, labels and seeds and its own condition canvas; the start canvas comes from the engine of the first
        executed step and the final image from that of the last (entries that do not depend on the precision).  A schedule whose
        executed steps share one name is ``precision=NAME``, call for call.  Step lanes are decided per step with the step's
        precision.  Works in all three drivers and with every other keyword, which act on the fp32 canvases.  ``precision_log``: a
        list that receives the precision of every executed step.  ``ValueError`` before anything is sampled: a malformed schedule,
        counts that do not fit ``num_sample_steps``, ``precision`` and ``precision_schedule`` in one call; not available on a canvas
        sharded over ranks or in the EDM wrapper (``NotImplementedError``).  Picture quality on trained weights is not measured."""
        if precision_schedule is not None:
            if precision is not None:
                raise ValueError("precision and precision_schedule in one call: a run has one precision or one schedule")
            precision_schedule = parse_schedule(precision_schedule)
            if self.canvas_group is not None:
                raise NotImplementedError(_SCHEDULE_SHARDED)
        if precision_log is not None and not isinstance(precision_log, list):
            raise ValueError("precision_log: None or a list")
        schedule_kw = dict(precision_schedule=precision_schedule, precision_log=precision_log)
        region = None
        if region_known is not None or regions is not None:
            if self.canvas_group is not None:
                raise NotImplementedError("region_known / regions on a canvas sharded over ranks (canvas_group)")
            if not isinstance(condition_x, (list, tuple)) and (not torch.is_tensor(condition_x) or condition_x.dim() != 4):
                raise ValueError("condition_x must be [B,3,H,W] (B=1 in the reference, whose tile gather assumes batch 1)")
            region = check_region_args(region_known, regions, [(int(c.shape[-2]), int(c.shape[-1])) for c in condition_x])
        if region_log is not None and not isinstance(region_log, list):
            raise ValueError("region_log: None or a list")
        region_kw = {} if region is None else dict(region=region, region_skip_tiles=bool(region_skip_tiles), region_log=region_log)
        sampler, eta, step_spacing = check_sampler(sampler, eta, step_spacing)
        threshold = check_percentile(dynamic_threshold)
        if threshold is not None and self.canvas_group is not None:
            raise NotImplementedError("dynamic_threshold on a canvas sharded over ranks (canvas_group)")
        if threshold_log is not None and not isinstance(threshold_log, list):
            raise ValueError("threshold_log: None or a list")
        solver = None if is_default(sampler, eta, step_spacing) else (sampler, eta, step_spacing)
        color_fix = check_mode(color_fix)
        back_project = _back_project_steps(back_project, condition_x)
        guidance = _consistency_guidance(consistency_guidance, consistency_guidance_start_steps, condition_x)
        if guidance is not None and self.canvas_group is not None:
            raise NotImplementedError("consistency_guidance on a canvas sharded over ranks (canvas_group)")
        if sampler == "dpmpp2m" and self.canvas_group is not None:
            raise NotImplementedError("sampler='dpmpp2m' on a canvas sharded over ranks (canvas_group)")
        if reference is not None:
            reference = _packed_reference(reference, condition_x, crop_border, self)
        num_sample_steps = self.num_sample_steps if num_sample_steps is None else num_sample_steps
        if precision_schedule is not None:  # the counts against the run's length, before anything is sampled
            plan_steps(precision_schedule, num_sample_steps)
        if seeds is not None:
            as_list = isinstance(condition_x, (list, tuple))
            seeds = _noise_seeds(seeds, len(condition_x) if as_list else int(condition_x.shape[0]))
            if with_images or with_x0_images:
                raise NotImplementedError("seeds together with with_images / with_x0_images (trajectories of a seeded group)")
            if self.canvas_group is not None:
                raise NotImplementedError("seeds on a canvas sharded over ranks (canvas_group)")
            if not as_list:
                if condition_x.dim() != 4 or condition_x.shape[1] != 3:
                    raise ValueError("condition_x must be [B,3,H,W] (B=1 in the reference, whose tile gather assumes batch 1)")
                condition_x = [condition_x[i:i + 1] for i in range(condition_x.shape[0])]
            joint = _check_joint(joint_guidance, cond_scale, class_cond_scale, class_label, self.canvas_group)
            if tile_size != 256 or tile_stride != 256:
                raise NotImplementedError("tile_size/tile_stride other than 256 are unusable in the reference too "
                                          "(get_coord_and_pad is called without them, model.py:3301)")
            outs = self._tiled_sample_images(batch_size, tile_size, list(condition_x), class_label, cond_scale,
                                             guidance_start_steps, class_cond_scale, class_guidance_start_steps,
                                             generation_start_steps, num_sample_steps, start_white_noise, precision, seeds=seeds,
                                             color_fix=color_fix, reference=reference, crop_border=crop_border, back_project=back_project,
                                             guidance=guidance, solver=solver, threshold=threshold, threshold_log=threshold_log,
                                             joint=joint, **region_kw, **schedule_kw)
            if reference is not None:
                return (outs[0] if as_list else torch.cat(outs[0], 0)), outs[1]
            return outs if as_list else torch.cat(outs, 0)
        if isinstance(condition_x, (list, tuple)):
            if with_images or with_x0_images:
                raise NotImplementedError("with_images / with_x0_images of a mixed-size group (trajectories of different shapes)")
            if self.canvas_group is not None:
                raise NotImplementedError("mixed-size lock-step on a canvas sharded over ranks (canvas_group)")
            joint = _check_joint(joint_guidance, cond_scale, class_cond_scale, class_label, self.canvas_group)
            if tile_size != 256 or tile_stride != 256:
                raise NotImplementedError("tile_size/tile_stride other than 256 are unusable in the reference too "
                                          "(get_coord_and_pad is called without them, model.py:3301)")
            return self._tiled_sample_images(batch_size, tile_size, list(condition_x), class_label, cond_scale,
                                             guidance_start_steps, class_cond_scale, class_guidance_start_steps,
                                             generation_start_steps, num_sample_steps, start_white_noise, precision,
                                             color_fix=color_fix, reference=reference, crop_border=crop_border, back_project=back_project,
                                             guidance=guidance, solver=solver, threshold=threshold, threshold_log=threshold_log,
                                             joint=joint, **region_kw, **schedule_kw)
        joint = _check_joint(joint_guidance, cond_scale, class_cond_scale, class_label, self.canvas_group)
        if tile_size != 256 or tile_stride != 256:
            raise NotImplementedError("tile_size/tile_stride other than 256 are unusable in the reference too "
                                      "(get_coord_and_pad is called without them, model.py:3301)")
        dev = self.device
        if dev.type != "cuda":
            raise _lib.SrgdHipError("tiled_sample runs on MI355X only (no CPU fallback)")
        batch, c, h, w = condition_x.shape
        if batch < 1 or c != 3:
            raise ValueError("condition_x must be [B,3,H,W] (B=1 in the reference, whose tile gather assumes batch 1)")
        f = self.model.downsample_factor
        assert tile_size % f == 0, f"your input dimensions need to be divisible by {f}, given the unet"
        class_id, image_ids = _run_labels(_image_class_ids(class_label, batch))
        if image_ids is not None and self.canvas_group is not None:
            raise NotImplementedError("per-image class labels on a canvas sharded over ranks (canvas_group)")
        plan, names = self._precision_plan(precision, precision_schedule, num_sample_steps, generation_start_steps)
        engines = {name: self.model.engine(name) for name in names}
        eng = engines[names[0]]             # of the first executed step: the start canvas and the region run's draws

        (left, top, right, bottom), pad = get_coord_and_pad(h, w)
        hp, wp = h + pad[2] + pad[3], w + pad[0] + pad[1]
        if max(pad[0], pad[1]) >= w or max(pad[2], pad[3]) >= h:
            raise RuntimeError("Padding size should be less than the corresponding input dimension "
                               f"(reflect pad {pad} of a {h}x{w} image)")
        coords0 = get_coords(hp, wp, tile_size, tile_size, diff=0)
        if hp <= tile_size and wp <= tile_size:
            coords1 = get_coords(hp, wp, tile_size, tile_stride, diff=0)
        else:
            coords1 = get_coords(hp - tile_size, wp - tile_size, tile_size, tile_stride, diff=tile_size // 2)
        (sl, st_, sr, sb), _ = get_area(coords1, hp, wp)
        geo = SamplerGeometry(H=h, W=w, Hp=hp, Wp=wp, left=left, top=top, inner_l=sl, inner_t=st_, inner_r=sr,
                              inner_b=sb, tile=tile_size, n_even=len(coords0), n_odd=len(coords1), n_images=batch)
        scalars, log_snrs = _schedule_of(num_sample_steps, solver, no_clamp=threshold is not None)

        cond01 = condition_x.to(dev, torch.float32).contiguous()
        cond_canvas = torch.empty(batch, 3, hp, wp, device=dev, dtype=torch.float32)

        def begin(e_, canvas):
            e_.sampler_begin(geo, cond01, canvas, [(a, c_) for (a, _, c_, _) in coords0],
                             [(a, c_) for (a, _, c_, _) in coords1], scalars, log_snrs, class_id)
            if image_ids is not None:
                e_.sampler_image_labels(image_ids)
        # every precision of the plan: its engine begun with the same run and its own copy of the condition canvas
        canvases = {name: cond_canvas if name == names[0] else torch.empty_like(cond_canvas) for name in names}
        for name in names:
            begin(engines[name], canvases[name])

        host_noise = self.noise_source == "host"
        if generation_start_steps > 0 or not start_white_noise:
            # start from the forward-diffused condition (model.py:3305-3308 / :3312-3315); same single draw
            ls0 = _start_log_snr(generation_start_steps, num_sample_steps, step_spacing)
            img = torch.empty(batch, 3, hp, wp, device=dev)
            eng.sampler_q_start(cond01, _host_randn(self.host_generator, 1, 3, hp, wp).to(dev) if host_noise else None,
                                float(ls0.sigmoid().sqrt()), float((-ls0).sigmoid().sqrt()), img, self.device_noise_seed)
        elif host_noise:
            img = _host_randn(self.host_generator, 1, 3, hp, wp).to(dev).repeat(batch, 1, 1, 1)   # reference draw #1 (model.py:3311)
        else:
            img = eng.randn_(torch.empty(1, 3, hp, wp, device=dev), self.device_noise_seed, 0).repeat(batch, 1, 1, 1)
        regional = None
        if region is not None:              # the start canvas outside R: the known image at the start level
            regional = _RegionRun(eng, [RegionImage(b * 3 * hp * wp, b * 3 * h * w, hp, wp, top, left, h, w, coords0, coords1, 0,
                                                    None if region[b] is None else region[b][1]) for b in range(batch)],
                                  [None if r is None else r[0] for r in region], [(hp, wp)], [self.device_noise_seed],
                                  num_sample_steps, region_skip_tiles, dev, batch * 3 * hp * wp, batch * 3 * h * w)
            ls0 = _start_log_snr(generation_start_steps, num_sample_steps, step_spacing)
            regional.replace(num_sample_steps, float(ls0.sigmoid().sqrt()), float((-ls0).sigmoid().sqrt()), img)
        x_start = img.clone() if with_x0_images or guidance is not None or sampler == "dpmpp2m" or threshold is not None else None
        image_list = [img[:, :, top:bottom, left:right].clone().cpu()] if with_images else None
        x0_image_list = [img[:, :, top:bottom, left:right].clone().cpu()] if with_x0_images else None
        thresholded = None
        if threshold is not None:
            thresholded = _ThresholdRun(threshold, [(b * 3 * hp * wp, hp, wp, top, left, h, w, st_, sl, sb - st_, sr - sl)
                                                    for b in range(batch)], num_sample_steps - generation_start_steps, dev)
        guided = None
        if guidance is not None:            # x_start is laid out like img: final_step_kernel addresses both alike
            guided = _GuidedRun(guidance, [(b * 3 * hp * wp, b * 3 * h * w, hp, wp, top, left, h, w) for b in range(batch)], dev)
        history = None
        if sampler == "dpmpp2m":            # the inner box of the odd grid: what is never re-noised
            history = _SolverRun(num_sample_steps, step_spacing, generation_start_steps,
                                 [(b * 3 * hp * wp, hp, wp, st_, sl, sb - st_, sr - sl) for b in range(batch)], x_start)

        sub_batch = self.max_tiles_per_launch or batch_size
        grids = (coords0, coords1)
        lanes_of = {}                       # one StepLanes per precision, built on first need
        eng_i = eng
        for i in range(num_sample_steps):
            if i < generation_start_steps:
                continue
            prec_i = plan[i]                # the step's precision: its engine and that engine's condition canvas
            eng_i, cond_canvas = engines[prec_i], canvases[prec_i]
            if precision_log is not None:
                precision_log.append(prec_i)
            passes, kind, scale = _step_guidance(i, cond_scale, guidance_start_steps, class_cond_scale,
                                                 class_guidance_start_steps, joint)
            step_tiles = _launch_tiles(passes, sub_batch)
            n_tiles = len(grids[i % 2])
            last = i == num_sample_steps - 1
            noise_tiles = noise_canvas = None
            if host_noise:
                # identical to the reference's per-minibatch randn_like draws (SURVEY Appendix D:
                # 16-element block property makes one contiguous draw equal to the minibatch draws)
                if not last:
                    noise_tiles = _host_randn(self.host_generator, n_tiles, 3, tile_size, tile_size).to(dev, non_blocking=True)
                if i % 2 == 1:
                    noise_canvas = _host_randn(self.host_generator, 1, 3, hp, wp).to(dev, non_blocking=True)
            n_step = n_tiles * batch
            n_lanes = lanes_wanted(n_step, passes, step_tiles, self.step_lanes, prec_i) \
                if self.canvas_group is None and regional is None else 1
            if regional is not None:        # the tiles that touch R, without the ring: it lies outside R and is replaced below
                for first, count, ring in regional.step_ranges(i):
                    _ddpm_step(eng_i, i, (first, count, ring), img, cond_canvas, x_start, noise_tiles, noise_canvas, passes, kind, scale,
                               step_tiles, self.device_noise_seed)
            elif n_lanes > 1:
                lanes = lanes_of.get(prec_i)
                if lanes is None or len(lanes.engines) != n_lanes:   # further engines: same run geometry, own copies of the condition canvas
                    more = [self.model.engine(prec_i, lane=k) for k in range(1, n_lanes)]
                    for e_ in more:
                        begin(e_, torch.empty_like(cond_canvas))
                    lanes = lanes_of[prec_i] = StepLanes([eng_i] + more, dev)
                lanes.run(n_step, lambda e_, first, count, ring: _ddpm_step(
                    e_, i, (first, count, ring), img, cond_canvas, x_start, noise_tiles, noise_canvas, passes, kind, scale, step_tiles,
                    self.device_noise_seed))
            elif self.canvas_group is None:
                _ddpm_step(eng_i, i, None, img, cond_canvas, x_start, noise_tiles, noise_canvas, passes, kind, scale, step_tiles,
                           self.device_noise_seed)
            else:
                from .parallel import sharded_step
                sharded_step(eng_i, self.canvas_group, i, n_tiles * batch, img, cond_canvas, x_start, noise_tiles,
                             noise_canvas, passes, kind, scale, sub_batch, self.device_noise_seed)
            if thresholded is not None:     # the lanes have joined the main stream: plain launches after the step's
                thresholded.step(i, scalars, img, x_start)
            if guided is not None:          # after the threshold: it corrects the completed prediction
                guided.step(i, scalars, img, x_start, cond01)
            if history is not None:         # after the guidance: the history holds the corrected predictions
                history.step(i, img, x_start)
            if regional is not None:        # last: the canvases outside R are the known image at the step's end level
                regional.after_step(i, scalars, img, x_start)
            if with_images:
                image_list.append(img.clone().cpu())
            if with_x0_images:
                x0_image_list.append(x_start.clone().cpu())

        out = torch.empty(batch, 3, h, w, device=dev, dtype=torch.float32)
        eng_i.sampler_end(img, out)         # the engine of the last executed step
        if thresholded is not None and threshold_log is not None:
            threshold_log.append(thresholded.log())
        if color_fix is not None:           # in place on the [B,3,H,W] result; the trajectories above stay raw
            color_fix_flat(out, cond01, [b * 3 * h * w for b in range(batch)], [(h, w)] * batch, color_fix)
        if back_project is not None:        # after the colour fix, in place: the image as it will be saved
            back_project_flat(out.view(-1), cond01.view(-1), [b * 3 * h * w for b in range(batch)], [(h, w)] * batch, back_project)
        if regional is not None:            # the image as saved: outside R it is the known image, bit for bit
            regional.composite(out)
            if region_log is not None:
                region_log.extend(regional.log)
        ret = ((out, image_list, x0_image_list) if with_x0_images else (out, image_list)) if with_images else out
        if reference is not None:           # of the image as saved: after the colour fix
            quality = metrics_flat(out.view(-1), reference[0], [b * 3 * h * w for b in range(batch)], reference[1], [(h, w)] * batch,
                                   crop_border)
            return ret + (quality,) if with_images else (out, quality)
        return ret

    def _tiled_sample_images(self, batch_size, tile_size, conds, class_label, cond_scale, guidance_start_steps,
                             class_cond_scale, class_guidance_start_steps, generation_start_steps, num_sample_steps,
                             start_white_noise, precision, seeds=None, color_fix=None, reference=None, crop_border=4,
                             back_project=None, guidance=None, solver=None, threshold=None, threshold_log=None, joint=False,
                             region=None, region_skip_tiles=True, region_log=None, precision_schedule=None, precision_log=None):
        """Mixed-size lock-step (srgd_sampler_begin_images): every image keeps its own canvas, crop box, padding, inner box and
        tile grids; a step's tiles of all images share the U-Net launches.  Noise: the images of one noise class (canvas size)
        see the draw sequence a run of one of them alone sees.  Host noise: the generator state is taken once at entry and
        each class draws from its own generator started at that state, in the reference's order; on return the caller's
        generator (``host_generator`` or torch's global one) holds the state a run of the FIRST image alone would leave.

        ``seeds`` (one per image, validated by the caller): a noise class is a noise stream (canvas size, seed).  Host noise:
        stream k draws from a private ``torch.Generator().manual_seed(seed_k)`` - the stream of the global generator after
        ``torch.manual_seed(seed_k)`` - and the caller's generator is left alone.  Device noise: every engine of the run gets
        the streams' seeds (srgd_sampler_noise_seeds) and draws all of them in one launch per use.

        ``reference``: None, or ``(flat uint8 buffer, byte offsets)`` of the images' ground truth (``pack_references``); the return
        value is then ``(outputs, list of metric dicts)``.

        ``guidance``: None, or ``(weight, start step)`` of ``consistency_guidance`` (validated by the caller): the run keeps an
        ``x_start`` buffer laid out like ``img`` and makes one batched guidance call for all images after every guided step.

        ``solver``: None, or ``(sampler, eta, step_spacing)`` of a non-default sampler (validated by the caller): the step table and
        the levels are ``_schedule``'s of it; "dpmpp2m" keeps ``x_start`` and a history buffer and makes one batched history call
        for all images after every step, after the guidance call.

        ``threshold``: None, or the fp32 percentile of ``dynamic_threshold`` (validated by the caller): the step table is built with
        ``no_clamp``, the run keeps ``x_start`` and makes one batched threshold call for all images after every executed step, before
        the guidance call; ``threshold_log`` (a list or None) receives the [executed steps, images] tensor of s.

        ``joint``: ``joint_guidance`` is active (validated by the caller): steps with both scales current are three-pass steps.

        ``region``: None, or ``check_region_args``'s list of one ``None`` / ``(known image, boxes)`` per image (validated by the
        caller): the run's ``_RegionRun`` plans the tile ranges of every step over all images - an image without a known image keeps
        all its tiles - and makes the replacement step after the history call; lanes are off.

        ``precision_schedule``: None, or the parsed schedule of the call (validated by the caller; without it and without
        ``precision`` the wrapper's attribute holds): every precision with an executed step has its engine begun with the run and
        its own condition canvas, and step i runs on the engine of its precision; ``precision_log`` (a list or None) receives the
        precision of every executed step."""
        from .lockstep import plan_mixed_group
        dev = self.device
        if dev.type != "cuda":
            raise _lib.SrgdHipError("tiled_sample runs on MI355X only (no CPU fallback)")
        if not conds:
            raise ValueError("condition_x: empty list")
        for c in conds:
            if not torch.is_tensor(c) or c.dim() != 4 or c.shape[0] != 1 or c.shape[1] != 3:
                raise ValueError("a list condition_x holds [1,3,H,W] tensors")
        sizes = [(int(c.shape[2]), int(c.shape[3])) for c in conds]
        class_seeds = None
        if seeds is None:
            plans, classes = plan_mixed_group(sizes, tile_size)
        else:
            plans, classes, class_seeds = plan_mixed_group(sizes, tile_size, seeds=seeds)
        plan, names = self._precision_plan(precision, precision_schedule, num_sample_steps, generation_start_steps)
        class_id, image_ids = _run_labels(_image_class_ids(class_label, len(conds)))
        engines = {name: self.model.engine(name) for name in names}
        eng = engines[names[0]]             # of the first executed step: the start canvas and the region run's draws
        images = [_lib.SamplerImage(H=p.H, W=p.W, Hp=p.Hp, Wp=p.Wp, left=p.box[0], top=p.box[1], inner_l=p.inner[0],
                                    inner_t=p.inner[1], inner_r=p.inner[2], inner_b=p.inner[3], n_even=len(p.coords0),
                                    n_odd=len(p.coords1), noise_class=p.noise_class) for p in plans]
        tiles_even = [(a, c_) for p in plans for (a, _, c_, _) in p.coords0]
        tiles_odd = [(a, c_) for p in plans for (a, _, c_, _) in p.coords1]
        scalars, log_snrs = _schedule_of(num_sample_steps, solver, no_clamp=threshold is not None)
        sampler_name, step_spacing = ("ddpm", "time") if solver is None else (solver[0], solver[2])
        cond01 = torch.cat([c.to(dev, torch.float32).reshape(-1) for c in conds])
        cond_canvas = torch.empty(sum(3 * p.Hp * p.Wp for p in plans), device=dev, dtype=torch.float32)

        host_noise = self.noise_source == "host"

        def begin(e_, canvas):
            e_.sampler_begin_images(tile_size, images, cond01, canvas, tiles_even, tiles_odd, scalars, log_snrs, class_id)
            if image_ids is not None:
                e_.sampler_image_labels(image_ids)
            if class_seeds is not None and not host_noise:   # host noise arrives drawn: the engine makes no draw of its own
                e_.sampler_noise_seeds(class_seeds)
        # every precision of the plan: its engine begun with the same run and its own copy of the condition canvas
        canvases = {name: cond_canvas if name == names[0] else torch.empty_like(cond_canvas) for name in names}
        for name in names:
            begin(engines[name], canvases[name])

        first_of_class = [next(p for p in plans if p.noise_class == k) for k in range(len(classes))]
        if host_noise:
            if class_seeds is not None:     # a private generator per stream; the caller's is neither read nor advanced
                gens = [torch.Generator().manual_seed(s_) for s_ in class_seeds]
            else:
                caller_gen = self.host_generator if self.host_generator is not None else torch.default_generator
                state = caller_gen.get_state()
                gens = []
                for _ in classes:
                    g_ = torch.Generator()
                    g_.set_state(state)
                    gens.append(g_)

            def draw(shape_of_class):       # per-class draws in class order, concatenated (the engine's noise layout)
                return torch.cat([_host_randn(g_, *shape_of_class(k)).reshape(-1) for k, g_ in enumerate(gens)]).to(dev)

            def canvas_draw():
                return draw(lambda k: (1, 3) + classes[k])
        if generation_start_steps > 0 or not start_white_noise:
            ls0 = _start_log_snr(generation_start_steps, num_sample_steps, step_spacing)
            img = torch.empty_like(cond_canvas)
            eng.sampler_q_start(cond01, canvas_draw() if host_noise else None, float(ls0.sigmoid().sqrt()),
                                float((-ls0).sigmoid().sqrt()), img, self.device_noise_seed)
        else:
            offs = [0]
            for (hp, wp) in classes:
                offs.append(offs[-1] + 3 * hp * wp)
            if host_noise:
                start = canvas_draw()
            elif class_seeds is not None:   # every stream's canvas from its own seed, one launch
                start = eng.randn_streams_(torch.empty(offs[-1], device=dev), offs[:-1],
                                           [b_ - a_ for a_, b_ in zip(offs, offs[1:])], class_seeds, 0)
            else:                           # the counter-based draw of each class's canvas, as a run alone draws it
                start = torch.cat([eng.randn_(torch.empty(3 * hp * wp, device=dev), self.device_noise_seed, 0)
                                   for (hp, wp) in classes])
            img = torch.cat([start[offs[p.noise_class]:offs[p.noise_class + 1]] for p in plans])

        x_start = guided = history = thresholded = None
        canvas_offs, cond_offs = [0], [0]
        for p in plans:
            canvas_offs.append(canvas_offs[-1] + 3 * p.Hp * p.Wp)
            cond_offs.append(cond_offs[-1] + 3 * p.H * p.W)
        regional = None
        if region is not None:              # the start canvases outside R: the known images at the start level
            regional = _RegionRun(eng, [RegionImage(canvas_offs[k], cond_offs[k], p.Hp, p.Wp, p.box[1], p.box[0], p.H, p.W, p.coords0,
                                                    p.coords1, p.noise_class, None if region[k] is None else region[k][1])
                                        for k, p in enumerate(plans)],
                                  [None if r is None else r[0] for r in region], classes,
                                  class_seeds if class_seeds is not None else [self.device_noise_seed] * len(classes),
                                  num_sample_steps, region_skip_tiles, dev, canvas_offs[-1], cond_offs[-1])
            ls0 = _start_log_snr(generation_start_steps, num_sample_steps, step_spacing)
            regional.replace(num_sample_steps, float(ls0.sigmoid().sqrt()), float((-ls0).sigmoid().sqrt()), img)
        if guidance is not None or sampler_name == "dpmpp2m" or threshold is not None:
            x_start = img.clone()
        if threshold is not None:
            thresholded = _ThresholdRun(threshold, [(canvas_offs[k], p.Hp, p.Wp, p.box[1], p.box[0], p.H, p.W, p.inner[1], p.inner[0],
                                                     p.inner[3] - p.inner[1], p.inner[2] - p.inner[0]) for k, p in enumerate(plans)],
                                        num_sample_steps - generation_start_steps, dev)
        if sampler_name == "dpmpp2m":       # every image's inner box: what is never re-noised
            history = _SolverRun(num_sample_steps, step_spacing, generation_start_steps,
                                 [(canvas_offs[k], p.Hp, p.Wp, p.inner[1], p.inner[0], p.inner[3] - p.inner[1], p.inner[2] - p.inner[0])
                                  for k, p in enumerate(plans)], x_start)
        if guidance is not None:
            guided = _GuidedRun(guidance, [(canvas_offs[k], cond_offs[k], p.Hp, p.Wp, p.box[1], p.box[0], p.H, p.W)
                                           for k, p in enumerate(plans)], dev)

        sub_batch = self.max_tiles_per_launch or batch_size
        n_grid = (len(tiles_even), len(tiles_odd))
        lanes_of = {}                       # one StepLanes per precision, built on first need
        eng_i = eng
        for i in range(num_sample_steps):
            if i < generation_start_steps:
                continue
            prec_i = plan[i]                # the step's precision: its engine and that engine's condition canvas
            eng_i, cond_canvas = engines[prec_i], canvases[prec_i]
            if precision_log is not None:
                precision_log.append(prec_i)
            passes, kind, scale = _step_guidance(i, cond_scale, guidance_start_steps, class_cond_scale,
                                                 class_guidance_start_steps, joint)
            step_tiles = _launch_tiles(passes, sub_batch)
            last = i == num_sample_steps - 1
            noise_tiles = noise_canvas = None
            if host_noise:                  # each class in the reference's order: the step's tile noise, then the odd-step ring
                if not last:
                    noise_tiles = draw(lambda k: (len((first_of_class[k].coords0, first_of_class[k].coords1)[i % 2]), 3,
                                                  tile_size, tile_size))
                if i % 2 == 1:
                    noise_canvas = canvas_draw()
            n_step = n_grid[i % 2]
            n_lanes = lanes_wanted(n_step, passes, step_tiles, self.step_lanes, prec_i) if regional is None else 1
            if regional is not None:        # the tiles that touch R (all tiles of an image sampled whole)
                for first, count, ring in regional.step_ranges(i):
                    _ddpm_step(eng_i, i, (first, count, ring), img, cond_canvas, x_start, noise_tiles, noise_canvas, passes, kind, scale,
                               step_tiles, self.device_noise_seed)
            elif n_lanes > 1:
                lanes = lanes_of.get(prec_i)
                if lanes is None or len(lanes.engines) != n_lanes:   # further engines: the same mixed run, own condition canvas
                    more = [self.model.engine(prec_i, lane=k) for k in range(1, n_lanes)]
                    for e_ in more:
                        begin(e_, torch.empty_like(cond_canvas))
                    lanes = lanes_of[prec_i] = StepLanes([eng_i] + more, dev)
                lanes.run(n_step, lambda e_, first, count, ring: _ddpm_step(
                    e_, i, (first, count, ring), img, cond_canvas, x_start, noise_tiles, noise_canvas, passes, kind, scale, step_tiles,
                    self.device_noise_seed))
            else:
                _ddpm_step(eng_i, i, None, img, cond_canvas, x_start, noise_tiles, noise_canvas, passes, kind, scale, step_tiles,
                           self.device_noise_seed)
            if thresholded is not None:
                thresholded.step(i, scalars, img, x_start)
            if guided is not None:
                guided.step(i, scalars, img, x_start, cond01)
            if history is not None:
                history.step(i, img, x_start)
            if regional is not None:
                regional.after_step(i, scalars, img, x_start)

        out = torch.empty(sum(3 * p.H * p.W for p in plans), device=dev, dtype=torch.float32)
        eng_i.sampler_end(img, out)         # the engine of the last executed step
        if thresholded is not None and threshold_log is not None:
            threshold_log.append(thresholded.log())
        starts = [0]
        for p in plans:
            starts.append(starts[-1] + 3 * p.H * p.W)
        if color_fix is not None:           # on the run's flat buffers: out and cond01 share the per-image layout
            color_fix_flat(out, cond01, starts[:-1], [(p.H, p.W) for p in plans], color_fix)
        if back_project is not None:        # after the colour fix, in place: the images as they will be saved
            back_project_flat(out, cond01, starts[:-1], [(p.H, p.W) for p in plans], back_project)
        if regional is not None:            # the images as saved: outside R the known image, bit for bit
            regional.composite(out)
            if region_log is not None:
                region_log.extend(regional.log)
        quality = None
        if reference is not None:           # on the same flat layout, after the colour fix
            quality = metrics_flat(out, reference[0], starts[:-1], reference[1], [(p.H, p.W) for p in plans], crop_border)
        if host_noise and class_seeds is None:
            caller_gen.set_state(gens[plans[0].noise_class].get_state())
        outs, off = [], 0
        for p in plans:
            outs.append(out[off:off + 3 * p.H * p.W].view(1, 3, p.H, p.W))
            off += 3 * p.H * p.W
        return outs if reference is None else (outs, quality)

    @torch.inference_mode()
    def sample(self, batch_size=16, condition_x=None, class_label=None, cond_scale=1.0, guidance_start_steps=0,
               class_cond_scale=1.0, class_guidance_start_steps=0, generation_start_steps=0, num_sample_steps=None,
               with_images=False, with_x0_images=False, x0=None, amp=False, precision=None, joint_guidance=False):
        """Un-tiled sampling of a batch of ``image_size`` x ``image_size`` images (reference model.py:3417-3432,
        p_sample_loop :3191-3247): every image has its own noise (one ``randn`` over ``[B,3,S,S]`` per draw, host mode).

        Runs on the tiled machinery: the batch is laid out as one canvas of B stacked tiles (``[3, B*S, S]``, no padding, no
        ring re-noise), so one U-Net launch covers the whole batch.  Needs ``image_size == 256`` (the tile edge of the kernels;
        the shipped config).  ``amp`` / ``precision`` as in ``tiled_sample``.  ``joint_guidance`` is ``tiled_sample``'s: both scales
        are refused here with or without it."""
        num_sample_steps = self.num_sample_steps if num_sample_steps is None else num_sample_steps
        if cond_scale != 1.0 and class_cond_scale != 1.0:
            raise NotImplementedError("Currently, you cannot specify both cond_scale and class_cond_scale at the same time.")
        s_ = self.image_size
        if s_ != 256:
            raise NotImplementedError(f"sample(): image_size={s_}; this engine's un-tiled path needs image_size == 256")
        dev = self.device
        if dev.type != "cuda":
            raise _lib.SrgdHipError("sample runs on MI355X only (no CPU fallback)")
        b = int(batch_size)
        if tuple(condition_x.shape) != (b, self.channels, s_, s_):
            raise ValueError(f"condition_x must be [{b},{self.channels},{s_},{s_}] (model.py:3426 pairs it with the noise batch)")
        eng = self.model.engine(precision or self.precision)
        class_id = _single_class_id(class_label)
        to_canvas = lambda t: t.permute(1, 0, 2, 3).reshape(1, 3, b * s_, s_).contiguous()       # [B,3,S,S] -> [1,3,B*S,S]
        from_canvas = lambda t: t.reshape(3, b, s_, s_).permute(1, 0, 2, 3).contiguous()
        tiles = [(i * s_, 0) for i in range(b)]
        geo = SamplerGeometry(H=b * s_, W=s_, Hp=b * s_, Wp=s_, left=0, top=0, inner_l=0, inner_t=0, inner_r=s_, inner_b=b * s_,
                              tile=s_, n_even=b, n_odd=b, n_images=1)
        scalars, log_snrs = _schedule(num_sample_steps)
        cond01 = to_canvas(condition_x.to(dev, torch.float32))
        cond_canvas = torch.empty(1, 3, b * s_, s_, device=dev, dtype=torch.float32)
        eng.sampler_begin(geo, cond01, cond_canvas, tiles, tiles, scalars, log_snrs, class_id)
        host_noise = self.noise_source == "host"
        seed = self.device_noise_seed
        if generation_start_steps > 0:                                   # q_sample(condition, t_start) :3198-3201
            ls0 = beta_linear_log_snr(1.0 - torch.tensor(generation_start_steps / num_sample_steps))
            img = torch.empty(1, 3, b * s_, s_, device=dev)
            nz = to_canvas(_host_randn(self.host_generator, b, 3, s_, s_).to(dev)) if host_noise else None
            eng.sampler_q_start(cond01, nz, float(ls0.sigmoid().sqrt()), float((-ls0).sigmoid().sqrt()), img, seed)
        elif host_noise:
            img = to_canvas(_host_randn(self.host_generator, b, 3, s_, s_).to(dev))           # :3203
        else:
            img = eng.randn_(torch.empty(1, 3, b * s_, s_, device=dev), seed, 0)
        x_start = img.clone() if with_x0_images else None
        image_list = [from_canvas(img).cpu()] if with_images else None
        x0_image_list = [from_canvas(img).cpu()] if with_x0_images else None
        for i in range(num_sample_steps):
            if i < generation_start_steps:
                continue
            cur_cond_scale = 1.0 if i < guidance_start_steps else cond_scale
            cur_class_scale = 1.0 if i < class_guidance_start_steps else class_cond_scale
            if cur_cond_scale != 1.0:
                passes, kind, scale = 2, 2, cur_cond_scale
            elif cur_class_scale != 1.0:
                passes, kind, scale = 2, 1, cur_class_scale
            else:
                passes, kind, scale = 1, 0, 1.0
            last = i == num_sample_steps - 1
            noise_tiles = _host_randn(self.host_generator, b, 3, s_, s_).to(dev, non_blocking=True) if (host_noise and not last) else None
            # no ring re-noise in the un-tiled loop: run the step over all tiles with do_ring = False
            eng.sampler_step_tiles(i, 0, b, False, img, cond_canvas, x_start, noise_tiles, None, passes, kind, scale,
                                   self.max_tiles_per_launch or b, seed=seed)
            if with_images:
                image_list.append(from_canvas(img).cpu())
            if with_x0_images:
                x0_image_list.append(from_canvas(x_start).cpu())
        out = torch.empty(1, 3, b * s_, s_, device=dev, dtype=torch.float32)
        eng.sampler_end(img, out)
        out = from_canvas(out)
        if with_images:
            return (out, image_list, x0_image_list) if with_x0_images else (out, image_list)
        return out

    def forward(self, *args, **kwargs):
        raise NotImplementedError("training (p_losses) is not part of the inference-only release this engine mirrors")


# ---------------------------------------------------------------------------------------------
# EDM (Karras et al.) sampler over the same U-Net (reference model.py:2059-2475)
# ---------------------------------------------------------------------------------------------
def _tiling(h: int, w: int, tile_size: int, tile_stride: int):
    """Canvas + both tile grids of one image (reference model.py:2321-2323, :2360-2371 / :3301-3342)."""
    (left, top, right, bottom), pad = get_coord_and_pad(h, w)
    hp, wp = h + pad[2] + pad[3], w + pad[0] + pad[1]
    if max(pad[0], pad[1]) >= w or max(pad[2], pad[3]) >= h:
        raise RuntimeError("Padding size should be less than the corresponding input dimension "
                           f"(reflect pad {pad} of a {h}x{w} image)")
    coords0 = get_coords(hp, wp, tile_size, tile_size, diff=0)
    if hp <= tile_size and wp <= tile_size:
        coords1 = get_coords(hp, wp, tile_size, tile_stride, diff=0)
    else:
        coords1 = get_coords(hp - tile_size, wp - tile_size, tile_size, tile_stride, diff=tile_size // 2)
    inner, _ = get_area(coords1, hp, wp)
    return (left, top, right, bottom), (hp, wp), coords0, coords1, inner


class ConditionalElucidatedDiffusionSR(nn.Module):
    """``ConditionalElucidatedDiffusionSR`` of the reference (model.py:2059-2128 ctor, :2309-2475 ``tiled_sample``): Heun
    2nd-order EDM sampling, two U-Net evaluations per step, same tiling as the DDPM wrapper.

    The base class ``denoising_diffusion_pytorch.ElucidatedDiffusion`` (un-vendored, pinned 1.8.15) contributes the
    rho-schedule and the preconditioning coefficients; they are restated here from the published algorithm
    (``sample_schedule`` / ``c_in`` / ``c_skip`` / ``c_out`` / ``c_noise``) with torch fp32 ops, and handed to the engine as
    per-step scalars.  Inference only (``tiled_sample``, ``sample`` -> ``sample_org`` / ``sample_using_dpmpp``)."""

    def __init__(self, net, *, image_size, channels=3, num_sample_steps=32, sigma_min=0.002, sigma_max=80, sigma_data=0.5,
                 rho=7, P_mean=-1.2, P_std=1.2, S_churn=80, S_tmin=0.05, S_tmax=50, S_noise=1.003, cond_drop_prob=0.0,
                 class_cond_drop_prob=0.0, use_dpmpp_solver=False, loss_type="l2"):
        super().__init__()
        assert net.random_or_learned_sinusoidal_cond
        self.self_condition = net.self_condition
        self.net = net
        self.channels, self.image_size = channels, image_size
        self.sigma_min, self.sigma_max, self.sigma_data, self.rho = sigma_min, sigma_max, sigma_data, rho
        self.P_mean, self.P_std, self.num_sample_steps = P_mean, P_std, num_sample_steps
        self.S_churn, self.S_tmin, self.S_tmax, self.S_noise = S_churn, S_tmin, S_tmax, S_noise
        self.cond_drop_prob, self.class_cond_drop_prob = cond_drop_prob, class_cond_drop_prob
        self.use_dpmpp_solver, self.loss_type = use_dpmpp_solver, loss_type
        # engine knobs (not part of the reference surface)
        self.noise_source = "host"
        self.host_generator = None         # as in the DDPM wrapper: None = torch's global CPU generator
        self.device_noise_seed = 0
        self.max_tiles_per_launch = None
        self.step_lanes = lanes_setting_from_env()   # as in the DDPM wrapper
        self.precision = "fp32"            # as in the DDPM wrapper
        self.canvas_group = None           # set by srgd_amd.parallel.shard_canvas: tiles of every step split over its ranks

    def set_seed(self, seed):
        torch.cuda.manual_seed(seed)
        self.device_noise_seed = int(seed)

    @property
    def device(self):
        return next(self.net.parameters()).device

    # ---- the base class's published formulas (fp32 torch ops, as the reference evaluates them) ----
    def c_skip(self, sigma):
        return (self.sigma_data ** 2) / (sigma ** 2 + self.sigma_data ** 2)

    def c_out(self, sigma):
        return sigma * self.sigma_data * (self.sigma_data ** 2 + sigma ** 2) ** -0.5

    def c_in(self, sigma):
        return 1 * (sigma ** 2 + self.sigma_data ** 2) ** -0.5

    def c_noise(self, sigma):
        return torch.log(sigma.clamp(min=1e-20)) * 0.25

    def sample_schedule(self, num_sample_steps=None):
        n = self.num_sample_steps if num_sample_steps is None else num_sample_steps
        inv_rho = 1 / self.rho
        steps = torch.arange(n, dtype=torch.float32)
        sigmas = (self.sigma_max ** inv_rho + steps / (n - 1) * (self.sigma_min ** inv_rho - self.sigma_max ** inv_rho)) ** self.rho
        return torch.nn.functional.pad(sigmas, (0, 1), value=0.0)

    def _step_tables(self, n: int, clamp: bool, with_ring: bool = True):
        """Per-step scalars of the Heun loops.  ``with_ring``: the tiled loop re-noises the ring on odd steps from the
        CONSTRUCTOR's schedule (below); the un-tiled ``sample_org`` never does (model.py:2212-2306 has no get_noised_images
        call per step) and so runs with any per-call step count.  Odd steps beyond the constructor's schedule get
        ``ring_sigma = nan`` here; ``tiled_sample`` raises upstream's IndexError when the loop reaches the first of them."""
        from ._lib import EdmScalars
        sigmas = self.sample_schedule(n)
        # get_noised_images (model.py:2186-2189) is called without num_sample_steps at :2342 and :2457, so the
        # generation-start sigma and the odd-step ring sigmas come from the CONSTRUCTOR's schedule, not the per-call one
        noised_sigmas = self.sample_schedule(self.num_sample_steps)
        gammas = torch.where((sigmas >= self.S_tmin) & (sigmas <= self.S_tmax),
                             min(self.S_churn / n, math.sqrt(2) - 1), 0.0)                      # model.py:2333-2337
        scalars, c_noise = [], []
        for i in range(n):
            sigma, sigma_next, gamma = sigmas[i].item(), sigmas[i + 1].item(), gammas[i].item()
            sigma_hat = sigma + gamma * sigma                                                    # :2388
            sh, sn = torch.full((1,), sigma_hat), torch.full((1,), sigma_next)                   # :2137 fp32 tensors
            scalars.append(EdmScalars(
                s_noise=self.S_noise, hat_coef=math.sqrt(sigma_hat ** 2 - sigma ** 2), sigma_hat=sigma_hat,
                sigma_next=sigma_next, dt=sigma_next - sigma_hat, half_dt=0.5 * (sigma_next - sigma_hat),
                c_in_hat=float(self.c_in(sh)), c_skip_hat=float(self.c_skip(sh)), c_out_hat=float(self.c_out(sh)),
                c_in_next=float(self.c_in(sn)), c_skip_next=float(self.c_skip(sn)), c_out_next=float(self.c_out(sn)),
                # read on odd steps of the tiled loop only; upstream indexes its constructor-length schedule there
                ring_sigma=(float(noised_sigmas[i]) if i < len(noised_sigmas) else math.nan) if (with_ring and i % 2 == 1) else 0.0,
                clamp=1.0 if clamp else 0.0, dpm_gamma=0.0, pad1=0.0))
            c_noise += [float(self.c_noise(sh)), float(self.c_noise(sn))]
        return sigmas, noised_sigmas, scalars, c_noise

    @torch.inference_mode()
    def tiled_sample(self, batch_size=4, tile_size=256, tile_stride=256, condition_x=None, class_label=None,
                     cond_scale=1.0, guidance_start_steps=0, class_cond_scale=1.0, class_guidance_start_steps=0,
                     generation_start_steps=0, num_sample_steps=None, clamp=True, zero_init=False, with_images=False,
                     with_x0_images=False, start_white_noise=True, amp=False, precision=None, seeds=None, color_fix=None,
                     reference=None, crop_border=4, back_project=0, consistency_guidance=0.0, consistency_guidance_start_steps=0,
                     sampler="ddpm", eta=None, step_spacing="time", dynamic_threshold=None, threshold_log=None,
                     joint_guidance=False, region_known=None, regions=None, region_skip_tiles=True, region_log=None,
                     precision_schedule=None, precision_log=None):
        """Reference model.py:2309-2475 (``start_white_noise`` and ``amp`` are accepted and unused there too; ``precision``
        is the engine-only override of ``self.precision``).  ``seeds`` (per-image noise seeds) is a DDPM-sampler feature and is
        refused here.  ``color_fix``: as in the DDPM wrapper's ``tiled_sample`` - the final image of every image of the batch
        colour-corrected against its condition, trajectories raw.  ``reference`` / ``crop_border``: as there too - the ground
        truth of every image of the batch; the return value gains a trailing list of metric dicts.  ``back_project``: as there
        too - N back-projection steps on the final image, after the colour fix and before the metrics.
        ``consistency_guidance``: a DDPM-sampler feature; a non-zero weight is refused here.
        ``sampler``, ``eta``, ``step_spacing``: the DDPM wrapper's few-step samplers; any non-default value is refused here.
        ``dynamic_threshold``: a DDPM-sampler feature; a percentile other than None / 0 is refused here.
        ``joint_guidance``: a DDPM-sampler feature; both scales are refused here with or without it.
        ``region_known`` / ``regions``: region resampling is a DDPM-sampler feature and is refused here.
        ``precision_schedule`` / ``precision_log``: a precision per step is a DDPM-sampler feature and is refused here."""
        if precision_schedule is not None or precision_log is not None:
            raise NotImplementedError("precision_schedule is built for the DDPM sampler only: the EDM loop begins one engine per run")
        if region_known is not None or regions is not None:
            raise NotImplementedError("region_known / regions are built for the DDPM sampler only: the known image is forward-diffused "
                                      "with the DDPM schedule's (alpha, sigma) after every step")
        color_fix = check_mode(color_fix)
        back_project = _back_project_steps(back_project, condition_x)
        if check_percentile(dynamic_threshold) is not None:
            raise NotImplementedError("dynamic_threshold is built for the DDPM sampler only: its correction of the canvas rests on the "
                                      "DDPM posterior mean, linear in the predicted clean image (the EDM wrapper has its own clamp)")
        check_start_steps(consistency_guidance_start_steps)
        if check_weight(consistency_guidance) is not None:
            raise NotImplementedError("consistency_guidance is built for the DDPM sampler only: its correction of the canvas rests on "
                                      "the DDPM posterior mean, linear in the predicted clean image")
        if not is_default(*check_sampler(sampler, eta, step_spacing)):
            raise NotImplementedError("sampler / eta / step_spacing are built for the DDPM sampler only: the EDM wrapper has its own "
                                      "schedule and its own solvers (sample_using_dpmpp)")
        if reference is not None and not isinstance(condition_x, (list, tuple)):
            reference = _packed_reference(reference, condition_x, crop_border, self)
        n = self.num_sample_steps if num_sample_steps is None else num_sample_steps
        if isinstance(condition_x, (list, tuple)):
            raise NotImplementedError("mixed-size lock-step (a list condition_x) is built for the DDPM sampler only; "
                                      "sample EDM images one size at a time")
        if seeds is not None:
            raise NotImplementedError("seeds (per-image noise seeds) are built for the DDPM sampler only: the EDM step kernels "
                                      "address one noise canvas shared by all images")
        if cond_scale != 1.0 and class_cond_scale != 1.0:
            raise NotImplementedError("Currently, you cannot specify both cond_scale and class_cond_scale at the same time.")
        if tile_size != 256 or tile_stride != 256:
            raise NotImplementedError("tile_size/tile_stride other than 256 are unusable in the reference too "
                                      "(get_coord_and_pad is called without them, model.py:2321)")
        dev = self.device
        if dev.type != "cuda":
            raise _lib.SrgdHipError("tiled_sample runs on MI355X only (no CPU fallback)")
        batch, c, h, w = condition_x.shape
        if batch < 1 or c != 3:
            raise ValueError("condition_x must be [B,3,H,W] (B=1 in the reference; B>1 = same-sized images in lock-step, "
                             "each sampled as it would be alone with the same seed)")
        class_id, image_ids = _run_labels(_image_class_ids(class_label, batch))
        if image_ids is not None and self.canvas_group is not None:
            raise NotImplementedError("per-image class labels on a canvas sharded over ranks (canvas_group)")
        eng = self.net.engine(precision or self.precision)
        (left, top, right, bottom), (hp, wp), coords0, coords1, (sl, st_, sr, sb) = _tiling(h, w, tile_size, tile_stride)
        geo = SamplerGeometry(H=h, W=w, Hp=hp, Wp=wp, left=left, top=top, inner_l=sl, inner_t=st_, inner_r=sr,
                              inner_b=sb, tile=tile_size, n_even=len(coords0), n_odd=len(coords1), n_images=batch)
        sigmas, noised_sigmas, scalars, c_noise = self._step_tables(n, clamp)
        cond01 = condition_x.to(dev, torch.float32).contiguous()
        cond_canvas = torch.empty(batch, 3, hp, wp, device=dev, dtype=torch.float32)
        eng.edm_begin(geo, cond01, cond_canvas, [(a, c_) for (a, _, c_, _) in coords0],
                      [(a, c_) for (a, _, c_, _) in coords1], scalars, c_noise, class_id)
        if image_ids is not None:
            eng.sampler_image_labels(image_ids)
        host_noise = self.noise_source == "host"
        seed = self.device_noise_seed

        def canvas_noise(stream_id):
            if host_noise:
                return _host_randn(self.host_generator, 1, 3, hp, wp).to(dev, non_blocking=True)
            return eng.randn_(torch.empty(1, 3, hp, wp, device=dev), seed, stream_id)

        if generation_start_steps > 0:                                  # get_noised_images(condition, step) :2340, :2185
            img = torch.empty(batch, 3, hp, wp, device=dev)
            eng.sampler_q_start(cond01, canvas_noise(1), 1.0, float(noised_sigmas[generation_start_steps]), img, seed)
        elif zero_init:
            img = torch.zeros(batch, 3, hp, wp, device=dev)
        else:
            img = (canvas_noise(1) * float(sigmas[0])).repeat(batch, 1, 1, 1)   # :2346 (a tensor * tensor product upstream)
        x_start = img.clone() if with_x0_images else None
        image_list = [img[:, :, top:bottom, left:right].clone().cpu()] if with_images else None
        x0_image_list = [img[:, :, top:bottom, left:right].clone().cpu()] if with_x0_images else None
        work = torch.empty(2, batch, 3, hp, wp, device=dev, dtype=torch.float32)
        sub_batch = self.max_tiles_per_launch or batch_size
        lanes = None
        for i in range(n):
            if i < generation_start_steps:
                continue
            cur_cond_scale = 1.0 if i < guidance_start_steps else cond_scale
            cur_class_scale = 1.0 if i < class_guidance_start_steps else class_cond_scale
            if cur_cond_scale != 1.0:
                passes, kind, scale = 2, 2, cur_cond_scale
            elif cur_class_scale != 1.0:
                passes, kind, scale = 2, 1, cur_class_scale
            else:
                passes, kind, scale = 1, 0, 1.0
            if i % 2 == 1 and i >= len(noised_sigmas):
                # upstream fails here too, mid-loop: get_noised_images(images, i) indexes the constructor's schedule (:2457 -> :2187)
                raise IndexError(f"index {i} is out of bounds for dimension 0 with size {len(noised_sigmas)}")
            z = canvas_noise(None) if host_noise else None              # eps of the step (:2386), before the ring draw
            ring = canvas_noise(None) if (host_noise and i % 2 == 1) else None
            n_step = (len(coords1) if i % 2 else len(coords0)) * batch
            n_lanes = lanes_wanted(n_step, passes, sub_batch, self.step_lanes, precision or self.precision) if self.canvas_group is None else 1
            if n_lanes > 1:
                if lanes is None or len(lanes.engines) != n_lanes:   # further engines (srgd_amd.lanes): same run geometry
                    more = [self.net.engine(precision or self.precision, lane=k) for k in range(1, n_lanes)]
                    for e_ in more:
                        e_.edm_begin(geo, cond01, torch.empty_like(cond_canvas), [(a, c_) for (a, _, c_, _) in coords0],
                                     [(a, c_) for (a, _, c_, _) in coords1], scalars, c_noise, class_id)
                        if image_ids is not None:
                            e_.sampler_image_labels(image_ids)
                    lanes = StepLanes([eng] + more, dev)
                lanes.run(n_step, lambda e_, first, count, do_ring: e_.edm_step_tiles(
                    i, first, count, do_ring, img, cond_canvas, x_start, work, z, ring, passes, kind, scale, sub_batch, seed))
            elif self.canvas_group is None:
                eng.edm_step(i, img, cond_canvas, x_start, work, z, ring, passes, kind, scale, sub_batch, seed=seed)
            else:
                from .parallel import sharded_edm_step
                n_tiles = (len(coords1) if i % 2 else len(coords0)) * batch
                sharded_edm_step(eng, self.canvas_group, i, n_tiles, img, cond_canvas, x_start, work, z, ring, passes, kind,
                                 scale, sub_batch, seed)
            if with_images:
                image_list.append(img.clone().cpu())
            if with_x0_images:
                x0_image_list.append(x_start.clone().cpu())
        out = torch.empty(batch, 3, h, w, device=dev, dtype=torch.float32)
        eng.sampler_end(img, out)
        if color_fix is not None:
            color_fix_flat(out, cond01, [b * 3 * h * w for b in range(batch)], [(h, w)] * batch, color_fix)
        if back_project is not None:        # after the colour fix, in place: the image as it will be saved
            back_project_flat(out.view(-1), cond01.view(-1), [b * 3 * h * w for b in range(batch)], [(h, w)] * batch, back_project)
        ret = ((out, image_list, x0_image_list) if with_x0_images else (out, image_list)) if with_images else out
        if reference is not None:           # of the image as saved: after the colour fix
            quality = metrics_flat(out.view(-1), reference[0], [b * 3 * h * w for b in range(batch)], reference[1], [(h, w)] * batch,
                                   crop_border)
            return ret + (quality,) if with_images else (out, quality)
        return ret

    def _dpmpp_tables(self, n: int, clamp: bool):
        """Per-step scalars of ``sample_using_dpmpp`` (model.py:2513-2541), evaluated with the reference's fp32 tensor ops:
        preconditioning at sigma_i, update coefficients sigma_fn(t_next)/sigma_fn(t) and expm1(-h), multistep weight gamma."""
        from ._lib import EdmScalars
        sigmas = self.sample_schedule(n)
        t_fn = lambda sigma: sigma.log().neg()
        sigma_fn = lambda t: t.neg().exp()
        scalars, c_noise = [], []
        for i in range(n):
            si = torch.full((1,), sigmas[i].item())                                             # :2137 fp32 tensor
            t, t_next = t_fn(sigmas[i]), t_fn(sigmas[i + 1])
            h = t_next - t
            scalars.append(EdmScalars(
                s_noise=0.0, hat_coef=0.0, sigma_hat=float(sigmas[i]), sigma_next=float(sigmas[i + 1]),
                dt=float(sigma_fn(t_next) / sigma_fn(t)), half_dt=float((-h).expm1()),
                c_in_hat=float(self.c_in(si)), c_skip_hat=float(self.c_skip(si)), c_out_hat=float(self.c_out(si)),
                c_in_next=0.0, c_skip_next=0.0, c_out_next=0.0, ring_sigma=0.0, clamp=1.0 if clamp else 0.0,
                dpm_gamma=0.0, pad1=0.0))                                    # dpm_gamma: set per call (depends on the start step)
            c_noise += [float(self.c_noise(si)), 0.0]
        return sigmas, scalars, c_noise

    @torch.inference_mode()
    def sample(self, batch_size=16, condition_x=None, class_label=None, cond_scale=1.0, guidance_start_steps=0,
               class_cond_scale=1.0, class_guidance_start_steps=0, generation_start_steps=0, num_sample_steps=None,
               clamp=True, with_images=False, with_x0_images=False, zero_init=False, precision=None):
        """Reference model.py:2196-2209: un-tiled sampling of a ``[B,3,256,256]`` batch - the Heun loop ``sample_org``
        (:2212-2306), or ``sample_using_dpmpp`` when the wrapper was built with ``use_dpmpp_solver``."""
        fn = self.sample_using_dpmpp if self.use_dpmpp_solver else self.sample_org
        return fn(batch_size, condition_x, class_label, cond_scale, guidance_start_steps, class_cond_scale,
                  class_guidance_start_steps, generation_start_steps, num_sample_steps, clamp, with_images, with_x0_images,
                  zero_init, precision=precision)

    def _untiled_setup(self, batch_size, condition_x, class_label, cond_scale, class_cond_scale, generation_start_steps,
                       zero_init, sigma0, precision):
        """Shared front end of the two un-tiled loops: the batch becomes one canvas of B stacked tiles (``[1,3,B*S,S]``, no
        padding, empty ring) exactly as in the DDPM wrapper's ``sample``; returns the engine, layout helpers and the start
        canvas (model.py:2219-2244 / :2490-2503)."""
        if cond_scale != 1.0 and class_cond_scale != 1.0:
            raise NotImplementedError("Currently, you cannot specify both cond_scale and class_cond_scale at the same time.")
        dev = self.device
        if dev.type != "cuda":
            raise _lib.SrgdHipError("sample runs on MI355X only (no CPU fallback)")
        b = int(batch_size)
        s_ = 256
        if tuple(condition_x.shape) != (b, self.channels, s_, s_):
            raise NotImplementedError(f"condition_x must be [{b},{self.channels},{s_},{s_}]: this engine's un-tiled path runs "
                                      "256 x 256 images (the tile edge of its kernels; the shipped image_size)")
        if generation_start_steps > 0 and b not in (1, s_):
            # get_noised_images (model.py:2191-2193) multiplies a [B] sigma vector into a [B,3,h,w] tensor
            raise RuntimeError(f"The size of tensor a ({b}) must match the size of tensor b ({s_}) at non-singleton dimension 3")
        eng = self.net.engine(precision or self.precision)
        to_canvas = lambda t: t.permute(1, 0, 2, 3).reshape(1, 3, b * s_, s_).contiguous()       # [B,3,S,S] -> [1,3,B*S,S]
        from_canvas = lambda t: t.reshape(3, b, s_, s_).permute(1, 0, 2, 3).contiguous()
        tiles = [(i * s_, 0) for i in range(b)]
        geo = SamplerGeometry(H=b * s_, W=s_, Hp=b * s_, Wp=s_, left=0, top=0, inner_l=0, inner_t=0, inner_r=s_, inner_b=b * s_,
                              tile=s_, n_even=b, n_odd=b, n_images=1)
        cond01 = to_canvas(condition_x.to(dev, torch.float32))
        host_noise = self.noise_source == "host"
        seed = self.device_noise_seed

        def batch_noise(stream_id):
            if host_noise:
                return to_canvas(_host_randn(self.host_generator, b, 3, s_, s_).to(dev, non_blocking=True))
            return eng.randn_(torch.empty(1, 3, b * s_, s_, device=dev), seed, stream_id)

        def start(eng_):
            if generation_start_steps > 0:                               # get_noised_images: the CONSTRUCTOR's schedule
                img = torch.empty(1, 3, b * s_, s_, device=dev)
                sig = float(self.sample_schedule(self.num_sample_steps)[generation_start_steps])
                eng_.sampler_q_start(cond01, batch_noise(1), 1.0, sig, img, seed)
                return img
            if zero_init:
                return torch.zeros(1, 3, b * s_, s_, device=dev)
            return batch_noise(1) * sigma0
        from types import SimpleNamespace
        return SimpleNamespace(eng=eng, b=b, s=s_, dev=dev, geo=geo, tiles=tiles, cond01=cond01, from_canvas=from_canvas,
                               batch_noise=batch_noise, start=start, host_noise=host_noise, seed=seed)

    @staticmethod
    def _guidance(i, cond_scale, guidance_start_steps, class_cond_scale, class_guidance_start_steps):
        cur_cond_scale = 1.0 if i < guidance_start_steps else cond_scale
        cur_class_scale = 1.0 if i < class_guidance_start_steps else class_cond_scale
        if cur_cond_scale != 1.0:
            return 2, 2, cur_cond_scale
        if cur_class_scale != 1.0:
            return 2, 1, cur_class_scale
        return 1, 0, 1.0

    @torch.inference_mode()
    def sample_org(self, batch_size=16, condition_x=None, class_label=None, cond_scale=1.0, guidance_start_steps=0,
                   class_cond_scale=1.0, class_guidance_start_steps=0, generation_start_steps=0, num_sample_steps=None,
                   clamp=True, with_images=False, with_x0_images=False, zero_init=False, precision=None):
        """Reference model.py:2212-2306 (stochastic Heun, two network evaluations per step) on the tiled EDM machinery:
        the same per-step arithmetic as ``tiled_sample`` with one tile per image, per-image noise and no ring."""
        n = self.num_sample_steps if num_sample_steps is None else num_sample_steps
        sigmas, _, scalars, c_noise = self._step_tables(n, clamp, with_ring=False)
        u = self._untiled_setup(batch_size, condition_x, class_label, cond_scale, class_cond_scale, generation_start_steps,
                                zero_init, float(sigmas[0]), precision)
        eng, b, s_, dev = u.eng, u.b, u.s, u.dev
        cond_canvas = torch.empty(1, 3, b * s_, s_, device=dev, dtype=torch.float32)
        eng.edm_begin(u.geo, u.cond01, cond_canvas, u.tiles, u.tiles, scalars, c_noise, _single_class_id(class_label))
        img = u.start(eng)
        x_start = img.clone() if with_x0_images else None
        image_list = [u.from_canvas(img).cpu()] if with_images else None
        x0_image_list = [u.from_canvas(img).cpu()] if with_x0_images else None
        work = torch.empty(2, 1, 3, b * s_, s_, device=dev, dtype=torch.float32)
        for i in range(n):
            if i < generation_start_steps:
                continue
            passes, kind, scale = self._guidance(i, cond_scale, guidance_start_steps, class_cond_scale,
                                                 class_guidance_start_steps)
            z = u.batch_noise(None) if u.host_noise else None           # eps of the step (:2269)
            # the ring of this geometry is empty (inner area = the whole canvas): no second draw on odd steps
            eng.edm_step(i, img, cond_canvas, x_start, work, z, None, passes, kind, scale, self.max_tiles_per_launch or b,
                         seed=u.seed)
            if with_images:
                image_list.append(u.from_canvas(img).cpu())
            if with_x0_images:
                x0_image_list.append(u.from_canvas(x_start).cpu())
        out = torch.empty(1, 3, b * s_, s_, device=dev, dtype=torch.float32)
        eng.sampler_end(img, out)
        out = u.from_canvas(out)
        if with_images:
            return (out, image_list, x0_image_list) if with_x0_images else (out, image_list)
        return out

    @torch.inference_mode()
    def sample_using_dpmpp(self, batch_size=16, condition_x=None, class_label=None, cond_scale=1.0, guidance_start_steps=0,
                           class_cond_scale=1.0, class_guidance_start_steps=0, generation_start_steps=0,
                           num_sample_steps=None, clamp=True, with_images=False, with_x0_images=False, zero_init=False,
                           precision=None):
        """Reference model.py:2479-2557: DPM-Solver++(2M) in t = -log sigma, one network evaluation per step
        (``srgd_edm_dpmpp_step``); deterministic after the start canvas."""
        n = self.num_sample_steps if num_sample_steps is None else num_sample_steps
        sigmas, scalars, c_noise = self._dpmpp_tables(n, clamp)
        t_fn = lambda sigma: sigma.log().neg()
        for i in range(n):                                               # :2533-2538; old_denoised is None on the first
            first = i == max(generation_start_steps, 0)                  # executed step, the multistep term is dropped on the last
            if not first and sigmas[i + 1] != 0 and i > 0:
                t, t_next = t_fn(sigmas[i]), t_fn(sigmas[i + 1])
                r = (t - t_fn(sigmas[i - 1])) / (t_next - t)
                scalars[i].dpm_gamma = float(-1 / (2 * r))
        u = self._untiled_setup(batch_size, condition_x, class_label, cond_scale, class_cond_scale, generation_start_steps,
                                zero_init, float(sigmas[0]), precision)
        eng, b, s_, dev = u.eng, u.b, u.s, u.dev
        cond_canvas = torch.empty(1, 3, b * s_, s_, device=dev, dtype=torch.float32)
        eng.edm_begin(u.geo, u.cond01, cond_canvas, u.tiles, u.tiles, scalars, c_noise, _single_class_id(class_label))
        img = u.start(eng)
        x_start = img.clone() if with_x0_images else None
        image_list = [u.from_canvas(img).cpu()] if with_images else None
        x0_image_list = [u.from_canvas(img).cpu()] if with_x0_images else None
        old = torch.zeros(1, 3, b * s_, s_, device=dev, dtype=torch.float32)
        for i in range(n):
            if i < generation_start_steps:
                continue
            passes, kind, scale = self._guidance(i, cond_scale, guidance_start_steps, class_cond_scale,
                                                 class_guidance_start_steps)
            eng.edm_dpmpp_step(i, img, cond_canvas, x_start, old, passes, kind, scale, self.max_tiles_per_launch or b)
            if with_images:
                image_list.append(u.from_canvas(img).cpu())
            if with_x0_images:
                x0_image_list.append(u.from_canvas(x_start).cpu())
        out = torch.empty(1, 3, b * s_, s_, device=dev, dtype=torch.float32)
        eng.sampler_end(img, out)
        out = u.from_canvas(out)
        if with_images:
            return (out, image_list, x0_image_list) if with_x0_images else (out, image_list)
        return out

    def forward(self, *args, **kwargs):
        raise NotImplementedError("training is not part of the inference-only release this engine mirrors")


# ---------------------------------------------------------------------------------------------
# factory (reference model.py:3500-3666)
# ---------------------------------------------------------------------------------------------
class ModelEma(nn.Module):
    """Stand-in for ``timm.utils.ModelEmaV2`` as the reference uses it at inference: a holder whose
    ``.module`` is an eval-mode copy that receives ``ckpt['ema_model']`` (model.py:3657-3662)."""

    def __init__(self, model, decay=0.9999, device=None):
        super().__init__()
        self.module = copy.deepcopy(model)
        self.module.eval()
        self.decay, self.device = decay, device


def _parse_bool_list(text: str) -> Tuple[bool, ...]:
    table = {"true": True, "false": False}
    try:
        return tuple(table[t.strip().lower()] for t in text.split(","))
    except KeyError as exc:
        raise ValueError(f"full_attn must be a comma list of True/False, got {text!r}") from exc


def get_model(conf, logger):
    dim_mults = tuple(int(t) for t in conf.ddpm_unet_dim_mults.split(","))
    full_attn = _parse_bool_list(conf.full_attn)
    if conf.model not in ("conditional_continuous", "conditional_elucidated"):
        raise NotImplementedError(
            f"model={conf.model!r}: this engine covers the shipped 'conditional_continuous' path and the "
            "'conditional_elucidated' (EDM) sampler over the same U-Net (SURVEY.md section 8; the other wrappers have "
            "no released config or weights)")
    unet = ConditionalSRUnet(dim=conf.unet_dim, dim_mults=dim_mults, full_attn=full_attn,
                             learned_variance=conf.learned_variance,
                             learned_sinusoidal_cond=conf.learned_sinusoidal_cond,
                             learned_sinusoidal_dim=conf.learned_sinusoidal_dim, flash_attn=conf.flash_attn,
                             pixel_shuffle_upsample=conf.pixel_shuffle_upsample, num_classes=conf.num_classes)
    logger.info(f"ConditionalSRUnet: channels=6 dim={conf.unet_dim} dim_mults={conf.ddpm_unet_dim_mults} "
                f"num_classes={conf.num_classes}")
    assert conf.learned_sinusoidal_cond
    if conf.model == "conditional_elucidated":                          # reference model.py:3593-3614
        model = ConditionalElucidatedDiffusionSR(
            net=unet, image_size=conf.image_size, num_sample_steps=conf.num_sample_steps, sigma_min=conf.sigma_min,
            sigma_max=conf.sigma_max, sigma_data=conf.sigma_data, rho=conf.rho, P_mean=conf.P_mean, P_std=conf.P_std,
            S_churn=conf.S_churn, S_tmin=conf.S_tmin, S_tmax=conf.S_tmax, S_noise=conf.S_noise,
            cond_drop_prob=conf.cond_drop_prob, class_cond_drop_prob=conf.class_cond_drop_prob,
            use_dpmpp_solver=conf.use_dpmpp_solver, loss_type=conf.loss_type)
        logger.info(f"ConditionalElucidatedDiffusionSR: image_size={conf.image_size} num_sample_steps={conf.num_sample_steps}")
        ema_model = ModelEma(model, decay=conf.ema_decay)
        if conf.ckpt_path:
            ckpt = torch.load(conf.ckpt_path, map_location="cpu", weights_only=True)
            check = ema_model.module.load_state_dict(ckpt["ema_model"], strict=conf.load_strict)
            logger.info(f"load ema_model weight from : {conf.ckpt_path}")
            logger.info(f"check: {check}")
        return ema_model
    conf.use_dpmpp_solver = False
    model = ConditionalContinuousTimeGaussianDiffusionSR(
        unet, image_size=conf.image_size, noise_schedule=conf.noise_schedule,
        num_sample_steps=conf.num_sample_steps, clip_sample_denoised=conf.clip_sample_denoised,
        learned_schedule_net_hidden_dim=conf.learned_schedule_net_hidden_dim,
        learned_noise_schedule_frac_gradient=conf.learned_noise_schedule_frac_gradient,
        min_snr_loss_weight=conf.min_snr_loss_weight, min_snr_gamma=conf.min_snr_gamma,
        cond_drop_prob=conf.cond_drop_prob, class_cond_drop_prob=conf.class_cond_drop_prob,
        loss_type=conf.loss_type)
    logger.info(f"ConditionalContinuousTimeGaussianDiffusionSR: image_size={conf.image_size} "
                f"num_sample_steps={conf.num_sample_steps}")
    ema_model = ModelEma(model, decay=conf.ema_decay)
    if conf.ckpt_path:
        ckpt = torch.load(conf.ckpt_path, map_location="cpu", weights_only=True)
        check = ema_model.module.load_state_dict(ckpt["ema_model"], strict=conf.load_strict)
        logger.info(f"load ema_model weight from : {conf.ckpt_path}")
        logger.info(f"check: {check}")
    return ema_model
