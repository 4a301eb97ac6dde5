"""Device-noise sampling (noise_source = "device") against references, draw by draw.

a. ``philox_normal_kernel`` / ``philox_normal_streams_kernel`` against the CPU restatement (oracle/philox.py, itself pinned by
   tests/test_philox_cpu.py), element by element.  The counter word ``q >> 32`` is not reached: it needs more than 2^34
   elements (64 GiB) in one call.
b. The step-mixed ring stream observed directly in a run's canvas trajectory.
c. Whole runs against the CPU oracle fed, through ``ReplayNoise``, exactly the noise the engine draws
   (``philox.device_noise_draws``) - the same bars the host-noise runs are held to.

Lock-step groups (same size, mixed sizes, per-image seeds, per-image labels) are not repeated here: tests/test_engine_gpu.py,
test_mixed_lockstep_gpu.py, test_noise_seeds_gpu.py and test_class_labels_gpu.py tie every image of a device-noise group bit
for bit to its solo run, and the batched Philox kernel to the single-stream one; with the solo runs pinned here, the groups
follow by transitivity.

Tolerances.  a/b: the restatement rounds u1, u2 and theta as the kernel does; what is left is the device's __logf, sqrtf,
__sincosf and two float32 products.  The floor F is the max-abs distance of numpy's float32 evaluation from the float64 one
over the very elements compared (computed here, from the restatement alone; about 5e-7); the device gets 32 * F - a few
float32 ulps at radius <= 6.66 for the fast intrinsics - five orders below the O(1) error of a wrong counter, key, lane or
stream.  c: final images 1e-3 (the bar) and 2e-4 (practice) as test_tiled_sample_fp32_matches_reference; canvas trajectories
(in [-1,1] units, which the output map (v+1)/2 halves) twice that.  Every case first asserts, from the oracle's schedule alone,
that the draws it claims to pin enter at >= 100 x the canvas bar (0.2): a test cannot pin noise it cannot see.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import philox as P
from oracle import srgd_oracle as O
from srgd_amd.synth import synth_state_dict
from tests.test_engine_gpu import _report, _schema, build_edm_sampler, build_sampler

pytestmark = pytest.mark.gpu

DIM, SEED = 16, 71
BAR, PRACTICE = 1e-3, 2e-4                  # final pixels in [0,1]
CANVAS_BAR, CANVAS_PRACTICE = 2e-3, 4e-4    # canvas trajectories in [-1,1] units
VISIBLE = 100 * CANVAS_BAR                  # the blindness guard, canvas units
STREAMS = [0, 1, 1 << 32, (1 << 32) | 0x80000000, 2 << 32]


def _engine():
    return build_sampler(DIM).model.engine("fp32")


@functools.lru_cache(maxsize=None)
def _pair(n, seed, stream_id, step=None):
    """(float64 restatement, floor F over these elements)"""
    z = P.philox_normal(n, seed, stream_id, step)
    f = float(np.abs(P.philox_normal(n, seed, stream_id, step, dtype=np.float32).astype(np.float64) - z).max()) if n else 0.0
    return z, f


# ------------------------------------------------------------------------------------------- a. kernel vs restatement
@pytest.mark.parametrize("seed", [0, 71, 2 ** 32 + 7, 2 ** 63 + 5])
def test_philox_kernel_matches_the_restatement_elementwise(seed):
    eng = _engine()
    guard = -12345.0
    worst, worst_f = 0.0, 0.0
    for stream_id in STREAMS:
        for n in (1, 2, 3, 4, 5, 1023, 3 * 256 * 256 + 1):
            dst = torch.full((n + 1,), guard, device="cuda")
            eng.randn_(dst[:n], seed, stream_id)
            got = dst.cpu().numpy().astype(np.float64)
            assert got[n] == guard, (n, "guard overwritten")
            want, _ = _pair(n, seed, stream_id)
            # the elements compared for this (seed, stream) are those of the largest buffer - the shorter calls are prefixes of
            # it (tests/test_philox_cpu.py) - so that is where the floor is taken, not over a handful of elements
            f = _pair(3 * 256 * 256 + 1, seed, stream_id)[1]
            err = float(np.abs(got[:n] - want).max())
            worst, worst_f = max(worst, err), max(worst_f, f)
            assert err <= 32 * f, (n, hex(stream_id), err, f)
    _report(test="philox_vs_float64", seed=seed, max_abs=worst, floor_f=worst_f, bound=32 * worst_f)


def test_philox_streams_kernel_matches_the_restatement_at_unaligned_offsets():
    eng = _engine()
    counts = [5, 1023, 3 * 256 * 256 + 1, 2]
    seeds = [2 ** 63 + 5, 0, 71, 2 ** 32 + 7]
    stream_id = 1 << 32
    offsets, off = [], 1
    for n in counts:
        offsets.append(off)
        off += n + 1
    assert any(o % 4 for o in offsets)
    guard = -12345.0
    dst = torch.full((off,), guard, device="cuda")
    eng.randn_streams_(dst, offsets, counts, seeds, stream_id)
    got = dst.cpu().numpy().astype(np.float64)
    worst = 0.0
    f_call = max(_pair(n, s, stream_id)[1] for n, s in zip(counts, seeds))      # the floor over the elements of this one call
    for o, n, s in zip(offsets, counts, seeds):
        want, _ = _pair(n, s, stream_id)
        err = float(np.abs(got[o:o + n] - want).max())
        worst = max(worst, err)
        assert err <= 32 * f_call, (n, s, err, f_call)
        assert got[o - 1] == guard and got[o + n] == guard, (n, "guard overwritten")
    _report(test="philox_vs_float64", kernel="streams", max_abs=worst, floor_f=f_call, bound=32 * f_call)


# ------------------------------------------------------------------------------------------- b. step-mixed streams, observed
def test_ring_renoise_is_the_ring_stream_of_that_step():
    # 264 x 272 -> 768^2 canvas, inner box 512^2: after odd step i the ring is noise * sigma_next(i), nothing else
    # (canvas_ring_renoise_kernel), so the draw of (ring stream, step i) can be read off the trajectory
    steps = 4
    h, w = 264, 272
    sampler = build_sampler(DIM)
    cond = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(2))
    (_, _, _, _), pad = O.canvas_box_and_pad(h, w)
    hp, wp = h + pad[2] + pad[3], w + pad[0] + pad[1]
    assert (hp, wp) == (768, 768)
    (il, it, ir, ib), _ = O.grid_bbox(O.sampling_grids(hp, wp)[1], hp, wp)
    ring = torch.ones(1, 3, hp, wp, dtype=torch.bool)
    ring[:, :, it:ib, il:ir] = False
    ring = ring.numpy()
    assert ring.sum() == 3 * (768 * 768 - 512 * 512)
    sampler.noise_source = "device"
    sampler.device_noise_seed = SEED
    try:
        _, imgs = sampler.tiled_sample(batch_size=9, condition_x=cond.cuda(), class_label=torch.tensor([1]).cuda(),
                                       num_sample_steps=steps, with_images=True, precision="fp32")
    finally:
        sampler.noise_source = "host"
    ts = torch.linspace(1.0, 0.0, steps + 1)
    n = 3 * hp * wp
    for i in (1, 3):
        got = imgs[i + 1].numpy().astype(np.float64)
        assert got.shape == (1, 3, hp, wp)
        sigma = float((-O.log_snr_linear(ts[i + 1])).sigmoid().sqrt())
        want, _ = _pair(n, SEED, P.STREAM_RING, i)
        z32 = P.philox_normal(n, SEED, P.STREAM_RING, i, dtype=np.float32).astype(np.float64)
        m = ring.reshape(-1)
        f = float(np.abs(z32 - want)[m].max())
        err = float(np.abs(got.reshape(-1) - want * sigma)[m].max())
        _report(test="ring_renoise_vs_float64", step=i, sigma=sigma, max_abs=err, floor_f=f, bound=32 * f * sigma)
        assert err <= 32 * f * sigma, (i, err, f, sigma)
        # and it is no other step's draw and not the tile stream: those are independent normals, O(sigma) away
        for sid, step in ((P.STREAM_RING, i - 1), (P.STREAM_RING, i + 1), (P.STREAM_TILES, i)):
            other = P.philox_normal(n, SEED, sid, step) * sigma
            assert float(np.abs(got.reshape(-1) - other)[m].max()) > 3 * sigma, (i, hex(sid), step)
        # the inner box is NOT the ring draw: it keeps the sampled image
        assert float(np.abs(got.reshape(-1) - want * sigma)[~m].max()) > 1e-2


# ------------------------------------------------------------------------------------------- c. runs vs the oracle on replayed noise
@functools.lru_cache(maxsize=None)
def _ddpm_weights():
    return synth_state_dict(_schema(DIM), seed=0)


def _cond(h, w, k=0, b=1):
    return torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + k))


def _noise_scales(num_sample_steps, first=0):
    """sqrt(var) of every executed step that draws tile noise (all but the last), from the oracle's schedule"""
    ts = torch.linspace(1.0, 0.0, num_sample_steps + 1)
    return [float(O.step_scalars(ts[i], ts[i + 1])["var"].sqrt()) for i in range(first, num_sample_steps - 1)]


def _replay(draws):
    # copies: the oracle samples in place in the tensor its start draw hands it
    return O.ReplayNoise([d.clone() for d in draws])


def _oracle_tiled(h, w, k, draws, **kw):
    noise = _replay(draws)
    trace = {}
    with torch.inference_mode():
        out = O.tiled_sample(O.strip_model_prefix(_ddpm_weights()), O.UnetCfg(dim=DIM), _cond(h, w, k), torch.tensor([1]),
                             noise=noise, trace=trace, **kw)
    assert noise.i == len(draws), "the oracle must consume the whole plan"
    return out, trace


def _device_run(sampler, fn):
    sampler.noise_source = "device"
    sampler.device_noise_seed = SEED
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    finally:
        sampler.noise_source = "host"


def _check_image(name, got, want, **kw):
    err = (got.cpu() - want).abs().max().item()
    _report(test="device_noise_vs_oracle", case=name, max_abs=err, **kw)
    assert got.shape == want.shape
    assert err <= BAR, err
    assert err <= PRACTICE, err


@functools.lru_cache(maxsize=None)
def _case1_oracle():
    draws = P.device_noise_draws("ddpm_tiled", seed=SEED, num_sample_steps=4, height=136, width=200, batch_size=4)
    return _oracle_tiled(136, 200, 1, draws, batch_size=4, num_sample_steps=4)[0]


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_case1_one_tile_from_noise(precision):
    # 136 x 200 in one 256^2 tile, reflect-padded: start draw (stream 0), tile stream with steps 0, 1, 2 mixed in; the ring draws of
    # steps 1 and 3 are made and change nothing (the inner box is the canvas)
    scales = _noise_scales(4)
    assert len(scales) == 3 and min(scales) >= VISIBLE, scales
    want = _case1_oracle()
    sampler = build_sampler(DIM)
    got = _device_run(sampler, lambda: sampler.tiled_sample(
        batch_size=4, condition_x=_cond(136, 200, 1).cuda(), class_label=torch.tensor([1]).cuda(), num_sample_steps=4,
        precision=precision))
    _check_image("one_tile_from_noise", got, want, precision=precision)


CASE2 = dict(h=264, w=272, k=2, steps=2)


@functools.lru_cache(maxsize=None)
def _case2_oracle(swapped=False):
    c = CASE2
    draws = P.device_noise_draws("ddpm_tiled", seed=SEED, num_sample_steps=c["steps"], height=c["h"], width=c["w"], batch_size=4,
                                 tile_step_of=(lambda i: 1 - i) if swapped else None)
    return (draws,) + _oracle_tiled(c["h"], c["w"], c["k"], draws, batch_size=4, num_sample_steps=c["steps"])


def test_case2_oracle_sees_which_steps_tile_noise_it_is_given():
    # the blindness guard of case 2, on the CPU: the same plan with step 0's tile buffer drawn as step 1's (a step counter that
    # was not yet set, or was off by one) moves the oracle's canvas after step 0 by far more than the bar
    assert min(_noise_scales(CASE2["steps"])) >= VISIBLE
    _, _, trace = _case2_oracle()
    _, _, wrong = _case2_oracle(swapped=True)
    moved = (trace["img"][0] - wrong["img"][0]).abs().max().item()
    assert moved >= VISIBLE, moved


def test_case2_canvas_trajectories_nine_tiles():
    # 768^2 canvas, 9 / 4 tiles, the engine in one launch of 9, the oracle in minibatches 4 + 4 + 1 out of ONE tile-noise draw
    # (tile-local noise index, independence of sub_batch); step 1 is odd: ring re-noise.  img and x_start after every step.
    c = CASE2
    assert min(_noise_scales(c["steps"])) >= VISIBLE
    draws, want, trace = _case2_oracle()
    sampler = build_sampler(DIM)
    got, imgs, x0s = _device_run(sampler, lambda: sampler.tiled_sample(
        batch_size=9, condition_x=_cond(c["h"], c["w"], c["k"]).cuda(), class_label=torch.tensor([1]).cuda(),
        num_sample_steps=c["steps"], with_images=True, with_x0_images=True, precision="fp32"))
    assert len(imgs) == len(x0s) == c["steps"] + 1 and len(trace["img"]) == len(trace["x_start"]) == c["steps"]
    # the same run in launches of 3 + 3 + 3 tiles (a limit of 4, balanced): a launch that does not start at tile 0 must still read
    # its tiles' own noise (tl, not the index inside the launch) - bit for bit the one-launch run
    got4, imgs4, x0s4 = _device_run(sampler, lambda: sampler.tiled_sample(
        batch_size=4, condition_x=_cond(c["h"], c["w"], c["k"]).cuda(), class_label=torch.tensor([1]).cuda(),
        num_sample_steps=c["steps"], with_images=True, with_x0_images=True, precision="fp32"))
    assert torch.equal(got, got4) and all(torch.equal(a, b) for a, b in zip(imgs + x0s, imgs4 + x0s4))
    (left, top, right, bottom), _ = O.canvas_box_and_pad(c["h"], c["w"])
    start_err = (imgs[0] - draws[0][:, :, top:bottom, left:right]).abs().max().item()
    assert start_err <= CANVAS_PRACTICE, start_err
    errs = {}
    for name, mine, theirs in (("img", imgs, trace["img"]), ("x_start", x0s, trace["x_start"])):
        for i in range(c["steps"]):
            assert mine[i + 1].shape == theirs[i].shape == (1, 3, 768, 768)
            errs[f"{name}{i}"] = (mine[i + 1] - theirs[i]).abs().max().item()
    _report(test="device_noise_vs_oracle", case="nine_tiles_trajectories", start=start_err, **errs)
    assert max(errs.values()) <= CANVAS_BAR, errs
    assert max(errs.values()) <= CANVAS_PRACTICE, errs
    _check_image("nine_tiles", got, want)


@pytest.mark.parametrize("kw", [dict(generation_start_steps=2, num_sample_steps=4), dict(start_white_noise=False, num_sample_steps=2)],
                         ids=["skipped_prefix", "no_white_start"])
def test_case3_q_sample_start_with_class_guidance(kw):
    # canvas_q_start_kernel on device noise (stream 0); two passes per tile consume ONE noise tile per tile; after a skipped
    # prefix of two steps the first executed step mixes in the loop index 2, not 0 (device_noise_draws' docstring)
    n, first = kw["num_sample_steps"], kw.get("generation_start_steps", 0)
    scales = _noise_scales(n, first)
    assert len(scales) == 1 and min(scales) >= VISIBLE, scales
    t0 = torch.tensor(1.0 - first / n) if first else torch.tensor(1.0)
    assert float((-O.log_snr_linear(t0)).sigmoid().sqrt()) >= VISIBLE            # the start draw's scale
    draws = P.device_noise_draws("ddpm_tiled", seed=SEED, num_sample_steps=n, generation_start_steps=first, height=136, width=200)
    want, _ = _oracle_tiled(136, 200, 3, draws, batch_size=4, class_cond_scale=2.0, **kw)
    sampler = build_sampler(DIM)
    got = _device_run(sampler, lambda: sampler.tiled_sample(
        batch_size=4, condition_x=_cond(136, 200, 3).cuda(), class_label=torch.tensor([1]).cuda(), class_cond_scale=2.0,
        precision="fp32", **kw))
    _check_image("q_start_class_guidance", got, want, **kw)


def test_case4_edm_tiled():
    # stream 1 start; the eps canvas (stream 2<<32, step mixed in) addressed per canvas pixel by the gather and by both passes of
    # the Heun step.  Schedule constants chosen so that EVERY step churns (gamma > 0): with the defaults only the middle one of
    # three steps does, and a step with gamma = 0 has hat_coef = 0 - its noise is drawn and not used
    steps = 3
    e = O.EdmCfg(sigma_min=0.5, S_tmax=100.0, num_sample_steps=steps)
    sigmas = O.edm_sigmas(e, steps)
    gammas = O.edm_gammas(e, sigmas, steps)
    assert int((gammas[:steps] > 0).sum()) >= 2, gammas
    for i in range(steps):
        s, g = float(sigmas[i]), float(gammas[i])
        hat_coef = ((s + g * s) ** 2 - s ** 2) ** 0.5
        assert hat_coef * e.S_noise >= VISIBLE, (i, hat_coef)
    assert float(sigmas[0]) >= VISIBLE                                           # the start draw's scale
    schema = {"net." + k[len("model."):]: v for k, v in _schema(DIM).items()}
    usd = {k[len("net."):]: v for k, v in synth_state_dict(schema, seed=0).items()}
    draws = P.device_noise_draws("edm_tiled", seed=SEED, num_sample_steps=steps, height=136, width=200)
    noise = _replay(draws)
    with torch.inference_mode():
        want = O.edm_tiled_sample(usd, O.UnetCfg(dim=DIM), e, _cond(136, 200, 4), torch.tensor([1]), batch_size=4,
                                  num_sample_steps=steps, noise=noise)
    assert noise.i == len(draws)
    sampler = build_edm_sampler(DIM)
    keep = (sampler.num_sample_steps, sampler.sigma_min, sampler.S_tmax)
    try:
        sampler.num_sample_steps, sampler.sigma_min, sampler.S_tmax = steps, e.sigma_min, e.S_tmax
        got = _device_run(sampler, lambda: sampler.tiled_sample(
            batch_size=4, condition_x=_cond(136, 200, 4).cuda(), class_label=torch.tensor([1]).cuda(), num_sample_steps=steps,
            precision="fp32"))
    finally:
        sampler.num_sample_steps, sampler.sigma_min, sampler.S_tmax = keep
    _check_image("edm_tiled", got, want)


def test_case5_untiled_sample_batch_of_two():
    # the batch as one canvas [3][b*S][S]: the start draw is made in that layout and read back per image; per-step noise [b,3,S,S]
    steps, b = 3, 2
    scales = _noise_scales(steps)
    assert len(scales) == 2 and min(scales) >= VISIBLE, scales
    cond = _cond(256, 256, 5, b=b)
    draws = P.device_noise_draws("ddpm_sample", seed=SEED, num_sample_steps=steps, batch=b)
    assert not torch.equal(draws[0][0], draws[0][1])                             # per-image noise
    noise = _replay(draws)
    with torch.inference_mode():
        want = O.sample(O.strip_model_prefix(_ddpm_weights()), O.UnetCfg(dim=DIM), cond, torch.tensor([1]),
                        num_sample_steps=steps, noise=noise)
    assert noise.i == len(draws)
    sampler = build_sampler(DIM)
    got = _device_run(sampler, lambda: sampler.sample(batch_size=b, condition_x=cond.cuda(), class_label=torch.tensor([1]).cuda(),
                                                      num_sample_steps=steps, precision="fp32"))
    _check_image("untiled_sample_b2", got, want)
