"""Region resampling on the MI355X (``tiled_sample(region_known=..., regions=...)``, srgd_amd.region) on the dim-16 model of
tests/guidance_cases.py: skipping tiles is exact, the evaluated tiles are the planned ones, the result outside R is the known image
bit for bit, a lock-step group is its solo runs, the run against the region oracle (tests/region_cases.py (b)) on host noise, and
the footprint of a NaN."""
import numpy as np
import pytest
import torch

from srgd_amd import region as RG
from srgd_amd.lockstep import image_plan
from tests import guidance_cases as G
from tests import region_cases as R

pytestmark = pytest.mark.gpu
LABEL = torch.tensor([G.LABEL])


def _sampler(noise="device"):
    from tests.test_engine_gpu import build_sampler
    sampler = build_sampler(G.DIM)
    sampler.noise_source = noise
    return sampler


def _run(model, seed, **kw):
    """One call after seeding both noise sources; the model is the session's shared one and leaves with host noise again (``kw`` may
    hold ``tiled_sample``'s own ``sampler`` keyword)."""
    torch.manual_seed(seed)
    model.device_noise_seed = seed
    try:
        return model.tiled_sample(class_label=LABEL.cuda(), **kw)
    finally:
        model.noise_source = "host"


@pytest.fixture(scope="module")
def big():
    """(condition, known image) [1,3,1024,1024] on the GPU: uniform noise, read-only by convention."""
    g = torch.Generator().manual_seed(11)
    return torch.rand(1, 3, 1024, 1024, generator=g).cuda(), torch.rand(1, 3, 1024, 1024, generator=g).cuda()


def _inside(boxes, h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    for (t, l, bh, bw) in boxes:
        m[t:t + bh, l:l + bw] = True
    return m


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------- 1. skipping is exact
@pytest.mark.parametrize("sampler_name", ["ddpm", "dpmpp2m"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_skipping_tiles_changes_no_bit_of_the_output_or_the_trajectories(big, precision, sampler_name):
    cond, known = big
    kw = dict(batch_size=8, condition_x=cond, num_sample_steps=4, precision=precision, sampler=sampler_name, region_known=known,
              regions=R.EXACT_CASE["boxes"], with_images=True, with_x0_images=True)
    logs = ([], [])
    skip = _run(_sampler(), 3, region_skip_tiles=True, region_log=logs[0], **kw)
    full = _run(_sampler(), 3, region_skip_tiles=False, region_log=logs[1], **kw)
    assert logs[0] == [[4], [1], [4], [1]] and logs[1] == [[25], [16], [25], [16]]
    assert torch.equal(_bits(skip[0]), _bits(full[0]))
    for name, a, b in (("img", skip[1], full[1]), ("x_start", skip[2], full[2])):
        assert len(a) == len(b) == 5
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(_bits(x), _bits(y)), (name, i)
    assert torch.isfinite(skip[0]).all()


# ------------------------------------------------------------------------------------------- 2. tile counts
def test_the_log_holds_the_planned_tile_counts(big):
    cond, known = big
    case = R.COUNT_CASE
    p = image_plan(*case["size"])
    _, want = RG.plan_region_steps([(p.coords0, p.coords1, p.box[1], p.box[0], tuple(case["boxes"]))])
    assert (want[0], want[1]) == case["counts"] == ([4], [4]) and (len(p.coords0), len(p.coords1)) == (25, 16)
    log = []
    _run(_sampler(), 5, batch_size=8, condition_x=cond, num_sample_steps=5, precision="bf16", region_known=known, regions=case["boxes"],
         region_log=log, generation_start_steps=1)
    assert log == [want[i % 2] for i in range(1, 5)] == [[4]] * 4


# ------------------------------------------------------------------------------------------- 3. outside R
@pytest.mark.parametrize("post", [{}, {"color_fix": "wavelet", "back_project": 2}], ids=["plain", "color_fix_back_project"])
def test_outside_the_region_the_result_is_the_known_image_bit_for_bit(post):
    g = torch.Generator().manual_seed(13)
    cond, known = torch.rand(1, 3, 300, 260, generator=g).cuda(), torch.rand(1, 3, 300, 260, generator=g).cuda()
    boxes = [(100, 90, 70, 50), (150, 120, 40, 60), (0, 0, 3, 3), (299, 259, 1, 1)]
    inside = _inside(boxes, 300, 260)
    kw = dict(batch_size=8, condition_x=cond, num_sample_steps=4, precision="bf16", region_known=known, regions=boxes, **post)
    a = _run(_sampler(), 21, **kw).cpu()
    b = _run(_sampler(), 22, **kw).cpu()
    for out in (a, b):
        assert torch.equal(_bits(out[0][:, ~inside]), _bits(known[0].cpu()[:, ~inside]))
        assert torch.isfinite(out).all()
    assert not torch.equal(a[0][:, inside], b[0][:, inside])            # two seeds: two alternatives of the region
    assert not torch.equal(a[0][:, inside], known[0].cpu()[:, inside])
    plain = _run(_sampler(), 21, batch_size=8, condition_x=cond, num_sample_steps=4, precision="bf16", **post).cpu()
    assert not torch.equal(a[0][:, inside], plain[0][:, inside])        # the surroundings steer what is drawn inside


# ------------------------------------------------------------------------------------------- 4. lock-step
@pytest.mark.parametrize("noise", ["device", "host"])
def test_a_mixed_group_is_its_solo_runs(noise):
    g = torch.Generator().manual_seed(17)
    sizes = ((300, 260), (256, 256), (300, 260))
    conds = [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in sizes]
    known = [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in sizes]
    boxes = [[(100, 90, 70, 50)], None, [(5, 5, 20, 30), (200, 100, 64, 64)]]
    kw = dict(batch_size=6, num_sample_steps=4, precision="bf16")
    log = []
    group = _run(_sampler(noise), 31, condition_x=conds, region_known=[known[0], None, known[2]], regions=boxes, region_log=log, **kw)
    assert len(log) == 4 and log[0][1] == 1 and log[1][1] == 1 and log[0][0] < 9
    for k in (0, 2):
        solo = _run(_sampler(noise), 31, condition_x=conds[k], region_known=known[k], regions=boxes[k], **kw)
        assert torch.equal(_bits(group[k]), _bits(solo)), k
    assert torch.equal(_bits(group[1]), _bits(_run(_sampler(noise), 31, condition_x=conds[1], **kw)))
    # a [B,3,H,W] condition with a None neighbour, and per-image seeds
    batch = torch.cat([conds[0], conds[2]], 0)
    both = _run(_sampler(noise), 31, condition_x=batch, region_known=[None, known[2]], regions=boxes[2], **kw)
    assert torch.equal(_bits(both[1:2]), _bits(_run(_sampler(noise), 31, condition_x=conds[2], region_known=known[2], regions=boxes[2], **kw)))
    assert torch.equal(_bits(both[0:1]), _bits(_run(_sampler(noise), 31, condition_x=conds[0], **kw)))
    seeded = _run(_sampler(noise), 1, condition_x=[conds[0], conds[0]], region_known=[known[0], known[0]], regions=boxes[0], seeds=[31, 32], **kw)
    assert torch.equal(_bits(seeded[0]), _bits(group[0])) and not torch.equal(seeded[0], seeded[1])


# ------------------------------------------------------------------------------------------- 5. the oracle
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_the_region_run_matches_the_region_oracle(precision):
    """Bars: the project's host-noise bars - final pixels 1e-3, canvas and predicted-clean-image trajectories 2e-3.
    The case: 300 x 300, 4 steps, class guidance 2.0, two boxes; the three figures are printed per precision."""
    case = R.ORACLE_CASE
    cond, known = R.oracle_input()
    want, trace = R.oracle_run()
    out, xts, x0s = _run(_sampler("host"), case["seed"], batch_size=case["batch_size"], condition_x=cond.cuda(), num_sample_steps=case["steps"],
                         class_cond_scale=case["class_cond_scale"], precision=precision, region_known=known, regions=case["boxes"],
                         with_images=True, with_x0_images=True)
    torch.cuda.synchronize()
    assert len(xts) == len(x0s) == case["steps"] + 1 and out.shape == want.shape
    err = float((out.cpu() - want).abs().max())
    xt_err = [float((a - b).abs().max()) for a, b in zip(xts[1:], trace["img"])]
    x0_err = [float((a - b).abs().max()) for a, b in zip(x0s[1:], trace["x_start"])]
    print(f"region oracle {precision}: final {err:.3e}, canvas {max(xt_err):.3e}, x0 {max(x0_err):.3e}")
    assert err <= 1e-3, err
    assert max(xt_err) <= 2e-3 and max(x0_err) <= 2e-3, (xt_err, x0_err)
    inside = _inside(case["boxes"], *want.shape[-2:])
    assert torch.equal(_bits(out[0].cpu()[:, ~inside]), _bits(known[0][:, ~inside]))


# ------------------------------------------------------------------------------------------- 6. non-finite values
def test_a_nan_of_the_known_image_stays_where_it_is(big):
    cond, known = big
    boxes = R.EXACT_CASE["boxes"]
    inside = _inside(boxes, 1024, 1024)
    bad = known.clone()
    bad[0, 1, 900, 910] = float("nan")                                # outside R, in no tile that touches R
    out, xts = _run(_sampler(), 3, batch_size=8, condition_x=cond, num_sample_steps=4, precision="bf16", region_known=bad, regions=boxes,
                    with_images=True)
    out = out.cpu()
    nans = torch.isnan(out[0])
    assert nans[1, 900, 910] and int(nans.sum()) == 1
    assert torch.isfinite(out[0][:, inside]).all()
    p = image_plan(1024, 1024)
    last = xts[-1][0]                                                  # the canvas after the last step's composite
    canvas_inside = torch.zeros(p.Hp, p.Wp, dtype=torch.bool)
    canvas_inside[p.box[1]:p.box[1] + 1024, p.box[0]:p.box[0] + 1024] = inside
    assert torch.isfinite(last[:, canvas_inside]).all() and torch.isnan(last[1, p.box[1] + 900, p.box[0] + 910])
    clean = _run(_sampler(), 3, batch_size=8, condition_x=cond, num_sample_steps=4, precision="bf16", region_known=known, regions=boxes).cpu()
    assert torch.equal(_bits(out[0][:, inside]), _bits(clean[0][:, inside]))  # and R never saw it


def test_a_nan_inside_the_region_stays_inside(big, monkeypatch):
    cond, known = big
    boxes = R.EXACT_CASE["boxes"]
    inside = _inside(boxes, 1024, 1024)
    p = image_plan(1024, 1024)
    steps = 4
    after_step = RG._RegionRun.after_step

    def planted(self, i, scalars, img, x_start=None):
        after_step(self, i, scalars, img, x_start)
        if i == steps - 2:                                             # into R of the canvas the last step reads
            img.view(-1, 3, p.Hp, p.Wp)[0, 2, p.box[1] + 360, p.box[0] + 370] = float("nan")

    monkeypatch.setattr(RG._RegionRun, "after_step", planted)
    out, xts = _run(_sampler(), 3, batch_size=8, condition_x=cond, num_sample_steps=steps, precision="bf16", region_known=known,
                    regions=boxes, with_images=True)
    out = out.cpu()
    assert torch.isnan(out[0][:, inside]).any()
    assert torch.equal(_bits(out[0][:, ~inside]), _bits(known[0].cpu()[:, ~inside]))
    canvas_inside = torch.zeros(p.Hp, p.Wp, dtype=torch.bool)
    canvas_inside[p.box[1]:p.box[1] + 1024, p.box[0]:p.box[0] + 1024] = inside
    assert torch.isfinite(xts[-1][0][:, ~canvas_inside]).all() and torch.isnan(xts[-1][0][:, canvas_inside]).any()
