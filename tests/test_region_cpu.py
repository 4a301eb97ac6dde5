"""Region resampling without a GPU: the active-tile planning against a brute-force restatement (tests/region_cases.py (a)), the
coverage of R by the active tiles of either parity, the tile-count case of the GPU test, the refusals of ``tiled_sample`` before
the model is touched, and the command line."""
import inspect
import os

import pytest
import torch
from PIL import Image

from srgd_amd import inference as INF
from srgd_amd import model as MODEL
from srgd_amd import region as RG
from srgd_amd.lockstep import image_plan
from tests import region_cases as R


# ------------------------------------------------------------------------------------------------ planning
@pytest.mark.parametrize("h,w", R.GEOMETRIES)
def test_the_active_tiles_are_those_of_the_brute_force_restatement(h, w):
    p = image_plan(h, w)
    top, left = p.box[1], p.box[0]
    for boxes in R.boxes_of(h, w):
        for coords in (p.coords0, p.coords1):
            got = RG.active_tiles(coords, top, left, boxes)
            assert got == R.brute_active(coords, p.Hp, p.Wp, top, left, boxes), (boxes, coords)
            assert got == sorted(set(got)) and len(got) >= 1
            assert RG.tile_runs(got) == R.brute_runs(got)
    whole = [(0, 0, h, w)]
    # the whole image touches every tile of both grids: the image's box reaches into every tile of its canvas
    assert RG.active_tiles(p.coords0, top, left, whole) == list(range(len(p.coords0)))
    assert RG.active_tiles(p.coords1, top, left, whole) == list(range(len(p.coords1)))


@pytest.mark.parametrize("h,w", R.GEOMETRIES)
def test_every_pixel_of_the_region_lies_in_an_active_tile_of_either_parity(h, w):
    import numpy as np
    p = image_plan(h, w)
    top, left = p.box[1], p.box[0]
    for boxes in R.boxes_of(h, w):
        for coords in (p.coords0, p.coords1):
            covered = np.zeros((p.Hp, p.Wp), dtype=bool)
            for j in RG.active_tiles(coords, top, left, boxes):
                hs, he, ws, we = coords[j]
                covered[hs:he, ws:we] = True
            for (t, l, bh, bw) in boxes:
                assert covered[top + t:top + t + bh, left + l:left + l + bw].all(), (boxes, coords)


def test_runs_and_counts_of_a_group():
    assert RG.tile_runs([]) == [] and RG.tile_runs([3]) == [(3, 1)] and RG.tile_runs([0, 1, 2, 5, 7, 8]) == [(0, 3), (5, 1), (7, 2)]
    a, b = image_plan(1024, 1024), image_plan(300, 300)
    box = R.COUNT_CASE["boxes"]
    images = [(a.coords0, a.coords1, a.box[1], a.box[0], tuple(box)), (b.coords0, b.coords1, b.box[1], b.box[0], None),
              (a.coords0, a.coords1, a.box[1], a.box[0], tuple(box))]
    runs, counts = RG.plan_region_steps(images)
    assert counts == [[4, 9, 4], [4, 4, 4]]
    # even grid (5 x 5): tiles 6, 7, 11, 12 of image 0; all 9 of image 1 at 25 .. 33; 34 + (6, 7, 11, 12) of image 2
    assert runs[0] == [(6, 2), (11, 2), (25, 9), (40, 2), (45, 2)]
    # odd grid (4 x 4): tiles 5, 6, 9, 10; all 4 of image 1 at 16 .. 19; 20 + (5, 6, 9, 10)
    assert runs[1] == [(5, 2), (9, 2), (16, 4), (25, 2), (29, 2)]
    full_runs, full_counts = RG.plan_region_steps(images, skip_tiles=False)
    assert full_runs == [[(0, 59)], [(0, 36)]] and full_counts == [[25, 9, 25], [16, 4, 16]]


def test_the_tile_count_case_of_the_gpu_test():
    case = R.COUNT_CASE
    p = image_plan(*case["size"])
    assert (len(p.coords0), len(p.coords1)) == case["grids"]
    runs, counts = RG.plan_region_steps([(p.coords0, p.coords1, p.box[1], p.box[0], tuple(case["boxes"]))])
    assert (counts[0], counts[1]) == case["counts"]
    assert len(R.brute_active(p.coords0, p.Hp, p.Wp, p.box[1], p.box[0], case["boxes"])) == 4
    assert len(R.brute_active(p.coords1, p.Hp, p.Wp, p.box[1], p.box[0], case["boxes"])) == 4
    # the exactness case sits across the even seam only: 4 of 25 and 1 of 16
    _, counts = RG.plan_region_steps([(p.coords0, p.coords1, p.box[1], p.box[0], tuple(R.EXACT_CASE["boxes"]))])
    assert counts == [[4], [1]]


def test_the_stream_of_the_known_images_noise():
    from oracle import philox as PH
    taken = {PH.STREAM_START >> 32, PH.STREAM_EDM_START >> 32, PH.STREAM_TILES >> 32, PH.STREAM_RING >> 32, PH.STREAM_EDM_EPS >> 32}
    assert taken == {0, 1, 2} and RG.STREAM_HIGH == 3
    assert RG.region_stream_id(0) == 3 << 32 and RG.region_stream_id(7) == (3 << 32) | 7
    # the high counter word of a stream that mixes a step in keeps the stream's high word in its low byte: 3 is never met
    assert all(PH.counter_words(s, step)[1] & 0xFF in (0, 1, 2) for s in (PH.STREAM_TILES, PH.STREAM_RING, PH.STREAM_EDM_EPS)
               for step in (0, 1, 3, 255, 256, 2 ** 24 - 1))
    assert PH.counter_words(RG.region_stream_id(5), None) == (5, 3)


# ------------------------------------------------------------------------------------------------ refusals
class _Unused:
    """A sampler whose every attribute access fails the test: the refusals come before the model is touched."""
    canvas_group = None

    def __getattr__(self, name):
        raise AssertionError(f"the sampler was touched ({name}) before the arguments were checked")


class _Sharded(_Unused):
    canvas_group = object()


def test_refusals():
    fn = inspect.unwrap(MODEL.ConditionalContinuousTimeGaussianDiffusionSR.tiled_sample)
    cond = torch.zeros(1, 3, 256, 300)
    known = torch.zeros(1, 3, 256, 300)
    box = [(0, 0, 8, 8)]
    solo = dict(condition_x=cond, num_sample_steps=4)
    group = dict(condition_x=[cond, cond], num_sample_steps=4)
    for form, kn in ((solo, known), (group, [known, None]), (dict(group, seeds=[1, 2]), [known, known]),
                     (dict(condition_x=torch.zeros(2, 3, 256, 300), num_sample_steps=4), [None, known])):
        for bad in ([(0, 0, 257, 8)], [(0, 293, 8, 8)], [(-1, 0, 8, 8)], [(0, 0, 0, 8)], [(0, 0, 8)], [], box * 17, [(0.5, 0, 8, 8)]):
            with pytest.raises(ValueError, match="regions"):
                fn(_Unused(), region_known=kn, regions=bad, **form)
        with pytest.raises(ValueError, match="regions without region_known"):
            fn(_Unused(), regions=box, **form)
        with pytest.raises(ValueError, match="region_known without regions"):
            fn(_Unused(), region_known=kn, **form)
        with pytest.raises(NotImplementedError, match="canvas_group"):
            fn(_Sharded(), region_known=kn, regions=box, **form)
        with pytest.raises(ValueError, match="region_log"):
            fn(_Unused(), region_known=kn, regions=box, region_log=(), **form)
    for wrong in (torch.zeros(1, 3, 256, 256), torch.zeros(1, 3, 256, 300, dtype=torch.float64), torch.zeros(3, 256, 300),
                  torch.zeros(2, 3, 256, 300), "known.png"):
        with pytest.raises(ValueError, match="region_known"):
            fn(_Unused(), region_known=wrong, regions=box, **solo)
    with pytest.raises(ValueError, match="region_known"):
        fn(_Unused(), region_known=[known], regions=box, **group)              # one entry for two images
    with pytest.raises(ValueError, match="region_known"):
        fn(_Unused(), region_known=[None, None], regions=box, **group)         # nothing to resample
    with pytest.raises(ValueError, match="regions"):
        fn(_Unused(), region_known=[known, None], regions=[box, box], **group)  # boxes for the image sampled whole
    # trajectories of a group: refused as they are without the keywords

    class _Steps(_Unused):
        num_sample_steps = 4
    for form in (group, dict(group, seeds=[1, 2])):
        with pytest.raises(NotImplementedError, match="with_images"):
            fn(_Steps(), region_known=[known, known], regions=box, with_images=True, **form)
    edm = inspect.unwrap(MODEL.ConditionalElucidatedDiffusionSR.tiled_sample)
    with pytest.raises(NotImplementedError, match="DDPM sampler only"):
        edm(_Unused(), condition_x=cond, region_known=known, regions=box)
    with pytest.raises(NotImplementedError, match="DDPM sampler only"):
        edm(_Unused(), condition_x=cond, regions=box)


def test_the_checked_arguments():
    known = torch.zeros(1, 3, 64, 80)
    assert RG.check_region_args(None, None, [(64, 80)]) is None
    got = RG.check_region_args(known, [(0, 0, 64, 80), [1, 2, 3, 4]], [(64, 80)])
    assert got[0][0].data_ptr() == known.data_ptr() and got[0][1] == ((0, 0, 64, 80), (1, 2, 3, 4))
    got = RG.check_region_args([known, None, known], [[(0, 0, 1, 1)], None, [(5, 5, 2, 2), (6, 6, 2, 2)]], [(64, 80)] * 3)
    assert got[1] is None and got[0][1] == ((0, 0, 1, 1),) and got[2][1] == ((5, 5, 2, 2), (6, 6, 2, 2))
    got = RG.check_region_args([None, known], [(3, 4, 5, 6)], [(64, 80)] * 2)    # one box list for every image with a known image
    assert got[0] is None and got[1][1] == ((3, 4, 5, 6),)
    batch = torch.zeros(2, 3, 64, 80)
    got = RG.check_region_args(batch, [(3, 4, 5, 6)], [(64, 80)] * 2)
    assert [g[1] for g in got] == [((3, 4, 5, 6),)] * 2 and got[1][0].shape == (1, 3, 64, 80)
    assert RG.check_boxes([(0, 0, 64, 80)] * 16, 64, 80) == ((0, 0, 64, 80),) * 16


# ------------------------------------------------------------------------------------------------ the command line
def _argv(*extra):
    return ["-c", "x", "-m", "w", "--input_dir", "i", "--output_dir", "o", *extra]


def test_the_flags_parse_and_are_handed_on_only_when_set():
    a = INF.parse_args(_argv())
    assert a.region_known_dir is None and a.region is None
    a = INF.parse_args(_argv("--region_known_dir", "k", "--region", "1,2,3,4", "--region", "0,0,256,256"))
    assert a.region_known_dir == "k" and a.region == [(1, 2, 3, 4), (0, 0, 256, 256)]
    for bad in (("--region", "1,2,3,4"), ("--region_known_dir", "k"),
                ("--region_known_dir", "k", "--region", "1,2,3"), ("--region_known_dir", "k", "--region", "1,2,3,x"),
                ("--region_known_dir", "k", "--region", "1,2,0,4"), ("--region_known_dir", "k", "--region=-1,2,3,4"),
                ("--region_known_dir", "k", *(["--region", "1,2,3,4"] * 17)),
                ("--region_known_dir", "k", "--region", "1,2,3,4", "--self_ensemble", "2"),
                ("--region_known_dir", "k", "--region", "1,2,3,4", "--ensemble", "--samples", "2")):
        with pytest.raises(SystemExit) as err:
            INF.parse_args(_argv(*bad))
        assert "--region" in str(err.value), bad
    assert INF.parse_region("4,3,2,1") == (4, 3, 2, 1)
    assert INF._region_kw(None, None) == {} and INF._region_kw("k", [(1, 2, 3, 4)]) == {"region_known": "k", "regions": [(1, 2, 3, 4)]}
    ddpm, edm = MODEL.ConditionalContinuousTimeGaussianDiffusionSR, MODEL.ConditionalElucidatedDiffusionSR
    for fn in (INF.sr_target_image, INF.sr_target_images, INF.sr_target_images_mixed, INF.sr_target_images_seeded,
               ddpm.tiled_sample, edm.tiled_sample):
        params = inspect.signature(fn).parameters
        assert params["region_known"].default is None and params["regions"].default is None, fn.__qualname__
    params = inspect.signature(INF.batch_sr_target_images).parameters
    assert params["region_known_dir"].default is None and params["regions"].default is None
    assert inspect.signature(ddpm.tiled_sample).parameters["region_skip_tiles"].default is True
    src = inspect.getsource(INF.main)
    assert "check_region_known(" in src and '"region_known_dir": args.region_known_dir' in src


def test_the_known_files_are_checked_before_anything_is_sampled(tmp_path):
    inputs, known = tmp_path / "in", tmp_path / "known"
    inputs.mkdir()
    known.mkdir()
    for name, size in (("a.png", (20, 10)), ("b.png", (16, 16)), ("c.png", (8, 8)), ("d.png", (8, 8))):
        Image.new("RGB", size).save(inputs / name)
    (inputs / "notes.png").write_text("not an image")
    Image.new("RGB", (80, 40)).save(known / "a_out.png")
    Image.new("RGB", (64, 60)).save(known / "b_out.png")               # not x4
    (known / "d_out.png").write_text("not an image")
    files = sorted(str(p) for p in inputs.iterdir())
    box = [(0, 0, 32, 32)]
    got = INF.region_known_problems(files, str(known), box)
    assert len(got) == 3 and "b.png: known output b_out.png is 64x60" in got[0] and "c.png" in got[1] and "missing" in got[1] \
        and "d.png" in got[2] and "cannot be read" in got[2]
    with pytest.raises(SystemExit) as err:
        INF.check_region_known(files, str(known), box)
    assert "--region_known_dir: 3 problem(s)" in str(err.value)
    assert INF.region_known_problems(files[:1], str(known), box) == []
    INF.check_region_known(files[:1], str(known), box)
    got = INF.region_known_problems(files[:1], str(known), [(0, 0, 41, 8), (0, 73, 8, 8), (39, 79, 1, 1)])
    assert len(got) == 2 and all("does not lie inside the 80x40 output" in g for g in got)
    # --samples K: sample k starts from its own file where there is one, else from the one <name>_out.png
    assert INF.region_known_path(str(known), files[0], 0, 3) == os.path.join(str(known), "a_out.png")
    assert INF.region_known_path(str(known), files[0], 2, 3) == os.path.join(str(known), "a_out.png")
    Image.new("RGB", (80, 40)).save(known / "a_out_s2.png")
    assert INF.region_known_path(str(known), files[0], 2, 3) == os.path.join(str(known), "a_out_s2.png")
    assert INF.region_known_path(str(known), files[0], 1, 3) == os.path.join(str(known), "a_out.png")
    assert INF.region_known_problems(files[:1], str(known), box, samples=3) == []
    Image.new("RGB", (80, 44)).save(known / "a_out_s1.png")
    assert len(INF.region_known_problems(files[:1], str(known), box, samples=3)) == 1
    # the bytes of a known file survive the round trip through the fp32 image and the writer's mul(255).byte()
    import numpy as np
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    Image.fromarray(ramp, "RGB").save(known / "ramp.png")
    t = INF.load_region_known(str(known / "ramp.png"))
    assert t.shape == (1, 3, 16, 16) and t.dtype == torch.float32
    assert np.array_equal(np.asarray(INF.unit_tensor_to_pil(t[0])), ramp)


def test_the_batch_driver_hands_every_entry_its_known_file(tmp_path, monkeypatch):
    import numpy as np
    inputs, known, out = tmp_path / "in", tmp_path / "known", tmp_path / "out"
    inputs.mkdir()
    known.mkdir()
    for name, value in (("a.png", 10), ("b.png", 20)):
        Image.new("RGB", (8, 6), (value, value, value)).save(inputs / name)
    Image.new("RGB", (32, 24), (1, 2, 3)).save(known / "a_out.png")
    Image.new("RGB", (32, 24), (4, 5, 6)).save(known / "a_out_s1.png")
    Image.new("RGB", (32, 24), (7, 8, 9)).save(known / "b_out.png")          # b: both samples start from the one file
    calls = []

    def solo(image, sr_model, **kw):
        calls.append(("solo", kw))
        return Image.new("RGB", (image.size[0] * 4, image.size[1] * 4))

    def seeded(images, seeds, sr_model, **kw):
        calls.append(("seeded", dict(kw, seeds=list(seeds))))
        return [Image.new("RGB", (im.size[0] * 4, im.size[1] * 4)) for im in images]

    monkeypatch.setattr(INF, "sr_target_image", solo)
    monkeypatch.setattr(INF, "sr_target_images_seeded", seeded)
    boxes = [(1, 2, 3, 4), (0, 0, 24, 32)]
    INF.batch_sr_target_images(str(inputs), str(out), object(), samples=2, seed=5, region_known_dir=str(known), regions=boxes)
    assert [c[0] for c in calls] == ["seeded", "seeded"] and all(c[1]["regions"] == boxes and c[1]["seeds"] == [5, 6] for c in calls)
    first = lambda t: tuple(int(v) for v in (t[0, :, 0, 0] * 255 + 0.5))     # noqa: E731
    got = [[first(t) for t in c[1]["region_known"]] for c in calls]
    assert got == [[(1, 2, 3), (4, 5, 6)], [(7, 8, 9), (7, 8, 9)]]
    assert all(t.shape == (1, 3, 24, 32) and t.dtype == torch.float32 for c in calls for t in c[1]["region_known"])
    assert sorted(os.listdir(out)) == ["a_out.png", "a_out_s1.png", "b_out.png", "b_out_s1.png"]
    # one sample per file, no lock-step: the solo form takes the tensor itself; without the flags the keywords are not passed
    calls.clear()
    INF.batch_sr_target_images(str(inputs), str(tmp_path / "out2"), object(), region_known_dir=str(known), regions=boxes[:1])
    assert [c[0] for c in calls] == ["solo", "solo"] and all(torch.is_tensor(c[1]["region_known"]) and c[1]["regions"] == boxes[:1]
                                                             for c in calls)
    assert np.allclose(calls[1][1]["region_known"][0, :, 0, 0].numpy() * 255, (7, 8, 9))
    calls.clear()
    INF.batch_sr_target_images(str(inputs), str(tmp_path / "out3"), object())
    assert len(calls) == 2 and all("region_known" not in c[1] and "regions" not in c[1] for c in calls)
    # a missing known file ends the run before anything is sampled
    os.remove(known / "b_out.png")
    calls.clear()
    with pytest.raises(SystemExit, match="b.png: known output"):
        INF.batch_sr_target_images(str(inputs), str(tmp_path / "out4"), object(), region_known_dir=str(known), regions=boxes)
    assert not calls


def test_the_batch_driver_refuses_before_it_samples(tmp_path):
    (tmp_path / "in").mkdir()
    kw = dict(input_dir=str(tmp_path / "in"), output_dir=str(tmp_path / "out"), sr_model=None)
    with pytest.raises(ValueError, match="go together"):
        INF.batch_sr_target_images(**kw, regions=[(0, 0, 1, 1)])
    with pytest.raises(ValueError, match="go together"):
        INF.batch_sr_target_images(**kw, region_known_dir=str(tmp_path))
    with pytest.raises(ValueError, match="not together"):
        INF.batch_sr_target_images(**kw, region_known_dir=str(tmp_path), regions=[(0, 0, 1, 1)], ensemble=True, samples=2)
    with pytest.raises(ValueError, match="boxes"):
        INF.batch_sr_target_images(**kw, region_known_dir=str(tmp_path), regions=[(0, 0, 1, 1)] * 17)
