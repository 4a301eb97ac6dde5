"""Characterisation of srgd_amd.inference's folder driver and of its four sampling functions, without a GPU: what they call, print and
write, compared for equality with tests/golden/driver_trace.json.

Driver level: ``batch_sr_target_images`` over a small folder (three same-sized images, one of another size, one RGBA image, one file that
is no image) with the four ``sr_target_image*`` functions and every ``*_on_device`` function replaced by fakes whose outputs are a
deterministic function of size, seed and label.  Per case: the ordered calls, the captured stdout, the SHA-256 of every written file and
the parsed JSON documents.  Sampler level: each of the four functions on a fake model whose ``tiled_sample(**kw)`` records its keywords,
with no optional keyword and with every one set.

``python -m tests.test_driver_trace_cpu --record`` writes the golden file; it is recorded from the code a change starts from and never
from the code under test."""
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile
from unittest import mock

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from srgd_amd import inference as INF  # noqa: E402
from srgd_amd import resize as RZ  # noqa: E402
from tests import selfens_cases as SC  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "driver_trace.json")
SIZES = {"a.png": (32, 30), "b.png": (32, 30), "c.png": (30, 36), "d.png": (32, 30), "e.png": (32, 30)}       # (w, h); d is RGBA
LABELS = {"b.png": 1, "e.png": 0}
SAMPLERS = {"solo": "sr_target_image", "same": "sr_target_images", "mixed": "sr_target_images_mixed", "seeded": "sr_target_images_seeded"}


def _sha(data):
    return hashlib.sha256(data).hexdigest()


def _t(x):
    """A tensor or array argument as something JSON holds: shape, dtype and a digest of its bytes."""
    a = x.numpy() if torch.is_tensor(x) else np.asarray(x)
    return [list(a.shape), str(a.dtype), _sha(np.ascontiguousarray(a).tobytes())[:16]]


def _scalar(v):
    return v is None or isinstance(v, (bool, int, float, str))


def _pattern(h, w, seed, label):
    """The fake samplers' output: uint8 [h,w,3], a function of size, seed and label only."""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return ((3 * x + 5 * y + 7 * c + 31 * seed + 17 * (9 if label is None else label) + h * w) % 256).astype(np.uint8)


def _nearest(a, h, w):
    return a[(np.arange(h) * a.shape[0] // h)[:, None], (np.arange(w) * a.shape[1] // w)[None, :]]


# ------------------------------------------------------------------------------------------- driver level
def _fakes(calls):
    """``{(module, name): fake}`` for the four samplers and every device function the driver calls; each appends to ``calls``."""
    def sampler(kind):
        def run(images, *a, **kw):
            ims = images if isinstance(images, list) else [images]
            seeds = list(a[0]) if kind == "seeded" else [kw.get("seed")] * len(ims)
            model = a[1] if kind == "seeded" else a[0]
            labels = kw.get("test_label")
            per_image = list(labels) if isinstance(labels, (list, tuple)) else [labels] * len(ims)
            calls.append({"fn": SAMPLERS[kind], "sizes": [list(im.size) for im in ims], "modes": [im.mode for im in ims],
                          "inputs": [_t(im) for im in ims], "distinct_inputs": len({id(im) for im in ims}),
                          "labels": labels, "seeds": list(a[0]) if kind == "seeded" else None, "model": type(model).__name__,
                          "positional": len(a), "keywords": sorted(kw), "scalars": {k: v for k, v in sorted(kw.items()) if _scalar(v)},
                          "reference": None if "reference" not in kw else [_t(r) for r in (kw["reference"] if kind != "solo" else [kw["reference"]])],
                          "region_known": None if "region_known" not in kw else
                          [_t(r) for r in (kw["region_known"] if kind != "solo" else [kw["region_known"]])],
                          "regions": kw.get("regions")})
            outs = [Image.fromarray(_pattern(4 * im.size[1], 4 * im.size[0], s, lab), "RGB") for im, s, lab in zip(ims, seeds, per_image)]
            ret = outs if isinstance(images, list) else outs[0]
            if "reference" not in kw:
                return ret
            quality = [{"psnr_y": 20.0 + s % 7 + im.size[0], "psnr_rgb": 10.0 + 0.5 * i, "ssim_y": 0.5 + 0.01 * im.size[1]}
                       for i, (im, s) in enumerate(zip(ims, seeds))]
            return ret, quality
        return run

    def dihedral(images, ops):
        calls.append({"fn": "dihedral_on_device", "images": [_t(t) for t in images], "ops": list(ops)})
        return [torch.from_numpy(SC.apply(t.numpy(), op)) for t, op in zip(images, ops)]

    def merge(groups, return_mean01=False):
        calls.append({"fn": "self_ensemble_on_device", "groups": [[[_t(t), op] for t, op in g] for g in groups], "return_mean01": return_mean01})
        merged = [SC.merge([t.numpy() for t, _ in g], [op for _, op in g]) for g in groups]
        if not return_mean01:
            return [torch.from_numpy(m) for m in merged]
        return [(torch.from_numpy(m), torch.from_numpy(SC.mean01(m))[None]) for m in merged]

    def metrics(outs, refs, crop_border=4):
        calls.append({"fn": "metrics_on_device", "outs": [_t(o) for o in outs], "refs": [_t(r) for r in refs], "crop_border": crop_border})
        return [{"psnr_y": float(int(o.sum()) % 97), "psnr_rgb": float(r.shape[0]), "ssim_y": 0.25} for o, r in zip(outs, refs)]

    def consistency(outputs, inputs, return_down=False):
        calls.append({"fn": "consistency_on_device", "outputs": [_t(o) for o in outputs], "inputs": [_t(i) for i in inputs],
                      "distinct_inputs": len({id(i) for i in inputs}), "return_down": return_down})
        return [{"lr_psnr": float(int(o.numpy().astype(np.int64).sum()) % 1000) / 8, "lr_mse": float(i.shape[1]), "lr_max_abs": 2.0}
                for o, i in zip(outputs, inputs)]

    def ensemble(stacks, return_mean01=False):
        calls.append({"fn": "ensemble_on_device", "stacks": [_t(s) for s in stacks], "return_mean01": return_mean01})
        results = []
        for s in stacks:
            a = s.numpy().astype(np.int64)
            mean = ((2 * a.sum(0) + len(a)) // (2 * len(a))).astype(np.uint8)
            std = (a.max(0) - a.min(0)).astype(np.uint8)
            res = (torch.from_numpy(mean), torch.from_numpy(std), {"mean_std": float(std.mean()), "max_std": float(std.max())})
            results.append(res + (torch.from_numpy(SC.mean01(mean))[None],) if return_mean01 else res)
        return results

    def bleed(images, passes):
        calls.append({"fn": "bleed_on_device", "images": [_t(t) for t in images], "passes": passes})
        return [torch.where(t[:, :, 3:] > 0, t[:, :, :3], torch.full_like(t[:, :, :3], passes)) for t in images]

    def attach(outs, planes, scale, filter_name):
        calls.append({"fn": "attach_alpha_on_device", "outs": [_t(o) for o in outs], "planes": [_t(p) for p in planes],
                      "distinct_planes": len({id(p) for p in planes}), "scale": scale, "filter": filter_name})
        return [torch.from_numpy(np.dstack([o.numpy(), _nearest(p.numpy(), o.shape[0], o.shape[1])])) for o, p in zip(outs, planes)]

    def resize(images, sizes, filter_name):
        calls.append({"fn": "resize_on_device", "images": [_t(t) for t in images], "sizes": [list(s) for s in sizes], "filter": filter_name})
        return [torch.from_numpy(np.ascontiguousarray(_nearest(t.numpy(), h, w))) for t, (h, w) in zip(images, sizes)]

    fakes = {(INF, name): sampler(kind) for kind, name in SAMPLERS.items()}
    fakes.update({(INF, "dihedral_on_device"): dihedral, (INF, "self_ensemble_on_device"): merge, (INF, "metrics_on_device"): metrics,
                  (INF, "consistency_on_device"): consistency, (INF, "ensemble_on_device"): ensemble, (INF, "bleed_on_device"): bleed,
                  (INF, "attach_alpha_on_device"): attach, (RZ, "resize_on_device"): resize})
    for name in ("color_fix_on_device", "back_project_on_device", "resize_planes_on_device", "upsample_bicubic_on_device",
                 "unit_tensor_to_pil_on_device", "unit_tensor_to_u8_on_device"):      # never the driver's business
        def forbidden(*a, _name=name, **kw):
            raise AssertionError(f"the driver called {_name}")
        fakes[(INF, name)] = forbidden
    return fakes


def _folders(tmp):
    """The input folder, the ground truth and the known outputs of --region_known_dir."""
    indir, gt, known = (os.path.join(tmp, d) for d in ("in", "gt", "known"))
    for d in (indir, gt, known):
        os.mkdir(d)
    for i, (name, (w, h)) in enumerate(SIZES.items()):
        low = SC.image(h, w, seed=3 + i)
        if name == "d.png":
            plane = ((np.arange(h)[:, None] + np.arange(w)[None, :]) % 3 * 120).astype(np.uint8)             # 0, 120 and 240
            Image.fromarray(np.dstack([low, plane]), "RGBA").save(os.path.join(indir, name))
        else:
            Image.fromarray(low, "RGB").save(os.path.join(indir, name))
        Image.fromarray(SC.image(4 * h, 4 * w, seed=40 + i), "RGB").save(os.path.join(gt, name))
        Image.fromarray(SC.image(4 * h, 4 * w, seed=60 + i), "RGB").save(os.path.join(known, name.replace(".png", "_out.png")))
    Image.fromarray(SC.image(120, 128, seed=80), "RGB").save(os.path.join(known, "b_out_s1.png"))          # b alone has its own second file
    with open(os.path.join(indir, "f_notes.txt"), "w") as f:
        f.write("not an image\n")
    return indir, gt, known


def _case_runs(name, indir, gt, known):
    """The ``batch_sr_target_images`` keyword sets of a case, one per run into the case's one output folder, and what to delete between
    two runs."""
    cases = {
        "defaults": [{}],
        "lockstep2": [dict(lockstep=2)],
        "lockstep_tiles16_labels": [dict(lockstep_tiles=16, labels=LABELS)],
        "lockstep_tiles2_labels": [dict(lockstep_tiles=2, labels=LABELS)],
        "samples3_resumed": [dict(samples=3), dict(samples=3)],
        "ensemble_reference_consistency": [dict(samples=2, ensemble=True, reference_dir=gt, crop_border=2, consistency=True, color_fix="wavelet",
                                                back_project=2)],
        "self_ensemble_alpha_outscale": [dict(self_ensemble=4, samples=2, lockstep=3, alpha="keep", alpha_bleed=2, outscale=2.0, reference_dir=gt,
                                              crop_border=2, consistency=True)],
        "region_samples2": [dict(region_known_dir=known, regions=[(1, 2, 3, 4), (0, 0, 16, 16)], samples=2)],
        "unlabelled_next_to_labelled": [dict(test_label=None, labels=LABELS, lockstep=3)],
        "unlabelled_lockstep_tiles16": [dict(test_label=None, labels=LABELS, lockstep_tiles=16)],
        "every_sampler_keyword": [dict(lockstep=2, test_label=3, scale=4, batch_size=5, cond_scale=1.5, guidance_start_steps=2, class_cond_scale=1.0,
                                       class_guidance_start_steps=1, generation_start_steps=3, num_sample_steps=9, enable_amp=True,
                                       interpolation="lanczos", seed=5, start_index=3, end_index=6, color_fix="adain", back_project=1,
                                       consistency_guidance=0.5, consistency_guidance_start_steps=2, sampler="ddim", eta=0.25,
                                       step_spacing="logsnr", dynamic_threshold=0.9, joint_guidance=True, outscale=3.0,
                                       outscale_filter="lanczos", alpha="keep")],
    }
    return cases[name], {"samples3_resumed": "b_out_s1.png"}.get(name)


CASES = ["defaults", "lockstep2", "lockstep_tiles16_labels", "lockstep_tiles2_labels", "samples3_resumed", "ensemble_reference_consistency",
         "self_ensemble_alpha_outscale", "region_samples2", "unlabelled_next_to_labelled", "unlabelled_lockstep_tiles16", "every_sampler_keyword"]


def driver_trace(name):
    """One case: every run's calls and stdout, then the written files and the JSON documents."""
    with tempfile.TemporaryDirectory() as tmp:
        indir, gt, known = _folders(tmp)
        out = os.path.join(tmp, "out")
        runs, delete = _case_runs(name, indir, gt, known)
        trace = {"runs": []}
        for no, kw in enumerate(runs):
            if no and delete:
                os.remove(os.path.join(out, delete))
            calls, text = [], io.StringIO()
            with contextlib.ExitStack() as stack:
                for (mod, attr), fake in _fakes(calls).items():
                    stack.enter_context(mock.patch.object(mod, attr, fake))
                stack.enter_context(contextlib.redirect_stdout(text))
                INF.batch_sr_target_images(indir, out, object(), **kw)
            trace["runs"].append({"calls": calls, "stdout": text.getvalue().replace(tmp, "<tmp>")})
        trace["files"] = {f: _sha(open(os.path.join(out, f), "rb").read()) for f in sorted(os.listdir(out))}
        trace["modes"] = {}
        for f in sorted(os.listdir(out)):
            if f.endswith(".png"):
                with Image.open(os.path.join(out, f)) as im:
                    trace["modes"][f] = [im.mode, list(im.size)]
        trace["documents"] = {f: json.load(open(os.path.join(out, f))) for f in sorted(os.listdir(out)) if f.endswith(".json")}
    return json.loads(json.dumps(trace))


# ------------------------------------------------------------------------------------------- sampler level
class FakeModel:
    """``tiled_sample(**kw)`` records its keywords and returns zeros of the condition's shape(s)."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def tiled_sample(self, **kw):
        cond = kw["condition_x"]
        shapes = [list(c.shape) for c in cond] if isinstance(cond, list) else list(cond.shape)
        label = kw["class_label"]
        self.calls.append({"keywords": sorted(kw), "batch_size": kw["batch_size"], "condition_x": shapes,
                           "distinct_conditions": len({id(c) for c in cond}) if isinstance(cond, list) else None,
                           "class_label": None if label is None else [str(label.dtype), label.tolist()], "seeds": kw.get("seeds"),
                           "device_noise_seed": self.device_noise_seed, "torch_seed": torch.initial_seed(),
                           "scalars": {k: v for k, v in sorted(kw.items()) if _scalar(v)},
                           "reference": None if "reference" not in kw else [_t(r) for r in kw["reference"]] if isinstance(kw["reference"], list)
                           else _t(kw["reference"]),
                           "region_known": None if "region_known" not in kw else [_t(r) for r in kw["region_known"]]
                           if isinstance(kw["region_known"], list) else _t(kw["region_known"]),
                           "regions": kw.get("regions"), "inference_mode": torch.is_inference_mode_enabled()})
        out = [torch.full_like(c, 0.5) for c in cond] if isinstance(cond, list) else torch.full_like(cond, 0.25)
        if "reference" not in kw:
            return out
        return out, [{"psnr_y": 1.0 + i, "psnr_rgb": 2.0, "ssim_y": 0.5} for i in range(len(cond))]


EVERY = dict(scale=4, batch_size=3, cond_scale=1.5, guidance_start_steps=2, class_cond_scale=2.5, class_guidance_start_steps=1,
             generation_start_steps=3, num_sample_steps=9, enable_amp=True, interpolation="lanczos", seed=5, color_fix="wavelet", crop_border=2,
             back_project=2, consistency_guidance=0.5, consistency_guidance_start_steps=2, sampler="ddim", eta=0.25, step_spacing="logsnr",
             dynamic_threshold=0.9, joint_guidance=True, regions=[(1, 2, 3, 4)])
# explicit values that are the defaults, or that stand for "off": none of them may reach tiled_sample
OFF = dict(color_fix="none", reference=None, crop_border=7, back_project=0, consistency_guidance=0.0, consistency_guidance_start_steps=4,
           sampler="ddpm", eta=None, step_spacing="time", dynamic_threshold=0.0, joint_guidance=False, region_known=None, regions=[(1, 2, 3, 4)])


def _result(ret):
    describe = lambda r: [r.mode, list(r.size)] if isinstance(r, Image.Image) else [describe(v) for v in r] if isinstance(r, (list, tuple)) else r  # noqa: E731
    return [type(ret).__name__, describe(ret)]


def sampler_trace():
    images = [Image.fromarray(SC.image(h, w, seed=i), "RGB") for i, (w, h) in enumerate([(6, 5), (6, 5), (6, 5)])]
    other = Image.fromarray(SC.image(7, 4, seed=9), "RGB")
    uploads = []

    def upsample(image, scale, device):
        uploads.append([list(image.size), scale, str(device)])
        return torch.zeros(1, 3, image.size[1] * scale, image.size[0] * scale)

    def extras(ims, solo=False):
        refs = [torch.full((4 * im.size[1], 4 * im.size[0], 3), 7, dtype=torch.uint8) for im in ims]
        known = [torch.full((1, 3, 4 * im.size[1], 4 * im.size[0]), 0.5) for im in ims]
        return dict(EVERY, reference=refs[0] if solo else refs, region_known=known[0] if solo else known)
    trace = {}
    with mock.patch.object(INF, "upsample_bicubic_on_device", upsample), \
            mock.patch.object(INF, "unit_tensor_to_pil_on_device", INF.unit_tensor_to_pil):
        def run(tag, fn, *a, **kw):
            model = FakeModel()
            del uploads[:]
            ret = getattr(INF, fn)(*a, model, **kw)
            trace[tag] = {"tiled_sample": model.calls, "uploads": list(uploads), "result": _result(ret)}
        mixed = [images[0], other, images[1]]
        twice = [images[0], images[0], other, images[0]]                           # seeded: an image several times, upsampled once
        for tag, kw_of in (("none", lambda ims, solo=False: {}), ("off", lambda ims, solo=False: dict(OFF)), ("every", extras)):
            run(f"solo/{tag}", "sr_target_image", images[0], **kw_of([images[0]], True))
            run(f"same/{tag}", "sr_target_images", images, **kw_of(images))
            run(f"mixed/{tag}", "sr_target_images_mixed", mixed, **kw_of(mixed))
            run(f"seeded/{tag}", "sr_target_images_seeded", twice, [71, 72, 71, 73], **kw_of(twice))
        for tag, label in (("label_none", None), ("label_list_uniform", [4, 4, 4]), ("label_list_mixed", [0, 3, 1]), ("label_tuple", (2, 2, 1))):
            if not isinstance(label, (list, tuple)):
                run(f"solo/{tag}", "sr_target_image", other, test_label=label)
            run(f"same/{tag}", "sr_target_images", images, test_label=label)
            run(f"mixed/{tag}", "sr_target_images_mixed", mixed, test_label=label)
            run(f"seeded/{tag}", "sr_target_images_seeded", mixed, [1, 2, 3], test_label=label)
    return json.loads(json.dumps(trace))


# ------------------------------------------------------------------------------------------- the comparison
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_these_cases(golden):
    assert sorted(golden) == ["driver", "sampler"] and list(golden["driver"]) == CASES
    assert len(golden["sampler"]) == 3 * 4 + 3 * 4 + 1


@pytest.mark.parametrize("name", CASES)
def test_the_driver_calls_prints_and_writes_what_it_did(name, golden):
    got, want = driver_trace(name), golden["driver"][name]
    assert len(got["runs"]) == len(want["runs"])
    for run, run0 in zip(got["runs"], want["runs"]):
        assert [c["fn"] for c in run["calls"]] == [c["fn"] for c in run0["calls"]]
        for call, call0 in zip(run["calls"], run0["calls"]):
            assert call == call0
        assert run["stdout"] == run0["stdout"]
    assert got["files"] == want["files"] and got["modes"] == want["modes"] and got["documents"] == want["documents"]
    assert got == want


def test_the_four_sampling_functions_pass_tiled_sample_what_they_did(golden):
    got = sampler_trace()
    assert sorted(got) == sorted(golden["sampler"])
    for tag in got:
        assert got[tag] == golden["sampler"][tag], tag
    plain = {"amp", "batch_size", "class_cond_scale", "class_guidance_start_steps", "class_label", "cond_scale", "condition_x",
             "generation_start_steps", "guidance_start_steps", "num_sample_steps"}
    for kind in ("solo", "same", "mixed", "seeded"):                           # a keyword at its default is not passed at all
        for tag in ("none", "off"):
            assert set(got[f"{kind}/{tag}"]["tiled_sample"][0]["keywords"]) == plain | ({"seeds"} if kind == "seeded" else set()), (kind, tag)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python -m tests.test_driver_trace_cpu --record"
    with open(GOLDEN, "w") as f:
        json.dump({"driver": {name: driver_trace(name) for name in CASES}, "sampler": sampler_trace()}, f, indent=1)
        f.write("\n")
    print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes")
