"""Per-image class labels, host side: the label-normalising helper of forward / tiled_sample, the CLI's --label_file, the two
new C-ABI entries (no GPU)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")


def test_one_label_broadcasts_and_one_per_image_is_kept():
    from srgd_amd.model import _image_class_ids, _run_labels
    assert _image_class_ids(None, 3) is None
    assert _image_class_ids(torch.tensor([2]), 3) == [2, 2, 2]
    assert _image_class_ids(torch.tensor([2]), 1) == [2]
    assert _image_class_ids(torch.tensor([0, 2, 1]), 3) == [0, 2, 1]
    assert _image_class_ids(torch.tensor([[0], [2]]), 2) == [0, 2]          # any shape, B entries
    for count in (2, 4):
        with pytest.raises(ValueError, match="3 images"):
            _image_class_ids(torch.arange(count), 3)
    with pytest.raises(ValueError):
        _image_class_ids(torch.tensor([0, 1]), 1)
    # what the begin entry and srgd_sampler_image_labels receive
    assert _run_labels(None) == (-1, None)
    assert _run_labels([2, 2, 2]) == (2, None)                               # equal labels: the one-label run, unchanged
    assert _run_labels([0, 2, 1]) == (0, [0, 2, 1])


def test_single_class_id_still_refuses_differing_labels():
    from srgd_amd.model import _single_class_id
    assert _single_class_id(None) == -1 and _single_class_id(torch.tensor([1, 1])) == 1
    with pytest.raises(NotImplementedError, match="per-image class labels"):
        _single_class_id(torch.tensor([0, 2]))


def _folder(tmp_path, names=("a.png", "b.png", "c d.png")):
    src = tmp_path / "in"
    src.mkdir()
    for n in names:
        (src / n).write_bytes(b"x")
    return src


def _argv(src, label_file=None, extra=()):
    base = ["-c", CONF, "-m", "w", "--input_dir", str(src), "--output_dir", "o"]
    return base + (["--label_file", str(label_file)] if label_file is not None else []) + list(extra)


def test_label_file_is_parsed_against_the_folder_and_the_config(tmp_path):
    from srgd_amd.inference import parse_args
    src = _folder(tmp_path)
    a = parse_args(_argv(src))
    assert a.label_file is None and a.labels is None and a.test_label is None
    lf = tmp_path / "labels.txt"
    lf.write_text("# degradation class per file\na.png 0\n\nc d.png   2   # a name with a blank\n")
    a = parse_args(_argv(src, lf, ["--test_label", "1", "--lockstep_tiles", "64"]))
    assert a.labels == {"a.png": 0, "c d.png": 2} and a.test_label == 1 and a.lockstep_tiles == 64
    assert parse_args(_argv(src, lf, ["--lockstep", "3"])).labels == {"a.png": 0, "c d.png": 2}
    lf.write_text("")
    assert parse_args(_argv(src, lf)).labels == {}


@pytest.mark.parametrize("text", ["missing.png 1\n",            # not a file of --input_dir
                                  "a.png one\n",                # not an integer
                                  "a.png 1.0\n",
                                  "a.png 3\n",                  # the shipped config has num_classes = 3
                                  "a.png -1\n",
                                  "a.png\n"])                   # no label at all
def test_label_file_errors_end_the_run_at_parse_time(tmp_path, text):
    from srgd_amd.inference import parse_args
    src = _folder(tmp_path)
    lf = tmp_path / "labels.txt"
    lf.write_text("b.png 2\n" + text)
    with pytest.raises(SystemExit):
        parse_args(_argv(src, lf))


def test_label_file_that_cannot_be_read_ends_the_run(tmp_path):
    from srgd_amd.inference import parse_args
    with pytest.raises(SystemExit):
        parse_args(_argv(_folder(tmp_path), tmp_path / "nowhere.txt"))


def test_cli_groups_carry_each_files_label(tmp_path, monkeypatch):
    # the folder walk with the sampling replaced: which labels reach which call
    from PIL import Image
    import srgd_amd.inference as I
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    for name in "abcde":
        Image.new("RGB", (120, 80), (10, 20, 30)).save(src / f"{name}.png")
    calls = []

    def fake_many(images, sr_model, test_label=None, **kw):
        calls.append(test_label)
        return [Image.new("RGB", (im.size[0] * 4, im.size[1] * 4)) for im in images]

    def fake_one(image, sr_model, test_label=None, **kw):
        return fake_many([image], sr_model, test_label=test_label, **kw)[0]
    for fn in ("sr_target_images_mixed", "sr_target_images"):
        monkeypatch.setattr(I, fn, fake_many)
    monkeypatch.setattr(I, "sr_target_image", fake_one)
    labels = {"a.png": 0, "d.png": 2}
    I.batch_sr_target_images(str(src), str(dst), sr_model=None, test_label=1, lockstep_tiles=18, labels=labels)
    assert calls == [[0, 1], [1, 2], 1]                      # a, b | c, d | e: mixed groups get a list, others one label
    calls.clear()
    I.batch_sr_target_images(str(src), str(tmp_path / "out2"), sr_model=None, test_label=1, lockstep=3, labels=labels)
    assert calls == [[0, 1, 1], [2, 1]]
    calls.clear()
    I.batch_sr_target_images(str(src), str(tmp_path / "out3"), sr_model=None, test_label=1, lockstep=2)
    assert calls == [1, 1, 1]                                # no label file: one label per call, as before
    calls.clear()
    # without --test_label the unnamed images carry no label: they do not join a labelled group
    I.batch_sr_target_images(str(src), str(tmp_path / "out4"), sr_model=None, test_label=None, lockstep=5, labels=labels)
    assert calls == [0, None, 2, None]


def test_label_entries_are_exported_and_declared():
    from srgd_amd import _lib
    from srgd_amd.build import build
    build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srgd_hip.h")).read(), flags=re.S)
    for name in ("srgd_unet_forward_labels", "srgd_sampler_image_labels"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.lib(), name)
    # the existing entries keep their signatures: labels come through new calls only
    assert re.search(r"srgd_unet_forward\s*\([^)]*int class_id", text)
    assert re.search(r"srgd_sampler_image_labels\s*\(\s*srgd_engine\s*\*\s*e,\s*const int32_t\s*\*\s*class_ids_host,\s*int n_images", text)
