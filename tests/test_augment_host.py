"""CPU-only: the numpy restatement of the augmentation arithmetic (tests/aug_ref.py) equals Pillow bit for bit; the split
of DataAugmentationDINO into draw + apply changes neither its tensors nor its use of the generator (fixture recorded
from the code before the split: tests/golden/make_golden_dino_aug.py); the C entries and the command-line switch."""
import ctypes
import dataclasses
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import aug_ref  # noqa: E402
import make_golden_dino_aug as fixture  # noqa: E402

from sais_amd.dino_data import (DataAugmentationDINO, ViewParams, apply_view_pillow, draw_view,  # noqa: E402
                                random_resized_crop)


@pytest.fixture(scope="module")
def cube():
    """Every RGB triple once, 4096 x 4096."""
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


# ------------------------------------------------------------------ aug_ref == Pillow
def test_luma_grayscale_solarize_on_every_colour(cube):
    img = Image.fromarray(cube)
    assert np.array_equal(aug_ref.luma(cube), np.asarray(img.convert("L")))
    assert np.array_equal(aug_ref.grayscale(cube), np.asarray(img.convert("L").convert("RGB")))
    assert np.array_equal(aug_ref.solarize(cube), np.asarray(ImageOps.solarize(img)))


@pytest.mark.parametrize("factor", [0.6, 0.8, 0.83, 1.0, 1.17, 1.2, 1.4])
def test_enhancers_on_every_colour(cube, factor):
    img = Image.fromarray(cube)
    assert np.array_equal(aug_ref.brightness(cube, factor), np.asarray(ImageEnhance.Brightness(img).enhance(factor)))
    assert np.array_equal(aug_ref.saturation(cube, factor), np.asarray(ImageEnhance.Color(img).enhance(factor)))
    assert np.array_equal(aug_ref.contrast(cube, factor), np.asarray(ImageEnhance.Contrast(img).enhance(factor)))


def test_contrast_mean_rounding():
    rng = np.random.default_rng(0)
    for k in range(20):
        a = rng.integers(0, 40 + 10 * k, (31, 17, 3), dtype=np.uint8)
        for f in (0.6, 1.4):
            assert np.array_equal(aug_ref.contrast(a, f), np.asarray(ImageEnhance.Contrast(Image.fromarray(a)).enhance(f)))


def test_hue_on_every_colour(cube):
    img = Image.fromarray(cube)
    hsv = np.asarray(img.convert("HSV"))
    assert np.array_equal(aug_ref.rgb_to_hsv(cube), hsv)
    for factor in (-0.1, -0.05, -0.004, 0.0, 0.02, 0.1):
        shift = int(factor * 255)
        hh = hsv.copy()
        hh[..., 0] = (hh[..., 0].astype(np.int16) + shift) % 256
        want = np.asarray(Image.fromarray(hh, "HSV").convert("RGB"))
        assert np.array_equal(aug_ref.hue(cube, shift), want), factor


def test_hsv_to_rgb_on_every_triple(cube):
    """Every (H, S, V), not only those rgb_to_hsv produces."""
    assert np.array_equal(aug_ref.hsv_to_rgb(cube), np.asarray(Image.fromarray(cube, "HSV").convert("RGB")))


@pytest.mark.parametrize("radius", [0.1, 0.25, 0.5, 0.7, 1.0, 1.3, 1.5, 1.77, 1.9999, 2.0])
def test_gaussian_blur(radius):
    rng = np.random.default_rng(int(radius * 100))
    yy, xx = np.mgrid[0:96, 0:224]
    smooth = np.stack([128 + 100 * np.sin(xx / 9.0 + c) * np.cos(yy / 6.0) for c in range(3)], -1).astype(np.uint8)
    for a in (rng.integers(0, 256, (224, 224, 3), dtype=np.uint8), rng.integers(0, 256, (96, 96, 3), dtype=np.uint8), smooth):
        want = np.asarray(Image.fromarray(a).filter(ImageFilter.GaussianBlur(radius=radius)))
        assert np.array_equal(aug_ref.gaussian_blur(a, radius), want)


BOXES = [((10, 20, 910, 560), 224), ((100, 50, 271, 180), 96), ((5, 5, 45, 35), 96), ((0, 0, 1024, 576), 224),
         ((3, 100, 4, 300), 96), ((800, 0, 1024, 224), 224), ((0, 0, 96, 300), 96), ((1000, 500, 1024, 576), 224),
         ((0, 575, 1024, 576), 96), ((1023, 0, 1024, 576), 224), ((17, 3, 18, 4), 96), ((0, 0, 1024, 576), 96),
         ((300, 200, 524, 424), 224), ((300, 200, 523, 425), 224)]


@pytest.mark.parametrize("box,size", BOXES)
def test_crop_resize(box, size):
    rng = np.random.default_rng(1)
    frame = rng.integers(0, 256, (576, 1024, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(frame).crop(box).resize((size, size), Image.BICUBIC))
    assert np.array_equal(aug_ref.crop_resize(frame, box, size), want)


def test_whole_view_through_the_reference():
    """aug_ref.view(frame, params) == apply_view_pillow for drawn parameters (every op in the chain, in order)."""
    rng = random.Random(12)
    img = fixture.image(180, 320, 3)
    a = np.asarray(img)
    for k in range(24):
        p = draw_view(rng, 320, 180, (48, 32)[k % 2], (0.05, 1.0), 0.7, 0.5)
        assert np.array_equal(aug_ref.view(a, p), apply_view_pillow(img, p).numpy()), p


# ------------------------------------------------------------------ draw + apply == what DataAugmentationDINO did
def test_draw_then_apply_equals_call_and_leaves_the_generator_alike():
    img = fixture.image(120, 160, 8)
    a = DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), 4, seed=21, global_size=40, local_size=24)
    b = DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), 4, seed=21, global_size=40, local_size=24)
    seen = set()
    for _ in range(12):
        crops = a(img)
        params = b.draw(*img.size)
        assert len(params) == 6 and [p.size for p in params] == [40, 40, 24, 24, 24, 24]
        assert all(torch.equal(c, apply_view_pillow(img, p)) for c, p in zip(crops, params))
        assert a.rng.getstate() == b.rng.getstate()
        for p in params:
            seen |= {("flip", p.flip), ("jitter", p.jitter), ("gray", p.gray), ("blur", p.blur is not None), ("sol", p.solarize)}
            assert p.jitter or (p.brightness, p.contrast, p.saturation, p.hue) == (1.0, 1.0, 1.0, 0.0)
            assert p.blur is None or 0.1 <= p.blur <= 2.0
    assert len(seen) == 10                                          # every gate was seen open and closed
    assert params[0].blur is not None and not params[0].solarize     # first global view: blur p = 1, no solarize gate


def test_parent_commit_fixture():
    """The crops and the generator state recorded before draw / apply were split."""
    g = np.load(os.path.join(HERE, "golden", "dino_aug.npz"))
    for name, (h, w), seed, nloc, gs, ls, calls in fixture.CASES:
        aug = DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), nloc, seed=seed, global_size=gs, local_size=ls)
        via_draw = DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), nloc, seed=seed, global_size=gs, local_size=ls)
        img = fixture.image(h, w, seed)
        for k in range(calls):
            crops = aug(img)
            split = [apply_view_pillow(img, p) for p in via_draw.draw(w, h)]
            assert len(crops) == 2 + nloc
            for i, (c, s) in enumerate(zip(crops, split)):
                assert np.array_equal(c.numpy(), g[f"{name}_{k}_{i}"]), (name, k, i)
                assert np.array_equal(s.numpy(), g[f"{name}_{k}_{i}"]), (name, k, i)
        assert np.array_equal(fixture.state_digest(aug.rng), g[f"{name}_state"]), name
        assert np.array_equal(fixture.state_digest(via_draw.rng), g[f"{name}_state"]), name


def test_fallback_branch_is_drawn_and_applied_alike():
    """8 x 400: no attempt of RandomResizedCrop fits (ratio <= 4/3, area >= 5 %), the centre-crop fallback is taken."""
    W, H = 400, 8
    img = fixture.image(H, W, 2)
    r1, r2 = random.Random(5), random.Random(5)
    for _ in range(5):
        p = draw_view(r1, W, H, 16, (0.05, 0.4), 0.5)
        assert p.box == ((W - 11) // 2, 0, (W - 11) // 2 + 11, 8)                  # w = round(8 * 4/3), h = H
        want = random_resized_crop(img, 16, (0.05, 0.4), r2)
        assert np.array_equal(np.asarray(want), aug_ref.crop_resize(np.asarray(img), p.box, 16))
        assert np.array_equal(np.asarray(want), np.asarray(img.crop(p.box).resize((16, 16), Image.BICUBIC)))
        _replay_after_crop(r2)                                       # r2 catches up with the non-crop draws of r1
        assert r1.getstate() == r2.getstate()
    tall = draw_view(random.Random(1), 8, 400, 16, (0.4, 1.0), 1.0)
    assert tall.box == (0, (400 - 11) // 2, 8, (400 - 11) // 2 + 11)


def _replay_after_crop(rng):
    """Consume what a view consumes after its crop (blur p = 0.5, no solarize gate), as _view always has."""
    rng.random()
    if rng.random() < 0.8:
        ops = [0, 1, 2, 3]
        rng.shuffle(ops)
        for _ in range(4):
            rng.uniform(0, 1)
    rng.random()
    if rng.random() <= 0.5:
        rng.uniform(0.1, 2.0)


# ------------------------------------------------------------------ C entries, binding, command line
def test_header_struct_and_exports():
    from sais_amd import _lib
    from sais_amd.augment import VIEW_DTYPE, normalize_table, view_table
    from sais_amd.dino_data import to_normalized_tensor
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sais_hip.h")).read()
    for name in ("sais_augment_workspace_bytes", "sais_augment_crop_resize", "sais_augment_color"):
        assert name in hdr and name in _lib.SIGNATURES
    assert "#define SAIS_ABI_VERSION 13" in hdr and "#define SAIS_AUG_MAX_SIZE 224" in hdr
    assert VIEW_DTYPE.itemsize == ctypes.sizeof(_lib.SaisAugView) == 104
    for f, _ in _lib.SaisAugView._fields_:
        assert VIEW_DTYPE.fields[f][1] == getattr(_lib.SaisAugView, f).offset, f
    ramp = np.repeat(np.arange(256, dtype=np.uint8).reshape(1, 256, 1), 3, -1)
    assert np.array_equal(normalize_table(), to_normalized_tensor(Image.fromarray(ramp))[:, 0, :].numpy())
    p = ViewParams((1, 2, 30, 40), 96, True, True, (3, 1, 0, 2), 0.7, 1.2, 0.9, -0.1, False, 1.5, True)
    q = dataclasses.replace(p, size=224, blur=None, jitter=False)
    t, sizes = view_table([[q, p], [q, p]])
    assert sizes == [224, 96] and len(t) == 4 and list(t["frame"]) == [0, 1, 0, 1] and list(t["size"]) == [224, 224, 96, 96]
    assert list(t["u8_offset"]) == [0, 150528, 301056, 301056 + 27648] and list(t["out_offset"]) == list(t["u8_offset"])
    assert t[2]["hue_shift"] == -25 and t[2]["blur"] == 1 and t[0]["blur"] == 0 and list(t[3]["order"]) == [3, 1, 0, 2]
    assert _lib.load().sais_augment_workspace_bytes(t.ctypes.data, 4) == (301056 + 2 * 27648 + 255) // 256 * 256


def test_bad_arguments_are_rejected_without_a_gpu():
    from sais_amd import _lib
    from sais_amd.augment import view_table
    lib = _lib.load()
    p = ViewParams((0, 0, 30, 40), 96, False, True, (0, 1, 2, 3), 1.0, 1.0, 1.0, 0.0, False, 1.0, False)
    one = ctypes.c_void_p(16)                                      # a non-null pointer nothing dereferences
    border = (ctypes.c_int * 4)(0, 0, 64, 48)

    def resize(params, border=border, nframes=1, h=48, w=64, nbytes=1 << 20):
        t, _ = view_table([params])
        return lib.sais_augment_crop_resize(one, nframes, h, w, border, t.ctypes.data, one, len(t), one, nbytes, None)

    def color(params, nbytes=1 << 20, nout=1 << 20):
        t, _ = view_table([params])
        return lib.sais_augment_color(one, nbytes, t.ctypes.data, one, len(t), one, one, nout, None)

    assert lib.sais_augment_workspace_bytes(None, 1) == 0
    assert lib.sais_augment_crop_resize(None, 1, 48, 64, border, None, None, 1, None, 0, None) == -1
    assert lib.sais_augment_color(None, 0, None, None, 1, None, None, 0, None) == -1
    rep = dataclasses.replace
    for bad in (rep(p, box=(0, 0, 65, 40)), rep(p, box=(0, 0, 30, 49)), rep(p, box=(10, 0, 10, 40)), rep(p, box=(-1, 0, 30, 40)),
                rep(p, size=225), rep(p, size=0)):
        assert resize([bad]) == -1, bad
    assert resize([p], border=(ctypes.c_int * 4)(0, 0, 65, 48)) == -1 and resize([p], nframes=0) == -1
    assert resize([p], nbytes=96 * 96 * 3 - 1) == -1
    for bad in (rep(p, blur=2.01), rep(p, blur=-1.0), rep(p, blur=float("nan")), rep(p, order=(0, 0, 1, 2)), rep(p, order=(0, 1, 2, 4)),
                rep(p, brightness=-0.1), rep(p, contrast=2.5), rep(p, saturation=float("inf")), rep(p, size=225)):
        assert color([bad]) == -1, bad
    assert color([p], nbytes=96 * 96 * 3 - 1) == -1 and color([p], nout=96 * 96 * 3 - 1) == -1


def test_cli_switch_and_untouched_reference_parser():
    from test_dino_host import _load_cli
    mod = _load_cli()
    cli = mod.get_cli_parser()
    assert cli.parse_args([]).gpu_augment is False
    assert cli.parse_args(["--gpu_augment", "true", "--epochs", "3"]).gpu_augment is True
    with pytest.raises(SystemExit):
        cli.parse_args(["--gpu_augment", "maybe"])
    flags = {a.option_strings[0] for a in mod.get_args_parser()._actions if a.option_strings}
    assert "--gpu_augment" not in flags
    assert {a.option_strings[0] for a in cli._actions if a.option_strings} - flags == {"-h", "--gpu_augment"}
    assert not hasattr(mod.get_args_parser().parse_args([]), "gpu_augment")


def test_gpu_mode_items_carry_bytes_header_and_draws(tmp_path):
    import pandas as pd
    from sais_amd import jpeg
    from sais_amd.dino_data import SurgDataset, border_box, collate_raw
    root = tmp_path / "frames"
    (root / "v").mkdir(parents=True)
    (tmp_path / "paths").mkdir()
    rng = np.random.default_rng(0)
    arr = rng.integers(0, 256, (90, 160, 3), dtype=np.uint8)
    Image.fromarray(arr).save(root / "v" / "a.jpg", quality=90)
    Image.fromarray(arr).save(root / "v" / "b.jpg", quality=90, progressive=True)
    pd.DataFrame([("v\\a.jpg", "x"), ("v\\b.jpg", "y")], columns=["path", "label"]).to_csv(tmp_path / "paths" / "VUA_Gronau_Paths.csv")
    mk = lambda: DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), 2, seed=6)
    raw = SurgDataset(str(tmp_path), ["VUA_Gronau"], mk(), frames_root=str(root), gpu_augment=True)
    pil = SurgDataset(str(tmp_path), ["VUA_Gronau"], mk(), frames_root=str(root))
    assert border_box(160, 90, raw.crop_fracs()) == (24, 9, 112, 72)
    for i in range(2):
        blob, hdr, params, label, name = raw[i]
        assert blob == (root / "v" / ("a.jpg", "b.jpg")[i]).read_bytes()
        assert (hdr is None) == (i == 1) and label == "xy"[i] and name == "VUA_Gronau"
        if hdr is not None:
            h = jpeg.SaisJpegHeader.from_buffer_copy(hdr)
            assert (h.height, h.width) == (90, 160)
        crops, _, _ = pil[i]                                         # same seed, same order of items: the same views
        img = Image.open(root / "v" / ("a.jpg", "b.jpg")[i]).crop((24, 9, 136, 81))
        assert all(torch.equal(c, apply_view_pillow(img, p)) for c, p in zip(crops, params))
    items, labels, names = collate_raw([raw[0], raw[1]])
    assert len(items) == 2 and labels == ["x", "y"] and names == ["VUA_Gronau"] * 2
