"""GPU: sais_amd.augment.DinoAugmenter equals the Pillow path of sais_amd/dino_data.py bit for bit — the colour half on
every RGB triple, the crop + resize half on the frame sizes of test_preprocess, the whole path from JPEG files to the
crop list, and main_dino.py --gpu_augment."""
import dataclasses
import io
import math
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_jpeg_host import encode, frame  # noqa: E402
from test_preprocess import SIZES  # noqa: E402

from sais_amd.dino_data import (BRIGHTNESS, CONTRAST, HUE, SATURATION, DataAugmentationDINO, ViewParams,  # noqa: E402
                                apply_view_pillow, border_box, gpu_crops, to_normalized_tensor)

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
PLAIN = ViewParams(box=(0, 0, 1, 1), size=224, flip=False, jitter=False, order=(0, 1, 2, 3), brightness=1.0, contrast=1.0,
                   saturation=1.0, hue=0.0, gray=False, blur=None, solarize=False)


def vp(**kw):
    return dataclasses.replace(PLAIN, **kw)


def only(op, factor):
    """Jitter parameters under which `op` is the one step that changes pixels (factor 1 blends are the identity); the
    op comes first, so it sees the input image."""
    order = (op,) + tuple(o for o in (BRIGHTNESS, CONTRAST, SATURATION) if o != op)
    name = {BRIGHTNESS: "brightness", CONTRAST: "contrast", SATURATION: "saturation"}[op]
    return vp(jitter=True, order=order + (HUE,), **{name: factor})


def lut():
    """to_normalized_tensor of every byte: [3][256]."""
    ramp = np.repeat(np.arange(256, dtype=np.uint8).reshape(1, 256, 1), 3, -1)
    return to_normalized_tensor(Image.fromarray(ramp))[:, 0, :]


def normalized(u8, table):
    """uint8 [N,s,s,3] (device) -> float [N,3,s,s] through the table."""
    x = u8.permute(0, 3, 1, 2).long()
    return torch.stack([table[c][x[:, c]] for c in range(3)], 1)


@pytest.fixture(scope="module")
def aug():
    from sais_amd.augment import DinoAugmenter
    return DinoAugmenter(DEV)


@pytest.fixture(scope="module")
def cube():
    """Every RGB triple once, as 335 views of 224 x 224 (the tail is black)."""
    n = -(-(1 << 24) // (224 * 224))
    c = np.zeros(n * 224 * 224, np.uint32)
    c[:1 << 24] = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(n, 224, 224, 3)


def run_color(aug, views, p):
    got = aug.color([torch.from_numpy(views).to(DEV)], [[p]] * len(views))
    assert len(got) == 1
    return got[0]


def check_color(aug, views, p, expected_u8):
    got = run_color(aug, views, p)
    want = normalized(torch.from_numpy(np.ascontiguousarray(expected_u8)).to(DEV), lut().to(DEV))
    assert torch.equal(got, want), (p, int((got != want).sum()))


# ------------------------------------------------------------------ second half alone
@gpu
@pytest.mark.parametrize("factor", [0.6, 0.8, 1.0, 1.2, 1.4])
def test_brightness_and_saturation_on_every_colour(aug, cube, factor):
    img = Image.fromarray(cube.reshape(-1, 224, 3))
    # hue comes last in only(): it is a round trip through HSV, applied to the expectation too
    def after_hue(im):
        return np.asarray(im.convert("HSV").convert("RGB")).reshape(cube.shape)
    check_color(aug, cube, only(BRIGHTNESS, factor), after_hue(ImageEnhance.Brightness(img).enhance(factor)))
    check_color(aug, cube, only(SATURATION, factor), after_hue(ImageEnhance.Color(img).enhance(factor)))


@gpu
@pytest.mark.parametrize("factor", [0.6, 0.8, 1.0, 1.2, 1.4])
def test_contrast_on_every_colour(aug, cube, factor):
    """The degenerate image is the view's own mean luminance: Pillow runs per view."""
    want = np.stack([np.asarray(ImageEnhance.Contrast(Image.fromarray(v)).enhance(factor).convert("HSV").convert("RGB"))
                     for v in cube])
    check_color(aug, cube, only(CONTRAST, factor), want)


@gpu
@pytest.mark.parametrize("hue", [-0.1, -0.037, 0.0, 0.004, 0.05, 0.1])
def test_hue_on_every_colour(aug, cube, hue):
    h, s, v = Image.fromarray(cube.reshape(-1, 224, 3)).convert("HSV").split()
    hh = (np.asarray(h, dtype=np.int16) + int(hue * 255)) % 256
    want = np.asarray(Image.merge("HSV", (Image.fromarray(hh.astype(np.uint8), "L"), s, v)).convert("RGB"))
    check_color(aug, cube, vp(jitter=True, order=(HUE, BRIGHTNESS, CONTRAST, SATURATION), hue=hue), want.reshape(cube.shape))


@gpu
def test_grayscale_solarize_flip_and_identity_on_every_colour(aug, cube):
    img = Image.fromarray(cube.reshape(-1, 224, 3))
    check_color(aug, cube, PLAIN, cube)
    check_color(aug, cube, vp(gray=True), np.asarray(img.convert("L").convert("RGB")).reshape(cube.shape))
    check_color(aug, cube, vp(solarize=True), np.asarray(ImageOps.solarize(img)).reshape(cube.shape))
    check_color(aug, cube, vp(flip=True), cube[:, :, ::-1])
    check_color(aug, cube, vp(gray=True, solarize=True, flip=True),
                np.asarray(ImageOps.solarize(img.convert("L").convert("RGB"))).reshape(cube.shape)[:, :, ::-1])


@gpu
@pytest.mark.parametrize("size", [224, 96])
def test_blur_radii_on_noise_and_smooth_views(aug, size):
    rng = np.random.default_rng(5)
    views = np.stack([rng.integers(0, 256, (size, size, 3), dtype=np.uint8), frame(size, size, 0), frame(size, size, 30, seed=2),
                      np.full((size, size, 3), 255, np.uint8)])
    for radius in [0.1, 0.25, 0.5, 0.7, 1.0, 1.3, 1.5, 1.77, 1.9999, 2.0]:
        want = np.stack([np.asarray(Image.fromarray(v).filter(ImageFilter.GaussianBlur(radius=radius))) for v in views])
        check_color(aug, views, vp(size=size, blur=radius), want)


# ------------------------------------------------------------------ first half alone
def boxes_for(W, H):
    b = [(0, 0, W, H), (0, 0, max(W // 3, 1), max(H // 3, 1)), (W - max(W // 2, 1), H - max(H // 2, 1), W, H),
         (W // 2, 0, W // 2 + 1, H), (0, H // 2, W, H // 2 + 1), (W // 4, H // 4, W // 4 + min(40, W - W // 4), H // 4 + min(30, H - H // 4))]
    if W >= 224 and H >= 224:
        b.append((W - 224, H - 224, W, H))                                         # no resampling at 224
    return b


@gpu
@pytest.mark.parametrize("hw", SIZES)
def test_crop_resize_matches_pillow(aug, hw):
    H, W = hw
    a = frame(H, W, 25, seed=H)
    img = Image.fromarray(a)
    frames = torch.from_numpy(a[None]).to(DEV)
    for border in [(0, 0, W, H), border_box(W, H, (0.8, 0.8)), border_box(W, H, (0.8, 0.7))]:
        bl, bt, bw, bh = border
        if bw < 1 or bh < 1:
            continue
        inner = img.crop((bl, bt, bl + bw, bt + bh))
        for box in boxes_for(bw, bh):
            params = [[vp(box=box, size=224), vp(box=box, size=96)]]
            got = aug.crop_resize(frames, params, border)
            for g, s in zip(got, (224, 96)):
                want = np.asarray(inner.crop(box).resize((s, s), Image.BICUBIC))
                assert np.array_equal(g[0].cpu().numpy(), want), (hw, border, box, s)


# ------------------------------------------------------------------ whole path
FORCED = [PLAIN, vp(flip=True), vp(gray=True), vp(blur=0.1), vp(blur=2.0), vp(solarize=True),
          only(BRIGHTNESS, 0.6), only(BRIGHTNESS, 1.4), only(CONTRAST, 0.6), only(CONTRAST, 1.4), only(SATURATION, 0.8),
          only(SATURATION, 1.2), vp(jitter=True, hue=-0.1), vp(jitter=True, hue=0.1)] + \
         [vp(jitter=True, order=o, brightness=0.7, contrast=1.3, saturation=1.15, hue=0.06, flip=i % 2 == 0, gray=i == 3,
             blur=0.9 if i else None, solarize=i == 1)
          for i, o in enumerate([(0, 1, 2, 3), (1, 2, 3, 0), (2, 3, 0, 1), (3, 0, 1, 2), (3, 2, 1, 0)])]


def pillow_views(blob, fracs, params):
    img = Image.open(io.BytesIO(blob))
    left, top, cw, ch = border_box(*img.size, fracs)
    img = img.crop((left, top, left + cw, top + ch)).convert("RGB")
    return [apply_view_pillow(img, p) for p in params]


def item(blob, params):
    from sais_amd import jpeg
    h = jpeg.parse_header(blob)
    return blob, None if h is None else bytes(h), params, 0, "VUA"


def check_batch(aug, blobs, params, fracs):
    from sais_amd.jpeg import JpegDecoder
    got = gpu_crops([item(b, p) for b, p in zip(blobs, params)], JpegDecoder(DEV), aug, fracs)
    want = [pillow_views(b, fracs, p) for b, p in zip(blobs, params)]
    assert len(got) == len(params[0])
    for j, g in enumerate(got):
        w = torch.stack([want[i][j] for i in range(len(blobs))])
        assert g.dtype == torch.float32 and torch.equal(g.cpu(), w), (j, int((g.cpu() != w).sum()))


@gpu
@pytest.mark.parametrize("fracs", [(0.8, 0.8), (0.8, 0.7)])
@pytest.mark.parametrize("n_local", [8, 0])
def test_seeded_batch_of_two_geometries_equals_pillow(aug, fracs, n_local):
    geoms = [(270, 480), (216, 384), (270, 480), (270, 480), (216, 384), (216, 384)]
    blobs = [encode(frame(h, w, 12, seed=i), quality=85, subsampling=(2, 0)[i % 2]) for i, (h, w) in enumerate(geoms)]
    t = DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), n_local, seed=4)
    params = [t.draw(*border_box(w, h, fracs)[2:]) for h, w in geoms]
    assert [p.size for p in params[0]] == [224, 224] + [96] * n_local
    check_batch(aug, blobs, params, fracs)


@gpu
def test_forced_parameter_sets_equal_pillow(aug):
    """Nothing applied, flip, every op on its own, the jitter orders with each op once first and once last."""
    geoms = [(270, 480), (231, 517)]
    blobs = [encode(frame(*geoms[i % 2], 12, seed=i), quality=90) for i in range(len(FORCED))]
    params = []
    for i, f in enumerate(FORCED):
        h, w = geoms[i % 2]
        _, _, cw, ch = border_box(w, h, (0.8, 0.8))
        params.append([dataclasses.replace(f, box=(3, 5, cw - 7, ch - 2), size=224),
                       dataclasses.replace(f, box=(cw // 3, ch // 4, cw // 3 + 50, ch // 4 + 41), size=96)])
    check_batch(aug, blobs, params, (0.8, 0.8))


@gpu
def test_progressive_and_grayscale_files_go_through_the_host(aug):
    a = frame(200, 300, 10, seed=3)
    blobs = [encode(a, quality=85), encode(a[::-1].copy(), quality=85, progressive=True), encode(a[..., 1], quality=85),
             encode(a[:, ::-1].copy(), quality=70, subsampling=0)]
    assert [item(b, None)[1] is None for b in blobs] == [False, True, True, False]
    t = DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), 3, seed=9)
    params = [t.draw(*border_box(300, 200, (0.8, 0.8))[2:]) for _ in blobs]
    check_batch(aug, blobs, params, (0.8, 0.8))


# ------------------------------------------------------------------ errors: rejected on the host side, nothing launched
@gpu
def test_out_of_range_parameters_are_rejected(aug):
    from sais_amd import _lib
    frames = torch.zeros(1, 64, 80, 3, dtype=torch.uint8, device=DEV)
    border = (0, 0, 80, 64)
    ok = vp(box=(0, 0, 80, 64), size=96)
    assert aug(frames, [[ok]], border)[0].shape == (1, 3, 96, 96)
    torch.cuda.synchronize()
    for bad in [vp(box=(0, 0, 81, 64), size=96), vp(box=(5, 5, 5, 20), size=96), vp(box=(-1, 0, 10, 10), size=96),
                vp(box=(0, 0, 80, 64), size=225), vp(box=(0, 0, 80, 64), size=0),
                dataclasses.replace(ok, blur=2.5), dataclasses.replace(ok, blur=-0.1), dataclasses.replace(ok, blur=float("nan")),
                dataclasses.replace(ok, jitter=True, order=(0, 1, 2, 2)), dataclasses.replace(ok, jitter=True, brightness=2.5),
                dataclasses.replace(ok, jitter=True, contrast=-0.5)]:
        with pytest.raises(_lib.SaisHipError):
            aug(frames, [[bad]], border)
    with pytest.raises(_lib.SaisHipError):
        aug(frames, [[ok]], (0, 0, 81, 64))                              # border outside the frame
    torch.cuda.synchronize()
    assert aug(frames, [[ok]], border)[0].shape == (1, 3, 96, 96)         # and the augmenter still works


def test_cpu_device_raises():
    from sais_amd import _lib
    from sais_amd.augment import DinoAugmenter
    with pytest.raises(_lib.SaisHipError):
        DinoAugmenter("cpu")


# ------------------------------------------------------------------ the command line
def _dataset(tmp_path, n=8):
    import pandas as pd
    d = tmp_path / "frames" / "Images" / "vidA"
    d.mkdir(parents=True)
    (tmp_path / "paths").mkdir()
    rows = []
    for i in range(n):
        h, w = ((270, 480), (216, 384))[i % 2]
        (d / f"frames_{i:08d}.jpg").write_bytes(encode(frame(h, w, 15, seed=i), quality=90))
        rows.append((f"Images\\vidA\\frames_{i:08d}.jpg", "vidA"))
    pd.DataFrame(rows, columns=["path", "label"]).to_csv(tmp_path / "paths" / "VUA_Paths.csv")


@gpu
def test_main_dino_with_gpu_augment(tmp_path):
    import json
    import subprocess
    from test_dino_host import _load_cli
    _dataset(tmp_path)
    out = tmp_path / "out"
    flags = ["--data_path", str(tmp_path), "--frames_root", str(tmp_path / "frames"), "--datasets", "VUA", "--output_dir", str(out),
             "--batch_size_per_gpu", "4", "--local_crops_number", "2", "--out_dim", "1024", "--warmup_epochs", "1",
             "--num_workers", "0", "--saveckp_freq", "1", "--lr", "0.01", "--seed", "3"]
    # the first batch of both loaders, same seed, no workers: the same crops
    mod = _load_cli()
    first = []
    for switch in ("false", "true"):
        args = mod.get_cli_parser().parse_args(flags + ["--gpu_augment", switch])
        args.rank, args.world_size = 0, 1
        _, sampler, loader, to_device = mod.build_loader(args, torch.device(DEV))
        sampler.set_epoch(0)
        first.append([c.cpu() for c in to_device(next(iter(loader))[0])])
    assert [tuple(c.shape) for c in first[1]] == [(4, 3, 224, 224)] * 2 + [(4, 3, 96, 96)] * 2
    assert all(torch.equal(a, b) for a, b in zip(*first))
    cmd = [sys.executable, os.path.join(os.path.dirname(HERE), "SAIS", "scripts", "dino-main", "main_dino.py")] + flags
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(28800 + os.getpid() % 1000), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd + ["--epochs", "1", "--gpu_augment", "true"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    log = [json.loads(l) for l in open(out / "log.txt")]
    assert [l["epoch"] for l in log] == [0] and math.isfinite(log[0]["train_loss"]) and log[0]["train_loss"] > 0
    ck = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["args"].gpu_augment is True
