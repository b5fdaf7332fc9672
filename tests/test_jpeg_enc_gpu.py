"""The JPEG encoder (csrc/jpeg_enc.hip, sais_amd/jpeg_enc.py) on a real MI355X: its files against Pillow + libjpeg-turbo byte for
byte, its status for slots that are too small, and the two scripts that write their images through it."""
import csv
import importlib.util
import io
import os
import sys

import numpy as np
import pytest
import torch

from tests import jpeg_enc_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DPI = (100, 100)


@pytest.fixture(scope="module")
def enc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sais_amd.jpeg_enc import JpegEncoder
    return JpegEncoder(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _script(path):
    spec = importlib.util.spec_from_file_location("jpeg_enc_cli_" + os.path.basename(path)[:-3], os.path.join(ROOT, "SAIS", "scripts", path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _heat_maps(frames, grid, seed):
    """rendered inferno heat maps u8 [frames, 16 h, 16 w, 3] on the device: the workload's kind of content"""
    from sais_amd import attnviz
    g = torch.Generator().manual_seed(seed)
    probs = torch.softmax(3 * torch.randn(frames, 6, 1 + grid[0] * grid[1], generator=g), dim=2)
    return attnviz.render(probs.to(DEV), grid, threshold=0.6, cmap="inferno", patch=16)[1]


def test_whole_matrix_equals_pillow(enc):
    """every case of the host test's matrix; the four kinds of content of one (geometry, quality, subsampling) share a batch"""
    for (H, W) in R.GEOMETRIES:
        imgs = [R.content(kind, H, W) for kind in R.CONTENTS]
        batch = dev(np.stack(imgs))
        for q in R.QUALITIES:
            for s in R.SUBSAMPLINGS:
                for dpi in (None, DPI):
                    files = enc.encode(batch, quality=q, subsampling=s, dpi=dpi)
                    for kind, a, f in zip(R.CONTENTS, imgs, files):
                        assert f == R.pillow_file(a, q, s, dpi), (H, W, kind, q, s, dpi)


@pytest.mark.parametrize("n", [1, 3, 64])
def test_batches_of_mixed_content(enc, n):
    imgs = [R.content(R.CONTENTS[(i * 3 + i // 4) % 4], 37, 53, seed=i) for i in range(n)]
    for s in R.SUBSAMPLINGS:
        files = enc.encode(dev(np.stack(imgs)), quality=75, subsampling=s)
        assert n < 3 or len({len(f) for f in files}) > 1                   # lengths differ within the batch
        for i, (a, f) in enumerate(zip(imgs, files)):
            assert f == R.pillow_file(a, 75, s), (n, i, s)


@pytest.mark.parametrize("grid", [(6, 10), (30, 53)])
def test_rendered_heat_maps(enc, grid):
    rgb = _heat_maps(2, grid, 17)
    assert tuple(rgb.shape) == (2, 16 * grid[0], 16 * grid[1], 3)
    host = rgb.cpu().numpy()
    for j, f in enumerate(enc.encode(rgb, dpi=DPI)):
        assert f == R.pillow_file(host[j], 75, 2, DPI), (grid, j)


def test_two_launches_give_the_same_bytes(enc):
    batch = dev(np.stack([R.content(kind, 130, 250) for kind in R.CONTENTS]))
    out, nbytes = enc.encode_to_device(batch, quality=95)
    first, lens = out.clone(), nbytes.clone()
    out.fill_(0x5A)
    out2, nbytes2 = enc.encode_to_device(batch, quality=95)
    assert torch.equal(lens, nbytes2)
    for i, m in enumerate(lens.tolist()):
        assert m > 2 and torch.equal(first[i, :m], out2[i, :m]), i


def test_one_encoder_across_geometries_and_qualities(enc):
    for (H, W, kind, q, s) in [(130, 250, "noise", 100, 0), (1, 1, "flat", 1, 2), (37, 53, "ramp", 50, 2), (130, 250, "ramp", 24, 2),
                               (9, 40, "saturated", 95, 0), (130, 250, "noise", 100, 0)]:
        a = R.content(kind, H, W)
        assert enc.encode(dev(a[None]), quality=q, subsampling=s) == [R.pillow_file(a, q, s)], (H, W, kind, q, s)


def test_slot_too_small_is_a_status(enc):
    """out_stride holds the flat images, not the noise images: -1 for the latter, nothing written to their slots, and nothing
    written past the end of any stream"""
    from sais_amd.jpeg_enc import header
    kinds = ["flat", "noise", "flat", "saturated", "noise", "flat"]
    imgs = [R.content(k, 37, 53, seed=i) for i, k in enumerate(kinds)]
    want = [R.pillow_file(a, 90, 2)[len(header(37, 53, 90, 2)):] for a in imgs]
    stride = max(len(w) for k, w in zip(kinds, want) if k == "flat") + 16
    assert all(len(w) > stride for k, w in zip(kinds, want) if k != "flat")
    out = torch.full((len(imgs), stride), 0xA5, dtype=torch.uint8, device=DEV)
    got, nbytes = enc.encode_to_device(dev(np.stack(imgs)), quality=90, out=out)
    assert got is out
    lens, host = nbytes.cpu().tolist(), out.cpu().numpy()
    for i, k in enumerate(kinds):
        if k == "flat":
            assert lens[i] == len(want[i]) and host[i, :lens[i]].tobytes() == want[i], i
            assert (host[i, lens[i]:] == 0xA5).all(), i
        else:
            assert lens[i] == -1 and (host[i] == 0xA5).all(), i
    for width, fit in ((len(want[0]), True), (len(want[0]) - 1, False)):                 # the tightest slot that fits, and one less
        _, nb = enc.encode_to_device(dev(imgs[0][None]), quality=90, out_stride=width)
        assert nb.cpu().tolist() == [len(want[0]) if fit else -1]


def test_slots_past_two_gib(enc):
    """three small images in slots of 2^30 + 8 bytes: the third slot starts past 2^31"""
    from sais_amd.jpeg_enc import header
    imgs = [R.content(k, 17, 13, seed=i) for i, k in enumerate(("noise", "ramp", "saturated"))]
    want = [R.pillow_file(a, 75, 2)[len(header(17, 13, 75, 2)):] for a in imgs]
    out = torch.full((3, 2 ** 30 + 8), 0xA5, dtype=torch.uint8, device=DEV)
    _, nbytes = enc.encode_to_device(dev(np.stack(imgs)), out=out)
    assert nbytes.cpu().tolist() == [len(w) for w in want]
    for i, w in enumerate(want):
        assert out[i, :len(w)].cpu().numpy().tobytes() == w, i
        assert bool((out[i, len(w):] == 0xA5).all()), i
    del out
    torch.cuda.empty_cache()


def test_round_trip_through_the_decoder(enc):
    from PIL import Image
    from sais_amd.jpeg import JpegDecoder
    imgs = [R.content(kind, 130, 250) for kind in R.CONTENTS]
    for s in R.SUBSAMPLINGS:
        files = enc.encode(dev(np.stack(imgs)), quality=75, subsampling=s)
        dec = JpegDecoder(DEV)
        got = dec.decode(files).cpu().numpy()
        assert dec.stats["gpu"] == len(files)
        for i, a in enumerate(imgs):
            assert np.array_equal(got[i], np.asarray(Image.open(io.BytesIO(R.pillow_file(a, 75, s))))), (s, i)


def test_save_jpegs_equals_save_jpeg(enc, tmp_path):
    from sais_amd import attnviz
    rgb = _heat_maps(3, (6, 10), 23)
    names = [str(tmp_path / f"batch-{j}.jpg") for j in range(3)]
    attnviz.save_jpegs(names, rgb)
    for j, name in enumerate(names):
        attnviz.save_jpeg(str(tmp_path / "one.jpg"), rgb[j])
        assert open(name, "rb").read() == (tmp_path / "one.jpg").read_bytes(), j
    with pytest.raises(ValueError):
        attnviz.save_jpegs(names, rgb.cpu())
    with pytest.raises(ValueError):
        attnviz.save_jpegs(names[:2], rgb)


def test_video_generation_writes_save_jpeg_bytes(enc, tmp_path, monkeypatch):
    """5 synthetic frames through the script: every attn-*.jpg is the file a loop over save_jpeg writes for the rendered frames"""
    from PIL import Image
    from sais_amd import attnviz
    (tmp_path / "in").mkdir()
    rng = np.random.Generator(np.random.PCG64(5))
    yy, xx = np.mgrid[:64, :96]
    names = []
    for t in range(5):
        base = (np.stack([xx * 2.5 + 9 * t, yy * 3.5, (xx + yy) * 1.5], -1) % 256).astype(np.float32)
        names.append(f"frame-{t:04d}.jpg")
        Image.fromarray(np.clip(base + 8 * rng.standard_normal((64, 96, 3)), 0, 255).astype(np.uint8)).save(tmp_path / "in" / names[-1], quality=92)
    rendered = []
    real = attnviz.render
    monkeypatch.setattr(attnviz, "render", lambda *a, **k: rendered.append(real(*a, **k)) or rendered[-1])
    vg = _script("dino-main/video_generation.py")
    vg.main(["--input_path", str(tmp_path / "in"), "--output_path", str(tmp_path / "out"), "--bs", "3"])
    frames = torch.cat([r[1] for r in rendered]).cpu().numpy()
    assert frames.shape == (5, 64, 96, 3) and len(rendered) == 2                  # passes of 3 and 2 frames
    assert sorted(os.listdir(tmp_path / "out" / "attention")) == ["attn-" + n for n in names]
    for j, n in enumerate(names):
        attnviz.save_jpeg(str(tmp_path / "one.jpg"), frames[j])
        assert (tmp_path / "out" / "attention" / ("attn-" + n)).read_bytes() == (tmp_path / "one.jpg").read_bytes(), n


def test_flow_stage_writes_image_save_bytes(enc, tmp_path, monkeypatch):
    """extract_representations.py --optical_flow on 16 synthetic frames (one pair 15 apart: the fewest the stage takes): every
    flows_*.jpg is what Image.save writes for the same colour-coded map"""
    from PIL import Image
    from sais_amd import raft
    (tmp_path / "paths").mkdir()
    with open(tmp_path / "paths" / "Custom_FlowPaths.csv", "w", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        w.writerow(["", "path1", "path2", "category", "label", "flowpath"])
        w.writerow([0, "images/vid_01/frames_00000000.jpg", "images/vid_01/frames_00000015.jpg", "vid_01", "vid_01",
                    "flows/vid_01/flows_00000000.jpg"])
    maps = []
    real = raft.flow_image_uint8_device
    monkeypatch.setattr(raft, "flow_image_uint8_device", lambda rgb: maps.append((rgb, real(rgb))) or maps[-1][1])
    monkeypatch.setattr(sys, "argv", ["extract_representations.py", "--data_path", str(tmp_path) + "/", "--data_list", "Custom",
                                      "--optical_flow", "--synthetic_frames", "16", "--raft_random_weights", "--raft_iters", "2",
                                      "--batch_size_per_gpu", "2"])
    _script("extract_representations.py").main()
    files = sorted(f for f in os.listdir(tmp_path / "flows" / "vid_01") if not f.startswith("."))
    assert files == ["flows_00000000.jpg"] and len(maps) == 1
    a = maps[0][1].cpu().numpy()
    assert a.shape == (224, 224, 3) and np.array_equal(a, raft.flow_image_uint8(maps[0][0]))      # the values of the host form
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="jpeg")
    assert (tmp_path / "flows" / "vid_01" / files[0]).read_bytes() == buf.getvalue()
