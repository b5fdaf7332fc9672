"""GPU: sais_amd.jpeg.JpegDecoder equals np.asarray(Image.open(f)) bit for bit, falls back to Pillow per file, and feeds
frame_batches() of the feature-extraction stage."""
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_jpeg_host import encode, frame, pillow  # noqa: E402
from test_preprocess import SIZES  # noqa: E402

gpu = pytest.mark.gpu


def check(dec, blobs, expect_gpu=None):
    before = dict(dec.stats)
    out = dec.decode(blobs).cpu().numpy()
    for i, b in enumerate(blobs):
        assert np.array_equal(out[i], pillow(b)), i
    if expect_gpu is not None:
        assert dec.stats["gpu"] - before["gpu"] == expect_gpu, dec.stats
    return out


@gpu
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("ss", [0, 1, 2])
def test_decode_matches_pillow(hw, ss):
    from sais_amd.jpeg import JpegDecoder
    dec = JpegDecoder("cuda:0")
    blobs = [encode(frame(*hw, 12, seed=s), quality=q, subsampling=ss) for s, q in enumerate((75, 95))]
    check(dec, blobs, expect_gpu=2)


@gpu
def test_optimised_restart_and_mixed_tables():
    from sais_amd.jpeg import JpegDecoder
    dec = JpegDecoder("cuda:0")
    h, w = 231, 517
    blobs = [encode(frame(h, w, 15, seed=1), quality=90, subsampling=2, optimize=True),
             encode(frame(h, w, 15, seed=2), quality=60, subsampling=0, restart_marker_blocks=4),
             encode(frame(h, w, 15, seed=3), quality=97, subsampling=1, restart_marker_rows=1),
             encode(frame(h, w, 120, seed=4), quality=100, subsampling=2, optimize=True, restart_marker_blocks=7),
             encode(frame(h, w, 5, seed=5), quality=30, subsampling=2)]
    check(dec, blobs, expect_gpu=len(blobs))


@gpu
@pytest.mark.parametrize("n", [1, 256])
def test_batch_sizes(n):
    from sais_amd.jpeg import JpegDecoder
    dec = JpegDecoder("cuda:0")
    base = frame(720, 1280, 10)
    rng = np.random.default_rng(3)
    blobs = []
    for i in range(n):
        a = np.roll(base, 7 * i, axis=1)
        blobs.append(encode(a, quality=int(rng.integers(70, 96)), subsampling=2, optimize=bool(i % 3 == 0)))
    check(dec, blobs, expect_gpu=n)


@gpu
def test_mixed_batch_falls_back_per_file():
    from sais_amd.jpeg import JpegDecoder, JpegModeError
    dec = JpegDecoder("cuda:0")
    a = frame(97, 133, 10)
    good = [encode(a, quality=80), encode(a[::-1].copy(), quality=90, subsampling=0)]
    prog = encode(a, quality=80, progressive=True)
    check(dec, good[:1] + [prog] + good[1:], expect_gpu=2)
    assert dec.stats["unsupported"] == 1
    gray = encode(a[..., 0], quality=80)
    with pytest.raises(JpegModeError):
        dec.decode(good + [gray])


@gpu
def test_corrupt_scans_fall_back_then_valid_batch_decodes():
    from sais_amd.jpeg import JpegDecoder
    dec = JpegDecoder("cuda:0")
    h, w = 224, 224
    d = encode(frame(h, w, 20), quality=90)
    rst = encode(frame(h, w, 20, seed=1), quality=90, restart_marker_blocks=2)
    sos = d.find(b'\xff\xda') + 14
    truncated = d[:sos + (len(d) - sos) // 2] + b'\xff\xd9'
    rng = np.random.default_rng(11)
    noisy = bytearray(d)
    noisy[sos + 100:sos + 400] = rng.integers(0, 255, 300, dtype=np.uint8).tobytes()
    bad_rst = bytearray(rst)
    i = bad_rst.find(b'\xff\xd1', rst.find(b'\xff\xda'))
    bad_rst[i + 1] = 0xD5                                      # RST1 -> RST5: out of sequence
    blobs = [truncated, bytes(noisy), bytes(bad_rst)]
    expected = []
    for b in blobs:
        try:
            expected.append(pillow(b))
        except OSError:
            expected.append(None)
    if any(e is None for e in expected):                       # Pillow itself refuses a file: so does decode()
        with pytest.raises(OSError):
            dec.decode(blobs)
        blobs = [b for b, e in zip(blobs, expected) if e is not None]
    if blobs:
        out = dec.decode(blobs).cpu().numpy()
        for o, b in zip(out, blobs):
            assert np.array_equal(o, pillow(b))
        assert (dec.last_status != 0).all(), dec.last_status
        assert dec.stats["failed"] >= len(blobs)
    check(dec, [d, rst], expect_gpu=2)


def with_quant(data, value):
    """The file with every entry of every 8-bit DQT table set to `value`."""
    d, pos = bytearray(data), 2
    while d[pos + 1] != 0xDA:
        n = int.from_bytes(d[pos + 2:pos + 4], 'big')
        if d[pos + 1] == 0xDB:
            o = pos + 4
            while o < pos + 2 + n:
                assert d[o] >> 4 == 0
                d[o + 1:o + 65] = bytes([value]) * 64
                o += 65
        pos += 2 + n
    return bytes(d)


@gpu
def test_dequantised_values_beyond_int16_fall_back():
    """q100 coefficients rescaled by quantisers of 255: |coef * q| leaves int16, where Pillow's result is not the C
    arithmetic of jidctint.c (tests/jpeg_ref.py differs from Pillow on this file); it goes to Pillow (status
    SAIS_JPEG_E_RANGE) and the batch still equals Pillow.  One MCU per restart interval keeps the sync passes out of it."""
    from sais_amd.jpeg import JpegDecoder
    dec = JpegDecoder("cuda:0")
    ok = encode(frame(61, 45, 20), quality=90)
    big = with_quant(encode(frame(61, 45, 20, seed=3), quality=100, restart_marker_blocks=1), 255)
    check(dec, [ok, big], expect_gpu=1)
    assert list(dec.last_status) == [0, 32], dec.last_status


@gpu
def test_frame_batches_through_the_gpu_decoder(tmp_path, capsys):
    from SAIS.scripts.extract_representations import MEAN, STD, frame_batches
    from sais_amd.preprocess import FramePreprocessor
    files = []
    for i in range(5):
        files.append(encode(frame(120, 160, 10, seed=i), quality=85))
    files.append(encode(frame(120, 160, 10, seed=9), quality=85, progressive=True))
    for i in range(3):
        files.append(encode(frame(90, 200, 10, seed=20 + i), quality=80, subsampling=0))
    for i, b in enumerate(files):
        (tmp_path / f'frames_{i:08d}.jpg').write_bytes(b)
    dev = torch.device('cuda:0')
    got = torch.cat([t.cpu() for t in frame_batches(str(tmp_path), dev, chunk=4)])
    log = capsys.readouterr().out
    assert '8 decoded on the GPU, 1 on the host' in log, log
    want = []
    for b in files:
        a = pillow(b)
        want.append(FramePreprocessor(a.shape[0], a.shape[1], 0.8, 0.8, MEAN, STD, device=dev)(a[None]).cpu())
    assert torch.equal(got, torch.cat(want))


@gpu
def test_grayscale_frame_raises_frame_error(tmp_path):
    from SAIS.scripts.extract_representations import FrameError, frame_batches
    (tmp_path / 'frames_00000000.jpg').write_bytes(encode(frame(64, 64, 5), quality=80))
    (tmp_path / 'frames_00000001.jpg').write_bytes(encode(frame(64, 64, 5)[..., 0], quality=80))
    with pytest.raises(FrameError):
        list(frame_batches(str(tmp_path), torch.device('cuda:0')))


def test_cpu_device_raises():
    from sais_amd import _lib
    from sais_amd.jpeg import JpegDecoder
    with pytest.raises(_lib.SaisHipError):
        JpegDecoder("cpu")
