"""CPU-only: the host side of the JPEG encoder (sais_amd/jpeg_enc.py) and the numpy model of its kernels (tests/jpeg_enc_ref.py)
against Pillow + libjpeg-turbo, byte for byte."""
import ctypes

import numpy as np
import pytest

from sais_amd import _lib, jpeg_enc
from tests import jpeg_enc_ref as R

DPI = (100, 100)


@pytest.fixture(scope="module")
def model():
    """case -> (image, scan bytes of the model, statistics), computed once."""
    out = {}
    for case in R.matrix():
        H, W, kind, q, s = case
        a = R.content(kind, H, W)
        out[case] = (a,) + R.encode_scan(a, q, s)
    return out


def test_model_and_header_equal_pillow(model):
    for (H, W, kind, q, s), (a, scan, _) in model.items():
        for dpi in (None, DPI):
            assert jpeg_enc.header(H, W, q, s, dpi) + scan == R.pillow_file(a, q, s, dpi), (H, W, kind, q, s, dpi)


def test_matrix_reaches_the_hard_cases(model):
    st = [v[2] for v in model.values()]
    assert max(x["longest_run"] for x in st) >= 48 and max(x["zrl"] for x in st) >= 3        # three ZRLs in a row
    assert max(x["stuffed"] for x in st) >= 1
    assert max(x["dc_cat"] for x in st) == 11 and max(x["ac_cat"] for x in st) == 10
    assert any(x["dummy_right"] for x in st) and any(x["dummy_bottom"] for x in st) and any(x["dummy_both"] for x in st)
    assert {x["pad_bits"] for x in st} == set(range(8))
    # an even H whose 4:2:0 chroma rows do not fill their blocks: padded from the DOWNSAMPLED last row
    assert any(H % 2 == 0 and ((H + 1) // 2) % 8 != 0 and s == 2 for (H, W, kind, q, s) in model)


def test_quant_tables_equal_pillow_dqt():
    a = np.zeros((8, 8, 3), np.uint8)
    for q in range(1, 101):
        blob = R.pillow_file(a, q, 2)
        at = blob.index(b"\xff\xdb")
        got = []
        for _ in range(2):
            assert blob[at:at + 4] == b"\xff\xdb\x00\x43"
            got.append(np.frombuffer(blob[at + 5:at + 69], np.uint8))
            at += 69
        want = jpeg_enc.quant_tables(q)[:, list(jpeg_enc.ZIGZAG)]
        assert (np.stack(got) == want).all(), q
    assert (jpeg_enc.quant_tables(0) == jpeg_enc.quant_tables(1)).all() and (jpeg_enc.quant_tables(400) == 1).all()


def test_bound_covers_every_case(model):
    for (H, W, kind, q, s), (_, scan, _) in model.items():
        assert jpeg_enc.encode_bound(H, W, s) >= len(scan), (H, W, kind, q, s)
    for s in R.SUBSAMPLINGS:                      # the largest streams: saturated noise at quality 100
        a = R.content("saturated", 130, 250)
        assert jpeg_enc.encode_bound(130, 250, s) >= len(R.encode_scan(a, 100, s)[0])
    # derived from the tables: blocks x the longest block code (11 + 9 DC bits, 63 x (16 + 10) AC bits for luma; 11 + 11 and the
    # same AC bits for chroma), every byte stuffed, the padding byte and FF D9
    luma, chroma = 20 + 63 * 26, 22 + 63 * 26
    assert jpeg_enc.encode_bound(16, 16, 2) == 2 * ((4 * luma + 2 * chroma + 7) // 8 + 1) + 2
    assert jpeg_enc.encode_bound(8, 8, 0) == 2 * ((luma + 2 * chroma + 7) // 8 + 1) + 2
    assert jpeg_enc.encode_bound(17, 33, 2) == 2 * ((6 * (4 * luma + 2 * chroma) + 7) // 8 + 1) + 2


def test_refusals():
    lib = _lib.load()
    assert lib.sais_jpeg_encode_bound(0, 8, 2) == 0 and lib.sais_jpeg_encode_bound(8, 65536, 2) == 0
    assert lib.sais_jpeg_encode_bound(8, 8, 1) == 0
    assert lib.sais_jpeg_encode_workspace_bytes(0, 8, 8, 2) == 0 and lib.sais_jpeg_encode_workspace_bytes(1, 8, 8, 2) > 0
    p = jpeg_enc.SaisJpegEncParams()
    p.subsampling = 2
    for t, table in enumerate(jpeg_enc.quant_tables(75)):
        for k in range(64):
            p.q[t][k] = int(table[k])
    ptr = ctypes.c_void_p(256)                    # never dereferenced: every call below fails its argument checks first
    args = lambda n=1, h=8, w=8, ws=1 << 20, stride=4096: (ptr, n, h, w, ctypes.byref(p), ptr, ws, ptr, stride, ptr, None)
    assert lib.sais_jpeg_encode(None, 1, 8, 8, ctypes.byref(p), ptr, 1 << 20, ptr, 4096, ptr, None) == -1
    assert lib.sais_jpeg_encode(*args(n=0)) == -1 and lib.sais_jpeg_encode(*args(h=0)) == -1
    assert lib.sais_jpeg_encode(*args(w=65536)) == -1 and lib.sais_jpeg_encode(*args(ws=16)) == -1
    assert lib.sais_jpeg_encode(*args(stride=1)) == -1
    p.subsampling = 1
    assert lib.sais_jpeg_encode(*args()) == -1
    p.subsampling = 2
    p.q[1][63] = 0
    assert lib.sais_jpeg_encode(*args()) == -1
    p.q[1][63] = 256
    assert lib.sais_jpeg_encode(*args()) == -1
    # the Python layer
    with pytest.raises(_lib.SaisHipError):
        jpeg_enc.JpegEncoder("cpu")
    for kw in ({"optimize": True}, {"progressive": True}, {"grayscale": True}, {"restart_marker_blocks": 4}, {"restart_marker_rows": 1}):
        with pytest.raises(ValueError, match=next(iter(kw)).split("_")[0]):
            jpeg_enc.check_options(**kw)
    for sub in ("4:2:2", 1, "4:1:1"):
        with pytest.raises(ValueError, match="subsampling"):
            jpeg_enc.header(8, 8, 75, sub)
    with pytest.raises(ValueError):
        jpeg_enc.header(0, 8)
    with pytest.raises(ValueError):
        jpeg_enc.header(8, 8, dpi=(0, 100))
