"""CPU-only: the numpy restatement of the JPEG decode (tests/jpeg_ref.py) equals Pillow bit for bit, and the host parser
of the GPU decoder (sais_jpeg_parse) agrees with Pillow and rejects what it must."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref  # noqa: E402


def frame(h, w, noise, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, noise, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a).save(b, 'JPEG', **kw)
    return b.getvalue()


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def insert_before_sof(data, seg):
    i = data.find(b'\xff\xc0')
    return data[:i] + seg + data[i:]


def move_dht_after_sof(data):
    """Rewrite the file so that every DHT segment follows SOF0 (still before SOS)."""
    pos, segs, out_head = 2, [], [data[:2]]
    while True:
        m = data[pos + 1]
        n = int.from_bytes(data[pos + 2:pos + 4], 'big')
        seg = data[pos:pos + 2 + n]
        if m == 0xDA:
            break
        segs.append((m, seg))
        pos += 2 + n
    dht = [s for m, s in segs if m == 0xC4]
    rest = [s for m, s in segs if m != 0xC4]
    out_head += rest + dht
    return b''.join(out_head) + data[pos:]


SIZES = [(1, 1), (8, 8), (17, 33), (61, 45), (97, 133)]
QUAL = [(50, 10), (92, 20), (100, 120)]


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("ss", [0, 1, 2])
def test_reference_equals_pillow(hw, ss):
    for q, noise in QUAL:
        for kw in ({}, {'optimize': True}, {'restart_marker_blocks': 4}, {'restart_marker_rows': 1}):
            d = encode(frame(*hw, noise), quality=q, subsampling=ss, **kw)
            assert np.array_equal(jpeg_ref.decode(d), pillow(d)), (hw, ss, q, kw)


def test_reference_equals_pillow_on_rearranged_markers():
    d = encode(frame(61, 45, 20), quality=85, subsampling=2)
    com = b'\xff\xfe\x00\x07hello'
    app = b'\xff\xe5\x00\x06abcd'
    for v in (insert_before_sof(d, com + app), move_dht_after_sof(d), d + b'\x00\x01trailing'):
        assert np.array_equal(jpeg_ref.decode(v), pillow(v))


def lib():
    import __graft_entry__ as ge
    from sais_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_parse_agrees_with_pillow():
    lib()
    from sais_amd import jpeg
    for (h, w) in [(17, 33), (97, 133), (720, 1280)]:
        for ss, samp in ((0, (1, 1)), (1, (2, 1)), (2, (2, 2))):
            for kw in ({}, {'restart_marker_blocks': 4}):
                d = encode(frame(h, w, 10), quality=75, subsampling=ss, **kw)
                rc, hd = jpeg.parse_rc(d)
                assert rc == 0
                im = Image.open(io.BytesIO(d))
                assert (hd.width, hd.height) == im.size
                assert (hd.hsamp, hd.vsamp) == samp and im.layer[0][1:3] == samp and im.layer[1][1:3] == (1, 1)
                for c in range(3):
                    assert hd.qsel[c] == im.layer[c][3]
                for t, table in im.quantization.items():             # Pillow lists them in natural order
                    assert list(hd.quant[t]) == list(table)
                mcux, mcuy = -(-w // (8 * samp[0])), -(-h // (8 * samp[1]))
                assert hd.mcu_count == mcux * mcuy
                ri = hd.restart_interval
                assert hd.segments == (-(-hd.mcu_count // ri) if ri else 1)
                assert hd.scan_offset + hd.scan_bytes == len(d) and d[hd.scan_offset - 14:hd.scan_offset - 12] == b'\xff\xda'


def test_parse_classifies_unsupported_files():
    lib()
    from sais_amd import jpeg
    a = frame(40, 56, 10)
    prog = encode(a, quality=80, progressive=True)
    gray = encode(a[..., 0], quality=80)
    b = io.BytesIO()
    Image.fromarray(a).convert('CMYK').save(b, 'JPEG', quality=80)
    cmyk = b.getvalue()
    for d in (prog, gray, cmyk):
        assert jpeg.parse_rc(d)[0] == jpeg.UNSUPPORTED
        assert jpeg.parse_header(d) is None


def test_parse_rejects_truncated_and_garbage_headers():
    l = lib()
    from sais_amd import jpeg
    d = encode(frame(33, 47, 10), quality=80)
    sos = d.find(b'\xff\xda')
    for cut in (0, 1, 2, 3, 10, 25, sos - 3, sos + 5):
        assert jpeg.parse_rc(d[:cut])[0] < 0, cut
    assert jpeg.parse_rc(b'garbage' * 10)[0] < 0
    assert l.sais_jpeg_parse(None, 10, None) == -1
    rng = np.random.default_rng(7)
    head = bytearray(d[:sos + 14])
    for _ in range(3000):                                      # seeded header mutations: host only, never a crash
        m = bytearray(head)
        for _ in range(int(rng.integers(1, 6))):
            m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 256))
        rc, h = jpeg.parse_rc(bytes(m) + d[sos + 14:])
        assert rc in (0, -1, jpeg.UNSUPPORTED)
        if rc == 0:
            assert h.scan_offset + h.scan_bytes == len(d) and h.hsamp in (1, 2) and h.vsamp in (1, 2)


def test_decode_entry_rejects_bad_arguments_without_a_gpu():
    l = lib()
    from sais_amd import jpeg
    bt = jpeg.SaisJpegBatch(1, 8, 8, 1, 100, 100)
    p = ctypes.c_void_p(256)
    assert l.sais_jpeg_decode(None, p, p, p, 1 << 30, p, p, None) == -1
    assert l.sais_jpeg_decode(ctypes.byref(bt), None, p, p, 1 << 30, p, p, None) == -1
    assert l.sais_jpeg_decode(ctypes.byref(bt), p, p, p, 16, p, p, None) == -1           # workspace too small
    bad = jpeg.SaisJpegBatch(0, 8, 8, 1, 100, 100)
    assert l.sais_jpeg_decode(ctypes.byref(bad), p, p, p, 1 << 30, p, p, None) == -1
    bad = jpeg.SaisJpegBatch(2, 8, 8, 1, 100, 100)                                       # fewer segments than images
    assert l.sais_jpeg_decode(ctypes.byref(bad), p, p, p, 1 << 30, p, p, None) == -1
    assert l.sais_jpeg_workspace_bytes(0, 8, 8, 100, 1) == 0
    assert l.sais_jpeg_workspace_bytes(256, 720, 1280, 256 * 120000, 256) > 256 * 720 * 1280 * 3


def test_header_struct_matches_the_c_layout():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sais_hip.h')).read()
    from sais_amd import jpeg
    assert 'SaisJpegHeader' in src
    assert jpeg.SaisJpegHeader.scan_offset.offset == 64 and jpeg.SaisJpegHeader.quant.offset == 80
    assert ctypes.sizeof(jpeg.SaisJpegBatch) == 32


def overfill_dht(data, tc, th, counts):
    """The file with the 16 code-length counts of DHT table (tc, th) replaced (the total must stay the same)."""
    d, pos = bytearray(data), 2
    while d[pos + 1] != 0xDA:
        n = int.from_bytes(d[pos + 2:pos + 4], 'big')
        if d[pos + 1] == 0xC4:
            o, end = pos + 4, pos + 2 + n
            while o < end:
                total = sum(d[o + 1:o + 17])
                if d[o] == (tc << 4 | th):
                    assert sum(counts) == total
                    d[o + 1:o + 17] = bytes(counts)
                o += 17 + total
        pos += 2 + n
    return bytes(d)


def test_parse_rejects_overfilled_huffman_tables():
    """Counts that put more codes at a short length than it has (still well formed by length) are a bogus table for
    libjpeg; the parser must say so before it builds the lookup (sais_jpeg_parse used to write past its tables)."""
    lib()
    from sais_amd import jpeg
    d = encode(frame(64, 64, 30), quality=95)
    for tc, th in ((1, 1), (1, 0), (0, 0)):
        rc, _ = jpeg.parse_rc(d)
        assert rc == 0
        total = None
        pos = 2
        while d[pos + 1] != 0xDA:                              # the table's symbol count
            n = int.from_bytes(d[pos + 2:pos + 4], 'big')
            if d[pos + 1] == 0xC4:
                o = pos + 4
                while o < pos + 2 + n:
                    t = sum(d[o + 1:o + 17])
                    if d[o] == (tc << 4 | th):
                        total = t
                    o += 17 + t
            pos += 2 + n
        cases = [[total] + [0] * 15, [total - 2, 2] + [0] * 14, [0, 0, total] + [0] * 13]
        if total > 128:                                        # 7-bit codes: the lookup is filled 4 entries per code
            cases.append([0] * 6 + [total] + [0] * 9)
        for counts in cases:
            bad = overfill_dht(d, tc, th, counts)
            assert jpeg.parse_rc(bad)[0] in (-1, jpeg.UNSUPPORTED), (tc, th, counts)
            with pytest.raises(OSError):                           # Pillow refuses the same file
                pillow(bad)
