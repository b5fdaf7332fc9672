"""Baseline-JPEG file builder (numpy, CPU, tests only): writes the files no encoder writes, for tests/test_jpeg_edges_host.py
and tests/test_jpeg_edges_gpu.py.  Input is quantised coefficients and every table and selector of the file; output is the file
and the destuffed length of every restart interval.  cases() is the matrix both test files share."""
import collections
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_enc_ref import _codes, pack_bits, stuff  # noqa: E402

from sais_amd.jpeg_enc import HUFFMAN, ZIGZAG  # noqa: E402

SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}
# (class, id) -> (counts [16], symbols): the Annex K tables Pillow writes
STD_HUFF = {(t >> 4, t & 15): (tuple(c), tuple(s)) for t, c, s in HUFFMAN}
DC_SYMBOLS = tuple(range(12))
AC_SYMBOLS = (0x00, 0xF0) + tuple(r << 4 | s for r in range(16) for s in range(1, 11))

# file bytes; destuffed bytes per interval; those bytes (u8 arrays); the (class, code length) pairs in use
Built = collections.namedtuple("Built", "data lens raw used")


def check_spec(counts):
    """What libjpeg's jpeg_make_d_derived_tbl demands of the 16 counts: after the codes of length l, code < 2^l (so the all-ones
    code of every length stays free and the Kraft sum stays below 1)."""
    assert len(counts) == 16 and all(0 <= c <= 255 for c in counts) and 0 < sum(counts) <= 256, counts
    code, kraft = 0, 0.0
    for length in range(1, 17):
        c = counts[length - 1]
        assert code + c < (1 << length), (length, counts)
        kraft += c / (1 << length)
        code = (code + c) << 1
    assert kraft < 1.0


def spec_from_lengths(symbols, lengths):
    """A Huffman spec (counts, symbols) that gives symbols[i] a code of lengths[i] bits (any order; ties keep the given order)."""
    assert len(symbols) == len(lengths) == len(set(symbols))
    order = sorted(range(len(symbols)), key=lambda i: lengths[i])
    counts = [0] * 16
    for n in lengths:
        counts[n - 1] += 1
    check_spec(counts)
    return tuple(counts), tuple(symbols[i] for i in order)


def geometry(H, W, sub):
    hs, vs = SAMPLING[sub]
    return hs, vs, -(-W // (8 * hs)), -(-H // (8 * vs))


def slot_components(sub):
    hs, vs = SAMPLING[sub]
    return (0,) * (hs * vs) + (1, 2)


def _size(v):
    return int(abs(int(v))).bit_length()


def _vbits(v, n):
    return (int(v) if v >= 0 else int(v) - 1) & ((1 << n) - 1)


def ac_ops(block):
    """The (symbol, value) list a standard encoder writes for coefficients 1..63 (zig-zag order) of one block."""
    ops, run = [], 0
    for k in range(1, 64):
        v = int(block[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            ops.append((0xF0, 0))
            run -= 16
        ops.append((run << 4 | _size(v), v))
        run = 0
    if run:
        ops.append((0x00, 0))
    return ops


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def build(H, W, blocks, sub=2, quant=None, qsel=(0, 1, 1), pq=None, huff=None, dcsel=(0, 1, 1), acsel=(0, 1, 1), sof=0xC0,
          ri=0, fill_rst=0, fill_eoi=0, extra=(), one_dht=False, raw_ac=None, eoi=True, short=()):
    """blocks: int [mcus * blocks_per_mcu, 64] in scan order, zig-zag order inside a block, DC as the value (not the difference).
    quant: {id: u16 [64] natural order}; pq: {id: 0 | 1} (default 0).  huff: {(class, id): (counts, symbols)} (default: Annex K).
    raw_ac: {block index: [(symbol, value)]} written instead of the block's standard AC codes (a ZRL past the block end, ...).
    fill_rst / fill_eoi: extra 0xFF bytes before every RSTn / before EOI.  extra: whole segments put after SOI.
    Corrupt files: eoi=False ends the file with the scan; short: the restart intervals written without their last MCU."""
    hs, vs, mcux, mcuy = geometry(H, W, sub)
    comps = slot_components(sub)
    bpm, mcus = len(comps), mcux * mcuy
    blocks = np.asarray(blocks, np.int64)
    assert blocks.shape == (mcus * bpm, 64), (blocks.shape, mcus, bpm)
    quant = quant if quant is not None else {0: np.full(64, 3), 1: np.full(64, 5)}
    huff = dict(STD_HUFF) if huff is None else dict(huff)
    pq = pq or {}
    raw_ac = raw_ac or {}
    for counts, _ in huff.values():
        check_spec(counts)
    code = {key: _codes(counts, symbols) for key, (counts, symbols) in huff.items()}
    raws, bits, lens, pred, used = [], [], [], [0, 0, 0], set()

    def flush():
        raw, _ = pack_bits(bits, lens) if bits else (np.zeros(0, np.uint8), 0)
        raws.append(raw)
        del bits[:], lens[:]

    for m in range(mcus):
        if ri and m and m % ri == 0:
            flush()
            pred = [0, 0, 0]
        if ri and m // ri in short and (m % ri == ri - 1 or m == mcus - 1):
            continue
        for s, c in enumerate(comps):
            b = m * bpm + s
            blk = blocks[b]
            diff = int(blk[0]) - pred[c]
            pred[c] = int(blk[0])
            n = _size(diff)
            assert n <= 11, diff
            cw, cl = code[(0, dcsel[c])][n]
            used.add((0, cl))
            bits.append(cw << n | _vbits(diff, n))
            lens.append(cl + n)
            for sym, v in (raw_ac[b] if b in raw_ac else ac_ops(blk)):
                n = sym & 15
                assert n <= 10 and (n == 0 or _size(v) == n), (sym, v)
                cw, cl = code[(1, acsel[c])][sym]
                used.add((1, cl))
                bits.append(cw << n | _vbits(v, n) if n else cw)
                lens.append(cl + n)
    flush()
    scan = bytearray()
    for i, raw in enumerate(raws):
        if i:
            scan += b"\xff" * fill_rst + bytes([0xFF, 0xD0 + (i - 1) % 8])
        scan += stuff(raw)[0].tobytes()
    out = bytearray(b"\xff\xd8")
    for seg in extra:
        out += seg
    for t in sorted(quant):
        q = np.asarray(quant[t], np.int64)[list(ZIGZAG)]
        assert q.min() >= 1 and q.max() <= (65535 if pq.get(t) else 255)
        body = bytes([pq.get(t, 0) << 4 | t]) + (q.astype(">u2").tobytes() if pq.get(t) else q.astype(np.uint8).tobytes())
        out += _segment(0xDB, body)
    frame = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3])
    for c in range(3):
        frame += bytes([c + 1, (hs << 4 | vs) if c == 0 else 0x11, qsel[c]])
    out += _segment(sof, frame)
    tables = [bytes([tc << 4 | th]) + bytes(counts) + bytes(symbols) for (tc, th), (counts, symbols) in sorted(huff.items())]
    if one_dht:
        out += _segment(0xC4, b"".join(tables))
    else:
        for t in tables:
            out += _segment(0xC4, t)
    if ri:
        out += _segment(0xDD, ri.to_bytes(2, "big"))
    out += _segment(0xDA, bytes([3]) + b"".join(bytes([c + 1, dcsel[c] << 4 | acsel[c]]) for c in range(3)) + bytes([0, 63, 0]))
    out += scan
    if eoi:
        out += b"\xff" * fill_eoi + b"\xff\xd9"
    return Built(bytes(out), [len(r) for r in raws], raws, used)


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


# ---- the hand-built matrix ---------------------------------------------------------------------------------------------------
def noise_blocks(H, W, sub, amp, seed, dc=60, nz=0.5):
    """Seeded coefficients: DC uniform in +-dc, AC uniform in +-amp and zero with probability 1 - nz."""
    hs, vs, mcux, mcuy = geometry(H, W, sub)
    rng = np.random.default_rng([seed, H, W, sub])
    nb = mcux * mcuy * (hs * vs + 2)
    b = rng.integers(-amp, amp + 1, (nb, 64)) * (rng.random((nb, 64)) < nz)
    b[:, 0] = rng.integers(-dc, dc + 1, nb)
    return b


# DC: category 0 on the 1-bit code, then 9, 10 and 16 bits; AC: EOB on the 1-bit code, every length of the 9-bit lookup's far
# side (10 and 16) on symbols the noise of lengths_case() uses
def _lengths_tables():
    dc = spec_from_lengths(DC_SYMBOLS, [1, 9, 9, 10, 10, 16, 16, 16, 16, 16, 16, 16])
    acl = []
    for sym in AC_SYMBOLS:
        r, s = sym >> 4, sym & 15
        acl.append(1 if sym == 0 else 9 if (r < 2 and s == 1) or sym == 0xF0 else 10 if r < 4 and s <= 2 else 16)
    ac = spec_from_lengths(AC_SYMBOLS, acl)
    return dc, ac


def _tiny_tables():
    """1-bit DC code for category 0 and a 1-bit EOB: a block of zeros is 2 bits."""
    dc = spec_from_lengths(DC_SYMBOLS, [1] + [5] * 11)
    ac = spec_from_lengths(AC_SYMBOLS, [1] + [9] * 161)
    return dc, ac


def _interval_case(length, short=()):
    """48 x 40 4:4:4, ri = 8: interval 1 has a destuffed length of exactly `length` bytes.  Free parameters: how many leading AC
    coefficients of the interval's blocks are non-zero, and one coefficient's magnitude."""
    H, W, sub, ri = 48, 40, 0, 8
    base = noise_blocks(H, W, sub, 3, 5, nz=0.3)

    def make(fill, mag):
        b = base.copy()
        seg = b[ri * 3:2 * ri * 3]
        flat = np.zeros(seg.shape[0] * 63, np.int64)
        flat[:fill] = 1 + (np.arange(fill) % 3)
        seg[:, 1:] = flat.reshape(-1, 63)
        seg[0, 1] = 1 << mag if mag < 10 else -(1 << (mag - 6))
        return build(H, W, b, sub, ri=ri, short=short)
    lo, hi = 0, ri * 3 * 63                                           # the length grows with `fill`: bisect, then search nearby
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if make(mid, 0).lens[1] <= length else (lo, mid - 1)
    for fill in range(lo, max(lo - 12, -1), -1):
        for mag in range(16):
            b = make(fill, mag)
            if b.lens[1] == length:
                return b
    raise AssertionError("no parameter reaches a destuffed length of %d" % length)


def ff_edges(b):
    """Where the 0xFF bytes of a built file's destuffed intervals sit: the counts the dense-0xFF case must reach."""
    e = dict(stuffed=0, last=0, boundary=0, pairs=0)
    for r in b.raw:
        ff = r == 0xFF
        e["stuffed"] += int(ff.sum())
        e["last"] += int(len(r) > 0 and ff[-1])                        # the last byte of an interval
        e["boundary"] += int(ff[127::128].sum() + ff[128::128].sum())   # byte 127 or 128 of a subsequence
        e["pairs"] += int((ff[:-1] & ff[1:]).sum())                    # two stuffed bytes in a row
    return e


def _dense_ff():
    """Dense 0xFF: a unary AC table (one code per length 1..16) with symbol 0x0A on 1111111111111110, so that a 1023 after a 1023
    is a run of 25 one-bits; the last block of interval 0 ends on a 1023 at k = 63, so the interval's last byte is 0xFF; fill bytes
    before RSTn and before EOI; COM and APP5 segments.  The seed is searched until every edge of ff_edges() is reached."""
    H, W, ri = 40, 48, 7
    un_syms = (0x00, 0x01, 0x02, 0x11, 0xF0, 0x03, 0x21, 0x12, 0x04, 0x22, 0x05, 0x41, 0x06, 0xDA, 0x07, 0x0A)
    unary = spec_from_lengths(un_syms, list(range(1, 17)))
    kw = dict(quant={0: np.full(64, 1), 1: np.full(64, 1)}, ri=ri, fill_rst=3, fill_eoi=2, acsel=(0, 0, 0),
              huff={(0, 0): STD_HUFF[(0, 0)], (0, 1): STD_HUFF[(0, 1)], (1, 0): unary},
              extra=(_segment(0xFE, b"built by tests/jpeg_build.py"), _segment(0xE5, b"abcd")))
    for seed in range(400):
        rng = np.random.default_rng(seed)
        b = np.zeros((6 * 5 * 3, 64), np.int64)
        b[:, 0] = rng.integers(-30, 31, len(b))
        for i in range(len(b)):                                        # at most two 1023s per block: the IDCT output stays in range
            n = int(rng.integers(0, 12))
            b[i, 3:3 + n] = rng.choice([1, -1, 2, -3], n)
            if i % 2 == 0:
                b[i, 1], b[i, 2] = 1023, 1023 if i % 4 else -1023
        b[ri * 3 - 1, 1:] = 0
        b[ri * 3 - 1, 1], b[ri * 3 - 1, 63] = 1023, 1023
        bl = build(H, W, b, 0, **kw)
        e = ff_edges(bl)
        if e["last"] and e["boundary"] and e["pairs"] and len(bl.raw[0]) > 129:
            return bl, kw
    raise AssertionError("no seed reaches every 0xFF edge")


def cases():
    """name -> (Built, keyword arguments of build() the host test checks against the parsed header).  Every case is meant to be a
    legal file that Pillow decodes; each comes with the edge it reaches, asserted in tests/test_jpeg_edges_host.py."""
    out = {}
    H, W = 40, 48

    def add(name, H, W, blocks, sub, **kw):
        out[name] = (build(H, W, blocks, sub, **kw), dict(H=H, W=W, sub=sub, **kw))

    dcl, acl = _lengths_tables()
    kw = dict(huff={(0, 0): dcl, (1, 0): acl, (0, 1): STD_HUFF[(0, 1)], (1, 1): STD_HUFF[(1, 1)]}, dcsel=(0, 1, 0), acsel=(0, 1, 0))
    b = noise_blocks(H, W, 2, 12, 1, dc=300, nz=0.2)
    b[6:18, 0] = 77                                                           # DC differences of 0: the 1-bit DC code
    add("lengths_1_9_10_16", H, W, b, 2, **kw)
    dct, act = _tiny_tables()
    zeros = np.zeros((5 * 55 * 3, 64), np.int64)
    zeros[0, 0] = 5
    zeros[7::50, 3] = 1
    add("one_bit_blocks", 40, 440, zeros, 0, huff={(0, 0): dct, (1, 0): act}, dcsel=(0, 0, 0), acsel=(0, 0, 0))
    add("sel_y1_c0", H, W, noise_blocks(H, W, 2, 8, 2), 2, dcsel=(1, 0, 0), acsel=(1, 0, 0))
    add("sel_cross", H, W, noise_blocks(H, W, 1, 8, 3), 1, dcsel=(0, 0, 1), acsel=(0, 1, 0))
    add("sel_all0", H, W, noise_blocks(H, W, 0, 8, 4), 0, dcsel=(0, 0, 0), acsel=(0, 0, 0),
        huff={(0, 0): STD_HUFF[(0, 0)], (1, 0): STD_HUFF[(1, 0)]}, one_dht=True)
    q3 = {3: np.full(64, 1), 0: np.full(64, 255), 2: np.where(np.arange(64) % 2, 1, 255)}
    b = noise_blocks(H, W, 2, 1, 5, dc=3, nz=0.03)                         # |coef x 255| summed over a block stays small
    add("quant_3_tables", H, W, b, 2, quant=q3, qsel=(3, 0, 2))
    add("sof1", H, W, noise_blocks(H, W, 2, 8, 6), 2, sof=0xC1)
    add("pq1", H, W, noise_blocks(H, W, 0, 8, 7), 0, quant={0: np.arange(1, 65) // 4 + 1, 1: np.full(64, 9)}, pq={0: 1, 1: 1})
    # extremes: DC 1023 -> -1024 -> 1023 (differences of -2047, +2047), AC +-1023, a block with all 63 AC non-zero
    b = noise_blocks(H, W, 0, 2, 8, nz=0.2)
    b[3, 0], b[6, 0], b[9, 0] = 1023, -1024, 1023
    b[12, 5], b[15, 9] = 1023, -1023
    b[18, 1:] = np.where(np.arange(63) % 2, 1, -1)
    add("extremes", H, W, b, 0, quant={0: np.full(64, 1), 1: np.full(64, 2)})
    # runs of 15, 16 and 62, and a ZRL that passes the block end (k = 51 + 16 > 64: the block closes without an EOB)
    b = noise_blocks(H, W, 2, 3, 9, nz=0.1)
    b[0, 1:], b[1, 1:], b[2, 1:], b[3, 1:] = 0, 0, 0, 0
    b[0, 16], b[1, 17], b[2, 63], b[3, 50] = 2, -3, 1, 4
    add("runs_and_zrl", H, W, b, 2, raw_ac={3: [(0xF0, 0), (0xF0, 0), (0xF0, 0), (0x13, 4), (0xF0, 0)]})
    bl, kw = _dense_ff()
    out["dense_ff"] = (bl, dict(H=H, W=W, sub=0, **kw))
    # restart shapes (48 x 40 4:4:4 = 6 x 5 MCUs; 4:2:0 = 3 x 3)
    b0 = noise_blocks(H, W, 0, 8, 11)
    add("ri_1", H, W, b0, 0, ri=1)                                            # 30 intervals: RST index wraps three times
    add("ri_not_dividing", H, W, b0, 0, ri=4)
    add("ri_row_plus_1", H, W, b0, 0, ri=7)
    add("ri_ge_mcus", H, W, noise_blocks(H, W, 2, 8, 12), 2, ri=9)
    add("ri_above_mcus", H, W, noise_blocks(H, W, 2, 8, 12), 2, ri=500)
    for n in (127, 128, 129, 256):
        bl = _interval_case(n)
        out["interval_%d" % n] = (bl, dict(H=48, W=40, sub=0, ri=8))
    # the shortest interval a legal MCU fits: three blocks of zeros at 2 bits each with the 1-bit tables = 6 bits = 1 byte
    z = np.zeros((6 * 5 * 3, 64), np.int64)
    z[0, 0] = 9
    z[0, 2] = -2
    add("interval_1_byte", H, W, z, 0, ri=1, huff={(0, 0): dct, (1, 0): act}, dcsel=(0, 0, 0), acsel=(0, 0, 0))
    return out


_CACHE = {}


def cached_cases():
    if not _CACHE:
        _CACHE.update(cases())
    return _CACHE


# ---- synchronisation bands (tests/jpeg_sync_ref.py says which band a file is in) ----------------------------------------------
BATCH_HW = (160, 192)


def shared_table_noise(seed=21):
    """160 x 192 4:4:4 noise with all three components on table pair 0: once the bit position agrees, a wrong slot decodes the same
    codewords as the right one, so a wrong guess never corrects itself and the right state crawls one subsequence per pass."""
    H, W = BATCH_HW
    return build(H, W, noise_blocks(H, W, 0, 4, seed, nz=0.7), 0, dcsel=(0, 0, 0), acsel=(0, 0, 0),
                 huff={(0, 0): STD_HUFF[(0, 0)], (1, 0): STD_HUFF[(1, 0)]}).data


def sync_cases():
    """name -> (file, band): 'decode' (P <= 20 wanted), 'fail' (P >= 256 wanted) or 'either'."""
    from test_jpeg_host import encode, frame
    rng = np.random.default_rng(0)
    return {
        "noise20_q90_444": (encode(frame(256, 256, 20), quality=90, subsampling=0), "decode"),
        "noise40_q95_420": (encode(frame(256, 256, 40), quality=95, subsampling=2), "decode"),
        # a flat 4:2:0 frame: every MCU after the first is 32 bits, the stream is periodic and a wrong phase never corrects itself;
        # 1056 x 2048 is the smallest multiple of 16 rows at this width with P >= 256 (1024 x 2048: P = 249)
        "black_420": (encode(np.zeros((1056, 2048, 3), np.uint8), quality=75, subsampling=2), "fail"),
        "shared_tables_444": (shared_table_noise(), "fail"),
        "uniform_q100_444": (encode(rng.integers(0, 256, (128, 128, 3), dtype=np.uint8), quality=100, subsampling=0), "either"),
    }


def batch_files():
    """One geometry: must-fail files first, in the middle and last among must-decode files -> (files, bands)."""
    from test_jpeg_host import encode, frame
    H, W = BATCH_HW
    good = [encode(frame(H, W, 12, seed=s), quality=q, subsampling=ss) for s, (q, ss) in enumerate(((75, 2), (90, 0), (80, 1), (85, 2)))]
    bad = [shared_table_noise(seed) for seed in (21, 22, 23)]
    files = [bad[0], good[0], good[1], bad[1], good[2], good[3], bad[2]]
    return files, ["fail", "decode", "decode", "fail", "decode", "decode", "fail"]


# ---- corrupt restart intervals ---------------------------------------------------------------------------------------------------
def split_scan(data):
    """-> (bytes before the scan data, [the bytes of each restart interval], [the RSTn marker after each but the last], the rest)."""
    import jpeg_ref
    i = start = jpeg_ref.parse(data)["scan"]
    parts, marks = [], []
    while True:
        if data[i] == 0xFF and data[i + 1] not in (0x00, 0xFF):
            parts.append(data[start:i])
            if not 0xD0 <= data[i + 1] <= 0xD7:
                return data[:jpeg_ref.parse(data)["scan"]], parts, marks, data[i:]
            marks.append(data[i:i + 2])
            i = start = i + 2
        else:
            i += 1


def geometry_of(data):
    import jpeg_ref
    hd = jpeg_ref.parse(data)
    return hd["h"], hd["w"]


def with_empty_interval(data, which):
    """The file with the entropy bytes of restart interval `which` removed (its RSTn markers stay, now adjacent)."""
    head, parts, marks, tail = split_scan(data)
    parts = list(parts)
    parts[which] = b""
    return head + b"".join(p + m for p, m in zip(parts, marks + [b""])) + tail


def corrupt_cases():
    """name -> file.  64 x 64 4:4:4 = 64 MCUs; restart interval 2 (Pillow's encoder) for the empty intervals."""
    from test_jpeg_host import encode, frame
    rst = encode(frame(64, 64, 20, seed=1), quality=90, subsampling=0, restart_marker_blocks=2)
    b = noise_blocks(40, 48, 0, 8, 31)
    return {
        "empty_first": with_empty_interval(rst, 0),
        "empty_middle": with_empty_interval(rst, 13),
        "empty_last": with_empty_interval(rst, 31),
        "one_mcu_short": build(40, 48, b, 0, ri=4, short=(2,)).data,
        "last_interval_short": build(40, 48, b, 0, ri=4, short=(7,)).data,
        # one MCU too few in an interval whose destuffed length is exactly one subsequence: its only subsequence must be `last`
        "short_on_boundary": _interval_case(128, short=(1,)).data,
        "no_marker_after_scan": build(40, 48, b, 0, ri=4, eoi=False).data,
    }


def out_of_range_file():
    """Legal coefficients whose IDCT output leaves [-512, 511]: beyond the range-limit table, where jidctint.c wraps (`& RANGE_MASK`)
    and libjpeg-turbo's SIMD IDCT saturates.  Which of the two Pillow runs depends on the host, so the GPU must not guess."""
    return build(40, 48, noise_blocks(40, 48, 0, 20, 11), 0, quant={0: np.full(64, 16), 1: np.full(64, 17)}).data
