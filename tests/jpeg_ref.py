"""CPU restatement of the baseline-JPEG decode that sais_amd/csrc/jpeg.hip runs on the GPU (tests only).

The rules are libjpeg-turbo's at Pillow's defaults: sequential Huffman decode (jdhuff.c), JDCT_ISLOW (jidctint.c,
CONST_BITS 13, PASS1_BITS 2, `& RANGE_MASK` into the range-limit table), fancy upsampling (jdsample.c h2v1 / h2v2,
box replication when the chroma plane is at most 2 samples wide), and jdcolor.c ycc_rgb_convert.  Huffman decoding is
plain Python, so this is for small images.
"""
import struct

import numpy as np

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63])


class Unsupported(Exception):
    pass


def parse(data):
    """Marker walk of a baseline / extended-sequential 3-component file -> dict; raises Unsupported otherwise."""
    if data[:2] != b'\xff\xd8':
        raise Unsupported('no SOI')
    pos, qt, ht, ri, frame = 2, {}, {}, 0, None
    while True:
        while pos < len(data) and data[pos] == 0xFF and pos + 1 < len(data) and data[pos + 1] == 0xFF:
            pos += 1
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise Unsupported('bad marker')
        m = data[pos + 1]
        seg_len = struct.unpack('>H', data[pos + 2:pos + 4])[0]
        seg = data[pos + 4:pos + 2 + seg_len]
        if seg_len < 2 or pos + 2 + seg_len > len(data):
            raise Unsupported('short segment')
        if m in (0xC0, 0xC1):
            p, h, w, nc = seg[0], *struct.unpack('>HH', seg[1:5]), seg[5]
            if p != 8 or nc != 3:
                raise Unsupported('precision / components')
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(3)]
            frame = (h, w, comps)
        elif m in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Unsupported('SOF%d' % (m - 0xC0))
        elif m == 0xC4:
            o = 0
            while o < len(seg):
                tc, th = seg[o] >> 4, seg[o] & 15
                counts = list(seg[o + 1:o + 17])
                vals = list(seg[o + 17:o + 17 + sum(counts)])
                ht[(tc, th)] = (counts, vals)
                o += 17 + sum(counts)
        elif m == 0xDB:
            o = 0
            while o < len(seg):
                pq, tq = seg[o] >> 4, seg[o] & 15
                if pq:
                    q = np.frombuffer(seg[o + 1:o + 129], '>u2').astype(np.int64)
                    o += 129
                else:
                    q = np.frombuffer(seg[o + 1:o + 65], np.uint8).astype(np.int64)
                    o += 65
                nat = np.zeros(64, np.int64)
                nat[ZIGZAG] = q
                qt[tq] = nat
        elif m == 0xDD:
            ri = struct.unpack('>H', seg[:2])[0]
        elif m == 0xDA:
            ns = seg[0]
            sel = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
            if frame is None or ns != 3:
                raise Unsupported('scan')
            h, w, comps = frame
            if [c[0] for c in comps] != [s[0] for s in sel]:
                raise Unsupported('scan order')
            return dict(h=h, w=w, comps=comps, sel=sel, qt=qt, ht=ht, ri=ri, scan=pos + 2 + seg_len)
        elif m == 0xD9:
            raise Unsupported('EOI before SOS')
        pos += 2 + seg_len


class _Bits:
    def __init__(self, data, pos):
        self.d, self.p, self.acc, self.n = data, pos, 0, 0

    def _fill(self):
        b = 0
        if self.p < len(self.d):
            b = self.d[self.p]
            if b == 0xFF:
                nxt = self.d[self.p + 1] if self.p + 1 < len(self.d) else 0xD9
                if nxt == 0:
                    self.p += 2
                else:
                    b = 0                       # a marker: zeros from here on (libjpeg's behaviour)
            else:
                self.p += 1
        self.acc = (self.acc << 8) | b
        self.n += 8

    def bits(self, k):
        while self.n < k:
            self._fill()
        self.n -= k
        return (self.acc >> self.n) & ((1 << k) - 1)

    def restart(self):
        self.acc, self.n = 0, 0
        while self.p + 1 < len(self.d) and not (self.d[self.p] == 0xFF and 0xD0 <= self.d[self.p + 1] <= 0xD7):
            self.p += 1
        self.p += 2


def _huff(counts, vals):
    table, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            table[(ln, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _decode_sym(br, table):
    code = 0
    for ln in range(1, 17):
        code = (code << 1) | br.bits(1)
        if (ln, code) in table:
            return table[(ln, code)]
    raise ValueError('bad Huffman code')


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def coefficients(data, hdr=None):
    """Entropy decode -> per component int64 [bh, bw, 64] (natural order, DC predicted), padded block grids."""
    hd = hdr or parse(data)
    h, w, comps = hd['h'], hd['w'], hd['comps']
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    coef = [np.zeros((mcuy * c[2], mcux * c[1], 64), np.int64) for c in comps]
    dct = [_huff(*hd['ht'][(0, s[1])]) for s in hd['sel']]
    act = [_huff(*hd['ht'][(1, s[2])]) for s in hd['sel']]
    br, pred, ri = _Bits(data, hd['scan']), [0, 0, 0], hd['ri']
    for m in range(mcux * mcuy):
        if ri and m and m % ri == 0:
            br.restart()
            pred = [0, 0, 0]
        my, mx = divmod(m, mcux)
        for ci, (_, hs, vs, _) in enumerate(comps):
            for by in range(vs):
                for bx in range(hs):
                    blk = coef[ci][my * vs + by, mx * hs + bx]
                    s = _decode_sym(br, dct[ci])
                    pred[ci] += _extend(br.bits(s), s) if s else 0
                    blk[0] = np.int16(pred[ci])
                    k = 1
                    while k < 64:
                        rs = _decode_sym(br, act[ci])
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            if k > 63:
                                raise ValueError('run past 63')
                            blk[ZIGZAG[k]] = np.int16(_extend(br.bits(s), s))
                            k += 1
                        elif r == 15:
                            k += 16
                        else:
                            break
    return coef


C = dict(c0=2446, c1=3196, c2=4433, c3=6270, c4=7373, c5=9633, c6=12299, c7=15137, c8=16069, c9=16819, c10=20995,
         c11=25172)


def _idct_1d(x0, x1, x2, x3, x4, x5, x6, x7, first):
    z2, z3 = x2, x6
    z1 = (z2 + z3) * C['c2']
    tmp2 = z1 - z3 * C['c7']
    tmp3 = z1 + z2 * C['c3']
    tmp0 = (x0 + x4) << 13
    tmp1 = (x0 - x4) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = x7, x5, x3, x1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * C['c5']
    t0, t1, t2, t3 = t0 * C['c0'], t1 * C['c9'], t2 * C['c11'], t3 * C['c6']
    z1, z2, z3, z4 = -z1 * C['c4'], -z2 * C['c10'], -z3 * C['c8'] + z5, -z4 * C['c1'] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    n = 11 if first else 18
    d = lambda v: (v + (1 << (n - 1))) >> n  # noqa: E731
    return [d(t10 + t3), d(t11 + t2), d(t12 + t1), d(t13 + t0), d(t13 - t0), d(t12 - t1), d(t11 - t2), d(t10 - t3)]


def range_limit_idct(v):
    x = v & 1023
    return np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896)))


def idct_islow(coef, q):
    """coef int64 [..., 64] natural order, q [64] -> uint8 [..., 8, 8] (jpeg_idct_islow, vectorised over blocks)."""
    d = (coef * q).reshape(coef.shape[:-1] + (8, 8))
    cols = _idct_1d(*[d[..., r, :] for r in range(8)], first=True)          # pass 1: columns (rows of the 8x8 = r)
    ws = np.stack(cols, axis=-2)                                             # [..., 8 rows, 8 cols]
    rows = _idct_1d(*[ws[..., :, c] for c in range(8)], first=False)
    out = np.stack(rows, axis=-1)
    return range_limit_idct(out).astype(np.uint8)


def _plane(blocks, q):
    px = idct_islow(blocks, q)                                               # [bh, bw, 8, 8]
    bh, bw = blocks.shape[:2]
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8).astype(np.int64)


def _up_h(p, dw):
    if dw <= 2:
        return np.repeat(p, 2, axis=1)
    prev = np.concatenate([p[:, :1], p[:, :-1]], 1)
    nxt = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + prev + 1) >> 2
    out[:, 1::2] = (3 * p + nxt + 2) >> 2
    return out


def _up_hv(p, dw):
    if dw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    above = np.concatenate([p[:1], p[:-1]], 0)
    below = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    for r, far in ((0, above), (1, below)):
        cs = 3 * p + far
        last = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
        nxt = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        out[r::2, 0::2] = (3 * cs + last + 8) >> 4
        out[r::2, 1::2] = (3 * cs + nxt + 7) >> 4
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc_to_rgb(y, cb, cr):
    x = np.arange(256, dtype=np.int64) - 128
    cr_r = (_fix(1.40200) * x + 32768) >> 16
    cb_b = (_fix(1.77200) * x + 32768) >> 16
    cr_g = -_fix(0.71414) * x
    cb_g = -_fix(0.34414) * x + 32768
    r = y + cr_r[cr]
    g = y + ((cb_g[cb] + cr_g[cr]) >> 16)
    b = y + cb_b[cb]
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    """bytes of a supported file -> uint8 [H, W, 3], meant to equal np.asarray(Image.open(f)) bit for bit."""
    hd = parse(data)
    h, w, comps = hd['h'], hd['w'], hd['comps']
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    coef = coefficients(data, hd)
    planes = []
    for ci, (_, hs, vs, tq) in enumerate(comps):
        p = _plane(coef[ci], hd['qt'][tq])
        dh, dw = -(-h * vs // vmax), -(-w * hs // hmax)
        p = p[:dh, :dw]
        if (hs, vs) != (hmax, vmax):
            if hmax == 2 * hs and vmax == vs:
                p = _up_h(p, dw)
            elif hmax == 2 * hs and vmax == 2 * vs:
                p = _up_hv(p, dw)
            else:
                raise Unsupported('sampling')
        planes.append(p[:h, :w])
    return ycc_to_rgb(*planes)
