"""Numpy restatement of `img.thumbnail((imsize, imsize), Image.LANCZOS)` on a plain RGB `Image` (no draft mode: the image was
converted first), the reference of sais_amd/csrc/thumbnail.hip and of sais_amd.imgfolder.thumbnail_geometry:

  size rule   Image.thumbnail's preserve_aspect_ratio / round_aspect; (x, y) >= (W, H) leaves the image untouched
  factors     Image.resize with reducing_gap = 2.0: int(W / x / 2.0) or 1, int(H / y / 2.0) or 1
  reduce      Image.reduce / Reduce.c: every output pixel is ((sum + n / 2) * multiplier(n)) >> 24 over its n source pixels,
              the block clipped at the right and bottom edge; multiplier(n) = (UINT32)(2^32 as float / (256 * n)), a FLOAT
              division (division_UINT32).  The special-cased factor pairs of Reduce.c (1xN, Nx1, 2x2 ... 5x5) shift instead
              of multiplying where n is a power of two, which is the same number: the multiplier is then exact and the
              product stays below 2^32
  rows        Resample.c precompute_coeffs + normalize_coeffs_8bpc with a box [0, in1): Lanczos-3 from math.sin in double.
              in1 is W / fx ROUNDED TO A C FLOAT: Image.resize hands the box to _imaging.c, which parses it with "(ffff)"
  passes      ImagingResampleInner: horizontal, rounded and clipped to uint8, then vertical; a pass whose axis keeps its
              size with a whole box is skipped
  order       Image.resize ends with a branch for tall, narrow images: where the (reduced) image is more than 100 times as
              high as wide and the output is lower than it, the VERTICAL pass runs first (a call of its own, its result
              stored as uint8), then the horizontal one (vertical_first).  sais_thumbnail has no such order: the library
              refuses that geometry and the loader routes it to Pillow
tests/test_thumbnail_host.py holds every step against Pillow bit for bit."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

# (W, H, imsize): tall, narrow images that take Image.resize's vertical-first branch (the last one without a reduce)
TALL = [(3, 1980, 431), (16, 2000, 700), (8, 1000, 300), (4, 600, 500), (2, 250, 64)]

# (W, H, imsize): the geometry list of the thumbnail tests
GEOMETRIES = [(12, 9, 16), (63, 47, 16), (63, 16, 16), (67, 45, 16), (100, 7, 24), (40, 30, 10), (255, 3, 16), (130, 97, 8),
              (97, 130, 8), (17, 1, 16), (1, 17, 16), (31, 33, 32), (33, 31, 32), (64, 64, 16), (1023, 767, 224)]


def make_image(w, h, seed=0):
    """uint8 [h, w, 3]: smooth gradients plus noise, so that neighbouring taps differ and clipping happens."""
    rng = np.random.default_rng(seed * 1000003 + w * 1009 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 7) % 256], -1)
    noise = rng.integers(-90, 91, size=(h, w, 3))
    return np.clip(base + noise, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ geometry
def _round_aspect(number, key):
    return max(min(math.floor(number), math.ceil(number), key=key), 1)


def thumbnail_size(w, h, imsize):
    """(x, y) of Image.thumbnail((imsize, imsize)), or None where the image is left untouched."""
    x = y = int(math.floor(imsize))
    if x >= w and y >= h:
        return None
    aspect = w / h
    if x / y >= aspect:
        x = _round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = _round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def geometry(w, h, imsize):
    """None (untouched) or ((x, y), (fx, fy))."""
    size = thumbnail_size(w, h, imsize)
    if size is None:
        return None
    x, y = size
    return (x, y), (int(w / x / 2.0) or 1, int(h / y / 2.0) or 1)


# ------------------------------------------------------------------------------------------------ reduce
def multiplier(n):
    """Reduce.c division_UINT32(n, 8): float, not double."""
    n = np.asarray(n)
    return (np.float32(4294967296.0) / (n.astype(np.uint32) * np.uint32(256)).astype(np.float32)).astype(np.uint32)


def reduce(a, fx, fy):
    """uint8 [H, W, C] -> uint8 [ceil(H / fy), ceil(W / fx), C] = Image.reduce((fx, fy))."""
    h, w = a.shape[:2]
    ys, xs = np.arange(0, h, fy), np.arange(0, w, fx)
    s = np.add.reduceat(np.add.reduceat(a.astype(np.uint64), ys, axis=0), xs, axis=1)
    n = np.minimum(fy, h - ys)[:, None] * np.minimum(fx, w - xs)[None, :]
    ss = s + (n // 2)[:, :, None].astype(np.uint64)
    prod = (ss * multiplier(n)[:, :, None].astype(np.uint64)) & np.uint64(0xFFFFFFFF)          # UINT32 arithmetic
    return ((prod >> np.uint64(24)) & np.uint64(0xFF)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ coefficient rows
def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def lanczos_rows(in_size, in1, out_size):
    """precompute_coeffs(in_size, 0, in1, out_size, LANCZOS) + normalize_coeffs_8bpc: (bounds int [out][2] = first input
    index, tap count; coef int [out][ksize])."""
    scale = in1 / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        k = [lanczos((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in k:
            ww += v
        for x in range(n):
            v = k[x] / ww if ww != 0.0 else k[x]
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = xmin, n
    return bounds, coef


def _pass_axis0(a, bounds, coef):
    out = np.empty((len(bounds),) + a.shape[1:], np.uint8)
    a = a.astype(np.int64)
    for i, (lo, n) in enumerate(bounds):
        k = coef[i, :n].astype(np.int64).reshape((n,) + (1,) * (a.ndim - 1))
        acc = (a[lo:lo + n] * k).sum(0) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def needs_pass(in_size, in1, out_size):
    """ImagingResampleInner: out != in, or the box is not the whole axis."""
    return out_size != in_size or in1 != in_size


def vertical_first(rw, rh, out_h):
    """The last branch of Image.resize, on the size of the image after the reduce: `self.size[1] > self.size[0] * 100 and
    size[1] < self.size[1]`."""
    return rh > rw * 100 and out_h < rh


def resample(a, size, box_end):
    """uint8 [h, w, 3] -> [y, x, 3] = Image.resize's tail on the reduced image: resize((x, y), LANCZOS, box=(0, 0, box_end[0],
    box_end[1])) with pass skipping, horizontal pass first; for a tall, narrow image (vertical_first) the vertical pass first."""
    (x, y), (bx, by) = size, (float(np.float32(v)) for v in box_end)           # _imaging.c _resize parses the box as C floats
    if vertical_first(a.shape[1], a.shape[0], y):
        a = _pass_axis0(a, *lanczos_rows(a.shape[0], by, y))                   # y < rh: this pass is never skipped
        if needs_pass(a.shape[1], bx, x):
            a = _pass_axis0(a.transpose(1, 0, 2), *lanczos_rows(a.shape[1], bx, x)).transpose(1, 0, 2)
        return np.ascontiguousarray(a)
    if needs_pass(a.shape[1], bx, x):
        a = _pass_axis0(a.transpose(1, 0, 2), *lanczos_rows(a.shape[1], bx, x)).transpose(1, 0, 2)
    if needs_pass(a.shape[0], by, y):
        a = _pass_axis0(a, *lanczos_rows(a.shape[0], by, y))
    return np.ascontiguousarray(a)


def thumbnail_u8(img, imsize):
    """uint8 [y, x, 3] of img.thumbnail((imsize, imsize), LANCZOS); img uint8 [H, W, 3]."""
    h, w = img.shape[:2]
    g = geometry(w, h, imsize)
    if g is None:
        return img
    (x, y), (fx, fy) = g
    a = reduce(img, fx, fy) if fx > 1 or fy > 1 else img
    return resample(a, (x, y), (w / fx, h / fy))


def normalize_table():
    a = np.arange(256, dtype=np.float32) / np.float32(255.0)
    return np.stack([(a - np.float32(MEAN[c])) / np.float32(STD[c]) for c in range(3)]).astype(np.float32)


def to_tensor(u8):
    """ToTensor + Normalize of a uint8 [h, w, 3] image: float32 [3, h, w]."""
    a = u8.astype(np.float32) / 255.0
    a = (a - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    return np.ascontiguousarray(a.transpose(2, 0, 1))
