"""Numpy restatement of the image-folder transforms (sais_amd/csrc/imgfolder.hip), as Pillow computes them: crop a box,
resample it to rw x rh with the 8-bit ImagingResample of Resample.c (bilinear or bicubic), keep the out_w x out_h window at
(win_left, win_top), mirror it, ToTensor + Normalize.  Only the output indices of the window are evaluated, and no pass is
skipped: a pass that changes nothing has the identity as its coefficient rows.  tests/test_imgfolder_host.py holds every
function here against Pillow bit for bit; the GPU tests hold the kernel against the Pillow datasets.

EVAL_SIZES, TRAIN_BOXES and SQUARE_SIZES are the geometries both test files use."""
import numpy as np

PRECISION_BITS = 32 - 8 - 2
BILINEAR, BICUBIC = 0, 1

# (w, h) of the eval transform (Resize(256, bicubic) + CenterCrop(224))
EVAL_SIZES = [(20, 31), (300, 500), (500, 375), (256, 300), (640, 256), (1200, 900), (64, 700), (1, 1), (257, 255)]
# ((w, h), box) of the train transform (box -> 224 x 224, bilinear): two corner boxes of a few pixels, a large interior box
TRAIN_BOXES = [((300, 200), (0, 0, 3, 2)), ((300, 200), (297, 198, 300, 200)), ((300, 200), (21, 17, 263, 181))]
# ((w, h), imsize) of the copy-detection transform (whole image -> imsize x imsize, bicubic)
SQUARE_SIZES = [((333, 211), 320)]


def bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def coefficients(in_size, out_size, filt, first, count):
    """precompute_coeffs + normalize_coeffs_8bpc for the output indices first .. first + count - 1 of an axis of in_size
    samples resampled to out_size: (bounds [count][2] = first input index, tap count; coef [count][ksize])."""
    fn, support = (bicubic, 2.0) if filt == BICUBIC else (bilinear, 1.0)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = support * fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((count, 2), np.int64)
    coef = np.zeros((count, ksize), np.int64)
    for i in range(count):
        c = (first + i + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - c + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            coef[i, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[i] = xmin, n
    return bounds, coef


def _resample_axis0(a, out_size, filt, first, count):
    """a: uint8 [in, ...] -> uint8 [count, ...]: output rows first .. first + count - 1 of the axis resampled to out_size."""
    bounds, coef = coefficients(a.shape[0], out_size, filt, first, count)
    out = np.empty((count,) + a.shape[1:], np.uint8)
    a = a.astype(np.int64)
    for i in range(count):
        lo, n = bounds[i]
        k = coef[i, :n].reshape((n,) + (1,) * (a.ndim - 1))
        acc = (a[lo:lo + n] * k).sum(0) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def window_u8(img, box, rw, rh, win_left, win_top, out_w, out_h, filt, flip=False):
    """uint8 [out_h, out_w, 3] = img.crop(box).resize((rw, rh), filt).crop(window) [mirrored]; img uint8 [H, W, 3]."""
    l, t, r, b = box
    assert 0 <= l < r <= img.shape[1] and 0 <= t < b <= img.shape[0]
    assert 0 <= win_left <= rw - out_w and 0 <= win_top <= rh - out_h
    a = img[t:b, l:r]
    a = _resample_axis0(a.transpose(1, 0, 2), rw, filt, win_left, out_w).transpose(1, 0, 2)   # horizontal first, rounded to uint8
    a = _resample_axis0(a, rh, filt, win_top, out_h)
    return np.ascontiguousarray(a[:, ::-1] if flip else a)


def normalize_table():
    """[3][256] float32: ToTensor + Normalize(ImageNet) of every byte per channel, by the datasets' very expression."""
    mean = np.asarray((0.485, 0.456, 0.406), np.float32)
    std = np.asarray((0.229, 0.224, 0.225), np.float32)
    a = np.broadcast_to(np.arange(256, dtype=np.float32).reshape(256, 1), (256, 3)) / 255.0
    return np.ascontiguousarray(((a - mean) / std).T)


def to_tensor(u8):
    """float32 [3, h, w] of a uint8 [h, w, 3] window, through the table as the kernel does."""
    lut = normalize_table()
    return np.stack([lut[c][u8[:, :, c]] for c in range(3)])


def make_image(w, h, seed=0):
    """A uint8 [h, w, 3] image with smooth parts and noise, so that rounding and clipping both occur."""
    rng = np.random.default_rng(seed * 7919 + w * 31 + h)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 5 + y * 3) % 256, (x * y) % 256, (255 - x * 2 - y) % 256], -1)
    noise = rng.integers(0, 256, (h, w, 3))
    return np.where(rng.random((h, w, 1)) < 0.5, base, noise).astype(np.uint8)
