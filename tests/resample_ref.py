"""Numpy restatement of Pillow's 8-bit ImagingResample (Resample.c), the one copy the test references share: crop a box,
resample it to rw x rh (bilinear or bicubic), keep the out_w x out_h window at (win_left, win_top).  Only the output indices
of the window are evaluated, and no pass is skipped: a pass that changes nothing has the identity as its coefficient rows.
sais_amd/csrc/resample.hpp is the same arithmetic on the device; tests/test_augment_host.py and tests/test_imgfolder_host.py
hold it against Pillow bit for bit through tests/aug_ref.py and tests/imgfolder_ref.py."""
import numpy as np

PRECISION_BITS = 32 - 8 - 2
BILINEAR, BICUBIC = 0, 1


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
