"""Numpy restatement of the pixel operations of the DINO multi-crop augmentation, as Pillow computes them (array in,
array out).  tests/test_augment_host.py holds every function here against Pillow bit for bit; the kernels of
sais_amd/csrc/augment.hip implement exactly this arithmetic.

Source of each: Pillow's Resample.c (8-bit ImagingResample, bicubic: tests/resample_ref.py), Convert.c (rgb2l, rgb2hsv, hsv2rgb), Blend.c
(ImageEnhance = Image.blend(degenerate, image, factor)), BoxBlur.c (GaussianBlur = three box passes per axis),
ImageOps.solarize."""
import numpy as np

from resample_ref import BICUBIC, window_u8

f32 = np.float32


# ------------------------------------------------------------------ crop + bicubic resize
def crop_resize(frame, box, size):
    """img.crop(box).resize((size, size), Image.BICUBIC) of a uint8 [H,W,3] frame; box = left, top, right, bottom."""
    return window_u8(frame, box, size, size, 0, 0, size, size, BICUBIC)


# ------------------------------------------------------------------ pointwise colour operations
def luma(a):
    """convert("L"): uint8 [...,3] -> uint8 [...]."""
    a = a.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def grayscale(a):
    return np.repeat(luma(a)[..., None], 3, -1)


def blend(degenerate, a, factor):
    """Image.blend(degenerate, image, factor): float32 arithmetic, truncation, clipping only when extrapolating."""
    f = f32(factor)
    d, s = degenerate.astype(np.int32), a.astype(np.int32)
    t = d.astype(f32) + f * (s - d).astype(f32)
    if 0 <= f <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.minimum(t, 255).astype(np.int32))).astype(np.uint8)


def brightness(a, factor):
    return blend(np.zeros_like(a), a, factor)


def saturation(a, factor):
    return blend(grayscale(a), a, factor)


def contrast_mean(a):
    lum = luma(a)
    return int(int(lum.astype(np.int64).sum()) / lum.size + 0.5)


def contrast(a, factor):
    return blend(np.full_like(a, contrast_mean(a)), a, factor)


def solarize(a):
    return np.where(a < 128, a, 255 - a).astype(np.uint8)


def rgb_to_hsv(a):
    """convert("HSV"): float32 variables, double wherever a double literal enters the expression."""
    r, g, b = (a[..., i].astype(np.int32) for i in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    flat = maxc == minc
    cr = np.where(flat, 1, maxc - minc).astype(f32)
    s = cr / np.where(flat, 1, maxc).astype(f32)
    rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
    h = np.where(r == maxc, bc - gc,
                 np.where(g == maxc, (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(f32),
                          (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(f32)))
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(flat, 0, uh), np.where(flat, 0, us), maxc], -1).astype(np.uint8)


def _round_half_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def hsv_to_rgb(a):
    """convert("RGB") of an HSV image."""
    h, s, v = (a[..., i] for i in range(3))
    hf = h.astype(f32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(hf).astype(np.int32)
    f = (hf - i.astype(f32).astype(np.float64)).astype(f32).astype(np.float64)
    fs = (s.astype(f32).astype(np.float64) / 255.0).astype(f32).astype(np.float64)
    vf = v.astype(f32).astype(np.float64)
    p = np.clip(_round_half_away(vf * (1.0 - fs)), 0, 255).astype(np.uint8)
    q = np.clip(_round_half_away(vf * (1.0 - fs * f)), 0, 255).astype(np.uint8)
    t = np.clip(_round_half_away(vf * (1.0 - fs * (1.0 - f))), 0, 255).astype(np.uint8)
    k = i % 6
    r = np.choose(k, [v, q, p, p, t, v])
    g = np.choose(k, [t, v, v, q, p, p])
    b = np.choose(k, [p, p, t, v, v, q])
    out = np.stack([r, g, b], -1)
    return np.where((s == 0)[..., None], v[..., None], out).astype(np.uint8)


def hue(a, shift):
    """ColorJitter's hue step on the Pillow backend: H of convert("HSV") moves by `shift` (= int(factor * 255)) mod 256."""
    hsv = rgb_to_hsv(a)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + shift) % 256).astype(np.uint8)
    return hsv_to_rgb(hsv)


# ------------------------------------------------------------------ Gaussian blur
def box_radius(radius, passes=3):
    """_gaussian_blur_radius: float32 variables, double inside the expressions with double literals."""
    r = f32(radius)
    sigma2 = f32(f32(r * r) / f32(passes))
    L = f32(np.sqrt(12.0 * np.float64(sigma2) + 1.0))
    l = f32(np.floor((np.float64(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    return f32(l + a)


def box_constants(fr):
    """(r, ww, fw) of ImagingHorizontalBoxBlur for the float32 box radius fr."""
    fr = f32(fr)
    r = int(fr)
    ww = int(f32(1 << 24) / f32(f32(fr * f32(2)) + f32(1)))
    fw = (((1 << 24) - (2 * r + 1) * ww) & 0xFFFFFFFF) // 2
    return r, ww, fw


def _box_pass(a, r, ww, fw):
    """One box pass along axis 1 of uint8 [rows, n, ...]; the line is extended by its edge pixels."""
    n = a.shape[1]
    idx = np.arange(n)
    src = a.astype(np.int64)
    acc = sum(src[:, np.clip(idx + j, 0, n - 1)] for j in range(-r, r + 1))
    far = src[:, np.clip(idx - r - 1, 0, n - 1)] + src[:, np.clip(idx + r + 1, 0, n - 1)]
    return (((acc * ww + far * fw + (1 << 23)) & 0xFFFFFFFF) >> 24).astype(np.uint8)


def gaussian_blur(a, radius):
    """img.filter(ImageFilter.GaussianBlur(radius)) of uint8 [H,W,3]."""
    r, ww, fw = box_constants(box_radius(radius))
    if box_radius(radius) == 0:
        return a.copy()
    for _ in range(3):
        a = _box_pass(a, r, ww, fw)
    a = a.transpose(1, 0, 2)
    for _ in range(3):
        a = _box_pass(a, r, ww, fw)
    return np.ascontiguousarray(a.transpose(1, 0, 2))


# ------------------------------------------------------------------ a whole view
MEAN = np.array((0.485, 0.456, 0.406), dtype=np.float32)
STD = np.array((0.229, 0.224, 0.225), dtype=np.float32)


def normalize(a):
    x = a.astype(np.float32).transpose(2, 0, 1) / 255.0
    return (x - MEAN.reshape(3, 1, 1)) / STD.reshape(3, 1, 1)


def color_chain(a, p):
    """Everything of a view after crop + resize, up to the uint8 image that is normalised; p: ViewParams-like."""
    if p.flip:
        a = a[:, ::-1]
    if p.jitter:
        for op in p.order:
            a = (lambda x: brightness(x, p.brightness), lambda x: contrast(x, p.contrast),
                 lambda x: saturation(x, p.saturation), lambda x: hue(x, int(p.hue * 255)))[op](a)
    if p.gray:
        a = grayscale(a)
    if p.blur is not None:
        a = gaussian_blur(a, p.blur)
    if p.solarize:
        a = solarize(a)
    return np.ascontiguousarray(a)


def view(frame, p):
    return normalize(color_chain(crop_resize(frame, p.box, p.size), p))
