"""Numpy restatement of the image-folder transforms (sais_amd/csrc/imgfolder.hip), as Pillow computes them: crop a box,
resample it to rw x rh with the 8-bit ImagingResample of Resample.c (bilinear or bicubic), keep the out_w x out_h window at
(win_left, win_top), mirror it (all of that is window_u8 of tests/resample_ref.py, re-exported here), ToTensor + Normalize.
tests/test_imgfolder_host.py holds every function here against Pillow bit for bit; the GPU tests hold the kernel against
the Pillow datasets.

EVAL_SIZES, TRAIN_BOXES and SQUARE_SIZES are the geometries both test files use."""
import numpy as np

from resample_ref import (BICUBIC, BILINEAR, PRECISION_BITS, _resample_axis0, bicubic, bilinear, coefficients,  # noqa: F401
                          window_u8)

# (w, h) of the eval transform (Resize(256, bicubic) + CenterCrop(224))
EVAL_SIZES = [(20, 31), (300, 500), (500, 375), (256, 300), (640, 256), (1200, 900), (64, 700), (1, 1), (257, 255)]
# ((w, h), box) of the train transform (box -> 224 x 224, bilinear): two corner boxes of a few pixels, a large interior box
TRAIN_BOXES = [((300, 200), (0, 0, 3, 2)), ((300, 200), (297, 198, 300, 200)), ((300, 200), (21, 17, 263, 181))]
# ((w, h), imsize) of the copy-detection transform (whole image -> imsize x imsize, bicubic)
SQUARE_SIZES = [((333, 211), 320)]


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
