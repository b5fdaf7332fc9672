"""numpy restatements of the attention-map rendering path (dino-main/video_generation.py :190-241, visualize_attention.py
:179-208): the CLS row of the last block's softmax in fp64, the "keep xx% of the mass" mask in fp64 with the stable order and the
analysis of which elements rounding can move, the head mean in numpy's own f32 arithmetic, and matplotlib's Normalize +
Colormap.__call__ on an f32 array.  Shared by test_attnviz_gpu.py, test_attnviz_host.py and golden/make_golden_attnviz.py;
numpy only (the host test holds `to_rgb` to matplotlib itself)."""
import numpy as np

HEADS, HD, D = 6, 64, 384
FRAGILE_CAP = 2             # fragile elements per (frame, head) row the test inputs may have (asserted before any comparison)

# name, H, W, seed of vos_ref.dense_input; F = 2.  25 tokens: one partial key tile; 171: a ragged tail; 197: the resident kernel's
# size; 274: more than four tiles
CLS_CASES = [("c64x96", 64, 96, 241), ("c160x272", 160, 272, 242), ("c224x224", 224, 224, 243), ("c208x336", 208, 336, 244)]
VIDEO_CASES = ["c64x96", "c160x272"]       # golden (ii): the frames VideoGenerator._inference ran on, two of each size
THRESHOLD = 0.6                            # video_generation.py's default
TIE_SHAPE, TIE_SEED = (6, 24), 251         # golden (iii): rows quantised to 1/64


def tie_rows():
    """f32 [6, 24] of positive multiples of 1/64 with many repeats (exact in f32, and so are their sums)"""
    rng = np.random.Generator(np.random.PCG64(TIE_SEED))
    return (rng.integers(1, 9, size=TIE_SHAPE) / 64.0).astype(np.float32)


def cls_probs(qkv, frames, ntok):
    """fp64 [frames, 6, ntok]: softmax_j(q_cls,h . k_j,h / 8) over all ntok keys, from qkv [frames * ntok, 1152] = q | k | v
    head-major (row 0 of Attention.forward's attn, vision_transformer.py:83-90)."""
    a = np.asarray(qkv, dtype=np.float64).reshape(frames, ntok, 3, HEADS, HD)
    q, k = a[:, 0, 0], a[:, :, 1]                                   # [F, 6, 64], [F, ntok, 6, 64]
    s = np.einsum("fhd,fjhd->fhj", q, k) * 0.125
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _shares(p):
    """(order, inclusive cumulative share in that order), fp64, along the last axis: ascending by value, equal values by
    ascending index (stable); a row whose sum is 0 has share 0 everywhere"""
    v = np.asarray(p, dtype=np.float64)
    order = np.argsort(v, axis=-1, kind="stable")
    tot = v.sum(-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.cumsum(np.take_along_axis(v, order, -1) / tot, axis=-1)
    return order, np.where(tot > 0, share, 0.0)


def _unsort(a, order):
    out = np.empty_like(a)
    np.put_along_axis(out, order, a, -1)
    return out


def mass_mask(p, threshold):
    """u8 like p: element j is kept iff its inclusive cumulative share of the row (last axis) is > 1 - threshold
    (video_generation.py:197-205)."""
    order, share = _shares(p)
    return _unsort(share > 1.0 - threshold, order).astype(np.uint8)


def fragile(p, threshold):
    """bool like p: elements whose fp64 cumulative share lies within n 2^-24 of the cut, the worst-case error of an n-term f32
    sum of a unit-mass row: only there may an f32 evaluation (the reference's, in any summation order) decide otherwise."""
    order, share = _shares(p)
    n = np.asarray(p).shape[-1]
    return _unsort(np.abs(share - (1.0 - threshold)) <= n * 2.0 ** -24, order)


def heat(p, keep=None, head0=0, nheads=None):
    """f32 [F, n]: sum(attentions[i] * 1 / nh for i in range(nh)) of video_generation.py:235-238 after `attentions * th_attn`
    (:229), as numpy evaluates it in f32: per head an f32 product by 0 or 1 and an f32 division, summed in ascending head order
    starting from the first term.  p f32 [F, heads, n], keep u8 like p or None."""
    p = np.asarray(p, dtype=np.float32)
    nheads = p.shape[1] - head0 if nheads is None else nheads
    acc = None
    for hh in range(head0, head0 + nheads):
        m = np.float32(1.0) if keep is None else (np.asarray(keep)[:, hh] != 0).astype(np.float32)
        term = (p[:, hh] * m) / np.float32(nheads)
        acc = term if acc is None else acc + term
    assert acc.dtype == np.float32
    return acc


def colour_index(a):
    """int [..]: the table index ScalarMappable.to_rgba gives every element of ONE f32 map: Normalize with vmin / vmax = the map's
    minimum / maximum (in place, in f32: subtract, divide; all zero when they are equal), then Colormap.__call__: times N = 256 in
    f32, the value 256 -> 255, truncation (the result is never below 0 or above 255 here)."""
    a = np.array(a, dtype=np.float32, copy=True)
    vmin, vmax = a.min(), a.max()
    if vmin == vmax:
        return np.zeros(a.shape, dtype=np.int64)
    a -= vmin
    a /= (vmax - vmin)
    a *= np.float32(256.0)
    a[a == 256.0] = 255.0
    return np.clip(a.astype(np.int64), 0, 255)


def to_rgb(heat_maps, lut, patch=1):
    """u8 [F, h patch, w patch, 3]: the colours of f32 maps [F, h, w] under the byte table lut u8 [256, 3], every frame
    normalised on its own, nearest upsampling by `patch` (which commutes with the colormap: a patch holds one value)."""
    out = np.stack([np.asarray(lut)[colour_index(m)] for m in np.asarray(heat_maps)])
    return np.repeat(np.repeat(out, patch, axis=1), patch, axis=2)
