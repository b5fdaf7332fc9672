"""fp64 restatements of label propagation (dino-main/eval_video_segmentation.py:113-150), of its queue (:45-71) and of the
upsample / norm_mask / argmax tail (:74-76, :102-110), the input generators of the video-segmentation tests and the analysis
of which queries' top-k cut rounding can move.  Shared by test_vos_gpu.py, test_vos_host.py and golden/make_golden_vos.py;
numpy only."""
import hashlib

import numpy as np

TAU = 2.0 ** -15            # the bound the kernel's cosines must meet (knn_ref.TAU: the project's bf16x3 bound with its margin)
DIM = 384
FRAGILE_CAP = 0.05
PROP_TOL = 1e-3             # |out - fp64| <= PROP_TOL * max|segs| on non-fragile queries: every kept weight is off by at most
#                             e^(10 TAU) - 1 = 3.05e-4 relative, twice that after normalisation, rounded up for the f32 exp and sums
ARGMAX_MARGIN = 1e-5        # pixels whose two best normalised channels are closer than this may differ
ARGMAX_EXCEPT_CAP = 0.01

# name, h, w, nctx, C, r, topk, seed
GOLDEN_CASES = [
    ("borders", 7, 10, 3, 3, 2, 5, 201),        # windows cut by every border
    ("corners", 6, 9, 1, 2, 1, 5, 202),         # corners have 4 < topk candidates
    ("queue", 9, 13, 8, 4, 3, 5, 203),          # full queue
    ("global", 5, 8, 2, 3, 0, 5, 204),          # no restriction
    ("limits", 12, 17, 16, 64, 12, 16, 205),    # every limit at once, a window wider than the grid
]
WORKLOAD_CASE = ("workload", 30, 52, 8, 3, 12, 5, 206)      # the workload's own grid: fp64 restatement only
TIE_CASE = ("ties", 8, 11, 4, 3, 2, 5, 207)                  # slots 1 and 3 repeat slots 0 and 2 bit for bit
SEQ = dict(h=6, w=9, frames=5, C=3, n_last_frames=2, r=2, topk=5, seed=211)
# name, C, h, w, patch, seed, special (0: none; 1: last channel all zero, the one before a positive constant; 2: last all zero)
UPSAMPLE_CASES = [("u0", 3, 5, 7, 16, 221, 0), ("u1", 4, 6, 4, 8, 222, 1), ("u2", 3, 4, 5, 16, 223, 2)]


DENSE_CASES = [("d160x272", 160, 272, 1, 231), ("d208x336", 208, 336, 2, 232)]     # name, H, W, n (last blocks), seed; F = 2
DENSE_ROWS = [0, 1, 21, 22, 137, 272, 273]      # token rows of d208x336 kept in the golden file (d160x272 keeps all 171)


def dense_input(H, W, seed, frames=2):
    """frames f32 [frames, 3, H, W] ~ N(0, 1): normalised pixels"""
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((frames, 3, H, W)).astype(np.float32)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def _smooth(a):
    """3 x 3 box filter over the first two axes (edge-replicated), rescaled to unit standard deviation"""
    p = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="edge")
    s = sum(p[i:i + a.shape[0], j:j + a.shape[1]] for i in range(3) for j in range(3)) / 9.0
    return s / s.std()


def soft_masks(rng, n_frames, C, n):
    """positive soft masks [n_frames, C, n] that sum to one over the channels"""
    e = np.exp(2.0 * rng.standard_normal((n_frames, C, n)))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def make_case(h, w, nctx, C, r, topk, seed, noise=0.5):
    """(feat_tar f32 [n, 384], ctx_feats f32 [nctx, n, 384], segs f32 [nctx, C, n]); features are spatially smoothed noise
    shared by all frames plus per-frame noise, un-normalised."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = h * w
    base = _smooth(rng.standard_normal((h, w, DIM))).reshape(n, DIM)
    tar = (base + noise * rng.standard_normal((n, DIM))).astype(np.float32)
    ctx = (base[None] + noise * rng.standard_normal((nctx, n, DIM))).astype(np.float32)
    return tar, ctx, soft_masks(rng, nctx, C, n)


def make_tie_case():
    _, h, w, nctx, C, r, topk, seed = TIE_CASE
    tar, ctx, segs = make_case(h, w, nctx, C, r, topk, seed)
    ctx[1], ctx[3] = ctx[0], ctx[2]              # every cosine occurs twice; the masks of the twins differ
    return tar, ctx, segs


def make_sequence():
    """(feats f32 [frames, n, 384], first_seg f32 [C, n] one-hot): a scene that drifts slowly"""
    s = SEQ
    rng = np.random.Generator(np.random.PCG64(s["seed"]))
    n = s["h"] * s["w"]
    base = _smooth(rng.standard_normal((s["h"], s["w"], DIM))).reshape(n, DIM)
    feats = np.stack([base + 0.5 * rng.standard_normal((n, DIM)) for _ in range(s["frames"])]).astype(np.float32)
    yy, xx = np.divmod(np.arange(n), s["w"])
    lab = np.where(xx < 3, 0, np.where(yy < 3, 1, 2))
    first = np.zeros((s["C"], n), dtype=np.float32)
    first[lab, np.arange(n)] = 1.0
    return feats, first


def make_upsample_case(C, h, w, patch, seed, special=0):
    """seg f32 [C, h, w]: smooth positive maps; special: the all-zero channel is norm_mask's `max <= 0` side, the positive
    constant one its 0 / 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    seg = np.abs(_smooth(rng.standard_normal((h, w, C)))).transpose(2, 0, 1).astype(np.float32)
    if special:
        seg[-1] = 0.0
    if special == 1:
        seg[-2] = 0.25
    return np.ascontiguousarray(seg)


# ------------------------------------------------------------------------------------------------- propagation
def window(h, w, r):
    """bool [n (key), n (query)]: restrict_neighborhood (:85-99), everything when r == 0"""
    n = h * w
    if r == 0:
        return np.ones((n, n), dtype=bool)
    y, x = np.divmod(np.arange(n), w)
    return (np.abs(y[:, None] - y[None, :]) <= r) & (np.abs(x[:, None] - x[None, :]) <= r)


def cosines(tar, ctx):
    """fp64 [nctx, n (key), n (query)] of the L2-normalised rows; one product per context, so bit-identical context frames give
    bit-identical cosines"""
    t = tar.astype(np.float64)
    t /= np.maximum(np.sqrt((t * t).sum(1, keepdims=True)), 1e-12)
    out = []
    for c in range(ctx.shape[0]):
        k = ctx[c].astype(np.float64)
        k /= np.maximum(np.sqrt((k * k).sum(1, keepdims=True)), 1e-12)
        out.append(k @ t.T)
    return np.stack(out)


def propagate(tar, ctx, segs, h, w, r, topk):
    """label_propagation in fp64 -> [C, n].  a = exp(cos / 0.1) inside the window and 0 outside; per query the topk-th largest
    of ALL nctx * n values is the threshold (0 when the window holds fewer): everything below it is dropped, ties stay."""
    nctx, C, n = segs.shape
    a = np.exp(cosines(tar, ctx) / 0.1) * window(h, w, r)[None]
    a = a.reshape(nctx * n, n)
    t = np.sort(a, axis=0)[-topk]
    a = np.where(a < t[None], 0.0, a)
    a /= a.sum(0, keepdims=True)
    s = segs.astype(np.float64).transpose(1, 0, 2).reshape(C, nctx * n)
    return s @ a


def fragile_queries(tar, ctx, h, w, r, topk, tau=TAU):
    """bool [n]: queries whose kept set can change when every cosine moves by at most tau: the topk-th largest in-window
    cosine and the next SMALLER one differ by less than 2 tau (values equal to the topk-th are kept with it, so exact twins
    on the cut are not fragile by themselves).  Only the features decide this."""
    cos = cosines(tar, ctx)
    win = window(h, w, r)
    n = h * w
    out = np.zeros(n, dtype=bool)
    for q in range(n):
        v = np.sort(cos[:, win[:, q], q].ravel())[::-1]
        if v.size <= topk:
            continue
        below = v[v < v[topk - 1]]
        out[q] = below.size > 0 and v[topk - 1] - below[0] < 2 * tau
    return out


def run_sequence(feats, first_seg, h, w, n_last_frames, r, topk, fragile=None):
    """The queue of eval_video_tracking_davis (:45-71) around `propagate`: soft masks fp64 [frames - 1, C, n] of frames
    1 .. frames - 1.  fragile: a list that receives the fragile-query count of every step."""
    que, out = [], []
    for t in range(1, feats.shape[0]):
        ctx = np.stack([feats[0]] + [p[0] for p in que])
        segs = np.stack([first_seg] + [p[1] for p in que]).astype(np.float64)
        seg = propagate(feats[t], ctx, segs, h, w, r, topk)
        if fragile is not None:
            fragile.append(int(fragile_queries(feats[t], ctx, h, w, r, topk).sum()))
        if len(que) == n_last_frames:
            que.pop(0)
        que.append((feats[t], seg))
        out.append(seg)
    return np.stack(out)


# ------------------------------------------------------------------------------------------------- upsample + argmax
def upsample(seg, patch):
    """F.interpolate(scale_factor=patch, mode='bilinear', align_corners=False) of [C, h, w] in fp64"""
    C, h, w = seg.shape
    s = seg.astype(np.float64)

    def axis(n):
        src = np.maximum((np.arange(n * patch) + 0.5) / patch - 0.5, 0.0)
        i0 = np.floor(src).astype(np.int64)
        return i0, np.minimum(i0 + 1, n - 1), src - i0
    y0, y1, ly = axis(h)
    x0, x1, lx = axis(w)
    ly, lx = ly[:, None], lx[None, :]
    top = (1 - lx) * s[:, y0][:, :, x0] + lx * s[:, y0][:, :, x1]
    bot = (1 - lx) * s[:, y1][:, :, x0] + lx * s[:, y1][:, :, x1]
    return (1 - ly) * top + ly * bot


def norm_mask(up):
    """norm_mask (:102-110) in fp64: a channel whose maximum is <= 0 is left as it is"""
    out = up.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(up.shape[0]):
            if up[c].max() > 0:
                sh = up[c] - up[c].min()
                out[c] = sh / sh.max()
    return out


def upsample_argmax(seg, patch):
    """(labels u8 [h patch, w patch], near [same] bool): torch.max(dim=0) of the normalised upsampled map — the first of the
    largest, a NaN counting as the largest — and the pixels whose two best channels lie within ARGMAX_MARGIN."""
    m = norm_mask(upsample(seg, patch))
    labels = np.argmax(m, axis=0).astype(np.uint8)             # numpy's argmax: the first NaN, else the first maximum
    if m.shape[0] == 1:
        return labels, np.zeros(labels.shape, dtype=bool)
    finite = np.where(np.isnan(m), np.inf, m)                  # a NaN channel wins by any margin
    top2 = np.sort(finite, axis=0)[-2:]
    with np.errstate(invalid="ignore"):
        near = (top2[1] - top2[0]) < ARGMAX_MARGIN
    return labels, near
