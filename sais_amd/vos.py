"""Video object segmentation by label propagation (dino-main/eval_video_segmentation.py) on the HIP kernels of csrc/vos.hip.

`label_propagation` has the reference's meaning (:113-150) without its [nctx hw, hw] affinity matrix, its dense neighbourhood
mask (restrict_neighborhood, :85-99) and its column-wise topk: sais_vos_propagate does the windowed top-k and the weighted
sum of the soft masks in one launch.  `LabelPropagator` keeps the reference's queue (:45-71) as device ring buffers,
`upsample_argmax` is the tail of eval_video_tracking_davis (:74-76).  There is no CPU fallback: host tensors raise.  The frame
and annotation readers of the CLI (SAIS/scripts/dino-main/eval_video_segmentation.py) live here too.
"""
import ctypes
import glob
import os

import numpy as np
import torch

from . import _lib as L
from . import ops

DIM, MAX_CONTEXT, MAX_CLASSES, MAX_TOPK, MAX_PATCHES, UPSAMPLE_WS_FLOATS = 384, 16, 64, 16, 4096, 128
MEAN, STD = (0.485, 0.456, 0.406), (0.228, 0.224, 0.225)      # color_normalize (:244): the reference's 0.228 for red included


def _dev(t, name, dims):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a device tensor (the propagation path has no CPU fallback)")
    if t.dim() not in dims:
        raise ValueError(f"{name}: expected {' or '.join(str(d) for d in dims)} dimensions, got {tuple(t.shape)}")
    return t.float().contiguous()


def _check_limits(n, nctx, C, topk, radius, dim):
    if dim != DIM:
        raise ValueError(f"feature dimension {dim}: the kernel takes {DIM}")
    if not 1 <= n <= MAX_PATCHES:
        raise ValueError(f"h * w = {n} must be in [1, {MAX_PATCHES}]")
    if not 1 <= nctx <= MAX_CONTEXT:
        raise ValueError(f"{nctx} context frames: must be in [1, {MAX_CONTEXT}]")
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"{C} classes: must be in [1, {MAX_CLASSES}]")
    if not 1 <= topk <= MAX_TOPK:
        raise ValueError(f"topk = {topk} must be in [1, {MAX_TOPK}]")
    if radius < 0:
        raise ValueError("size_mask_neighborhood must be >= 0")


def normalize_rows(feat, out=None):
    """F.normalize(feat, dim=1, p=2) (:125-126) of f32 [rows, 384] on the device."""
    out = torch.empty_like(feat) if out is None else out
    inv = torch.empty(feat.shape[0], dtype=torch.float32, device=feat.device)
    ops.l2norm_fwd(feat, out, inv)
    return out


def propagate_normalized(tar, ctx, segs, h, w, radius, topk, nctx=None, order=None, out=None):
    """sais_vos_propagate on L2-normalised features: tar [n, 384], ctx [slots, n, 384], segs [slots, C, n] -> out [C, n].
    order: the slot of every context frame (default 0 .. nctx - 1)."""
    n, C = tar.shape[0], segs.shape[1]
    nctx = ctx.shape[0] if nctx is None else nctx
    order = list(range(nctx)) if order is None else [int(s) for s in order]
    if len(order) != nctx or any(not 0 <= s < ctx.shape[0] for s in order):
        raise ValueError(f"context order {order} does not name {nctx} of the {ctx.shape[0]} slots")
    out = torch.empty(C, n, dtype=torch.float32, device=tar.device) if out is None else out
    L.call("sais_vos_propagate", ops._p(tar), ops._p(ctx), ops._p(segs), nctx, C, h, w, tar.shape[1], int(radius), int(topk),
           (ctypes.c_int * nctx)(*order), ops._p(out), ops._stream())
    return out


@torch.no_grad()
def label_propagation(feat_tar, ctx_feats, ctx_segs, h, w, size_mask_neighborhood, topk):
    """label_propagation (:113-150): feat_tar f32 [h w, 384] (patch features of the target frame, un-normalised), ctx_feats
    [nctx, h w, 384], ctx_segs [nctx, C, h, w] (or [nctx, C, h w]) soft masks -> seg_tar f32 [C, h, w].  Context order: as the
    reference's lists (first frame, then oldest to newest)."""
    tar = _dev(feat_tar, "feat_tar", (2,))
    ctx = _dev(ctx_feats, "ctx_feats", (3,))
    segs = _dev(ctx_segs, "ctx_segs", (3, 4))
    n, nctx = int(h) * int(w), ctx.shape[0]
    _check_limits(n, nctx, segs.shape[1], int(topk), int(size_mask_neighborhood), tar.shape[1])
    segs = segs.reshape(nctx, segs.shape[1], -1)
    if tar.shape[0] != n or tuple(ctx.shape[1:]) != (n, tar.shape[1]) or segs.shape[0] != nctx or segs.shape[2] != n:
        raise ValueError(f"shapes {tuple(tar.shape)}, {tuple(ctx.shape)}, {tuple(segs.shape)} do not fit a {h} x {w} grid")
    tar_n = normalize_rows(tar)
    ctx_n = normalize_rows(ctx.view(nctx * n, -1)).view(nctx, n, -1)
    return propagate_normalized(tar_n, ctx_n, segs, int(h), int(w), size_mask_neighborhood, topk).view(-1, int(h), int(w))


class LabelPropagator:
    """The queue of eval_video_tracking_davis (:45-71) on the device: slot 0 holds the first frame's (normalised) features and
    its mask for the whole video, slots 1 .. n_last_frames are a ring of the last frames and the soft masks propagated to
    them.  A frame is normalised once, when it enters.  The context of a step is read in the reference's order — first
    frame, then oldest to newest — through the kernel's slot list, so the ring never moves."""

    def __init__(self, first_feat, first_seg, h, w, n_last_frames=7, size_mask_neighborhood=12, topk=5):
        feat = _dev(first_feat, "first_feat", (2,))
        seg = _dev(first_seg, "first_seg", (3, 4))
        seg = seg.reshape(-1, int(h) * int(w)) if seg.dim() == 3 else seg.reshape(seg.shape[1], -1)
        self.h, self.w, self.n, self.C = int(h), int(w), int(h) * int(w), seg.shape[0]
        self.n_last, self.radius, self.topk = int(n_last_frames), int(size_mask_neighborhood), int(topk)
        if self.n_last < 0:
            raise ValueError("n_last_frames must be >= 0")
        _check_limits(self.n, 1 + self.n_last, self.C, self.topk, self.radius, feat.shape[1])
        if feat.shape[0] != self.n or seg.shape[1] != self.n:
            raise ValueError(f"first frame {tuple(feat.shape)} / mask {tuple(seg.shape)} do not fit a {h} x {w} grid")
        dev = feat.device
        self.feats = torch.empty(1 + self.n_last, self.n, DIM, dtype=torch.float32, device=dev)
        self.segs = torch.empty(1 + self.n_last, self.C, self.n, dtype=torch.float32, device=dev)
        normalize_rows(feat, self.feats[0])
        self.segs[0].copy_(seg)
        self.count = 0          # frames pushed so far; frame j (0-based) lives in slot 1 + j % n_last
        self._tar = torch.empty(self.n, DIM, dtype=torch.float32, device=dev)

    def context_order(self):
        """Slots of the current context: the first frame, then the queue from oldest to newest."""
        held = min(self.count, self.n_last)
        return [0] + [1 + j % self.n_last for j in range(self.count - held, self.count)]

    @torch.no_grad()
    def step(self, feat_tar):
        """Propagate to the next frame (features f32 [h w, 384], un-normalised), push the result, return seg_tar [C, h, w]."""
        feat = _dev(feat_tar, "feat_tar", (2,))
        if tuple(feat.shape) != (self.n, DIM):
            raise ValueError(f"feat_tar: expected [{self.n}, {DIM}], got {tuple(feat.shape)}")
        normalize_rows(feat, self._tar)
        order = self.context_order()
        seg = propagate_normalized(self._tar, self.feats, self.segs, self.h, self.w, self.radius, self.topk, nctx=len(order),
                                   order=order)
        if self.n_last > 0:          # the slot taken may be the oldest context frame: written after the launch, on its stream
            slot = 1 + self.count % self.n_last
            self.feats[slot].copy_(self._tar)
            self.segs[slot].copy_(seg)
        self.count += 1
        return seg.view(self.C, self.h, self.w)


@torch.no_grad()
def upsample_argmax(seg, patch=16):
    """F.interpolate(scale_factor=patch, bilinear, align_corners=False) + norm_mask + torch.max(dim=0) (:74-76, :102-110):
    seg f32 [C, h, w] on the device -> labels uint8 [h patch, w patch]."""
    s = _dev(seg, "seg", (3,))
    C, h, w = s.shape
    patch = int(patch)
    if not 1 <= C <= MAX_CLASSES or not 1 <= h * w <= MAX_PATCHES or not 1 <= patch <= 64:
        raise ValueError(f"seg {tuple(s.shape)}, patch {patch}: at most {MAX_CLASSES} classes, {MAX_PATCHES} patches, patch <= 64")
    labels = torch.empty(h * patch, w * patch, dtype=torch.uint8, device=s.device)
    ws = torch.empty(C * UPSAMPLE_WS_FLOATS, dtype=torch.float32, device=s.device)
    L.call("sais_vos_upsample_argmax", ops._p(s), C, h, w, patch, ops._p(labels), ops._p(ws), ops._stream())
    return labels


# ---------------------------------------------------------------------------------------------- CLI helpers (host side)
def to_one_hot(y_tensor, n_dims=None):
    """to_one_hot (:176-188): integer labels [1, h, w] -> one-hot f32 [1, n_dims, h, w] (n_dims: max label + 1)."""
    if n_dims is None:
        n_dims = int(y_tensor.max() + 1)
    _, h, w = y_tensor.size()
    y = y_tensor.long().view(-1, 1)
    one_hot = torch.zeros(y.shape[0], n_dims).scatter_(1, y, 1)
    return one_hot.view(h, w, n_dims).permute(2, 0, 1).unsqueeze(0)


def target_size(ori_h, ori_w, scale=480):
    """The (th, tw) rule of read_frame (:203-211): the short side becomes `scale`, the long side is scaled with it and floored
    to a multiple of 64."""
    if ori_h > ori_w:
        tw = scale
        th = int(((tw * ori_h) / ori_w // 64) * 64)
    else:
        th = scale
        tw = int(((th * ori_w) / ori_h // 64) * 64)
    return th, tw


def read_frame_list(video_dir):
    return sorted(glob.glob(os.path.join(video_dir, "*.jpg")))


def read_frame(path, scale=480):
    """read_frame (:197-221) on Pillow: (f32 [3, th, tw] normalised RGB, ori_h, ori_w).  The resize filter (Pillow's bilinear)
    is not cv2.resize's: this step is parity-unpinned."""
    from PIL import Image
    with open(path, "rb") as fh:
        img = Image.open(fh).convert("RGB")
    ori_w, ori_h = img.size
    th, tw = target_size(ori_h, ori_w, scale)
    a = np.asarray(img.resize((tw, th), Image.BILINEAR), dtype=np.float32) / 255.0
    a = (a - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))), ori_h, ori_w


def read_seg(path, factor, scale=480):
    """read_seg (:224-241): (one-hot first mask f32 [1, C, th / factor, tw / factor], the annotation as an array, its palette
    as uint8 [256, 3] — the reference downloads a palette instead; this one is the annotation's own)."""
    from PIL import Image
    seg = Image.open(path)
    w_, h_ = seg.size
    th, tw = target_size(h_, w_, scale)
    small = np.array(seg.resize((tw // factor, th // factor), 0))
    small = torch.from_numpy(small.copy()).contiguous().float().unsqueeze(0)
    pal = seg.getpalette()
    if pal is None:
        raise ValueError(f"{path}: the first annotation must be an indexed PNG (its palette colours the outputs)")
    pal = np.asarray(list(pal) + [0] * (768 - len(pal)), dtype=np.uint8).reshape(-1, 3)
    return to_one_hot(small), np.asarray(seg), pal


def imwrite_indexed(filename, array, color_palette):
    """imwrite_indexed (:166-173): a 2-D uint8 label map as an indexed PNG."""
    from PIL import Image
    if np.atleast_3d(array).shape[2] != 1:
        raise ValueError("saving indexed PNGs requires a 2-D array")
    im = Image.fromarray(array)
    im.putpalette(np.asarray(color_palette, dtype=np.uint8).ravel())
    im.save(filename, format="PNG")
