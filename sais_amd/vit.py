"""DINO ViT-S/16 spatial encoder on MI355X — drop-in for the reference's SAIS/scripts/dino-main/vision_transformer.py
(`vit_small`, `VisionTransformer.forward` :209-214, `get_last_selfattention` :216-223, `get_intermediate_layers` :225-233) with
the same parameter names / shapes (150-tensor state_dict), so `dino_deitsmall16_pretrain.pth` loads strictly.

Every block runs as hand-written gfx950 kernels through the C ABI (include/sais_hip.h):
  LN -> [MFMA GEMM qkv] -> [attention] -> [MFMA GEMM proj + residual] -> LN -> [MFMA GEMM fc1 + GELU] -> [MFMA GEMM fc2 + residual]
with bf16 MFMA operands, fp32 accumulation, fp32 residual stream and fp32 LN/softmax statistics.  Backward is hand-written too
(dX GEMMs on pre-transposed bf16 weight shadows, dW GEMMs with transposed LDS reads, recompute-from-LSE attention backward);
parameter gradients are accumulated by the kernels directly into the flat gradient buffer that p.grad views.

Only the ViT-S geometry is built.  A pass over the blocks (`_forward_kernels`, `_backward_kernels`) has exactly one
of three forms, chosen once by `_pass_form`; everything that differs between them is a method of the form's class:
- resident (`_GroupPass`): resolution groups of 224 x 224 (197 tokens) / 96 x 96 (37 tokens: DINO's local crops), a head's keys
  and values resident in LDS (csrc/attn_vit.hip), one C call per block where it can.  Reached by `forward` at those sizes (both
  directions), `get_last_selfattention`, `get_intermediate_layers`, `probe_features` and DINO's multi-crop pass (dino.py).
- streaming (`_GroupPass` with `streaming`): uniform groups of any H x W in multiples of the patch size up to 4097 tokens; keys
  and values move through LDS in tiles (csrc/attn_any.hip, backward csrc/attn_any_bwd.hip), patchify_rect.  Reached by
  `dense_features`, `retrieval_features` and `cls_attention` (which ends in the CLS row of the last softmax, csrc/attnviz.hip) on
  a tensor, by `forward` under grad at any other size, by a multi-crop pass with such a group, and by EVERY pass of
  `vit_small(patch_size=8)` (ViT-S/8, inference only: the 8 x 8 gather of csrc/vit8.hip, the patch GEMM at K = 192, a 28 x 28
  positional grid; its CLS-only last block past the 200 tokens of attn_cls.hip takes sais_vit_attn_cls_fwd_any).
- segmented (`_SegPass`, patch 16): frames of DIFFERENT sizes, each a segment of the stacked token rows (csrc/attn_seg.hip,
  vit_seg.SegPlan); the launch list does not depend on the number of frames or shapes.  Reached by a LIST given to
  `dense_features`, `retrieval_features(cls_only=True)` or `forward` (under grad a training pass; without, the retrieval bits).
DropPath (vision_transformer.py:27-46: train() only, rates linspace(0, drop_path_rate, depth)) is a per-row scale in the epilogues
of the residual GEMMs; the keep draws come from Philox (`drop_path_seed`, this library's stream, not torch's):
`last_droppath_scales` holds what a forward used.
"""
import math
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .flat import ensure_flat
from .vit_seg import SegPlan

D, NTOK, HEADS, HID, PATCH_K = 384, 197, 6, 1536, 768
_PRUNE_Q = os.environ.get("SAIS_VIT_PRUNE_Q", "1") != "0"     # the CLS-only last block computes q for the CLS rows only
SIDES = {224: 197, 96: 37}          # frame sizes forward() takes -> tokens (the resident attention is instantiated per count)
MAX_DENSE_TOKENS = 4097             # dense_features: the streaming attention (sais_vit_attn_fwd_any) takes any count up to this
CLS_WAVE_MAX_TOKENS = 200           # the one-wave CLS-query attention (attn_cls.hip); beyond it: sais_vit_attn_cls_fwd_any


def _cubic_taps(t, A=-0.75):
    """The four Keys cubic-convolution weights (A = -0.75, what F.interpolate(mode='bicubic') uses) of the taps at
    floor(x) - 1 .. floor(x) + 2 for fractional offsets t = x - floor(x); t: [n] -> [n, 4]."""
    def near(x):           # |x| <= 1
        return ((A + 2) * x - (A + 3)) * x * x + 1
    def far(x):            # 1 < |x| < 2
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return np.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], axis=1)


def pos_axis_matrix(side_in, n0):
    """interpolate_pos_encoding (vision_transformer.py:174-194) along one axis, f64 [n0, side_in]: F.interpolate(scale_factor=
    (n0 + 0.1) / side_in, mode='bicubic', align_corners=False) samples at (dst + 0.5) / scale - 0.5 with border-clamped taps
    (clamped taps add up)."""
    scale = (n0 + 0.1) / side_in
    n_out = int(math.floor(side_in * scale))
    if n_out != n0:
        raise ValueError(f"interpolate_pos_encoding: {n_out} != {n0} (vision_transformer.py:191)")
    x = (np.arange(n_out) + 0.5) / scale - 0.5
    x0 = np.floor(x)
    taps = _cubic_taps(x - x0)
    M = np.zeros((n_out, side_in))
    for k in range(4):
        idx = np.clip(x0.astype(np.int64) + k - 1, 0, side_in - 1)
        np.add.at(M, (np.arange(n_out), idx), taps[:, k])
    return M


def pos_interp_matrix(side_in, w, h, patch=16):
    """interpolate_pos_encoding (vision_transformer.py:174-194) as a matrix: [w0 * h0, side_in^2] with
    patch_pos(w, h) = M @ patch_pos(224): the Kronecker product of the two per-axis maps (pos_axis_matrix; first axis = the
    first index of the 14 x 14 grid)."""
    return np.kron(pos_axis_matrix(side_in, w // patch), pos_axis_matrix(side_in, h // patch))


class _Attention(nn.Module):
    def __init__(self):
        super().__init__()
        self.qkv = nn.Linear(D, 3 * D, bias=True)
        self.proj = nn.Linear(D, D)


class _Mlp(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = nn.Linear(D, HID)
        self.fc2 = nn.Linear(HID, D)


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.norm1 = nn.LayerNorm(D, eps=1e-6)
        self.attn = _Attention()
        self.norm2 = nn.LayerNorm(D, eps=1e-6)
        self.mlp = _Mlp()


class _PatchEmbed(nn.Module):
    def __init__(self, patch_size=16):
        super().__init__()
        self.proj = nn.Conv2d(3, D, kernel_size=patch_size, stride=patch_size)
        self.num_patches = (224 // patch_size) ** 2
        self.patch_size = patch_size


def _trunc_normal_(t, std=0.02):
    # utils.trunc_normal_ (dino-main/utils.py:513-551) with a=-2, b=2
    return nn.init.trunc_normal_(t, mean=0.0, std=std, a=-2.0, b=2.0)


def _empty(dtype, dev):
    return lambda *s: torch.empty(*s, dtype=dtype, device=dev)


def _row_groups(imgs, patch=16):
    """One dict per resolution group: frames, tokens, its row / patch-row / frame offset in the stacked tensors and the same
    ranges as slices (`rows`, `prows`, `frames`), the interpolation map (set by the embedding).  Returns also the three totals."""
    groups, off, poff, foff = [], 0, 0, 0
    for im in imgs:
        Fr, ntok = im.shape[0], 1 + (im.shape[2] // patch) * (im.shape[3] // patch)
        n, npat = Fr * ntok, Fr * (ntok - 1)
        groups.append(dict(Fr=Fr, ntok=ntok, off=off, poff=poff, foff=foff, interp=None, rows=slice(off, off + n),
                           prows=slice(poff, poff + npat), frames=slice(foff, foff + Fr)))
        off, poff, foff = off + n, poff + npat, foff + Fr
    return groups, off, poff, foff


def _rows(t, g):
    """Group g's rows of a stacked [M, ...] tensor: the tensor itself when g is the only group (a view costs the host a few
    microseconds, twice per block in passes that are bound by the launch rate)."""
    return t if t.shape[0] == g["Fr"] * g["ntok"] else t[g["rows"]]


class _GroupPass:
    """The form of a pass over resolution groups: resident, or `streaming` (another patch gather and attention entry).  A form
    owns the totals, the embedding, the DropPath draw, a block's `lse`, its attention and the norm of the CLS rows, both ways."""
    seg = None

    def __init__(self, model, rows, streaming):
        self.m, self.streaming = model, streaming
        self.groups, self.M, self.NP, self.Ftot = rows
        self.resident = not streaming                    # (the streaming pass has never taken the fused-MLP switch)
        self.one_call = not streaming and len(self.groups) == 1      # a block's C call sequences ONE group's resident attention

    def record(self):                                    # in `saved`: the form for the backward, the rest for other readers
        return {"form": self, "groups": self.groups, "M": self.M, "Ftot": self.Ftot, "streaming": self.streaming, "seg": self.seg}

    def cls_only(self, save):
        """May the last block run on the CLS rows only?  Saved: while sais_vit_attn_cls_bwd (one wave) holds every group."""
        return not (save and any(g["ntok"] > CLS_WAVE_MAX_TOKENS for g in self.groups))

    def embed_fwd(self, pl, imgs):
        """Patchify, patch GEMM (+ bias + positional table) and CLS rows per group -> (patches bf16 [NP, K], x f32 [M, 384])."""
        m, f, K = self.m, self.m.flat, self.m.patch_k
        gather = ops.patchify_rect8 if m.patch == 8 else ops.patchify_rect if self.streaming else ops.patchify
        patches, x = pl.e16(self.NP, K), pl.e32(self.M, D)
        for im, g in zip(imgs, self.groups):
            Fr, ntok = g["Fr"], g["ntok"]
            pg = patches[g["prows"]]
            xg = x[g["rows"]].view(Fr, ntok, D)
            gather(im, pg)
            pos, g["interp"] = m._pos_table(im.shape[2], im.shape[3], pl.dev)
            ops.gemm_nt(pg, f.w("patch_embed.proj.weight").view(D, K), L.EPI_PATCH_F32, xg,
                        bias=f.w32("patch_embed.proj.bias"), aux=pos, grp=(ntok - 1, ntok, 1))
            ops.vit_cls_rows(f.w32("cls_token"), pos, xg, Fr, ntok)
        return patches, x

    def embed_bwd(self, dx, dpatch):
        f = self.m.flat
        for g in self.groups:
            Fr, ntok = g["Fr"], g["ntok"]
            dxg, dpg = dx[g["rows"]], dpatch[g["prows"]]
            if g["interp"] is None:
                ops.vit_embed_bwd(dxg, Fr, f.g("cls_token"), f.g("pos_embed"), dpg)
            else:                                   # through the transpose of the bicubic map (autograd of :174-194)
                dpos = torch.zeros(ntok, D, dtype=torch.float32, device=dx.device)
                ops.vit_embed_bwd(dxg, Fr, f.g("cls_token"), dpos, dpg, ntok=ntok)
                ops.pos_interp_bwd(g["interp"], dpos, f.g("pos_embed").view(NTOK, D))

    def droppath_draw(self, dev):
        """DropPath (train mode): row scales keep_f / (1 - p_i) for the 2 x depth residual branches, one Philox draw per
        frame and branch; branch 2i = attention of block i, 2i + 1 = its MLP.  f32 [2 x depth, M]."""
        m, parts = self.m, []
        m._droppath_state(dev)
        for g in self.groups:                            # one advance + draw per group (what separate passes would do)
            ops.rng_advance(m._rng)
            parts.append(ops.droppath_scales(m._dp_rates, g["Fr"], g["ntok"], m._rng))
        m.last_droppath_scales = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        return m.last_droppath_scales

    def lse(self, pl):
        return [pl.e32(g["Fr"], HEADS, g["ntok"]) if pl.save else None for g in self.groups]

    def qkv_fwd(self, i, b):
        f, p = self.m.flat, f"blocks.{i}."
        ops.gemm_nt(b["xn1"], f.w(p + "attn.qkv.weight"), L.EPI_BIAS_BF16, b["qkv"], bias=f.w32(p + "attn.qkv.bias"))

    def attn_fwd(self, pl, i, b, want_probs=False):
        """qkv and the attention of block i per group; want_probs (get_last_selfattention): it also writes its probabilities f32
        [frames, heads, ntok, ntok], which are returned (one group)."""
        self.qkv_fwd(i, b)
        probs = None
        for g, lg in zip(self.groups, b["lse"]):
            if want_probs:
                probs = pl.e32(g["Fr"], HEADS, g["ntok"], g["ntok"])
            qkv, ao = _rows(b["qkv"], g), _rows(b["ao"], g)
            if self.streaming:
                ops.vit_attn_fwd_any(qkv, g["Fr"], g["ntok"], ao, lg)
            else:
                ops.vit_attn_fwd(qkv, g["Fr"], ao, lg, probs, ntok=g["ntok"])
        return probs

    def attn_bwd(self, s, dao, dqkv):
        for g, lg in zip(self.groups, s["lse"]):
            r = g["rows"]
            if self.streaming:
                ops.vit_attn_bwd_any(s["qkv"][r], dao[r], s["ao"][r], lg, g["Fr"], g["ntok"], dqkv[r])
            else:
                ops.vit_attn_bwd(s["qkv"][r], dao[r], s["ao"][r], lg, None, g["Fr"], dqkv[r], ntok=g["ntok"])

    def cls_norm_fwd(self, x, reps, mean=None, rstd=None):
        """The final norm of x's CLS rows (row stride = ntok * 384) into reps [frames, 384]; returns what the norm read."""
        for g in self.groups:
            fr = g["frames"]
            ops.layernorm_fwd(x[g["rows"]], g["Fr"], g["ntok"] * D, *self.m._norm_p(), y32=reps[fr],
                              mean=None if mean is None else mean[fr], rstd=None if rstd is None else rstd[fr],
                              ldy32=reps.stride(0))
        return x

    def cls_norm_bwd(self, saved, dreps, dx):
        f = self.m.flat
        for g in self.groups:
            r, fr = g["rows"], g["frames"]
            ops.layernorm_bwd(saved["x_final"][r], g["ntok"] * D, saved["meanN"][fr], saved["rstdN"][fr], f.w32("norm.weight"),
                              g["Fr"], dy32=dreps[fr], dx32=dx[r], lddx32=g["ntok"] * D, dgamma=f.g("norm.weight"),
                              dbeta=f.g("norm.bias"))


class _SegPass(_GroupPass):
    """The form of a segmented pass (patch 16): a streaming pass in which every frame is a segment of the stacked rows (`seg`, a
    SegPlan on the device).  The embedding, the attention and the CLS gather / scatter are one launch each over all segments,
    both ways, and the last block runs on every row (the one-wave CLS kernels take one token count per launch)."""

    def __init__(self, model, rows, seg):
        super().__init__(model, rows, True)
        self.seg = seg

    cls_only = staticmethod(lambda save: False)

    def embed_fwd(self, pl, imgs):
        """Four launches whatever the frames: the pixels packed, one gather, the patch GEMM with its bias, and the token rows
        (CLS rows, patch rows + the positional table interpolated per segment from two per-axis tap matrices)."""
        f, seg = self.m.flat, self.seg
        pixels = imgs[0].reshape(-1) if len(imgs) == 1 else torch.cat([im.reshape(-1) for im in imgs])
        patches, pe, x = pl.e16(self.NP, PATCH_K), pl.e32(self.NP, D), pl.e32(self.M, D)
        ops.patchify_seg(pixels, seg, patches)
        ops.gemm_nt(patches, f.w("patch_embed.proj.weight").view(D, PATCH_K), L.EPI_BIAS_F32, pe,
                    bias=f.w32("patch_embed.proj.bias"))
        ops.vit_embed_seg(pe, f.w32("cls_token"), f.w32("pos_embed"), seg, x)
        return patches, x

    def embed_bwd(self, dx, dpatch):                     # through the per-axis taps: no [hw, 196] map
        ops.vit_embed_bwd_seg(dx, self.seg, self.m.flat.g("cls_token"), self.m.flat.g("pos_embed"), dpatch)

    def droppath_draw(self, dev):
        """ONE advance and one launch that draws per segment in list order (`last_droppath_frame_scales`, f32 [2 x depth, nseg]),
        expanded to the rows by one more (f32 [2 x depth, M])."""
        m = self.m
        m._droppath_state(dev)
        ops.rng_advance(m._rng)
        per = m.last_droppath_frame_scales = ops.droppath_scales(m._dp_rates, self.seg.nseg, 1, m._rng)
        m.last_droppath_scales = ops.vit_rows_expand_seg(per, self.seg)
        return m.last_droppath_scales

    def lse(self, pl):                                   # segment s owns [6, ntok] at 6 row0 of one tensor
        return [pl.e32(HEADS * self.M) if pl.save else None]

    def attn_fwd(self, pl, i, b, want_probs=False):
        self.qkv_fwd(i, b)
        ops.vit_attn_fwd_seg(b["qkv"], self.seg, b["ao"], b["lse"][0])

    def attn_bwd(self, s, dao, dqkv):
        ops.vit_attn_bwd_seg(s["qkv"], dao, s["ao"], s["lse"][0], self.seg, dqkv)

    def cls_norm_fwd(self, x, reps, mean=None, rstd=None):
        """The CLS rows gathered (sais_vit_cls_gather_seg), then one norm launch over them."""
        cls = torch.empty(self.Ftot, D, dtype=torch.float32, device=x.device)      # (Ftot: one segment per frame)
        ops.vit_cls_gather_seg(x, self.seg, cls)
        ops.layernorm_fwd(cls, self.Ftot, D, *self.m._norm_p(), y32=reps, mean=mean, rstd=rstd, ldy32=reps.stride(0))
        return cls

    def cls_norm_bwd(self, saved, dreps, dx):
        """On the gathered [nseg, 384] rows, then scattered to the CLS rows (sais_vit_cls_scatter_seg)."""
        f, seg = self.m.flat, self.seg
        dcls = torch.empty(seg.nseg, D, dtype=torch.float32, device=dx.device)
        ops.layernorm_bwd(saved["x_final"], D, saved["meanN"], saved["rstdN"], f.w32("norm.weight"), seg.nseg, dy32=dreps,
                          dx32=dcls, dgamma=f.g("norm.weight"), dbeta=f.g("norm.bias"))
        ops.vit_cls_scatter_seg(dcls, seg, dx)


class _PendingDW:
    """Weight gradients of G blocks in ONE grouped launch (ops.dw_group, LABNOTES R6.8).  A deferred block leaves here what that
    launch reads — the records of its C call (`calls`) or its four (p, q, dW, db) items (`items`) — and these keep its operands
    alive until then (its du / d(mid) / dqkv, the bf16 gradient that entered it, the saved activations).  `extra`: the k / v
    item of the CLS-only last block, which rides in the first launch (4 more tiles)."""

    def __init__(self, model, saved, G, hooked):
        self.model, self.saved = model, saved
        self.takes_extra = G > 1 and not hooked
        self.calls, self.items, self.extra, self.blocks = [], [], [], []

    def flush(self):
        if self.calls:
            ops.vit_blocks_dw([c[:3] for c in self.calls], extra=self.extra)
        elif self.items or self.extra:            # (extra alone: no block below the CLS-only one, depth 1)
            ops.gemm_tn_grouped(self.items + self.extra, self.saved["M"])
        for j in self.blocks:
            self.model._block_finished(self.saved, j)
        self.calls, self.items, self.extra, self.blocks = [], [], [], []


class _ViTFn(torch.autograd.Function):
    """Whole-ViT forward/backward as one autograd node.  Parameter gradients are written by the HIP
    kernels into model.flat.grad (p.grad views) as a side effect; `anchor` only keeps the node alive."""

    @staticmethod
    def forward(ctx, model, x, anchor, streaming=False, seg=None):       # seg: x is a list, one segmented pass
        reps, ctx.saved = model._forward_kernels(x, save=True, streaming=streaming, seg=seg)
        ctx.model = model
        return reps

    @staticmethod
    def backward(ctx, dreps):
        ctx.model._backward_kernels(ctx.saved, dreps.contiguous())
        ctx.saved = None
        return None, None, None, None, None


class VisionTransformer(nn.Module):
    def __init__(self, img_size=[224], patch_size=16, in_chans=3, num_classes=0, embed_dim=384, depth=12,
                 num_heads=6, mlp_ratio=4., qkv_bias=True, drop_path_rate=0., **kwargs):
        super().__init__()
        if (in_chans, embed_dim, num_heads, int(embed_dim * mlp_ratio), img_size[0], num_classes) != \
                (3, D, HEADS, HID, 224, 0) or not qkv_bias or patch_size not in (16, 8):
            raise NotImplementedError("the MI355X kernels implement the ViT-S/16 @224 geometry only (and ViT-S/8 for inference)")
        # patch 16: training and inference.  patch 8: inference only, every method on the streaming launch list
        self.patch = patch_size
        self.grid0 = 224 // patch_size               # side of the positional grid: 14 or 28
        self.ntok0 = 1 + self.grid0 ** 2             # rows of pos_embed: 197 or 785
        self.patch_k = 3 * patch_size ** 2           # K of the patch GEMM: 768 or 192
        self.num_features = self.embed_dim = embed_dim
        self.depth = depth
        self.drop_path_rate = drop_path_rate        # identity in eval(); per-sample stochastic depth in train()
        self.drop_path_seed = 0
        # forward() returns norm(x)[:, 0] (:212-214): of the LAST block only the CLS rows are ever read, so its row-local half
        # (proj, norm2, MLP, residual adds) runs on the CLS rows and its attention for the CLS query only; outputs and all
        # parameter gradients are unchanged.  SAIS_VIT_PRUNE_LAST=0 / prune_last_block = False computes every row.
        self.prune_last_block = os.environ.get("SAIS_VIT_PRUNE_LAST", "1") != "0"
        # one C call per Block (sais_vit_block_fwd / _bwd) instead of the per-launch Python sequence; SAIS_VIT_BLOCK_CALLS=0 off
        self.block_calls = os.environ.get("SAIS_VIT_BLOCK_CALLS", "1") != "0"
        self._bp, self._wsbuf = None, {}
        self._rng = None
        self.last_droppath_scales = None
        self.last_droppath_frame_scales = None       # a segmented pass: one column per frame, f32 [2 x depth, nseg]
        self.patch_embed = _PatchEmbed(patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, D))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.ntok0, D))
        self.blocks = nn.ModuleList([_Block() for _ in range(depth)])
        self.norm = nn.LayerNorm(D, eps=1e-6)
        self.head = nn.Identity()
        _trunc_normal_(self.pos_embed)
        _trunc_normal_(self.cls_token)
        for m in self.modules():                     # _init_weights, vision_transformer.py:165-172
            if isinstance(m, nn.Linear):
                _trunc_normal_(m.weight)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)
        self.flat = None
        self._anchor = None
        self._interp = {}                            # (H, W) -> device f32 [ntok - 1, grid0^2] bicubic map
        self.grad_ready_hook = None                  # callable(lo, hi): flat-grad slice [lo,hi) is final
        self._t_names = [f"blocks.{i}.{n}.weight" for i in range(depth) for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")]

    # ------------------------------------------------------------------ engine plumbing
    def _engine(self, device):
        if ensure_flat(self, device, transposed=self._t_names,
                       sentinels=("cls_token", "patch_embed.proj.weight", "blocks.0.attn.qkv.weight", "norm.weight",
                                  f"blocks.{self.depth - 1}.mlp.fc2.weight")):
            self._anchor = torch.zeros(1, device=device, requires_grad=True)
        self.flat.fresh()
        return self.flat

    def load_state_dict(self, *a, **k):
        if self.flat is not None:
            self.flat.mark_dirty()
        return super().load_state_dict(*a, **k)

    def sgd_step(self, lr, grad_scale=1.0):
        """Fused vanilla SGD over the whole flat buffer (prepare_model.py:566-567) + shadow refresh."""
        self.flat.sgd_step(lr, grad_scale)

    def block_grad_range(self, i):
        """[lo, hi) slice of the flat gradient buffer that belongs to block i."""
        f = self.flat
        lo = f.offsets[f"blocks.{i}.norm1.weight"]
        hi = f.offsets[f"blocks.{i + 1}.norm1.weight"] if i + 1 < self.depth else f.offsets["norm.weight"]
        return lo, hi

    # ------------------------------------------------------------------ public API (reference signatures)
    def forward(self, x):
        """norm(x)[:, 0] (:209-214), f32 [F, 384].  x a LIST or tuple of tensors [F_i, 3, H_i, W_i] of different sizes (patch 16;
        the checks and error texts of dense_features on a list): f32 [sum F_i, 384] in list order from ONE segmented pass.
        Under grad it is a training pass (every row of the last block computed); without, the bits of
        retrieval_features(list, cls_only=True)."""
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in (self.cls_token, self.norm.weight))
        if isinstance(x, (list, tuple)):
            items = self._check_list(x, "forward")
            if not need_grad:
                return self.retrieval_features(items, cls_only=True)
            self._engine(items[0].device)
            return _ViTFn.apply(self, items, self._anchor, True, self._seg_plan(items))
        if self.patch == 8 and need_grad:
            raise NotImplementedError("the patch-8 backbone is inference only (call it under torch.no_grad() or freeze its "
                                      "parameters): training runs on patch 16")
        # training, and a patch-8 model, take any H x W in multiples of the patch size
        x = self._check_input(x, "forward" if need_grad or self.patch == 8 else None)
        self._engine(x.device)
        if need_grad:
            return _ViTFn.apply(self, x, self._anchor, self.streaming_pass([x]))
        return self._forward_kernels(x, save=False, streaming=self.patch == 8)[0]

    @staticmethod
    def streaming_pass(imgs):
        """True iff a training pass over these resolution groups is a streaming one: some group is not a square side of SIDES.
        Every group of such a pass (a 224 x 224 one included) takes patchify_rect, sais_vit_attn_fwd_any and sais_vit_attn_bwd_any."""
        return any(im.shape[2] != im.shape[3] or im.shape[2] not in SIDES for im in imgs)

    def get_last_selfattention(self, x):
        if self.patch == 8:
            raise NotImplementedError("get_last_selfattention (the [F, 6, N, N] tensor) is a patch-16 call at 224 x 224 / 96 x 96; "
                                      "cls_attention returns its CLS row at any size")
        x = self._check_input(x)
        self._engine(x.device)
        return self._forward_kernels(x, save=False, end="probs")[0]

    def _last_norms(self, x, n, streaming, view=None):
        """norm(x) after each of the last n blocks, oldest first, each normalised (one launch, f32 [M, 384]) before the next block
        overwrites the stream: n tensors [F, ntok, 384]; x a checked list (one segmented pass): n times view(stacked tensor)."""
        first, out, Fr = self.depth - self._check_n(n), [], len(x)
        view = view or (lambda y: y.view(Fr, -1, D))

        def tap(i, xs):
            if i >= first:
                y = torch.empty(xs.shape[0], D, dtype=torch.float32, device=xs.device)
                ops.layernorm_fwd(xs, xs.shape[0], D, *self._norm_p(), y32=y)
                out.append(view(y))
        self._engine(x[0].device if isinstance(x, list) else x.device)
        self._forward_kernels(x, save=False, end="blocks", tap=tap, streaming=streaming,
                              seg=self._seg_plan(x) if isinstance(x, list) else None)
        return out

    def _check_n(self, n):
        n = int(n)
        if not 1 <= n <= self.depth:
            raise ValueError(f"n = {n} must be in [1, {self.depth}]")
        return n

    def _norm_p(self):                               # the final LayerNorm's (gamma, beta, eps)
        return self.flat.w32("norm.weight"), self.flat.w32("norm.bias"), 1e-6

    @torch.no_grad()
    def get_intermediate_layers(self, x, n=1):
        """vision_transformer.py:225-233: norm(x) after each of the last n blocks, oldest first, as n tensors f32
        [F, 197, 384].  Inference only (runs under no_grad, nothing is saved for a backward); 224 x 224 frames only.  Every row
        of the last block is computed (no CLS-only tail)."""
        x = self._check_input(x, "get_intermediate_layers" if self.patch == 8 else None)      # patch 8: any size
        if self.patch != 8 and x.shape[-1] != 224:
            raise ValueError("get_intermediate_layers takes 224 x 224 frames")
        return self._last_norms(x, n, streaming=self.patch == 8)

    @torch.no_grad()
    def probe_features(self, x, n=4, avgpool=False):
        """The classifier input of the linear probe, f32 [F, dim] (eval_linear.py:166-170), inference only.
        avgpool = False: dim = 384 n, the CLS rows of norm(x) after the last n blocks, oldest first; the last 384 columns are
        forward()'s output (the CLS-only last block stays in use), each earlier slot is one LayerNorm launch over the strided
        CLS rows written straight into its columns.  avgpool = True: as the reference, only n = 1 (its torch.cat raises for
        n > 1), dim = 768 INTERLEAVED: column 2 j is CLS[j], column 2 j + 1 the mean of the patch tokens of norm(x)[j]."""
        n = int(n)
        if avgpool and n != 1:
            raise ValueError("avgpool_patchtokens needs n_last_blocks = 1: the reference's torch.cat (eval_linear.py:169) "
                             f"cannot join [F, {D * n}, 1] with [F, {D}, 1]")
        streaming = self.patch == 8                  # patch 8: any size, the streaming launch list
        x = self._check_input(x, "probe_features" if streaming else None)
        if not streaming and x.shape[-1] != 224:
            raise ValueError("probe_features takes 224 x 224 frames")
        n = self._check_n(n)
        self._engine(x.device)
        Fr, ntok = x.shape[0], 1 + (x.shape[2] // self.patch) * (x.shape[3] // self.patch)
        if avgpool:
            xs = self._forward_kernels(x, save=False, end="blocks", streaming=streaming)[0]
            feats = torch.empty(Fr, 2 * D, dtype=torch.float32, device=x.device)
            ops.vit_cls_avgpool_norm(xs, Fr, *self._norm_p(), feats, ntok=ntok)
            return feats
        if n == 1:
            return self._forward_kernels(x, save=False, streaming=streaming)[0]
        feats, first = torch.empty(Fr, D * n, dtype=torch.float32, device=x.device), self.depth - n

        def tap(i, xs):            # slots of the earlier blocks; the last slot is written by the pass itself (reps_out)
            if first <= i < self.depth - 1:
                ops.layernorm_fwd(xs, Fr, ntok * D, *self._norm_p(), y32=feats[:, (i - first) * D:], ldy32=D * n)
        self._forward_kernels(x, save=False, tap=tap, reps_out=feats[:, (n - 1) * D:], streaming=streaming)
        return feats

    @torch.no_grad()
    def dense_features(self, x, n=1):
        """get_intermediate_layers (vision_transformer.py:225-233) at ANY resolution: x f32 [F, 3, H, W] on the device, H and W
        multiples of 16 (not necessarily equal), 1 + (H/16)(W/16) <= 4097 tokens.  Returns n tensors f32 [F, 1 + hw, 384],
        oldest first: norm(x) after each of the last n blocks.  Inference only, every row of every block is computed, in a
        streaming pass (a 224 x 224 input too; dino-main/eval_video_segmentation.py runs it at 480 x 832: 1561 tokens).
        x a LIST or tuple of such tensors [F_i, 3, H_i, W_i] of different sizes (patch 16 only): ONE segmented pass over all
        frames.  Returns per requested layer a list of [F_i, 1 + hw_i, 384] views of one stacked tensor.  The checks and error
        texts are the single tensor's, per item; an empty list raises."""
        if not isinstance(x, (list, tuple)):
            return self._last_norms(self._check_input(x, "dense_features"), n, streaming=True)
        items = self._check_list(x, "dense_features")
        groups = _row_groups(items, self.patch)[0]
        return self._last_norms(items, n, True, lambda y: [y[g["rows"]].view(g["Fr"], g["ntok"], D) for g in groups])

    def _check_list(self, items, name):
        """A list of device tensors [F_i, 3, H_i, W_i] for one segmented pass: _check_input per item, with its errors."""
        if self.patch != 16:
            raise NotImplementedError(f"VisionTransformer.{name} on a list of frames of different sizes is a patch-16 pass: a "
                                      "patch-8 model takes one tensor per call")
        if len(items) == 0:
            raise ValueError(f"VisionTransformer.{name}: an empty list of frames")
        return [self._check_input(x, name) for x in items]

    @staticmethod
    def _seg_plan(items):
        """The SegPlan of a pass over these items on their device (one pinned copy): one segment per frame, in list order."""
        grids = [(im.shape[2] // 16, im.shape[3] // 16) for im in items for _ in range(im.shape[0])]
        return SegPlan(grids).to_device(items[0].device)

    @torch.no_grad()
    def retrieval_features(self, x, cls_only=False):
        """The Copydays descriptor (eval_copy_detection.py:166-175), f32 [F, 768], at ANY resolution: x as dense_features takes it
        (same checks, same errors).  Columns 0..383 are the CLS token of norm(x) after the last block, columns 384..767 the GeM
        pooling with exponent 4 of its patch tokens clamped at 1e-6 — the reference's torch.cat(dim=1), concatenated, not
        interleaved.  Inference only.  Launches: dense_features' for every block, then sais_vit_cls_gem_norm on the residual
        stream: the normed [F, N, 384] tensor is never written.  cls_only: f32 [F, 384], the first half alone (what
        eval_image_retrieval.py reads: model(x) at any resolution) — the blocks, then the form's norm over the CLS rows (the
        launch that writes the first half of the full descriptor, so the bits are the same); no GeM pass.
        x a LIST or tuple of tensors [F_i, 3, H_i, W_i] of different sizes (patch 16, cls_only=True only; the GeM half over
        segments is not built): one segmented pass, then its norm over the gathered CLS rows: f32 [sum F_i, 384] in list order.
        A frame's row agrees with the single-tensor call up to the rounding of the batch-dependent GEMM tiling and of the
        separable positional interpolation (sixteen f32 terms instead of one f32 GEMM row)."""
        many = isinstance(x, (list, tuple))
        x = self._check_list(x, "retrieval_features") if many else self._check_input(x, "retrieval_features")
        if many and not cls_only:
            raise NotImplementedError("retrieval_features on a list returns the CLS half only (cls_only=True): the GeM "
                                      "pooling over segments of different sizes is not built")
        self._engine(x[0].device if many else x.device)
        form, imgs = self._pass_form(x, True, self._seg_plan(x) if many else None, "blocks")
        xs = self._pass(form, imgs, False, "blocks")[0]
        feats = torch.empty(form.Ftot, D if cls_only else 2 * D, dtype=torch.float32, device=xs.device)
        if cls_only:                                 # every row of the last block, then the form's norm over the CLS rows
            form.cls_norm_fwd(xs, feats)
        else:
            ops.vit_cls_gem_norm(xs, form.Ftot, form.groups[0]["ntok"], *self._norm_p(), feats)
        return feats

    @torch.no_grad()
    def cls_attention(self, x):
        """get_last_selfattention(x)[:, :, 0, :] (vision_transformer.py:216-223) at ANY resolution: x as dense_features takes it
        (same checks, same errors), returns f32 [F, 6, 1 + hw]: the softmax row of the CLS query of the last block over all
        tokens, the CLS key included — what video_generation.py and visualize_attention.py read.  Inference only.  Launches:
        dense_features' for every block but the last, then the last block's norm1, the K third of its qkv GEMM over all rows,
        the Q third over the CLS rows only and sais_vit_cls_probs: no V, no attention output, no proj, no MLP, and no
        [F, 6, N, N] tensor (off 224 x 224 / 96 x 96 that one is not built: nothing in the reference reads it)."""
        x = self._check_input(x, "cls_attention")
        f, dev, Fr = self._engine(x.device), x.device, x.shape[0]
        xn = self._forward_kernels(x, save=False, end="norm1", streaming=True)[0]
        M, ntok = xn.shape[0], xn.shape[0] // Fr
        p = f"blocks.{self.depth - 1}."
        Wq, bq = f.w(p + "attn.qkv.weight"), f.w32(p + "attn.qkv.bias")
        k = torch.empty(M, D, dtype=torch.bfloat16, device=dev)
        q = torch.empty(Fr, D, dtype=torch.bfloat16, device=dev)
        ops.gemm_nt(xn, Wq[D:2 * D], L.EPI_BIAS_BF16, k, bias=bq[D:2 * D])
        ops.gemm_nt(xn.view(Fr, ntok, D)[:, 0], Wq[:D], L.EPI_BIAS_BF16, q, bias=bq[:D])
        probs = torch.empty(Fr, HEADS, ntok, dtype=torch.float32, device=dev)
        ops.vit_cls_probs(q, k, Fr, ntok, probs)
        return probs

    def _check_input(self, x, any_size=None):
        """forward()'s input as a contiguous f32 tensor.  any_size: the name of the caller that takes every H x W in multiples of
        the patch size (dense_features, cls_attention, forward under grad; every method of a patch-8 model) instead of the square
        sides of SIDES."""
        P = self.patch
        if any_size is None:
            if not x.is_cuda:
                raise L.SaisHipError("VisionTransformer.forward needs a device tensor: the HIP path has no CPU fallback")
            if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.shape[2] not in SIDES:
                raise ValueError(f"expected [F,3,S,S] with S in {sorted(SIDES)}, got {tuple(x.shape)}")
            return x.contiguous().float()
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise L.SaisHipError(f"VisionTransformer.{any_size} needs a device tensor: the HIP path has no CPU fallback")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1 or x.shape[2] < P or x.shape[3] < P or x.shape[2] % P or x.shape[3] % P:
            raise ValueError(f"expected [F,3,H,W] with H and W positive multiples of {P}, got {tuple(x.shape)}")
        H, W = x.shape[2], x.shape[3]
        ntok = 1 + (H // P) * (W // P)
        if ntok > MAX_DENSE_TOKENS:
            raise ValueError(f"{H} x {W} frames are {ntok} tokens; at most {MAX_DENSE_TOKENS}")
        return x.contiguous().float()

    def _pos_table(self, H, W, dev):
        """(positional table f32 [1 + (H/P)(W/P), 384], interpolation map or None) for H x W frames; the bicubic map is cached
        per (H, W).  The table is the parameter itself only at 224 x 224 (:177-178: as many patches AND a square frame — a
        448 x 112 frame at patch 8 has 784 patches and is interpolated)."""
        pos = self.flat.w32("pos_embed").view(self.ntok0, D)
        if H == W == 224:
            return pos, None
        Wm = self._interp.get((H, W))
        if Wm is None or Wm.device != dev:
            Wm = torch.from_numpy(pos_interp_matrix(self.grid0, H, W, patch=self.patch).astype(np.float32)).to(dev)
            self._interp[(H, W)] = Wm
        out = torch.empty(1 + Wm.shape[0], D, dtype=torch.float32, device=dev)
        ops.pos_interp_fwd(Wm, pos, out)
        return out, Wm

    # ------------------------------------------------------------------ forward kernels
    def _forward_kernels(self, img, save, end="reps", tap=None, reps_out=None, streaming=False, seg=None):
        """img: one [F,3,H,W] tensor, or a LIST of them with different sizes (DINO's multi-crop student, utils.py:611-630):
        the groups are then stacked along the token-row axis and every GEMM / LayerNorm of a block runs ONCE over all rows
        (44 160 rows in one launch fill the chip where 25 216 + 18 944 in two leave workgroup slots empty; what is per group is
        the form's).  Returns (result, saved).  `end` names where the pass stops and what the result is: "reps": after the
        final norm, reps f32 [sum F, 384] in group order; "probs": in the last block's attention, its probabilities
        (get_last_selfattention); "norm1": at the last block's norm1, its bf16 output [M, 384] (cls_attention); "blocks": after
        the last block, the residual stream f32 [M, 384], every row computed and no final norm.  tap(i, x): called after every
        block but a CLS-only last one with the residual stream the block left (without `save` the next block overwrites it);
        reps_out: a [sum F, 384] view (any row stride) that receives reps instead of a new tensor.  streaming, seg: which form
        the pass has (_pass_form; the module docstring); `saved` records the form and the backward follows it.  A streaming
        or segmented pass has no block-level C call and no fused-MLP kernel, in either direction."""
        form, imgs = self._pass_form(img, streaming, seg, end)
        return self._pass(form, imgs, save, end, tap, reps_out)

    def _pass_form(self, img, streaming, seg, end):
        """(the form of the pass `_forward_kernels` was asked for, its inputs as a list): the one place that tells resident,
        streaming and segmented apart, and the one that refuses an impossible combination."""
        imgs = list(img) if isinstance(img, (list, tuple)) else [img]
        rows = _row_groups(imgs, self.patch)
        if end == "probs" and len(rows[0]) > 1:
            raise ValueError("get_last_selfattention takes one resolution")
        if seg is None:
            return _GroupPass(self, rows, streaming), imgs
        if end not in ("blocks", "reps") or not streaming or self.patch != 16 or seg.M != rows[1]:
            raise NotImplementedError("the segmented pass is the patch-16 streaming pass to the last block or the final norm")
        return _SegPass(self, rows, seg), imgs

    def _pass(self, form, imgs, save, end="reps", tap=None, reps_out=None):
        """_forward_kernels on a form."""
        f, dev, groups, M, Ftot = self.flat, imgs[0].device, form.groups, form.M, form.Ftot
        # Every decision of the pass, taken once; inside the loop only "is this the last block" is left.
        pl = SimpleNamespace(form=form, groups=groups, M=M, Ftot=Ftot, dev=dev, save=save, e16=_empty(torch.bfloat16, dev),
                             e32=_empty(torch.float32, dev), reps_out=reps_out)
        # Large M (training step, big extraction batches): the N = 384 GEMMs run on the row-owning kernel with the FOLLOWING
        # LayerNorm in their epilogue (sais_gemm_ln_fwd: proj -> norm2, fc2 -> next norm1); block 0's norm1 and the final norm stay
        pl.fused = fused = M >= ops.ROW_GEMM_MIN_M
        # the CLS-only tail runs its [frames, 384] GEMMs on the split-K small-M kernel (SAIS_EPI_RAW_SLABS_F32: M < 8192 only), so a
        # pass with 8192 or more FRAMES computes the last block on every row like the others (`saved` records
        # pruned=False, the backward follows it), and so does a form without a CLS-only tail for this pass (form.cls_only)
        pl.prune = end == "reps" and self.prune_last_block and Ftot < ops.ROW_GEMM_MIN_M and form.cls_only(save)
        pl.prune_q = pl.prune and len(groups) == 1 and _PRUNE_Q
        pl.mlp_fused = form.resident and ops.mlp_fused_enabled(M)
        # One C call per Block (sais_vit_block_fwd: the launches of _block_fwd_launches, sequenced by the library) whenever nothing
        # needs the per-launch view: no HIP-event instrumentation (bench.py's roofline pass), a form that has one
        pl.block_call = self.block_calls and ops.TIMER is None and form.one_call and fused and not pl.mlp_fused
        patches, x = form.embed_fwd(pl, imgs)
        draw = self.training and self.drop_path_rate > 0 and end != "probs"
        pl.dp = dp = form.droppath_draw(dev) if draw else None
        saved = dict(form.record(), patches=patches, blocks=[], dp=dp, pruned=False) if save else None
        b = ln1 = None                                   # the block's tensors; (xn, mean1, rstd1) of its norm1
        # norm1's outputs for a block: its own with `save`, else one xn for the whole pass and no statistics
        norm1_out = lambda: (pl.e16(M, D), pl.e32(M), pl.e32(M)) if save else ln1 or (pl.e16(M, D), None, None)
        for i in range(self.depth):
            p = f"blocks.{i}."
            last = i == self.depth - 1
            if i == 0 or not fused:                      # otherwise xn / mean1 / rstd1 came out of the previous fc2
                ln1 = norm1_out()
                ops.layernorm_fwd(x, M, D, f.w32(p + "norm1.weight"), f.w32(p + "norm1.bias"), 1e-6, y16=ln1[0], mean=ln1[1],
                                  rstd=ln1[2])
            if end == "norm1" and last:
                return ln1[0], None
            if pl.prune and last:                        # the CLS-only last block: its qkv here, the rest in _cls_tail_fwd
                xn = ln1[0]
                qkv = pl.e16(M, 3 * D) if save or b is None else b["qkv"]      # (with `save` it keeps its tensors itself)
                Wq, bq = f.w(p + "attn.qkv.weight"), f.w32(p + "attn.qkv.bias")
                if pl.prune_q:
                    # keys and values of every token, the query of the CLS rows only (the other rows' q columns of `qkv` stay
                    # unwritten: nothing reads them)
                    ops.gemm_nt(xn, Wq[D:], L.EPI_BIAS_BF16, qkv[:, D:], bias=bq[D:])
                    g0 = groups[0]
                    ops.gemm_nt(xn.view(g0["Fr"], g0["ntok"], D)[:, 0], Wq[:D], L.EPI_BIAS_BF16,
                                qkv.view(g0["Fr"], g0["ntok"], 3 * D)[:, 0, :D], bias=bq[:D])
                else:
                    ops.gemm_nt(xn, Wq, L.EPI_BIAS_BF16, qkv, bias=bq)
                reps, tail = self._cls_tail_fwd(pl, i, x, ln1, qkv)
                if save:
                    saved["blocks"].append(tail)
                    saved.update(x_final=tail["x_out"], meanN=tail["meanN"], rstdN=tail["rstdN"], pruned=True)
                return reps, saved
            if save or b is None:                        # without `save` one set of tensors serves every block
                b = self._block_buffers(pl, x, ln1)
            if end == "probs" and last:
                return form.attn_fwd(pl, i, b, want_probs=True), None
            nxt = norm1_out() if fused and not last else None
            x_out = pl.e32(M, D) if save else x          # (without `save` the residual stream is updated in place)
            rs_attn, rs_mlp = (None, None) if dp is None else (dp[2 * i], dp[2 * i + 1])
            if pl.block_call:
                g0 = groups[0]
                ws = None if save else ops.cached_workspace(self._wsbuf, L.OP_VIT_BLOCK_FWD, g0["Fr"], g0["ntok"], dev)
                ops.vit_block_fwd(self._block_params(i), g0["Fr"], g0["ntok"], b["xn1"], x, b["qkv"], b["ao"], b["lse"][0],
                                  b["x_mid"], b["xn2"], b["mean2"], b["rstd2"], b["h"], b["dgelu"], x_out,
                                  *(nxt or (None, None, None)), rs_attn, rs_mlp, ws)
            else:
                self._block_fwd_launches(pl, i, b, x_out, nxt, rs_attn, rs_mlp)
            if save:
                saved["blocks"].append(b)
            x, ln1 = x_out, nxt or ln1
            if tap is not None:
                tap(i, x)
        if end == "blocks":
            return x, saved
        reps = pl.e32(Ftot, D) if reps_out is None else reps_out
        meanN, rstdN = (pl.e32(Ftot), pl.e32(Ftot)) if save else (None, None)
        x_final = form.cls_norm_fwd(x, reps, meanN, rstdN)      # what the norm read (the gathered CLS rows or x)
        if save:
            saved.update(x_final=x_final, meanN=meanN, rstdN=rstdN)
        return reps, saved

    def _droppath_state(self, dev):
        """The Philox state and the per-branch rates on the device, made on first use."""
        if self._rng is None or self._rng.device != dev:
            self._rng = ops.rng_state(self.drop_path_seed, dev)
            rates = torch.linspace(0, self.drop_path_rate, self.depth).repeat_interleave(2)      # :150
            self._dp_rates = rates.to(dev, torch.float32)

    @staticmethod
    def _block_buffers(pl, x, ln1):
        """The tensors of one block, for the C call or the launch list; with `save` this dict is what the backward gets.  Without,
        the stream is updated in place and only the launch list needs h (the C call keeps GELU(u) in its workspace)."""
        M, save, e16, e32 = pl.M, pl.save, pl.e16, pl.e32
        return dict(x_in=x, mean1=ln1[1], rstd1=ln1[2], xn1=ln1[0], qkv=e16(M, 3 * D), ao=e16(M, D),
                    lse=pl.form.lse(pl), x_mid=e32(M, D) if save else x, mean2=e32(M) if save else None,
                    rstd2=e32(M) if save else None,
                    xn2=e16(M, D), dgelu=ops.gelu_grad_buffer(M, HID, pl.dev) if save else None,
                    h=e16(M, HID) if save or not pl.block_call else None)

    def _block_fwd_launches(self, pl, i, b, x_out, nxt, rs_attn, rs_mlp):
        """One block as its launches; nxt: where fc2's epilogue puts the next block's norm1, or None."""
        f, p, M, save = self.flat, f"blocks.{i}.", pl.M, pl.save
        x, x_mid, xn2, h, u = b["x_in"], b["x_mid"], b["xn2"], b["h"], b["dgelu"]
        pl.form.attn_fwd(pl, i, b)
        if pl.fused:
            ops.gemm_ln_fwd(b["ao"], f.w(p + "attn.proj.weight"), f.w32(p + "attn.proj.bias"), x, x_mid, xn2,
                            f.w32(p + "norm2.weight"), f.w32(p + "norm2.bias"), 1e-6, b["mean2"], b["rstd2"], rowscale=rs_attn)
        else:
            ops.gemm_nt(b["ao"], f.w(p + "attn.proj.weight"), L.EPI_BIAS_RESID_F32, x_mid,
                        bias=f.w32(p + "attn.proj.bias"), aux=x, rowscale=rs_attn)
            ops.layernorm_fwd(x_mid, M, D, f.w32(p + "norm2.weight"), f.w32(p + "norm2.bias"), 1e-6, y16=xn2,
                              mean=b["mean2"], rstd=b["rstd2"])
        xn, mean1, rstd1 = nxt or (None, None, None)
        q = f"blocks.{i + 1}." if nxt else None
        if pl.mlp_fused:
            # the whole MLP branch in ONE launch: fc1 + GELU (+ GELU') -> fc2 + residual (+ the next block's norm1); h is
            # written for the backward pass but never read back, and in inference it is not materialised at all
            ops.mlp_fwd(xn2, f.w(p + "mlp.fc1.weight"), f.w32(p + "mlp.fc1.bias"), f.w(p + "mlp.fc2.weight"),
                        f.w32(p + "mlp.fc2.bias"), x_mid, x_out, h=h if save else None, g=u, xn_out=xn,
                        gamma=f.w32(q + "norm1.weight") if nxt else None, beta=f.w32(q + "norm1.bias") if nxt else None,
                        eps=1e-6, mean=mean1, rstd=rstd1, rowscale=rs_mlp)
        else:
            ops.gemm_nt(xn2, f.w(p + "mlp.fc1.weight"), ops.epi_gelu_grad(M) if save else L.EPI_BIAS_GELU_BF16, h,
                        bias=f.w32(p + "mlp.fc1.bias"), out2=u)
            if nxt:
                ops.gemm_ln_fwd(h, f.w(p + "mlp.fc2.weight"), f.w32(p + "mlp.fc2.bias"), x_mid, x_out, xn,
                                f.w32(q + "norm1.weight"), f.w32(q + "norm1.bias"), 1e-6, mean1, rstd1, rowscale=rs_mlp)
            else:
                ops.gemm_nt(h, f.w(p + "mlp.fc2.weight"), L.EPI_BIAS_RESID_F32, x_out, bias=f.w32(p + "mlp.fc2.bias"),
                            aux=x_mid, rowscale=rs_mlp)

    def _block_params(self, i):
        """ctypes parameter blocks of the Blocks (pointers into the flat buffers), rebuilt when those are."""
        f = self.flat
        key = (f.flat.data_ptr(), f.grad.data_ptr(), f.w16.data_ptr(), 0 if f.wt_buf is None else f.wt_buf.data_ptr())
        if self._bp is None or self._bp[0] != key:
            self._bp = (key, [ops.vit_block_params(f, j, self.depth) for j in range(self.depth)])
        return self._bp[1][i]

    def _cls_tail_fwd(self, pl, i, x, ln1, qkv):
        """The last block from its qkv on, restricted to what forward() returns (the CLS rows): attention for the CLS query
        (sais_vit_attn_cls_fwd, one launch per resolution group; sais_vit_attn_cls_fwd_any for a token count its one wave per
        (frame, head) cannot hold: more than CLS_WAVE_MAX_TOKENS, a patch-8 model at 224 x 224), then proj + residual, norm2, fc1 + GELU, fc2 + residual and
        the final norm on [frames, 384] tensors (all groups together).  The residual input is the strided view x[::ntok]."""
        f, p = self.flat, f"blocks.{i}."
        groups, Ftot, dp, save, e16, e32 = pl.groups, pl.Ftot, pl.dp, pl.save, pl.e16, pl.e32
        ao = e16(Ftot, D)
        for g in groups:
            if g["ntok"] > CLS_WAVE_MAX_TOKENS:
                ops.vit_attn_cls_fwd_any(qkv[g["rows"]], g["Fr"], g["ntok"], ao[g["frames"]])
            else:
                ops.vit_attn_cls_fwd(qkv[g["rows"]], g["Fr"], ao[g["frames"]], g["ntok"])
        cls_rows = lambda t, w: [t[g["rows"]].view(g["Fr"], g["ntok"], *w)[:, 0] for g in groups]
        one = len(groups) == 1
        x_cls = cls_rows(x, (D,))[0] if one else torch.cat(cls_rows(x, (D,)))
        rs_attn = None if dp is None else torch.cat(cls_rows(dp[2 * i], ())).contiguous()
        rs_mlp = None if dp is None else torch.cat(cls_rows(dp[2 * i + 1], ())).contiguous()
        x_mid, xn2, x_out = e32(Ftot, D), e16(Ftot, D), e32(Ftot, D)
        mean2, rstd2 = (e32(Ftot), e32(Ftot)) if save else (None, None)
        # [frames, 384] outputs: 6 tiles of 128 x 128 — the K loop is cut over workgroups (deterministic split-K)
        ops.gemm_nt_splitk(ao, f.w(p + "attn.proj.weight"), 6, bias=f.w32(p + "attn.proj.bias"), rowscale=rs_attn, aux=x_cls,
                           out32=x_mid)
        ops.layernorm_fwd(x_mid, Ftot, D, f.w32(p + "norm2.weight"), f.w32(p + "norm2.bias"), 1e-6, y16=xn2, mean=mean2,
                          rstd=rstd2)
        h, u = e16(Ftot, HID), (ops.gelu_grad_buffer(Ftot, HID, x.device) if save else None)
        ops.gemm_nt(xn2, f.w(p + "mlp.fc1.weight"), ops.epi_gelu_grad(Ftot) if save else L.EPI_BIAS_GELU_BF16, h,
                    bias=f.w32(p + "mlp.fc1.bias"), out2=u)
        ops.gemm_nt_splitk(h, f.w(p + "mlp.fc2.weight"), 12, bias=f.w32(p + "mlp.fc2.bias"), rowscale=rs_mlp, aux=x_mid,
                           out32=x_out)
        reps = e32(Ftot, D) if pl.reps_out is None else pl.reps_out
        meanN, rstdN = (e32(Ftot), e32(Ftot)) if save else (None, None)
        ops.layernorm_fwd(x_out, Ftot, D, *self._norm_p(), y32=reps, mean=meanN, rstd=rstdN, ldy32=reps.stride(0))
        tail = dict(cls=True, x_in=x, mean1=ln1[1], rstd1=ln1[2], xn1=ln1[0], qkv=qkv, ao=ao, x_mid=x_mid, mean2=mean2, rstd2=rstd2,
                    xn2=xn2, dgelu=u, h=h, rs_attn=rs_attn, rs_mlp=rs_mlp, x_out=x_out, meanN=meanN, rstdN=rstdN) if save else None
        return reps, tail

    def _cls_tail_bwd(self, pl, saved, dreps, dx, dxa, dqkv, pend):
        """Backward of _cls_tail_fwd: the gradient enters on the CLS rows only.  Everything row-local stays on [frames, 384]
        tensors; the attention backward (sais_vit_attn_cls_bwd) writes the whole dqkv (dk, dv of every token, dq of the CLS
        rows, zeros elsewhere); the dX of qkv + norm1's backward then writes EVERY row of dx / dxa, taking the residual-stream
        gradient from the compact CLS tensor (dres_period) — no zero-filled [M, 384] buffer, no full-size cast.  With several
        resolution groups the two token-count-dependent launches run once per group on its rows."""
        i = self.depth - 1
        f, p = self.flat, f"blocks.{i}."
        s = saved["blocks"][i]
        groups, M, e16, Ftot = pl.groups, pl.M, pl.e16, saved["Ftot"]
        dx_c = torch.empty(Ftot, D, dtype=torch.float32, device=dreps.device)
        ops.layernorm_bwd(s["x_out"], D, s["meanN"], s["rstdN"], f.w32("norm.weight"), Ftot, dy32=dreps, dx32=dx_c,
                          dgamma=f.g("norm.weight"), dbeta=f.g("norm.bias"))
        if self.grad_ready_hook:
            self.grad_ready_hook(f.offsets["norm.weight"], f.numel)
        dxa_c, du, dxn, dxb_c, dao = e16(Ftot, D), e16(Ftot, HID), e16(Ftot, D), e16(Ftot, D), e16(Ftot, D)
        if s["rs_mlp"] is None:
            ops.cast_bf16(dx_c, dxa_c)
        else:
            ops.cast_bf16_rows(dx_c, s["rs_mlp"], dxa_c)
        ops.gemm_nt(dxa_c, f.wt16[p + "mlp.fc2.weight"], ops.epi_mul(Ftot), du, aux=s["dgelu"])
        ops.gemm_nt_splitk(du, f.wt16[p + "mlp.fc1.weight"], 12, out16=dxn)
        ops.layernorm_bwd(s["x_mid"], D, s["mean2"], s["rstd2"], f.w32(p + "norm2.weight"), Ftot, dy16=dxn, dres=dx_c, dx32=dx_c,
                          dx16=dxb_c, dgamma=f.g(p + "norm2.weight"), dbeta=f.g(p + "norm2.bias"), rowscale16=s["rs_attn"])
        ops.gemm_nt_splitk(dxb_c, f.wt16[p + "attn.proj.weight"], 6, out16=dao)
        for g in groups:
            ops.vit_attn_cls_bwd(s["qkv"][g["rows"]], dao[g["frames"]], g["Fr"], dqkv[g["rows"]], g["ntok"])
        compact = [
            (dxa_c, s["h"], f.g(p + "mlp.fc2.weight"), f.g(p + "mlp.fc2.bias")),
            (du, s["xn2"], f.g(p + "mlp.fc1.weight"), f.g(p + "mlp.fc1.bias")),
            (dxb_c, s["ao"], f.g(p + "attn.proj.weight"), f.g(p + "attn.proj.bias"))]
        gW, gb = f.g(p + "attn.qkv.weight"), f.g(p + "attn.qkv.bias")
        if len(groups) == 1 and _PRUNE_Q:      # dq is zero off the CLS rows: its weight gradient is a [frames, 384] GEMM too
            Fr, ntok = groups[0]["Fr"], groups[0]["ntok"]
            compact.append((dqkv.view(Fr, ntok, 3 * D)[:, 0, :D], s["xn1"].view(Fr, ntok, D)[:, 0], gW[:D], gb[:D]))
            ops.gemm_tn_grouped(compact, Ftot)
            kv = (dqkv[:, D:], s["xn1"], gW[D:], gb[D:])
            if pend.takes_extra:                      # rides in the first grouped launch of the blocks below (4 more tiles)
                pend.extra.append(kv)
            else:
                ops.gemm_tn_grouped([kv], M)
        else:
            ops.gemm_tn_grouped(compact, Ftot)
            ops.gemm_tn_grouped([(dqkv, s["xn1"], gW, gb)], M)
        dp = saved["dp"]
        rs_prev = None if dp is None or i == 0 else dp[2 * (i - 1) + 1]
        if pl.fused and all(g["Fr"] * g["ntok"] >= ops.ROW_GEMM_MIN_M for g in groups):
            for g in groups:
                r = g["rows"]
                ops.gemm_ln_bwd(dqkv[r], f.wt16[p + "attn.qkv.weight"], s["x_in"][r], s["mean1"][r], s["rstd1"][r],
                                f.w32(p + "norm1.weight"), dres=dx_c[g["frames"]], dres_period=g["ntok"], dx32=dx[r],
                                dx16=dxa[r], dgamma=f.g(p + "norm1.weight"), dbeta=f.g(p + "norm1.bias"),
                                rowscale16=None if rs_prev is None else rs_prev[r],
                                xn16=s["xn1"][r], beta=f.w32(p + "norm1.bias"))
        else:                                         # small M: scatter the CLS gradient into a zeroed residual-stream gradient
            dx.zero_()
            for g in groups:
                dx[g["rows"]].view(g["Fr"], g["ntok"], D)[:, 0].copy_(dx_c[g["frames"]])
            dxn_full = e16(M, D)
            ops.gemm_nt(dqkv, f.wt16[p + "attn.qkv.weight"], L.EPI_BIAS_BF16, dxn_full)
            ops.layernorm_bwd(s["x_in"], D, s["mean1"], s["rstd1"], f.w32(p + "norm1.weight"), M, dy16=dxn_full, dres=dx,
                              dx32=dx, dx16=dxa, dgamma=f.g(p + "norm1.weight"), dbeta=f.g(p + "norm1.bias"),
                              rowscale16=rs_prev)
        # (the k / v weight gradient above may still be pending in `pend`, which happens only without an ACTIVE hook: a hook that
        # carries active = False is then told about this block before that gradient is written — ADVICE r6 #3)
        self._block_finished(saved, i)

    # ------------------------------------------------------------------ backward kernels
    def _block_finished(self, saved, i):
        """Block i's backward is issued: drop what the forward saved; its gradient slice is final, DP all-reduce may start."""
        saved["blocks"][i] = None
        if self.grad_ready_hook:
            self.grad_ready_hook(*self.block_grad_range(i))

    def _backward_kernels(self, saved, dreps):
        f = self.flat
        f.attach_grads()
        dev = dreps.device
        form, dp, pruned = saved["form"], saved["dp"], saved["pruned"]      # (what the forward recorded)
        groups, M, e16 = form.groups, form.M, _empty(torch.bfloat16, dev)
        # Every decision of the pass, taken once (from this pass's own inputs, not from what the forward decided).
        fused = M >= ops.ROW_GEMM_MIN_M
        mlp_fused = form.resident and ops.mlp_fused_enabled(M)
        block_call = self.block_calls and ops.TIMER is None and form.one_call and fused and not mlp_fused
        # a data-parallel hook that all-reduces the blocks' gradients while the backward goes on (an idle one — GradSync in a world
        # of one — carries active = False)
        hooked = self.grad_ready_hook is not None and getattr(self.grad_ready_hook, "active", True)
        # blocks per weight-gradient launch (_PendingDW); 1: every block launches its own
        G = ops.dw_group(dp_hooks=hooked) if fused and M % 32 == 0 and not mlp_fused else 1
        pl = SimpleNamespace(form=form, groups=groups, M=M, e16=e16, fused=fused, mlp_fused=mlp_fused, defer=G > 1)
        pend = _PendingDW(self, saved, G, hooked)
        dxa = e16(M, D)                            # bf16 copy of the residual-stream gradient that enters a block
        # scratch of the launch list (the C call has its workspace; dqkv also serves the CLS-only block): dxb = the bf16 gradient at
        # a block's middle.  With deferred weight gradients du / dqkv / dxb are operands of the pending launch: a set per block
        shared = not (block_call or pl.defer)
        t = SimpleNamespace(dqkv=e16(M, 3 * D) if pruned or shared else None, du=e16(M, HID) if shared else None,
                            dxb=e16(M, D) if shared else None, dxn=None if block_call or fused else e16(M, D),
                            dao=None if block_call else e16(M, D))
        if pruned:                                  # every row of dx is WRITTEN by the last block's dX qkv + norm1' kernel
            dx = torch.empty(M, D, dtype=torch.float32, device=dev)
            self._cls_tail_bwd(pl, saved, dreps, dx, dxa, t.dqkv, pend)
        else:
            dx = torch.zeros(M, D, dtype=torch.float32, device=dev)
            self._final_norm_bwd(form, saved, dreps, dx, dxa)
        for i in reversed(range(self.depth - 1 if pruned else self.depth)):
            s = saved["blocks"][i]
            rs_attn = None if dp is None else dp[2 * i]                        # this block's attention branch
            rs_prev = None if dp is None or i == 0 else dp[2 * (i - 1) + 1]     # the MLP branch of block i - 1
            # deferred: dxa stays an operand of the pending launch, the NEXT block's bf16 gradient is written beside it
            dxa_out = e16(M, D) if pl.defer else dxa
            if block_call:
                g0, P = groups[0], self._block_params(i)
                ws = ops.cached_workspace(self._wsbuf, L.OP_VIT_BLOCK_BWD, g0["Fr"], g0["ntok"], dev, slot=len(pend.calls))
                a = ops.vit_block_bwd(P, g0["Fr"], g0["ntok"], s, dx, dxa, dxa_out, rs_attn, rs_prev, s["lse"][0], ws,
                                      defer_dw=pl.defer)
                if pl.defer:
                    pend.calls.append((P, a, ws, dxa, s))                      # dxa, s: kept alive for the launch
            else:
                self._block_bwd_launches(pl, i, s, dx, dxa, dxa_out, t, rs_attn, rs_prev, pend)
            dxa = dxa_out
            pend.blocks.append(i)
            if len(pend.blocks) == G or i == 0:        # (G = 1: nothing is pending, the block is just finished)
                pend.flush()
        pend.flush()
        self._embed_bwd(saved, dx)

    def _final_norm_bwd(self, form, saved, dreps, dx, dxa):
        """Backward of the final norm on the CLS rows into the (zeroed) residual-stream gradient, and its bf16 copy."""
        f, dp = self.flat, saved["dp"]
        form.cls_norm_bwd(saved, dreps, dx)
        # with DropPath the gradient that enters a branch is s dx (the residual stream keeps dx): the bf16 copies carry the
        # NEXT branch's scale — dxa feeds an MLP branch (2i + 1), dxb an attention branch (2i)
        if dp is None:
            ops.cast_bf16(dx, dxa)
        else:
            ops.cast_bf16_rows(dx, dp[2 * (self.depth - 1) + 1], dxa)
        if self.grad_ready_hook:
            self.grad_ready_hook(f.offsets["norm.weight"], f.numel)

    def _block_bwd_launches(self, pl, i, s, dx, dxa, dxa_out, t, rs_attn, rs_prev, pend):
        """One block's backward as its launches; its weight gradients are launched here or left to `pend`."""
        f, p, M, fused = self.flat, f"blocks.{i}.", pl.M, pl.fused
        if pl.defer:                                  # this block's gradient tensors are its own
            t.du, t.dqkv, t.dxb = pl.e16(M, HID), pl.e16(M, 3 * D), pl.e16(M, D)
        du, dqkv, dxb, dxn, dao = t.du, t.dqkv, t.dxb, t.dxn, t.dao
        # MLP branch
        if pl.mlp_fused:                              # dX of fc2 x GELU' -> dX of fc1 -> norm2's backward: ONE launch
            ops.mlp_bwd(dxa, f.wt16[p + "mlp.fc2.weight"], s["dgelu"], f.wt16[p + "mlp.fc1.weight"], du, s["x_mid"],
                        s["mean2"], s["rstd2"], f.w32(p + "norm2.weight"), dres=dx, dx32=dx, dx16=dxb,
                        dgamma=f.g(p + "norm2.weight"), dbeta=f.g(p + "norm2.bias"), rowscale16=rs_attn)
        elif fused:       # dX of fc1 with norm2's backward (+ residual gradient) in its epilogue
            ops.gemm_nt(dxa, f.wt16[p + "mlp.fc2.weight"], ops.epi_mul(M), du, aux=s["dgelu"])
            ops.gemm_ln_bwd(du, f.wt16[p + "mlp.fc1.weight"], s["x_mid"], s["mean2"], s["rstd2"],
                            f.w32(p + "norm2.weight"), dres=dx, dx32=dx, dx16=dxb, dgamma=f.g(p + "norm2.weight"),
                            dbeta=f.g(p + "norm2.bias"), rowscale16=rs_attn, xn16=s["xn2"], beta=f.w32(p + "norm2.bias"))
        else:
            ops.gemm_nt(dxa, f.wt16[p + "mlp.fc2.weight"], ops.epi_mul(M), du, aux=s["dgelu"])
            ops.gemm_nt(du, f.wt16[p + "mlp.fc1.weight"], L.EPI_BIAS_BF16, dxn)
            ops.layernorm_bwd(s["x_mid"], D, s["mean2"], s["rstd2"], f.w32(p + "norm2.weight"), M, dy16=dxn, dres=dx,
                              dx32=dx, dx16=dxb, dgamma=f.g(p + "norm2.weight"), dbeta=f.g(p + "norm2.bias"),
                              rowscale16=rs_attn)
        # attention branch
        ops.gemm_nt(dxb, f.wt16[p + "attn.proj.weight"], L.EPI_BIAS_BF16, dao)
        pl.form.attn_bwd(s, dao, dqkv)
        # all four weight / bias gradients of the block in one launch.  (A side stream for this launch was measured
        # in round 1: 20.4 vs 19.6 ms/step — both kernels fill the chip — and removed.)
        dw = [(dxa, s["h"], f.g(p + "mlp.fc2.weight"), f.g(p + "mlp.fc2.bias")),
              (du, s["xn2"], f.g(p + "mlp.fc1.weight"), f.g(p + "mlp.fc1.bias")),
              (dxb, s["ao"], f.g(p + "attn.proj.weight"), f.g(p + "attn.proj.bias")),
              (dqkv, s["xn1"], f.g(p + "attn.qkv.weight"), f.g(p + "attn.qkv.bias"))]
        if pl.defer:
            pend.items += dw
        else:
            ops.gemm_tn_grouped(dw, M)
        if fused:         # dX of qkv with norm1's backward in its epilogue
            ops.gemm_ln_bwd(dqkv, f.wt16[p + "attn.qkv.weight"], s["x_in"], s["mean1"], s["rstd1"],
                            f.w32(p + "norm1.weight"), dres=dx, dx32=dx, dx16=dxa_out, dgamma=f.g(p + "norm1.weight"),
                            dbeta=f.g(p + "norm1.bias"), rowscale16=rs_prev, xn16=s["xn1"], beta=f.w32(p + "norm1.bias"))
        else:
            ops.gemm_nt(dqkv, f.wt16[p + "attn.qkv.weight"], L.EPI_BIAS_BF16, dxn)
            ops.layernorm_bwd(s["x_in"], D, s["mean1"], s["rstd1"], f.w32(p + "norm1.weight"), M, dy16=dxn, dres=dx,
                              dx32=dx, dx16=dxa_out, dgamma=f.g(p + "norm1.weight"), dbeta=f.g(p + "norm1.bias"),
                              rowscale16=rs_prev)

    def _embed_bwd(self, saved, dx):
        """Backward of the embedding in the pass's form, then the patch projection's weight gradient over all rows."""
        f = self.flat
        dpatch = torch.empty(saved["patches"].shape[0], D, dtype=torch.bfloat16, device=dx.device)
        saved["form"].embed_bwd(dx, dpatch)
        # (the ping-pong 128 x 384 dW kernel is no better here: 6 wide tiles x 42 row splits, 77 us against 65-68 us)
        ops.gemm_tn(dpatch, saved["patches"], f.g("patch_embed.proj.weight").view(D, PATCH_K),
                    f.g("patch_embed.proj.bias"))
        if self.grad_ready_hook:
            self.grad_ready_hook(0, f.offsets["blocks.0.norm1.weight"])


def vit_small(patch_size=16, **kwargs):
    """vision_transformer.py:243-247."""
    return VisionTransformer(patch_size=patch_size, embed_dim=384, depth=kwargs.pop("depth", 12), num_heads=6,
                             mlp_ratio=4, qkv_bias=True, **kwargs)
