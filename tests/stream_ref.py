"""fp64 references, bars, exact-data recipes and case tables for the streaming kernels of the ViT step and the DINO objective
(csrc/norm.hip, misc.hip, dino.hip).  No GPU code; imported by test_stream_ref_host.py and test_stream_edges_gpu.py.

Every reference takes the tensors the kernel takes (fp32 / bf16, any device), widens them to fp64 on the CPU and returns fp64.
Scalars that cross the C ABI as `float` (eps, scale, lr, ...) are rounded to fp32 first (`f32`).  The bars:
  * a quantity an older test pins keeps that test's bar (the constants below), now measured against fp64;
  * results that grow with their inputs add the rounding of the fp32 result itself, 2 ulp32(|ref|);
  * hard LayerNorm rows: 4 x the error of torch's own fp32 CPU layer_norm on the same rows, the old bar as the floor;
  * LayerNorm mean: 17 2^-24 mean_k |x_k| + ulp32(|ref|), the kernel's 12 + 5 additions;
  * random-data sums: (terms + 8) 2^-24 sum |terms|, in fp64.
Integer recipes (values in [-4, 4], gamma in {0.5, 1, 2}, mean = 0 and rstd = 1 handed to the backward) make sums independent of
their order; each asserts its condition (`int_exact`) on the fp64 result.  The models at the end restate what a kernel computes
(never when), with the mutations the GPU cases have to notice."""
import math

import torch
import torch.nn.functional as F

import gemm_ref as G

D = 384
NAN = G.NAN
SENTINEL_IN = 1e30
EMB_CHUNKS = 4                                                   # csrc/misc.hip
U24 = 2.0 ** -24

# ------------------------------------------------------------------------------------------------ the old bars
Y32_ATOL = 2e-5                                                  # test_layernorm_fwd_bwd
DX32_ATOL, DX32_RTOL = 1e-4, 1e-4
BF16_ATOL, BF16_RTOL = 2e-2, 1e-2
RSTD_RTOL = 1e-4                                                 # test_gemm_ln_fwd
LSE_ATOL, LOSS_RTOL, DLOGITS_REL, CENTER_ATOL = 2e-5, 1e-5, 2e-5, 1e-7      # test_dino_loss_*
GELU_ATOL, DGELU_ATOL = 1e-6, 3e-6                               # test_gelu_l2norm_weightnorm_vs_torch
NORM_FWD, NORM_BWD_REL = 1e-6, 1e-5
POS_ATOL = 1e-5                                                  # test_pos_interp_kernels
ADAMW_ATOL, SGD_ATOL = 2e-6, 1e-6                                # test_adamw_clip_ema_vs_oracle, test_sgd_cast_transpose
GRAD_NORM_RTOL, GRAD_NORM_ATOL = 1e-5, 1e-9
# 1 / max(||z||, eps): <= 16 fmas per lane and 6 butterfly additions on positive terms (22 2^-24 on the sum, halved by the square
# root), the square root and the division: 13 2^-24, taken as 16
INV_RTOL = 16 * U24

# ------------------------------------------------------------------------------------------------ the GPU case lists
LN_FWD_ROWS = [1, 7, 8, 9, 8200]
LN_EPS = [1e-6, 1e-5]
LN_KINDS = ["plain", "offset1000", "offset100", "outlier", "small"]
LN_HARD = ("offset1000", "offset100", "outlier")
LN_BWD_ROWS = [1, 7, 9, 8200, 16391]                            # 1024 workgroups x 8 rows = 8192: one and two grid-stride rounds
LN_BWD_INT_ROWS = [9, 8200, 16391]
AVGPOOL_NTOK = [2, 8, 9, 37, 197]
PATCHIFY = [(side, fr) for side in (16, 96, 224) for fr in (1, 3)] + [(224, 57)]
EMBED_FRAMES = [1, 2, 3, 4, 5, 7, 9, 13]
EMBED_NTOK = [2, 37, 197]
SGD_N = [1, 3, 4, 5, 1023, 1025, 2097159]
GRID2048 = 2048 * 256                                            # grid_for (csrc/misc.hip): elements of one grid round
GRID4096 = 4096 * 256                                            # ew_grid (csrc/dino.hip), in float4
CAST_N = [1, 3, 255, 257, GRID2048 + 37]
CAST_ROWS = [(7, 5), (3, 384), (GRID2048 // 384 + 2, 384)]
TRANSPOSE = [(1, 1), (1, 384), (31, 33), (32, 32), (33, 31), (65, 37)]
LSE_N = [4, 4092, 4096, 4100, 8196]
LSE_KINDS = ["plain", "equal", "peak", "shifted"]
LOSS_N = [4, 1020, 1024, 1028, 4100]
LOSS_B = [1, 3]
LOSS_NCROPS = [2, 3, 10]
COLSUM_ROWS = [1, 2, 3, 4, 5, 7]
COLSUM_N = [4, 252, 256, 260]
CENTER_N = [4, 1020, 1024, 1028]
GELU_N = [4, 1020, 1028, 4 * GRID4096 + 4]
SPLIT3 = [(1, 4), (37, 252), (4100, 1028)]
ROW_DIMS = [4, 252, 256, 260, 512, 1020, 1024]
ROW_ROWS = [1, 3, 4, 5]
L2_EPS = [1e-12, 1.3e-8, 2.7e-5]
L2_KINDS = ["plain", "zero", "half_eps", "two_eps"]
POS_SIZES = [(96, 96), (224, 224), (96, 160), (16, 16)]         # (16, 16): one patch, the smallest map there is
POS_DIMS = [4, 384, 508, 512]
ADAMW_SIZES = [4, 1020, 1028, 8188, 8192, 8196, 24576, 65 * 8192 + 4]
ADAMW_CLIPS = [0.0, 1e-3, 1e9]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32(v):
    """a Python scalar as the C ABI's `float` sees it"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def d64(t):
    return None if t is None else t.detach().double().cpu()


def ulp32(ref):
    """spacing of fp32 at |ref| (fp64 tensor)"""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(ref), e - 24)


def ratio(got, ref, atol, rtol=0.0, ulps=0):
    """max |got - ref| / (atol + rtol |ref| + ulps ulp32(|ref|)); NaN when anything is NaN"""
    got, ref = d64(got), d64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    tol = atol + rtol * ref.abs() + (ulps * ulp32(ref) if ulps else 0.0)
    return float(((got - ref).abs() / tol).max())


def rel_l2(got, ref, denom=None):
    got, ref = d64(got), d64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).norm() / (ref if denom is None else d64(denom)).norm().clamp_min(1e-300))


def sum_bar(abs_terms, terms):
    """bar of a random-data sum of `terms` addends: (terms + 8) 2^-24 sum |terms|"""
    return (terms + 8) * U24 * abs_terms


def int_exact(*abs_sums):
    """the condition of an integer recipe: every sum of |terms| (an upper bound of every partial sum) is an integer below 2^24"""
    return all(bool(torch.equal(s, s.round())) and float(s.max()) < 2 ** 24 for s in abs_sums)


def strided_in(t, pad, off, rows_extra=0):
    """gemm_ref.padded for an INPUT: the gap holds 1e30, so a stray read shows in the result"""
    view, buf = G.padded(t, pad, off, rows_extra)
    buf.nan_to_num_(nan=SENTINEL_IN)
    return view, buf


def ints(shape, seed, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).float()


def gamma_int(seed):
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (D,), generator=gen(seed))]


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_rows(kind, rows, seed=0):
    x = torch.randn(rows, D, generator=gen(1000 + seed))
    if kind == "offset1000":
        x = 1000.0 + x
    elif kind == "offset100":
        x = 100.0 + 0.5 * x
    elif kind == "outlier":
        x[:, 17] += 300.0
    elif kind == "small":
        x = 1e-3 * x
    else:
        assert kind == "plain"
        x = 2.0 * x + 0.3
    return x


def ln_params(seed=0):
    return 1 + 0.1 * torch.randn(D, generator=gen(2000 + seed)), 0.1 * torch.randn(D, generator=gen(3000 + seed))


def ln_fwd(x, gamma, beta, eps):
    x = d64(x)
    mean = x.mean(-1)
    rstd = 1.0 / torch.sqrt(x.var(-1, unbiased=False) + f32(eps))
    return (x - mean[:, None]) * rstd[:, None] * d64(gamma) + d64(beta), mean, rstd


def ln_y_atol(x, gamma, beta, eps):
    """bar of y32: 4 x the error of torch's fp32 CPU layer_norm on these rows, at least the old bar"""
    xc, gc, bc = x.detach().float().cpu(), gamma.detach().float().cpu(), beta.detach().float().cpu()
    err = float((F.layer_norm(xc, (D,), gc, bc, f32(eps)).double() - ln_fwd(xc, gc, bc, eps)[0]).abs().max())
    return max(Y32_ATOL, 4 * err), err


def ln_mean_bar(x, mean_ref):
    return 17 * U24 * d64(x).abs().mean(-1) + ulp32(mean_ref)


def ln_bwd(dy, x, mean, rstd, gamma, dres=None):
    """autograd of y = (x - mean) rstd gamma + beta with the GIVEN mean / rstd: dx (+ dres), dgamma, dbeta and, for the sum bars,
    sum |terms| of dgamma and dbeta"""
    dy, x, g = d64(dy), d64(x), d64(gamma)
    xhat = (x - d64(mean)[:, None]) * d64(rstd)[:, None]
    gy = dy * g
    dx = d64(rstd)[:, None] * (gy - gy.mean(-1, keepdim=True) - xhat * (gy * xhat).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + d64(dres)
    return dx, (dy * xhat).sum(0), dy.sum(0), (dy * xhat).abs().sum(0), dy.abs().sum(0)


def cls_avgpool_norm(x, gamma, beta, eps):
    """x [frames, ntok, 384] -> [frames, 768]: column 2 j = norm(x)[:, 0, j], 2 j + 1 = mean over the patch rows"""
    fr, ntok, _ = x.shape
    y = ln_fwd(d64(x).reshape(fr * ntok, D), gamma, beta, eps)[0].reshape(fr, ntok, D)
    return torch.stack([y[:, 0], y[:, 1:].mean(1)], dim=-1).reshape(fr, 2 * D)


# ---- fp32 emulation of the statistics' summation order: lane l of a half-wave owns columns 128 i + 4 l .. + 3 (i = 0..2), adds
# its 12 values in register order, then the 32 lanes are combined by the xor butterfly 16, 8, 4, 2, 1 (csrc/row384.hpp)
def lanes(x):
    return x.reshape(x.shape[0], 3, 32, 4).permute(0, 2, 1, 3).reshape(x.shape[0], 32, 12)


def unlanes(v):
    return v.reshape(v.shape[0], 32, 3, 4).permute(0, 2, 1, 3).reshape(v.shape[0], D)


def _half_sum(s):
    idx = torch.arange(32)
    for o in (16, 8, 4, 2, 1):
        s = s + s[:, idx ^ o]
    return s


def _lane_sum(v):
    s = torch.zeros(v.shape[:2], dtype=torch.float32)
    for i in range(12):
        s = s + v[:, :, i]
    return s


def ln_emul(x, gamma, beta, eps, one_pass=False):
    """(y, mean, rstd) in fp32 in the kernel's order.  one_pass: var = E[x^2] - mean^2, the error the hard rows must notice."""
    v = lanes(x.detach().float().cpu())
    inv_d = torch.tensor(1.0 / D, dtype=torch.float32)
    mu = _half_sum(_lane_sum(v)) * inv_d
    if one_pass:
        var = _half_sum(_lane_sum(v * v)) * inv_d - mu * mu
    else:
        d = v - mu[:, :, None]
        var = _half_sum(_lane_sum(d * d)) * inv_d
    rs = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    gm, bt = lanes(gamma.detach().float().cpu()[None]), lanes(beta.detach().float().cpu()[None])
    return unlanes((v - mu[:, :, None]) * rs[:, :, None] * gm + bt), mu[:, 0], rs[:, 0]


def ln_fwd_model(xview, gamma, beta, eps, ld_ignored=False):
    """the forward over a strided view; ld_ignored: the row stride taken as the width"""
    if ld_ignored:
        xview = xview.as_strided(xview.shape, (D, 1), xview.storage_offset())
    return ln_fwd(xview, gamma, beta, eps)[0]


# ------------------------------------------------------------------------------------------------ embedding backward
def embed_bwd(dtok, dcls0, dpos0):
    """dtok [F, ntok, dim]: dcls0 + sum_f dtok[f, 0], dpos0 + sum_f dtok[f], the bf16 patch-gradient rows, sum |terms| of dpos"""
    t = d64(dtok)
    s = t.sum(0)
    patch = dtok.detach().cpu()[:, 1:].reshape(-1, dtok.shape[-1]).to(torch.bfloat16)
    return d64(dcls0) + s[0], d64(dpos0) + s, patch, d64(dpos0).abs() + t.abs().sum(0)


def embed_bwd_model(dtok, dcls0, dpos0, drop_last_frame=False):
    """the fused kernel's frame chunks: EMB_CHUNKS chunks of ceil(F / 4) frames, ragged or empty at the end.  drop_last_frame: a
    chunk of two or more frames loses its last one (a four-frame test, one frame per chunk, cannot see it)."""
    t = d64(dtok)
    per = (t.shape[0] + EMB_CHUNKS - 1) // EMB_CHUNKS
    dcls, dpos = d64(dcls0).clone(), d64(dpos0).clone()
    for c in range(EMB_CHUNKS):
        f0, f1 = c * per, min(t.shape[0], c * per + per)
        if drop_last_frame and f1 - f0 >= 2:
            f1 -= 1
        if f1 > f0:
            s = t[f0:f1].sum(0)
            dpos += s
            dcls += s[0]
    return dcls, dpos


# ------------------------------------------------------------------------------------------------ optimizer, casts
def sgd(p, g, lr, grad_scale):
    return d64(p) - (f32(lr) * f32(grad_scale)) * d64(g)


def cast_rows(src, rowscale):
    """bf16(fl32(src * rowscale[row])): the product of two fp32 numbers is exact in fp64, so one rounding to fp32"""
    return (d64(src) * d64(rowscale)[:, None]).float().to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ DINO loss
def lse_rows(kind, rows, n, seed=0):
    x = 0.3 * torch.randn(rows, n, generator=gen(4000 + seed))
    if kind == "equal":
        x = torch.full((rows, n), 0.25)
    elif kind == "peak":
        x[:, (7 * n) // 8 + 1 if n > 4 else 2] += 50.0
    elif kind == "shifted":
        x = x + 300.0
    else:
        assert kind == "plain"
    return x


def row_lse(x, scale, center=None):
    v = d64(x) if center is None else d64(x) - d64(center)
    return torch.logsumexp(v * f32(scale), -1)


def dino_loss(student, teacher, center, teacher_temp, ncrops, student_temp=0.1):
    """(loss, dloss / dstudent) of oracle.dino_oracle.dino_loss by fp64 autograd"""
    from oracle import dino_oracle as do
    s = d64(student).clone().requires_grad_(True)
    loss = do.dino_loss(s, d64(teacher), d64(center).view(1, -1), f32(teacher_temp), ncrops, f32(student_temp))
    loss.backward()
    return loss.detach(), s.grad


def colsum(x):
    return d64(x).sum(0), d64(x).abs().sum(0)


def center_ema(center, csum, momentum, inv_count):
    return d64(center) * f32(momentum) + d64(csum) * f32(inv_count) * (1.0 - f32(momentum))


# ------------------------------------------------------------------------------------------------ DINO head
def gelu_inputs(n, seed=0):
    """seeded values at scale 2 behind the edge values (n >= 4 keeps +-0 and +-12, n >= 8 all eight)"""
    u = 2.0 * torch.randn(n, generator=gen(5000 + seed))
    edge = torch.tensor([0.0, -0.0, 12.0, -12.0, 1e-30, -1e-30, 5.0, -5.0])[:min(n, 8)]
    u[:edge.numel()] = edge
    return u


def _phi_cdf(u):
    return 0.5 * torch.special.erfc(-u / math.sqrt(2.0))         # erfc: no cancellation in the left tail


def gelu(u):
    u = d64(u)
    return u * _phi_cdf(u)


def dgelu(u):
    u = d64(u)
    return _phi_cdf(u) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def l2_rows(rows, dim, eps, seed=0):
    """rows of kind L2_KINDS[(r + rows) % 4]: plain (scale 3), zero, ||z|| = eps / 2, ||z|| = 2 eps.  Returns (z, kinds)."""
    z = 3.0 * torch.randn(rows, dim, generator=gen(6000 + seed))
    kinds = [L2_KINDS[(r + rows) % 4] for r in range(rows)]
    e = f32(eps)
    for r, k in enumerate(kinds):
        if k == "zero":
            z[r] = 0.0
        elif k != "plain":
            z[r] = (z[r].double() / z[r].double().norm() * (0.5 * e if k == "half_eps" else 2.0 * e)).float()
    return z, kinds


def l2_clamp_rows(kinds):
    return [r for r, k in enumerate(kinds) if k in ("zero", "half_eps")]


def l2_condition(z, eps):
    """no row norm within 16 ulp32 of eps: which side of the clamp a row is on does not hang on a rounding"""
    e = torch.tensor(f32(eps), dtype=torch.float64)
    return bool(((d64(z).norm(dim=-1) - e).abs() > 16 * ulp32(e)).all())


def l2norm(z, eps, dout=None):
    """F.normalize(z, dim=-1, eps) and 1 / max(||z||, eps); with dout, dz by fp64 autograd"""
    zd = d64(z).clone().requires_grad_(dout is not None)
    out = F.normalize(zd, dim=-1, p=2, eps=f32(eps))
    inv = 1.0 / zd.detach().norm(dim=-1).clamp_min(f32(eps))
    if dout is None:
        return out.detach(), inv
    out.backward(d64(dout))
    return out.detach(), inv, zd.grad


def l2norm_bwd_model(dout, out, inv, z, eps, keep_projection=False):
    """dz = inv (dout - out (dout . out)), the projection dropped on a clamp row.  keep_projection: the clamp branch never taken"""
    g, o = d64(dout), d64(out)
    clamp = (d64(z).norm(dim=-1) < f32(eps)) & (not keep_projection)
    d = torch.where(clamp, torch.zeros(()).double(), (g * o).sum(-1))
    return (g - o * d[:, None]) * d64(inv)[:, None]


def weight_norm(v, g, dw=None):
    """w = g v / ||v||_row and 1 / ||v||; with dw: dv, dg by fp64 autograd and sum_i |dw_i v_i| / ||v|| (the terms of dg)"""
    vd, gd = d64(v).clone().requires_grad_(dw is not None), d64(g).clone().requires_grad_(dw is not None)
    nrm = vd.norm(dim=1, keepdim=True)
    w = gd.view(-1, 1) * vd / nrm
    if dw is None:
        return w.detach(), 1.0 / nrm.detach().view(-1)
    w.backward(d64(dw))
    return w.detach(), 1.0 / nrm.detach().view(-1), vd.grad, gd.grad.view(-1), (d64(dw) * vd.detach()).abs().sum(1) / nrm.detach().view(-1)


def split3(x, b_side):
    """[hi | hi | lo] (A side) or [hi | lo | hi] (B side), hi = bf16(x), lo = bf16(x - hi): csrc/common.hpp split8"""
    hi, lo = G.split8(x.detach().float().cpu())
    parts = [hi, lo, hi] if b_side else [hi, hi, lo]
    return torch.cat(parts, dim=1).to(torch.bfloat16)


def split3_values(rows, K, seed=0):
    """magnitudes from 1e-20 to 1e20, log-uniform, both signs"""
    g = gen(7000 + seed)
    mag = torch.pow(10.0, 40.0 * torch.rand(rows, K, generator=g, dtype=torch.float64) - 20.0)
    return (mag * (torch.randint(0, 2, (rows, K), generator=g) * 2 - 1)).float()


# ------------------------------------------------------------------------------------------------ positional map
def pos_interp_fwd(Wm, pos):
    return torch.cat([d64(pos)[:1], d64(Wm) @ d64(pos)[1:]])


def pos_interp_bwd(Wm, dout, dpos0):
    return d64(dpos0) + torch.cat([d64(dout)[:1], d64(Wm).t() @ d64(dout)[1:]])


# ------------------------------------------------------------------------------------------------ clip + AdamW + EMA
class OptRef:
    """oracle.dino_oracle's clip_coef / adamw_update / ema over named fp64 tensors, as test_adamw_clip_ema_vs_oracle drives them.
    class1: the tensors the freeze applies to; no_grad: tensors without a gradient (their teacher copy still moves)."""

    def __init__(self, params, class1=(), no_grad=()):
        self.st = {n: d64(p).clone() for n, p in params.items()}
        self.tt = {n: v.clone() for n, v in self.st.items()}
        self.m = {n: torch.zeros_like(v) for n, v in self.st.items()}
        self.v = {n: torch.zeros_like(v) for n, v in self.st.items()}
        self.steps = {n: 0 for n in self.st}
        self.class1, self.no_grad = tuple(class1), tuple(no_grad)

    def step(self, grads, clip, lr, wd, mom, frozen, decay_everything=False):
        """returns the pre-clip norms.  decay_everything: the mutation, weight decay also on biases and 1-D tensors"""
        from oracle import dino_oracle as do
        norms = {}
        for n in self.st:
            if n not in self.no_grad:
                g = d64(grads[n])
                norms[n], c = do.clip_coef(g, f32(clip))
                if not clip > 0:
                    c = 1.0
                if not (n in self.class1 and frozen):
                    self.steps[n] += 1
                    decay = decay_everything or do.is_regularized(n, self.st[n].shape)
                    self.st[n], self.m[n], self.v[n] = do.adamw_update(self.st[n], g * c, self.m[n], self.v[n], self.steps[n],
                                                                       f32(lr), f32(wd) if decay else 0.0)
            self.tt[n] = do.ema(self.tt[n], self.st[n], f32(mom))
        return norms


def adamw_toy_shapes():
    """name -> shape over ADAMW_SIZES: 2-D tensors are decayed, 1-D ones and `.bias` are not; `last.weight` is class 1 (8196
    elements: two chunks, the second of 4), `big.weight` has 66 chunks (the norm kernel strides over a tensor's chunks by 64)"""
    return {"a.weight": (2, 2), "a.bias": (1020,), "b.weight": (4, 257), "b.bias": (8188,), "c.weight": (64, 128),
            "last.weight": (2, 4098), "d.weight": (64, 384), "big.weight": (4, 65 * 2048 + 1), "fixed": (12, 1)}


ADAMW_CLASS1, ADAMW_NO_GRAD, ADAMW_ZERO_GRAD = ("last.weight",), ("fixed",), "c.weight"


def lse_naive_f32(x, scale, center=None):
    """the mutation: log sum exp without the max subtraction, in fp32"""
    v = x.detach().float().cpu() if center is None else x.detach().float().cpu() - center.detach().float().cpu()
    return torch.log(torch.exp(v * torch.tensor(scale, dtype=torch.float32)).sum(-1))
