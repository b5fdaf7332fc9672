"""fp64 references, derived error bounds, input layouts, fp32 restatements and launcher rules for the temporal encoder kernels
(csrc/tattn.hip, csrc/temporal.hip) and the row-LayerNorm backwards they feed (csrc/tgemm.hip, csrc/norm.hip).  Shared by
test_temporal_ref_host.py (which proves the bounds sound and sharp on the CPU) and test_temporal_edges_gpu.py; torch only, no
GPU dependency.  Where oracle/sais_oracle.py has the function it is the reference (in fp64, gradients by fp64 autograd):
temporal_prepare, nce_loss, cosine_logits, probs_from_logits, importance_loss.  The attention core of its temporal_layer and
the head part of its mil_forward are not callable on their own; attn_fp64 / mil_head_ref restate them line by line and the
host test ties attn_fp64 to temporal_layer's returned map.

Attention forward bounds (derived from tattn.hip, not tuned).  eps = 2^-24 is the unit roundoff of fp32.  Per query,
  sigma = 96^-1/2 max_key sum_d |q_d| |k_d|,   smax = max_key |s|   (unmasked keys),   E = eps (194 sigma + 4 smax + 128).
  * a score is a 96-term fmaf chain on the matrix core (dot_tile: 4 k-slots x 24 steps, plus the rounding of q * 96^-1/2 in
    load24): |s~ - s| <= 97 eps sigma to first order.  The exponent takes s - m, and m is such a score too: 2 x 97 = 194.
  * s - m is rounded (eps |s - m| <= 2 eps smax) and __expf multiplies it by log2(e) in fp32 (another eps |s - m|): 4 smax.
    An absolute error in the exponent is a relative error in exp.
  * v_exp_f32 (~2 eps), the <= 96-term sum of non-negative terms (<= 96 eps relative), the reciprocal and the product
    (~3 eps), and the second-order slack: 128.
  |P - ref| <= E ref + 1e-30 (results below 2^-126 flush to zero: the absolute term).
  P' = P keep / (1 - p) is one more product, exactly 0 where dropped.  attn_avg adds v / 4 (exact) of the four heads with
  atomics in any order: three more roundings.  |avg - ref| <= mean_h(E P') + 4 eps ref + 1e-30.
  ctx = P' v is a <= 96-term fmaf chain of its own: |ctx - ref| <= (E + 97 eps) A + 1e-30, A = P' |v|.
These are worst-case constants; plain fp32 torch sits at 0.005 - 0.05 of them.  The bar of the GPU tests is therefore
min(1, 8 x r_emu) of the bound: r_emu is the worst ratio of the fp32 restatement (emulate: torch float32, same formula) to the
bound per layout and quantity, recorded in R_EMU and recomputed by the host test.  The factor 8 covers what the restatement
does not model: the kernel's summation order (4 MFMA k-slots x 24 fmaf steps against torch's blocked sums) and the hardware
exp2 against libm.  It still sits two orders below any indexing or masking mistake (MUTATIONS, shown by the host test).
The backward bar is per part (dq, dk, dv): relative L2 against fp64 autograd <= 8 x the fp32 restatement's own relative L2 of
that case (BWD_EMU), floored at the rand layout's value at the same S.  None of this is calibrated from a kernel's output."""
import math

import torch
import torch.nn.functional as F

from oracle import sais_oracle as O

TH, THD, DM, EMB = 4, 96, 384, 256
SCALE = 96 ** -0.5
EPS = 2.0 ** -24
S_LIST = (1, 2, 15, 16, 17, 32, 33, 64, 65, 81, 96)
LAYOUTS = ("rand", "peaky", "planted", "same")
BWD_LAYOUTS = ("rand", "peaky", "planted")
DROP_CASES = tuple((S, p, site) for S in (17, 65) for p in (0.1, 0.5) for site in (0, 7))
MUTATIONS = ("mask_off_by_one", "no_tail_mask", "dropout_transposed", "dropout_head_stride", "keep_unscaled",
             "avg_of_kept_heads", "drop_last_slab")
PLANTED_MULT = 1.25


# ---------------------------------------------------------------------------------------------- the launchers' published rules
def tattn_tiles(S):
    """16-token tiles of sais_temporal_attn_fwd / _bwd (tattn.hip: nt = (S + 15) >> 4, MAXT = 6); None = rejected"""
    return (S + 15) // 16 if 1 <= S <= 96 else None


def nce_lds_small(B, C):
    """bytes of the norms, sim, dsim and row-loss arrays of sais_nce (temporal.hip: lds)"""
    return (B + C + 2 * B * C + B + 3) * 4


def nce_staged(B, C):
    """whether sais_nce stages its (B + C) x 256 operands in LDS: iff everything fits 60 KiB"""
    return nce_lds_small(B, C) + (B + C) * EMB * 4 <= 60 * 1024


def ln_bwd_grid(rows):
    """workgroups (of 8 rows a trip) of sais_temporal_ln_bwd and sais_layernorm_bwd"""
    return min((rows + 7) // 8, 1024)


# ---------------------------------------------------------------------------------------------- masks and layouts
def mask_patterns(S):
    """[(name, bool [S], True = masked)].  Key 0 (the CLS token) is never masked."""
    out = [("none", torch.zeros(S, dtype=torch.bool))]

    def tail(last):
        m = torch.zeros(S, dtype=torch.bool)
        m[last + 1:] = True
        return m
    if S >= 2:
        out.append(("only0", tail(0)))
    if S >= 17:
        out.append(("last15", tail(15)))
    if S >= 18:
        out.append(("last16", tail(16)))
    if S >= 6:
        m = torch.zeros(S, dtype=torch.bool)
        m[3] = m[S - 2] = True
        out.append(("holes", m))
    return out


def masks(S):
    """bool [B, S], one sequence per pattern"""
    return torch.stack([m for _, m in mask_patterns(S)])


def _coprime_mult(n):
    a = 3
    while n % a == 0 or any(a % d == 0 for d in range(3, a, 2)):
        a += 2
    return a


def planted_key(pad_row):
    """key [S] of every query of one sequence: kept[(a q + n - 1) mod n] over its n unmasked keys (a the smallest odd prime
    that does not divide n), so query 0's key is the LAST unmasked one and the queries walk over every unmasked key"""
    kept = torch.nonzero(~pad_row).flatten()
    n, S = kept.numel(), pad_row.numel()
    return kept[(_coprime_mult(n) * torch.arange(S) + n - 1) % n]


def layouts(name, pad, seed):
    """fp32 qkv [B * S, 1152] on the CPU for the masks pad [B, S].
      rand     N(0, 1)
      peaky    k x 12: scaled scores ~ N(0, 12^2), near +-50 at the ends: the max subtraction carries the result
      planted  a +-1 code per unmasked key; k[key] = 1.25 code, q = the code of planted_key(q): the planted score is
               1.25 x 96^1/2 = 12.2 against ~ 1.25 N(0, 1) for every other key
      same     q = 0: every score is exactly 0, every unmasked probability exactly 1 / n"""
    B, S = pad.shape
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B, S, 3, TH, THD, generator=g)
    if name == "peaky":
        t[:, :, 1] *= 12.0
    elif name == "planted":
        code = torch.randint(0, 2, (B, S, TH, THD), generator=g).float() * 2 - 1
        for b in range(B):
            t[b, :, 1] = PLANTED_MULT * code[b]
            t[b, :, 0] = code[b, planted_key(pad[b])]
    elif name == "same":
        t[:, :, 0] = 0.0
    elif name != "rand":
        raise ValueError(name)
    return t.reshape(B * S, 3 * DM)


def case_seed(name, S):
    return 7000 + 100 * LAYOUTS.index(name) + S


def heads(qkv, B, S):
    """[B * S, 1152] -> q, k, v views [B, 4, S, 96]"""
    t = qkv.reshape(B, S, 3, TH, THD).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def host_keep(B, S, p, seed):
    """a Bernoulli(1 - p) keep mask [B, 4, S, S] for the CPU tests (the GPU tests take the kernel's own Philox mask)"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, TH, S, S, generator=g) >= p


# ---------------------------------------------------------------------------------------------- attention: reference and bounds
def _attn(qkv, pad, keep, p, dt):
    B, S = pad.shape
    q, k, v = heads(qkv.to(dt), B, S)
    s = (q * torch.tensor(SCALE, dtype=dt)) @ k.transpose(-2, -1)
    s = s.masked_fill(pad.view(B, 1, 1, S), float("-inf"))
    P = s.softmax(-1)
    Pd = P if keep is None else P * keep.to(dt) / (1.0 - p)
    return q, k, v, s, P, Pd


def attn_fp64(qkv, pad, keep=None, p=0.0):
    """The attention core of oracle.temporal_layer (lines scores .. ctx) in fp64 with an explicit keep mask [B, 4, S, S]:
    P' = P keep / (1 - p), avg = mean_h P', ctx = P' v.  -> dict(P, Pd [B,4,S,S], avg [B,S,S], ctx, A [B*S,384], E [B,4,S])"""
    B, S = pad.shape
    q, k, v, s, P, Pd = _attn(qkv, pad, keep, p, torch.float64)
    pm = pad.view(B, 1, 1, S)
    sigma = SCALE * (q.abs() @ k.abs().transpose(-2, -1)).masked_fill(pm, 0.0).amax(-1)
    smax = s.masked_fill(pm, 0.0).abs().amax(-1)
    flat = lambda t: t.transpose(1, 2).reshape(B * S, DM)
    return dict(P=P, Pd=Pd, avg=Pd.mean(1), ctx=flat(Pd @ v), A=flat(Pd @ v.abs()), E=EPS * (194 * sigma + 4 * smax + 128))


def p_bound(ref):
    return ref["E"].unsqueeze(-1) * ref["P"] + 1e-30


def avg_bound(ref):
    return (ref["E"].unsqueeze(-1) * ref["Pd"]).mean(1) + 4 * EPS * ref["avg"] + 1e-30


def ctx_bound(ref):
    B, _, S = ref["E"].shape
    e = (ref["E"] + 97 * EPS).transpose(1, 2).reshape(B * S, TH, 1)
    return (e * ref["A"].view(B * S, TH, THD)).reshape(B * S, DM) + 1e-30


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; NaN / inf in got count as inf"""
    r = (got.double() - ref).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max())


def attn_bwd_fp64(qkv, pad, dctx, keep=None, p=0.0, dt=torch.float64):
    """d qkv [B * S, 1152] by autograd of the attention (fp64; dt = float32: the fp32 restatement of the backward)"""
    B, S = pad.shape
    x = qkv.to(dt).detach().clone().requires_grad_(True)
    _, _, v, _, _, Pd = _attn(x, pad, keep, p, dt)
    (Pd @ v).transpose(1, 2).reshape(B * S, DM).backward(dctx.to(dt))
    return x.grad


def rel_l2_parts(got, ref):
    """per part (dq, dk, dv) relative L2 of a [M, 1152] gradient.  A part whose reference is exactly zero (S = 1: dq = dk = 0)
    gives 0 when got is exactly zero too, inf otherwise."""
    out = []
    for i in range(3):
        g, r = got[:, DM * i:DM * (i + 1)].double(), ref[:, DM * i:DM * (i + 1)].double()
        n = float(r.norm())
        d = float((g - r).norm())
        out.append(d / n if n > 0 else (0.0 if d == 0 else float("inf")))
    return out


# ---------------------------------------------------------------------------------------------- attention: fp32 restatement
def emulate(qkv, pad, keep=None, p=0.0, mutate=None):
    """The forward's arithmetic in torch float32: scores with q * 96^-1/2, -inf on masked keys, exp(s - max), one reciprocal of
    the sum, P' = P keep * (1 / (1 - p)), avg = sum_h P' / 4, ctx = P' v.  MFMA summation order and the hardware exp2 are not
    modelled.  -> dict(P, avg, ctx) float32.  mutate: one deliberate error -
      mask_off_by_one      the first masked key of every sequence counts as unmasked (a tail mask one key late)
      no_tail_mask         the zero-filled keys S .. 16 nt - 1 of the last tile count (score 0, value 0)
      dropout_transposed   keep[i, j] <-> keep[j, i]
      dropout_head_stride  the mask element index built from h * B + b where b * 4 + h belongs
      keep_unscaled        no 1 / (1 - p)
      avg_of_kept_heads    the map divided by the number of heads that kept the entry where 4 belongs"""
    assert mutate is None or mutate in MUTATIONS
    B, S = pad.shape
    q, k, v = (t.float() for t in heads(qkv, B, S))
    pad = pad.clone()
    if mutate == "mask_off_by_one":
        for b in range(B):
            idx = torch.nonzero(pad[b]).flatten()
            if idx.numel():
                pad[b, idx[0]] = False
    if mutate == "no_tail_mask":
        extra = 16 * tattn_tiles(S) - S
        k = torch.cat((k, torch.zeros(B, TH, extra, THD)), 2)
        v = torch.cat((v, torch.zeros(B, TH, extra, THD)), 2)
        pad = torch.cat((pad, torch.zeros(B, extra, dtype=torch.bool)), 1)
    s = (q * torch.tensor(SCALE, dtype=torch.float32)) @ k.transpose(-2, -1)
    s = s.masked_fill(pad.view(B, 1, 1, -1), float("-inf"))
    e = torch.exp(s - s.amax(-1, keepdim=True))
    P = (e * (1.0 / e.sum(-1, keepdim=True)))[..., :S]                 # the zero-filled keys have zero value rows
    v = v[:, :, :S]
    Pd = P
    if keep is not None:
        kp = keep
        if mutate == "dropout_transposed":
            kp = keep.transpose(-2, -1)
        elif mutate == "dropout_head_stride":
            kp = keep.reshape(TH, B, S, S).transpose(0, 1)
        inv = torch.tensor(1.0 if mutate == "keep_unscaled" else 1.0 / (1.0 - p), dtype=torch.float32)
        Pd = torch.where(kp, P * inv, torch.zeros(()))
    if mutate == "avg_of_kept_heads" and keep is not None:
        avg = Pd.sum(1) / keep.sum(1).clamp(min=1).float()
    else:
        avg = (Pd * 0.25).sum(1)
    ctx = (Pd @ v).transpose(1, 2).reshape(B * S, DM)
    return dict(P=P, avg=avg, ctx=ctx)


def emulate_bwd(qkv, pad, slabs, keep=None, p=0.0, mutate=None):
    """fp32 autograd of the same formula on dctx = the sum of the slabs [n, B * S, 384]; mutate = drop_last_slab: the last
    slab is not added"""
    n = slabs.shape[0] - (1 if mutate == "drop_last_slab" else 0)
    dctx = slabs[:n].float().sum(0) if n else torch.zeros_like(slabs[0])
    return attn_bwd_fp64(qkv, pad, dctx, keep, p, dt=torch.float32)


def attn_ratios(got, ref):
    """{P (when got has it), avg, ctx}: worst |got - ref| / bound"""
    r = dict(avg=worst_ratio(got["avg"], ref["avg"], avg_bound(ref)), ctx=worst_ratio(got["ctx"], ref["ctx"], ctx_bound(ref)))
    if "P" in got:
        r["P"] = worst_ratio(got["P"], ref["P"], p_bound(ref))
    return r


# worst ratio of emulate() to the bounds per layout, over every S of S_LIST and its masks at p = 0 and (rand) DROP_CASES with
# host_keep masks; measured on the CPU and recomputed by test_temporal_ref_host.py
R_EMU = {
    "rand": dict(P=2.061e-02, avg=1.347e-02, ctx=8.616e-03),
    "peaky": dict(P=2.844e-02, avg=2.348e-02, ctx=1.650e-02),
    "planted": dict(P=8.136e-02, avg=8.034e-02, ctx=4.919e-02),
    "same": dict(P=7.568e-03, avg=7.339e-03, ctx=1.594e-02),
}


def fwd_bar(name, what):
    """fraction of the derived bound the kernel must stay inside: min(1, 8 r_emu)"""
    return min(1.0, 8.0 * R_EMU[name][what])


# bwd_emu_case per part (dq, dk, dv), keyed (layout, S, p); p > 0 with host_keep(B, S, p, BWD_SEED + S)
BWD_SEED = 90
BWD_EMU = {
    ("rand", 1, 0.0): [0.000e+00, 0.000e+00, 4.324e-08],
    ("rand", 2, 0.0): [2.437e-07, 2.401e-07, 6.897e-08],
    ("rand", 15, 0.0): [2.572e-07, 2.491e-07, 1.308e-07],
    ("rand", 16, 0.0): [2.846e-07, 2.825e-07, 1.291e-07],
    ("rand", 17, 0.0): [2.584e-07, 2.559e-07, 1.446e-07],
    ("rand", 32, 0.0): [2.677e-07, 2.759e-07, 1.785e-07],
    ("rand", 33, 0.0): [2.921e-07, 2.975e-07, 1.694e-07],
    ("rand", 64, 0.0): [2.913e-07, 3.107e-07, 1.877e-07],
    ("rand", 65, 0.0): [2.992e-07, 3.212e-07, 1.978e-07],
    ("rand", 81, 0.0): [2.929e-07, 3.212e-07, 2.119e-07],
    ("rand", 96, 0.0): [3.014e-07, 3.318e-07, 2.288e-07],
    ("peaky", 1, 0.0): [0.000e+00, 0.000e+00, 4.324e-08],
    ("peaky", 2, 0.0): [7.572e-06, 6.642e-06, 5.365e-08],
    ("peaky", 15, 0.0): [2.132e-06, 2.200e-06, 4.831e-07],
    ("peaky", 16, 0.0): [2.218e-06, 2.161e-06, 4.398e-07],
    ("peaky", 17, 0.0): [2.019e-06, 1.904e-06, 4.552e-07],
    ("peaky", 32, 0.0): [1.763e-06, 1.749e-06, 6.961e-07],
    ("peaky", 33, 0.0): [1.998e-06, 2.045e-06, 7.407e-07],
    ("peaky", 64, 0.0): [2.206e-06, 2.260e-06, 8.059e-07],
    ("peaky", 65, 0.0): [1.923e-06, 1.911e-06, 7.309e-07],
    ("peaky", 81, 0.0): [2.274e-06, 2.318e-06, 7.874e-07],
    ("peaky", 96, 0.0): [2.336e-06, 2.337e-06, 7.675e-07],
    ("planted", 1, 0.0): [0.000e+00, 0.000e+00, 4.324e-08],
    ("planted", 2, 0.0): [4.116e-03, 3.845e-03, 5.467e-08],
    ("planted", 15, 0.0): [8.504e-04, 7.383e-04, 1.095e-07],
    ("planted", 16, 0.0): [4.436e-04, 4.013e-04, 1.020e-07],
    ("planted", 17, 0.0): [3.638e-04, 3.355e-04, 1.048e-07],
    ("planted", 32, 0.0): [2.878e-04, 2.411e-04, 1.326e-07],
    ("planted", 33, 0.0): [3.098e-04, 2.726e-04, 1.297e-07],
    ("planted", 64, 0.0): [1.984e-04, 1.779e-04, 1.662e-07],
    ("planted", 65, 0.0): [2.156e-04, 1.856e-04, 1.678e-07],
    ("planted", 81, 0.0): [1.782e-04, 1.554e-04, 1.839e-07],
    ("planted", 96, 0.0): [1.497e-04, 1.372e-04, 1.978e-07],
    ("rand", 17, 0.1): [2.602e-07, 2.585e-07, 1.512e-07],
    ("rand", 17, 0.5): [2.515e-07, 2.549e-07, 1.440e-07],
    ("rand", 65, 0.1): [3.021e-07, 3.243e-07, 1.963e-07],
    ("rand", 65, 0.5): [2.951e-07, 3.166e-07, 1.731e-07],
}


def bwd_case(name, S):
    """(qkv fp32 [B * S, 1152], pad bool [B, S], dctx fp32 [B * S, 384]) on the CPU"""
    pad = masks(S)
    g = torch.Generator().manual_seed(BWD_SEED + 1000 + S)
    return layouts(name, pad, case_seed(name, S)), pad, torch.randn(pad.shape[0] * S, DM, generator=g)


def bwd_bars(name, S, p=0.0):
    return [max(8.0 * e, r) for e, r in zip(BWD_EMU[(name, S, p)], BWD_EMU[("rand", S, 0.0)])]


def bwd_emu_case(name, S, p=0.0):
    """what BWD_EMU records: the fp32 restatement on dctx handed over as three slabs (the form with the most fp32 roundings:
    one bar serves the plain and the slab forms) against fp64 autograd on the fp64 sum of the slabs"""
    qkv, pad, dctx = bwd_case(name, S)
    keep = host_keep(pad.shape[0], S, p, BWD_SEED + S) if p > 0 else None
    buf, total = split_slabs(dctx, 3, 64, BWD_SEED + S)
    return rel_l2_parts(emulate_bwd(qkv, pad, slab_view(buf, dctx.shape[0]), keep, p), attn_bwd_fp64(qkv, pad, total, keep, p))


def slab_view(buf, M):
    """[n, M, 384] view of a gapped slab buffer [n, M * 384 + gap]: slab stride = M * 384 + gap floats"""
    return torch.as_strided(buf, (buf.shape[0], M, DM), (buf.stride(0), DM, 1))          # as_strided: keeps the stride for n = 1 too


def split_slabs(total, n, gap, seed):
    """n fp32 slabs, M * 384 + gap floats apart, whose sum is `total` [M, 384] up to fp32 rounding; NaN in the gaps.
    -> (the gapped buffer [n, M * 384 + gap], the fp64 sum of the slabs it holds)"""
    M = total.shape[0]
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((n, M * DM + gap), float("nan"))
    view = slab_view(buf, M)
    rest = total.clone()
    for z in range(n - 1):
        view[z] = torch.randn(M, DM, generator=g)
        rest = rest - view[z]
    view[n - 1] = rest
    return buf, view.double().sum(0)


# ---------------------------------------------------------------------------------------------- prepare
def prepare_fp64(x, pos, cls):
    """oracle.temporal_prepare on x [B, T, 384] -> [B, T + 1, 384] fp64"""
    B, T, _ = x.shape
    sd = {f"frame_pos_embeddings.{i}": pos[i:i + 1].double() for i in range(T)}
    sd["frame_cls"] = cls.double()
    return O.temporal_prepare(sd, x.double().unsqueeze(1))[:, 0]


# ---------------------------------------------------------------------------------------------- head
def head_fp64(zr, zf, W, bias, use_b=None, WB=None, biasB=None, dt=torch.float64):
    """fullModel's head (oracle.temporal_forward from `rep = rgb.mean(1)`): z* [B, ns, S, 384] or None -> leaves and
    (rep [B, 384], emb [B, 256]) under autograd in dt"""
    leaf = lambda t: None if t is None else t.detach().to(dt).clone().requires_grad_(True)
    L = dict(zr=leaf(zr), zf=leaf(zf), W=leaf(W), bias=leaf(bias), WB=leaf(WB), biasB=leaf(biasB))
    rep = 0
    for z in (L["zr"], L["zf"]):
        if z is not None:
            rep = rep + F.relu(z)[:, :, 0].mean(1)
    rrep = F.relu(rep)
    emb = F.linear(rrep, L["W"], L["bias"])
    if use_b is not None:
        emb = torch.where(use_b.bool().view(-1, 1), F.linear(rrep, L["WB"], L["biasB"]), emb)
    return L, rep, emb


# ---------------------------------------------------------------------------------------------- MIL
MIL_CASES = ((1, 1, 1, False), (2, 5, 2, False), (2, 127, 3, False), (3, 128, 3, False), (2, 5, 2, True))


def mil_case(B, ns, C, saturate, seed=300):
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * ns + C)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    big = 50.0 if saturate else 1.0
    return dict(enc=r(B, ns, DM), WA=r(EMB, DM, scale=0.05 * big), bA=r(EMB, scale=0.1), WB=r(EMB, DM, scale=0.05 * big),
                bB=r(EMB, scale=0.1), w_att=r(C, EMB, scale=0.2), b_att=r(C, scale=0.1), w_fin=r(C, DM, scale=0.05),
                b_fin=r(C, scale=0.1))


def mil_head_ref(c, dt=torch.float64):
    """the head part of oracle.mil_forward (from `reps = F.relu(z)`), restated on the encoder output c["enc"] [B, ns, 384].
    -> reps [B, ns, 384], logits [B, C], attention [C, B, ns].  dt = float32: the fp32 restatement."""
    t = {k: v.to(dt) for k, v in c.items()}
    reps = F.relu(t["enc"])
    a = torch.tanh(F.linear(reps, t["WA"], t["bA"]))
    g = torch.sigmoid(F.linear(reps, t["WB"], t["bB"]))
    logits, att = [], []
    for cl in range(t["w_att"].shape[0]):
        w = torch.softmax(F.linear(a * g, t["w_att"][cl:cl + 1], t["b_att"][cl:cl + 1]), 1)        # [B, ns, 1]
        video = (w * reps).sum(1)
        logits.append(F.linear(video, t["w_fin"][cl:cl + 1], t["b_fin"][cl:cl + 1]))
        att.append(w.squeeze(-1))
    return reps, torch.cat(logits, 1), torch.stack(att)


# worst |fp32 restatement - fp64| over MIL_CASES (logits, attention); one value per quantity, not per case: the error of a
# single scalar (logits of the (1, 1, 1) case) is noise, and a bar made from it would be too
MIL_EMU = dict(logits=1.763e-07, attention=3.481e-07)


def mil_bars():
    return {k: 8.0 * v for k, v in MIL_EMU.items()}


# ---------------------------------------------------------------------------------------------- importance head
def importance_fwd_bound(z, w, b):
    """out = relu(z) . w + b: a lane adds 6 products, the wave sum 6 levels, the bias one more: <= 14 roundings on any path
    -> 16 eps (sum |w| relu(z) + |b|)"""
    return 16 * EPS * (F.relu(z.double()) @ w.double().abs() + b.double().abs())


def importance_bwd_bounds(dl, z, w, dz0, dw0, db0):
    """(dz, dw, db) bounds of sais_importance_bwd.  dz += dl w where z > 0: one product, one sum -> 2 eps (|dz0| + |dl w|).
    dw, db: a workgroup adds the terms of its <= ceil(M / 64) rows in turn, then the <= 64 workgroups add theirs to the
    accumulator with atomics: <= ceil(M / 64) + 66 roundings on any path, taken on the magnitudes."""
    dl, z, w = dl.double(), z.double(), w.double()
    n = (math.ceil(dl.numel() / 64) + 66) * EPS
    dzb = 2 * EPS * (dz0.double().abs() + (dl[:, None] * w[None, :]).abs())
    dwb = n * (dl.abs() @ F.relu(z) + dw0.double().abs())
    dbb = n * (dl.abs().sum() + db0.double().abs())
    return dzb, dwb, dbb


def importance_loss_fp64(logits, target, ipad, labels, scale=1.0):
    """oracle.importance_loss on logits [B, S] (slot 0 = CLS), target [B, T], ipad bool [B, S], labels [B]
    -> (loss, d (scale loss) / d logits [B, S]) in fp64"""
    x = logits.double().detach().clone().requires_grad_(True)
    loss = O.importance_loss(x.view(x.shape[0], 1, -1, 1), target.double().unsqueeze(1), ipad.bool().unsqueeze(1), labels)
    (loss * scale).backward()
    return loss.detach(), x.grad


def importance_loss_bounds(logits, target, ipad, labels, scale=1.0):
    """(loss bound, dlogits bound [B, S]).  The loss is frac x the mean of B T terms max(x, 0) - x y + log1p(e^-|x|), each
    sub-term rounded (<= 4 eps of their magnitudes with __expf / log1pf), summed by 256 threads (<= ceil(B T / 256) terms
    each) and an 8-level tree, divided and multiplied: <= (ceil(B T / 256) + 16) eps on any path, taken on the magnitudes.
    dlogits = k (sigmoid(x) - y), sigmoid = 1 / (1 + __expf(-x)): __expf rounds x log2(e) before the hardware exp2, an
    absolute error of eps |x| log2(e) / 2 in the exponent = <= eps |x| relative in the result, which the reciprocal hands to
    the sigmoid; exp2, the add and the reciprocal add <= 6 eps: (|x| + 6) eps sigmoid.  The difference, the product and the
    three roundings of k: 4 eps (sigmoid + |y|).  Together eps |k| ((|x| + 10) sigmoid + 4 |y|)."""
    B, S = logits.shape
    T = S - 1
    x, y = logits.double()[:, 1:], target.double()
    low = labels == 0
    nlow = int(low.sum())
    frac = float((~ipad.bool())[low, :T].sum()) / (nlow * T) if nlow else float("nan")
    mag = (x.clamp(min=0) + (x * y).abs() + torch.log1p(torch.exp(-x.abs()))).mean()
    lb = (math.ceil(B * T / 256) + 16) * EPS * mag * abs(frac)
    k = abs(frac * scale / (B * T))
    db = torch.zeros(B, S, dtype=torch.float64)
    db[:, 1:] = EPS * k * ((x.abs() + 10) * torch.sigmoid(x) + 4 * y.abs())
    return lb, db


# ---------------------------------------------------------------------------------------------- NCE
NCE_CASES = ((1, 1), (1, 2), (8, 2), (14, 3), (56, 2), (57, 2), (300, 3))
NCE_SMALL = dict(sim=1e-6, probs=1e-6, loss=1e-6, demb=1e-7, dprotos=1e-7)          # the bars of test_nce_loss_and_grads


def nce_case(B, C, seed=80):
    emb = torch.randn(B, EMB, generator=torch.Generator().manual_seed(seed + B))
    protos = torch.rand(C, EMB, generator=torch.Generator().manual_seed(seed + 1 + B))
    lab = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed + 2 + B))
    return emb, protos, lab


def nce_ref(emb, protos, lab, loss_scale=1.0, dt=torch.float64):
    """oracle.nce_loss / cosine_logits / probs_from_logits in dt -> dict(sim, probs, loss, demb, dprotos)"""
    e = emb.detach().to(dt).clone().requires_grad_(True)
    pd = {str(c): protos[c:c + 1].detach().to(dt).clone().requires_grad_(True) for c in range(protos.shape[0])}
    loss = O.nce_loss(e, lab, pd)
    (loss * loss_scale).backward()
    sim = O.cosine_logits(e, pd).detach()
    return dict(sim=sim, probs=O.probs_from_logits(sim), loss=loss.detach(), demb=e.grad,
                dprotos=torch.cat([pd[str(c)].grad for c in range(protos.shape[0])]))


# worst |fp32 restatement - fp64| per quantity of the cases above B = 8 (loss_scale = 1)
NCE_EMU = {
    (14, 3): dict(sim=5.167e-08, probs=4.131e-08, loss=1.189e-07, demb=7.841e-11, dprotos=4.803e-10),
    (56, 2): dict(sim=6.706e-08, probs=7.348e-08, loss=9.018e-08, demb=2.558e-11, dprotos=4.370e-10),
    (57, 2): dict(sim=9.417e-08, probs=4.762e-08, loss=8.313e-11, demb=2.280e-11, dprotos=2.471e-10),
    (300, 3): dict(sim=1.032e-07, probs=5.673e-08, loss=8.075e-08, demb=7.846e-12, dprotos=3.336e-10),
}


def nce_bars(B, C):
    """the bars of test_nce_loss_and_grads up to B = 8; above, 8 x the fp32 restatement's error, floored at those"""
    if B <= 8:
        return dict(NCE_SMALL)
    return {k: max(NCE_SMALL[k], 8.0 * NCE_EMU[(B, C)][k]) for k in NCE_SMALL}


# ---------------------------------------------------------------------------------------------- row LayerNorm backward
def ln_bwd_fp64(x, gamma, dy, eps):
    """(mean, rstd, dx, dgamma, dbeta) of LayerNorm(x) under the output gradient dy, fp64"""
    xr = x.double().detach().clone().requires_grad_(True)
    gr = gamma.double().detach().clone().requires_grad_(True)
    br = torch.zeros_like(gr).requires_grad_(True)
    F.layer_norm(xr, (x.shape[-1],), gr, br, eps).backward(dy.double())
    mean = x.double().mean(1)
    rstd = 1 / torch.sqrt(x.double().var(1, unbiased=False) + eps)
    return mean, rstd, xr.grad, gr.grad, br.grad
