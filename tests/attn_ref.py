"""fp64 reference, derived error bounds, input layouts and f32 / bf16 emulations for the attention kernels (csrc/attn_any.hip,
csrc/attn_vit.hip, csrc/attn_cls.hip).  Shared by test_attn_ref_host.py (which proves the bounds sound and sharp on the CPU)
and test_attn_edges_gpu.py; torch only, no GPU dependency.  Attention.forward — dino-main/vision_transformer.py:80-92: 6 heads
of 64, scale 64^-0.5, qkv rows are [q | k | v] x [head] x [64].

Bounds (derived, not tuned).  U = 2^-8 is the unit roundoff of bf16, A = softmax(s) @ |v| per output element.
  * out:  |out - ref| <= U (|ref| + A) + 2^-14 A.
      Both forwards form p~ = exp(s - m) <= 1 in f32, round it ONCE to bf16 for the P V product (pack_p: attn_any.hip:119,
      attn_vit.hip:159), accumulate in f32 and divide by the f32 sum of the UNROUNDED p~ (attn_any.hip:134, attn_vit.hip:169).
      Rounding p~ moves sum_j p~_j v_j by at most U sum_j p~_j |v_j|; after the division that is U A.  The quotient is rounded
      once to bf16: U |ref| to first order.  2^-14 A covers the f32 parts: v_exp_f32 (~2^-22 relative), the rounding of the
      exponent argument (|score| log2e 2^-24 <= 2^-15 for |score| <= ~600, absolute in the exponent = relative in p, but common
      to numerator and denominator up to its variation over the keys), f32 accumulation over <= 4097 keys, and the online
      rescale of attn_any.hip (one f32 multiply per tile).  The resident kernel normalises AFTER the product like the
      streaming one, so one bound serves both.  attn_cls.hip keeps P in f32 (no rounding before the product): its error is
      below U |ref| + 2^-14 A, inside the same bound.
  * lse:  |lse - ref| <= 1e-4 + 2^-20 smax,  smax = max_j |s_qj| (scaled).
      A lane adds <= ~1100 f32 terms (4097 keys / 4 lane groups + the cross-lane sums) at 2^-24 relative each: < 7e-5 relative
      on the sum = absolute on its logarithm; __logf adds ~1e-6.  m is an f32 score (MFMA accumulation of exact bf16 x bf16
      products, a few 2^-24 |s|) and m * scale is exact; the second term covers that.
  * probs (resident forward only): the kernel writes p~ / sum in f32 BEFORE any bf16 rounding (attn_vit.hip:180), so the
    issue's 2^-8 ref + 1e-6 would be 100 x too loose.  What the code implies: the exponent argument fma(s, c, -m c) carries
    the f32 error of s (64-term accumulation: <= 64 x 2^-24 = 2^-18 of sum_d |q_d k_d| scale, worst case), of c = scale log2e
    and of m c (2^-24 |s| log2e each): absolute in the exponent = relative in p; v_exp_f32, the 197-term sum, the reciprocal
    and the product add a few 2^-22.  |p - ref| <= (2^-16 + 2^-18 smax) ref + 1e-30 (results below 2^-126 flush to zero).
"""

import torch

NH, HD, DM = 6, 64, 384
SCALE = 0.125
LOG2E = 1.4426950408889634
U = 2.0 ** -8
LAYOUTS = ("rand", "planted", "up", "down", "offp", "offn", "same")
MUTATIONS = ("no_mask", "no_rescale", "drop_last_key", "stale_max")
MULT = {"planted": 4.0, "up": 4.0, "down": 4.0, "offp": 48.0, "offn": 48.0}      # the knob of each layout (see layouts)


# ---------------------------------------------------------------------------------------------- the launchers' published rules
def stream_waves(frames, ntok):
    """Waves per workgroup sais_vit_attn_fwd_any launches (attn_any.hip: 64-query workgroups iff there are >= 512 of them)."""
    return 4 if frames * NH * ((ntok + 63) // 64) >= 512 else 2


def bwd_cap(ntok):
    """Persistent workgroups of sais_vit_attn_bwd (attn_vit.hip launch_bwd: 256 * per_cu, per_cu from bwd_lds<Geo<ntok>>())."""
    nkt = (ntok + 15) // 16
    rows = 32 * ((nkt + 1) // 2)
    lds = 3 * rows * 160 + 2 * rows * 4 + 2 * rows * 96
    per_cu = 1 if nkt > 4 else min(4, 160 * 1024 // lds)
    return 256 * per_cu


# ---------------------------------------------------------------------------------------------- reference
def heads(qkv, frames, ntok):
    """[frames * ntok, >= 1152] -> q, k, v views [frames, 6, ntok, 64]"""
    t = qkv[:, :3 * DM].reshape(frames, ntok, 3, NH, HD).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def attn_fp64(qkv, frames, ntok, probs=False):
    """dict(out, A [frames * ntok, 384], lse, smax [frames, 6, ntok], probs [frames, 6, ntok, ntok] if asked) in fp64 from the
    (bf16-rounded) qkv as given, on its device.  One (frame, head) at a time: the score matrix at 4097 tokens is 134 MB."""
    q, k, v = heads(qkv, frames, ntok)
    dev = qkv.device
    out = torch.empty(frames, ntok, NH, HD, dtype=torch.float64, device=dev)
    A = torch.empty_like(out)
    lse = torch.empty(frames, NH, ntok, dtype=torch.float64, device=dev)
    smax = torch.empty_like(lse)
    pr = torch.empty(frames, NH, ntok, ntok, dtype=torch.float64, device=dev) if probs else None
    for f in range(frames):
        for h in range(NH):
            s = (q[f, h].double() @ k[f, h].double().t()) * SCALE
            smax[f, h] = s.abs().amax(-1)
            m = s.amax(-1, keepdim=True)
            s.sub_(m).exp_()
            z = s.sum(-1, keepdim=True)
            lse[f, h] = (m + z.log()).squeeze(-1)
            s.div_(z)
            vd = v[f, h].double()
            out[f, :, h] = s @ vd
            A[f, :, h] = s @ vd.abs()
            if probs:
                pr[f, h] = s
    r = dict(out=out.reshape(frames * ntok, DM), A=A.reshape(frames * ntok, DM), lse=lse, smax=smax)
    if probs:
        r["probs"] = pr
    return r


def out_bound(ref, A):
    return U * (ref.abs() + A) + 2.0 ** -14 * A


def lse_bound(smax):
    return 1e-4 + 2.0 ** -20 * smax


def probs_bound(ref, smax):
    """smax [..., ntok] per query, ref [..., ntok, ntok]"""
    return (2.0 ** -16 + 2.0 ** -18 * smax).unsqueeze(-1) * ref + 1e-30


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; NaN / inf in got count as inf"""
    r = (got.double() - ref).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max())


def attn_bwd_fp64(qkv, dout, frames, ntok, cls_only=False):
    """d qkv [frames * ntok, 1152] by fp64 autograd of the attention on the qkv as given.  dout: [frames * ntok, 384], or with
    cls_only [frames, 384] = the gradient of the CLS rows of the output (zero elsewhere)."""
    x = qkv[:, :3 * DM].double().detach().clone().requires_grad_(True)
    q, k, v = heads(x, frames, ntok)
    p = torch.softmax((q @ k.transpose(-2, -1)) * SCALE, -1)
    o = (p @ v).transpose(1, 2).reshape(frames, ntok, DM)
    if cls_only:
        o[:, 0].backward(dout.double())
    else:
        o.reshape(frames * ntok, DM).backward(dout.double())
    return x.grad


def rel_l2_parts(got, ref):
    """per-part (dq, dk, dv) relative L2 of a [M, 1152] gradient"""
    return [float((got[:, DM * i:DM * (i + 1)].double() - ref[:, DM * i:DM * (i + 1)].double()).norm() /
                  ref[:, DM * i:DM * (i + 1)].double().norm()) for i in range(3)]


# ---------------------------------------------------------------------------------------------- input layouts
def _coprime_mult(ntok):
    a = 3
    while ntok % a == 0 or any(a % d == 0 for d in range(3, a, 2)):
        a += 2
    return a


def planted_perm(ntok):
    """pi(q) = (a q + ntok - 1) mod ntok, a the smallest odd prime that does not divide ntok: a bijection (for ntok = 2 the
    multiplier is odd, which is all a bijection needs) that sends query 0 to the LAST key"""
    return (_coprime_mult(ntok) * torch.arange(ntok) + ntok - 1) % ntok


def layouts(name, frames, ntok, seed, mult=None):
    """bf16 qkv [frames * ntok, 1152] on the CPU.  Every (frame, head) gets its own draws (one generator, consumed in order).
    mult: the layout's knob (MULT[name] by default) — planted: the key multiplier; up / down: the value of q[:, 0]; offp /
    offn: the magnitude of q[:, 1] and k[:, 1].
      rand     N(0, 1.5^2)
      planted  code = +-1 [ntok, 64]; q = code; k[pi(q)] = mult code[q]: the planted score is 8 mult against ~ mult N(0, 1)
               for the other keys — near one-hot rows whose key walks over every position of every tile, query 0's the last
      up/down  k *= 0.3; q[:, 0] = mult; k[:, 0] = linspace(0, 24, ntok) (down: reversed): the maximum rises in every tile and
               the mass sits in the last, ragged one / settles in tile 0 and every later tile adds small terms
      offp/n   rand with q[:, 1] = mult, k[:, 1] = +-mult: scores near +-mult^2 / 8 = +-288
      same     every key row equals key row 0: p = 1 / ntok, out = mean(v), lse = s + log ntok"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(frames, ntok, 3, NH, HD, generator=g) * 1.5
    mult = MULT.get(name) if mult is None else float(mult)
    if name == "planted":
        code = torch.randint(0, 2, (frames, ntok, NH, HD), generator=g).float() * 2 - 1
        t[:, :, 0] = code
        t[:, planted_perm(ntok), 1] = mult * code
    elif name in ("up", "down"):
        ramp = torch.linspace(0, 24, ntok)
        t[:, :, 1] *= 0.3
        t[:, :, 0, :, 0] = mult
        t[:, :, 1, :, 0] = (ramp if name == "up" else ramp.flip(0))[None, :, None]
    elif name in ("offp", "offn"):
        t[:, :, 0, :, 1] = mult
        t[:, :, 1, :, 1] = mult if name == "offp" else -mult
    elif name == "same":
        t[:, :, 1] = t[:, :1, 1]
    elif name != "rand":
        raise ValueError(name)
    return t.reshape(frames * ntok, 3 * DM).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- emulations
def emulate_stream(q, k, v, tile=64, mutate=None):
    """The streaming algorithm's arithmetic restated in torch f32 for one head (q, k, v [ntok, 64]): f32 scores, a running
    maximum and sum per query over tiles of `tile` keys, keys past the end loaded as copies of the last row and masked to -inf
    before the tile maximum (their V rows zero), P rounded to bf16 before P V, f32 accumulator rescaled when the maximum
    rises, the quotient rounded to bf16.  -> out bf16 [ntok, 64], lse f32 [ntok].
    mutate: one deliberate error —
      no_mask        keys past the end keep their score (they count as copies of the last key)
      no_rescale     the accumulator and the running sum are not multiplied by alpha
      drop_last_key  the last real key is masked too
      stale_max      the exponent takes the TILE's maximum where the running maximum belongs"""
    assert mutate is None or mutate in MUTATIONS
    q, k, v = q.float(), k.float(), v.float()
    ntok = q.shape[0]
    c = torch.tensor(SCALE * LOG2E, dtype=torch.float32)
    m = torch.full((ntok,), float("-inf"))
    lsum = torch.zeros(ntok)
    o = torch.zeros(ntok, v.shape[1])
    nvalid = ntok - 1 if mutate == "drop_last_key" else ntok
    for t0 in range(0, ntok, tile):
        idx = torch.arange(t0, t0 + tile)
        kt = k[idx.clamp(max=ntok - 1)]
        vt = torch.where((idx < ntok)[:, None], v[idx.clamp(max=ntok - 1)], torch.zeros(()))
        s = q @ kt.t()
        if mutate != "no_mask":
            s[:, idx >= nvalid] = float("-inf")
        elif nvalid < ntok:
            s[:, idx == ntok - 1] = float("-inf")
        tmax = s.amax(-1)
        mn = torch.maximum(m, tmax)
        alpha = torch.exp2((m - mn) * c)
        ref_max = tmax if mutate == "stale_max" else mn
        e = torch.exp2(s * c - (ref_max * c)[:, None])
        if mutate == "no_rescale":
            alpha = torch.ones_like(alpha)
        lsum = lsum * alpha + e.sum(-1)
        o = o * alpha[:, None] + e.to(torch.bfloat16).float() @ vt
        m = mn
    return (o / lsum[:, None]).to(torch.bfloat16), m * SCALE + torch.log(lsum)


def emulate_bwd(qkv, dout, frames, ntok):
    """The resident forward + backward restated in torch f32 with a bf16 cast wherever attn_vit.hip casts:
      forward   P~ = exp2((s - m) c) -> bf16 before P V (line 159), out = acc / sum -> bf16 (169), lse = m scale + log sum f32 (172)
      backward  P = exp2(s c - lse log2e) f32 (322), delta = rowsum(dO * the saved bf16 out) f32 (285-291),
                dS = P (dP - delta) f32 -> bf16 for dQ (326) and for dK (331), P -> bf16 for dV (331),
                dQ = dS K scale -> bf16 (361), dK = dS^T Q scale -> bf16, dV = P^T dO -> bf16 (374)
    MFMA accumulation order and the hardware exp2 are not modelled.  -> d qkv bf16 [frames * ntok, 1152]"""
    bf = lambda x: x.to(torch.bfloat16).float()
    q, k, v = (x.float() for x in heads(qkv, frames, ntok))
    do = dout.float().reshape(frames, ntok, NH, HD).permute(0, 2, 1, 3)
    c = SCALE * LOG2E
    s = q @ k.transpose(-2, -1)
    m = s.amax(-1, keepdim=True)
    e = torch.exp2((s - m) * c)
    z = e.sum(-1, keepdim=True)
    out = bf((bf(e) @ v) / z)
    lse = m * SCALE + z.log()
    p = torch.exp2(s * c - lse * LOG2E)
    delta = (do * out).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-2, -1) - delta)
    dv = bf(p).transpose(-2, -1) @ do
    dk = (bf(ds).transpose(-2, -1) @ q) * SCALE
    dq = (bf(ds) @ k) * SCALE
    g = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4)              # [frames, ntok, 3, 6, 64]
    return g.reshape(frames * ntok, 3 * DM).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- backward cases and bars
BWD_SEED, BWD_FRAMES = 70, 3
BWD_LAYOUTS = ("rand", "planted", "up", "down", "offp", "offn")
# The knob of each layout in the backward cases, per token count.  The rule: where the emulation's own rel-L2 against fp64 is
# above the 1.5e-2 bar of the backward, the layout is softened (first value of planted 1, 0.75, 0.5 / up, down 4, 3, 2) until
# the emulation alone is inside; the bar is never raised.  planted starts from k = 1 code (fully one-hot rows make dQ and dK
# vanish, and a relative error on nothing is meaningless) and gave dq 1.7e-2 (197) / 8.7e-2, 1.6e-2 (37: k = 1, 0.75);
# up / down gave dq 1.6e-2 .. 1.8e-2 at 4 and 1.53e-2 .. 1.57e-2 at 3: the ramp of k[:, 0] (up to 24) multiplies the bf16
# rounding of dS, whose exact row sums are zero.  offp / offn stay at 48 (dq 1.30e-2 / 1.36e-2, same cause).
BWD_MULT = {"rand": None, "planted": {197: 0.75, 37: 0.5}, "up": 2.0, "down": 2.0, "offp": None, "offn": None}
# emulate_bwd against fp64 autograd, per part (dq, dk, dv), measured on the CPU; test_attn_ref_host.py recomputes them
BWD_EMU = {
    ("rand", 197): [2.865e-03, 2.714e-03, 2.322e-03],
    ("planted", 197): [3.904e-03, 3.483e-03, 2.499e-03],
    ("up", 197): [1.294e-02, 2.393e-03, 2.342e-03],
    ("down", 197): [1.300e-02, 2.365e-03, 2.363e-03],
    ("offp", 197): [1.299e-02, 2.679e-03, 2.353e-03],
    ("offn", 197): [1.299e-02, 2.678e-03, 2.354e-03],
    ("rand", 37): [2.987e-03, 2.930e-03, 2.365e-03],
    ("planted", 37): [3.522e-03, 3.271e-03, 2.568e-03],
    ("up", 37): [1.279e-02, 2.478e-03, 2.372e-03],
    ("down", 37): [1.264e-02, 2.492e-03, 2.366e-03],
    ("offp", 37): [1.358e-02, 2.883e-03, 2.313e-03],
    ("offn", 37): [1.358e-02, 2.882e-03, 2.315e-03],
}


def bwd_case(name, ntok):
    """qkv bf16 [3 ntok, 1152], dout bf16 [3 ntok, 384] (CPU)"""
    mult = BWD_MULT[name]
    qkv = layouts(name, BWD_FRAMES, ntok, BWD_SEED + ntok, mult[ntok] if isinstance(mult, dict) else mult)
    g = torch.Generator().manual_seed(BWD_SEED + 1000 + ntok)
    return qkv, torch.randn(BWD_FRAMES * ntok, DM, generator=g).to(torch.bfloat16)


def bwd_bars(name, ntok):
    """per part: min(1.5e-2, 4 x the emulation's rel-L2 against fp64), floored at the rand layout's emulated value.  The 4 x
    covers MFMA accumulation order and the hardware exp2, which emulate_bwd does not model."""
    return [max(min(1.5e-2, 4.0 * e), r) for e, r in zip(BWD_EMU[(name, ntok)], BWD_EMU[("rand", ntok)])]
