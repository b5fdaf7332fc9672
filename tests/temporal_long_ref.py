"""References, derived bounds and fp32 restatements for the streaming temporal attention (csrc/tattn_long.hip): the kit of
temporal_ref.py (imported as R: heads, masks, layouts, attn_fp64, attn_bwd_fp64, host_keep, worst_ratio, rel_l2_parts,
split_slabs) carried past S = 96.  Shared by test_temporal_long_host.py and test_temporal_long_gpu.py; torch on the CPU only.

Bounds (derived from tattn_long.hip, not tuned).  R's constants assume S <= 96: the "96-term sum" inside its 128 and the
97-term P v chain.  The long forms, per query, nt = ceil(S / TILE) key tiles of TILE = 64:
  E = eps (194 sigma + 4 smax + (S + 32) + (nt + 1) (4 smax + 3)).
  * 194 sigma + 4 smax: a score and the exponent s - m, exactly as in R (the same dot_tile, the same __expf).
  * S + 32: the row sum has S non-negative terms in whatever order (a lane adds its own 4 keys per 16 tile after tile, the four
    lane groups are added at the end: no path is longer than S roundings); v_exp_f32, the reciprocal, the products and the
    second-order slack are R's 32.
  * (nt + 1) (4 smax + 3): the online form multiplies the running sum (and the accumulator) by alpha = exp(m - m') once per key tile.
    m - m' is rounded (<= 2 eps smax) and multiplied by log2(e) inside __expf (another 2 eps smax), v_exp_f32 adds ~2 eps and the
    product one: a relative error of (4 smax + 3) eps per tile in everything accumulated before it.  A tile that does not move
    the max has alpha = exp(0) = 1 exactly; nt is the worst case.  The two-pass map form takes its row sum from the same online
    recurrence, run by each of its four waves over a quarter of every key tile (at most nt factors on any term) and combined with
    one more factor exp(m_w - m) per wave: the + 1.  So P carries the term too.
  |P - ref| <= E ref + 1e-30.  P' = P keep / (1 - p): one more product (inside the 32).
  avg = ((P'_0 / 4 + P'_1 / 4) + P'_2 / 4) + P'_3 / 4, a FIXED order (one workgroup loops over the heads): the quarters are
  exact, three additions: |avg - ref| <= mean_h(E P') + 4 eps ref + 1e-30 (R's form; no atomics, no pre-zero contract).
  ctx = P' v is an S-term fmaf chain (the online form: e v accumulated, rescaled per tile - inside E - and divided once):
  |ctx - ref| <= (E + (S + 1) eps) A + 1e-30, A = P' |v|.  Both forward forms (one pass without the map, two with it) are held
  to this bound; the restatement returns both (ctx1: one pass, ctx: with the map).
The bars follow the project's rule: forward min(1, 8 r_emu) of the bound per layout and quantity (R_EMU_LONG); backward per
part relative L2 against fp64 autograd <= 8 x the restatement's own (BWD_EMU_LONG), floored at the rand layout's value at the
same S.  Nothing here is calibrated from a kernel's output: `PYTHONPATH=.:tests python tests/temporal_long_ref.py` prints both tables
from the CPU restatements and test_temporal_long_host.py recomputes them.

The dropout mask element of (b, h, i, j) is mask_index = ((b 4 + h) S + i) S + j as a 64-bit integer: 4 x 2001^2 x B crosses
2^32 at B = 269, which the launcher accepts, so a 32-bit index is a reachable error (mutation mask_index_32bit)."""
import functools

import torch

import temporal_ref as R

TILE = 64                                    # rows of a staging tile of tattn_long.hip (LT)
LONG_MAX_S = 2001
S_LONG = (97, 112, 113, 128, 129, 191, 257, 2001)
DROP_CASES_LONG = tuple((S, p, site) for S in (97, 129) for p in (0.1, 0.5) for site in (0, 7))
MUTATIONS_LONG = ("mask_off_by_one", "dropout_transposed", "dropout_head_stride", "keep_unscaled", "avg_of_kept_heads",
                  "drop_last_slab", "stale_rescale", "tile_tail_unmasked", "mask_index_32bit")
EPS = R.EPS


def tiles(S):
    """key (query) tiles of sais_temporal_attn_fwd_long / _bwd_long; None = rejected"""
    return (S + TILE - 1) // TILE if 1 <= S <= LONG_MAX_S else None


def bwd_workspace_bytes(B, S):
    """sais_temporal_attn_long_bwd_workspace_bytes: dctx summed [B S, 384] + row max, 1 / row sum, rowsum(P dP) [B, 4, S] each"""
    return (B * S * R.DM + 3 * B * R.TH * S) * 4


def mask_index(b, h, i, j, S, bits=64):
    """dropout mask element of (sequence, head, query, key); bits = 32: the mutation"""
    return (((b * R.TH + h) * S + i) * S + j) % (1 << bits)


def long_masks(S):
    """bool [B, S]: R.masks(S) for the small sizes; at the cap one ragged sequence, the last 37 keys padded"""
    if S < LONG_MAX_S:
        return R.masks(S)
    m = torch.zeros(1, S, dtype=torch.bool)
    m[0, S - 37:] = True
    return m


def long_case(name, S):
    """(qkv fp32 [B * S, 1152], pad bool [B, S]) on the CPU"""
    pad = long_masks(S)
    return R.layouts(name, pad, R.case_seed(name, S)), pad


def attn_fp64_long(qkv, pad, keep=None, p=0.0):
    """R.attn_fp64 with E in its long form (module docstring)"""
    B, S = pad.shape
    ref = R.attn_fp64(qkv, pad, keep, p)
    q, k, _ = R.heads(qkv.double(), B, S)
    smax = ((q * R.SCALE) @ k.transpose(-2, -1)).masked_fill(pad.view(B, 1, 1, S), 0.0).abs().amax(-1)
    nt = tiles(S)
    ref["E"] = ref["E"] + EPS * ((S + 32 - 128) + (nt + 1) * (4 * smax + 3))
    return ref


def ctx_bound_long(ref):
    B, _, S = ref["E"].shape
    e = (ref["E"] + (S + 1) * EPS).transpose(1, 2).reshape(B * S, R.TH, 1)
    return (e * ref["A"].view(B * S, R.TH, R.THD)).reshape(B * S, R.DM) + 1e-30


def attn_ratios_long(got, ref):
    """{P, avg, ctx, ctx1} (those `got` has): worst |got - ref| / bound"""
    r = {}
    if "P" in got:
        r["P"] = R.worst_ratio(got["P"], ref["P"], R.p_bound(ref))
    if "avg" in got:
        r["avg"] = R.worst_ratio(got["avg"], ref["avg"], R.avg_bound(ref))
    for k in ("ctx", "ctx1"):
        if k in got:
            r[k] = R.worst_ratio(got[k], ref["ctx"], ctx_bound_long(ref))
    return r


# ---------------------------------------------------------------------------------------------- fp32 restatements
def _prep(qkv, pad, keep, p, mutate):
    """q (scaled), k, v fp32 [B, 4, S', 96], pad [B, S'], keep factor fp32 [B, 4, S, S'] (1 / (1 - p) or 0) after the mutations
    that act on the inputs; S' = S, or 64 nt with tile_tail_unmasked"""
    B, S = pad.shape
    q, k, v = (t.float() for t in R.heads(qkv, B, S))
    pad = pad.clone()
    if mutate == "mask_off_by_one":
        for b in range(B):
            idx = torch.nonzero(pad[b]).flatten()
            if idx.numel():
                pad[b, idx[0]] = False
    kp = None
    if keep is not None:
        kp = keep
        if mutate == "dropout_transposed":
            kp = keep.transpose(-2, -1)
        elif mutate == "dropout_head_stride":
            kp = keep.reshape(R.TH, B, S, S).transpose(0, 1)
        inv = torch.tensor(1.0 if mutate == "keep_unscaled" else 1.0 / (1.0 - p), dtype=torch.float32)
        kp = kp.float() * inv
    if mutate == "tile_tail_unmasked":
        extra = TILE * tiles(S) - S
        k = torch.cat((k, torch.zeros(B, R.TH, extra, R.THD)), 2)
        v = torch.cat((v, torch.zeros(B, R.TH, extra, R.THD)), 2)
        pad = torch.cat((pad, torch.zeros(B, extra, dtype=torch.bool)), 1)
        if kp is not None:
            kp = torch.cat((kp, torch.ones(B, R.TH, S, extra)), 3)
    return q * torch.tensor(R.SCALE, dtype=torch.float32), k, v, pad, kp


def _online_stats(q, k, pad, extra=None):
    """the online recurrence of tattn_long.hip over 64-key tiles: running max m, sum l [B, 4, S, 1]; extra = (w [.., S'], like l):
    a second sum of exp(s - m) w carried along (rowsum(P dP) of the backward)"""
    B, S2 = pad.shape
    m = torch.full(q.shape[:3] + (1,), float("-inf"))
    l = torch.zeros_like(m)
    d = torch.zeros_like(m)
    for t0 in range(0, S2, TILE):
        s = (q @ k[:, :, t0:t0 + TILE].transpose(-2, -1)).masked_fill(pad[:, t0:t0 + TILE].view(B, 1, 1, -1), float("-inf"))
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)
        e = torch.exp(s - mn)
        l = l * alpha + e.sum(-1, keepdim=True)
        if extra is not None:
            d = d * alpha + (e * extra[..., t0:t0 + TILE]).sum(-1, keepdim=True)
        m = mn
    return m, l, d


def emulate_long(qkv, pad, keep=None, p=0.0, mutate=None):
    """The forward's arithmetic in torch float32, tile by tile as tattn_long.hip orders it.  -> dict(P, avg, ctx: the two-pass map
    form; ctx1: the one-pass online form).  MFMA summation order, the per-lane partial row sums, the split of a key tile over the
    four waves of the map form and the hardware exp2 are not modelled.  mutate: R's input mutations, and
      stale_rescale        the accumulator of the online form is not rescaled when the running max moves
      tile_tail_unmasked   the zero-filled keys S .. 64 nt - 1 of the last staging tile count (score 0, value 0)
    mask_index_32bit is not an input mutation: it shows from B = 269 at S = 2001 only, a 4.3-GB mask; it is stated as the rule
    mask_index and the host test checks that function."""
    assert mutate is None or (mutate in MUTATIONS_LONG and mutate != "mask_index_32bit")
    B, S = pad.shape
    q, k, v, pad2, kp = _prep(qkv, pad, keep, p, mutate)
    S2 = pad2.shape[1]
    # ---- two passes: statistics, then normalised probabilities
    m, l, _ = _online_stats(q, k, pad2)
    inv = 1.0 / l
    s = (q @ k.transpose(-2, -1)).masked_fill(pad2.view(B, 1, 1, S2), float("-inf"))
    P = torch.exp(s - m) * inv
    Pd = P if kp is None else P * kp
    ctx = torch.zeros(B, R.TH, S, R.THD)
    for t0 in range(0, S2, TILE):
        ctx = ctx + Pd[..., t0:t0 + TILE] @ v[:, :, t0:t0 + TILE]
    Pd = Pd[..., :S]
    if mutate == "avg_of_kept_heads" and keep is not None:
        avg = Pd.sum(1) / keep.sum(1).clamp(min=1).float()
    else:
        avg = ((Pd[:, 0] * 0.25 + Pd[:, 1] * 0.25) + Pd[:, 2] * 0.25) + Pd[:, 3] * 0.25
    # ---- one pass: online rescaling, one division at the end
    m1 = torch.full_like(m, float("-inf"))
    l1 = torch.zeros_like(m)
    acc = torch.zeros(B, R.TH, S, R.THD)
    for t0 in range(0, S2, TILE):
        st = s[..., t0:t0 + TILE]
        mn = torch.maximum(m1, st.amax(-1, keepdim=True))
        alpha = torch.exp(m1 - mn)
        e = torch.exp(st - mn)
        l1 = l1 * alpha + e.sum(-1, keepdim=True)
        if kp is not None:
            e = torch.where(kp[..., t0:t0 + TILE] != 0, e, torch.zeros(()))
        acc = (acc if mutate == "stale_rescale" else acc * alpha) + e @ v[:, :, t0:t0 + TILE]
        m1 = mn
    fin = torch.tensor(1.0 if (kp is None or mutate == "keep_unscaled") else 1.0 / (1.0 - p), dtype=torch.float32) / l1
    flat = lambda t: t.transpose(1, 2).reshape(B * S, R.DM)
    return dict(P=P[..., :S], avg=avg, ctx=flat(ctx), ctx1=flat(acc * fin))


def emulate_bwd_long(qkv, pad, slabs, keep=None, p=0.0, mutate=None):
    """The backward's arithmetic in torch float32 as tattn_long.hip orders it: dctx = slab 0 + slab 1 + ... in turn; row max, row
    sum and rowsum(P dP) from the online recurrence; dS = P (dP - rowsum) scale; dq summed over key tiles, dk and dv over
    query tiles.  -> d qkv [B * S, 1152].  mutate = drop_last_slab: the last slab is not added; stale_rescale: the online
    rowsum(P dP) is not rescaled when the max moves."""
    B, S = pad.shape
    n = slabs.shape[0] - (1 if mutate == "drop_last_slab" else 0)
    G = torch.zeros(B * S, R.DM)
    for z in range(n):
        G = slabs[z].float() if z == 0 else G + slabs[z].float()
    q, k, v, pad2, kp = _prep(qkv, pad, keep, p, None if mutate in ("drop_last_slab", "stale_rescale") else mutate)
    g = G.view(B, S, R.TH, R.THD).transpose(1, 2)
    dp = g @ v.transpose(-2, -1)
    if kp is not None:
        dp = dp * kp
    if mutate == "stale_rescale":
        m, l, _ = _online_stats(q, k, pad2)
        s0 = (q @ k.transpose(-2, -1)).masked_fill(pad2.view(B, 1, 1, -1), float("-inf"))
        d = torch.zeros_like(m)
        mr = torch.full_like(m, float("-inf"))
        for t0 in range(0, pad2.shape[1], TILE):
            mr = torch.maximum(mr, s0[..., t0:t0 + TILE].amax(-1, keepdim=True))
            d = d + (torch.exp(s0[..., t0:t0 + TILE] - mr) * dp[..., t0:t0 + TILE]).sum(-1, keepdim=True)
    else:
        m, l, d = _online_stats(q, k, pad2, extra=dp)
    inv = 1.0 / l
    dot = d * inv
    s = (q @ k.transpose(-2, -1)).masked_fill(pad2.view(B, 1, 1, -1), float("-inf"))
    P = torch.exp(s - m) * inv
    scale = torch.tensor(R.SCALE, dtype=torch.float32)
    dS = P * (dp - dot) * scale
    Pd = P if kp is None else P * kp
    q0 = R.heads(qkv, B, S)[0].float()
    dq = torch.zeros(B, R.TH, S, R.THD)
    dk = torch.zeros(B, R.TH, pad2.shape[1], R.THD)
    dv = torch.zeros_like(dk)
    for t0 in range(0, pad2.shape[1], TILE):
        dq = dq + dS[..., t0:t0 + TILE] @ k[:, :, t0:t0 + TILE]
    for t0 in range(0, S, TILE):
        dk = dk + dS[:, :, t0:t0 + TILE].transpose(-2, -1) @ q0[:, :, t0:t0 + TILE]
        dv = dv + Pd[:, :, t0:t0 + TILE].transpose(-2, -1) @ g[:, :, t0:t0 + TILE]
    out = torch.stack((dq, dk[:, :, :S], dv[:, :, :S]))                     # [3, B, 4, S, 96]
    return out.permute(1, 3, 0, 2, 4).reshape(B * S, 3 * R.DM)


# ---------------------------------------------------------------------------------------------- cases, shared references
@functools.lru_cache(maxsize=None)
def fwd_ref(name, S):
    """(qkv, pad, fp64 reference) of the p = 0 case, computed once per process and never modified"""
    qkv, pad = long_case(name, S)
    return qkv, pad, attn_fp64_long(qkv, pad)


def drop_case(S, p, site):
    """(qkv, pad, host keep mask) of a rand-layout dropout case on the CPU"""
    qkv, pad = long_case("rand", S)
    return qkv, pad, R.host_keep(pad.shape[0], S, p, 1000 * site + S)


def r_emu_long(name):
    """what R_EMU_LONG records for a layout: the worst ratios over every S of S_LONG at p = 0 and (rand) DROP_CASES_LONG"""
    worst = dict(P=0.0, avg=0.0, ctx=0.0, ctx1=0.0)
    for S in S_LONG:
        qkv, pad, ref = fwd_ref(name, S)
        for k, x in attn_ratios_long(emulate_long(qkv, pad), ref).items():
            worst[k] = max(worst[k], x)
    if name == "rand":
        for S, p, site in DROP_CASES_LONG:
            qkv, pad, keep = drop_case(S, p, site)
            for k, x in attn_ratios_long(emulate_long(qkv, pad, keep, p), attn_fp64_long(qkv, pad, keep, p)).items():
                worst[k] = max(worst[k], x)
    return worst


# worst ratio of emulate_long() to the bounds per layout; measured on the CPU, recomputed by test_temporal_long_host.py
R_EMU_LONG = {
    "rand": dict(P=2.290e-02, avg=1.749e-02, ctx=1.046e-02, ctx1=9.866e-03),
    "peaky": dict(P=2.968e-02, avg=2.575e-02, ctx=1.955e-02, ctx1=1.965e-02),
    "planted": dict(P=7.697e-02, avg=7.640e-02, ctx=4.956e-02, ctx1=4.956e-02),
    "same": dict(P=5.732e-03, avg=5.600e-03, ctx=1.472e-02, ctx1=1.459e-02),
}


def fwd_bar_long(name, what):
    """fraction of the derived bound the kernel must stay inside: min(1, 8 r_emu)"""
    return min(1.0, 8.0 * R_EMU_LONG[name][what])


BWD_SEED = R.BWD_SEED


def bwd_case_long(name, S):
    """(qkv fp32 [B * S, 1152], pad bool [B, S], dctx fp32 [B * S, 384]) on the CPU"""
    qkv, pad = long_case(name, S)
    g = torch.Generator().manual_seed(BWD_SEED + 1000 + S)
    return qkv, pad, torch.randn(pad.shape[0] * S, R.DM, generator=g)


@functools.lru_cache(maxsize=None)
def bwd_ref(name, S, p=0.0):
    """(qkv, pad, gapped three-slab buffer of dctx, keep or None, fp64 autograd on the fp64 sum of the slabs): once per process"""
    qkv, pad, dctx = bwd_case_long(name, S)
    keep = R.host_keep(pad.shape[0], S, p, BWD_SEED + S) if p > 0 else None
    buf, total = R.split_slabs(dctx, 3, 64, BWD_SEED + S)
    return qkv, pad, buf, keep, R.attn_bwd_fp64(qkv, pad, total, keep, p)


def bwd_emu_case_long(name, S, p=0.0):
    """what BWD_EMU_LONG records: the restatement on dctx handed over as three slabs against fp64 autograd, per part"""
    qkv, pad, buf, keep, ref = bwd_ref(name, S, p)
    return R.rel_l2_parts(emulate_bwd_long(qkv, pad, R.slab_view(buf, qkv.shape[0]), keep, p), ref)


AGREE_S = (33, 96)                           # where the GPU test runs the resident and the streaming kernels on the same inputs
BWD_KEYS = tuple((n, S, 0.0) for n in R.BWD_LAYOUTS for S in S_LONG) + tuple(("rand", S, p) for S in (97, 129) for p in (0.1, 0.5)) + \
    tuple(("rand", S, 0.0) for S in AGREE_S)
# bwd_emu_case_long per part (dq, dk, dv), keyed (layout, S, p); p > 0 with host_keep(B, S, p, BWD_SEED + S)
BWD_EMU_LONG = {
    ("rand", 97, 0.0): [2.957e-07, 3.112e-07, 1.940e-07],
    ("rand", 112, 0.0): [2.885e-07, 3.117e-07, 1.970e-07],
    ("rand", 113, 0.0): [2.936e-07, 3.085e-07, 1.957e-07],
    ("rand", 128, 0.0): [2.939e-07, 3.166e-07, 1.907e-07],
    ("rand", 129, 0.0): [2.944e-07, 3.176e-07, 1.981e-07],
    ("rand", 191, 0.0): [2.908e-07, 3.140e-07, 1.966e-07],
    ("rand", 257, 0.0): [2.899e-07, 3.196e-07, 1.890e-07],
    ("rand", 2001, 0.0): [4.477e-07, 4.499e-07, 4.146e-07],
    ("peaky", 97, 0.0): [2.196e-06, 2.229e-06, 7.680e-07],
    ("peaky", 112, 0.0): [2.305e-06, 2.357e-06, 7.967e-07],
    ("peaky", 113, 0.0): [2.379e-06, 2.426e-06, 8.066e-07],
    ("peaky", 128, 0.0): [2.200e-06, 2.234e-06, 8.036e-07],
    ("peaky", 129, 0.0): [2.509e-06, 2.539e-06, 7.796e-07],
    ("peaky", 191, 0.0): [2.363e-06, 2.419e-06, 8.044e-07],
    ("peaky", 257, 0.0): [2.438e-06, 2.457e-06, 8.943e-07],
    ("peaky", 2001, 0.0): [3.851e-06, 3.913e-06, 1.840e-06],
    ("planted", 97, 0.0): [1.634e-04, 1.363e-04, 1.636e-07],
    ("planted", 112, 0.0): [1.427e-04, 1.292e-04, 1.686e-07],
    ("planted", 113, 0.0): [1.476e-04, 1.319e-04, 1.722e-07],
    ("planted", 128, 0.0): [1.345e-04, 1.166e-04, 1.754e-07],
    ("planted", 129, 0.0): [1.377e-04, 1.235e-04, 1.794e-07],
    ("planted", 191, 0.0): [9.615e-05, 8.345e-05, 1.767e-07],
    ("planted", 257, 0.0): [7.699e-05, 6.755e-05, 1.831e-07],
    ("planted", 2001, 0.0): [1.552e-05, 1.446e-05, 3.349e-07],
    ("rand", 97, 0.1): [3.092e-07, 3.235e-07, 1.859e-07],
    ("rand", 97, 0.5): [2.944e-07, 3.082e-07, 1.601e-07],
    ("rand", 129, 0.1): [3.086e-07, 3.297e-07, 1.985e-07],
    ("rand", 129, 0.5): [2.971e-07, 3.219e-07, 1.704e-07],
    ("rand", 33, 0.0): [2.943e-07, 2.993e-07, 1.688e-07],
    ("rand", 96, 0.0): [2.984e-07, 3.111e-07, 1.953e-07],
}


def bwd_bars_long(name, S, p=0.0):
    return [max(8.0 * e, r) for e, r in zip(BWD_EMU_LONG[(name, S, p)], BWD_EMU_LONG[("rand", S, 0.0)])]


if __name__ == "__main__":                    # prints the two tables for this module
    print("R_EMU_LONG = {")
    for name in R.LAYOUTS:
        print('    "%s": dict(%s),' % (name, ", ".join("%s=%.3e" % kv for kv in r_emu_long(name).items())))
    print("}\nBWD_EMU_LONG = {")
    for key in BWD_KEYS:
        print('    ("%s", %d, %s): [%s],' % (key + (", ".join("%.3e" % x for x in bwd_emu_case_long(*key)),)))
    print("}")
