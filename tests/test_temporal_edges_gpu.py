"""The temporal encoder kernels (csrc/tattn.hip, csrc/temporal.hip) and the row-LayerNorm backwards past their grid cap, at
their tile edges, masks, dropout and launch forms, on a real MI355X.

References are fp64 (tests/temporal_ref.py: oracle/sais_oracle.py where it has the function, fp64 autograd for gradients); the
bars are the derived ones of that module, which test_temporal_ref_host.py proves sound and sharp on the CPU, or the existing
bars of test_kernels_gpu.py where the issue keeps them.  Every output buffer is oversized and NaN-filled: what a kernel owns
must be non-NaN and inside its bar, everything else must still be NaN.  Every accumulating output starts from non-zero values
and the increment is what is checked.  Shapes are the smallest that reach the form.  The tests never ask which kernel form
ran: they compute it from the launcher's published rule (temporal_ref.tattn_tiles, nce_staged, ln_bwd_grid) and assert on
results only.  Worst observed / bar ratios go to parity.parity_log("temporal_edge_...")."""
import functools
import math

import pytest
import torch

import parity
import temporal_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from sais_amd import ops as o
    return o


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def log(name, value, bar):
    """records value / bar (bar 0: 0 when the value is 0 too) and returns it"""
    value, bar = float(value), float(bar)
    r = value / bar if bar > 0 else (0.0 if value == 0 else float("inf"))
    r = r if math.isfinite(r) else float("inf")
    parity.parity_log("temporal_edge_" + name, r, 1.0)
    return r


def check(name, got, ref, bound):
    """every element of got inside ref +- bound (tensors or floats); logs the worst ratio"""
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref.double(), float(bound))
    r = log(name, R.worst_ratio(got, ref.double().to(got.device), bound.double().to(got.device) + 1e-300), 1.0)
    assert r <= 1.0, (name, r)


def owned(buf, n):
    """the first n entries of the leading dimension are the kernel's: no NaN there, nothing but NaN after"""
    assert torch.isnan(buf[n:]).all(), "wrote past what it owns"
    assert not torch.isnan(buf[:n]).any(), "left NaN in what it owns"
    return buf[:n]


# ------------------------------------------------------------------------------------------------ attention forward
@functools.lru_cache(maxsize=None)
def _fwd_case(name, S):
    """(qkv, bool pad, u8 pad) on the device: made once, shared, never written to"""
    pad = R.masks(S)
    return R.layouts(name, pad, R.case_seed(name, S)).to(DEV), pad.to(DEV), pad.to(torch.uint8).to(DEV)


def _attn_fwd(ops, qkv, padu, S, want_avg=True, p=0.0, rng=None, site=0):
    B = padu.shape[0]
    ctx, avg = nan(B * S + 3, 384), nan(B + 1, S, S) if want_avg else None
    ops.temporal_attn_fwd(qkv, padu, B, S, ctx, avg, p, rng, site)
    return owned(ctx, B * S), owned(avg, B) if want_avg else None


def _check_fwd(tag, name, ctx, avg, ref):
    r_ctx = log(f"fwd_ctx_{tag}", R.worst_ratio(ctx, ref["ctx"], R.ctx_bound(ref)), R.fwd_bar(name, "ctx"))
    r_avg = log(f"fwd_avg_{tag}", R.worst_ratio(avg, ref["avg"], R.avg_bound(ref)), R.fwd_bar(name, "avg"))
    print(f"{tag}: ctx {r_ctx:.3f}, avg {r_avg:.3f} of the bar ({R.fwd_bar(name, 'ctx'):.3f}, {R.fwd_bar(name, 'avg'):.3f} of the bound)")
    assert r_ctx <= 1.0 and r_avg <= 1.0, (tag, r_ctx, r_avg)


@pytest.mark.parametrize("name", R.LAYOUTS)
@pytest.mark.parametrize("S", R.S_LIST)
def test_attn_fwd_edges(ops, S, name):
    """one sequence per mask pattern: nothing masked, only key 0, a mask that ends on / one past the tile edge, holes"""
    assert R.tattn_tiles(S) == (S + 15) // 16
    qkv, pad, padu = _fwd_case(name, S)
    ref = R.attn_fp64(qkv, pad)
    ctx, avg = _attn_fwd(ops, qkv, padu, S)
    _check_fwd(f"{name}_S{S}", name, ctx, avg, ref)
    if name == "same":                                           # every unmasked probability is float32(1 / n), masked ones 0
        n = (~pad).sum(1).float()
        want = torch.where(pad, torch.zeros((), device=DEV), (1.0 / n)[:, None].expand(-1, S))[:, None, :].expand(-1, S, -1)
        assert float((avg - want).abs().max()) <= 2 * R.EPS      # four quarters added in any order
    assert float(avg[pad[:, None, :].expand(-1, S, -1)].abs().max() if pad.any() else 0.0) == 0.0
    ctx2, none = _attn_fwd(ops, qkv, padu, S, want_avg=False)
    assert none is None and torch.equal(ctx2, ctx)
    ctx3, avg3 = _attn_fwd(ops, qkv, padu, S)
    assert torch.equal(ctx3, ctx)                                # avg is summed with atomics: bounded, not bit-equal
    assert R.worst_ratio(avg3, ref["avg"], R.avg_bound(ref)) <= R.fwd_bar(name, "avg")


def test_attn_fwd_many_sequences(ops):
    B, S = 300, 33
    pad = R.masks(S).repeat(B // 5, 1)
    qkv = R.layouts("rand", pad, 4242).to(DEV)
    pad = pad.to(DEV)
    ctx, avg = _attn_fwd(ops, qkv, pad.to(torch.uint8), S)
    _check_fwd("rand_S33_B300", "rand", ctx, avg, R.attn_fp64(qkv, pad))


@pytest.mark.parametrize("S,p,site", R.DROP_CASES)
def test_attn_fwd_dropout(ops, S, p, site):
    """the keep mask is the library's own (sais_dropout_mask at the same state and site), element ((b 4 + h) S + i) S + j; the
    returned map is the dropped one; advancing the state changes the draw"""
    qkv, pad, padu = _fwd_case("rand", S)
    B = pad.shape[0]
    rng = ops.rng_state(1234 + S, DEV)
    res = []
    for trial in range(2):
        keep = ops.dropout_mask(B * 4 * S * S, p, rng, site, DEV).view(B, 4, S, S).bool()
        frac = float(keep.float().mean())
        assert abs(frac - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / keep.numel()), frac
        ref = R.attn_fp64(qkv, pad, keep, p)
        ctx, avg = _attn_fwd(ops, qkv, padu, S, True, p, rng, site)
        _check_fwd(f"rand_S{S}_p{p}_site{site}", "rand", ctx, avg, ref)
        ctx2, _ = _attn_fwd(ops, qkv, padu, S, False, p, rng, site)
        assert torch.equal(ctx2, ctx)
        res.append((keep, ctx))
        ops.rng_advance(rng)
    assert not torch.equal(res[0][0], res[1][0]) and not torch.equal(res[0][1], res[1][1])
    if site == 0:
        other = ops.dropout_mask(B * 4 * S * S, p, rng, 7, DEV).view(B, 4, S, S).bool()
        assert not torch.equal(other, ops.dropout_mask(B * 4 * S * S, p, rng, 0, DEV).view(B, 4, S, S).bool())


# ------------------------------------------------------------------------------------------------ attention backward
def _attn_bwd(ops, qkv, padu, S, dctx, p=0.0, rng=None, site=0):
    B = padu.shape[0]
    dqkv = nan(B * S + 3, 1152)
    ops.temporal_attn_bwd(qkv, padu, B, S, dctx, dqkv, p, rng, site)
    return owned(dqkv, B * S)


def _check_bwd(tag, got, ref, bars, pad):
    rel = R.rel_l2_parts(got, ref)
    rs = [log(f"bwd_{part}_{tag}", g, b) for part, g, b in zip(("dq", "dk", "dv"), rel, bars)]
    print(f"{tag}: " + ", ".join(f"{part} {g:.3e} (bar {b:.3e})" for part, g, b in zip(("dq", "dk", "dv"), rel, bars)))
    assert all(r <= 1.0 for r in rs), (tag, rel, bars)
    B, S = pad.shape
    if pad.any():
        assert float(got.view(B, S, 3, 384)[:, :, 1:][pad].abs().max()) == 0.0, "dk / dv of a masked key"


@pytest.mark.parametrize("name", R.BWD_LAYOUTS)
@pytest.mark.parametrize("S", R.S_LIST)
def test_attn_bwd_edges(ops, S, name):
    """dctx plain and as 1, 2, 3 raw slabs a gapped stride apart (NaN in the gaps), each against fp64 autograd on the fp64 sum
    of what the slabs hold"""
    qkv, pad, dctx = R.bwd_case(name, S)
    qkv, pad, padu = qkv.to(DEV), pad.to(DEV), pad.to(torch.uint8).to(DEV)
    M = pad.shape[0] * S
    bars = R.bwd_bars(name, S)
    got = _attn_bwd(ops, qkv, padu, S, dctx.to(DEV))
    _check_bwd(f"{name}_S{S}_plain", got, R.attn_bwd_fp64(qkv, pad, dctx.to(DEV)), bars, pad)
    assert torch.equal(_attn_bwd(ops, qkv, padu, S, dctx.to(DEV)), got)
    for n in (1, 2, 3):
        buf, total = R.split_slabs(dctx, n, 64, 10 * S + n)
        buf = buf.to(DEV)
        slabs = R.slab_view(buf, M)
        assert slabs.stride(0) == M * 384 + 64 and slabs.data_ptr() == buf.data_ptr()
        g = _attn_bwd(ops, qkv, padu, S, slabs)
        _check_bwd(f"{name}_S{S}_slabs{n}", g, R.attn_bwd_fp64(qkv, pad, total.to(DEV)), bars, pad)
        assert torch.isnan(buf[:, M * 384:]).all()
        if n == 1:
            assert torch.equal(g, got)                           # one slab is dctx itself


@pytest.mark.parametrize("S,p,site", R.DROP_CASES)
def test_attn_bwd_dropout(ops, S, p, site):
    """the backward draws the mask the forward drew"""
    qkv, pad, dctx = R.bwd_case("rand", S)
    qkv, pad, padu, dctx = qkv.to(DEV), pad.to(DEV), pad.to(torch.uint8).to(DEV), dctx.to(DEV)
    B = pad.shape[0]
    rng = ops.rng_state(99 + S, DEV)
    keep = ops.dropout_mask(B * 4 * S * S, p, rng, site, DEV).view(B, 4, S, S).bool()
    got = _attn_bwd(ops, qkv, padu, S, dctx, p, rng, site)
    _check_bwd(f"rand_S{S}_p{p}_site{site}", got, R.attn_bwd_fp64(qkv, pad, dctx, keep, p), R.bwd_bars("rand", S, p), pad)
    assert torch.equal(_attn_bwd(ops, qkv, padu, S, dctx, p, rng, site), got)


# ------------------------------------------------------------------------------------------------ prepare
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 9, 95])
def test_prepare_forms(ops, T, B):
    S = T + 1
    M = B * S
    fs, cs = 2 * 384, T * 2 * 384 + 128                          # frame stride, clip stride > T x frame stride
    xbuf = nan(B, cs)
    x = torch.as_strided(xbuf, (B, T, 384), (cs, fs, 1))
    x.copy_(rnd(B, T, 384, seed=500 + T))
    pos, cls = rnd(T, 384, seed=501), rnd(384, seed=502)
    ref = R.prepare_fp64(x, pos, cls).reshape(M, 384)
    z32 = nan(M + 2, 384)
    ops.temporal_prepare_fwd(x, cs, fs, pos, cls, B, T, z32, None)
    assert torch.equal(owned(z32, M), ref.float())               # one fp32 add per element: exact against the rounded fp64
    z32b, z16 = nan(M + 2, 384), nan(M + 2, 384, dtype=torch.bfloat16)
    ops.temporal_prepare_fwd(x, cs, fs, pos, cls, B, T, z32b, z16)
    assert torch.equal(owned(z32b, M), z32[:M]) and torch.equal(owned(z16, M), z32[:M].to(torch.bfloat16))
    # backward: dz = dz32 (or none) + 0 / 1 / 3 slabs a gapped stride apart; dx overwritten, accumulated into, or absent
    dz32 = rnd(M, 384, seed=503)
    for use_dz, nslab, accumulate, has_dx in ((True, 0, False, True), (False, 1, True, True), (True, 3, True, True),
                                              (False, 3, False, False), (True, 1, False, True)):
        slabs, tot = None, torch.zeros(M, 384, dtype=torch.float64, device=DEV)
        if nslab:
            buf, tot = R.split_slabs(torch.randn(M, 384, generator=torch.Generator().manual_seed(504 + nslab)), nslab, 64, 505)
            buf, tot = buf.to(DEV), tot.to(DEV)
            slabs = R.slab_view(buf, M)
        d = (tot + (dz32.double() if use_dz else 0)).view(B, S, 384)
        dxbuf = nan(B, cs)
        dx = torch.as_strided(dxbuf, (B, T, 384), (cs, fs, 1))
        dx0 = rnd(B, T, 384, seed=506)
        if accumulate:
            dx.copy_(dx0)
        dpos0, dcls0 = rnd(T, 384, seed=507), rnd(384, seed=508)
        dpos, dcls = nan(T + 1, 384), nan(2, 384)
        dpos[:T], dcls[0] = dpos0, dcls0
        ops.temporal_prepare_bwd(dz32 if use_dz else None, slabs, B, T, dx if has_dx else None, cs, fs, accumulate, dpos, dcls[0])
        tag = f"T{T}_B{B}_dz{int(use_dz)}_slabs{nslab}_acc{int(accumulate)}_dx{int(has_dx)}"
        if has_dx:
            assert not torch.isnan(dx).any()
            check(f"prepare_dx_{tag}", dx.contiguous(), d[:, 1:] + (dx0.double() if accumulate else 0), 1e-5)
            dx.fill_(NAN)
        assert torch.isnan(dxbuf).all()                          # the gaps between frames and clips (and all of it without dx)
        check(f"prepare_dpos_{tag}", owned(dpos, T) - dpos0, d[:, 1:].sum(0), 1e-4)
        check(f"prepare_dcls_{tag}", owned(dcls, 1)[0] - dcls0, d[:, 0].sum(0), 1e-4)


# ------------------------------------------------------------------------------------------------ head
def _second_forms(B):
    mixed = [0, 1, 1, 0, 1][:B]
    return [("none", None), ("all0", [0] * B), ("all1", [1] * B)] + ([("mixed", mixed)] if B > 1 else [])


@pytest.mark.parametrize("streams", ["rgb", "flow", "both"])
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("B", [1, 5])
def test_head_forms(ops, B, ns, streams):
    Sr, Sf = 3, 5                                                # tokens per sequence: the two streams have different clip strides
    zr, zf = rnd(B, ns, Sr, 384, seed=600 + ns), rnd(B, ns, Sf, 384, seed=601 + ns)
    zr[0, :, 0, 7] = -1.0
    zf[0, :, 0, 7] = -2.0                                        # rep[0, 7] exactly 0: the gate on rep is strict
    zr[B - 1, 0, 0, 9] = 0.0
    zf[B - 1, ns - 1, 0, 11] = 0.0                               # z exactly 0: the gate on z is strict
    use_r, use_f = streams != "flow", streams != "rgb"
    W, bias = rnd(256, 384, seed=602, scale=0.05), rnd(256, seed=603, scale=0.1)
    WB, biasB = rnd(256, 384, seed=604, scale=0.05), rnd(256, seed=605, scale=0.1)
    demb = rnd(B, 256, seed=606)
    for sname, flags in _second_forms(B):
        tag = f"B{B}_ns{ns}_{streams}_{sname}"
        ub = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device=DEV)
        L, rep_ref, emb_ref = R.head_fp64(zr if use_r else None, zf if use_f else None, W, bias, ub, WB if flags is not None else None,
                                          biasB if flags is not None else None)
        emb_ref.backward(demb.double())
        rep, emb = nan(B + 1, 384), nan(B + 1, 256)
        ops.head_fwd(zr if use_r else None, zf if use_f else None, Sr * 384 if use_r else Sf * 384, B, W, bias, rep, emb,
                     clip_stride_flow=Sf * 384, nsnippets=ns, second=None if flags is None else (ub, WB, biasB))
        rep_ref = rep_ref.detach()
        check(f"head_rep_{tag}", owned(rep, B), rep_ref, 8 * R.EPS * rep_ref)          # a mean of <= 6 non-negative terms
        assert float(rep[0, 7]) == 0.0 and float(rep_ref[0, 7]) == 0.0
        check(f"head_emb_{tag}", owned(emb, B), emb_ref.detach(), 1e-4)
        # backward, twice from equal starting buffers: owner threads, no atomics
        start = dict(dW=rnd(256, 384, seed=607), db=rnd(256, seed=608), dWB=rnd(256, 384, seed=609), dbB=rnd(256, seed=610))
        runs = []
        for _ in range(2):
            acc = {k: torch.cat((v.clone(), nan(1, *v.shape[1:]))) for k, v in start.items()}
            dzr, dzf = nan(B, ns, Sr, 384), nan(B, ns, Sf, 384)
            ops.head_bwd(demb, W, rep, zr if use_r else None, zf if use_f else None, Sr * 384 if use_r else Sf * 384, B,
                         acc["dW"], acc["db"], dzr if use_r else None, dzf if use_f else None, clip_stride_flow=Sf * 384,
                         nsnippets=ns, second=None if flags is None else (ub, WB, acc["dWB"], acc["dbB"]))
            runs.append((acc, dzr, dzf))
        acc, dzr, dzf = runs[0]
        n = {"dW": 256, "db": 256, "dWB": 256, "dbB": 256}
        refs = {"dW": L["W"].grad, "db": L["bias"].grad}
        if flags is not None:
            refs.update(dWB=L["WB"].grad, dbB=L["biasB"].grad)
        for k, bar in (("dW", 1e-4), ("db", 1e-5), ("dWB", 1e-4), ("dbB", 1e-5)):
            if k in refs:
                check(f"head_{k}_{tag}", owned(acc[k], n[k]) - start[k], refs[k], bar)
            else:
                assert torch.equal(acc[k][:n[k]], start[k])      # no second head: its accumulators are not touched
            assert torch.equal(runs[1][0][k][:n[k]], acc[k][:n[k]])
        for use, dz, key in ((use_r, dzr, "zr"), (use_f, dzf, "zf")):
            if not use:
                assert torch.isnan(dz).all()
                continue
            assert torch.isnan(dz[:, :, 1:]).all() and not torch.isnan(dz[:, :, 0]).any()         # the CLS rows only
            check(f"head_d{key}_{tag}", dz[:, :, 0], L[key].grad[:, :, 0], 1e-5)
            assert float(dz[0, :, 0, 7].abs().max()) == 0.0
        if use_r:
            assert float(dzr[B - 1, 0, 0, 9]) == 0.0 and torch.equal(runs[1][1][:, :, 0], dzr[:, :, 0])
        if use_f:
            assert float(dzf[B - 1, ns - 1, 0, 11]) == 0.0 and torch.equal(runs[1][2][:, :, 0], dzf[:, :, 0])


# ------------------------------------------------------------------------------------------------ MIL
@pytest.mark.parametrize("B,ns,C,saturate", R.MIL_CASES)
def test_mil_forms(ops, B, ns, C, saturate):
    tag = f"B{B}_ns{ns}_C{C}" + ("_saturated" if saturate else "")
    c = R.mil_case(B, ns, C, saturate)
    d = {k: v.to(DEV) for k, v in c.items()}
    # sais_mil_forward: tokens = relu(CLS row of each snippet's sequence) + clip position, one fp32 add: exact
    z, pos = rnd(B * ns, 3, 384, seed=700), rnd(ns, 384, seed=701)
    tokens = nan(B * ns + 2, 384)
    ops.mil_forward(z, 3 * 384, pos, B, ns, tokens)
    want = (torch.relu(z[:, 0].double()).view(B, ns, 384) + pos.double()).view(B * ns, 384).float()
    assert torch.equal(owned(tokens, B * ns), want)
    # sais_mil_head
    reps, logits, att = nan(B * ns + 2, 384), nan(B * C + 3), nan(C * B * ns + 5)
    ops.mil_head(d["enc"], B, ns, C, d["WA"], d["bA"], d["WB"], d["bB"], d["w_att"], d["b_att"], d["w_fin"], d["b_fin"], reps,
                 logits, att)
    reps_ref, l_ref, a_ref = R.mil_head_ref(c)
    assert torch.equal(owned(reps, B * ns).view(B, ns, 384), reps_ref.float().to(DEV))
    att = owned(att, C * B * ns).view(C, B, ns)
    assert float((att.double().sum(-1) - 1).abs().max()) <= 1e-6
    bars = R.mil_bars()
    check(f"mil_logits_{tag}", owned(logits, B * C).view(B, C), l_ref, bars["logits"])
    check(f"mil_attention_{tag}", att, a_ref, bars["attention"])


# ------------------------------------------------------------------------------------------------ importance head
@pytest.mark.parametrize("M", [1, 3, 4, 5, 264])
def test_importance_fwd(ops, M):
    z, w, b = rnd(M, 384, seed=800 + M), rnd(384, seed=801, scale=0.1), rnd(1, seed=802)
    out = nan(M + 3)
    ops.importance_fwd(z, w, b, M, out)
    ref = torch.relu(z.double()) @ w.double() + b.double()
    check(f"importance_fwd_M{M}", owned(out, M), ref, R.importance_fwd_bound(z, w, b))


@pytest.mark.parametrize("M", [1, 63, 64, 65, 200])
def test_importance_bwd(ops, M):
    """around the 64-workgroup stride; dz is touched only where z > 0"""
    z, w, dl = rnd(M, 384, seed=810 + M), rnd(384, seed=811, scale=0.1), rnd(M, seed=812)
    z[0, 5] = 0.0
    z[M - 1, 383] = 0.0
    dz0, dw0, db0 = rnd(M, 384, seed=813), rnd(384, seed=814), rnd(1, seed=815)
    dz, dw, db = torch.cat((dz0, nan(1, 384))), torch.cat((dw0, nan(3))), torch.cat((db0, nan(3)))
    ops.importance_bwd(dl, z, w, M, dz, dw, db)
    dzb, dwb, dbb = R.importance_bwd_bounds(dl, z, w, dz0, dw0, db0[0])
    open_ = z > 0
    got = owned(dz, M)
    assert torch.equal(got[~open_], dz0[~open_])                 # bit-identical where the gate is closed, z = 0 included
    ref = dz0.double() + dl.double()[:, None] * w.double()[None, :]
    check(f"importance_bwd_dz_M{M}", got[open_], ref[open_], dzb[open_])
    check(f"importance_bwd_dw_M{M}", owned(dw, 384), dw0.double() + dl.double() @ torch.relu(z.double()), dwb)
    check(f"importance_bwd_db_M{M}", owned(db, 1), db0.double() + dl.double().sum(), dbb.reshape(1))


def _importance_case(B, T, labels_kind):
    g = torch.Generator().manual_seed(820 + B + T)
    S = T + 1
    logits, target = torch.randn(B, S, generator=g) * 2, torch.rand(B, T, generator=g)
    ipad = torch.zeros(B, S, dtype=torch.bool)
    for b in range(B):                                           # tails of 0, 1, 2, ... masked slots, the LAST slot among them:
        n = b % (T + 1) if B > 1 else min(1, T - 1)              # frame t is masked by slot t, so slot T never counts
        if n:
            ipad[b, S - n:] = True
    labels = {"mixed": torch.arange(B) % 2, "all_low": torch.zeros(B, dtype=torch.long), "none_low": torch.ones(B, dtype=torch.long)}
    return logits, target, ipad, labels[labels_kind]


@pytest.mark.parametrize("kind", ["mixed", "all_low", "none_low"])
@pytest.mark.parametrize("B,T", [(1, 1), (8, 32), (9, 32), (3, 95)])
def test_importance_loss(ops, B, T, kind):
    S = T + 1
    logits, target, ipad, labels = _importance_case(B, T, kind)
    dev = lambda t, dt: t.to(dt).to(DEV)
    args = (dev(logits, torch.float32), dev(target, torch.float32), dev(ipad, torch.uint8), dev(labels, torch.int32), B, T)
    for scale in (1.0, 0.25):
        tag = f"B{B}_T{T}_{kind}_scale{scale}"
        ref_loss, ref_grad = R.importance_loss_fp64(logits, target, ipad, labels, scale)
        lb, db = R.importance_loss_bounds(logits, target, ipad, labels, scale)
        loss, dl = nan(3), nan(B * S + 5)
        ops.importance_loss(*args, loss=loss, dlogits=dl, scale=scale)
        assert torch.isnan(loss[1:]).all()
        got = owned(dl, B * S).view(B, S)
        assert float(got[:, 0].abs().max()) == 0.0
        if bool((labels == 0).any()):
            check(f"importance_loss_{tag}", loss[:1], ref_loss.reshape(1), lb.reshape(1))
            check(f"importance_dlogits_{tag}", got, ref_grad, db)
        else:
            # no low-skill sample: the mean over an empty selection is NaN and scatters nothing back (fp64 autograd of the
            # oracle gives exactly 0), so the step's gradients stay finite
            assert math.isnan(float(ref_loss)) and float(ref_grad.abs().max()) == 0.0
            assert math.isnan(float(loss[0]))
            assert torch.equal(got, torch.zeros(B, S, device=DEV))
            log(f"importance_dlogits_{tag}", float(got.abs().max()), 0.0)
        only_loss, only_grad = nan(3), nan(B * S + 5)
        ops.importance_loss(*args, loss=only_loss, dlogits=None, scale=scale)
        ops.importance_loss(*args, loss=None, dlogits=only_grad, scale=scale)
        assert torch.equal(only_loss.isnan(), loss.isnan()) and torch.equal(only_loss[~loss.isnan()], loss[~loss.isnan()])
        assert torch.equal(only_grad[:B * S], dl[:B * S]) and torch.isnan(only_grad[B * S:]).all()


# ------------------------------------------------------------------------------------------------ NCE
@pytest.mark.parametrize("B,C", R.NCE_CASES)
def test_nce_forms(ops, B, C):
    """(56, 2) / (57, 2): the last shape whose operands are staged in LDS and the first that reads them from memory;
    B + C > 16: the wave loops take more than one round"""
    assert R.nce_staged(B, C) == ((B, C) not in ((57, 2), (300, 3)))
    emb, protos, lab = R.nce_case(B, C)
    e, pr, lb = emb.to(DEV), protos.to(DEV), lab.int().to(DEV)
    bars = R.nce_bars(B, C)
    # accumulator start: non-zero and small enough for the rounding of start + increment (eps x 2^-7 = 5e-10) to stay two
    # orders under the 1e-7 bar of the increment
    dp0 = ((torch.arange(C * 256) % 3).float() - 1.25).view(C, 256).to(DEV) * 2.0 ** -7
    for scale in (1.0, 0.25):
        tag = f"B{B}_C{C}_scale{scale}"
        ref = R.nce_ref(emb, protos, lab, scale)
        sim, probs, loss, demb = nan(B * C + 3), nan(B * C + 3), nan(3), nan(B + 2, 256)
        dpro = torch.cat((dp0, nan(1, 256)))
        ops.nce(e, pr, lb, sim, probs, loss, demb, dpro, loss_scale=scale)
        check(f"nce_sim_{tag}", owned(sim, B * C).view(B, C), ref["sim"], bars["sim"])
        check(f"nce_probs_{tag}", owned(probs, B * C).view(B, C), ref["probs"], bars["probs"])
        check(f"nce_loss_{tag}", owned(loss, 1), ref["loss"].reshape(1), bars["loss"])
        check(f"nce_demb_{tag}", owned(demb, B), ref["demb"], bars["demb"])
        check(f"nce_dprotos_{tag}", owned(dpro, C) - dp0, ref["dprotos"], bars["dprotos"])
    sim2, probs2 = nan(B * C + 3), nan(B * C + 3)
    ops.nce(e, pr, None, sim2, probs2)                           # the inference form: sim and probs only
    assert torch.equal(owned(sim2, B * C), sim[:B * C]) and torch.equal(owned(probs2, B * C), probs[:B * C])


# ------------------------------------------------------------------------------------------------ row LayerNorm backward
@pytest.mark.parametrize("rows", [8192 + 8 + 3, 1])
def test_temporal_ln_bwd_past_the_grid_cap(ops, rows):
    """1026 row groups on 1024 workgroups: two take a second trip, one of them a ragged one"""
    assert R.ln_bwd_grid(rows) == min(1024, (rows + 7) // 8)
    x = rnd(rows, 384, seed=900, scale=2.0) + 0.3
    gamma, add = 1 + 0.1 * rnd(384, seed=901), rnd(rows, 384, seed=902)
    buf, tot = R.split_slabs(torch.randn(rows, 384, generator=torch.Generator().manual_seed(903)), 2, 64, 904)
    buf, tot = buf.to(DEV), tot.to(DEV)
    dy = tot + add.double()
    mean, rstd, dx_ref, dg_ref, db_ref = R.ln_bwd_fp64(x, gamma, dy, 1e-5)
    dx, dg, db = nan(rows + 2, 384), torch.zeros(384, device=DEV), torch.zeros(384, device=DEV)
    ops.temporal_ln_bwd(R.slab_view(buf, rows), add, x, mean.float(), rstd.float(), gamma, dx, dgamma=dg, dbeta=db)
    sc = max(1.0, float(dy.abs().max()))
    check(f"tln_bwd_dx_rows{rows}", owned(dx, rows), dx_ref, 2e-5 * sc)
    check(f"tln_bwd_dgamma_rows{rows}", dg, dg_ref, 2e-5 * sc * math.sqrt(rows))
    check(f"tln_bwd_dbeta_rows{rows}", db, db_ref, 2e-5 * sc * math.sqrt(rows))
    assert torch.isnan(buf[:, rows * 384:]).all()


@pytest.mark.parametrize("rows", [8192 + 8 + 3, 1])
def test_layernorm_bwd_past_the_grid_cap(ops, rows):
    assert R.ln_bwd_grid(rows) == min(1024, (rows + 7) // 8)
    x = rnd(rows, 384, seed=910, scale=2.0) + 0.3
    gamma = 1 + 0.1 * rnd(384, seed=911)
    dy16, dy32, dres = rnd(rows, 384, seed=912).to(torch.bfloat16), rnd(rows, 384, seed=913), rnd(rows, 384, seed=914)
    mean, rstd, dx_ref, dg_ref, db_ref = R.ln_bwd_fp64(x, gamma, dy16.double() + dy32.double(), 1e-6)
    dx_ref = dx_ref + dres.double()
    dx32, dx16 = nan(rows + 2, 384), nan(rows + 2, 384, dtype=torch.bfloat16)
    dg, db = torch.zeros(384, device=DEV), torch.zeros(384, device=DEV)
    ops.layernorm_bwd(x, 384, mean.float(), rstd.float(), gamma, rows, dy16=dy16, dy32=dy32, dres=dres, dx32=dx32, dx16=dx16,
                      dgamma=dg, dbeta=db)
    check(f"ln_bwd_dx32_rows{rows}", owned(dx32, rows), dx_ref, 1e-4 + 1e-4 * dx_ref.abs())
    check(f"ln_bwd_dx16_rows{rows}", owned(dx16, rows), dx_ref, 3e-2 + 1e-2 * dx_ref.abs())
    check(f"ln_bwd_dgamma_rows{rows}", dg, dg_ref, 2e-3 + 1e-4 * dg_ref.abs())
    check(f"ln_bwd_dbeta_rows{rows}", db, db_ref, 2e-3 + 1e-4 * db_ref.abs())


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections_launch_nothing(ops):
    """argument validation only: the return code, and nothing written"""
    from sais_amd import _lib as L
    E = L.SaisHipError
    S, B = 97, 1
    qkv, padu = torch.zeros(B * S, 1152, device=DEV), torch.zeros(B, S, dtype=torch.uint8, device=DEV)
    ctx, avg, dqkv, dctx = nan(B * S, 384), nan(B, S, S), nan(B * S, 1152), torch.zeros(2, B * S * 384 + 64, device=DEV)
    rng = ops.rng_state(1, DEV)
    with pytest.raises(E, match="code -1"):                      # S = 97
        ops.temporal_attn_fwd(qkv, padu, B, S, ctx, avg)
    with pytest.raises(E, match="code -1"):
        ops.temporal_attn_bwd(qkv, padu, B, S, dctx[0, :B * S * 384].view(B * S, 384), dqkv)
    with pytest.raises(E, match="code -1"):                      # a slab stride that is no multiple of 4
        ops.temporal_attn_bwd(qkv, padu, B, 33, torch.as_strided(dctx, (2, 33, 384), (33 * 384 + 2, 384, 1)), dqkv)
    with pytest.raises(E, match="code -1"):                      # p = 1
        ops.temporal_attn_fwd(qkv, padu, B, 33, ctx, avg, 1.0, rng, 0)
    with pytest.raises(E, match="code -1"):
        ops.temporal_attn_bwd(qkv, padu, B, 33, dctx[0, :33 * 384].view(33, 384), dqkv, 1.0, rng, 0)
    c = {k: v.to(DEV) for k, v in R.mil_case(1, 1, 1, False).items()}
    enc = torch.zeros(129, 384, device=DEV)
    reps, logits, att = nan(129, 384), nan(4), nan(4 * 129)
    w4 = torch.zeros(4, 384, device=DEV)
    with pytest.raises(E, match="code -1"):                      # 129 snippets
        ops.mil_head(enc, 1, 129, 1, c["WA"], c["bA"], c["WB"], c["bB"], w4[:, :256], w4[:, 0], w4, w4[:, 0], reps, logits, att)
    with pytest.raises(E, match="code -1"):                      # 4 classes
        ops.mil_head(enc, 1, 1, 4, c["WA"], c["bA"], c["WB"], c["bB"], w4[:, :256], w4[:, 0], w4, w4[:, 0], reps, logits, att)
    torch.cuda.synchronize()
    for t in (ctx, avg, dqkv, reps, logits, att):
        assert torch.isnan(t).all()
