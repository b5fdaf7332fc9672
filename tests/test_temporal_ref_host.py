"""CPU proof that the bars of tests/temporal_ref.py are sound (the fp32 restatement of each kernel's arithmetic is inside every
one, on every case the GPU file runs), that the recorded restatement values are what this machine computes, and that they are
sharp: each deliberate mutation of the restatement (temporal_ref.MUTATIONS) breaks a bar on a named case of the GPU list
while the unmutated restatement passes it.  No GPU, no kernel output anywhere."""
import math
import os
import re

import pytest
import torch

import temporal_ref as R
from oracle import sais_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def _fwd(name, S, p=0.0, site=0, mutate=None):
    pad = R.masks(S)
    qkv = R.layouts(name, pad, R.case_seed(name, S))
    keep = R.host_keep(pad.shape[0], S, p, R.BWD_SEED + S + site) if p > 0 else None
    return R.attn_ratios(R.emulate(qkv, pad, keep, p, mutate), R.attn_fp64(qkv, pad, keep, p))


def _inside(name, ratios):
    return all(ratios[w] <= R.fwd_bar(name, w) for w in ("avg", "ctx"))


# ------------------------------------------------------------------------------------------------ layouts and masks
@pytest.mark.parametrize("S", R.S_LIST)
def test_mask_patterns_keep_key_0_and_hit_the_tile_edge(S):
    pats = dict(R.mask_patterns(S))
    assert 1 <= len(pats) <= 5 and not any(bool(m[0]) for m in pats.values())
    assert not pats["none"].any()
    if S >= 2:
        assert int((~pats["only0"]).sum()) == 1
    assert ("last15" in pats) == (S >= 17) and ("last16" in pats) == (S >= 18) and ("holes" in pats) == (S >= 6)
    for nm, last in (("last15", 15), ("last16", 16)):
        if nm in pats:
            assert int(torch.nonzero(~pats[nm]).max()) == last and pats[nm][last + 1:].all() and not pats[nm][:last + 1].any()
    if "holes" in pats:
        m = pats["holes"]
        assert m[3] and m[S - 2] and not m[S - 1] and int(m.sum()) == 2


@pytest.mark.parametrize("S", R.S_LIST)
def test_layouts_are_what_they_claim(S):
    pad = R.masks(S)
    B = pad.shape[0]
    n = (~pad).sum(1)
    # same: every score exactly 0, every unmasked probability exactly 1 / n (fp64), float32(1 / n) in the restatement
    qkv = R.layouts("same", pad, R.case_seed("same", S))
    ref, emu = R.attn_fp64(qkv, pad), R.emulate(qkv, pad)
    for b in range(B):
        assert torch.equal(ref["P"][b][..., ~pad[b]], torch.full((R.TH, S, int(n[b])), 1.0 / int(n[b]), dtype=torch.float64))
        assert torch.equal(emu["P"][b][..., ~pad[b]], torch.full((R.TH, S, int(n[b])), 1.0).div(float(n[b])))
        assert float(ref["P"][b][..., pad[b]].abs().sum()) == 0.0
    # planted: row max >= 0.99 on the stated key; query 0's key is the last unmasked one; every unmasked key is some query's
    qkv = R.layouts("planted", pad, R.case_seed("planted", S))
    P = R.attn_fp64(qkv, pad)["P"]
    for b in range(B):
        key = R.planted_key(pad[b])
        assert int(key[0]) == int(torch.nonzero(~pad[b]).max())
        assert set(key.tolist()) == set(torch.nonzero(~pad[b]).flatten().tolist())
        got = P[b].gather(-1, key.view(1, S, 1).expand(R.TH, S, 1))
        assert float(got.min()) >= 0.99, (S, b, float(got.min()))
    # peaky: scaled scores reach far enough for the max subtraction to matter (|s| > 30 once S gives enough draws)
    if S >= 15:
        q, k, _ = R.heads(R.layouts("peaky", pad, R.case_seed("peaky", S)).double(), B, S)
        assert float(((q * R.SCALE) @ k.transpose(-2, -1)).abs().max()) > 30


def test_reference_is_the_oracles_attention_core():
    """oracle.temporal_layer returns mean_h(P'), the only part of its attention core visible from outside: attn_fp64 on the
    qkv of the same in_proj gives the same map, with masks and a keep mask"""
    S, p = 17, 0.1
    pad = R.masks(S)
    B = pad.shape[0]
    g = torch.Generator().manual_seed(5)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).double()
    pre = "l."
    sd = {pre + "self_attn.in_proj_weight": rn(1152, 384, sc=0.05), pre + "self_attn.in_proj_bias": rn(1152, sc=0.1),
          pre + "self_attn.out_proj.weight": rn(384, 384, sc=0.05), pre + "self_attn.out_proj.bias": rn(384, sc=0.1),
          pre + "linear1.weight": rn(64, 384, sc=0.05), pre + "linear1.bias": rn(64), pre + "linear2.weight": rn(384, 64, sc=0.05),
          pre + "linear2.bias": rn(384), pre + "norm1.weight": rn(384), pre + "norm1.bias": rn(384),
          pre + "norm2.weight": rn(384), pre + "norm2.bias": rn(384)}
    x = rn(B, S, 384)
    keep = R.host_keep(B, S, p, 11)
    drop = dict(attn=keep, d1=torch.ones(B, S, 384), ff=torch.ones(B, S, 64), d2=torch.ones(B, S, 384))
    _, avg = O.temporal_layer(sd, pre, x, pad, drop=drop, p=p)
    qkv = torch.nn.functional.linear(x, sd[pre + "self_attn.in_proj_weight"], sd[pre + "self_attn.in_proj_bias"])
    mine = R.attn_fp64(qkv.reshape(B * S, 1152), pad, keep, p)
    assert float((mine["avg"] - avg).abs().max()) <= 1e-15
    _, avg0 = O.temporal_layer(sd, pre, x, pad)
    assert float((R.attn_fp64(qkv.reshape(B * S, 1152), pad)["avg"] - avg0).abs().max()) <= 1e-15


# ------------------------------------------------------------------------------------------------ forward: sound, recorded, sharp
@pytest.mark.parametrize("name", R.LAYOUTS)
def test_forward_bounds_are_sound_and_recorded(name):
    """the restatement is inside every derived bound (ratio <= 1) AND inside the bar the GPU test applies, on every S and
    mask of the GPU list (and, rand, its dropout cases); its worst ratio per quantity is the recorded r_emu"""
    worst = dict(P=0.0, avg=0.0, ctx=0.0)
    cases = [(S, 0.0, 0) for S in R.S_LIST] + (list(R.DROP_CASES) if name == "rand" else [])
    for S, p, site in cases:
        r = _fwd(name, S, p, site)
        assert all(v <= 1.0 for v in r.values()), (name, S, p, r)
        assert _inside(name, r), (name, S, p, r)
        for k in worst:
            worst[k] = max(worst[k], r[k])
    print(name, worst)
    for k, rec in R.R_EMU[name].items():
        assert 0.5 * rec <= worst[k] <= 1.25 * rec, (name, k, worst[k], rec)
        assert 8 * rec < 1.0                                      # the bar is the restatement's, not the worst-case constant


SHARP = [("mask_off_by_one", "rand", 17, 0.0), ("mask_off_by_one", "planted", 33, 0.0), ("no_tail_mask", "rand", 17, 0.0),
         ("no_tail_mask", "same", 81, 0.0), ("dropout_transposed", "rand", 17, 0.1), ("dropout_head_stride", "rand", 17, 0.1),
         ("dropout_head_stride", "rand", 65, 0.5), ("keep_unscaled", "rand", 65, 0.1), ("avg_of_kept_heads", "rand", 17, 0.5)]


@pytest.mark.parametrize("mutate,name,S,p", SHARP)
def test_forward_mutations_break_a_bar(mutate, name, S, p):
    assert S in R.S_LIST and (p == 0 or (S, p, 0) in R.DROP_CASES)
    assert _inside(name, _fwd(name, S, p))
    bad = _fwd(name, S, p, mutate=mutate)
    print(mutate, name, S, p, bad)
    assert not _inside(name, bad)
    assert max(bad["avg"], bad["ctx"]) > 100 * max(R.fwd_bar(name, "avg"), R.fwd_bar(name, "ctx"))     # orders, not a hair


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("name", R.BWD_LAYOUTS)
def test_backward_recorded_values(name):
    cases = [(S, 0.0) for S in R.S_LIST] + ([(S, p) for S in (17, 65) for p in (0.1, 0.5)] if name == "rand" else [])
    for S, p in cases:
        emu = R.bwd_emu_case(name, S, p)
        rec, bars = R.BWD_EMU[(name, S, p)], R.bwd_bars(name, S, p)
        for e, r, b, rr in zip(emu, rec, bars, R.BWD_EMU[("rand", S, 0.0)]):
            assert abs(e - r) <= 0.05 * r + 1e-12, (name, S, p, emu, rec)
            assert b == max(8 * r, rr) and e <= b
        if S == 1:
            assert rec[:2] == [0.0, 0.0]                            # one key: P = 1, dS = 0, dq = dk = 0 exactly; dv = dctx


def test_backward_masked_keys_have_zero_gradient():
    qkv, pad, dctx = R.bwd_case("rand", 33)
    g = R.attn_bwd_fp64(qkv, pad, dctx).view(pad.shape[0], 33, 3, 384)
    assert float(g[:, :, 1:][pad].abs().max()) == 0.0 and float(g[:, :, 2][~pad].abs().amax(-1).min()) > 0.0


@pytest.mark.parametrize("n", [2, 3])
def test_drop_last_slab_breaks_the_backward_bar(n):
    name, S = "rand", 33
    qkv, pad, dctx = R.bwd_case(name, S)
    buf, total = R.split_slabs(dctx, n, 64, 3)
    slabs = R.slab_view(buf, dctx.shape[0])
    ref = R.attn_bwd_fp64(qkv, pad, total)
    ok = R.rel_l2_parts(R.emulate_bwd(qkv, pad, slabs), ref)
    bad = R.rel_l2_parts(R.emulate_bwd(qkv, pad, slabs, mutate="drop_last_slab"), ref)
    bars = R.bwd_bars(name, S)
    assert all(o <= b for o, b in zip(ok, bars)), (ok, bars)
    assert all(x > 1e4 * b for x, b in zip(bad, bars)), (bad, bars)


def test_split_slabs_leave_nan_in_the_gap():
    _, _, dctx = R.bwd_case("rand", 17)
    buf, total = R.split_slabs(dctx, 3, 64, 3)
    slabs = R.slab_view(buf, dctx.shape[0])
    assert slabs.stride(0) == dctx.numel() + 64 and slabs.stride(0) % 4 == 0 and slabs.data_ptr() == buf.data_ptr()
    assert torch.isnan(buf[:, dctx.numel():]).all() and not torch.isnan(slabs).any()
    assert float((total - dctx.double()).abs().max()) <= 8 * R.EPS * float(slabs.abs().max())


# ------------------------------------------------------------------------------------------------ launcher rules vs the sources
def test_launcher_rules_match_the_sources():
    hdr, tattn, temporal = _src("include", "sais_hip.h"), _src("sais_amd", "csrc", "tattn.hip"), _src("sais_amd", "csrc", "temporal.hip")
    for nm in ("SAIS_TEMPORAL_MAX_S_FWD", "SAIS_TEMPORAL_MAX_S_BWD"):
        top = int(re.search(rf"#define {nm} (\d+)", hdr).group(1))
        assert R.tattn_tiles(top) is not None and R.tattn_tiles(top + 1) is None and top == max(R.S_LIST)
    maxt = int(re.search(r"constexpr int MAXT = (\d+);", tattn).group(1))
    assert R.tattn_tiles(96) == maxt and R.tattn_tiles(1) == 1 and R.tattn_tiles(16) == 1 and R.tattn_tiles(17) == 2
    assert [R.tattn_tiles(S) for S in (64, 65, 81)] == [4, 5, 6]          # 65: a wave takes a second query tile; 81: odd tail
    assert "int lds = (B + C + 2 * B * C + B + 3) * 4;" in temporal
    assert "lds + stage <= 60 * 1024" in temporal and "(long)(B + C) * EMB * 4" in temporal
    assert re.search(r"EMB = (\d+)", temporal).group(1) == str(R.EMB)
    assert R.nce_staged(56, 2) and not R.nce_staged(57, 2) and not R.nce_staged(300, 3)
    assert all(R.nce_staged(B, C) for B, C in R.NCE_CASES if B <= 14)
    assert R.nce_lds_small(300, 3) <= 64 * 1024
    for f in ("tgemm.hip", "norm.hip"):
        s = _src("sais_amd", "csrc", f)
        assert "int grid = (rows + 7) / 8;\n    if (grid > 1024) grid = 1024;" in s, f
    assert R.ln_bwd_grid(1) == 1 and R.ln_bwd_grid(8192) == 1024 and R.ln_bwd_grid(8192 + 8 + 3) == 1024
    assert (8192 + 8 + 3 + 7) // 8 == 1026                                   # two workgroups take a second trip, one a ragged one


# ------------------------------------------------------------------------------------------------ the other references
def test_importance_loss_reference_without_a_low_skill_sample():
    """NaN loss and an exactly zero gradient: the mean over an empty selection scatters nothing back"""
    g = torch.Generator().manual_seed(1)
    B, T = 3, 5
    logits, target = torch.randn(B, T + 1, generator=g), torch.rand(B, T, generator=g)
    ipad = torch.zeros(B, T + 1, dtype=torch.bool)
    ipad[1, 3:] = True
    loss, grad = R.importance_loss_fp64(logits, target, ipad, torch.tensor([1, 1, 1]))
    assert math.isnan(float(loss)) and torch.equal(grad, torch.zeros(B, T + 1, dtype=torch.float64))
    loss, grad = R.importance_loss_fp64(logits, target, ipad, torch.tensor([1, 0, 1]), scale=0.25)
    assert math.isfinite(float(loss)) and float(grad[:, 1:].abs().min()) > 0 and float(grad[:, 0].abs().max()) == 0
    # the slot-t quirk: frame t is masked by slot t (slot 0 = CLS, never masked), so row 1 counts frames 0..2 of 5
    x, y = logits.double()[:, 1:], target.double()
    bce = torch.nn.functional.binary_cross_entropy_with_logits(x, y)
    assert abs(float(loss) - float(bce) * 3 / 5) <= 1e-15
    lb, db = R.importance_loss_bounds(logits, target, ipad, torch.tensor([1, 0, 1]), 0.25)
    l32, g32 = (t.float() for t in R.importance_loss_fp64(logits.float(), target.float(), ipad, torch.tensor([1, 0, 1]), 0.25))
    assert float(lb) > 0 and float(db[:, 1:].min()) > 0 and float(db[:, 0].max()) == 0
    assert abs(float(l32) - float(loss)) <= float(lb) and bool(((g32.double() - grad).abs() <= db).all())   # fp32 rounding of fp64 fits


def test_mil_recorded_values_and_saturation():
    worst = dict(logits=0.0, attention=0.0)
    for case in R.MIL_CASES:
        c = R.mil_case(*case)
        reps, l64, a64 = R.mil_head_ref(c)
        _, l32, a32 = R.mil_head_ref(c, torch.float32)
        assert torch.equal(reps, c["enc"].double().clamp(min=0))
        assert float((a64.sum(-1) - 1).abs().max()) <= 1e-12 and a64.shape == (case[2], case[0], case[1])
        worst["logits"] = max(worst["logits"], float((l32.double() - l64).abs().max()))
        worst["attention"] = max(worst["attention"], float((a32.double() - a64).abs().max()))
        if case[3]:                                                   # the saturated case: most gate units sit on the rails
            t = torch.tanh(torch.nn.functional.linear(reps, c["WA"].double(), c["bA"].double())).abs()
            assert float((t > 0.999).double().mean()) > 0.8
    for k in worst:
        assert 0.5 * R.MIL_EMU[k] <= worst[k] <= 1.25 * R.MIL_EMU[k], (k, worst[k], R.MIL_EMU[k])


def test_nce_recorded_values_and_bars():
    for B, C in R.NCE_CASES:
        emb, protos, lab = R.nce_case(B, C)
        r64, r32 = R.nce_ref(emb, protos, lab), R.nce_ref(emb, protos, lab, dt=torch.float32)
        bars = R.nce_bars(B, C)
        for k in R.NCE_SMALL:
            e = float((r32[k].double() - r64[k]).abs().max())
            assert e <= bars[k], (B, C, k, e)
            assert bars[k] >= R.NCE_SMALL[k]
            if B > 8:
                assert e <= 2 * R.NCE_EMU[(B, C)][k] + 1e-10, (B, C, k, e)
        q = R.nce_ref(emb, protos, lab, loss_scale=0.25)
        assert float((q["demb"] - 0.25 * r64["demb"]).abs().max()) <= 1e-15


def test_head_and_prepare_references():
    g = torch.Generator().manual_seed(2)
    B, ns, S = 5, 3, 4
    zr, zf = torch.randn(B, ns, S, 384, generator=g), torch.randn(B, ns, S, 384, generator=g)
    zr[0, :, 0, 7] = -1.0                                             # rep exactly 0: the second gate is strict
    zr[1, 0, 0, 9] = 0.0                                              # z exactly 0: the first gate is strict
    W, b = torch.randn(256, 384, generator=g), torch.randn(256, generator=g)
    WB, bB = torch.randn(256, 384, generator=g), torch.randn(256, generator=g)
    use = torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8)
    L, rep, emb = R.head_fp64(zr, None, W, b, use, WB, bB)
    assert float(rep.detach()[0, 7]) == 0.0
    emb.backward(torch.ones_like(emb))
    assert float(L["zr"].grad[0, :, 0, 7].abs().max()) == 0.0 and float(L["zr"].grad[1, 0, 0, 9]) == 0.0
    assert float(L["zr"].grad[:, :, 1:].abs().max()) == 0.0
    assert float(L["W"].grad[:, :].abs().sum()) > 0 and float(L["WB"].grad.abs().sum()) > 0
    both = R.head_fp64(zr, zf, W, b)[2]
    ref = torch.nn.functional.linear(torch.relu(torch.relu(zr.double())[:, :, 0].mean(1) + torch.relu(zf.double())[:, :, 0].mean(1)),
                                     W.double(), b.double())
    assert torch.equal(both, ref)
    x, pos, cls = torch.randn(3, 9, 384, generator=g), torch.randn(9, 384, generator=g), torch.randn(384, generator=g)
    z = R.prepare_fp64(x, pos, cls)
    assert torch.equal(z[:, 0], cls.double().expand(3, 384)) and torch.equal(z[:, 1:], x.double() + pos.double())
