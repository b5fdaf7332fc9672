"""The bars of tests/attn_ref.py are sound and sharp (CPU only): an f32 / bf16 restatement of the streaming algorithm stays inside
both bounds on every layout at every tile edge, and each deliberate error put into it breaks a bound on a case that
test_attn_edges_gpu.py runs.  Also: the layouts are what they claim, the launcher rules give the shapes the GPU tests rely
on, and the recorded emulation values behind the backward bars are reproduced."""
import math

import pytest
import torch

import attn_ref as R

SOUND_NTOK = [2, 63, 64, 65, 129, 197, 1561, 4097]
GPU_EDGE_NTOK = [2, 17, 63, 64, 65, 128, 129, 193, 4097]           # the streaming cases of test_attn_edges_gpu.py
# mutation -> the (layout, ntok) of the GPU list that catches it, and by which quantity
CAUGHT_BY = {
    "no_mask": ("planted", 65, "lse"),
    "no_rescale": ("up", 129, "out"),
    "drop_last_key": ("planted", 65, "lse"),
    "stale_max": ("down", 129, "lse"),
}


def _ratios(name, ntok, nheads, mutate=None, seed=None):
    qkv = R.layouts(name, 1, ntok, 100 + ntok if seed is None else seed)
    ref = R.attn_fp64(qkv, 1, ntok)
    q, k, v = R.heads(qkv, 1, ntok)
    w_out = w_lse = 0.0
    for h in range(nheads):
        o, l = R.emulate_stream(q[0, h], k[0, h], v[0, h], mutate=mutate)
        sl = slice(R.HD * h, R.HD * (h + 1))
        w_out = max(w_out, R.worst_ratio(o, ref["out"][:, sl], R.out_bound(ref["out"][:, sl], ref["A"][:, sl])))
        w_lse = max(w_lse, R.worst_ratio(l, ref["lse"][0, h], R.lse_bound(ref["smax"][0, h])))
    return w_out, w_lse


@pytest.mark.parametrize("ntok", SOUND_NTOK)
def test_bounds_are_sound(ntok):
    """every layout: the emulation is inside the out and the lse bound (one head at 4097 tokens, six below)"""
    for name in R.LAYOUTS:
        w_out, w_lse = _ratios(name, ntok, 1 if ntok == 4097 else R.NH)
        print(f"{name} {ntok}: out {w_out:.3f}, lse {w_lse:.3f} of the bound")
        assert w_out <= 1.0 and w_lse <= 1.0, (name, ntok, w_out, w_lse)


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_bounds_are_sharp(mutate):
    """Each mutation of emulate_stream violates a bound on a case of the GPU list:
      no_mask        planted, 65 tokens: query 0's planted key is the last key and the only real one of the second tile; its 63
                     unmasked copies move lse by ~log 64 (also caught by out, whose V rows past the end are zero)
      no_rescale     up, 129 tokens: the maximum rises in all three tiles and the mass sits in the one-key tail
      drop_last_key  planted, 65 tokens: query 0 loses the key that holds its whole mass
      stale_max      down, 129 tokens: every tile after the first has a lower maximum and is over-weighted
    and none of them is caught by luck: the unmutated emulation passes the same case (test_bounds_are_sound)."""
    name, ntok, which = CAUGHT_BY[mutate]
    assert name in R.LAYOUTS and ntok in GPU_EDGE_NTOK
    w_out, w_lse = _ratios(name, ntok, 1, mutate)
    print(f"{mutate} on {name} {ntok}: out {w_out:.3g}, lse {w_lse:.3g} of the bound")
    assert (w_lse if which == "lse" else w_out) > 1.0
    ok_out, ok_lse = _ratios(name, ntok, 1)
    assert ok_out <= 1.0 and ok_lse <= 1.0


def test_every_mutation_is_caught_at_every_ragged_count():
    """wider than the named pairs: at each token count of the GPU list with a ragged last tile, planted catches all four (the
    first tile cannot catch no_rescale / stale_max, a full tile cannot catch no_mask)"""
    for ntok in (65, 129, 193):
        for mutate in R.MUTATIONS:
            assert max(_ratios("planted", ntok, 1, mutate)) > 1.0, (mutate, ntok)
    for ntok in (2, 17, 63):
        for mutate in ("no_mask", "drop_last_key"):
            assert max(_ratios("planted", ntok, 1, mutate)) > 1.0, (mutate, ntok)
    assert max(_ratios("planted", 64, 1, "drop_last_key")) > 1.0 and max(_ratios("planted", 128, 1, "drop_last_key")) > 1.0


def test_layouts_are_what_they_claim():
    for ntok in sorted(set(SOUND_NTOK + GPU_EDGE_NTOK + [37, 2689])):
        pi = R.planted_perm(ntok)
        assert sorted(pi.tolist()) == list(range(ntok)) and int(pi[0]) == ntok - 1
    assert [R._coprime_mult(n) for n in (2, 3, 15, 105, 4097)] == [3, 5, 7, 11, 3]
    ntok = 129
    # planted: near one-hot rows on the planted key, in every head
    qkv = R.layouts("planted", 2, ntok, 5)
    assert qkv.dtype == torch.bfloat16 and qkv.shape == (2 * ntok, 1152)
    ref = R.attn_fp64(qkv, 2, ntok, probs=True)
    assert torch.equal(ref["probs"].argmax(-1), R.planted_perm(ntok).expand(2, R.NH, ntok))
    assert float(ref["probs"].amax(-1).min()) > 0.99
    q, k, _ = R.heads(qkv, 2, ntok)
    assert not torch.equal(q[0, 0], q[0, 1]) and not torch.equal(q[0, 0], q[1, 0])          # own draws per frame and head
    # up / down: the per-tile maximum of every query rises / falls from full tile to full tile
    for name, sign in (("up", 1), ("down", -1)):
        q, k, _ = R.heads(R.layouts(name, 1, 256, 6), 1, 256)
        s = (q[0, 0].double() @ k[0, 0].double().t()) * R.SCALE
        tmax = torch.stack([s[:, t:t + 64].amax(-1) for t in range(0, 256, 64)], -1)
        assert bool((sign * (tmax[:, 1:] - tmax[:, :-1]) > 0).all())
    # offp / offn: every score within a few sigma of +-288
    for name, off in (("offp", 288.0), ("offn", -288.0)):
        ref = R.attn_fp64(R.layouts(name, 1, ntok, 7), 1, ntok)
        assert float((ref["lse"] - off).abs().max()) < 25 and float(ref["smax"].min()) > 250
    # same: p = 1 / ntok, out = mean(v), lse = s + log ntok — which also checks attn_fp64 against a closed form
    qkv = R.layouts("same", 1, ntok, 8)
    ref = R.attn_fp64(qkv, 1, ntok, probs=True)
    q, k, v = R.heads(qkv, 1, ntok)
    assert float((ref["probs"] - 1.0 / ntok).abs().max()) < 1e-15
    mean_v = v.double().mean(2)[0].reshape(1, 384).expand(ntok, 384)
    assert float((ref["out"] - mean_v).abs().max()) < 1e-13
    s0 = (q.double() * k[:, :, :1].double()).sum(-1) * R.SCALE
    assert float((ref["lse"] - s0 - math.log(ntok)).abs().max()) < 1e-11


def test_launcher_rules():
    """the shapes the GPU tests name are on the side of each threshold they are meant for"""
    four = [(86, 2), (43, 65), (22, 197), (2, 2689), (2, 4097)]
    assert all(R.stream_waves(f, n) == 4 for f, n in four)
    assert all(R.stream_waves(1, n) == 2 for _, n in four)
    assert R.stream_waves(85, 2) == 2 and R.stream_waves(1, 4097) == 2 and R.stream_waves(42, 65) == 2
    assert R.stream_waves(21, 197) == 2 and R.stream_waves(2, 2688) == 2
    assert all(R.stream_waves(2, n) == 2 for n in GPU_EDGE_NTOK[:-1])
    assert R.bwd_cap(37) == 768 and R.bwd_cap(197) == 256
    assert 128 * R.NH <= R.bwd_cap(37) < 129 * R.NH and 64 * R.NH > R.bwd_cap(197)


@pytest.mark.parametrize("ntok", [197, 37])
def test_backward_emulation_values_and_bars(ntok):
    """emulate_bwd against fp64 autograd reproduces the recorded per-part values (to 2 %: thread count and BLAS), every one of
    them is inside the backward's 1.5e-2 on its own, and the bars follow the stated rule"""
    for name in R.BWD_LAYOUTS:
        qkv, dout = R.bwd_case(name, ntok)
        emu = R.rel_l2_parts(R.emulate_bwd(qkv, dout, R.BWD_FRAMES, ntok), R.attn_bwd_fp64(qkv, dout, R.BWD_FRAMES, ntok))
        rec, bars = R.BWD_EMU[(name, ntok)], R.bwd_bars(name, ntok)
        print(f"{name} {ntok}: emulated " + ", ".join(f"{e:.3e}" for e in emu) + " bars " + ", ".join(f"{b:.3e}" for b in bars))
        for e, r, b, rr in zip(emu, rec, bars, R.BWD_EMU[("rand", ntok)]):
            assert abs(e - r) <= 0.02 * r
            assert r <= 1.5e-2 and r <= b <= 1.5e-2
            assert b == max(min(1.5e-2, 4 * r), rr)
