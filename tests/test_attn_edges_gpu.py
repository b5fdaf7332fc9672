"""The attention kernels at their tile edges, on hard score layouts and in every launch form, on a real MI355X.

References are fp64 on the device from the bf16-rounded inputs (attn_ref.attn_fp64, one (frame, head) at a time); the bars are
the derived bounds of tests/attn_ref.py, which test_attn_ref_host.py proves sound and sharp:
  * out    |out - ref| <= 2^-8 (|ref| + A) + 2^-14 A,  A = softmax(s) @ |v|
  * lse    |lse - ref| <= 1e-4 + 2^-20 max_j |s_qj|
  * probs  |p - ref| <= (2^-16 + 2^-18 smax) ref + 1e-30: the resident forward writes f32 probabilities before any bf16
           rounding, so the bound is the f32 one its code implies (derivation in attn_ref.py), not 2^-8 ref
  * backward: per-part rel-L2 against fp64 autograd <= attn_ref.bwd_bars = min(1.5e-2, 4 x the f32 / bf16 emulation's own
           rel-L2), floored at the rand layout's emulated value
Every output buffer is oversized and NaN-filled: what the kernel does not own must still be NaN, what it owns must not be.
The tests never ask which kernel form ran: they compute it from the launcher's published rule (attn_ref.stream_waves,
attn_ref.bwd_cap) to choose shapes, and assert on results only."""
import functools

import pytest
import torch

import attn_ref as R
import parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

EDGE_NTOK = [2, 17, 63, 64, 65, 128, 129, 193, 4097]
EDGE_CASES = [(2, n) for n in EDGE_NTOK] + [(1, 4097)]           # (1, 4097): 390 workgroups of 32 queries
# the smallest shapes that select the 64-query, 4-wave form: one partial tile in which all but one lane of a workgroup are tail
# queries; two query tiles, the second with three all-tail waves; the resident size; 42 tiles plus one key; the maximum
FOUR_WAVE = [(86, 2), (43, 65), (22, 197), (2, 2689), (2, 4097)]
FORM_LAYOUTS = ("rand", "planted", "up")


@pytest.fixture(scope="module")
def ops():
    from sais_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def _case(name, frames, ntok, probs=False):
    """(qkv on the device, its fp64 reference): computed once, shared by every test that names the case, never written to"""
    qkv = R.layouts(name, frames, ntok, 1000 * ntok + frames).to(DEV)
    return qkv, R.attn_fp64(qkv, frames, ntok, probs=probs)


def _stream(ops, qkv, frames, ntok):
    M = frames * ntok
    out = torch.full((M + 70, 384), NAN, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((frames, 6, ntok), NAN, device=DEV)
    ops.vit_attn_fwd_any(qkv, frames, ntok, out, lse)
    assert torch.isnan(out[M:]).all()
    return out[:M], lse


def _check_fwd(out, lse, ref, tag, name):
    r_out = R.worst_ratio(out, ref["out"], R.out_bound(ref["out"], ref["A"]))
    r_lse = R.worst_ratio(lse, ref["lse"], R.lse_bound(ref["smax"]))
    print(f"{tag} {name}: out {r_out:.3f}, lse {r_lse:.3f} of the bound")
    parity.parity_log(f"attn_edge_{tag}_out_{name}", r_out, 1.0)
    parity.parity_log(f"attn_edge_{tag}_lse_{name}", r_lse, 1.0)
    assert r_out <= 1.0 and r_lse <= 1.0, (tag, name, r_out, r_lse)


# ------------------------------------------------------------------------------------------------ streaming kernel
@pytest.mark.parametrize("name", R.LAYOUTS)
@pytest.mark.parametrize("frames,ntok", EDGE_CASES)
def test_stream_edges(ops, frames, ntok, name):
    """the minimum, one partial tile, one key short of a tile, exact tiles, one real key in the last tile, the maximum (two
    frames of 4097 tokens take the 64-query form, one frame the 32-query form; every smaller case the 32-query form)"""
    assert R.stream_waves(frames, ntok) == (4 if (frames, ntok) == (2, 4097) else 2)
    qkv, ref = _case(name, frames, ntok)
    out, lse = _stream(ops, qkv, frames, ntok)
    _check_fwd(out, lse, ref, "stream", name)
    again, again_lse = _stream(ops, qkv, frames, ntok)
    assert torch.equal(again, out) and torch.equal(again_lse, lse)


@pytest.mark.parametrize("name", FORM_LAYOUTS)
@pytest.mark.parametrize("frames,ntok", FOUR_WAVE + [(85, 2)])
def test_stream_four_wave_form(ops, frames, ntok, name):
    """The 64-query form against fp64 and, bit for bit, against the 32-query form: the same frames one at a time.  (85, 2) is
    the last shape on the other side of the threshold; it goes through the same checks."""
    assert R.stream_waves(frames, ntok) == (2 if frames == 85 else 4) and R.stream_waves(1, ntok) == 2
    qkv, ref = _case(name, frames, ntok)
    out, lse = _stream(ops, qkv, frames, ntok)
    _check_fwd(out, lse, ref, "stream", name)
    again, again_lse = _stream(ops, qkv, frames, ntok)
    assert torch.equal(again, out) and torch.equal(again_lse, lse)
    for f in range(frames):
        one, one_lse = _stream(ops, qkv[f * ntok:(f + 1) * ntok], 1, ntok)
        assert torch.equal(one, out[f * ntok:(f + 1) * ntok]), (f, "out depends on the workgroup size")
        assert torch.equal(one_lse[0], lse[f]), (f, "lse depends on the workgroup size")


def test_stream_strided_operands(ops):
    """qkv as the first 1152 columns of a [M, 1160] buffer, out as the first 384 of a [M, 388] one"""
    frames, ntok = 3, 65
    M = frames * ntok
    qkv, ref = _case("planted", frames, ntok)
    wide = torch.full((M, 1160), NAN, dtype=torch.bfloat16, device=DEV)
    wide[:, :1152] = qkv
    obuf = torch.full((M + 70, 388), NAN, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((frames, 6, ntok), NAN, device=DEV)
    ops.vit_attn_fwd_any(wide[:, :1152], frames, ntok, obuf[:, :384], lse)
    assert torch.isnan(obuf[:, 384:]).all() and torch.isnan(obuf[M:]).all()
    _check_fwd(obuf[:M, :384], lse, ref, "stream", "planted")
    out, lse_c = _stream(ops, qkv, frames, ntok)
    assert torch.equal(obuf[:M, :384], out) and torch.equal(lse, lse_c)


# ------------------------------------------------------------------------------------------------ resident kernels, forward
@pytest.mark.parametrize("name", R.LAYOUTS)
@pytest.mark.parametrize("ntok", [197, 37])
def test_resident_forward(ops, ntok, name):
    """sais_vit_attn_fwd (out, lse, probs), sais_vit_attn_cls_fwd (row 0 of the same reference) and the streaming kernel on the
    same input, all against fp64"""
    frames = 3
    M = frames * ntok
    qkv, ref = _case(name, frames, ntok, True)
    out = torch.full((M + 70, 384), NAN, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((frames, 6, ntok), NAN, device=DEV)
    probs = torch.full((frames + 1, 6, ntok, ntok), NAN, device=DEV)
    ops.vit_attn_fwd(qkv, frames, out, lse, probs, ntok=ntok)
    assert torch.isnan(out[M:]).all() and torch.isnan(probs[frames:]).all()
    _check_fwd(out[:M], lse, ref, "resident", name)
    r_p = R.worst_ratio(probs[:frames], ref["probs"], R.probs_bound(ref["probs"], ref["smax"]))
    print(f"resident {name}: probs {r_p:.3f} of the bound")
    parity.parity_log(f"attn_edge_resident_probs_{name}", r_p, 1.0)
    assert r_p <= 1.0
    out_c = torch.full((frames + 2, 384), NAN, dtype=torch.bfloat16, device=DEV)
    ops.vit_attn_cls_fwd(qkv, frames, out_c, ntok)
    assert torch.isnan(out_c[frames:]).all()
    ref_c, A_c = ref["out"].view(frames, ntok, 384)[:, 0], ref["A"].view(frames, ntok, 384)[:, 0]
    r_c = R.worst_ratio(out_c[:frames], ref_c, R.out_bound(ref_c, A_c))
    print(f"cls {name}: out {r_c:.3f} of the bound")
    parity.parity_log(f"attn_edge_cls_out_{name}", r_c, 1.0)
    assert r_c <= 1.0
    s_out, s_lse = _stream(ops, qkv, frames, ntok)
    _check_fwd(s_out, s_lse, ref, "stream", name)


# ------------------------------------------------------------------------------------------------ resident kernels, backward
# One past the persistent cap of the backward (attn_ref.bwd_cap): Geo<197> has cap 256 and test_kernels_gpu.py's
# test_vit_attention_fwd_bwd[64] already runs 384 problems; Geo<37> has cap 768 and test_dino_gpu.py's
# test_attention_37_tokens[129] runs 774.  The cases here are small: three frames, hard layouts.
@functools.lru_cache(maxsize=None)
def _bwd_case(name, ntok):
    qkv, dout = R.bwd_case(name, ntok)
    return qkv.to(DEV), dout.to(DEV)


@pytest.mark.parametrize("name", R.BWD_LAYOUTS)
@pytest.mark.parametrize("ntok", [197, 37])
def test_resident_backward_hard_layouts(ops, ntok, name):
    frames = R.BWD_FRAMES
    M = frames * ntok
    qkv, dout = _bwd_case(name, ntok)
    out = torch.empty(M, 384, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(frames, 6, ntok, device=DEV)
    ops.vit_attn_fwd(qkv, frames, out, lse, None, ntok=ntok)
    dqkv = torch.full((M + 8, 1152), NAN, dtype=torch.bfloat16, device=DEV)
    ops.vit_attn_bwd(qkv, dout, out, lse, None, frames, dqkv, ntok=ntok)
    assert torch.isnan(dqkv[M:]).all() and torch.isfinite(dqkv[:M].float()).all()
    ref = R.attn_bwd_fp64(qkv, dout, frames, ntok)
    got, bars = R.rel_l2_parts(dqkv[:M], ref), R.bwd_bars(name, ntok)
    print(f"{name} {ntok}: " + ", ".join(f"{p} {g:.3e} (bar {b:.3e}, emulated {e:.3e})"
                                         for p, g, b, e in zip(("dq", "dk", "dv"), got, bars, R.BWD_EMU[(name, ntok)])))
    for part, g, b in zip(("dq", "dk", "dv"), got, bars):
        parity.parity_log(f"attn_edge_bwd{ntok}_{part}_{name}", g, b)
    for part, g, b in zip(("dq", "dk", "dv"), got, bars):
        assert g <= b, (name, ntok, part, g, b)
    again = torch.full_like(dqkv, NAN)
    ops.vit_attn_bwd(qkv, dout, out, lse, None, frames, again, ntok=ntok)
    assert torch.equal(again[:M], dqkv[:M])


@pytest.mark.parametrize("name", ["offp", "up"])
@pytest.mark.parametrize("ntok", [197, 37])
def test_cls_backward_hard_layouts(ops, ntok, name):
    """sais_vit_attn_cls_bwd against fp64 autograd of the full attention with zero gradient off the CLS rows"""
    frames = R.BWD_FRAMES
    M = frames * ntok
    qkv, dout = _bwd_case(name, ntok)
    dout_c = dout.view(frames, ntok, 384)[:, 0].contiguous()
    dqkv = torch.full((M + 8, 1152), NAN, dtype=torch.bfloat16, device=DEV)
    ops.vit_attn_cls_bwd(qkv, dout_c, frames, dqkv, ntok)
    assert torch.isnan(dqkv[M:]).all() and torch.isfinite(dqkv[:M].float()).all()
    ref = R.attn_bwd_fp64(qkv, dout_c, frames, ntok, cls_only=True)
    got = R.rel_l2_parts(dqkv[:M], ref)
    print(f"cls {name} {ntok}: dq {got[0]:.3e}, dk {got[1]:.3e}, dv {got[2]:.3e} (bar 6e-3)")
    for part, g in zip(("dq", "dk", "dv"), got):
        parity.parity_log(f"attn_edge_clsbwd{ntok}_{part}_{name}", g, 6e-3)
        assert g <= 6e-3, (name, ntok, part, g)
    dq = dqkv[:M, :384].float().view(frames, ntok, 384)
    assert float(dq[:, 1:].abs().max()) == 0.0 and float(dq[:, 0].abs().max()) > 0
