"""sais_vit_attn_bwd_any (csrc/attn_any_bwd.hip) on the device: every case of attn_any_bwd_ref.CASES against fp64 autograd under
the derived bars, both launcher forms, agreement with the resident backward at its two token counts, run-to-run and
batch-position bit equality, strided buffers with NaN in every byte the kernel must not read.  Shapes are chosen with the
launcher's published rule (attn_any_bwd_ref.stream_bwd_waves); assertions are on results only."""
import functools

import pytest
import torch

import attn_any_bwd_ref as B
import attn_ref as R
import parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
PARTS = ("dq", "dk", "dv")


@pytest.fixture(scope="module")
def ops():
    from sais_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def _case(name, ntok, frames):
    """(qkv, dout on the device, fp64 reference): computed once, shared, never written to"""
    qkv, dout = B.case(name, ntok, frames)
    qkv, dout = qkv.to(DEV), dout.to(DEV)
    return qkv, dout, R.attn_bwd_fp64(qkv, dout, frames, ntok)


def _fwd(ops, qkv, frames, ntok):
    out = torch.empty(frames * ntok, R.DM, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(frames, R.NH, ntok, device=DEV)
    ops.vit_attn_fwd_any(qkv, frames, ntok, out, lse)
    return out, lse


def _bwd(ops, qkv, dout, out, lse, frames, ntok):
    dqkv = torch.full((frames * ntok, 3 * R.DM), NAN, dtype=torch.bfloat16, device=DEV)
    ops.vit_attn_bwd_any(qkv, dout, out, lse, frames, ntok, dqkv)
    return dqkv


def _run(ops, qkv, dout, frames, ntok):
    out, lse = _fwd(ops, qkv, frames, ntok)
    return _bwd(ops, qkv, dout, out, lse, frames, ntok)


def _check(dqkv, ref, bars, tag):
    got = R.rel_l2_parts(dqkv, ref)
    print(tag, " ".join(f"{p} {g:.3e} / {b:.3e}" for p, g, b in zip(PARTS, got, bars)))
    for p, g, b in zip(PARTS, got, bars):
        parity.parity_log(f"attn_any_bwd_{tag}_{p}", g / b, 1.0)
    assert torch.isfinite(dqkv.float()).all(), tag
    for p, g, b in zip(PARTS, got, bars):
        assert g <= b, (tag, p, g, b)


@pytest.mark.parametrize("name,ntok,frames", B.CASES, ids=[f"{n}-{t}x{f}" for n, t, f in B.CASES])
def test_cases_vs_fp64(ops, name, ntok, frames):
    qkv, dout, ref = _case(name, ntok, frames)
    _check(_run(ops, qkv, dout, frames, ntok), ref, B.bars(name, ntok), f"{name}_{ntok}")


# 129 tokens = 3 tiles per (frame, head): 3 frames are 54 workgroups of 64 rows (the 2-wave form), 30 frames 540 (the 4-wave form)
@pytest.mark.parametrize("frames,waves", [(3, 2), (30, 4)])
def test_both_launcher_forms(ops, frames, waves):
    assert B.stream_bwd_waves(frames, 129) == waves
    qkv, dout, ref = _case("rand", 129, frames)
    _check(_run(ops, qkv, dout, frames, 129), ref, B.bars("rand", 129), f"form{waves}_129")


@pytest.mark.parametrize("ntok", [197, 37])
@pytest.mark.parametrize("name", R.BWD_LAYOUTS)
def test_agrees_with_resident_backward(ops, name, ntok):
    """same qkv, dout, out and lse (the resident forward's): the two kernels restate one arithmetic, each within attn_ref.bwd_bars of
    fp64, so they differ by at most the sum of both bars"""
    frames = R.BWD_FRAMES
    qkv, dout = (t.to(DEV) for t in R.bwd_case(name, ntok))
    out = torch.empty(frames * ntok, R.DM, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(frames, R.NH, ntok, device=DEV)
    ops.vit_attn_fwd(qkv, frames, out, lse, None, ntok=ntok)
    res = torch.full((frames * ntok, 3 * R.DM), NAN, dtype=torch.bfloat16, device=DEV)
    ops.vit_attn_bwd(qkv, dout, out, lse, None, frames, res, ntok=ntok)
    got = _bwd(ops, qkv, dout, out, lse, frames, ntok)
    diff, bars = R.rel_l2_parts(got, res), R.bwd_bars(name, ntok)
    print(name, ntok, diff, bars)
    for p, d, b in zip(PARTS, diff, bars):
        parity.parity_log(f"attn_any_bwd_vs_resident{ntok}_{name}_{p}", d / (2 * b), 1.0)
        assert d <= 2 * b, (name, ntok, p, d, b)


@pytest.mark.parametrize("ntok,frames", [(129, 3), (129, 30), (785, 1)])
def test_two_runs_are_bit_equal(ops, ntok, frames):
    qkv, dout, _ = _case("rand", ntok, frames)
    out, lse = _fwd(ops, qkv, frames, ntok)
    assert torch.equal(_bwd(ops, qkv, dout, out, lse, frames, ntok), _bwd(ops, qkv, dout, out, lse, frames, ntok))


@pytest.mark.parametrize("frames,sub", [(3, slice(1, 2)), (30, slice(1, 30))])
def test_frame_rows_do_not_depend_on_the_batch(ops, frames, sub):
    """a frame launched alone (2-wave form, as its batch of 3) / 29 frames of a batch of 30 (both the 4-wave form)"""
    ntok = 129
    n = sub.stop - sub.start
    assert B.stream_bwd_waves(frames, ntok) == B.stream_bwd_waves(n, ntok)
    qkv, dout, _ = _case("rand", ntok, frames)
    rows = slice(sub.start * ntok, sub.stop * ntok)
    whole = _run(ops, qkv, dout, frames, ntok)
    part = _run(ops, qkv[rows].contiguous(), dout[rows].contiguous(), n, ntok)
    assert torch.equal(whole[rows], part)


@pytest.mark.parametrize("ntok", [65, 145])
def test_strided_buffers_and_guard_rows(ops, ntok):
    """row strides 1160 / 392, NaN in the pad columns and in guard rows past frames * ntok of every input; the sentinel of dqkv's pad
    columns and guard rows survives"""
    frames, G, SENT = 3, 70, 777.0
    M = frames * ntok
    qkv, dout, _ = _case("rand", ntok, frames)
    out, lse = _fwd(ops, qkv, frames, ntok)
    plain = _bwd(ops, qkv, dout, out, lse, frames, ntok)

    def padded(t, ld):
        buf = torch.full((M + G, ld), NAN, dtype=torch.bfloat16, device=DEV)
        buf[:M, :t.shape[1]] = t
        return buf[:M, :t.shape[1]]
    dbuf = torch.full((M + G, 1160), SENT, dtype=torch.bfloat16, device=DEV)
    ops.vit_attn_bwd_any(padded(qkv, 1160), padded(dout, 392), padded(out, 392), lse, frames, ntok, dbuf[:M, :1152])
    assert torch.equal(dbuf[:M, :1152], plain)
    assert (dbuf[M:] == SENT).all() and (dbuf[:M, 1152:] == SENT).all()
