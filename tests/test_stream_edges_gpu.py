"""The streaming kernels of the ViT step and the DINO objective (csrc/norm.hip, misc.hip, dino.hip) at their edges, on a real
MI355X: ragged and tiny sizes, a second grid-stride round, every optional operand, free row strides, hard rows.

Every comparison is against the fp64 references of tests/stream_ref.py under the bars stated there (the bars of
test_kernels_gpu.py / test_dino_gpu.py, unchanged, plus the principled terms for hard rows and growing results); observed / bar
goes to parity_log("stream_edge_<kernel>_<quantity>").  Outputs land in NaN-filled buffers (0xA5 for bytes), outputs through a
stride are checked with gemm_ref.untouched, inputs through a stride carry 1e30 in the gap, bit-exact cases are launched twice.
Shapes are the smallest that reach a path (test_stream_ref_host.py::test_grid_caps_are_crossed_and_chunks_are_ragged)."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn

import gemm_ref as G
import parity
import stream_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = G.NAN
BF16, F32 = torch.bfloat16, torch.float32
D = S.D
P_DROP = 0.1


@pytest.fixture(scope="module")
def ops():
    from sais_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from sais_amd import _lib
    return _lib


def nan(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def rnd(*shape, seed=0, scale=1.0, dtype=F32):
    return (torch.randn(*shape, generator=S.gen(seed)) * scale).to(dtype).to(DEV)


def bar(name, r):
    print(f"{name}: {r:.3f} of the bar")
    parity.parity_log(f"stream_edge_{name}", r, 1.0)
    assert r <= 1.0, (name, r)


def vec(n, dtype=F32, fill=None):
    """an n-element vector 4 elements into a NaN buffer of n + 8: (view, buffer)"""
    buf = nan(n + 8, dtype=dtype)
    view = buf[4:4 + n]
    if fill is not None:
        view.copy_(fill)
    return view, buf


def out2d(rows, cols, pad, off, dtype=F32):
    """a NaN [rows, cols] output with row stride cols + pad inside a NaN buffer, or contiguous with one spare row (pad = 0)"""
    if pad:
        return G.padded(nan(rows, cols, dtype=dtype), pad, off)
    buf = nan(rows + 1, cols, dtype=dtype)
    return buf[:rows], buf


def in2d(t, pad, off):
    return S.strided_in(t, pad, off) if pad else (t, t)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(G._bits(a.contiguous()), G._bits(b.contiguous()))


def inv_keep():
    one = torch.ones((), dtype=F32)
    return float(one / (one - torch.tensor(P_DROP, dtype=F32)))                 # fl(1 / (1 - p)) as the kernels form it


# ------------------------------------------------------------------------------------------------ ln_fwd
def _ln_fwd_case(ops, x, gamma, beta, eps, subset, strided, tag):
    rows = x.shape[0]
    px, p16, p32 = (8, 12, 16) if strided else (0, 0, 0)
    xv, _ = in2d(x, px, 4)
    y16, b16 = out2d(rows, D, p16, 8, BF16) if subset in ("all", "y16", "nostats") else (None, None)
    y32, b32 = out2d(rows, D, p32, 12) if subset in ("all", "y32", "nostats") else (None, None)
    (mean, bm), (rstd, br) = (vec(rows), vec(rows)) if subset in ("all", "y32") else ((None, None), (None, None))
    ops.layernorm_fwd(xv, rows, xv.stride(0), gamma, beta, eps, y16, y32, mean, rstd,
                      ldy16=D + p16 if y16 is not None else D, ldy32=D + p32 if y32 is not None else D)
    y, mu, rs = S.ln_fwd(x, gamma, beta, eps)
    atol, torch_err = S.ln_y_atol(x, gamma, beta, eps)
    if y32 is not None:
        G.untouched(b32, y32)
        r = S.ratio(y32, y, atol)
        print(f"{tag}: y32 at {S.ratio(y32, y, max(torch_err, 1e-30)):.2f} x torch's fp32 error")
        bar("ln_fwd_y32", r)
    if y16 is not None:
        G.untouched(b16, y16)
        bar("ln_fwd_y16", S.ratio(y16, y, S.BF16_ATOL, S.BF16_RTOL))
    if mean is not None:
        G.untouched(bm, mean), G.untouched(br, rstd)
        bar("ln_fwd_mean", float(((mean.double().cpu() - mu).abs() / S.ln_mean_bar(x, mu)).max()))
        bar("ln_fwd_rstd", S.ratio(rstd, rs, 0.0, S.RSTD_RTOL))


@pytest.mark.parametrize("eps", S.LN_EPS)
@pytest.mark.parametrize("rows", S.LN_FWD_ROWS)
def test_ln_fwd(ops, rows, eps):
    gamma, beta = (t.to(DEV) for t in S.ln_params())
    for k, kind in enumerate(S.LN_KINDS):
        x = S.ln_rows(kind, rows, seed=rows).to(DEV)
        _ln_fwd_case(ops, x, gamma, beta, eps, "all", strided=bool(k % 2), tag=f"{kind} rows={rows}")
    x = S.ln_rows("plain", rows, seed=rows).to(DEV)
    for subset, strided in itertools.product(("y16", "y32", "nostats", "all"), (False, True)):
        _ln_fwd_case(ops, x, gamma, beta, eps, subset, strided, tag=f"{subset} rows={rows}")
    _ln_fwd_case(ops, S.ln_rows("offset1000", rows, seed=rows).to(DEV), gamma, beta, eps, "all", True, tag="offset1000 strided")


@pytest.mark.parametrize("eps", S.LN_EPS)
def test_ln_fwd_constant_rows_give_beta_bit_for_bit(ops, eps):
    """rows of 0 and of 1: the sum of 384 equal small integers and its product with fl(1 / 384) are exact, so the centred row is 0"""
    gamma, beta = (t.to(DEV) for t in S.ln_params())
    for c, rows in itertools.product((0.0, 1.0), (1, 9)):
        x = torch.full((rows, D), c, device=DEV)
        for rep in range(2):
            y32, mean, rstd = nan(rows, D), nan(rows), nan(rows)
            ops.layernorm_fwd(x, rows, D, gamma, beta, eps, None, y32, mean, rstd)
            assert torch.equal(y32, beta.expand(rows, D)) and torch.equal(mean, torch.full((rows,), c, device=DEV))
            bar("ln_fwd_rstd", S.ratio(rstd, torch.full((rows,), S.f32(eps)).double().rsqrt(), 0.0, S.RSTD_RTOL))


# ------------------------------------------------------------------------------------------------ ln_bwd
def _ln_bwd_inputs(rows, seed):
    x = S.ln_rows("plain", rows, seed=seed)
    gamma, beta = S.ln_params()
    _, mean, rstd = S.ln_fwd(x, gamma, beta, 1e-6)
    return dict(x=x.to(DEV), gamma=gamma.to(DEV), mean=mean.float().to(DEV), rstd=rstd.float().to(DEV),
                dy16=rnd(rows, D, seed=seed + 1, dtype=BF16), dy32=rnd(rows, D, seed=seed + 2), dres=rnd(rows, D, seed=seed + 3))


def _ln_bwd_case(ops, t, ins, dres, outs, dgdb, strided=False, extras=False, seed=0):
    """one launch: ins in {"dy16", "dy32", "both"}, outs in {"dx32", "dx16", "both"}; extras: rowscale16 and dx32_drop"""
    rows = t["x"].shape[0]
    pads = (8, 12, 16, 20, 24, 28) if strided else (0,) * 6
    xv, _ = in2d(t["x"], pads[0], 4)
    d16, _ = in2d(t["dy16"], pads[1], 8) if ins != "dy32" else (None, None)
    d32, _ = in2d(t["dy32"], pads[2], 12) if ins != "dy16" else (None, None)
    dr, _ = in2d(t["dres"], pads[3], 4) if dres else (None, None)
    dx32, b32 = out2d(rows, D, pads[4], 8) if outs != "dx16" or extras else (None, None)
    dx16, b16 = out2d(rows, D, pads[5], 4, BF16) if outs != "dx32" else (None, None)
    drop, bdrop = out2d(rows, D, pads[4], 16 if strided else 0) if extras else (None, None)
    rs16 = None
    if extras and dx16 is not None:
        rs16 = (torch.randint(0, 2, (rows,), generator=S.gen(seed + 9)).float() * inv_keep()).to(DEV)
        if rows > 1:
            rs16[0], rs16[1] = 0.0, inv_keep()
    dg0, db0 = (rnd(D, seed=seed + 4), rnd(D, seed=seed + 5)) if dgdb else (None, None)
    dg, db = (dg0.clone(), db0.clone()) if dgdb else (None, None)
    rng = ops.rng_state(1234, DEV)
    ld = lambda v: D if v is None else v.stride(0)                                   # noqa: E731
    ops.layernorm_bwd(xv, xv.stride(0), t["mean"], t["rstd"], t["gamma"], rows, dy16=d16, dy32=d32, dres=dr, dx32=dx32, dx16=dx16,
                      dgamma=dg, dbeta=db, lddy16=ld(d16), lddy32=ld(d32), lddres=ld(dr), lddx32=ld(dx32), lddx16=ld(dx16),
                      rowscale16=rs16, dx32_drop=drop, drop=(P_DROP, rng, 3) if extras else None)
    dy = (t["dy16"].double() if ins != "dy32" else 0.0) + (t["dy32"].double() if ins != "dy16" else 0.0)
    ref, rg, rb, ag, ab = S.ln_bwd(dy, t["x"], t["mean"], t["rstd"], t["gamma"], t["dres"] if dres else None)
    if dx32 is not None:
        G.untouched(b32, dx32)
        bar("ln_bwd_dx32", S.ratio(dx32, ref, S.DX32_ATOL, S.DX32_RTOL))
    if dx16 is not None:
        G.untouched(b16, dx16)
        want = ref if rs16 is None else ref * rs16.double().cpu()[:, None]
        bar("ln_bwd_dx16", S.ratio(dx16, want, S.BF16_ATOL, S.BF16_RTOL))
        if rs16 is not None:
            assert bool((dx16[rs16 == 0] == 0).all())
    if drop is not None:
        G.untouched(bdrop, drop)
        keep = ops.dropout_mask(rows * D, P_DROP, rng, 3, DEV).view(rows, D).bool()
        assert bits_equal(drop, torch.where(keep, dx32 * inv_keep(), torch.zeros((), device=DEV)))
        assert 0 < int(keep.sum()) < keep.numel() or rows * D < 64
    if dgdb:
        bar("ln_bwd_dgamma", float(((dg.double().cpu() - (dg0.double().cpu() + rg)).abs()
                                    / S.sum_bar(ag + dg0.double().cpu().abs(), rows + 1)).max()))
        bar("ln_bwd_dbeta", float(((db.double().cpu() - (db0.double().cpu() + rb)).abs()
                                   / S.sum_bar(ab + db0.double().cpu().abs(), rows + 1)).max()))


@pytest.mark.parametrize("rows", S.LN_BWD_ROWS)
def test_ln_bwd_operand_sets(ops, rows):
    t = _ln_bwd_inputs(rows, seed=10 * rows)
    if rows <= 9:
        for ins, dres, outs, dgdb in itertools.product(("dy16", "dy32", "both"), (False, True), ("dx32", "dx16", "both"),
                                                      (False, True)):
            _ln_bwd_case(ops, t, ins, dres, outs, dgdb, seed=rows)
    else:
        _ln_bwd_case(ops, t, "dy16", False, "dx32", False, seed=rows)
        _ln_bwd_case(ops, t, "dy32", True, "dx16", True, seed=rows)
    _ln_bwd_case(ops, t, "both", True, "both", True, strided=True, seed=rows)
    _ln_bwd_case(ops, t, "both", False, "both", True, extras=True, seed=rows)
    _ln_bwd_case(ops, t, "dy16", True, "both", False, strided=True, extras=True, seed=rows)


@pytest.mark.parametrize("rows", S.LN_BWD_INT_ROWS)
def test_ln_bwd_integer_sums_exactly(ops, rows):
    dy16, dy32, x = S.ints((rows, D), 1), S.ints((rows, D), 2), S.ints((rows, D), 3)
    gamma, mean, rstd = S.gamma_int(4), torch.zeros(rows), torch.ones(rows)
    dg0, db0 = S.ints((D,), 5, 1, 4), S.ints((D,), 6, -4, -1)
    ref, rg, rb, ag, ab = S.ln_bwd(dy16 + dy32, x, mean, rstd, gamma)
    assert S.int_exact(ag + dg0.double().abs(), ab + db0.double().abs())
    dev = [t.to(DEV) for t in (x, mean, rstd, gamma, dy16.to(BF16), dy32)]
    for rep in range(2):
        dg, db, dx32 = dg0.to(DEV), db0.to(DEV), nan(rows, D)
        ops.layernorm_bwd(dev[0], D, dev[1], dev[2], dev[3], rows, dy16=dev[4], dy32=dev[5], dx32=dx32, dgamma=dg, dbeta=db)
        assert torch.equal(dg.double().cpu(), dg0.double() + rg) and torch.equal(db.double().cpu(), db0.double() + rb), rep
        bar("ln_bwd_dx32", S.ratio(dx32, ref, S.DX32_ATOL, S.DX32_RTOL))


# ------------------------------------------------------------------------------------------------ cls_avgpool_norm
@pytest.mark.parametrize("ntok", S.AVGPOOL_NTOK)
def test_cls_avgpool_norm(ops, L, ntok):
    gamma, beta = (t.to(DEV) for t in S.ln_params())
    for frames in (1, 3):
        x = S.ln_rows("plain", frames * ntok, seed=ntok).view(frames, ntok * D).to(DEV)
        xv, _ = S.strided_in(x, 16, 4)
        y, buf = G.padded(nan(frames, 2 * D), 8, 4)
        L.call("sais_vit_cls_avgpool_norm", ops._p(xv), xv.stride(0), frames, ntok, D, ops._p(gamma), ops._p(beta), 1e-6,
               ops._p(y), y.stride(0), ops._stream())
        G.untouched(buf, y)
        bar("cls_avgpool_norm_y", S.ratio(y, S.cls_avgpool_norm(x.view(frames, ntok, D), gamma, beta, 1e-6), S.Y32_ATOL))


# ------------------------------------------------------------------------------------------------ patchify, cls_rows
@pytest.mark.parametrize("side,frames", S.PATCHIFY)
def test_patchify(ops, side, frames):
    g = side // 16
    img = rnd(frames, 3, side, side, seed=side + frames)
    ref = img.reshape(frames, 3, g, 16, g, 16).permute(0, 2, 4, 1, 3, 5).reshape(frames * g * g, 768).to(BF16)
    for rep in range(2):
        out, buf = out2d(frames * g * g, 768, 0, 0, BF16)
        ops.patchify(img, out)
        assert bits_equal(out, ref), rep
        G.untouched(buf, out)


@pytest.mark.parametrize("ntok", [37, 197])
def test_cls_rows(ops, ntok):
    cls, pos0 = rnd(D, seed=41), rnd(D, seed=42)
    want = (cls.double() + pos0.double()).float()
    for frames, rep in itertools.product((1, 5), range(2)):
        tok = nan(frames, ntok, D)
        ops.vit_cls_rows(cls, pos0, tok, frames, ntok=ntok)
        assert bits_equal(tok[:, 0], want.expand(frames, D))
        G.untouched(tok, tok[:, 0])


# ------------------------------------------------------------------------------------------------ embed_bwd
@pytest.mark.parametrize("ntok", S.EMBED_NTOK)
def test_embed_bwd_integer_sums_exactly(ops, ntok):
    dcls0, dpos0 = S.ints((D,), 6, 1, 4), S.ints((ntok, D), 7, -4, -1)
    for frames in S.EMBED_FRAMES:
        dtok = S.ints((frames, ntok, D), 100 + frames)
        rc, rp, patch, apos = S.embed_bwd(dtok, dcls0, dpos0)
        assert S.int_exact(apos, apos[0] + dcls0.double().abs())
        for rep in range(2):
            dcls, dpos = dcls0.to(DEV), dpos0.to(DEV)
            dpatch, buf = out2d(frames * (ntok - 1), D, 0, 0, BF16)
            ops.vit_embed_bwd(dtok.to(DEV), frames, dcls, dpos, dpatch, ntok=ntok)
            assert torch.equal(dcls.double().cpu(), rc) and torch.equal(dpos.double().cpu(), rp), (frames, rep)
            assert bits_equal(dpatch.cpu(), patch), (frames, rep)
            G.untouched(buf, dpatch)


def test_embed_bwd_random(ops):
    frames, ntok = 7, 37
    dtok, dcls0, dpos0 = rnd(frames, ntok, D, seed=43), rnd(D, seed=44), rnd(ntok, D, seed=45)
    rc, rp, patch, apos = S.embed_bwd(dtok, dcls0, dpos0)
    dcls, dpos, dpatch = dcls0.clone(), dpos0.clone(), nan(frames * (ntok - 1), D, dtype=BF16)
    ops.vit_embed_bwd(dtok, frames, dcls, dpos, dpatch, ntok=ntok)
    acls = dcls0.double().cpu().abs() + dtok[:, 0].double().cpu().abs().sum(0)
    bar("embed_bwd_dcls", float(((dcls.double().cpu() - rc).abs() / S.sum_bar(acls, frames + 1)).max()))
    bar("embed_bwd_dpos", float(((dpos.double().cpu() - rp).abs() / S.sum_bar(apos, frames + 1)).max()))
    assert bits_equal(dpatch.cpu(), patch)


def test_embed_bwd_three_kernel_path_at_dim_516(ops, L):
    frames, ntok, dim = 5, 9, 516
    dtok, dcls0, dpos0 = S.ints((frames, ntok, dim), 46), S.ints((dim,), 47, 1, 4), S.ints((ntok, dim), 48, -4, -1)
    rc, rp, patch, apos = S.embed_bwd(dtok, dcls0, dpos0)
    assert S.int_exact(apos, apos[0] + dcls0.double().abs())
    for rep in range(2):
        dcls, dpos = dcls0.to(DEV), dpos0.to(DEV)
        dpatch, buf = out2d(frames * (ntok - 1), dim, 0, 0, BF16)
        L.call("sais_vit_embed_bwd", ops._p(dtok.to(DEV)), frames, ntok, dim, ops._p(dcls), ops._p(dpos), ops._p(dpatch),
               ops._stream())
        assert torch.equal(dcls.double().cpu(), rc) and torch.equal(dpos.double().cpu(), rp) and bits_equal(dpatch.cpu(), patch)
        G.untouched(buf, dpatch)


# ------------------------------------------------------------------------------------------------ sgd, casts, transposes
@pytest.mark.parametrize("n", S.SGD_N)
def test_sgd_step(ops, n):
    p0, g = rnd(n, seed=n), rnd(n, seed=n + 1)
    ref = S.sgd(p0, g, 0.1, 0.5)
    for shadow in (False, True):
        p, pbuf = vec(n, fill=p0)
        sh, sbuf = vec(n, BF16) if shadow else (None, None)
        ops.sgd_step(p, g, sh, 0.1, 0.5)
        G.untouched(pbuf, p)
        bar("sgd_step_param", S.ratio(p, ref, S.SGD_ATOL))
        if shadow:
            G.untouched(sbuf, sh)
            assert bits_equal(sh, p.to(BF16))


def test_sgd_step_rejects_a_misaligned_shadow(ops, L):
    n = 1025
    p0, g = rnd(n, seed=1), rnd(n, seed=2)
    p, sbuf = p0.clone(), nan(n + 8, dtype=BF16)
    for off in (1, 2, 3):
        with pytest.raises(L.SaisHipError, match="invalid argument"):
            ops.sgd_step(p, g, sbuf[off:off + n], 0.1, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(p, p0) and bool(torch.isnan(sbuf).all())                        # rejected, never launched
    ops.sgd_step(p, g, sbuf[4:4 + n], 0.1, 0.5)
    assert bits_equal(sbuf[4:4 + n], p.to(BF16))


def test_cast_bf16_and_scale(ops):
    for n, rep in itertools.product(S.CAST_N, range(2)):
        src = rnd(n, seed=n, scale=3.0)
        dst, buf = vec(n, BF16)
        ops.cast_bf16(src, dst)
        assert bits_equal(dst.cpu(), src.cpu().to(BF16)), n
        G.untouched(buf, dst)
        p, pbuf = vec(n, fill=src)
        ops.scale_(p, inv_keep())
        assert bits_equal(p.cpu(), (src.double().cpu() * inv_keep()).float()), n      # one rounding of an exact fp64 product
        G.untouched(pbuf, p)


@pytest.mark.parametrize("rows,dim", S.CAST_ROWS)
def test_cast_bf16_rows(ops, rows, dim):
    src = rnd(rows, dim, seed=rows, scale=3.0)
    scale = (torch.randint(0, 2, (rows,), generator=S.gen(rows)).float() * inv_keep()).to(DEV)
    scale[0], scale[-1] = 0.0, inv_keep()
    for rep in range(2):
        dst, buf = out2d(rows, dim, 0, 0, BF16)
        ops.cast_bf16_rows(src, scale, dst)
        assert bits_equal(dst.cpu(), S.cast_rows(src, scale)), rep
        G.untouched(buf, dst)


@pytest.mark.parametrize("rows,cols", S.TRANSPOSE)
def test_transposes(ops, rows, cols):
    src = rnd(rows, cols, seed=rows * 100 + cols, scale=3.0)
    for rep in range(2):
        d16, b16 = vec(rows * cols, BF16)
        d32, b32 = vec(rows * cols)
        ops.transpose_cast_bf16(src, rows, cols, d16)
        ops.transpose_f32(src, rows, cols, d32)
        assert bits_equal(d16.view(cols, rows), src.t().contiguous().to(BF16)), rep
        assert bits_equal(d32.view(cols, rows), src.t().contiguous()), rep
        G.untouched(b16, d16), G.untouched(b32, d32)


# ------------------------------------------------------------------------------------------------ DINO loss kernels
@pytest.mark.parametrize("n", S.LSE_N)
def test_dino_row_lse(ops, n):
    center = rnd(n, seed=n, scale=0.05)
    for rows, kind in itertools.product((1, 3), S.LSE_KINDS):
        x = S.lse_rows(kind, rows, n, seed=n + rows).to(DEV)
        xv, _ = S.strided_in(x, 8, 4)
        for c, scale in itertools.product((None, center), (10.0, 25.0)):
            lse, buf = vec(rows)
            ops.dino_row_lse(xv, scale, c, out=lse)
            G.untouched(buf, lse)
            bar("dino_row_lse_lse", S.ratio(lse, S.row_lse(x, scale, c), S.LSE_ATOL, ulps=2))


@pytest.mark.parametrize("B", S.LOSS_B)
@pytest.mark.parametrize("n", S.LOSS_N)
def test_dino_loss(ops, L, n, B):
    for ncrops in S.LOSS_NCROPS:
        s, t = rnd(ncrops * B, n, seed=n + ncrops, scale=0.4), rnd(2 * B, n, seed=n + 50, scale=0.4)
        c = rnd(n, seed=n + 51, scale=0.05)
        sv, _ = S.strided_in(s, 8, 4)
        tv, _ = S.strided_in(t, 12, 8)
        s_lse, t_lse = S.row_lse(s, 1.0 / S.f32(0.1)).float().to(DEV), S.row_lse(t, 1.0 / S.f32(0.05), c).float().to(DEV)
        ref, rdl = S.dino_loss(s, t, c, 0.05, ncrops)
        first = None
        for rep in range(2):
            dl, buf = G.padded(nan(ncrops * B, n), 16, 12)
            loss, partials = nan(), nan(L.load().sais_dino_loss_partials(B, n))
            ops.dino_loss(sv, tv, c, s_lse, t_lse, B, ncrops, 0.1, 0.05, dl, loss, partials=partials)
            G.untouched(buf, dl)
            bar("dino_loss_loss", abs(loss.item() - float(ref)) / (S.LOSS_RTOL * float(ref)))
            bar("dino_loss_dlogits", S.rel_l2(dl, rdl) / S.DLOGITS_REL)
            assert not bool(torch.isnan(partials).any())
            if first is not None:
                assert bits_equal(dl, first[0]) and bits_equal(loss, first[1]) and bits_equal(partials, first[2])
            first = (dl.clone(), loss.clone(), partials.clone())


@pytest.mark.parametrize("rows", S.COLSUM_ROWS)
def test_dino_colsum_integer_sums_exactly(ops, rows):
    for n in S.COLSUM_N:
        x = S.ints((rows, n), 60 + n, -64, 64)
        ref, a = S.colsum(x)
        assert S.int_exact(a)
        xv, _ = S.strided_in(x.to(DEV), 8, 4)
        for rep in range(2):
            out, buf = vec(n)
            ops.dino_colsum(xv, out)
            assert torch.equal(out.double().cpu(), ref), (n, rep)
            G.untouched(buf, out)


def test_dino_center_ema(ops):
    for n in S.CENTER_N:
        c0, cs = rnd(n, seed=n, scale=0.05), rnd(n, seed=n + 1, scale=1.5)
        c, buf = vec(n, fill=c0)
        ops.dino_center_ema(c, cs, 0.9, 1.0 / 6)
        G.untouched(buf, c)
        bar("dino_center_ema_center", S.ratio(c, S.center_ema(c0, cs, 0.9, 1.0 / 6), S.CENTER_ATOL))


# ------------------------------------------------------------------------------------------------ DINO head pieces
@pytest.mark.parametrize("n", S.GELU_N)
def test_gelu_fwd_bwd(ops, n):
    u, dh = S.gelu_inputs(n, seed=n).to(DEV), rnd(n, seed=n + 1)
    h, hbuf = vec(n)
    du, dbuf = vec(n)
    ops.gelu_fwd_f32(u, h)
    ops.gelu_bwd_f32(dh, u, du)
    G.untouched(hbuf, h), G.untouched(dbuf, du)
    bar("gelu_fwd_h", S.ratio(h, S.gelu(u), S.GELU_ATOL, ulps=2))
    bar("gelu_bwd_du", S.ratio(du, dh.double().cpu() * S.dgelu(u), S.DGELU_ATOL, ulps=2))


@pytest.mark.parametrize("b_side", [False, True])
@pytest.mark.parametrize("rows,K", S.SPLIT3)
def test_split_bf16x3(ops, rows, K, b_side):
    x = S.split3_values(rows, K, seed=rows)
    xv, _ = S.strided_in(x.to(DEV), 8, 4)
    ref = S.split3(x, b_side)
    for rep in range(2):
        dst, buf = out2d(rows, 3 * K, 0, 0, BF16)
        ops.split_bf16x3(xv, dst, b_side)
        assert bits_equal(dst.cpu(), ref), rep
        G.untouched(buf, dst)


@pytest.mark.parametrize("eps", S.L2_EPS)
@pytest.mark.parametrize("dim", S.ROW_DIMS)
def test_l2norm_fwd_bwd(ops, dim, eps):
    for rows in S.ROW_ROWS:
        z, kinds = S.l2_rows(rows, dim, eps, seed=dim)
        assert S.l2_condition(z, eps)
        dout = rnd(rows, dim, seed=dim + rows)
        ref, rinv, rdz = S.l2norm(z, eps, dout)
        out, obuf = out2d(rows, dim, 0, 0)
        dz, zbuf = out2d(rows, dim, 0, 0)
        inv, ibuf = vec(rows)
        ops.l2norm_fwd(z.to(DEV), out, inv, eps)
        ops.l2norm_bwd(dout, out, inv, dz, eps)
        G.untouched(obuf, out), G.untouched(zbuf, dz), G.untouched(ibuf, inv)
        bar("l2norm_fwd_out", S.ratio(out, ref, S.NORM_FWD, ulps=2))
        bar("l2norm_fwd_inv", S.ratio(inv, rinv, 0.0, S.INV_RTOL))
        groups = {"plain": [r for r, k in enumerate(kinds) if k == "plain"], "two_eps": [r for r, k in enumerate(kinds) if k == "two_eps"],
                  "clamp": S.l2_clamp_rows(kinds)}
        for name, rs in groups.items():                              # each magnitude class on its own: 1 / eps swamps the rest
            if rs:
                r = S.rel_l2(dz[rs], rdz[rs]) / S.NORM_BWD_REL
                print(f"l2norm_bwd {name} dim={dim} rows={rows} eps={eps}: {r:.3f} of the bar")
                bar(f"l2norm_bwd_dz_{name}", r)
        for r in S.l2_clamp_rows(kinds):                             # F.normalize's gradient below the clamp: dout / eps
            assert S.rel_l2(dz[r], dout[r].double().cpu() / S.f32(eps)) <= S.NORM_BWD_REL, (r, kinds[r])


@pytest.mark.parametrize("dim", S.ROW_DIMS)
def test_weight_norm_fwd_bwd(ops, dim):
    for rows, with_dg in itertools.product(S.ROW_ROWS, (True, False)):
        v, g, dw = rnd(rows, dim, seed=dim, scale=0.05), 1.0 + 0.1 * rnd(rows, seed=dim + 1), rnd(rows, dim, seed=dim + 2)
        dv0, dg0 = rnd(rows, dim, seed=dim + 3), rnd(rows, seed=dim + 4)
        rw, rinv, rdv, rdg, terms = S.weight_norm(v, g, dw)
        w, wbuf = out2d(rows, dim, 0, 0)
        inv, ibuf = vec(rows)
        ops.weight_norm_fwd(v, g, w, inv)
        G.untouched(wbuf, w), G.untouched(ibuf, inv)
        bar("weight_norm_fwd_w", S.rel_l2(w, rw) / S.NORM_FWD)
        bar("weight_norm_fwd_inv", S.ratio(inv, rinv, 0.0, S.INV_RTOL))
        dv, vbuf = out2d(rows, dim, 0, 0)
        dv.copy_(dv0)
        dg, gbuf = vec(rows, fill=dg0) if with_dg else (None, None)
        ops.weight_norm_bwd(dw, v, g, inv, dv, dg)
        G.untouched(vbuf, dv)
        bar("weight_norm_bwd_dv", S.rel_l2(dv, dv0.double().cpu() + rdv, denom=rdv) / S.NORM_BWD_REL)
        if with_dg:                                                  # one row's dot product can cancel: the old bar plus the sum bar
            G.untouched(gbuf, dg)
            tol = S.NORM_BWD_REL * rdg.abs() + S.sum_bar(terms + dg0.double().cpu().abs(), dim + 1)
            bar("weight_norm_bwd_dg", float(((dg.double().cpu() - (dg0.double().cpu() + rdg)).abs() / tol).max()))


@pytest.mark.parametrize("dim", S.POS_DIMS)
def test_pos_interp_fwd_bwd(ops, dim):
    from sais_amd import vit
    pos, dpos0 = rnd(197, dim, seed=dim), rnd(197, dim, seed=dim + 1)
    for w, h in S.POS_SIZES:
        Wm = torch.from_numpy(vit.pos_interp_matrix(14, w, h).astype(np.float32)).to(DEV)
        nout = Wm.shape[0]
        out, buf = out2d(nout + 1, dim, 0, 0)
        ops.pos_interp_fwd(Wm, pos, out)
        G.untouched(buf, out)
        bar("pos_interp_fwd_out", S.ratio(out, S.pos_interp_fwd(Wm, pos), S.POS_ATOL))
        dout = rnd(nout + 1, dim, seed=dim + w + h)
        dpos, dbuf = out2d(197, dim, 0, 0)
        dpos.copy_(dpos0)
        ops.pos_interp_bwd(Wm, dout, dpos)
        G.untouched(dbuf, dpos)
        bar("pos_interp_bwd_dpos", S.ratio(dpos, S.pos_interp_bwd(Wm, dout, dpos0), S.POS_ATOL))


# ------------------------------------------------------------------------------------------------ grad_norms + adamw_ema_step
class _Leaf(nn.Module):
    def __init__(self, weight, bias=None):
        super().__init__()
        self.weight = nn.Parameter(weight)
        if bias is not None:
            self.bias = nn.Parameter(bias)


class _Toy(nn.Module):
    def __init__(self):
        super().__init__()
        shapes = S.adamw_toy_shapes()
        t = {n: torch.randn(s, generator=S.gen(70 + i)) * 0.3 for i, (n, s) in enumerate(shapes.items())}
        self.a, self.b = _Leaf(t["a.weight"], t["a.bias"]), _Leaf(t["b.weight"], t["b.bias"])
        self.c, self.last, self.d, self.big = _Leaf(t["c.weight"]), _Leaf(t["last.weight"]), _Leaf(t["d.weight"]), _Leaf(t["big.weight"])
        self.fixed = nn.Parameter(t["fixed"], requires_grad=False)


@pytest.mark.parametrize("with_shadow", [True, False])
@pytest.mark.parametrize("clip", S.ADAMW_CLIPS)
def test_grad_norms_adamw_ema(clip, with_shadow):
    """two steps of dino._FlatAdamW over tensors of S.ADAMW_SIZES: class 1 frozen in the first, a tensor without a gradient whose
    teacher copy still moves, an all-zero gradient, decayed and undecayed tensors, with and without the bf16 shadows"""
    from sais_amd import dino
    from sais_amd.flat import FlatParams
    student, teacher = _Toy(), _Toy()
    with torch.no_grad():
        for p in teacher.parameters():
            p.mul_(0.5)                                              # a teacher that differs: the EMA has something to do
    init_s = {n: p.detach().clone() for n, p in student.named_parameters()}
    init_t = {n: p.detach().clone() for n, p in teacher.named_parameters()}
    sf, tf = FlatParams(student, DEV), FlatParams(teacher, DEV)
    sf.refresh_shadows([]), tf.refresh_shadows([])
    s16, t16 = sf.w16.clone(), tf.w16.clone()
    part = dino._FlatAdamW(sf, tf, "head.", S.ADAMW_CLASS1)
    ref = S.OptRef(init_s, S.ADAMW_CLASS1, S.ADAMW_NO_GRAD)
    ref.tt = {n: v.double() for n, v in init_t.items()}
    names = [n for n, _ in student.named_parameters()]
    counts = [0, 0]
    for it in range(2):
        frozen = it == 0
        lr, wd, mom = 1e-3 * (it + 1), 0.05 * (it + 1), 0.9 + 0.02 * it
        sf.grad.zero_()
        grads = {}
        for i, (n, p) in enumerate(student.named_parameters()):
            if p.requires_grad:
                grads[n] = torch.randn(p.shape, generator=S.gen(200 + 10 * it + i)) * (0.0 if n == S.ADAMW_ZERO_GRAD else 0.3)
                sf.g(n).copy_(grads[n])
        norms = part.grad_norms(1.0).cpu()
        counts[0] += 1
        counts[1] += 0 if frozen else 1
        part.step(clip, lr, wd, (0.9, 0.999), 1e-8, counts, frozen, mom, with_shadow=with_shadow)
        rn = ref.step(grads, clip, lr, wd, mom, frozen)
        for i, n in enumerate(names):
            if n in rn:
                bar("grad_norms_norm", abs(float(norms[i]) - float(rn[n])) / (S.GRAD_NORM_RTOL * float(rn[n]) + S.GRAD_NORM_ATOL))
        assert float(rn[S.ADAMW_ZERO_GRAD]) == 0.0 and len(rn) == len(names) - 1
        sp, tp = dict(student.named_parameters()), dict(teacher.named_parameters())
        for n in names:
            bar("adamw_ema_step_param", S.ratio(sp[n], ref.st[n], S.ADAMW_ATOL))
            bar("adamw_ema_step_teacher", S.ratio(tp[n], ref.tt[n], S.ADAMW_ATOL))
            if with_shadow:
                assert bits_equal(sf.w(n), sp[n].detach().to(BF16)) and bits_equal(tf.w(n), tp[n].detach().to(BF16)), (it, n)
        if not with_shadow:
            assert bits_equal(sf.w16, s16) and bits_equal(tf.w16, t16)
    assert ref.steps["last.weight"] == 1 and ref.steps["a.weight"] == 2
    assert torch.equal(student.fixed.detach().cpu(), init_s["fixed"])
    assert not torch.equal(teacher.fixed.detach().cpu(), init_t["fixed"])            # its teacher copy still moved
    assert not torch.equal(dict(student.named_parameters())[S.ADAMW_ZERO_GRAD].detach().cpu(), init_s[S.ADAMW_ZERO_GRAD])   # decay alone
