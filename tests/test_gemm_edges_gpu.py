"""The NT GEMM kernels (sais_gemm_nt, its row-owning form with the LayerNorm epilogues, sais_gemm_nt_f32, sais_tgemm) in every
launch form, at every K depth and with free row strides, on a real MI355X.

Exact cases use the recipes of tests/gemm_ref.py (`tern`, `x3`): the condition that makes the fp64 reference independent of the
summation order is asserted on the reference first, then the kernel output must be torch.equal to it, on two launches into
fresh NaN buffers.  What cannot be exact (GELU family, one-byte GELU' codes, LayerNorm statistics and gradients) runs on seeded
random data against fp64 under the bars of test_kernels_gpu.py (test_gemm_nt_epilogues, test_gemm_ln_fwd, test_gemm_ln_bwd,
test_gemm_ln_bwd_from_the_saved_bf16_layernorm_output), unchanged; observed / bar goes to parity_log("gemm_edge_...").
Shapes are chosen from the launchers' published rules (gemm_ref.w8p_tiles, row_waves, row_rows_per_tile; checked in
test_gemm_ref_host.py::test_launcher_rules); the tests assert on results only."""
import ctypes
import functools
import math

import pytest
import torch

import gemm_ref as G
import parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = G.NAN
BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-6


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
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype).to(DEV)


def eq(got, ref64):
    """bit for bit: the output, widened, IS the fp64 reference (a NaN left behind fails)"""
    return torch.equal(got.double(), ref64)


@functools.lru_cache(maxsize=2)
def _tern(M, N, K):
    """(A, W, bias on the device, A.W^T in fp64): computed once per shape, never written to"""
    a, w, bias = (t.to(DEV) for t in G.tern(M, N, K))
    return a, w, bias, G.mm64(a, w)


def ratio(got, ref, atol, rtol=0.0):
    return float(((got.double() - ref).abs() / (atol + rtol * ref.abs())).max())


def bar(name, got, ref, atol, rtol=0.0):
    r = ratio(got, ref, atol, rtol)
    print(f"{name}: {r:.3f} of the bar")
    parity.parity_log(f"gemm_edge_{name}", r, 1.0)
    assert r <= 1.0, (name, r)


# ------------------------------------------------------------------------------------------------ sais_gemm_nt, exact
def _nt_exact(ops, L, a, w, bias, acc, epis, tag):
    """every epilogue of `epis` twice into fresh NaN buffers, each bit-equal to fp64"""
    M, N = acc.shape
    ref = acc + bias.double()
    assert float(ref.abs().max()) <= G.BF16_MAX_INT and G.bf16_exact(ref), tag
    resid = G.tern_resid(M, N).to(DEV)
    aux = G.tern_aux(M, N).to(DEV) if ("mul" in epis or "drelu" in epis) else None
    rs = G.tern_rowscale(M).to(DEV)
    first = {}
    for rep in range(2):
        for e in epis:
            if e == "bias_bf16":
                out = ops.gemm_nt(a, w, L.EPI_BIAS_BF16, nan(M, N, dtype=BF16), bias=bias)
                assert eq(out, ref), (tag, e)
            elif e == "relu":
                out = ops.gemm_nt(a, w, L.EPI_BIAS_RELU_BF16, nan(M, N, dtype=BF16), bias=bias)
                assert eq(out, ref.relu()), (tag, e)
            elif e == "f32":
                out = ops.gemm_nt(a, w, L.EPI_BIAS_F32, nan(M, N), bias=bias)
                assert eq(out, ref), (tag, e)
            elif e == "resid2":
                want = ref + resid.double()
                assert G.bf16_exact(want)
                out, o2 = nan(M, N), nan(M, N, dtype=BF16)
                ops.gemm_nt(a, w, L.EPI_BIAS_RESID_F32, out, bias=bias, aux=resid, out2=o2)
                assert eq(out, want) and eq(o2, want), (tag, e)
            elif e == "resid":
                out = ops.gemm_nt(a, w, L.EPI_BIAS_RESID_F32, nan(M, N), bias=bias, aux=resid)
                assert eq(out, ref + resid.double()), (tag, e)
            elif e == "resid_rs":
                want = resid.double() + rs.double()[:, None] * ref
                assert G.f32_exact(want)
                out = ops.gemm_nt(a, w, L.EPI_BIAS_RESID_F32, nan(M, N), bias=bias, aux=resid, rowscale=rs)
                assert eq(out, want), (tag, e)
            elif e == "mul":
                want = acc * aux.double()
                assert G.bf16_exact(want)
                out = ops.gemm_nt(a, w, L.EPI_MUL_BF16, nan(M, N, dtype=BF16), aux=aux)
                assert eq(out, want), (tag, e)
            elif e == "drelu":
                out = ops.gemm_nt(a, w, L.EPI_DRELU_BF16, nan(M, N, dtype=BF16), aux=aux)
                assert eq(out, acc * (aux.double() > 0)), (tag, e)
            else:
                raise KeyError(e)
            if rep == 0:
                first[e] = out
            else:
                assert torch.equal(out, first[e]), (tag, e, "second launch")
    return first


@pytest.mark.parametrize("M,N,K", G.W8P_DEPTH)
def test_w8p_k_depth(ops, L, M, N, K):
    """the persistent eight-wave kernel at 1, 2, 3, 4, 5, 7, 12 and 24 K-steps: 65 full row tiles x 8 (every workgroup's first
    tile full, eight take a second) and 66 with a ragged last one, through a 4-store, an 8-store and a 12-store epilogue"""
    assert G.w8p_tiles(M, N) > G.W8P_GRID
    _nt_exact(ops, L, *_tern(M, N, K), ("bias_bf16", "f32", "resid2"), ("w8p", M, K))


def _gelu_parts(u):
    cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
    return u * cdf, cdf + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def _gelu_family(ops, L, a, w, bias, tag, views=lambda t, i: t):
    """GELU + pre-activation, GELU + one-byte GELU' codes, the code multiply: bars of test_gemm_nt_epilogues.  `views` may
    replace an output / aux tensor by a strided view of a sentinel buffer."""
    M, N = a.shape[0], w.shape[0]
    ref = G.mm64(a, w) + bias.double()
    gelu, grad = _gelu_parts(ref)
    tol = dict(atol=2e-2, rtol=1e-2)
    out, u = views(nan(M, N, dtype=BF16), 0), views(nan(M, N, dtype=BF16), 1)
    ops.gemm_nt(a, w, L.EPI_BIAS_GELU_BF16, out, bias=bias, out2=u)
    bar(f"{tag}_gelu", out, gelu, **tol)
    bar(f"{tag}_gelu_pre", u, ref, **tol)
    out, dq = views(nan(M, N, dtype=BF16), 2), views(torch.full((M, N), G.U8_SENTINEL, dtype=torch.uint8, device=DEV), 3)
    ops.gemm_nt(a, w, L.EPI_BIAS_GELU_GRADQ_BF16, out, bias=bias, out2=dq)
    bar(f"{tag}_gelu_gradq_out", out, gelu, **tol)
    want = (26 + 203 * grad).round().clamp(0, 255)
    off, frac = float((dq.double() - want).abs().max()), float((dq.double() != want).double().mean())
    deq = float(((dq.double() - 26) / 203 - grad).abs().max())
    print(f"{tag}: codes off by at most {off:.0f}, {frac:.2e} of them; dequantised error {deq:.3e}")
    parity.parity_log(f"gemm_edge_{tag}_gradq_code_mismatch", frac, 2e-3)
    parity.parity_log(f"gemm_edge_{tag}_gradq_dequant", deq, 0.5 / 203 + 1.5e-3)
    assert off <= 1 and frac <= 2e-3 and deq <= 0.5 / 203 + 1.5e-3
    codes = torch.randint(0, 256, (M, N), dtype=torch.uint8, generator=torch.Generator().manual_seed(12)).to(DEV)
    out = views(nan(M, N, dtype=BF16), 4)
    ops.gemm_nt(a, w, L.EPI_MULQ_BF16, out, aux=views(codes, 5))
    bar(f"{tag}_mulq", out, (ref - bias.double()) * ((codes.double() - 26) / 203), **tol)


@pytest.mark.parametrize("M,N,K", G.W8P_RANDOM)
def test_w8p_k_depth_gelu_family(ops, L, M, N, K):
    a = rnd(M, K, seed=3, dtype=BF16)
    w = rnd(N, K, seed=4, scale=0.05, dtype=BF16)
    _gelu_family(ops, L, a, w, rnd(N, seed=5, scale=0.1), f"w8p_k{K}")


@pytest.mark.parametrize("M,N,K", G.PATCH)
def test_w8p_patch_embedding(ops, L, M, N, K):
    """EPI_PATCH_F32 at K = 768 on the eight-wave kernel, one round (198 tiles) and 405 tiles: token rows exact, CLS rows untouched"""
    a, w, bias, acc = _tern(M, N, K)
    Fr = M // 196
    pos = G.tern_resid(197, N).to(DEV)
    want = (acc + bias.double()).view(Fr, 196, N) + pos[1:].double()
    assert G.f32_exact(want)
    for _ in range(2):
        tok = nan(Fr, 197, N)
        ops.gemm_nt(a, w, L.EPI_PATCH_F32, tok, bias=bias, aux=pos, grp=(196, 197, 1))
        assert eq(tok[:, 1:], want)
        assert torch.isnan(tok[:, 0]).all()


@pytest.mark.parametrize("M,N,K", G.PREFETCH)
def test_w8p_prefetch_edges(ops, L, M, N, K):
    """7, 8, 11, 16 and 17 column tiles at K = 384: both sides of both ends of the L2 prefetch's range, and 11, where
    ceil(128 / 11) x 11 > 128 rows; 75 row tiles with a ragged last one"""
    _nt_exact(ops, L, *_tern(M, N, K), ("bias_bf16", "f32"), ("prefetch", N))


@pytest.mark.parametrize("M,N,K", G.NTN1)
def test_w8p_one_column_tile_second_round(ops, L, M, N, K):
    _nt_exact(ops, L, *_tern(M, N, K), ("bias_bf16", "f32", "resid2"), ("ntn1", K))


@pytest.mark.parametrize("M,N,K", G.BOUNDARY)
def test_dispatch_boundaries(ops, L, M, N, K):
    """M - 1 and M on the two sides of a kernel switch (four-wave | eight-wave persistent or row-owning; four-wave | eight-wave
    row tile): both bit-equal to fp64, hence to each other on their common rows"""
    a, w, bias, acc = _tern(M, N, K)
    hi = _nt_exact(ops, L, a, w, bias, acc, ("bias_bf16", "resid"), ("boundary", M))
    lo = _nt_exact(ops, L, a[:M - 1], w, bias, acc[:M - 1], ("bias_bf16", "resid"), ("boundary", M - 1))
    for e in hi:
        assert torch.equal(hi[e][:M - 1], lo[e])


@pytest.mark.parametrize("M,N,K", G.ROW_PLAIN)
def test_row_kernel_plain_epilogues(ops, L, M, N, K):
    """row tiles of 112 (four waves), 224, 120 (half 1 owns 8 rows; the last tile lies in half 0), 224 x 256 and one row into a
    second round; 1, 2, 3, 6 and 24 K-steps; bf16 and residual epilogues, the latter with and without a row scale"""
    assert G.takes_row_kernel(M, N)
    _nt_exact(ops, L, *_tern(M, N, K), ("bias_bf16", "resid", "resid_rs"), ("row", M, K))


# ------------------------------------------------------------------------------------------------ LayerNorm epilogues
def _ln64(x, gamma, beta):
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + EPS)
    return (x - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double(), mean, rstd


def _check_ln_fwd(tag, x_out, xn, mean, rstd, want, gamma, beta):
    assert eq(x_out, want), (tag, "x_out")
    y, m, r = _ln64(want, gamma, beta)
    bar(f"ln_fwd_mean_{tag}", mean, m, 1e-4)
    bar(f"ln_fwd_rstd_{tag}", rstd, r, 0.0, 1e-4)
    bar(f"ln_fwd_xn_{tag}", xn, y, 2e-2, 1e-2)


@pytest.mark.parametrize("M,N,K", G.LN_CASES)
def test_row_kernel_ln_fwd(ops, M, N, K):
    """x_out = A.W^T + bias + [rowscale] resid bit-exact on tern data; xn, mean, rstd against the fp64 LayerNorm of that x_out"""
    a, w, bias, acc = _tern(M, N, K)
    resid, rs = G.tern_resid(M, N).to(DEV), G.tern_rowscale(M).to(DEV)
    gamma, beta = 1 + 0.1 * rnd(384, seed=204), 0.05 * rnd(384, seed=205)
    ref = acc + bias.double()
    for scale in (None, rs):
        want = resid.double() + (ref if scale is None else scale.double()[:, None] * ref)
        assert G.f32_exact(want)
        x_out, xn, mean, rstd = nan(M, 384), nan(M, 384, dtype=BF16), nan(M), nan(M)
        ops.gemm_ln_fwd(a, w, bias, resid, x_out, xn, gamma, beta, EPS, mean, rstd, rowscale=scale)
        _check_ln_fwd(f"k{K}" + ("" if scale is None else "_rs"), x_out, xn, mean, rstd, want, gamma, beta)


def _ln_bwd_data(M, K):
    a = rnd(M, K, seed=210, scale=0.5, dtype=BF16)
    w = rnd(384, K, seed=211, scale=0.05, dtype=BF16)
    x = rnd(M, 384, seed=212, scale=1.5)
    x[:, 11] -= 20.0
    gamma, beta = 1 + 0.1 * rnd(384, seed=213), 0.05 * rnd(384, seed=224)
    y, mean, rstd = _ln64(x.double(), gamma, beta)
    return a, w, x, gamma, beta, mean.float(), rstd.float(), y.to(BF16)


def _ln_bwd64(a, w, x, gamma, dres_full):
    dy = G.mm64(a, w)
    x = x.double()
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + EPS)
    xhat = (x - mean) * rstd
    g = dy * gamma.double()
    dx = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    if dres_full is not None:
        dx = dx + dres_full.double()
    return dx, (dy * xhat).sum(0), dy.sum(0), float(dy.abs().max())


def _check_ln_bwd(tag, M, ref, dx32, dx16, dgamma, dbeta, from_y16=False, gmax=1.0, dgamma_bar_applies=True):
    dx, dg, db, scale = ref
    if dx32 is not None:
        bar(f"ln_bwd_dx32_{tag}", dx32, dx, (1e-3 * max(1.0, gmax) if from_y16 else 2e-4) * scale, 1e-4)
    if dx16 is not None:
        bar(f"ln_bwd_dx16_{tag}", dx16, dx, 2e-2, 1e-2)
    if dgamma is not None:
        if from_y16:
            assert bool(torch.isfinite(dgamma).all()), tag
            rel = float((dgamma.double() - dg).norm() / dg.norm())
            assert math.isfinite(rel), (tag, rel)
            print(f"ln_bwd_dgamma_{tag}: rel-L2 {rel:.3e} (bar 4e-3)")
            if dgamma_bar_applies:
                parity.parity_log(f"gemm_edge_ln_bwd_dgamma_rel_l2_{tag}", rel, 4e-3)
                assert rel <= 4e-3, (tag, rel)
            else:                       # M <= 113: the rounding of y does not average out over the rows; the value is recorded only
                parity.parity_log(f"gemm_edge_ln_bwd_dgamma_rel_l2_{tag}_few_rows_not_asserted", rel, 4e-3)
        else:
            bar(f"ln_bwd_dgamma_{tag}", dgamma, dg, 2e-4 * scale * math.sqrt(M), 1e-4)
        bar(f"ln_bwd_dbeta_{tag}", dbeta, db, 2e-4 * scale * math.sqrt(M), 1e-4)


@pytest.mark.parametrize("M,N,K", G.LN_CASES)
def test_row_kernel_ln_bwd(ops, M, N, K):
    """dx = dres + dLN(A.W^T), dgamma, dbeta on the random data of test_gemm_ln_bwd against fp64, with the residual gradient in
    place and without it, and in the form that rebuilds xhat from the saved bf16 LayerNorm output y (xn16 + beta), at every M.
    In that form dx32 (xhat enters dx only through xhat * mean(dy g xhat): a bound per row), dx16 (bf16 rounding) and dbeta (no
    xhat in it) keep their bars at any M.  Its dgamma bar, 4e-3 relative L2, rests on the rounding of y averaging out over
    thousands of rows: it is asserted at the M >= 8192 of the list; at M in {1, 111, 112, 113} the value is logged only."""
    a, w, x, gamma, beta, mean, rstd, y16 = _ln_bwd_data(M, K)
    dres = rnd(M, 384, seed=214)
    ref = _ln_bwd64(a, w, x, gamma, dres)
    dx32, dx16, dg, db = dres.clone(), nan(M, 384, dtype=BF16), torch.zeros(384, device=DEV), torch.zeros(384, device=DEV)
    ops.gemm_ln_bwd(a, w, x, mean, rstd, gamma, dres=dx32, dx32=dx32, dx16=dx16, dgamma=dg, dbeta=db)
    _check_ln_bwd(f"k{K}", M, ref, dx32, dx16, dg, db)
    dx_only = nan(M, 384)
    ops.gemm_ln_bwd(a, w, x, mean, rstd, gamma, dx32=dx_only)
    _check_ln_bwd(f"k{K}_nodres", M, _ln_bwd64(a, w, x, gamma, None), dx_only, None, None, None)
    dx32, dx16, dg, db = dres.clone(), nan(M, 384, dtype=BF16), torch.zeros(384, device=DEV), torch.zeros(384, device=DEV)
    ops.gemm_ln_bwd(a, w, x, mean, rstd, gamma, dres=dx32, dx32=dx32, dx16=dx16, dgamma=dg, dbeta=db, xn16=y16, beta=beta)
    _check_ln_bwd(f"k{K}_y16", M, ref, dx32, dx16, dg, db, from_y16=True, gmax=float(gamma.abs().max()),
                  dgamma_bar_applies=M >= 8192)


@pytest.mark.parametrize("M,N,K", G.LN_PERIOD)
def test_row_kernel_ln_bwd_compact_dres(ops, M, N, K):
    """dres_period = 197: the residual gradient exists on the first row of every frame only (four-wave and eight-wave tile)"""
    a, w, x, gamma, beta, mean, rstd, _ = _ln_bwd_data(M, K)
    compact = rnd(M // 197, 384, seed=215)
    full = torch.zeros(M, 384, device=DEV)
    full[::197] = compact
    dx32, dx16, dg, db = nan(M, 384), nan(M, 384, dtype=BF16), torch.zeros(384, device=DEV), torch.zeros(384, device=DEV)
    ops.gemm_ln_bwd(a, w, x, mean, rstd, gamma, dres=compact, dx32=dx32, dx16=dx16, dgamma=dg, dbeta=db, dres_period=197)
    _check_ln_bwd(f"k{K}_period", M, _ln_bwd64(a, w, x, gamma, full), dx32, dx16, dg, db)


# ------------------------------------------------------------------------------------------------ small M
@pytest.mark.parametrize("M,N,K", G.SMALL_NT)
def test_four_wave_small_m(ops, L, M, N, K):
    """the four-wave kernel at 1, 63, 127, 128 and 129 rows, 1 and 24 K-steps: every exact epilogue, and raw split-K slabs (one
    K-step per slice) finished with bias, row scale and residual"""
    a, w, bias, acc = _tern(M, N, K)
    _nt_exact(ops, L, a, w, bias, acc, ("bias_bf16", "relu", "f32", "resid2", "mul", "drelu"), ("small", M, N, K))
    resid, rs = G.tern_resid(M, N).to(DEV), G.tern_rowscale(M).to(DEV)
    ref = acc + bias.double()
    o32 = nan(M, N)
    ops.gemm_nt_splitk(a, w, K // 64, bias=bias, rowscale=rs, aux=resid, out32=o32)
    assert eq(o32, resid.double() + rs.double()[:, None] * ref)
    o32, o16 = nan(M, N), nan(M, N, dtype=BF16)
    ops.gemm_nt_splitk(a, w, K // 64, bias=bias, aux=resid, out32=o32, out16=o16)
    assert G.bf16_exact(ref + resid.double()) and eq(o32, ref + resid.double()) and eq(o16, ref + resid.double())


def _gemm_nt_f32(ops, L, a, w, epilogue, out, bias=None, aux=None, ks=None):
    """ops.gemm_nt_f32, or the same entry with a forced K split `ks` (workspace [ks, M, N])"""
    if ks is None:
        return ops.gemm_nt_f32(a, w, epilogue, out, bias=bias, aux=aux)
    M, (N, K) = a.shape[0], w.shape
    ws = nan(ks, M, N) if ks > 1 else None
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    g = L.SaisGemm(A=ptr(a), lda=a.stride(0), B=ptr(w), ldb=w.stride(0), M=M, N=N, K=K, epilogue=epilogue, bias=ptr(bias),
                   out=ptr(out), ldo=out.stride(-2), out2=ptr(ws), ldo2=ks if ks > 1 else 0, aux=ptr(aux),
                   ldaux=0 if aux is None else aux.stride(-2))                        # fields by name; the rest stay zero
    L.call("sais_gemm_nt_f32", ctypes.byref(g), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out


def _x3_case(M, N, K):
    a, w = (t.to(DEV) for t in G.x3_pair(M, N, K))
    assert G.x3_condition(a, w)
    ref = G.x3_ref(a, w)
    assert G.x3_ref_condition(ref)
    bias = torch.randint(-1, 2, (N,), generator=torch.Generator().manual_seed(N)).float().to(DEV)
    aux = G.tern_resid(M, N).to(DEV)
    return a, w, ref, bias, aux


def _f32_exact(ops, L, a, w, ref, bias, aux, ks, tag, out_view=lambda t: t, aux_view=lambda t: t):
    refb = ref + bias.double()
    aux_v = aux_view(aux)
    for epi, want, kw in ((L.EPI_BIAS_F32, refb, dict(bias=bias)), (L.EPI_BIAS_RELU_F32, refb.relu(), dict(bias=bias)),
                          (L.EPI_BIAS_RESID_F32, refb + aux.double(), dict(bias=bias, aux=aux_v)),
                          (L.EPI_DRELU_F32, ref * (aux.double() > 0), dict(aux=aux_v))):
        assert G.f32_exact(want)
        out = out_view(nan(*ref.shape))
        _gemm_nt_f32(ops, L, a, w, epi, out, ks=ks, **kw)
        assert eq(out, want), (tag, epi, ks)


@pytest.mark.parametrize("M,N,K", G.SMALL_F32)
def test_f32_bf16x3_small_m_three_terms_exactly(ops, L, M, N, K):
    """sais_gemm_nt_f32 == ah wh + ah wl + al wh in fp64, bit for bit, in all four epilogues: with the K split the wrapper picks
    (none, 6, 8) and with one K-step per split"""
    a, w, ref, bias, aux = _x3_case(M, N, K)
    _f32_exact(ops, L, a, w, ref, bias, aux, None, ("f32", M, K))
    forced = K // 64 != G.f32_default_ks(M, N, K)              # at K = 64 and 384 the wrapper's split already is one step each
    assert forced == (K == 2048)
    if forced:
        _f32_exact(ops, L, a, w, ref, bias, aux, K // 64, ("f32", M, K))


@pytest.mark.parametrize("K,ns", G.TGEMM_KS)
@pytest.mark.parametrize("N", [64, 384])
def test_tgemm_three_terms_exactly(ops, L, N, K, ns):
    """sais_tgemm at 1, 63, 64, 65 and 264 rows with 1, 3, 5 (odd: the loop's tail) and 8 K-steps per split: every raw slab is the
    fp64 three-term sum over its own K range; bias, ReLU and dReLU epilogues on the whole K"""
    for M in (1, 63, 64, 65, 264):
        assert (M, N, K, ns) in G.TGEMM
        a, w, ref, bias, aux = _x3_case(M, N, K)
        slabs = nan(ns, M, N)
        ops.tgemm(a, w, L.TG_RAW, slabs, nsplit=ns)
        for z in range(ns):
            assert eq(slabs[z], G.x3_ref(a, w, z * (K // ns), (z + 1) * (K // ns))), (M, z)
        assert eq(ops.tgemm(a, w, L.TG_BIAS, nan(M, N), bias=bias), ref + bias.double()), M
        assert eq(ops.tgemm(a, w, L.TG_BIAS, nan(M, N)), ref), M
        assert eq(ops.tgemm(a, w, L.TG_BIAS_RELU, nan(M, N), bias=bias), (ref + bias.double()).relu()), M
        assert eq(ops.tgemm(a, w, L.TG_DRELU, nan(M, N), aux=aux), ref * (aux.double() > 0)), M


# ------------------------------------------------------------------------------------------------ strided operands
class Pads:
    """hands out a different (pad, offset) per tensor, in units of the entry's granularity, and remembers the outputs"""

    def __init__(self, rows_extra=0):
        self.i, self.outs, self.rows_extra = 0, [], rows_extra

    def __call__(self, t, out=False):
        unit = 16 if t.dtype == torch.uint8 else 8 if t.dtype == BF16 else 4
        self.i += 1
        v, buf = G.padded(t, unit * (self.i + 1), unit * (1 + self.i % 2), rows_extra=self.rows_extra if out else 0)
        if out:
            self.outs.append((buf, v))
        return v

    def check(self):
        assert self.outs
        for buf, v in self.outs:
            G.untouched(buf, v)


@pytest.mark.parametrize("entry", ["nt_small", "nt_large"])
def test_strided_gemm_nt(ops, L, entry):
    """A, W, out, out2 and aux each inside a wider NaN-filled buffer with its own pad and column offset; the large-M case
    also has 128 more rows behind every output: exact results, and nothing outside the views is written"""
    M, N, K = G.STRIDED[entry]
    a, w, bias, acc = _tern(M, N, K)
    P = Pads(G.OVERALLOC_ROWS if entry == "nt_large" else 0)
    resid = G.tern_resid(M, N).to(DEV)
    want = acc + bias.double() + resid.double()
    assert G.bf16_exact(want)
    a_v, w_v = P(a), P(w)
    out, o2 = P(nan(M, N), True), P(nan(M, N, dtype=BF16), True)
    ops.gemm_nt(a_v, w_v, L.EPI_BIAS_RESID_F32, out, bias=bias, aux=P(resid), out2=o2)
    assert eq(out, want) and eq(o2, want)
    o16 = P(nan(M, N, dtype=BF16), True)
    ops.gemm_nt(a_v, w_v, L.EPI_BIAS_BF16, o16, bias=bias)
    assert eq(o16, acc + bias.double())
    P.check()
    # byte strides of the one-byte GELU' codes (granularity 16), random data under the existing bars
    P = Pads(G.OVERALLOC_ROWS if entry == "nt_large" else 0)
    ar, wr = rnd(M, K, seed=3, dtype=BF16), rnd(N, K, seed=4, scale=0.05, dtype=BF16)
    _gelu_family(ops, L, P(ar), P(wr), rnd(N, seed=5, scale=0.1), f"strided_{entry}", views=lambda t, i: P(t, out=i != 5))
    P.check()


def test_strided_row_kernel_plain(ops, L):
    M, N, K = G.STRIDED["row_plain"]
    a, w, bias, acc = _tern(M, N, K)
    P = Pads(G.OVERALLOC_ROWS)
    resid, rs = G.tern_resid(M, N).to(DEV), G.tern_rowscale(M).to(DEV)
    a_v, w_v = P(a), P(w)
    out = P(nan(M, N), True)
    ops.gemm_nt(a_v, w_v, L.EPI_BIAS_RESID_F32, out, bias=bias, aux=P(resid), rowscale=rs)
    assert eq(out, resid.double() + rs.double()[:, None] * (acc + bias.double()))
    o16 = P(nan(M, N, dtype=BF16), True)
    ops.gemm_nt(a_v, w_v, L.EPI_BIAS_BF16, o16, bias=bias)
    assert eq(o16, acc + bias.double())
    P.check()


def test_strided_row_kernel_ln_fwd(ops):
    M, N, K = G.STRIDED["ln_fwd"]
    a, w, bias, acc = _tern(M, N, K)
    P = Pads()
    resid = G.tern_resid(M, N).to(DEV)
    gamma, beta = 1 + 0.1 * rnd(384, seed=204), 0.05 * rnd(384, seed=205)
    x_out, xn, mean, rstd = P(nan(M, 384), True), P(nan(M, 384, dtype=BF16), True), nan(M), nan(M)
    ops.gemm_ln_fwd(P(a), P(w), bias, P(resid), x_out, xn, gamma, beta, EPS, mean, rstd)
    _check_ln_fwd("strided", x_out, xn, mean, rstd, acc + bias.double() + resid.double(), gamma, beta)
    P.check()


def test_strided_row_kernel_ln_bwd(ops):
    M, N, K = G.STRIDED["ln_bwd"]
    a, w, x, gamma, beta, mean, rstd, y16 = _ln_bwd_data(M, K)
    dres = rnd(M, 384, seed=214)
    ref = _ln_bwd64(a, w, x, gamma, dres)
    P = Pads()
    a_v, w_v, x_v, dres_v = P(a), P(w), P(x), P(dres)
    for from_y16 in (False, True):
        dx32, dx16 = P(nan(M, 384), True), P(nan(M, 384, dtype=BF16), True)
        dg, db = torch.zeros(384, device=DEV), torch.zeros(384, device=DEV)
        kw = dict(xn16=P(y16), beta=beta) if from_y16 else {}
        ops.gemm_ln_bwd(a_v, w_v, x_v, mean, rstd, gamma, dres=dres_v, dx32=dx32, dx16=dx16, dgamma=dg, dbeta=db, **kw)
        _check_ln_bwd("strided" + ("_y16" if from_y16 else ""), M, ref, dx32, dx16, dg, db, from_y16=from_y16,
                      gmax=float(gamma.abs().max()))
    P.check()


def test_strided_f32_bf16x3(ops, L):
    M, N, K = G.STRIDED["f32"]
    a, w, ref, bias, aux = _x3_case(M, N, K)
    P = Pads()
    a_v, w_v = P(a), P(w)
    for ks in (None, 1):                                   # the wrapper's split (3, through the reduce kernel) and the direct epilogue
        _f32_exact(ops, L, a_v, w_v, ref, bias, aux, ks, "f32 strided", out_view=lambda t: P(t, True), aux_view=P)
    P.check()


def test_strided_tgemm(ops, L):
    M, N, K = G.STRIDED["tgemm"]
    a, w, ref, bias, aux = _x3_case(M, N, K)
    P = Pads()
    a_v, w_v = P(a), P(w)
    out = P(nan(M, N), True)
    ops.tgemm(a_v, w_v, L.TG_DRELU, out, aux=P(aux))
    assert eq(out, ref * (aux.double() > 0))
    out = P(nan(M, N), True)
    ops.tgemm(a_v, w_v, L.TG_BIAS_RELU, out, bias=bias)
    assert eq(out, (ref + bias.double()).relu())
    slabs = P(nan(3, M, N), True)
    ops.tgemm(a_v, w_v, L.TG_RAW, slabs, nsplit=3)
    for z in range(3):
        assert eq(slabs[z], G.x3_ref(a, w, 64 * z, 64 * z + 64))
    P.check()


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections(ops, L):
    """each raises before any launch: the outputs keep their NaN"""
    E = L.SaisHipError
    a, w = torch.zeros(128, 128, dtype=BF16, device=DEV), torch.zeros(256, 128, dtype=BF16, device=DEV)
    out, o8 = nan(128, 256, dtype=BF16), torch.full((128, 264), G.U8_SENTINEL, dtype=torch.uint8, device=DEV)
    with pytest.raises(E):                                                       # K = 96
        ops.gemm_nt(a[:, :96], w[:, :96], L.EPI_BIAS_BF16, out)
    with pytest.raises(E):                                                       # N = 192
        ops.gemm_nt(a, w[:192], L.EPI_BIAS_BF16, out[:, :192])
    wide = torch.zeros(128, 68, dtype=BF16, device=DEV)
    with pytest.raises(E):                                                       # lda = K + 4
        ops.gemm_nt(wide[:, :64], w[:, :64], L.EPI_BIAS_BF16, out)
    with pytest.raises(E):                                                       # ldo2 = 264 for the one-byte codes
        ops.gemm_nt(a, w, L.EPI_BIAS_GELU_GRADQ_BF16, out, out2=o8[:, :256])
    af, wf, slabs = torch.zeros(64, 192, device=DEV), torch.zeros(64, 192, device=DEV), nan(2, 64, 64)
    with pytest.raises(E):                                                       # 2 does not divide K / 64 = 3
        ops.tgemm(af, wf, L.TG_RAW, slabs, nsplit=2)
    rs = torch.ones(128, device=DEV)
    with pytest.raises(E):                                                       # a row scale needs the residual epilogue
        ops.gemm_nt(a, w, L.EPI_BIAS_BF16, out, rowscale=rs)
    M = 8192
    ab, wb = torch.zeros(M, 64, dtype=BF16, device=DEV), torch.zeros(512, 64, dtype=BF16, device=DEV)
    o32, res = nan(M, 512), torch.zeros(M, 512, device=DEV)
    with pytest.raises(E):                                                       # the eight-wave kernel has no row scale
        ops.gemm_nt(ab, wb, L.EPI_BIAS_RESID_F32, o32, aux=res, rowscale=torch.ones(M, device=DEV))
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(o32).all() and torch.isnan(slabs).all() and bool((o8 == G.U8_SENTINEL).all())
