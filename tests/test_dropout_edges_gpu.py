"""Every kernel that draws a dropout or DropPath mask, element for element against the independent Philox4x32-10 model of
tests/philox_ref.py (numpy, written from the published rule; its known answers are checked in test_philox_ref_host.py), on a
real MI355X.  Nothing here asks the library for a mask to compare another kernel with: the expected keep bits come from the
model alone, and every comparison is exact (torch.equal / np.array_equal) unless stated.

  a. sais_dropout_mask, sais_dropout_f32, sais_rng_advance   (csrc/misc.hip: philox_keep)
  b. sais_tgemm, TG_BIAS_RELU / TG_DRELU                      (csrc/tgemm.hip: keep4 -> philox_u32x4, four draws per block)
  c. sais_gemm_nt_f32, direct epilogue and splitk_reduce_kernel (csrc/gemm_nt_f32.hip: philox_keep)
  d. sais_temporal_ln_fwd / _bwd                              (csrc/tgemm.hip: drop12 -> keep4)
  e. sais_droppath_scales                                     (csrc/misc.hip: philox_keep)
  f. inherited, not repeated here: the attention sites (csrc/tattn_frag.hpp, used by tattn.hip and tattn_long.hip) and
     sais_layernorm_bwd's dx32_drop (csrc/norm.hip) are compared element for element with sais_dropout_mask at their tile
     edges in test_temporal_edges_gpu.py, test_temporal_long_gpu.py and test_stream_edges_gpu.py; with (a) pinning
     sais_dropout_mask to the model, they are pinned to it as well.

GEMM operands follow the `x3` recipe of tests/gemm_ref.py (every partial sum exact), the row kernels get small integers, and
at p = 0.5 / 0.75 the scale 1 / (1 - p) is a power of two: neither rounding nor FMA contraction can move a bit.  At p = 0.1 /
0.25 the set of zeros must be exactly the model's dropped set (the pre-dropout values are asserted nonzero first).  States with
high words in seed and offset, sites up to 2^32 - 1 and one element (philox_ref.WITNESS) whose draw lies between the fp32
threshold of p = 0.1 and the float64 one are part of every family.

MODEL_MUTATION is the reviewer's switch: set to any name of philox_ref.MUTATIONS, (a), (b), (d) and (e) fail (and so does (c))."""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import gemm_ref as G
import philox_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = G.NAN
MODEL_MUTATION = None

OFF_HI = 0x0000000300000007
STATES = [(0, 0), (1234, 1), (0x0123456789abcdef, OFF_HI), (2 ** 64 - 1, 2 ** 64 - 1)]
SITES = [0, 7, 2 ** 31, 2 ** 32 - 1]                          # the ctypes binding (c_uint) takes all of them
PS = [0.0, 2.0 ** -24, 0.1, 0.25, 0.5, 0.9, 1 - 2.0 ** -24]
NS = [1, 3, 4, 5, 255, 256, 257, 524288, 524289, 2 * 524288 + 5]      # grid cap 2048 x 256: the last two run the stride loop
W_STATE, W_SITE, W_IDX = R.WITNESS[:2], R.WITNESS[2], R.WITNESS[3]
ONES = (2 ** 64 - 1, 2 ** 64 - 1)
D = 384


@pytest.fixture(scope="module")
def ops():
    from sais_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from sais_amd import _lib
    return _lib


def nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def eq(got, ref64):
    return torch.equal(got.double(), ref64)


def _s64(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def rng(state):
    """the state tensor of (seed, offset) in [0, 2^64): the same bits as int64"""
    return torch.tensor([_s64(state[0]), _s64(state[1])], dtype=torch.int64, device=DEV)


@functools.lru_cache(maxsize=8)
def model_draws(state, site, n):
    """draws of elements 0 .. n - 1: computed once per (state, site), shared by every p; never written to"""
    r = R.draws(state[0], state[1], site, np.arange(n, dtype=np.uint64), mutate=MODEL_MUTATION)
    r.setflags(write=False)
    return r


def model_keep(state, site, n, p):
    return R.keep_draws(model_draws(state, site, n), p, mutate=MODEL_MUTATION)


def keep_dev(state, site, shape, p, nmax=None):
    n = int(np.prod(shape))
    return torch.from_numpy(model_keep(state, site, nmax or n, p)[:n].reshape(shape)).to(DEV)


# ------------------------------------------------------------------------------------------------ a. stand-alone kernels
@pytest.mark.parametrize("state", STATES, ids=["zero", "small", "high_words", "all_ones"])
def test_mask_is_the_model_bit_for_bit(ops, state):
    st = rng(state)
    for site in SITES:
        r = model_draws(state, site, NS[-1])
        for p in PS:
            want = R.keep_draws(r, p, mutate=MODEL_MUTATION).astype(np.uint8)
            for n in NS:
                got = ops.dropout_mask(n, p, st, site, DEV).cpu().numpy()
                assert np.array_equal(got, want[:n]), (site, p, n, int((got != want[:n]).sum()))
    assert st.tolist() == [_s64(state[0]), _s64(state[1])]                    # drawing does not advance the state


def test_mask_threshold_witness_and_buffer_tail(ops, L):
    """the recorded element whose draw lies between the fp32 and the float64 threshold of p = 0.1 is dropped; the n bytes of
    the mask are written and nothing behind them"""
    st = rng(W_STATE)
    n = W_IDX + 1
    got = ops.dropout_mask(n, R.WITNESS_P, st, W_SITE, DEV).cpu().numpy()
    want = model_keep(W_STATE, W_SITE, 264 * D, R.WITNESS_P)
    assert np.array_equal(got, want[:n].astype(np.uint8)) and got[W_IDX] == 0
    want = model_keep(W_STATE, W_SITE, 524289, 0.5).astype(np.uint8)
    for n in (1, 5, 257, 524289):
        buf = torch.full((n + 64,), G.U8_SENTINEL, dtype=torch.uint8, device=DEV)
        L.call("sais_dropout_mask", ctypes.c_void_p(buf.data_ptr()), n, 0.5, ctypes.c_void_p(st.data_ptr()), W_SITE,
               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert np.array_equal(buf[:n].cpu().numpy(), want[:n]), n
        assert bool((buf[n:] == G.U8_SENTINEL).all()), n


def _exact_threshold(p32):
    """floor(p * 2^32) clamped, in exact rational arithmetic (p an fp32 number): independent of philox_ref.threshold"""
    return min(int(Fraction(float(p32)) * 2 ** 32), R.THR_MAX)


def test_mask_direct_known_answer_by_bisection(ops):
    """state (0, 0), site 0, elements 0 .. 3: the largest fp32 p that keeps an element and its successor bracket the draw.
    The brackets must hold the four words of the first Random123 vector and be as narrow as fp32 p allows — the kernel alone
    against the published numbers, no model in between."""
    words = (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    st = rng((0, 0))
    as_p = lambda bits: np.array([bits], dtype=np.uint32).view(np.float32)[0]
    top = int(np.array([np.nextafter(np.float32(1), np.float32(0))], dtype=np.float32).view(np.uint32)[0])
    launches = 0
    for e in range(4):
        lo, hi = 0, top                                                       # bit patterns of positive floats are ordered
        assert int(ops.dropout_mask(4, float(as_p(lo)), st, 0, DEV)[e]) == 1  # p = 0 keeps
        assert int(ops.dropout_mask(4, float(as_p(hi)), st, 0, DEV)[e]) == 0  # every word is below 2^32 - 256
        while hi - lo > 1:
            mid = (lo + hi) // 2
            kept = int(ops.dropout_mask(4, float(as_p(mid)), st, 0, DEV)[e])
            launches += 1
            lo, hi = (mid, hi) if kept else (lo, mid)
        a, b = _exact_threshold(as_p(lo)), _exact_threshold(as_p(hi))         # kept at a: draw >= a; dropped at b: draw < b
        assert a <= words[e] < b, (e, hex(a), hex(b))
        assert b - a <= 256, (e, b - a)
    assert launches <= 4 * 32


def test_rng_advance_carries_into_the_key_word(ops):
    n, p = 4099, 0.5
    st = rng((1234, 2 ** 32 - 1))
    before = ops.dropout_mask(n, p, st, 7, DEV).cpu().numpy()
    assert np.array_equal(before, model_keep((1234, 2 ** 32 - 1), 7, n, p).astype(np.uint8))
    ops.rng_advance(st)
    assert st.tolist() == [1234, 2 ** 32]
    after = ops.dropout_mask(n, p, st, 7, DEV).cpu().numpy()
    assert np.array_equal(after, model_keep((1234, 2 ** 32), 7, n, p).astype(np.uint8))
    assert not np.array_equal(after, model_keep((1234, 0), 7, n, p).astype(np.uint8))        # offset hi is part of the key
    st = rng(ONES)                                                            # 2^64 - 1 wraps to offset 0
    ops.rng_advance(st)
    assert st.tolist() == [-1, 0]
    assert np.array_equal(ops.dropout_mask(n, p, st, 7, DEV).cpu().numpy(), model_keep((2 ** 64 - 1, 0), 7, n, p).astype(np.uint8))


def test_mask_element_index_past_32_bits(ops):
    """one mask of 2^32 + 4096 bytes: elements on both sides of 2^32 (idx / 4 stays below 2^32: that carry needs 16 GiB)"""
    state, site, p = STATES[2], 7, 0.5
    n, first = 2 ** 32 + 4096, 2 ** 32 - 2048
    m = ops.dropout_mask(n, p, rng(state), site, DEV)
    tail, head = m[first:].cpu().numpy(), m[:4096].cpu().numpy()
    del m
    torch.cuda.empty_cache()
    idx = np.arange(first, n, dtype=np.uint64)
    want = R.keep(state[0], state[1], site, idx, p, mutate=MODEL_MUTATION).astype(np.uint8)
    assert np.array_equal(tail, want)
    assert np.array_equal(head, model_keep(state, site, 4096, p).astype(np.uint8))
    assert not np.array_equal(tail[2048:], head)                              # element 2^32 + i is not element i


@pytest.mark.parametrize("p", [0.5, 0.1])
def test_dropout_f32_is_the_model_mask_times_inv(ops, p):
    state, site = STATES[2], 2 ** 31
    st, inv = rng(state), float(R.inv(p))
    for n in (1, 5, 257, 524289):
        g = torch.Generator().manual_seed(n)
        x, r = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
        m = keep_dev(state, site, (n,), p, nmax=524289)
        v = torch.where(m, x * inv, torch.zeros_like(x))                      # torch fp32 arithmetic, as test_dropout_gpu.py has it
        out = ops.dropout(x, p, st, site, resid=r, out=nan(n))
        assert torch.equal(out, r + v), n
        assert torch.equal(ops.dropout(x, p, st, site, out=nan(n)), v), n
        y = x.clone()
        assert ops.dropout(y, p, st, site, resid=r) is y and torch.equal(y, r + v), n        # in place
        y = x.clone()
        ops.dropout(y, p, st, site)
        assert torch.equal(y, v), n


# ------------------------------------------------------------------------------------------------ b, c: GEMM epilogues
GEMM_DRAWS = 264 * 2048                                        # element m N + n of the site: a prefix of this range


@functools.lru_cache(maxsize=4)
def _gemm_case(M, N, K):
    """x3 operands, a positive integer bias above max |ref| (so every pre-dropout value is positive), positive aux, small-integer
    residual.  pre = ref + bias in fp64; asserted exact and positive on the reference."""
    a, w = (t.to(DEV) for t in G.x3_pair(M, N, K))
    assert G.x3_condition(a, w)
    ref = G.x3_ref(a, w)
    assert G.x3_ref_condition(ref)
    bias = (float(int(ref.abs().max())) + 1 + torch.arange(N) % 5).float().to(DEV)
    pre = ref + bias.double()
    assert float(pre.min()) > 0 and G.f32_exact(4 * pre)
    aux = 1 + G.tern_resid(M, N).abs().to(DEV)
    resid = G.tern_resid(M, N, seed=9).to(DEV)
    assert float(aux.min()) > 0 and G.f32_exact(4 * pre + resid.double())
    return a, w, bias, pre, aux, resid


def _check_dropped(tag, out, pre, keep, p, K, base=None):
    """out = base + where(keep, pre * inv, 0): bit for bit where inv is a power of two, else the zero pattern exactly and the
    kept values under the 2e-5 sqrt(K) bar of the bf16x3 GEMMs"""
    inv = float(R.inv(p))
    zero = torch.zeros_like(pre)
    want = torch.where(keep, pre * inv, zero) + (zero if base is None else base.double())
    if p in (0.5, 0.75):
        assert inv in (2.0, 4.0) and eq(out, want), (tag, p)
    else:
        dropped = out == (0 if base is None else base)
        assert torch.equal(dropped, ~keep), (tag, p, int((dropped != ~keep).sum()))
        assert float((out.double() - want).abs().max()) <= 2e-5 * K ** 0.5, (tag, p)


GEMM_STATES = [(W_STATE, W_SITE), (ONES, 2 ** 32 - 1)]         # the first holds philox_ref.WITNESS at p = 0.1


@pytest.mark.parametrize("N", [64, 384, 2048])
def test_tgemm_epilogue_dropout_is_the_model(ops, L, N):
    K = 64
    for M in (1, 63, 64, 65, 264):
        a, w, bias, pre, aux, _ = _gemm_case(M, N, K)
        for state, site in GEMM_STATES:
            st = rng(state)
            for p in (0.5, 0.75, 0.1, 0.25):
                keep = keep_dev(state, site, (M, N), p, nmax=GEMM_DRAWS)
                if state == W_STATE and p == R.WITNESS_P and M * N > W_IDX:
                    assert not bool(keep.view(-1)[W_IDX])
                relu = ops.tgemm(a, w, L.TG_BIAS_RELU, nan(M, N), bias=bias, drop=(p, st, site))
                _check_dropped(("tg relu", M), relu, pre, keep, p, K)
                drelu = ops.tgemm(a, w, L.TG_DRELU, nan(M, N), bias=bias, aux=aux, drop=(p, st, site))
                _check_dropped(("tg drelu", M), drelu, pre, keep, p, K)
                assert torch.equal(relu == 0, drelu == 0)                     # the backward zeroes what the forward zeroed


def test_tgemm_dropout_strided_output(ops, L):
    """ldo > N: the mask element is m N + n, not m ldo + n, and the padding keeps its NaN"""
    M, N, K = 65, 384, 64
    a, w, bias, pre, aux, _ = _gemm_case(M, N, K)
    (state, site), p = GEMM_STATES[0], 0.5
    keep = keep_dev(state, site, (M, N), p, nmax=GEMM_DRAWS)
    for epi, kw in ((L.TG_BIAS_RELU, {}), (L.TG_DRELU, dict(aux=G.padded(aux, 12, 8)[0]))):
        out, buf = G.padded(nan(M, N), 8, 4)
        assert out.stride(0) == N + 8
        ops.tgemm(a, w, epi, out, bias=bias, drop=(p, rng(state), site), **kw)
        _check_dropped("tg strided", out, pre, keep, p, K)
        G.untouched(buf, out)
    wrong = keep_dev(state, site, (M, N + 8), p, nmax=GEMM_DRAWS)[:, :N]     # what indexing by ldo would give
    assert not torch.equal(wrong, keep)


F32_CASES = [(264, 2048, 64)] + [(M, 384, 384) for M in (1, 127, 129, 264)]


@pytest.mark.parametrize("M,N,K", F32_CASES)
def test_gemm_nt_f32_epilogue_dropout_is_the_model(ops, L, M, N, K):
    """both arms: 48 tiles run the direct epilogue; N = K = 384 is split by 6 and splitk_reduce_kernel applies the mask"""
    ks = G.f32_default_ks(M, N, K)
    assert ks == (1 if N == 2048 else 6)
    a, w, bias, pre, aux, resid = _gemm_case(M, N, K)
    for state, site in GEMM_STATES:
        st = rng(state)
        for p in (0.5, 0.75, 0.1, 0.25):
            keep = keep_dev(state, site, (M, N), p, nmax=GEMM_DRAWS)
            if state == W_STATE and p == R.WITNESS_P and M * N > W_IDX:
                assert not bool(keep.view(-1)[W_IDX])
            drop = (p, st, site)
            relu = ops.gemm_nt_f32(a, w, L.EPI_BIAS_RELU_F32, nan(M, N), bias=bias, drop=drop)
            _check_dropped(("f32 relu", ks), relu, pre, keep, p, K)
            drelu = ops.gemm_nt_f32(a, w, L.EPI_DRELU_F32, nan(M, N), bias=bias, aux=aux, drop=drop)
            _check_dropped(("f32 drelu", ks), drelu, pre, keep, p, K)
            assert torch.equal(relu == 0, drelu == 0)
            out = ops.gemm_nt_f32(a, w, L.EPI_BIAS_RESID_F32, nan(M, N), bias=bias, aux=resid, drop=drop)
            _check_dropped(("f32 resid", ks), out, pre, keep, p, K, base=resid)


def test_gemm_nt_f32_dropout_rejections(ops, L):
    """each is refused before any launch: the output keeps its NaN"""
    M, N, K = 129, 384, 384
    a, w, bias, _, aux, _ = _gemm_case(M, N, K)
    st, out = rng((1, 0)), nan(M, N)
    with pytest.raises(L.SaisHipError):                                       # the plain bias epilogue has no dropout
        ops.gemm_nt_f32(a, w, L.EPI_BIAS_F32, out, bias=bias, drop=(0.5, st, 0))
    for p in (1.0, 1.5):
        with pytest.raises(L.SaisHipError):
            ops.gemm_nt_f32(a, w, L.EPI_BIAS_RELU_F32, out, bias=bias, drop=(p, st, 0))
    with pytest.raises(L.SaisHipError):                                       # p > 0 without a state
        ops.gemm_nt_f32(a, w, L.EPI_BIAS_RESID_F32, out, bias=bias, aux=aux, drop=(0.5, None, 0))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ d. row kernels (drop12)
TLN_ROWS = [1, 7, 8, 9, 264, 8192 + 8 + 3]                    # the backward's grid is capped at 1024 x 8 rows
TLN_CASES = sorted({(rows, 3) for rows in TLN_ROWS} | {(rows, ns) for rows in (9, 264) for ns in (1, 3, 4, 5)})
TLN_DRAWS = TLN_ROWS[-1] * D
TLN_STATES = {0.5: (ONES, 2 ** 32 - 1), 0.1: (W_STATE, W_SITE)}


@functools.lru_cache(maxsize=1)
def _tln_data():
    """small integers: every sum is exact in any order.  slabs in [-3, 3], bias in [20, 24]: sum + bias >= 5 for nslab <= 5"""
    rows, g = TLN_ROWS[-1], torch.Generator().manual_seed(41)
    slabs = torch.randint(-3, 4, (5, rows, D), generator=g).float().to(DEV)
    bias = (20 + torch.arange(D) % 5).float().to(DEV)
    resid = torch.randint(-4, 5, (rows, D), generator=g).float().to(DEV)
    add = torch.randint(-4, 5, (rows, D), generator=g).float().to(DEV)
    x = torch.randn(rows, D, generator=g).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV), (0.05 * torch.randn(D, generator=g)).to(DEV)
    mean = x.mean(1)
    rstd = 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)
    return slabs, bias, resid, add, x, gamma, beta, mean, rstd


@pytest.mark.parametrize("rows,nslab", TLN_CASES)
def test_temporal_ln_fwd_dropout_is_the_model(ops, rows, nslab):
    slabs, bias, resid, _, _, gamma, beta, _, _ = _tln_data()
    sl, rs = slabs[:nslab, :rows].contiguous(), resid[:rows]
    pre = sl.double().sum(0) + bias.double()
    assert float(pre.min()) >= 5
    for p, (state, site) in TLN_STATES.items():
        keep = keep_dev(state, site, (rows, D), p, nmax=TLN_DRAWS)
        if p == R.WITNESS_P and rows * D > W_IDX:
            assert not bool(keep.view(-1)[W_IDX])
        y, z = nan(rows, D), nan(rows, D)
        ops.temporal_ln_fwd(sl, bias, rs, gamma, beta, 1e-5, z, y=y, drop=(p, rng(state), site))
        assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(y).all())
        if p == 0.5:
            assert eq(y, rs.double() + torch.where(keep, 2 * pre, torch.zeros_like(pre))), (rows, nslab)
        else:
            assert torch.equal((y - rs) == 0, ~keep), (rows, nslab)


@pytest.mark.parametrize("rows,nslab", TLN_CASES)
def test_temporal_ln_bwd_dropout_is_the_model(ops, rows, nslab):
    slabs, _, _, add, x, gamma, _, mean, rstd = _tln_data()
    sl = slabs[:nslab, :rows].contiguous()
    args = (sl, add[:rows], x[:rows], mean[:rows], rstd[:rows], gamma)
    plain = nan(rows, D)
    ops.temporal_ln_bwd(*args, plain)
    assert bool(torch.isfinite(plain).all()) and bool((plain != 0).all())     # the pre-dropout values
    for p, (state, site) in TLN_STATES.items():
        keep = keep_dev(state, site, (rows, D), p, nmax=TLN_DRAWS)
        dx, dxd = nan(rows, D), nan(rows, D)
        ops.temporal_ln_bwd(*args, dx, dx_drop=dxd, drop=(p, rng(state), site))
        assert torch.equal(dx, plain), (rows, nslab)                          # dx does not know about dx_drop
        if p == 0.5:
            assert torch.equal(dxd, torch.where(keep, 2 * dx, torch.zeros_like(dx))), (rows, nslab)
        else:
            assert torch.equal(dxd == 0, ~keep), (rows, nslab)
            kept = torch.where(keep, dx.double() * float(R.inv(p)), torch.zeros_like(dx, dtype=torch.float64))
            assert float((dxd.double() - kept).abs().max()) <= 2.0 ** -23 * float(dx.abs().max()) * 1.2      # one fp32 rounding


# ------------------------------------------------------------------------------------------------ e. DropPath
DP_RATES = np.concatenate([np.repeat(np.linspace(0, 0.1, 11), 2), [0.0, 0.5]])      # the ViT's linspace, two branches per block
DP_STATES = [R.WITNESS_DROPPATH[:2], ONES]


def _droppath_model(state, site0, samples, rows_per_sample):
    out = np.empty((len(DP_RATES), samples, rows_per_sample), dtype=np.float32)
    for j, rate in enumerate(DP_RATES):
        k = R.keep(state[0], state[1], site0 + j, np.arange(samples), rate, mutate=MODEL_MUTATION)
        out[j] = (np.where(k, R.inv(rate), np.float32(0)) if rate > 0 else np.ones(samples, dtype=np.float32))[:, None]
    return out.reshape(len(DP_RATES), samples * rows_per_sample)


@pytest.mark.parametrize("site0", [0, 5])
def test_droppath_scales_are_the_model(ops, site0):
    assert len(DP_RATES) == 24 and DP_RATES[20] == R.WITNESS_P
    rates = torch.from_numpy(DP_RATES.astype(np.float32)).to(DEV)
    for state in DP_STATES:
        st = rng(state)
        for samples in (1, 3, 4, 5, 257):
            for rps in (1, 37, 197):                                          # 24 x 257 x 197 is past one grid sweep
                got = ops.droppath_scales(rates, samples, rps, st, site0=site0).cpu().numpy()
                want = _droppath_model(state, site0, samples, rps)
                assert got.shape == want.shape
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (state, samples, rps)
                per = got.reshape(24, samples, rps)
                assert (per == per[:, :, :1]).all()                           # all rows of a sample are equal
                assert (got[:2] == 1).all() and (got[22] == 1).all()          # rate 0: exactly 1.0
                assert set(np.unique(got[23])) <= {0.0, 2.0}
    if site0 == 0:                                                            # the recorded sample between the two thresholds
        seed, offset, site, idx = R.WITNESS_DROPPATH
        got = ops.droppath_scales(rates, 257, 1, rng((seed, offset)), site0=0)
        assert float(got[site, idx]) == 0.0
