"""Exact data, strided views and case lists for the NT GEMM edge tests (no GPU code; imported by test_gemm_ref_host.py and
test_gemm_edges_gpu.py).

Two recipes make a GEMM output independent of the summation order, so a kernel is compared bit for bit with fp64:
  tern   A, W and bias in {-1, 0, 1}: every partial sum is an integer below 2^24, an f32 output equals the fp64 reference in
         any order, and a bf16 output is exact when the reference is representable in bf16 (integers up to 256, their
         halves and doubles for the MUL epilogue).  The condition is asserted on the reference alone (bf16_exact).
  x3     f32 operands s * (h + j 2^-10), s = +-1, h in {1, 2, 3}, j in {0 .. 3}: split8 (csrc/common.hpp) gives hi = h (the
         integer part) and lo = j 2^-10 exactly, and the three products hi hi + hi lo + lo hi of the bf16x3 kernels are
         multiples of 2^-10 below 2^10: every partial sum has at most 20 significant bits.  The expected value is that
         three-term sum in fp64 (x3_ref), NOT a @ w: the dropped lo lo term is a multiple of 2^-20 and shows in fp64.
The launcher rules restated here (w8p_tiles, row_waves, row_rows_per_tile) only CHOOSE shapes; no test asks which kernel ran.
"""
import torch

NAN = float("nan")
U8_SENTINEL = 0xA5
BF16_MAX_INT = 256              # every integer up to 2^8 is a bf16

# ------------------------------------------------------------------------------------------------ launcher rules
BM = BN = 128
BK = 64
W8P_MIN_M = 8192
W8P_GRID = 512


def w8p_tiles(M, N):
    """nt_tiles (csrc/gemm_nt_tile.hpp): 128 x 128 output tiles; the eight-wave kernel runs on min(tiles, 512) workgroups
    (csrc/gemm.hip, sais_gemm_nt: `big = M >= 8192`, `nt_grid = 512`)"""
    return ((M + BM - 1) // BM) * (N // BN)


def takes_row_kernel(M, N):
    """csrc/gemm.hip, sais_gemm_nt: `big && N == 384` with EPI_BIAS_BF16, or EPI_BIAS_RESID_F32 without out2"""
    return M >= W8P_MIN_M and N == 384


def row_waves(M):
    """csrc/gemm_row.hip, use_eight_waves: `M >= 256 * 112`"""
    return 8 if M >= 256 * 112 else 4


def row_rows_per_tile(M):
    """csrc/gemm_row.hip, rows_per_tile<NW>: cap = 112 (NW / 4), slots = 512 | 256, `rows < cap / 2 + 8 -> cap`"""
    nw = row_waves(M)
    cap, slots = 112 * (nw // 4), 512 if nw == 4 else 256
    rounds = (M + slots * cap - 1) // (slots * cap)
    rows = (M + slots * rounds - 1) // (slots * rounds)
    return cap if rows < cap // 2 + 8 else rows


def f32_default_ks(M, N, K):
    """the K split sais_amd/ops.py gemm_nt_f32 picks: below 48 tiles the first of (8, 6, 4, 3, 2) that divides K / 64 and keeps
    tiles x split <= 256.  test_f32_bf16x3_small_m_three_terms_exactly asserts which cases this leaves for the forced split."""
    tiles, nk = (N // 128) * ((M + 127) // 128), K // 64
    if tiles < 48:
        for cand in (8, 6, 4, 3, 2):
            if nk % cand == 0 and tiles * cand <= 256:
                return cand
    return 1


# ------------------------------------------------------------------------------------------------ the GPU case lists
W8P_DEPTH_K = [64, 128, 192, 256, 320, 448, 768, 1536]
W8P_DEPTH_M = [8320, 8377]
W8P_DEPTH = [(M, 1024, K) for K in W8P_DEPTH_K for M in W8P_DEPTH_M]
W8P_RANDOM = [(8377, 1024, K) for K in (64, 192, 1536)]
PATCH = [(196 * 43, 384, 768), (196 * 88, 384, 768)]
PREFETCH = [(9529, N, 384) for N in (896, 1024, 1408, 2048, 2176)]
NTN1 = [(65665, 128, K) for K in (64, 384)]
BOUNDARY = [(8192, 384, 384), (8192, 512, 384), (28672, 384, 384)]          # each runs at M and at M - 1
ROW_M = [8192 + 57, 28672, 30465, 57344, 57345]
ROW_PLAIN = [(M, 384, K) for M in ROW_M for K in ((64, 384) if M >= 57344 else (64, 128, 192, 384, 1536))]
LN_M = [1, 111, 112, 113] + ROW_M
LN_K = [64, 128, 192]
LN_CASES = [(M, 384, K) for M in LN_M for K in LN_K]
LN_PERIOD = [(197 * 43, 384, 128), (197 * 146, 384, 128)]                   # dres_period = 197: four-wave and eight-wave tile
SMALL_NT = [(M, N, K) for M in (1, 63, 127, 128, 129) for N in (128, 384) for K in (64, 1536)]
SMALL_F32 = [(M, 384, K) for M in (1, 127, 129, 264) for K in (64, 384, 2048)]
TGEMM_KS = [(64, 1), (128, 2), (192, 1), (320, 1), (384, 2), (2048, 4)]
TGEMM = [(M, N, K, ns) for (K, ns) in TGEMM_KS for N in (64, 384) for M in (1, 63, 64, 65, 264)]
# strided operands: entry -> (M, N, K)
STRIDED = {"nt_small": (129, 256, 192), "nt_large": (8377, 512, 192), "row_plain": (8192 + 57, 384, 192),
           "ln_fwd": (8192 + 57, 384, 128), "ln_bwd": (8192 + 57, 384, 128), "f32": (129, 128, 192), "tgemm": (65, 128, 192)}
OVERALLOC_ROWS = 128

TERN_CASES = sorted(set(W8P_DEPTH + PATCH + PREFETCH + NTN1 + BOUNDARY + [(M - 1, N, K) for M, N, K in BOUNDARY] + ROW_PLAIN +
                        LN_CASES + SMALL_NT + [STRIDED[k] for k in ("nt_small", "nt_large", "row_plain", "ln_fwd")]))
X3_CASES = sorted(set(SMALL_F32 + [c[:3] for c in TGEMM] + [STRIDED["f32"], STRIDED["tgemm"]]))


# ------------------------------------------------------------------------------------------------ tern
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def tern(M, N, K, seed=0):
    """A [M,K], W [N,K] bf16 and bias f32 [N], all in {-1, 0, 1}.  The seed depends on (N, K) only and A is drawn row by row:
    the first rows of a larger M are the rows of a smaller one."""
    g = _gen(1000003 * N + 7 * K + seed)
    w = torch.randint(-1, 2, (N, K), generator=g).to(torch.bfloat16)
    bias = torch.randint(-1, 2, (N,), generator=g).float()
    a = torch.randint(-1, 2, (M, K), generator=g).to(torch.bfloat16)
    return a, w, bias


def tern_resid(M, N, seed=1):
    """residual / position rows: small integers"""
    return torch.randint(-4, 5, (M, N), generator=_gen(77 * N + seed)).float()


def tern_aux(M, N, seed=2):
    """aux of MUL / DRELU: {0, +-0.5, +-1, +-2}"""
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    return vals[torch.randint(0, 7, (M, N), generator=_gen(55 * N + seed))].to(torch.bfloat16)


def tern_rowscale(M, seed=3):
    return torch.randint(0, 3, (M,), generator=_gen(M + seed)).float()


def mm64(a, w):
    return a.double() @ w.double().t()


def bf16_exact(ref):
    """the condition of a bf16 comparison: the fp64 reference is a bf16 number"""
    return bool(torch.equal(ref.to(torch.bfloat16).double(), ref))


def f32_exact(ref):
    return bool(torch.equal(ref.float().double(), ref)) and float(ref.abs().max()) < 2 ** 24


# ------------------------------------------------------------------------------------------------ x3
def x3(rows, K, seed):
    g = _gen(seed)
    s = torch.randint(0, 2, (rows, K), generator=g).float() * 2 - 1
    h = torch.randint(1, 4, (rows, K), generator=g).float()
    j = torch.randint(0, 4, (rows, K), generator=g).float()
    return s * (h + j * 2.0 ** -10)


def x3_pair(M, N, K):
    return x3(M, K, 31 * K + 5), x3(N, K, 1009 * N + K + 6)


def split8(x):
    """csrc/common.hpp split8 in torch: hi = bf16(x), lo = bf16(x - hi), as f32"""
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


def x3_terms(a, w):
    ah, al = split8(a)
    wh, wl = split8(w)
    return [(ah, wh), (ah, wl), (al, wh)], (al, wl)


def x3_ref(a, w, k0=0, k1=None):
    """what the bf16x3 kernels compute over columns [k0, k1): ah wh + ah wl + al wh, in fp64"""
    terms, _ = x3_terms(a[:, k0:k1], w[:, k0:k1])
    return sum(mm64(p, q) for p, q in terms)


def x3_condition(a, w):
    """hi + lo == x, hi is the integer part, and the three-term sum fits f32 with room: multiples of 2^-10 below 2^10"""
    ok = True
    for x in (a, w):
        hi, lo = split8(x)
        ok = ok and torch.equal(hi + lo, x) and torch.equal(hi, torch.trunc(x)) and float(lo.abs().max()) <= 3 * 2.0 ** -10
    return bool(ok)


def x3_ref_condition(ref):
    return float(ref.abs().max()) < 1024 and bool(torch.equal(torch.round(ref * 1024), ref * 1024))


# ------------------------------------------------------------------------------------------------ strided views
def _sentinel(dtype):
    return U8_SENTINEL if dtype == torch.uint8 else NAN


def padded(t, pad, off, rows_extra=0):
    """A view equal to `t` (2-D, or 3-D slabs) inside a wider sentinel-filled buffer on t's device: row stride = width + pad,
    first column `off` (off <= pad), `rows_extra` more rows behind the last.  Returns (view, buffer)."""
    assert 0 < off <= pad and t.dim() in (2, 3)
    shape = list(t.shape)
    shape[-1] += pad
    shape[-2] += rows_extra
    buf = torch.full(shape, _sentinel(t.dtype), dtype=t.dtype, device=t.device)
    view = buf[..., :t.shape[-2], off:off + t.shape[-1]]
    view.copy_(t)
    return view, buf


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def untouched(buf, view):
    """every element of `buf` outside `view` still holds the sentinel, bit for bit"""
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(False)
    want = torch.full((1,), _sentinel(buf.dtype), dtype=buf.dtype, device=buf.device)
    bad = (_bits(buf) != _bits(want)) & mask
    assert not bool(bad.any()), f"{int(bad.sum())} elements outside the view were written, first at {bad.nonzero()[0].tolist()}"
    assert int(mask.sum()) == buf.numel() - view.numel()


# ------------------------------------------------------------------------------------------------ the loop, restated
MUTATIONS = ("drop_kstep", "stale_slot", "ld_ignored", "tail_rows_stored", "drop_lo_term", "four_terms")


def ring_gemm(a, w, out, M, slots=3, tile_m=128, mutate=None, split=False):
    """out[:M] = a[:M] . w^T, K in steps of 64 through an n-slot ring of A chunks, in fp64 (f32 operands split as the bf16x3
    kernels do when `split`).  `a`, `w` are views (row stride free), `out` a view into a sentinel-filled buffer.  The mutations
    are the errors the GPU list has to notice; this models what is computed, not when."""
    assert mutate is None or mutate in MUTATIONS
    N, K = w.shape
    nk = K // BK
    if mutate == "ld_ignored":                                   # row stride taken as the width
        a = a.as_strided((a.shape[0], K), (K, 1), a.storage_offset())
    ops = [(a, w)]
    if split:
        ops, lolo = x3_terms(a, w)
        if mutate == "drop_lo_term":
            ops = ops[:2]
        if mutate == "four_terms":
            ops = ops + [lolo]
    acc = torch.zeros(a.shape[0], N, dtype=torch.float64)
    for pa, pw in ops:
        ring = [torch.zeros(a.shape[0], BK, dtype=torch.float64) for _ in range(slots)]
        for kt in range(nk):
            if mutate == "drop_kstep" and kt == nk - 1:
                continue
            if not (mutate == "stale_slot" and kt == nk - 1):    # the last refill is lost: step kt reads the chunk of kt - slots
                ring[kt % slots] = pa[:, BK * kt:BK * (kt + 1)].double()
            acc += ring[kt % slots] @ pw[:, BK * kt:BK * (kt + 1)].double().t()
    rows = M
    if mutate == "tail_rows_stored":                             # a full tile written at a ragged M (rows past M: the clamped row)
        rows = min((M + tile_m - 1) // tile_m * tile_m, M + OVERALLOC_ROWS)       # `out` lies in an over-allocated buffer
        acc = torch.cat([acc[:M], acc[M - 1:M].expand(rows - M, N)])
        out = out.as_strided((rows, N), out.stride(), out.storage_offset())
    out.copy_(acc[:rows].to(out.dtype))
    return acc[:M]
