"""The exact-data recipes of tests/gemm_ref.py hold for every shape test_gemm_edges_gpu.py runs, and that list would notice the
errors a K loop over a slot ring can make (CPU only).  For each recipe the condition is a property of the fp64 reference alone;
for each deliberate error put into gemm_ref.ring_gemm a NAMED case of the GPU lists fails the check that case uses, while the
unmutated loop passes it."""
import pytest
import torch

import gemm_ref as G

MAX_ROWS = 4096


def _by_nk(cases):
    out = {}
    for c in cases:
        M, N, K = c[:3]
        out[(N, K)] = max(out.get((N, K), 0), M)
    return sorted(out.items())


@pytest.mark.parametrize("nk,M", _by_nk(G.TERN_CASES), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tern_condition(nk, M):
    """tern: |A.W^T + bias| <= 256 on (at most) the first 4096 rows of the largest M of every (N, K), so every bf16 output of the
    list is exact: the plain, RELU, residual (+ small integers), MUL / DRELU (x {0, +-0.5, +-1, +-2}) forms; f32 outputs with
    a row scale in {0, 1, 2} stay integers below 2^24"""
    N, K = nk
    rows = min(M, MAX_ROWS)
    a, w, bias = G.tern(rows, N, K)
    assert set(a.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}
    acc = G.mm64(a, w)
    ref = acc + bias.double()
    worst = float(ref.abs().max())
    print(f"N {N} K {K} rows {rows}: max |ref| {worst:.0f}")
    assert worst <= G.BF16_MAX_INT and K < 2 ** 24
    resid, aux, rs = G.tern_resid(rows, N).double(), G.tern_aux(rows, N).double(), G.tern_rowscale(rows).double()
    assert G.bf16_exact(ref) and G.bf16_exact(ref.relu()) and G.bf16_exact(ref + resid)
    assert G.bf16_exact(acc * aux) and G.bf16_exact(acc * (aux > 0))
    assert G.f32_exact(resid + rs[:, None] * ref)
    assert set(aux.unique().tolist()) == {0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0} and set(rs.unique().tolist()) <= {0.0, 1.0, 2.0}


def test_tern_rows_of_a_smaller_m_are_the_first_rows_of_a_larger_one():
    a1, w1, b1 = G.tern(8191, 384, 384)
    a2, w2, b2 = G.tern(8192, 384, 384)
    assert torch.equal(a2[:8191], a1) and torch.equal(w1, w2) and torch.equal(b1, b2)


@pytest.mark.parametrize("nk,M", _by_nk(G.X3_CASES), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_x3_condition_and_order_independence(nk, M):
    """x3: the split is exact with hi the integer part; the three-term sum is a multiple of 2^-10 below 2^10; an f32 chain over
    the 64-wide K chunks equals the fp64 value bit for bit in ascending, descending and a shuffled chunk order (with the term
    order rotated per chunk); and the value is NOT the rounded full product on most outputs"""
    N, K = nk
    a, w = G.x3_pair(min(M, MAX_ROWS), N, K)
    assert G.x3_condition(a, w)
    ref = G.x3_ref(a, w)
    assert G.x3_ref_condition(ref) and G.f32_exact(ref)
    terms, _ = G.x3_terms(a, w)
    nkk = K // 64
    orders = [list(range(nkk)), list(range(nkk))[::-1], torch.randperm(nkk, generator=torch.Generator().manual_seed(K)).tolist()]
    for o, order in enumerate(orders):
        acc = torch.zeros(a.shape[0], N)
        for i, kt in enumerate(order):
            for t in range(3):
                p, q = terms[(t + o + i) % 3]
                acc = acc + p[:, 64 * kt:64 * kt + 64] @ q[:, 64 * kt:64 * kt + 64].t()
        assert torch.equal(acc.double(), ref), (N, K, o)
    full = G.mm64(a, w)
    differs = float((full.float().double() != ref).double().mean())
    print(f"N {N} K {K}: max |ref| {float(ref.abs().max()):.3f}, rounded a @ w differs on {100 * differs:.1f} % of the outputs")
    assert differs > 0.5 and not torch.equal(full, ref)


# mutation -> (the GPU list, the case, the check of that case)
CAUGHT_BY = {
    "drop_kstep": ("SMALL_NT", (129, 384, 1536), "equal"),
    "stale_slot": ("SMALL_NT", (129, 384, 1536), "equal"),
    "ld_ignored": ("STRIDED", G.STRIDED["nt_small"], "equal"),
    "tail_rows_stored": ("STRIDED", G.STRIDED["nt_large"], "untouched"),
    "drop_lo_term": ("SMALL_F32", (127, 384, 384), "equal"),
    "four_terms": ("SMALL_F32", (127, 384, 384), "equal"),
}


def _run(mutate):
    lst, (M, N, K), check = CAUGHT_BY[mutate]
    assert (M, N, K) in (G.STRIDED.values() if lst == "STRIDED" else getattr(G, lst))
    split = lst == "SMALL_F32"
    if split:
        a, w = G.x3_pair(M, N, K)
        ref = G.x3_ref(a, w)
    else:
        a, w, _ = G.tern(M, N, K)
        ref = G.mm64(a, w)
    a_v, _ = G.padded(a, 24, 8)
    w_v, _ = G.padded(w, 16, 8)
    out_v, out_buf = G.padded(torch.zeros(M, N, dtype=torch.float64), 8, 4, rows_extra=G.OVERALLOC_ROWS)
    out_buf.fill_(G.NAN)

    def verdict(m):
        out_buf.fill_(G.NAN)
        G.ring_gemm(a_v, w_v, out_v, M, mutate=m, split=split)
        if check == "equal":
            return torch.equal(out_v, ref)
        try:
            G.untouched(out_buf, out_v)
        except AssertionError:
            return False
        return torch.equal(out_v, ref)
    return verdict


@pytest.mark.parametrize("mutate", G.MUTATIONS)
def test_the_gpu_list_notices(mutate):
    """  drop_kstep / stale_slot   tern, K = 1536 at M = 129: 24 K-steps, the last one lost or read from the slot of step 20
      ld_ignored               the strided four-wave case: A with row stride K + 24
      tail_rows_stored         the over-allocated large-M strided case (8377 rows = 65 tiles + 57): rows 8377 .. 8447 written
      drop_lo_term, four_terms the bf16x3 case at M = 127, K = 384
    and the unmutated loop passes the same check on the same case."""
    verdict = _run(mutate)
    assert verdict(None)
    assert not verdict(mutate)


def test_helpers():
    t = torch.arange(12.0).view(3, 4)
    v, buf = G.padded(t, 8, 4, rows_extra=2)
    assert buf.shape == (5, 12) and v.stride() == (12, 1) and v.storage_offset() == 4 and torch.equal(v, t)
    G.untouched(buf, v)
    v.fill_(1.0)
    G.untouched(buf, v)
    for r, c in ((0, 3), (2, 8), (3, 4), (4, 11)):                          # left of, right of, below the view, the last element
        buf2 = buf.clone()
        buf2[r, c] = 0.0
        with pytest.raises(AssertionError):
            G.untouched(buf2, buf2[:3, 4:8])
    u8, b8 = G.padded(torch.zeros(2, 16, dtype=torch.uint8), 16, 16)
    G.untouched(b8, u8)
    b8[1, 0] = 0
    with pytest.raises(AssertionError):
        G.untouched(b8, u8)
    s, sb = G.padded(torch.zeros(2, 3, 4), 4, 4)                          # slabs: [nsplit, M, N + pad], slab stride M * ld
    assert s.stride() == (24, 8, 1)
    G.untouched(sb, s)


def test_launcher_rules():
    """the shapes the GPU tests name are on the side of each threshold they are meant for"""
    assert G.w8p_tiles(8320, 1024) == 520 and G.w8p_tiles(8377, 1024) == 528 and 8377 % 128 == 57
    assert [G.w8p_tiles(M, N) for M, N, _ in G.PATCH] == [66 * 3, 135 * 3]
    assert all(G.w8p_tiles(M, N) > G.W8P_GRID for M, N, _ in G.W8P_DEPTH + G.PREFETCH + G.NTN1)
    assert [N // 128 for _, N, _ in G.PREFETCH] == [7, 8, 11, 16, 17] and -(-128 // 11) * 11 > 128
    assert G.w8p_tiles(65665, 128) == 514
    assert not G.takes_row_kernel(8191, 384) and G.takes_row_kernel(8192, 384) and not G.takes_row_kernel(8192, 512)
    assert (G.row_waves(28671), G.row_waves(28672)) == (4, 8)
    assert [G.row_rows_per_tile(M) for M in G.ROW_M] == [112, 224, 120, 224, 224]
    assert G.row_rows_per_tile(30464) == 224 and 30465 % 120 == 105 <= 112       # 120: half 1 owns 8 rows; last tile in half 0
    assert -(-57344 // 224) == 256 and -(-57345 // 224) == 257                      # one tile into the second round
    assert [G.f32_default_ks(264, 384, K) for K in (64, 384, 2048)] == [1, 6, 8]
    assert all((K // 64) % ns == 0 for _, _, K, ns in G.TGEMM)
    assert sorted({(K // 64) // ns for _, _, K, ns in G.TGEMM}) == [1, 3, 5, 8]     # K-steps per split: odd 1, 3, 5 and even 8
