"""tests/stream_ref.py on the CPU: every reference against torch fp64 autograd or the oracle at one plain shape, every case
table's stated condition, and the teeth of the bars: deliberately wrong variants go through the assertions of
test_stream_edges_gpu.py and each has to fail."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as G
import stream_ref as S

D = S.D


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=S.gen(seed)) * scale


# ------------------------------------------------------------------------------------------------ references
def test_layernorm_references_equal_fp64_autograd():
    x, (gamma, beta) = S.ln_rows("plain", 13), S.ln_params()
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    ref = F.layer_norm(xd, (D,), gd, bd, S.f32(1e-6))
    y, mean, rstd = S.ln_fwd(x, gamma, beta, 1e-6)
    assert float((y - ref.detach()).abs().max()) < 1e-12
    dy, dres = rnd(13, D, seed=1), rnd(13, D, seed=2)
    ref.backward(dy.double())
    dx, dg, db, ag, ab = S.ln_bwd(dy, x, mean, rstd, gamma, dres)
    assert float((dx - (xd.grad + dres.double())).abs().max()) < 1e-12
    assert float((dg - gd.grad).abs().max()) < 1e-12 and float((db - bd.grad).abs().max()) < 1e-12
    assert bool((ag >= dg.abs()).all()) and bool((ab >= db.abs()).all())
    xf = rnd(3, 9, D, seed=3)
    pooled = S.cls_avgpool_norm(xf, gamma, beta, 1e-6)
    full = F.layer_norm(xf.double(), (D,), gamma.double(), beta.double(), S.f32(1e-6))
    assert float((pooled[:, 0::2] - full[:, 0]).abs().max()) < 1e-12
    assert float((pooled[:, 1::2] - full[:, 1:].mean(1)).abs().max()) < 1e-12


def test_dino_loss_references_equal_the_formulas():
    from oracle import dino_oracle as do
    B, ncrops, n = 3, 3, 1028
    s, t, c = rnd(ncrops * B, n, seed=4, scale=0.4), rnd(2 * B, n, seed=5, scale=0.4), rnd(n, seed=6, scale=0.05)
    assert float((S.row_lse(t, 20.0, c) - torch.logsumexp((t.double() - c.double()) * 20.0, -1)).abs().max()) < 1e-12
    loss, dl = S.dino_loss(s, t, c, 0.05, ncrops)
    q = F.softmax((t.double() - c.double()) / S.f32(0.05), -1).view(2, B, n)
    p = F.softmax(s.double() / S.f32(0.1), -1).view(ncrops, B, n)
    coef = 1.0 / ((2 * ncrops - 2) * B * S.f32(0.1))
    for v in range(ncrops):                                     # the kernel's header: coef (n_i(v) p_v - sum_{i != v} q_i)
        others = [i for i in range(2) if i != v]
        want = coef * (len(others) * p[v] - sum(q[i] for i in others))
        assert float((dl.view(ncrops, B, n)[v] - want).abs().max()) < 1e-14
    assert float(loss) > 0
    cs, ca = S.colsum(t)
    got = S.center_ema(c, cs, 0.9, 1.0 / (2 * B * 4))
    ref = do.center_update(c.double().view(1, -1), t.double(), world_size=4, momentum=S.f32(0.9))[0]
    assert float((got - ref).abs().max()) < 1e-9 and bool((ca >= cs.abs()).all())   # inv_count is an fp32 here


def test_head_references_equal_torch_fp64():
    u = S.gelu_inputs(1028)
    ud = u.double().requires_grad_(True)
    ref = F.gelu(ud)
    ref.backward(torch.ones_like(ref))
    assert float((S.gelu(u) - ref).abs().max()) < 1e-14 and float((S.dgelu(u) - ud.grad).abs().max()) < 1e-14
    assert float(S.gelu(torch.tensor([-12.0]))) < 0                # erfc keeps the left tail: 1 + erf cancels to 0 there
    # F.normalize: the closed form, dout / eps on the clamp rows
    z, kinds = S.l2_rows(5, 260, 2.7e-5)
    dout = rnd(5, 260, seed=7)
    out, inv, dz = S.l2norm(z, 2.7e-5, dout)
    model = S.l2norm_bwd_model(dout, out, inv, z, 2.7e-5)
    assert S.rel_l2(dz, model) < 1e-12
    for r in S.l2_clamp_rows(kinds):
        assert S.rel_l2(dz[r], dout[r].double() / S.f32(2.7e-5)) < 1e-12
    # weight_norm against torch's own
    v, g, dw = rnd(5, 252, seed=8, scale=0.05), 1.0 + 0.1 * rnd(5, seed=9), rnd(5, 252, seed=10)
    vd, gd = v.double().requires_grad_(True), g.double().view(-1, 1).requires_grad_(True)
    ref = torch._weight_norm(vd, gd, 0)
    ref.backward(dw.double())
    w, winv, dv, dg, terms = S.weight_norm(v, g, dw)
    assert S.rel_l2(w, ref) < 1e-14 and S.rel_l2(dv, vd.grad) < 1e-12 and S.rel_l2(dg, gd.grad.view(-1)) < 1e-12
    assert bool((terms >= dg.abs() - 1e-12).all()) and S.rel_l2(winv, 1.0 / v.double().norm(dim=1)) < 1e-14
    # the split recipe: hi + lo restores x to 16 bits, both layouts
    x = S.split3_values(7, 12)
    a, b = S.split3(x, False).float(), S.split3(x, True).float()
    assert torch.equal(a[:, :12], a[:, 12:24]) and torch.equal(b[:, :12], b[:, 24:]) and torch.equal(a[:, 24:], b[:, 12:24])
    assert torch.equal(a[:, :12], x.to(torch.bfloat16).float())
    assert float(((a[:, :12].double() + a[:, 24:].double() - x.double()).abs() / x.double().abs()).max()) < 2.0 ** -15
    assert float(x.abs().min()) < 1e-15 and float(x.abs().max()) > 1e15


def test_positional_map_references_equal_the_oracle():
    from oracle import dino_oracle as do
    from sais_amd import vit
    for w, h in S.POS_SIZES:
        Wm = torch.from_numpy(vit.pos_interp_matrix(14, w, h).astype(np.float32))
        assert Wm.shape == ((w // 16) * (h // 16), 196)
        assert float((Wm.double() - torch.from_numpy(do.pos_interp_matrix(14, w, h))).abs().max()) < 1e-7
    assert Wm.shape[0] == 1                                        # (16, 16): no smaller map exists, 0 patches is rejected
    pos = rnd(197, 8, seed=11).double().requires_grad_(True)
    Wm = torch.from_numpy(vit.pos_interp_matrix(14, 96, 160)).double()
    out = S.pos_interp_fwd(Wm, pos.detach())
    ref = torch.cat([pos[:1], Wm @ pos[1:]])
    dout = rnd(out.shape[0], 8, seed=12).double()
    ref.backward(dout)
    assert torch.equal(out, ref.detach())
    assert float((S.pos_interp_bwd(Wm, dout, torch.ones(197, 8)) - (pos.grad + 1.0)).abs().max()) < 1e-13


def test_optimizer_references_equal_torch():
    p, g = rnd(1025, seed=13), rnd(1025, seed=14)
    pt = torch.nn.Parameter(p.double().clone())
    pt.grad = g.double() * S.f32(0.5)
    torch.optim.SGD([pt], lr=S.f32(0.1)).step()
    assert float((S.sgd(p, g, 0.1, 0.5) - pt.detach()).abs().max()) < 1e-15
    shapes = {"w.weight": (6, 50), "w.bias": (50,)}
    params = {n: rnd(*s, seed=15 + i, scale=0.3) for i, (n, s) in enumerate(shapes.items())}
    ref = S.OptRef(params)
    tp = {n: torch.nn.Parameter(v.double().clone()) for n, v in params.items()}
    opts = [torch.optim.AdamW([tp["w.weight"]], lr=S.f32(1e-3), weight_decay=S.f32(0.05), eps=1e-8),
            torch.optim.AdamW([tp["w.bias"]], lr=S.f32(1e-3), weight_decay=0.0, eps=1e-8)]
    for it in range(2):
        grads = {n: rnd(*s, seed=20 + 2 * it + i) for i, (n, s) in enumerate(shapes.items())}
        norms = ref.step(grads, 0.0, 1e-3, 0.05, 0.9, False)
        for n in tp:
            tp[n].grad = grads[n].double()
            assert abs(float(norms[n]) - float(grads[n].double().norm())) < 1e-12
        for o in opts:
            o.step()
        for n in tp:
            assert float((ref.st[n] - tp[n].detach()).abs().max()) < 1e-12, (it, n)
    assert float((ref.tt["w.bias"] - params["w.bias"].double()).abs().max()) > 0          # the teacher copy moved


# ------------------------------------------------------------------------------------------------ case tables
def test_integer_recipes_are_exact_in_any_order():
    for rows in S.LN_BWD_INT_ROWS:
        dy16, dy32, x = S.ints((rows, D), 1), S.ints((rows, D), 2), S.ints((rows, D), 3)
        assert torch.equal(dy16.to(torch.bfloat16).float(), dy16)
        _, dg, db, ag, ab = S.ln_bwd(dy16 + dy32, x, torch.zeros(rows), torch.ones(rows), S.gamma_int(4))
        assert S.int_exact(ag + 4, ab + 4) and torch.equal(dg, dg.round()) and torch.equal(db, db.round())
    for ntok in S.EMBED_NTOK:
        for fr in S.EMBED_FRAMES:
            dtok = S.ints((fr, ntok, 8), 5)
            dcls, dpos, patch, apos = S.embed_bwd(dtok, S.ints((8,), 6), S.ints((ntok, 8), 7))
            assert S.int_exact(apos) and torch.equal(patch.double(), dtok[:, 1:].reshape(-1, 8).double())
            m = S.embed_bwd_model(dtok, S.ints((8,), 6), S.ints((ntok, 8), 7))
            assert torch.equal(m[0], dcls) and torch.equal(m[1], dpos)
    for rows in S.COLSUM_ROWS:
        s, a = S.colsum(S.ints((rows, 260), 8, -64, 64))
        assert S.int_exact(a) and torch.equal(s, s.round())
    assert not S.int_exact(torch.tensor([0.5]).double()) and not S.int_exact(torch.tensor([2.0 ** 24]).double())


def test_grid_caps_are_crossed_and_chunks_are_ragged():
    assert max(S.LN_BWD_ROWS) > 2 * 8192 > 8200 > 8192 and 57 * 196 * 48 > S.GRID2048 > 3 * 196 * 48
    assert max(S.SGD_N) // 4 > S.GRID2048 and max(S.CAST_N) > S.GRID2048 and max(r * d for r, d in S.CAST_ROWS) > S.GRID2048
    assert max(S.GELU_N) // 4 > S.GRID4096 and max(r * k for r, k in S.SPLIT3) // 4 > S.GRID4096
    per = [(f + 3) // 4 for f in S.EMBED_FRAMES]
    assert any(4 * p - f >= p for p, f in zip(per, S.EMBED_FRAMES))          # an empty chunk
    assert any(f % p for p, f in zip(per, S.EMBED_FRAMES)) and max(per) >= 4  # a ragged chunk, a full unrolled group
    assert all(n % 4 == 0 for n in S.LSE_N + S.LOSS_N + S.COLSUM_N + S.CENTER_N + S.ROW_DIMS + S.ADAMW_SIZES)
    assert any(n % 1024 for n in S.LSE_N) and any(n > 4096 and n % 4096 for n in S.LSE_N)
    sizes = sorted(math.prod(s) for n, s in S.adamw_toy_shapes().items() if n not in S.ADAMW_NO_GRAD)
    assert sizes == sorted(S.ADAMW_SIZES) and (max(sizes) + 8191) // 8192 > 64


@pytest.mark.parametrize("eps", S.L2_EPS)
def test_no_clamp_row_norm_within_16_ulp_of_eps(eps):
    for dim in S.ROW_DIMS:
        for rows in S.ROW_ROWS:
            z, kinds = S.l2_rows(rows, dim, eps)
            assert S.l2_condition(z, eps), (dim, rows)
            nrm = z.double().norm(dim=-1)
            for r, k in enumerate(kinds):
                assert (float(nrm[r]) < S.f32(eps)) == (k in ("zero", "half_eps")), (dim, rows, r, k)
    seen = {k for rows in S.ROW_ROWS for k in S.l2_rows(rows, 4, eps)[1]}
    assert seen == set(S.L2_KINDS)
    assert not S.l2_condition(torch.tensor([[S.f32(eps) * (1 + 2.0 ** -22), 0.0, 0.0, 0.0]]), eps)


@pytest.mark.parametrize("kind", S.LN_KINDS)
@pytest.mark.parametrize("eps", S.LN_EPS)
def test_layernorm_emulation_sits_inside_its_bars(kind, eps):
    x, (gamma, beta) = S.ln_rows(kind, 64), S.ln_params()
    y, mean, rstd = S.ln_fwd(x, gamma, beta, eps)
    atol, torch_err = S.ln_y_atol(x, gamma, beta, eps)
    ey, emu, ers = S.ln_emul(x, gamma, beta, eps)
    assert S.ratio(ey, y, atol) <= 1.0, (S.ratio(ey, y, atol), torch_err)
    assert float(((emu.double() - mean).abs() / S.ln_mean_bar(x, mean)).max()) <= 1.0
    assert S.ratio(ers, rstd, 0.0, S.RSTD_RTOL) <= 1.0
    assert atol == S.Y32_ATOL or kind in S.LN_HARD                  # well-scaled rows keep the old bar


def test_constant_rows_have_an_exact_mean_in_the_kernel_order():
    gamma, beta = S.ln_params()
    for c in (0.0, 1.0):
        y, mu, rs = S.ln_emul(torch.full((2, D), c), gamma, beta, 1e-6)
        assert torch.equal(mu, torch.full((2,), c)) and torch.equal(y, beta.expand(2, D))


# ------------------------------------------------------------------------------------------------ the bars have teeth
def test_one_pass_variance_fails_the_offset_rows():
    gamma, beta = S.ln_params()
    for kind in ("offset1000", "offset100"):
        x = S.ln_rows(kind, 64)
        y = S.ln_fwd(x, gamma, beta, 1e-6)[0]
        atol, _ = S.ln_y_atol(x, gamma, beta, 1e-6)
        assert S.ratio(S.ln_emul(x, gamma, beta, 1e-6)[0], y, atol) <= 1.0
        assert not S.ratio(S.ln_emul(x, gamma, beta, 1e-6, one_pass=True)[0], y, atol) <= 1.0
    x = S.ln_rows("plain", 64)                                      # the friendly rows of the older test cannot tell
    assert S.ratio(S.ln_emul(x, gamma, beta, 1e-6, one_pass=True)[0], S.ln_fwd(x, gamma, beta, 1e-6)[0], S.Y32_ATOL) <= 1.0


def test_dropped_frame_fails_the_embedding_sums():
    for fr in S.EMBED_FRAMES:
        dtok = S.ints((fr, 37, 8), 5) * 2 + 1                       # odd values: a dropped frame always shows
        dcls, dpos, _, _ = S.embed_bwd(dtok, S.ints((8,), 6), S.ints((37, 8), 7))
        bad = S.embed_bwd_model(dtok, S.ints((8,), 6), S.ints((37, 8), 7), drop_last_frame=True)
        assert (torch.equal(bad[0], dcls) and torch.equal(bad[1], dpos)) == (fr <= 4), fr


def test_ignored_row_stride_fails_through_the_sentinel():
    x, (gamma, beta) = S.ln_rows("plain", 9), S.ln_params()
    xv, _ = S.strided_in(x, 8, 4)
    y = S.ln_fwd(x, gamma, beta, 1e-6)[0]
    assert S.ratio(S.ln_fwd_model(xv, gamma, beta, 1e-6), y, S.Y32_ATOL) <= 1.0
    assert not S.ratio(S.ln_fwd_model(xv, gamma, beta, 1e-6, ld_ignored=True), y, S.Y32_ATOL) <= 1.0
    out, buf = G.padded(torch.zeros(9, D), 8, 4)
    out.as_strided((9, D), (D, 1), out.storage_offset()).copy_(y.float())       # the same mistake on an output
    with pytest.raises(AssertionError):
        G.untouched(buf, out)


@pytest.mark.parametrize("eps", S.L2_EPS)
def test_projection_kept_on_a_clamp_row_fails(eps):
    z, kinds = S.l2_rows(4, 256, eps)
    dout = rnd(4, 256, seed=7)
    out, inv, dz = S.l2norm(z, eps, dout)
    clamp = S.l2_clamp_rows(kinds)
    half = [r for r, k in enumerate(kinds) if k == "half_eps"]
    good = S.l2norm_bwd_model(dout, out, inv, z, eps)
    bad = S.l2norm_bwd_model(dout, out, inv, z, eps, keep_projection=True)
    assert S.rel_l2(good[clamp], dz[clamp]) <= S.NORM_BWD_REL and S.rel_l2(bad[half], dz[half]) > 50 * S.NORM_BWD_REL
    # with every row in one norm the 1 / eps rows of the zero kind hide nothing, but a plain row's error would vanish
    assert S.rel_l2(torch.cat([good[clamp], 1.01 * good[[0]]]), torch.cat([dz[clamp], dz[[0]]])) <= S.NORM_BWD_REL


def test_lse_without_the_max_fails_the_shifted_rows():
    for kind in ("peak", "shifted"):
        x = S.lse_rows(kind, 3, 1028)
        ref = S.row_lse(x, 25.0)
        assert not S.ratio(S.lse_naive_f32(x, 25.0), ref, S.LSE_ATOL, ulps=2) <= 1.0
    x = S.lse_rows("plain", 3, 1028)
    assert S.ratio(S.lse_naive_f32(x, 10.0), S.row_lse(x, 10.0), S.LSE_ATOL, ulps=2) <= 1.0


def test_decay_on_a_no_decay_tensor_fails_the_adamw_bar():
    shapes = {"w.weight": (6, 50), "w.bias": (50,), "v": (40,)}
    params = {n: rnd(*s, seed=30 + i, scale=0.3) for i, (n, s) in enumerate(shapes.items())}
    good, bad = S.OptRef(params), S.OptRef(params)
    grads = {n: rnd(*s, seed=40 + i) for i, (n, s) in enumerate(shapes.items())}
    good.step(grads, 1e-3, 1e-3, 0.05, 0.9, False)
    bad.step(grads, 1e-3, 1e-3, 0.05, 0.9, False, decay_everything=True)
    assert S.ratio(bad.st["w.weight"], good.st["w.weight"], S.ADAMW_ATOL) <= 1.0
    for n in ("w.bias", "v"):
        assert S.ratio(bad.st[n], good.st[n], S.ADAMW_ATOL) > 1.0 and S.ratio(bad.tt[n], good.tt[n], S.ADAMW_ATOL) > 0.4


def test_l2norm_clamp_predicate_in_ieee_fp32():
    """`(1.0f / eps) * eps >= 1.0f`, the kernel's old predicate, holds for the default eps and fails for two of the table's
    three; `inv >= 1.0f / eps` with the forward's own expression holds for all, and for no row that is 16 ulp clear of eps"""
    one = np.float32(1.0)
    old = {e: bool((one / np.float32(e)) * np.float32(e) >= one) for e in S.L2_EPS}
    assert old == {1e-12: True, 1.3e-8: False, 2.7e-5: False}
    for e in S.L2_EPS:
        e32 = np.float32(e)
        assert one / np.maximum(np.float32(0.5) * e32, e32) >= one / e32
        clear = e32 * (one + np.float32(17 * 2.0 ** -23))
        assert not one / np.maximum(clear, e32) >= one / e32
