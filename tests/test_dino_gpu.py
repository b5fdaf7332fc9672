"""DINO pre-training objective on a real MI355X (sais_amd/dino.py + csrc/dino.hip through the C ABI) against
  * the vectors the reference itself produced (tests/golden/dino_step.npz, dino_loss.npz: main_dino.DINOLoss, the body
    of train_one_epoch with torch AdamW, DINOHead, MultiCropWrapper with 96 x 96 crops), and
  * the pinned oracle (oracle/dino_oracle.py, fp64) on seeded inputs at sizes the goldens do not cover.
Tolerances: fp32 streaming kernels ~1e-6 relative; anything that crosses the ViT's bf16 MFMA operands keeps the bars
of tests/test_model_gpu.py (features 2 % of max |ref|, gradients 2 % relative L2 per tensor)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import synth  # noqa: E402
from parity import parity_log  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sais_amd import ops as o
    return o


@pytest.fixture(scope="module")
def gstep():
    return np.load(os.path.join(HERE, "golden", "dino_step.npz"))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ------------------------------------------------------------------ DINOLoss kernels
@pytest.mark.parametrize("epoch", [0, 5])
def test_dino_loss_65536_vs_reference_golden(ops, epoch):
    """The reference's DINOLoss at its default out_dim = 65536, ncrops = 10, non-zero centre."""
    from oracle import dino_oracle as do
    g = np.load(os.path.join(HERE, "golden", "dino_loss.npz"))
    n, B, ncrops = 65536, 2, 10
    gen = synth._gen(410)
    s = (torch.randn(ncrops * B, n, generator=gen) * 0.3).to(DEV)
    t = (torch.randn(2 * B, n, generator=gen) * 0.3).to(DEV)
    c = (torch.randn(1, n, generator=gen) * 0.05).to(DEV)
    temp = float(do.teacher_temp_schedule(0.04, 0.07, 3, 10)[epoch])
    t_lse = ops.dino_row_lse(t, 1.0 / temp, c.view(-1))
    s_lse = ops.dino_row_lse(s, 10.0)
    ref_s = torch.logsumexp(s.double() * 10.0, -1)
    ref_t = torch.logsumexp((t.double() - c.double()) / temp, -1)
    assert (s_lse.double() - ref_s).abs().max().item() < 2e-5 and (t_lse.double() - ref_t).abs().max().item() < 2e-5
    dl = torch.full_like(s, float("nan"))
    loss = torch.empty((), device=DEV)
    ops.dino_loss(s, t, c.view(-1), s_lse, t_lse, B, ncrops, 0.1, temp, dl, loss)
    ref = float(g[f"e{epoch}/loss"])
    parity_log("dino_loss_rel", abs(loss.item() - ref) / ref, 2e-5)
    assert abs(loss.item() - ref) < 2e-5 * ref
    gc = g[f"e{epoch}/grad_cols"]
    assert np.abs(dl[:, ::257].cpu().numpy() - gc).max() < 2e-5 * np.abs(gc).max()
    np.testing.assert_allclose(dl.double().abs().sum(1).cpu().numpy(), g[f"e{epoch}/grad_abs_sum"], rtol=3e-5)
    # centre update (world size 1)
    colsum = torch.empty(n, device=DEV)
    ops.dino_colsum(t, colsum)
    center = c.clone().view(-1)
    ops.dino_center_ema(center, colsum, 0.9, 1.0 / (2 * B))
    assert np.abs(center.cpu().numpy() - g[f"e{epoch}/center_after"][0]).max() < 1e-7
    # bit-reproducible (fixed-order reductions, no float atomics)
    dl2, loss2 = torch.empty_like(dl), torch.empty((), device=DEV)
    ops.dino_loss(s, t, c.view(-1), s_lse, t_lse, B, ncrops, 0.1, temp, dl2, loss2)
    assert torch.equal(dl, dl2) and loss.item() == loss2.item()


@pytest.mark.parametrize("B,ncrops,n", [(3, 2, 1024), (5, 7, 4096), (64, 10, 8192)])
def test_dino_loss_shapes_vs_oracle(ops, B, ncrops, n):
    """ncrops = 2 (--local_crops_number 0), odd batch sizes, the benchmark's B = 64 with 2 + 8 crops."""
    from oracle import dino_oracle as do
    s, t, c = rnd(ncrops * B, n, seed=1, scale=0.4), rnd(2 * B, n, seed=2, scale=0.4), rnd(1, n, seed=3, scale=0.05)
    sd = s.double().cpu().requires_grad_(True)
    ref = do.dino_loss(sd, t.double().cpu(), c.double().cpu(), 0.05, ncrops)
    ref.backward()
    dl, loss = torch.empty_like(s), torch.empty((), device=DEV)
    ops.dino_loss(s, t, c.view(-1), ops.dino_row_lse(s, 10.0), ops.dino_row_lse(t, 20.0, c.view(-1)), B, ncrops, 0.1, 0.05,
                  dl, loss)
    assert abs(loss.item() - float(ref.detach())) < 1e-5 * float(ref.detach())
    assert rel(dl, sd.grad) < 2e-5
    c2 = do.center_update(c.double().cpu(), t.double().cpu(), world_size=4)
    colsum = torch.empty(n, device=DEV)
    ops.dino_colsum(t, colsum)
    cc = c.clone().view(-1)
    ops.dino_center_ema(cc, colsum, 0.9, 1.0 / (2 * B * 4))
    assert (cc.double().cpu() - c2[0]).abs().max().item() < 1e-7


# ------------------------------------------------------------------ DINOHead pieces
def test_gelu_l2norm_weightnorm_vs_torch(ops):
    import torch.nn.functional as F
    u = rnd(40, 2048, seed=5, scale=2.0)
    h, du = torch.empty_like(u), torch.empty_like(u)
    ops.gelu_fwd_f32(u, h)
    ud = u.double().cpu().requires_grad_(True)
    ref = F.gelu(ud)
    assert (h.double().cpu() - ref).abs().max().item() < 1e-6
    dh = rnd(40, 2048, seed=6)
    ref.backward(dh.double().cpu())
    ops.gelu_bwd_f32(dh, u, du)
    assert (du.double().cpu() - ud.grad).abs().max().item() < 3e-6
    # F.normalize
    z = rnd(37, 256, seed=7, scale=3.0)
    z[5] = 0.0                                                       # the eps branch
    out, inv, dz = torch.empty_like(z), torch.empty(37, device=DEV), torch.empty_like(z)
    ops.l2norm_fwd(z, out, inv)
    zd = z.double().cpu().requires_grad_(True)
    ref = F.normalize(zd, dim=-1, p=2)
    assert (out.double().cpu() - ref).abs().max().item() < 1e-6
    dout = rnd(37, 256, seed=8)
    ref.backward(dout.double().cpu())
    ops.l2norm_bwd(dout, out, inv, dz)
    keep = [i for i in range(37) if i != 5]
    assert rel(dz[keep], zd.grad[keep]) < 1e-5
    assert rel(dz[5], dout[5].double() / 1e-12) < 1e-5              # below the clamp: dout / eps
    # weight_norm
    v, g = rnd(1024, 256, seed=9, scale=0.05), (1.0 + 0.1 * rnd(1024, seed=10))
    w, winv = torch.empty_like(v), torch.empty(1024, device=DEV)
    ops.weight_norm_fwd(v, g, w, winv)
    vd, gd = v.double().cpu().requires_grad_(True), g.double().cpu().requires_grad_(True)
    ref = gd.view(-1, 1) * vd / vd.norm(dim=1, keepdim=True)
    assert rel(w, ref) < 1e-6
    dw = rnd(1024, 256, seed=11)
    ref.backward(dw.double().cpu())
    dv, dg = torch.ones_like(v), torch.ones_like(g)                  # accumulate on top of existing values
    ops.weight_norm_bwd(dw, v, g, winv, dv, dg)
    assert rel(dv - 1.0, vd.grad) < 1e-5 and rel(dg - 1.0, gd.grad) < 1e-5


def test_bf16x3_concat_gemm_is_fp32_grade(ops):
    """The logits GEMM: [hi | hi | lo] . [hi | lo | hi]^T on the bf16 kernel (K' = 3 K) against fp64; the plain bf16
    product of the same operands is ~2^-9 off, this one ~2^-17."""
    from sais_amd import _lib as L
    x = torch.nn.functional.normalize(rnd(40, 256, seed=16), dim=-1)
    w = torch.nn.functional.normalize(rnd(1024, 256, seed=17), dim=-1)
    x3 = torch.empty(40, 768, dtype=torch.bfloat16, device=DEV)
    w3 = torch.empty(1024, 768, dtype=torch.bfloat16, device=DEV)
    ops.split_bf16x3(x, x3, False)
    ops.split_bf16x3(w, w3, True)
    assert torch.equal(x3[:, :256], x.to(torch.bfloat16)) and torch.equal(x3[:, 256:512], x3[:, :256])
    assert torch.equal(w3[:, 512:], w.to(torch.bfloat16))
    assert torch.equal(w3[:, 256:512], (w - w.to(torch.bfloat16).float()).to(torch.bfloat16))
    out = torch.empty(40, 1024, device=DEV)
    ops.gemm_nt(x3, w3, L.EPI_BIAS_F32, out)
    ref = x.double() @ w.double().t()
    err = (out.double() - ref).abs().max().item()
    plain = (x.to(torch.bfloat16).double() @ w.to(torch.bfloat16).double().t() - ref).abs().max().item()
    parity_log("dino_bf16x3_concat_abs", err, 2e-5)
    assert err < 2e-5 and plain > 20 * err                            # cosines in [-1, 1]


def test_pos_interp_kernels(ops):
    from sais_amd import vit
    Wm = torch.from_numpy(vit.pos_interp_matrix(14, 96, 96).astype(np.float32)).to(DEV)
    pos = rnd(197, 384, seed=12)
    out = torch.empty(37, 384, device=DEV)
    ops.pos_interp_fwd(Wm, pos, out)
    ref = torch.cat([pos[:1].double(), Wm.double() @ pos[1:].double()])
    assert (out.double() - ref).abs().max().item() < 1e-5
    dout, dpos = rnd(37, 384, seed=13), torch.ones(197, 384, device=DEV)
    ops.pos_interp_bwd(Wm, dout, dpos)
    refb = torch.cat([dout[:1].double(), Wm.double().t() @ dout[1:].double()]) + 1.0
    assert (dpos.double() - refb).abs().max().item() < 1e-5


# ------------------------------------------------------------------ 37-token ViT
@pytest.mark.parametrize("frames", [70, 129])
def test_attention_37_tokens(ops, frames):
    """The backward's persistent grid for 37 tokens is capped at 256 x 3 = 768 workgroups (attn_vit.hip launch_bwd: three
    43.5-KB workgroups fit the LDS of a CU).  70 frames = 420 problems run in ONE pass; 129 frames = 774 problems is the
    smallest count past the cap, so six workgroups take a second problem (main_dino.py at batch 64 with 8 local crops runs
    3072 problems: four passes)."""
    qkv = (rnd(frames * 37, 1152, seed=30, scale=1.5)).to(torch.bfloat16)
    out = torch.empty(frames * 37, 384, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(frames, 6, 37, device=DEV)
    probs = torch.empty(frames, 6, 37, 37, device=DEV)
    ops.vit_attn_fwd(qkv, frames, out, lse, probs, ntok=37)
    qr = qkv.float().requires_grad_(True)
    q, k, v = qr.view(frames, 37, 3, 6, 64).permute(2, 0, 3, 1, 4)
    p = ((q @ k.transpose(-2, -1)) * 0.125).softmax(-1)
    ref = (p @ v).transpose(1, 2).reshape(frames * 37, 384)
    assert (probs - p).abs().max().item() < 4e-3
    assert rel(out.float(), ref) < 1e-2
    dout = rnd(frames * 37, 384, seed=31).to(torch.bfloat16)
    ref.backward(dout.float())
    dqkv = torch.full((frames * 37, 1152), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.vit_attn_bwd(qkv, dout, out, lse, None, frames, dqkv, ntok=37)
    for i, name in enumerate(("dq", "dk", "dv")):
        assert rel(dqkv[:, 384 * i:384 * (i + 1)].float(), qr.grad[:, 384 * i:384 * (i + 1)]) <= 1.5e-2, name
    again = torch.full_like(dqkv, float("nan"))
    ops.vit_attn_bwd(qkv, dout, out, lse, None, frames, again, ntok=37)
    assert torch.equal(again, dqkv)


def test_backbone_at_96_vs_reference_golden(gstep):
    from sais_amd import vit
    model = vit.vit_small(patch_size=16)
    model.load_state_dict(synth.vit_state_dict(seed=20))
    model = model.to(DEV).eval()
    x = synth.dino_crops(seed=300, B=2, n_local=1)[2].to(DEV)
    with torch.no_grad():
        got = model(x).cpu().numpy()
    ref = gstep["cls_96"]
    err = np.abs(got - ref).max() / np.abs(ref).max()
    parity_log("dino_cls96_rel_max", err, 2e-2)
    assert err < 2e-2


@pytest.mark.parametrize("frames,drop_path", [(6, 0.0), (256, 0.1)])
def test_backbone_gradients_at_96_vs_oracle(frames, drop_path):
    """fwd + bwd of the 37-token path incl. the transposed bicubic map into pos_embed's gradient, depth 2, fp64 oracle.
    256 frames = 9 472 token rows: the dispatch of the benchmark (row-owning GEMMs with LayerNorm in their epilogue,
    M >= 8192), with DropPath 0.1 (the oracle is fed the draws the kernels made)."""
    from oracle import dino_oracle as do
    from sais_amd import vit
    sd = synth.vit_state_dict(seed=22, depth=2)
    model = vit.vit_small(patch_size=16, depth=2, drop_path_rate=drop_path)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    x = synth.dino_crops(seed=301, B=frames, n_local=1)[2].to(DEV)
    wv = rnd(frames, 384, seed=14)
    model.zero_grad()
    rep = model(x)
    (rep * wv).sum().backward()
    dp = None
    if drop_path > 0:
        dp = model.last_droppath_scales.view(4, frames, 37)[:, :, 0].double().cpu()
        assert (dp == 0).any()
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ref = do.vit_forward_res(leaves, x.double().cpu(), depth=2, droppath=dp)
    (ref * wv.double().cpu()).sum().backward()
    assert (rep.detach().double().cpu() - ref.detach()).abs().max().item() < 2e-2 * ref.abs().max().item()
    worst = 0.0
    for n, p in model.named_parameters():
        e = rel(p.grad, leaves[n].grad)
        worst = max(worst, e)
        assert e < 2e-2, (n, e)
    parity_log("dino_vit96_grad_rel_l2", worst, 2e-2)


def test_multigroup_pass_equals_separate_passes():
    """The multi-crop student runs both resolutions in ONE backbone pass (rows stacked); it must give what one pass per
    resolution gives (utils.MultiCropWrapper's loop, utils.py:619-628): features bit-identical (row-wise kernels, the same
    K order), gradients equal up to the order of the fp32 atomics."""
    from sais_amd import vit
    model = vit.vit_small(patch_size=16, depth=2)
    model.load_state_dict(synth.vit_state_dict(seed=27, depth=2))
    model = model.to(DEV).train()
    model.prune_last_block = False          # single-resolution passes would otherwise take the CLS-only last block (its own
    #                                         test: test_pruned_last_block_equals_full_compute); this one is about row stacking
    crops = synth.dino_crops(seed=340, B=5, n_local=2)
    a, b = torch.cat(crops[:2]).to(DEV), torch.cat(crops[2:]).to(DEV)            # 10 x 224^2, 10 x 96^2
    model._engine(a.device)
    dfeat = rnd(20, 384, seed=15)
    with torch.no_grad():
        rep, saved = model._forward_kernels([a, b], save=True)
        model.flat.grad.zero_()
        model._backward_kernels(saved, dfeat)
        g_multi = model.flat.grad.clone()
        ra, sa = model._forward_kernels(a, save=True)
        rb, sb = model._forward_kernels(b, save=True)
        model.flat.grad.zero_()
        model._backward_kernels(sa, dfeat[:10].contiguous())
        model._backward_kernels(sb, dfeat[10:].contiguous())
        g_sep = model.flat.grad.clone()
    assert torch.equal(rep, torch.cat([ra, rb]))
    assert rel(g_multi, g_sep) < 1e-5


@pytest.mark.parametrize("B,n_local", [(5, 2), (24, 11)])
def test_multigroup_cls_only_last_block_equals_full_compute(B, n_local):
    """The multi-crop pass also runs its last block on the CLS rows only (one CLS-attention launch and one dX qkv + norm1'
    launch per resolution, the row-local half on all frames together): features and the flat gradient must equal the pass
    that computes every row, DropPath draws shared.  (5, 2): stand-alone kernels; (24, 11): both groups >= 8192 rows, the
    row-owning kernels with the compact residual gradient (dres_period) per group."""
    from sais_amd import vit

    def run(prune):
        model = vit.vit_small(patch_size=16, depth=2, drop_path_rate=0.1)
        model.load_state_dict(synth.vit_state_dict(seed=27, depth=2))
        model = model.to(DEV).train()
        model.prune_last_block = prune
        model.drop_path_seed = 5
        crops = synth.dino_crops(seed=341, B=B, n_local=n_local)
        a, b = torch.cat(crops[:2]).to(DEV), torch.cat(crops[2:]).to(DEV)
        model._engine(a.device)
        dfeat = rnd(2 * B + n_local * B, 384, seed=16)
        with torch.no_grad():
            rep, saved = model._forward_kernels([a, b], save=True)
            assert bool(saved.get("pruned")) == prune
            model.flat.grad.zero_()
            model._backward_kernels(saved, dfeat)
            ev, _ = model.eval()._forward_kernels([a, b], save=False)
        return rep.clone(), model.flat.grad.clone(), ev.clone(), model.flat

    r1, g1, e1, flat = run(True)
    r0, g0, e0, _ = run(False)
    scale = float(r0.abs().max())
    assert float((r1 - r0).abs().max()) <= 5e-3 * scale and float((e1 - e0).abs().max()) <= 5e-3 * scale
    for n in flat.names:
        o, k = flat.offsets[n], flat.params[flat.names.index(n)].numel()
        e = rel(g1[o:o + k], g0[o:o + k])
        assert e <= 1e-2, (n, e)


def test_graphed_train_step_equals_eager():
    """dino.GraphedTrainStep (forward, loss + centre, backward, norms as one hipGraph; optimizer tail eager) against
    dino.train_step: five iterations over two epochs of a teacher-temperature warm-up (so the graph is captured twice), new
    crops, lr, weight decay and momentum every iteration, DropPath 0.1, clipping on, last layer frozen in epoch 0.  Loss,
    gradient norms, centre and every student / teacher parameter must agree (what differs is the order of fp32 atomics)."""
    from sais_amd import dino
    out_dim, n_local, B, depth = 2048, 2, 4, 2
    sd = {"backbone." + k: v for k, v in synth.vit_state_dict(seed=23, depth=depth).items()}
    sd.update({"head." + k: v for k, v in synth.dino_head_state_dict(seed=24, out_dim=out_dim).items()})
    lr_s = dino.cosine_scheduler(2e-4, 1e-6, 2, 3)
    wd_s = dino.cosine_scheduler(0.04, 0.4, 2, 3)
    mom_s = dino.cosine_scheduler(0.99, 1.0, 2, 3)
    batches = [[t.to(DEV) for t in synth.dino_crops(seed=360 + it, B=B, n_local=n_local)] for it in range(5)]

    def run(graphed):
        student, teacher = dino.build_student_teacher(out_dim=out_dim, drop_path_rate=0.1, device=DEV, depth=depth)
        student.load_state_dict(sd)
        teacher.load_state_dict(student.state_dict())
        student.train()
        student.backbone.drop_path_seed = 11
        loss_mod = dino.DINOLoss(out_dim, n_local + 2, 0.04, 0.07, 2, 4).to(DEV)      # temperature 0.04 -> 0.07 over 2 epochs
        opt = dino.DINOOptimizer(student, teacher)
        static = [t.clone() for t in batches[0]]
        step = dino.GraphedTrainStep(student, teacher, loss_mod, opt, static, clip_grad=0.3) if graphed else None
        rec = []
        for it in range(5):
            epoch = it // 3
            if graphed:
                for d, src in zip(static, batches[it]):
                    d.copy_(src)
                loss, norms = step(it, epoch, lr_s, wd_s, mom_s, freeze_last_layer=1)
            else:
                loss, norms = dino.train_step(student, teacher, loss_mod, opt, batches[it], it, epoch, lr_s, wd_s, mom_s,
                                              clip_grad=0.3, freeze_last_layer=1)
            rec.append((float(loss), norms.clone(), loss_mod.center.clone()))
        params = {"s." + n: p.detach().clone() for n, p in student.named_parameters()}
        params.update({"t." + n: p.detach().clone() for n, p in teacher.named_parameters()})
        return rec, params, opt.steps

    rg, pg, sg = run(True)
    re_, pe, se = run(False)
    assert sg == se == [5, 2]
    for it, ((lg, ng, cg), (le, ne, ce)) in enumerate(zip(rg, re_)):
        assert abs(lg - le) <= 2e-5 * abs(le), (it, lg, le)
        # the two runs' weights part by up to 2 lr per element and step (below), so their gradients part a little more with every
        # step: 1.06e-3 at iteration 4 in one run of six on one box (fp32 atomics order), 3-7e-4 otherwise
        assert rel(ng, ne) < 1e-3 * (1 + it), (it, rel(ng, ne))
        assert float((cg - ce).abs().max()) <= 1e-6 + 1e-3 * float(ce.abs().max()), it      # the weights drift apart by ~lr (below)
    for n in pe:
        # AdamW moves an element by ~lr whatever the gradient's size: where the sign of a rounding-noise gradient differs between
        # two summation orders the runs part by up to 2 lr per step; the bulk must agree to a fraction of one step
        d = (pg[n] - pe[n]).abs()
        assert float(d.max()) <= 2.2 * 2e-4 * 5 + 1e-6, (n, float(d.max()))
        assert float(d.float().median()) <= 2e-5, (n, float(d.float().median()))


# ------------------------------------------------------------------ optimizer tail
def test_adamw_clip_ema_vs_oracle():
    """Four steps of the fused clip + AdamW + EMA kernel on a small two-buffer model against oracle.adamw_update /
    clip_coef / ema (fp64), with a frozen class-1 tensor in the first two steps and a requires_grad=False tensor."""
    import torch.nn as nn
    from oracle import dino_oracle as do
    from sais_amd import dino
    from sais_amd.flat import FlatParams

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = nn.Linear(300, 70)                              # weight 21000 (3 chunks), bias 70
            self.norm = nn.LayerNorm(52)
            self.last_layer = nn.Linear(33, 9, bias=False)           # 297 elements: padded to 300
            self.g = nn.Parameter(torch.ones(12, 1), requires_grad=False)

    torch.manual_seed(3)
    student, teacher = Toy(), Toy()
    teacher.load_state_dict(student.state_dict())
    sf, tf = FlatParams(student, DEV), FlatParams(teacher, DEV)
    sf.refresh_shadows([]), tf.refresh_shadows([])
    part = dino._FlatAdamW(sf, tf, "head.", ("last_layer.weight",))
    st = {n: p.detach().double().cpu().clone() for n, p in student.named_parameters()}
    tt = {n: v.clone() for n, v in st.items()}
    m = {n: torch.zeros_like(v) for n, v in st.items()}
    v2 = {n: torch.zeros_like(v) for n, v in st.items()}
    steps = {n: 0 for n in st}
    counts = [0, 0]
    clip, betas, eps = 0.5, (0.9, 0.999), 1e-8
    for it in range(4):
        frozen = it < 2
        lr, wd, mom = 1e-3 * (it + 1), 0.05 * (it + 1), 0.9 + 0.02 * it
        gen = torch.Generator().manual_seed(100 + it)
        sf.grad.zero_()
        grads = {}
        for n, p in student.named_parameters():
            if p.requires_grad:
                grads[n] = torch.randn(p.shape, generator=gen) * (0.3 if "a." in n else 0.01)
                sf.g(n).copy_(grads[n])
        gs = 1.0
        if it == 3:                                                  # data parallel: the buffer holds the SUM over 4 ranks
            sf.grad.mul_(4.0)
            gs = 0.25
        norms = part.grad_norms(gs)
        counts[0] += 1
        counts[1] += 0 if frozen else 1
        part.step(clip, lr, wd, betas, eps, counts, frozen, mom, with_shadow=True, grad_scale=gs)
        for i, (n, p) in enumerate(student.named_parameters()):
            if p.requires_grad:
                g = grads[n].double()
                nrm, c = do.clip_coef(g, clip)
                assert abs(norms[i].item() - float(nrm)) < 1e-5 * float(nrm) + 1e-9
                if not ("last_layer" in n and frozen):
                    steps[n] += 1
                    st[n], m[n], v2[n] = do.adamw_update(st[n], g * c, m[n], v2[n], steps[n], lr,
                                                         wd if do.is_regularized(n, p.shape) else 0.0)
            tt[n] = do.ema(tt[n], st[n], mom)
        for n, p in student.named_parameters():
            assert (p.detach().double().cpu() - st[n]).abs().max().item() < 2e-6, (it, n)
            assert (dict(teacher.named_parameters())[n].detach().double().cpu() - tt[n]).abs().max().item() < 2e-6, (it, n)
            assert torch.equal(sf.w(n).float().cpu(), p.detach().to(torch.bfloat16).float().cpu())
    assert steps["last_layer.weight"] == 2 and float(student.g.min()) == 1.0


# ------------------------------------------------------------------ the whole step vs the reference's own run
def _student_sd(out_dim):
    sd = {"backbone." + k: v for k, v in synth.vit_state_dict(seed=20).items()}
    sd.update({"head." + k: v for k, v in synth.dino_head_state_dict(seed=21, out_dim=out_dim).items()})
    return sd


def sample(t):
    t = t.detach().reshape(-1)
    return (t[::97] if t.numel() > 20000 else t).double().cpu().numpy()


def test_train_steps_vs_reference_golden(gstep):
    """Four iterations of train_one_epoch's body (main_dino.py:521-566) on the reference's own inputs: teacher / student
    logits, loss, centre, per-parameter gradient norms (clipping active), frozen last layer in epoch 0, AdamW, EMA."""
    from sais_amd import dino
    c = {k: float(v) for k, v in zip(gstep["cfg_keys"], gstep["cfg_vals"])}
    out_dim, n_local, B = int(c["out_dim"]), int(c["n_local"]), int(c["B"])
    student, teacher = dino.build_student_teacher(out_dim=out_dim, drop_path_rate=0.0, device=DEV)
    student.load_state_dict(_student_sd(out_dim))
    teacher.load_state_dict(student.state_dict())
    loss_mod = dino.DINOLoss(out_dim, n_local + 2, c["warmup_teacher_temp"], c["teacher_temp"],
                             int(c["warmup_teacher_temp_epochs"]), int(c["epochs"])).to(DEV)
    opt = dino.DINOOptimizer(student, teacher)
    lr_s, wd_s, mom_s = gstep["lr_schedule"], gstep["wd_schedule"], gstep["momentum_schedule"]
    track = sorted({k.split("/", 2)[2] for k in gstep.files if k.startswith("it0/student/")})
    P, T = dict(student.named_parameters()), dict(teacher.named_parameters())
    for it in range(int(c["iters"])):
        epoch = it // int(c["niter_per_ep"])
        images = [t.to(DEV) for t in synth.dino_crops(seed=300 + it, B=B, n_local=n_local)]
        if it == 0:                                                  # logits before anything moved: the tightest check
            with torch.no_grad():
                t_out = teacher(images[:2])
                s_out = student(images)
            k = "it0/"
            e_t = np.abs(t_out.cpu().numpy() - gstep[k + "teacher_out"]).max()
            e_s = np.abs(s_out.cpu().numpy() - gstep[k + "student_out"]).max()
            parity_log("dino_logits_max_abs", max(e_t, e_s), 1e-2)
            assert e_t < 1e-2 and e_s < 1e-2                          # cosines in [-1, 1] behind 12 bf16 blocks
        loss, norms = dino.train_step(student, teacher, loss_mod, opt, images, it, epoch, lr_s, wd_s, mom_s,
                                      clip_grad=c["clip_grad"], freeze_last_layer=int(c["freeze_last_layer"]))
        k = f"it{it}/"
        ref_loss = float(gstep[k + "loss"])
        parity_log("dino_step_loss_rel", abs(loss.item() - ref_loss) / ref_loss, 2e-3)
        assert abs(loss.item() - ref_loss) < 2e-3 * ref_loss, (it, loss.item(), ref_loss)
        cen = loss_mod.center.cpu().numpy()
        assert np.abs(cen - gstep[k + "center_after"]).max() < 2e-3
        ref_n = gstep[k + "norms"]
        got_n = norms.cpu().numpy()
        assert got_n.shape == ref_n.shape
        nerr = np.abs(got_n - ref_n) / np.maximum(ref_n, 1e-12)
        parity_log("dino_grad_norm_rel", float(nerr.max()), 5e-2)
        assert nerr.max() < 5e-2, (it, list(gstep[k + "norm_names"][nerr > 5e-2]))
        lr = float(lr_s[it])
        for n in track:
            for who, sd in (("student", P), ("teacher", T)):
                ref = gstep[k + who + "/" + n]
                d = np.abs(sample(sd[n]) - ref)
                # AdamW moves every element by ~lr per step whatever the gradient's size; where the gradient's SIGN
                # differs (elements whose gradient is rounding noise) the two runs part by up to 2 lr per step
                assert d.max() < 2.2 * 2e-4 * (it + 1) + 1e-6, (it, who, n, d.max())
                assert np.median(d) < 0.25 * max(lr, 2e-4) + 1e-6, (it, who, n, float(np.median(d)))
    assert opt.steps == [4, 2]
    # checkpoint round trip in the reference's format
    ck = dino.checkpoint_dict(student, teacher, opt, loss_mod, epoch=2)
    assert set(ck["optimizer"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    s2, t2 = dino.build_student_teacher(out_dim=out_dim, drop_path_rate=0.0, device=DEV)
    l2 = dino.DINOLoss(out_dim, n_local + 2, 0.04, 0.07, 2, 3).to(DEV)
    images = [t.to(DEV) for t in synth.dino_crops(seed=300, B=B, n_local=n_local)]
    with torch.no_grad():
        s2(images), t2(images[:2])                                   # builds the flat buffers
    o2 = dino.DINOOptimizer(s2, t2)
    assert dino.load_checkpoint(ck, s2, t2, o2, l2) == 2
    with torch.no_grad():
        assert torch.equal(s2(images), student(images)) and torch.equal(t2(images[:2]), teacher(images[:2]))
    assert o2.steps == [4, 2] and torch.equal(l2.center, loss_mod.center)
    for (pa, _), (pb, _) in zip(o2._parts, opt._parts):
        assert torch.equal(pa.exp_avg, pb.exp_avg) and torch.equal(pa.exp_avg_sq, pb.exp_avg_sq)


@pytest.mark.parametrize("n_local,norm_last_layer,B,depth,out_dim,dt", [
    (8, True, 3, 2, 4096, torch.float64), (0, False, 3, 2, 4096, torch.float64), (8, True, 32, 3, 65536, torch.float32)])
def test_train_step_gradients_vs_oracle_with_droppath(n_local, norm_last_layer, B, depth, out_dim, dt):
    """One step at the reference's default multi-crop shape (2 global + 8 local crops) and at `--local_crops_number 0
    --norm_last_layer false` (weight_g trainable), out_dim 4096, depth 2, B = 3, with DropPath 0.1 on the student: the HIP
    step's pre-clip gradients against the fp64 oracle fed the SAME DropPath draws.  Third case: B = 32, out_dim 65536,
    depth 3 — 12 608 / 9 472 token rows per resolution group, i.e. the kernels `bench.py --workload dino` dispatches
    (row-owning GEMMs with LayerNorm epilogues from M = 8192 on; the 65536-wide head, loss and centre) — against the fp32
    oracle (an fp64 autograd graph of that size does not fit a test)."""
    from oracle import dino_oracle as do
    from sais_amd import dino
    sd = {"backbone." + k: v for k, v in synth.vit_state_dict(seed=23, depth=depth).items()}
    sd.update({"head." + k: v for k, v in synth.dino_head_state_dict(seed=24, out_dim=out_dim).items()})
    student, teacher = dino.build_student_teacher(out_dim=out_dim, drop_path_rate=0.1, norm_last_layer=norm_last_layer,
                                                  device=DEV, depth=depth)
    if not norm_last_layer:
        sd["head.last_layer.weight_g"] = 1.0 + 0.2 * torch.randn(out_dim, 1, generator=synth._gen(6))
    student.load_state_dict(sd)
    teacher.load_state_dict(student.state_dict())
    student.train()
    loss_mod = dino.DINOLoss(out_dim, n_local + 2, 0.04, 0.07, 3, 10).to(DEV)
    loss_mod.center = (torch.randn(1, out_dim, generator=synth._gen(5)) * 0.02).to(DEV)
    c0 = loss_mod.center.clone()
    images = [t.to(DEV) for t in synth.dino_crops(seed=320, B=B, n_local=n_local)]
    with torch.no_grad():
        t_out = teacher.forward_kernels(images[:2], save=False)[0]
        scales = []
        bb = student.backbone
        s_out, saved = student.forward_kernels(images, save=True)
        for g in saved[0]["groups"]:                                  # the draws each resolution group used
            ntok, Fr, lo = g["ntok"], g["Fr"], g["off"]
            scales.append(saved[0]["dp"][:, lo:lo + Fr * ntok].reshape(2 * depth, Fr, ntok)[:, :, 0].to(dt).cpu())
        loss = loss_mod(s_out, t_out, 1)
        student.backbone.flat.grad.zero_(); student.head.flat.grad.zero_()
        student.backward_kernels(saved, loss_mod.dlogits)
    assert n_local == 0 or any((s == 0).any() for s in scales)        # some branches really dropped
    st = do.TrainState(sd, dtype=dt)
    leaves = {k: v.clone().requires_grad_(k != "head.last_layer.weight_g" or not norm_last_layer) for k, v in st.student.items()}
    crops = [t.to(dt).cpu() for t in images]
    with torch.no_grad():
        t_ref = do.multicrop_forward(st.teacher, crops[:2], depth)
    s_ref = do.multicrop_forward(leaves, crops, depth, droppath=scales)
    ref = do.dino_loss(s_ref, t_ref, c0.to(dt).cpu(), float(loss_mod.teacher_temp_schedule[1]), n_local + 2)
    ref.backward()
    assert abs(loss.item() - float(ref.detach())) < 2e-3 * float(ref.detach())
    c1 = do.center_update(c0.to(dt).cpu(), t_ref)
    assert (loss_mod.center.double().cpu() - c1).abs().max().item() < 1e-3
    worst = 0.0
    for who, mod in (("backbone.", student.backbone), ("head.", student.head)):
        for n, p in mod.named_parameters():
            if not p.requires_grad:
                continue
            e = rel(mod.flat.g(n), leaves[who + n].grad)
            worst = max(worst, e)
            assert e < 3e-2, (who + n, e)
    assert student.head.last_layer.weight_g.requires_grad == (not norm_last_layer)
    parity_log("dino_step_grad_rel_l2", worst, 3e-2)


# ------------------------------------------------------------------ data parallel (one process per GPU)
DP_CFG = dict(out_dim=1024, n_local=2, B=2, depth=2)


def _dp_build(dev):
    from sais_amd import dino
    c = DP_CFG
    sd = {"backbone." + k: v for k, v in synth.vit_state_dict(seed=25, depth=c["depth"]).items()}
    sd.update({"head." + k: v for k, v in synth.dino_head_state_dict(seed=26, out_dim=c["out_dim"]).items()})
    student, teacher = dino.build_student_teacher(out_dim=c["out_dim"], drop_path_rate=0.0, device=dev, depth=c["depth"])
    student.load_state_dict(sd)
    teacher.load_state_dict(student.state_dict())
    loss_mod = dino.DINOLoss(c["out_dim"], c["n_local"] + 2, 0.04, 0.07, 3, 10).to(dev)
    return student, teacher, loss_mod, dino.DINOOptimizer(student, teacher)


def _dp_step(dev, images):
    from sais_amd import dino
    student, teacher, loss_mod, opt = _dp_build(dev)
    lr_s, wd_s, mom_s = np.full(4, 1e-4), np.full(4, 0.05), np.full(4, 0.9)
    loss, norms = dino.train_step(student, teacher, loss_mod, opt, images, 0, 1, lr_s, wd_s, mom_s, clip_grad=0.05,
                                  freeze_last_layer=0)
    torch.cuda.synchronize()
    return dict(loss=loss.item(), norms=norms.cpu(), center=loss_mod.center.cpu(),          # flat.grad = SUM over ranks
                gb=student.backbone.flat.grad.cpu() * opt.grad_scale, gh=student.head.flat.grad.cpu() * opt.grad_scale,
                pb=student.backbone.flat.flat.cpu(), tb=teacher.backbone.flat.flat.cpu())


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    B = DP_CFG["B"]
    crops = synth.dino_crops(seed=330, B=world * B, n_local=DP_CFG["n_local"])
    r = _dp_step(dev, [t[rank * B:(rank + 1) * B].to(dev) for t in crops])
    losses = [None] * world
    dist.all_gather_object(losses, r["loss"])
    if rank == 0:
        r["loss"] = sum(losses) / world
        torch.save(r, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_gloo_dino_step_equals_single_process(tmp_path):
    """2 ranks x B crops-sets: after DDP-style gradient averaging and the centre all-reduce (main_dino.py:413,627) the
    step equals the single-process step on the concatenated 2B batch (the loss is a mean over samples)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import torch.multiprocessing as mp
    out = str(tmp_path / "dino_dp.pt")
    mp.spawn(_dp_worker, args=(2, 29700 + (os.getpid() % 2000), out), nprocs=2, join=True)
    got = torch.load(out)
    dev = torch.device("cuda", 0)
    crops = synth.dino_crops(seed=330, B=2 * DP_CFG["B"], n_local=DP_CFG["n_local"])
    ref = _dp_step(dev, [t.to(dev) for t in crops])
    assert abs(got["loss"] - ref["loss"]) < 1e-5 * ref["loss"]
    assert (got["center"] - ref["center"]).abs().max().item() < 1e-6
    assert rel(got["gb"], ref["gb"]) < 3e-3 and rel(got["gh"], ref["gh"]) < 3e-3       # summation order only
    assert ((got["norms"] - ref["norms"]).abs() / ref["norms"].clamp_min(1e-12)).max().item() < 5e-3
    # after AdamW both runs moved (almost) every element by the same +-lr; sign flips only where the gradient is noise
    d = (got["pb"] - ref["pb"]).abs()
    assert d.max().item() <= 2.1e-4 and (d > 1e-6).float().mean().item() < 2e-2
    assert (got["tb"] - ref["tb"]).abs().max().item() <= 2.1e-5


# ------------------------------------------------------------------ the command line, end to end
def test_main_dino_cli_trains_resumes_and_feeds_the_extraction_loader(tmp_path):
    """SAIS/scripts/dino-main/main_dino.py on 8 synthetic frames: 2 epochs, then a second invocation that resumes from
    checkpoint.pth; the checkpoint loads through the extraction script's loader (extract_representations.loadModel's
    'student' branch, :190-199)."""
    import json
    import subprocess
    import pandas as pd
    from PIL import Image
    root = os.path.dirname(HERE)
    rng = np.random.default_rng(1)
    frames = tmp_path / "frames" / "Images" / "vidA"
    frames.mkdir(parents=True)
    (tmp_path / "paths").mkdir()
    rows = []
    for i in range(8):
        Image.fromarray(rng.integers(0, 256, (270, 480, 3), dtype=np.uint8)).save(frames / f"frames_{i:08d}.jpg")
        rows.append((f"Images\\vidA\\frames_{i:08d}.jpg", "vidA"))
    pd.DataFrame(rows, columns=["path", "label"]).to_csv(tmp_path / "paths" / "VUA_Paths.csv")
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "SAIS", "scripts", "dino-main", "main_dino.py"), "--data_path", str(tmp_path),
           "--frames_root", str(tmp_path / "frames"), "--datasets", "VUA", "--output_dir", str(out), "--batch_size_per_gpu", "4",
           "--local_crops_number", "2", "--out_dim", "1024", "--warmup_epochs", "1", "--num_workers", "0",
           "--saveckp_freq", "1", "--lr", "0.01"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29800 + os.getpid() % 1000), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd + ["--epochs", "2"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Starting DINO training" in r.stdout and os.path.exists(out / "checkpoint0001.pth")
    log = [json.loads(l) for l in open(out / "log.txt")]
    assert [l["epoch"] for l in log] == [0, 1] and all(math.isfinite(l["train_loss"]) and l["train_loss"] > 0 for l in log)
    ck = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert ck["epoch"] == 2 and set(ck) >= {"student", "teacher", "optimizer", "epoch", "args", "dino_loss"}
    r = subprocess.run(cmd + ["--epochs", "3"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "resumed from" in r.stdout and "at epoch 2" in r.stdout
    assert [json.loads(l)["epoch"] for l in open(out / "log.txt")] == [0, 1, 2]
    from sais_amd.model_io import load_vit
    vit = load_vit(str(out / "checkpoint.pth"), device=DEV)
    with torch.no_grad():
        rep = vit(torch.randn(2, 3, 224, 224, device=DEV))
    assert tuple(rep.shape) == (2, 384) and torch.isfinite(rep).all()
    # the trained weights differ from the initial ones and student != teacher (EMA lag)
    ck3 = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)
    k = "backbone.blocks.0.attn.qkv.weight"
    assert not torch.equal(ck3["student"]["module." + k], ck3["teacher"][k])


def test_bench_dino_over_rccl_world_of_one():
    """`bench.py --workload dino` under torchrun with SAIS_BENCH_FORCE_DIST=1: RCCL process group with one rank, the
    overlapped gradient all-reduces (head buffer + per-block backbone slices from the backward hook) and the centre
    all-reduce are really issued on the NCCL backend; the JSON line carries the exchange volume."""
    import json
    import subprocess
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.dirname(HERE)
    port = 29900 + (os.getpid() % 900)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
                        "--workload", "dino", "--gpus", "1", "--steps", "2", "--warmup", "1", "--dino-batch", "4",
                        "--dino-local-crops", "2", "--dino-out-dim", "1024"],
                       capture_output=True, text=True, cwd=root, timeout=900,
                       env=dict(os.environ, SAIS_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["metric"] == "dino_pretrain_images_per_s" and line["value"] > 0 and math.isfinite(line["loss"])
    assert line["comm"]["world"] == 1 and line["comm"]["grad_sync"] == "GradSync"
    assert line["comm"]["allreduce_bytes_per_step"] > 80e6                # 21.7 M backbone + 5.3 M head parameters, fp32
