"""Training on frames of different sizes in ONE segmented pass on the MI355X (csrc/attn_seg.hip: sais_vit_attn_bwd_seg,
sais_vit_embed_bwd_seg, the CLS scatter and the row expansion; sais_amd/vit.py: forward(list) under grad; dino.py:
MultiCropWrapper.segmented).  Case lists and the fp64 restatement: tests/vit_seg_bwd_ref.py.

  1. attention backward: dqkv of every segment bit-equal to sais_vit_attn_bwd_any on that frame alone (same qkv, dout, out, lse), both
     workgroup forms, three orders, the cap, padded strides with NaN pads and sentinel rows, run to run; one comparison with fp64
  2. embedding backward: dpatch bit-equal to the bf16 cast; dcls / dpos within (terms + 2) 2^-24 sum |Ty Tx dx| + 2^-24 |start| of
     the fp64 restatement on the f32 taps the kernel reads (f32 accumulation in a fixed order), onto a non-zero start, run to run
  3. the model at depth 2 against oracle.dino_oracle.vit_forward_res in fp64: features 2e-2 of max|ref|, every parameter gradient
     2e-2 rel-L2; 8350 rows with DropPath 0.1 for the fused GEMM + LayerNorm form
  4. a frame's feature row does not depend on the rest of the list; 5. launch records; 6. the DINO step; 7. refusals
"""
import functools
import math

import numpy as np
import pytest
import torch

import attn_any_bwd_ref as AB
import attn_ref as AR
import synth
import vit_seg_bwd_ref as B
import vit_seg_ref as R
from parity import parity_log

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32
SENT = 777.0
DEPTH = 2


@pytest.fixture(scope="module")
def ops():
    from sais_amd import ops as o
    return o


def _plan(grids):
    from sais_amd.vit_seg import SegPlan
    return SegPlan(grids).to_device(DEV)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ 1. attention backward
@functools.lru_cache(maxsize=None)
def _segment(layout, ntok, variant=0):
    """One frame alone: (qkv, dout, out, lse, dqkv) with out / lse of sais_vit_attn_fwd_any and dqkv of sais_vit_attn_bwd_any at
    frames = 1: computed once per (layout, ntok, draw), never written to"""
    from sais_amd import ops
    seed = 7000 + ntok + 10000 * variant
    qkv = AR.layouts(layout, 1, ntok, seed, AB.MULT[layout]).to(DEV)
    dout = rnd(ntok, AR.DM, seed=seed + 1).to(BF16).to(DEV)
    out = torch.full((ntok, AR.DM), NAN, dtype=BF16, device=DEV)
    lse = torch.full((1, AR.NH, ntok), NAN, dtype=F32, device=DEV)
    ops.vit_attn_fwd_any(qkv, 1, ntok, out, lse)
    dqkv = torch.full((ntok, 3 * AR.DM), NAN, dtype=BF16, device=DEV)
    ops.vit_attn_bwd_any(qkv, dout, out, lse, 1, ntok, dqkv)
    assert not torch.isnan(dqkv.float()).any()
    return qkv, dout, out, lse, dqkv


def _attn_bwd_case(ops, layout, ntoks):
    """every input with row strides 1160 / 392, NaN in the pad columns and in 128 rows past the pass; dqkv starts as a sentinel"""
    plan = _plan([(1, n - 1) for n in ntoks])
    assert plan.qtile == R.qtile(ntoks)
    M, G = plan.M, R.SENTINEL_ROWS
    seen, draws = {}, []
    for n in ntoks:
        draws.append(seen.get(n, 0) % 5)
        seen[n] = seen.get(n, 0) + 1
    qkv = torch.full((M + G, 1160), NAN, dtype=BF16, device=DEV)
    dout = torch.full((M + G, 392), NAN, dtype=BF16, device=DEV)
    out = torch.full((M + G, 392), NAN, dtype=BF16, device=DEV)
    lse = torch.full((6 * (M + G),), NAN, dtype=F32, device=DEV)
    where = list(zip(R.layout(plan.grids), ntoks, draws))
    for (row0, n, *_), s, k in where:
        q, d, o, l, _ = _segment(layout, s, k)
        qkv[row0:row0 + n, :1152], dout[row0:row0 + n, :384], out[row0:row0 + n, :384] = q, d, o
        lse[6 * row0:6 * (row0 + n)] = l.reshape(-1)            # the layout the segmented forward writes: [6, ntok] at 6 row0

    def run():
        dqkv = torch.full((M + G, 1160), SENT, dtype=BF16, device=DEV)
        ops.vit_attn_bwd_seg(qkv[:, :1152], dout[:, :384], out[:, :384], lse, plan, dqkv[:, :1152])
        torch.cuda.synchronize()
        return dqkv
    got = run()
    for (row0, n, *_), s, k in where:
        assert torch.equal(_bits(got[row0:row0 + n, :1152]), _bits(_segment(layout, s, k)[4])), (layout, s, k)
    assert (got[M:] == SENT).all() and (got[:, 1152:] == SENT).all()
    assert torch.equal(_bits(run()), _bits(got))                # two runs are bit-equal
    return plan


@pytest.mark.parametrize("order", range(len(R.ATTN_ORDERS)))
@pytest.mark.parametrize("layout", AR.BWD_LAYOUTS)
def test_attention_backward_segments_equal_the_frame_alone(ops, layout, order):
    """2, 17, 63, 64, 65, 129, 197 and 785 tokens in one call (32-row form), in order and in two permutations"""
    ntoks = [R.ATTN_NTOKS[i] for i in R.ATTN_ORDERS[order]]
    assert R.qtile(ntoks) == 32
    _attn_bwd_case(ops, layout, ntoks)


@pytest.mark.parametrize("layout", ("rand", "planted"))
def test_attention_backward_many_segments_take_the_64_row_form(ops, layout):
    assert R.qtile(R.ATTN_MANY) == 64 and AB.stream_bwd_waves(1, 65) == 2      # alone the frame takes the other form: same bits
    _attn_bwd_case(ops, layout, list(R.ATTN_MANY))


def test_attention_backward_one_segment_at_the_cap(ops):
    _attn_bwd_case(ops, "rand", list(R.ATTN_CAP))


def test_attention_backward_after_the_segmented_forward(ops):
    """forward and backward of the pass together: out / lse as sais_vit_attn_fwd_seg writes them feed the backward, which equals
    the frame-alone pair"""
    ntoks = [65, 2, 197, 64]
    plan = _plan([(1, n - 1) for n in ntoks])
    segs = [_segment("rand", n) for n in ntoks]
    qkv, dout = torch.cat([s[0] for s in segs]), torch.cat([s[1] for s in segs])
    out = torch.full((plan.M, 384), NAN, dtype=BF16, device=DEV)
    lse = torch.full((6 * plan.M,), NAN, dtype=F32, device=DEV)
    dqkv = torch.full((plan.M, 1152), NAN, dtype=BF16, device=DEV)
    ops.vit_attn_fwd_seg(qkv, plan, out, lse)
    ops.vit_attn_bwd_seg(qkv, dout, out, lse, plan, dqkv)
    assert torch.equal(_bits(dqkv), _bits(torch.cat([s[4] for s in segs])))


def test_attention_backward_vs_fp64(ops):
    """the (down, 145) case of tests/attn_any_bwd_ref.py, its three frames as three segments, under that file's bars"""
    name, ntok, frames = "down", 145, 3
    qkv, dout = (t.to(DEV) for t in AB.case(name, ntok, frames))
    plan = _plan([(1, ntok - 1)] * frames)
    out = torch.empty(frames * ntok, 384, dtype=BF16, device=DEV)
    lse = torch.empty(6 * frames * ntok, dtype=F32, device=DEV)
    dqkv = torch.full((frames * ntok, 1152), NAN, dtype=BF16, device=DEV)
    ops.vit_attn_fwd_seg(qkv, plan, out, lse)
    ops.vit_attn_bwd_seg(qkv, dout, out, lse, plan, dqkv)
    got, bars = AR.rel_l2_parts(dqkv, AR.attn_bwd_fp64(qkv, dout, frames, ntok)), AB.bars(name, ntok)
    print("down 145:", " ".join(f"{p} {g:.3e} / {b:.3e}" for p, g, b in zip(("dq", "dk", "dv"), got, bars)))
    assert torch.isfinite(dqkv.float()).all()
    for p, g, b in zip(("dq", "dk", "dv"), got, bars):
        parity_log(f"vit_seg_bwd_attn_down_145_{p}", g / b, 1.0)
        assert g <= b, (p, g, b)


# ------------------------------------------------------------------------------------------------ 2. embedding backward
def test_embedding_backward_vs_the_restatement(ops):
    from sais_amd.vit_seg import axis_taps_f32
    grids = B.grids_of(B.EMBED_FRAMES)
    plan = _plan(grids)
    assert plan.nseg == 8 and any(int(t) < 0 for t in plan.segs["tap_y"])          # the 14 x 14 frame takes the table itself
    dx = rnd(plan.M, 384, seed=81).to(DEV)
    cls0, pos0 = rnd(384, seed=82), rnd(197, 384, seed=83)                        # the gradients accumulate onto these

    def run():
        dcls, dpos = cls0.to(DEV), pos0.to(DEV)
        dpatch = torch.full((plan.NP + 2, 384), NAN, dtype=BF16, device=DEV)
        ops.vit_embed_bwd_seg(dx, plan, dcls, dpos, dpatch)
        torch.cuda.synchronize()
        return dcls, dpos, dpatch
    dcls, dpos, dpatch = run()
    rows = torch.from_numpy(B.patch_rows(grids)).to(DEV)
    assert torch.equal(_bits(dpatch[:plan.NP]), _bits(dx[rows].to(BF16))) and torch.isnan(dpatch[plan.NP:].float()).all()
    # the restatement on the kernel's own inputs: f32 dx, the f32 tap matrices
    rc, rp, terms, mag = B.embed_bwd(dx.cpu().numpy(), grids, axis=axis_taps_f32)
    assert terms[0] == 8 and terms[1:].min() >= 1
    s_cls, s_pos = cls0.double().numpy(), pos0.double().numpy()
    bound = B.bound(terms, mag, B.U24, s_pos)
    ratio = np.abs(dpos.cpu().numpy().astype(np.float64) - (s_pos + rp)) / bound
    rcls = np.abs(dcls.cpu().numpy().astype(np.float64) - (s_cls + rc)) / B.bound(terms[0], mag[:1], B.U24, s_cls)[0]
    print(f"dpos {ratio.max():.3f}, dcls {rcls.max():.3f} of the bound; terms per row {terms.min()} .. {terms.max()}")
    parity_log("vit_seg_bwd_dpos_ratio", float(ratio.max()), 1.0)
    parity_log("vit_seg_bwd_dcls_ratio", float(rcls.max()), 1.0)
    assert ratio.max() <= 1.0 and rcls.max() <= 1.0
    again = run()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((dcls, dpos, dpatch[:plan.NP]), (again[0], again[1], again[2][:plan.NP])))


def test_cls_scatter_and_row_expansion(ops):
    grids = B.grids_of(B.EMBED_FRAMES)
    plan = _plan(grids)
    src = rnd(plan.nseg, 384, seed=84).to(DEV)
    dst = torch.full((plan.M + 3, 384), SENT, dtype=F32, device=DEV)
    ops.vit_cls_scatter_seg(src, plan, dst)
    back = torch.empty_like(src)
    ops.vit_cls_gather_seg(dst, plan, back)
    assert torch.equal(back, src)
    first = torch.zeros(plan.M + 3, dtype=torch.bool, device=DEV)
    first[torch.from_numpy(plan.segs["row0"].astype(np.int64)).to(DEV)] = True
    assert (dst[~first] == SENT).all()
    per = rnd(2 * DEPTH, plan.nseg, seed=85).to(DEV)
    rows = ops.vit_rows_expand_seg(per, plan)
    want = torch.repeat_interleave(per, torch.tensor(plan.ntoks, device=DEV), dim=1)
    assert rows.shape == (2 * DEPTH, plan.M) and torch.equal(rows, want)


# ------------------------------------------------------------------------------------------------ 3. the model at depth 2
def _model(drop_path=0.0, seed=22):
    from sais_amd import vit
    sd = synth.vit_state_dict(seed=seed, depth=DEPTH)
    model = vit.vit_small(patch_size=16, depth=DEPTH, drop_path_rate=drop_path)
    model.load_state_dict(sd)
    return model.to(DEV).train(), sd


def _items(spec, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(f, 3, h, w, generator=g) for f, h, w in spec]


@pytest.mark.parametrize("name,spec,drop_path", [("list", B.MODEL_LIST, 0.0), ("big", B.MODEL_BIG, 0.1)])
def test_forward_on_a_list_under_grad_vs_oracle(name, spec, drop_path):
    from oracle import dino_oracle as do
    from sais_amd import ops
    model, sd = _model(drop_path)
    items = _items(spec, 90 + len(spec))
    nfr = sum(x.shape[0] for x in items)
    assert (B.rows_of(spec) >= ops.ROW_GEMM_MIN_M) == (name == "big")
    wv = rnd(nfr, 384, seed=16)
    model.zero_grad()
    rep = model([x.to(DEV) for x in items])
    assert rep.shape == (nfr, 384) and rep.dtype == F32 and rep.requires_grad
    saved = rep.grad_fn.saved                                     # (the autograd node is the ctx of _ViTFn)
    assert saved["seg"] is not None and saved["seg"].nseg == nfr and saved["streaming"] and not saved["pruned"]
    (rep * wv.to(DEV)).sum().backward()
    dp = None
    if drop_path > 0:                                             # one draw per (frame, branch), in list order
        dp = model.last_droppath_frame_scales.double().cpu()
        assert dp.shape == (2 * DEPTH, nfr) and (dp == 0).any() and (dp > 0).any()
        rows = model.last_droppath_scales
        assert torch.equal(rows, torch.repeat_interleave(model.last_droppath_frame_scales,
                                                         torch.tensor(saved["seg"].ntoks, device=DEV), dim=1))
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    refs, at = [], 0
    for x in items:                                               # the oracle item by item, with the kernels' draws of its frames
        refs.append(do.vit_forward_res(leaves, x.double(), depth=DEPTH, droppath=None if dp is None else dp[:, at:at + x.shape[0]]))
        at += x.shape[0]
    ref = torch.cat(refs)
    (ref * wv.double()).sum().backward()
    ferr = (rep.detach().double().cpu() - ref.detach()).abs().max().item() / ref.abs().max().item()
    errs = {n: rel(p.grad, leaves[n].grad) for n, p in model.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"{name}: features {ferr:.3e} of max|ref|, worst gradient rel-L2 {errs[worst]:.3e} ({worst})")
    parity_log(f"vit_seg_bwd_feat_{name}", ferr, 2e-2)
    parity_log(f"vit_seg_bwd_grad_rel_l2_{name}", errs[worst], 2e-2)
    for n in ("cls_token", "pos_embed", "patch_embed.proj.weight"):
        parity_log(f"vit_seg_bwd_grad_rel_l2_{name}_{n}", errs[n], 2e-2)
    assert ferr < 2e-2
    for n, e in errs.items():
        assert e < 2e-2, (n, e)


# ------------------------------------------------------------------------------------------------ 4. forward independence
def test_a_frames_row_does_not_depend_on_the_rest_of_the_list():
    model, _ = _model()
    a, b, c, d = (x.to(DEV) for x in _items(((1, 48, 80), (2, 64, 64), (1, 224, 224), (1, 32, 112)), 95))
    one = model([a, b, c]).detach()
    two = model([d, c, b[1:], a, d]).detach()
    assert torch.equal(two[1], one[3]) and torch.equal(two[2], one[2]) and torch.equal(two[3], one[0])
    assert torch.equal(two[0], two[4])
    with torch.no_grad():                                         # without gradients: the bits of the retrieval call
        assert torch.equal(model([a, b, c]), model.retrieval_features([a, b, c], cls_only=True))
        assert model((a, b, c)).shape == (4, 384)


# ------------------------------------------------------------------------------------------------ 5. launch records
def _records(call):
    from sais_amd import ops
    ops.TIMER = ops.KernelTimer()
    try:
        call()
        torch.cuda.synchronize()
        return {tag: len(v) for tag, v in ops.TIMER.recs.items()}
    finally:
        ops.TIMER = None


def test_launch_records_do_not_depend_on_the_shapes():
    model, _ = _model()

    def step(x):
        model.zero_grad()
        model(x).sum().backward()
    two = [x.to(DEV) for x in _items(B.LAUNCH_2, 96)]
    five = [x.to(DEV) for x in _items(B.LAUNCH_5, 97)]
    a, b = _records(lambda: step(two)), _records(lambda: step(five))
    assert a == b, (a, b)
    assert a["vit_attn_bwd_seg"] == DEPTH and a["vit_attn_fwd_seg"] == DEPTH
    assert not {"vit_attn_bwd_any", "vit_attn_fwd_any", "vit_embed_bwd", "pos_interp_bwd", "vit_attn_bwd", "vit_attn_fwd"} & set(a)
    single = _records(lambda: step(five[0]))
    # (a single tensor keeps its CLS-only last block: the streaming pair runs in the blocks below it)
    assert single["vit_attn_bwd_any"] == DEPTH - 1 and not any("_seg" in t for t in single)


# ------------------------------------------------------------------------------------------------ 6. the DINO step
def test_dino_train_step_segmented_at_128_64_vs_oracle(monkeypatch):
    """test_dino_train_step_at_128_64_vs_oracle with the student's crops as segments of one pass, under its bars"""
    from oracle import dino_oracle as do
    from sais_amd import dino
    out_dim, n_local, Bn = 1024, 2, 2
    sd = {"backbone." + k: v for k, v in synth.vit_state_dict(seed=23, depth=DEPTH).items()}
    sd.update({"head." + k: v for k, v in synth.dino_head_state_dict(seed=24, out_dim=out_dim).items()})
    monkeypatch.delenv("SAIS_DINO_SEGMENTED", raising=False)
    student, teacher = dino.build_student_teacher(out_dim=out_dim, drop_path_rate=0.0, device=DEV, depth=DEPTH)
    assert student.segmented is False and teacher.segmented is False
    monkeypatch.setenv("SAIS_DINO_SEGMENTED", "1")
    assert dino.build_student_teacher(out_dim=out_dim, drop_path_rate=0.0, device=DEV, depth=1)[0].segmented is True
    student.load_state_dict(sd)
    teacher.load_state_dict(student.state_dict())
    student.train()
    student.segmented = True
    loss_mod = dino.DINOLoss(out_dim, n_local + 2, 0.04, 0.07, 3, 10).to(DEV)
    opt = dino.DINOOptimizer(student, teacher)
    crops = synth.dino_crops(seed=340, B=Bn, n_local=n_local, gsize=128, lsize=64)
    dev_crops = [c.to(DEV) for c in crops]
    with pytest.raises(NotImplementedError, match="segmented"):
        dino.GraphedTrainStep(student, teacher, loss_mod, opt, dev_crops)
    lr_s, wd_s, mom_s = np.full(4, 1e-4), np.full(4, 0.05), np.full(4, 0.9)
    from sais_amd import ops
    ops.TIMER = ops.KernelTimer()
    try:
        loss, norms = dino.train_step(student, teacher, loss_mod, opt, dev_crops, 0, 1, lr_s, wd_s, mom_s, clip_grad=0.05,
                                      freeze_last_layer=0)
        torch.cuda.synchronize()
        tags = set(ops.TIMER.recs)
    finally:
        ops.TIMER = None
    assert "vit_attn_bwd_seg" in tags and "vit_attn_bwd_any" not in tags
    st = do.TrainState(sd)
    ref = do.train_step(st, crops, 0, 1, lr_s, wd_s, mom_s, loss_mod.teacher_temp_schedule, 0.05, 0, n_local, depth=DEPTH)
    lerr = abs(loss.item() - ref["loss"]) / ref["loss"]
    parity_log("vit_seg_bwd_step_loss_rel", lerr, 2e-3)
    assert math.isfinite(loss.item()) and lerr < 2e-3
    names = [n for n, p in student.named_parameters() if p.requires_grad]
    got_n, ref_n = norms.double().cpu().numpy(), np.array([ref["norms"][n] for n in names])
    nerr = np.abs(got_n - ref_n) / np.maximum(ref_n, 1e-12)
    parity_log("vit_seg_bwd_step_grad_norm_rel", float(nerr.max()), 5e-2)
    assert nerr.max() < 5e-2, [n for n, e in zip(names, nerr) if e > 5e-2]
    worst = 0.0
    for who, mod in (("backbone.", student.backbone), ("head.", student.head)):
        for n, p in mod.named_parameters():
            if p.requires_grad:
                e = rel(mod.flat.g(n), ref["grads"][who + n])
                worst = max(worst, e)
                assert e < 3e-2, (who + n, e)
    parity_log("vit_seg_bwd_step_grad_rel_l2", worst, 3e-2)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals():
    from sais_amd import _lib as L
    from sais_amd.vit import vit_small
    model, _ = _model()
    x = torch.zeros(1, 3, 32, 48, device=DEV)
    v8 = vit_small(patch_size=8, depth=1).to(DEV)
    with pytest.raises(NotImplementedError, match="patch-16 pass"):
        v8([x])
    with torch.no_grad(), pytest.raises(NotImplementedError, match="patch-16 pass"):
        v8([x])
    for empty in ([], ()):
        with pytest.raises(ValueError, match="empty list"):
            model(empty)
    with pytest.raises(L.SaisHipError, match="needs a device tensor"):
        model([x, torch.zeros(1, 3, 32, 32)])
    with pytest.raises(ValueError, match="4098 tokens"):
        model([x, torch.zeros(1, 3, 16, 16 * 4097, device=DEV)])
    with pytest.raises(ValueError, match="multiples of 16"):
        model([x, torch.zeros(1, 3, 40, 32, device=DEV)])
    with pytest.raises(NotImplementedError):                      # the segmented pass stays a streaming patch-16 pass
        model._forward_kernels([x], save=True, streaming=False, seg=model._seg_plan([x]))
