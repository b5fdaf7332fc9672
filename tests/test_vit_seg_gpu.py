"""Frames of different sizes in one backbone pass (csrc/attn_seg.hip, sais_amd/vit_seg.py) on the MI355X.  Case lists and host
restatements: tests/vit_seg_ref.py.

  * attention: every segment's `out` and `lse` bit-equal to sais_vit_attn_fwd_any on that frame alone, both workgroup forms,
    permuted orders, sentinel rows and a wide row stride
  * sais_patchify_seg: bit-equal to sais_patchify_rect per frame
  * embedding: exact on exactly representable inputs where nothing is interpolated (the bar the patch-GEMM tests of the
    single-tensor path use: equality with fp64); the interpolated table alone within 16 x 2^-24 x sum |m| |p| per element (a
    sixteen-term f32 sum); rows that add an interpolated row to a patch value: that bound plus one rounding of the result
  * model at depth 2, multi_scale on a list: the project's one feature bar, FEAT_REL x max|ref|, against the fp64 oracle
  * launch records, refusals, the tool with --mixed_batch true
"""
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_ref as AR
import gemm_ref as G
import parity
import synth
import vit_seg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from sais_amd import ops as o
    return o


def _plan(grids):
    from sais_amd.vit_seg import SegPlan
    return SegPlan(grids).to_device(DEV)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. attention, bit for bit
@functools.lru_cache(maxsize=None)
def _segment(layout, ntok, variant=0):
    """(qkv bf16 [ntok, 1152], out, lse of sais_vit_attn_fwd_any on this frame alone): computed once per (layout, ntok, draw)"""
    from sais_amd import ops
    qkv = AR.layouts(layout, 1, ntok, 4000 + ntok + 10000 * variant).to(DEV)
    out = torch.full((ntok, AR.DM), NAN, dtype=BF16, device=DEV)
    lse = torch.full((1, AR.NH, ntok), NAN, dtype=F32, device=DEV)
    ops.vit_attn_fwd_any(qkv, 1, ntok, out, lse)
    assert not torch.isnan(out.float()).any() and not torch.isnan(lse).any()
    return qkv, out, lse


def _attn_case(ops, layout, ntoks, ldq=1160, ldo=392):
    plan = _plan([(1, n - 1) for n in ntoks])
    assert plan.qtile == R.qtile(ntoks)
    M = plan.M
    seen, draws = {}, []                                       # segments of one token count hold different draws (five at most)
    for n in ntoks:
        draws.append(seen.get(n, 0) % 5)
        seen[n] = seen.get(n, 0) + 1
    qkv = torch.full((M + R.SENTINEL_ROWS, ldq), NAN, dtype=BF16, device=DEV)
    for (row0, n, *_), s, k in zip(R.layout(plan.grids), ntoks, draws):
        qkv[row0:row0 + n, :1152] = _segment(layout, s, k)[0]
    out = torch.full((M + R.SENTINEL_ROWS, ldo), NAN, dtype=BF16, device=DEV)
    lse = torch.full((6 * (M + R.SENTINEL_ROWS),), NAN, dtype=F32, device=DEV)
    ops.vit_attn_fwd_seg(qkv[:, :1152], plan, out[:, :384], lse)
    torch.cuda.synchronize()
    for (row0, n, *_), s, k in zip(R.layout(plan.grids), ntoks, draws):
        _, want, want_lse = _segment(layout, s, k)
        assert torch.equal(_bits(out[row0:row0 + n, :384]), _bits(want)), (layout, s, "out")
        assert torch.equal(_bits(lse[6 * row0:6 * (row0 + n)]), _bits(want_lse.reshape(-1))), (layout, s, "lse")
    assert torch.isnan(out[M:].float()).all() and torch.isnan(out[:, 384:].float()).all() and torch.isnan(lse[6 * M:]).all()
    without = torch.full_like(out, NAN)                        # the optional lse left out: the same out
    ops.vit_attn_fwd_seg(qkv[:, :1152], plan, without[:, :384])
    assert torch.equal(_bits(without[:M, :384]), _bits(out[:M, :384]))


@pytest.mark.parametrize("order", range(len(R.ATTN_ORDERS)))
@pytest.mark.parametrize("layout", R.ATTN_LAYOUTS)
def test_attention_segments_equal_the_frame_alone(ops, layout, order):
    """eight token counts in one call (32-query form), in order and in two permutations"""
    ntoks = [R.ATTN_NTOKS[i] for i in R.ATTN_ORDERS[order]]
    assert R.qtile(ntoks) == 32
    _attn_case(ops, layout, ntoks)


@pytest.mark.parametrize("layout", ("rand", "planted"))
def test_attention_many_segments_take_the_64_query_form(ops, layout):
    assert R.qtile(R.ATTN_MANY) == 64 and AR.stream_waves(1, 65) == 2      # alone the frame takes the other form: same bits
    _attn_case(ops, layout, list(R.ATTN_MANY))


@pytest.mark.parametrize("layout", ("rand", "offp"))
def test_attention_one_segment_at_the_cap(ops, layout):
    _attn_case(ops, layout, list(R.ATTN_CAP))


# ------------------------------------------------------------------------------------------------ 2. the patch gather
def test_patchify_seg_equals_patchify_rect_per_frame(ops):
    frames = [torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(h * 1000 + w)).to(DEV) for h, w in R.PATCHIFY_FRAMES]
    plan = _plan([(h // 16, w // 16) for h, w in R.PATCHIFY_FRAMES])
    pixels = torch.cat([f.reshape(-1) for f in frames])
    assert pixels.numel() == plan.npix
    got = torch.full((plan.NP + 3, 768), NAN, dtype=BF16, device=DEV)
    ops.patchify_seg(pixels, plan, got[:plan.NP])
    row = 0
    for f in frames:
        n = (f.shape[2] // 16) * (f.shape[3] // 16)
        want = torch.empty(n, 768, dtype=BF16, device=DEV)
        ops.patchify_rect(f, want)
        assert torch.equal(_bits(got[row:row + n]), _bits(want)), tuple(f.shape)
        row += n
    assert row == plan.NP and torch.isnan(got[plan.NP:].float()).all()


# ------------------------------------------------------------------------------------------------ 3. the embedding
EMBED_GRIDS = [(3, 5), (14, 14), (1, 1), (13, 15), (5, 3), (1, 7), (14, 13)]


def _embed(ops, plan, pe, cls, pos):
    x = torch.full((plan.M + 2, 384), NAN, dtype=F32, device=DEV)
    ops.vit_embed_seg(pe, cls, pos, plan, x)
    torch.cuda.synchronize()
    assert torch.isnan(x[plan.M:]).all()
    return x[:plan.M].cpu().numpy()


def test_interpolated_table_alone(ops):
    """patch_out = 0, cls = 0: the rows are the interpolated table, 0 + p exactly.  Sixteen-term f32 sums: 16 x 2^-24 x
    sum |m| |p| per element (the f32 rounding of the two tap matrices, 2 x 2^-24, included)."""
    plan = _plan(EMBED_GRIDS)
    pos = synth.vit_state_dict(seed=0, depth=1)["pos_embed"][0].contiguous()
    got = _embed(ops, plan, torch.zeros(plan.NP, 384, device=DEV), torch.zeros(384, device=DEV), pos.to(DEV))
    worst = 0.0
    for (row0, ntok, gh, gw, _) in R.layout(EMBED_GRIDS):
        ref, mag = R.pos_rows(pos.double().numpy(), gh, gw)
        assert np.array_equal(got[row0], pos[0].numpy())
        err = np.abs(got[row0 + 1:row0 + ntok].astype(np.float64) - ref)
        if (gh, gw) == (14, 14):
            assert err.max() == 0.0
            continue
        ratio = float((err / (16 * U24 * mag)).max())
        print(f"grid {gh} x {gw}: {ratio:.3f} of the bound")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (gh, gw, ratio)
    parity.parity_log("vit_seg_pos_interp_ratio", worst, 1.0)


def test_token_rows_vs_fp64(ops):
    """cls + pos and patch W + b + pos against fp64.  Inputs in {-1, 0, 1} (patch GEMM, as the patch-GEMM tests of the
    single-tensor path) and small integers (pos, cls): the GEMM, the CLS rows and the rows of a 14 x 14 frame are exact; a row
    with an interpolated positional row p~ is (acc + p~) rounded once: |err| <= 16 x 2^-24 sum |m| |p| + 2^-24 |ref|."""
    from sais_amd import _lib as L
    plan = _plan(EMBED_GRIDS)
    a, w, bias = (t.to(DEV) for t in G.tern(plan.NP, 384, 768))
    pos = G.tern_resid(197, 384).to(DEV)
    cls = G.tern_resid(1, 384, seed=9)[0].to(DEV)
    pe = torch.empty(plan.NP, 384, dtype=F32, device=DEV)
    ops.gemm_nt(a, w, L.EPI_BIAS_F32, pe, bias=bias)
    acc = (G.mm64(a, w) + bias.double()).cpu().numpy()
    assert np.array_equal(pe.cpu().numpy().astype(np.float64), acc)
    got = _embed(ops, plan, pe, cls, pos).astype(np.float64)
    worst = 0.0
    for s, (row0, ntok, gh, gw, _) in enumerate(R.layout(EMBED_GRIDS)):
        assert np.array_equal(got[row0], (cls.double() + pos[0].double()).cpu().numpy())
        p, mag = R.pos_rows(pos.double().cpu().numpy(), gh, gw)
        ref = acc[row0 - s:row0 - s + ntok - 1] + p
        err = np.abs(got[row0 + 1:row0 + ntok] - ref)
        if (gh, gw) == (14, 14):
            assert err.max() == 0.0
            continue
        worst = max(worst, float((err / (16 * U24 * mag + U24 * np.abs(ref) + 1e-300)).max()))
    print(f"token rows: {worst:.3f} of the bound")
    parity.parity_log("vit_seg_embed_ratio", worst, 1.0)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 4. the model at depth 2
DEPTH = 2


@functools.lru_cache(maxsize=None)
def _sd64():
    return {k: v.double() for k, v in synth.vit_state_dict(seed=0, depth=DEPTH).items()}


@functools.lru_cache(maxsize=None)
def _vit():
    from sais_amd.vit import vit_small
    m = vit_small(patch_size=16, depth=DEPTH)
    m.load_state_dict(synth.vit_state_dict(seed=0, depth=DEPTH), strict=True)
    return m.to(DEV).eval()


def _items(spec, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(f, 3, h, w, generator=g) for f, h, w in spec]


def _oracle_tokens(x, depth):
    """norm(tokens) after `depth` blocks in fp64 [F, ntok, 384], from the oracle's own pieces; its CLS row is
    oracle.dino_oracle.vit_forward_res(depth=depth) (asserted)"""
    from oracle import dino_oracle as do, sais_oracle as so
    sd = _sd64()
    with torch.no_grad():
        tok = so.vit_patch_embed(sd, x)
        t = torch.cat((sd["cls_token"].expand(tok.shape[0], -1, -1), tok), dim=1)
        t = t + do.interpolate_pos_encoding(sd["pos_embed"], tok.shape[1], x.shape[2], x.shape[3])
        for i in range(depth):
            t = so.vit_block(sd, i, t)
        t = F.layer_norm(t, (384,), sd["norm.weight"], sd["norm.bias"], 1e-6)
        assert float((t[:, 0] - do.vit_forward_res(sd, x, depth=depth)).abs().max()) <= 1e-12
    return t


def _rel(name, got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    err, scale = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max()), float(np.abs(ref).max())
    print(f"{name}: max err {err:.3e} = {err / scale:.3e} max|ref|")
    parity.parity_log("vit_seg_" + name, err / scale, R.FEAT_REL)
    assert np.isfinite(err) and err <= R.FEAT_REL * scale, (name, err, scale)


@functools.lru_cache(maxsize=None)
def _model_case():
    items = _items(R.MODEL_LIST, 51)
    return items, [[_oracle_tokens(x.double(), d) for x in items] for d in (1, 2)]      # [after block 0, after block 1][item]


def test_retrieval_features_on_a_list_vs_the_oracle():
    items, ref = _model_case()
    vit = _vit()
    feats = vit.retrieval_features([x.to(DEV) for x in items], cls_only=True)
    assert feats.shape == (sum(x.shape[0] for x in items), 384) and feats.dtype == F32
    want = torch.cat([r[:, 0] for r in ref[1]]).numpy()
    _rel("retrieval_list", feats.cpu().numpy(), want)
    again = vit.retrieval_features(tuple(x.to(DEV) for x in items), cls_only=True)
    assert torch.equal(again, feats)
    # equal frames in different places of the list (items 0 and 4 are different draws; build a list that repeats one)
    twice = vit.retrieval_features([items[0].to(DEV), items[3].to(DEV), items[0].to(DEV)], cls_only=True)
    assert torch.equal(twice[0], twice[2])


def test_dense_features_on_a_list_vs_the_oracle():
    items, ref = _model_case()
    dense = _vit().dense_features([x.to(DEV) for x in items], 2)
    assert len(dense) == 2 and all(len(layer) == len(items) for layer in dense)
    for j in range(2):
        for i, (x, y) in enumerate(zip(items, dense[j])):
            assert y.shape == (x.shape[0], 1 + (x.shape[2] // 16) * (x.shape[3] // 16), 384) and y.dtype == F32
            _rel(f"dense_list_layer{j}", y.cpu().numpy(), ref[j][i].numpy())


def test_model_list_in_the_fused_gemm_layernorm_form():
    """46 frames of 208 x 240: 9016 stacked rows, from 8192 on the GEMMs carry the following LayerNorm"""
    from sais_amd import ops
    (f, h, w), = R.MODEL_BIG
    assert f * (1 + (h // 16) * (w // 16)) >= ops.ROW_GEMM_MIN_M
    x = _items(R.MODEL_BIG, 52)[0]
    vit = _vit()
    feats = vit.retrieval_features([x[:20].to(DEV), x[20:].to(DEV)], cls_only=True)
    dense = vit.dense_features([x[:20].to(DEV), x[20:].to(DEV)], 1)[0]
    keep = [0, 19, 20, 45]                                      # frames are independent: the oracle runs on four of them
    ref = _oracle_tokens(x[keep].double(), DEPTH).numpy()
    _rel("retrieval_list_fused", feats[keep].cpu().numpy(), ref[:, 0])
    _rel("dense_list_fused", torch.cat(dense)[keep].cpu().numpy(), ref)


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


def test_launch_records_do_not_depend_on_frames_or_shapes():
    vit = _vit()
    three = [x.to(DEV) for x in _items(R.LAUNCH_3, 53)]
    nine = [x.to(DEV) for x in _items(R.LAUNCH_9, 54)]
    assert len({tuple(x.shape) for x in nine}) == 9
    a = _records(lambda: vit.retrieval_features(three, cls_only=True))
    b = _records(lambda: vit.retrieval_features(nine, cls_only=True))
    assert a == b and sum(a.values()) == sum(b.values())
    assert a["vit_attn_fwd_seg"] == DEPTH and "vit_attn_fwd_any" not in a
    single = _records(lambda: vit.retrieval_features(nine[0], cls_only=True))
    assert single["vit_attn_fwd_any"] == DEPTH and not any("_seg" in t for t in single)


# ------------------------------------------------------------------------------------------------ 6. multi_scale on a list
def _multi_scale_oracle(x):
    """utils.multi_scale of ONE image in fp64: the mean of the oracle's features of the three scales, over its norm"""
    from oracle import dino_oracle as do
    import retrieval_ref as RR
    v = 0
    for s in RR.SCALES:
        inp = x.double() if s == 1 else F.interpolate(x.double(), scale_factor=s, mode="bilinear", align_corners=False)
        with torch.no_grad():
            v = v + do.vit_forward_res(_sd64(), torch.from_numpy(np.ascontiguousarray(RR.crop16(inp.numpy()))), depth=DEPTH)
    v = v / 3
    return (v / v.norm()).numpy()


def test_multi_scale_on_a_list():
    from sais_amd import retrieval
    g = torch.Generator().manual_seed(55)
    imgs = [torch.randn(1, 3, h, w, generator=g) for h, w in R.MULTI_SCALE_SIZES]
    model = retrieval.cls_features(_vit())
    got = retrieval.multi_scale([x.to(DEV) for x in imgs], model)
    assert got.shape == (4, 384)
    for i, x in enumerate(imgs):
        _rel("multi_scale_list", got[i:i + 1].cpu().numpy(), _multi_scale_oracle(x))
    assert float((got.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    # a row does not change when the other images of the list change
    others = [torch.randn(1, 3, 48, 112, generator=g), torch.randn(1, 3, 130, 40, generator=g)]
    again = retrieval.multi_scale([others[0].to(DEV), imgs[2].to(DEV), others[1].to(DEV), imgs[0].to(DEV)], model)
    assert torch.equal(again[1], got[2]) and torch.equal(again[3], got[0])


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals():
    from sais_amd import _lib as L
    from sais_amd.vit import vit_small
    vit = _vit()
    x = torch.zeros(1, 3, 32, 48, device=DEV)
    with pytest.raises(NotImplementedError):
        vit.retrieval_features([x], cls_only=False)
    with pytest.raises(NotImplementedError):
        vit.retrieval_features([x])                            # the default asks for the GeM half too
    v8 = vit_small(patch_size=8, depth=1).to(DEV).eval()
    with pytest.raises(NotImplementedError):
        v8.retrieval_features([x], cls_only=True)
    with pytest.raises(NotImplementedError):
        v8.dense_features([x], 1)
    with pytest.raises(ValueError, match="4098 tokens"):
        vit.retrieval_features([x, torch.zeros(1, 3, 16, 16 * 4097, device=DEV)], cls_only=True)
    with pytest.raises(ValueError):
        vit.retrieval_features([], cls_only=True)
    with pytest.raises(ValueError):
        vit.dense_features([], 1)
    with pytest.raises(L.SaisHipError, match="needs a device tensor"):
        vit.retrieval_features([x, torch.zeros(1, 3, 32, 32)], cls_only=True)
    with pytest.raises(ValueError, match="multiples of 16"):
        vit.dense_features([x, torch.zeros(1, 3, 40, 32, device=DEV)], 1)
    with pytest.raises(ValueError):
        vit.dense_features([x], 3)                              # depth 2


# ------------------------------------------------------------------------------------------------ 8. the tool
def test_tool_mixed_batch(tmp_path):
    """eval_image_retrieval.py --gpu_loader true --mixed_batch true on the synthetic roxford folder of test_thumbnail_gpu.py
    (eight distinct thumbnail shapes at --imsize 96) against the per-image --gpu_loader run"""
    import test_thumbnail_gpu as TG
    root = str(tmp_path / "data")
    os.makedirs(root)
    TG._write_roxford(root)
    from sais_amd.retrieval import OxfordParisDataset
    shapes = {tuple(OxfordParisDataset(root, "roxford5k", split, imsize=96)[i][0].shape)
              for split, n in (("train", len(TG.FOLDER) - 2), ("query", 2)) for i in range(n)}
    assert len(shapes) >= 6, shapes
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"teacher": {k: v.cpu() for k, v in TG.backbone().state_dict().items()}}, ckpt)
    runs = {}
    for leg, extra in (("single", []), ("mixed", ["--mixed_batch", "true"])):
        dump = str(tmp_path / leg)
        text = TG._run_tool("--data_path", root, "--dataset", "roxford5k", "--imsize", "96", "--pretrained_weights", ckpt,
                            "--dump_features", dump, "--gpu_loader", "true", "--gpu_loader_batch", "5", *extra)
        lines = re.findall(r"^>> .*$", text, flags=re.M)
        assert len(lines) == 2, text
        values = [float(v) for ln in lines for v in re.findall(r"-?\d+\.\d*|nan|inf", ln.split(":", 1)[1])]
        assert values and np.isfinite(values).all(), lines
        runs[leg] = (lines, torch.cat([torch.load(os.path.join(dump, "trainfeat.pth")),
                                       torch.load(os.path.join(dump, "queryfeat.pth"))]).double())
        print(leg, lines)
    single, mixed = runs["single"][1], runs["mixed"][1]
    assert mixed.shape == single.shape == (len(TG.FOLDER), 384)
    diff = float((mixed - single).abs().max())
    print(f"mixed vs per-image dump: max |d| = {diff:.3e} (rows are unit vectors)")
    parity.parity_log("vit_seg_tool_mixed_vs_single_abs", diff, R.FEAT_REL)
    assert diff <= R.FEAT_REL
