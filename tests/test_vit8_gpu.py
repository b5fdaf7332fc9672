"""The patch-8 backbone (ViT-S/8, inference) on a real MI355X: the two kernels of csrc/vit8.hip, the patch GEMM at K = 192 on both
NT kernels, the backbone against the reference's recorded outputs (tests/golden/make_golden_vit8.py), the consistency of its
passes with each other and one tool end to end.

Bars (stated here, used below):
  * sais_patchify_rect8: bit-equal to the unfold-built patches cast to bf16 (torch's cast rounds to nearest even)
  * patch GEMM: ternary operands of tests/gemm_ref.py, bit-equal to fp64
  * sais_vit_attn_cls_fwd_any: attn_ref.out_bound around row 0 of attn_ref.attn_fp64 (derived there; this kernel keeps P in f32
    like attn_cls.hip, whose error that docstring places inside the same bound); bit-equal between launches and launch sizes
  * features: the project's one feature bar, vit8_ref.FEAT_REL * max|ref|
  * CLS attention: vit8_ref.ATTN_TOL max-abs, row sums within vit8_ref.ROWSUM_TOL of 1
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import attn_ref as AR
import gemm_ref as G
import parity
import vit8_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    from sais_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from sais_amd import _lib
    return _lib


def _model():
    from sais_amd.vit import vit_small
    m = vit_small(patch_size=8)
    m.load_state_dict(R.state_dict(seed=0), strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def vit():
    return _model()


@pytest.fixture(scope="module")
def g():
    return R.golden()


def rel(name, got, ref, tag):
    """max|got - ref| / max|ref| under the feature bar"""
    ref = np.asarray(ref, dtype=np.float64)
    err, scale = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max()), float(np.abs(ref).max())
    print(f"{name} {tag}: max err {err:.3e} = {err / scale:.3e} max|ref|")
    parity.parity_log(f"vit8_{tag}_{name}", err / scale, R.FEAT_REL)
    assert np.isfinite(err) and err <= R.FEAT_REL * scale, (name, tag, err, scale)


# ------------------------------------------------------------------------------------------------ 1. the 8 x 8 gather
@pytest.mark.parametrize("F,H,W", [(1, 8, 8), (2, 64, 88), (3, 224, 224)])
def test_patchify_rect8_bits(ops, F, H, W):
    x = dev(R.frames(F, H, W, 810 + H))
    n = F * (H // 8) * (W // 8)
    want = x.unfold(2, 8, 8).unfold(3, 8, 8).permute(0, 2, 3, 1, 4, 5).reshape(n, 192).to(BF16)      # [F, gy, gx, c, py, px]
    out = torch.full((n + 3, 192), NAN, dtype=BF16, device=DEV)
    ops.patchify_rect8(x, out)
    assert torch.equal(out[:n].view(torch.int16), want.view(torch.int16))
    assert torch.isnan(out[n:]).all()


# ------------------------------------------------------------------------------------------------ 2. the patch GEMM at K = 192
@pytest.mark.parametrize("M", [2 * 784, 11 * 784])
def test_patch_gemm_k192(ops, L, M):
    """EPI_PATCH_F32 at K = 192 (three K steps) on the four-wave kernel (M = 1568) and the eight-wave one (M = 8624 >= 8192):
    token rows exact, CLS rows untouched"""
    N, K = 384, 192
    assert (M >= G.W8P_MIN_M) == (M == 11 * 784)
    a, w, bias = (t.to(DEV) for t in G.tern(M, N, K))
    acc = G.mm64(a, w)
    Fr = M // 784
    pos = G.tern_resid(785, N).to(DEV)
    want = (acc + bias.double()).view(Fr, 784, N) + pos[1:].double()
    assert G.f32_exact(want)
    for _ in range(2):
        tok = torch.full((Fr, 785, N), NAN, device=DEV)
        ops.gemm_nt(a, w, L.EPI_PATCH_F32, tok, bias=bias, aux=pos, grp=(784, 785, 1))
        assert torch.equal(tok[:, 1:].double(), want)
        assert torch.isnan(tok[:, 0]).all()


# ------------------------------------------------------------------------------------------------ 3. CLS-query attention
@functools.lru_cache(maxsize=1)
def _cls_case(layout, ntok):
    """(qkv with NaN in the q columns of every non-CLS row, row 0 of the fp64 output and of A per frame) for 3 frames"""
    qkv = AR.layouts(layout, 3, ntok, 900 + ntok).to(DEV)
    r = AR.attn_fp64(qkv, 3, ntok)
    ref, A = r["out"].view(3, ntok, AR.DM)[:, 0].clone(), r["A"].view(3, ntok, AR.DM)[:, 0].clone()
    qkv.view(3, ntok, 3 * AR.DM)[:, 1:, :AR.DM] = NAN
    return qkv, ref, A


@pytest.mark.parametrize("ntok", [2, 63, 64, 65, 257, 785, 4097])
@pytest.mark.parametrize("layout", ["rand", "planted", "offp", "offn", "same"])
def test_attn_cls_fwd_any(ops, layout, ntok):
    """one pass of 32 keys with three idle waves, both sides of two passes, a ragged ninth pass, the 224 x 224 count and the cap;
    three frames in one launch against fp64, again (bit-equal), and frame 1 launched alone (bit-equal)"""
    qkv, ref, A = _cls_case(layout, ntok)
    out = torch.full((4, AR.DM), NAN, dtype=BF16, device=DEV)
    ops.vit_attn_cls_fwd_any(qkv, 3, ntok, out[:3])
    ratio = AR.worst_ratio(out[:3], ref, AR.out_bound(ref, A))
    print(f"{layout} ntok {ntok}: {ratio:.3f} of the bound")
    parity.parity_log(f"vit8_attn_cls_any_{layout}", ratio, 1.0)
    assert ratio <= 1.0, (layout, ntok, ratio)
    assert torch.isnan(out[3]).all()
    again = torch.full_like(out, NAN)
    ops.vit_attn_cls_fwd_any(qkv, 3, ntok, again[:3])
    assert torch.equal(again[:3].view(torch.int16), out[:3].view(torch.int16))
    alone = torch.full((2, AR.DM), NAN, dtype=BF16, device=DEV)
    ops.vit_attn_cls_fwd_any(qkv[ntok:2 * ntok], 1, ntok, alone[:1])
    assert torch.equal(alone[0].view(torch.int16), out[1].view(torch.int16)) and torch.isnan(alone[1]).all()


def test_attn_cls_fwd_any_row_strides_and_the_one_wave_kernel(ops):
    """free row strides of qkv and out; at a count both kernels take (197) the one-wave kernel agrees inside the same bound"""
    ntok = 197
    qkv, ref, A = _cls_case("rand", ntok)
    wide = torch.full((3 * ntok, 1160), NAN, dtype=BF16, device=DEV)
    wide[:, :1152] = qkv
    out = torch.full((3, 392), NAN, dtype=BF16, device=DEV)
    ops.vit_attn_cls_fwd_any(wide[:, :1152], 3, ntok, out[:, :384])
    dense = torch.empty(3, 384, dtype=BF16, device=DEV)
    ops.vit_attn_cls_fwd_any(qkv, 3, ntok, dense)
    assert torch.equal(out[:, :384].view(torch.int16), dense.view(torch.int16)) and torch.isnan(out[:, 384:]).all()
    wave = torch.empty(3, 384, dtype=BF16, device=DEV)
    ops.vit_attn_cls_fwd(qkv, 3, wave, ntok)
    assert AR.worst_ratio(wave, ref, AR.out_bound(ref, A)) <= 1.0 and AR.worst_ratio(dense, ref, AR.out_bound(ref, A)) <= 1.0


# ------------------------------------------------------------------------------------------------ 4. the backbone against the reference
@functools.lru_cache(maxsize=1)
def _case_input(name):
    _, F, H, W, seed = next(c for c in R.CASES if c[0] == name)
    return R.frames(F, H, W, seed)


@pytest.mark.parametrize("name,F,H,W,seed", R.CASES)
def test_backbone_vs_reference(vit, g, name, F, H, W, seed):
    x = _case_input(name)
    assert np.array_equal(R.digest(x), g[f"{name}_sha256"])
    xd, n, keep = dev(x), R.ntok(H, W), R.rows(H, W)
    with torch.no_grad():
        fwd = vit(xd)
    assert fwd.shape == (F, 384) and fwd.dtype == F32
    rel("forward", host(fwd), g[f"{name}_fwd"], name)
    dense = vit.dense_features(xd, 2)
    assert len(dense) == 2 and all(t.shape == (F, n, 384) for t in dense)
    for j in range(2):
        rel(f"dense{j}", host(dense[j])[:, keep], g[f"{name}_rows"][j], name)
    probe = vit.probe_features(xd, R.N_LAST)
    assert probe.shape == (F, 384 * R.N_LAST)
    rel("probe", host(probe), np.concatenate(list(g[f"{name}_cls"]), axis=1), name)
    assert torch.equal(probe[:, -384:], fwd)                          # the last slot IS forward()'s output
    attn = vit.cls_attention(xd)
    assert attn.shape == (F, 6, n)
    err = float(np.abs(host(attn).astype(np.float64) - g[f"{name}_attn"]).max())
    rs = float((attn.double().sum(-1) - 1).abs().max())
    print(f"{name} cls_attention: max abs err {err:.3e}, row sums off by {rs:.3e}")
    parity.parity_log(f"vit8_{name}_attn_abs", err, R.ATTN_TOL)
    parity.parity_log(f"vit8_{name}_attn_rowsum", rs, R.ROWSUM_TOL)
    assert err <= R.ATTN_TOL and rs <= R.ROWSUM_TOL


def test_intermediate_layers_and_refusals(vit, g):
    name, F, H, W, _ = R.CASES[0]
    xd = dev(_case_input(name))
    inter = vit.get_intermediate_layers(xd, R.N_LAST)
    assert len(inter) == R.N_LAST and all(t.shape == (F, R.ntok(H, W), 384) for t in inter)
    rel("intermediate_cls", np.stack([host(t[:, 0]) for t in inter]), g[f"{name}_cls"], name)
    for j in range(2):
        rel(f"intermediate_rows{j}", host(inter[2 + j])[:, R.rows(H, W)], g[f"{name}_rows"][j], name)
    with pytest.raises(NotImplementedError, match="training runs on patch 16"):
        vit(xd)                                                       # gradients enabled, parameters trainable
    with pytest.raises(NotImplementedError):
        vit.get_last_selfattention(xd)
    with pytest.raises(ValueError, match="6241 tokens; at most 4097"):
        vit.dense_features(torch.zeros(1, 3, 480, 832, device=DEV))
    with pytest.raises(ValueError, match="multiples of 8"):
        vit.cls_attention(torch.zeros(1, 3, 68, 88, device=DEV))


# ------------------------------------------------------------------------------------------------ 5. consistency of the passes
@pytest.mark.parametrize("name", ["c64x88", "c224x224"])
def test_cls_only_tail_matches_the_full_block(vit, monkeypatch, name):
    """forward() (CLS-only last block: the one-wave attention at 89 tokens, sais_vit_attn_cls_fwd_any at 785) against the CLS row
    of dense_features' final norm, and against the pass that computes every row (SAIS_VIT_PRUNE_LAST=0)"""
    xd = dev(_case_input(name))
    with torch.no_grad():
        fwd = vit(xd)
        full = vit.dense_features(xd, 1)[0]
        rel("tail_vs_dense", host(fwd), host(full[:, 0]), name)
        monkeypatch.setenv("SAIS_VIT_PRUNE_LAST", "0")
        unpruned = _model()
        assert not unpruned.prune_last_block and vit.prune_last_block
        every = unpruned(xd)
        rel("tail_vs_unpruned", host(fwd), host(every), name)
        assert torch.equal(every, full[:, 0])                         # the same launches, the same final norm on the CLS rows
        vit.prune_last_block = False
        try:
            assert torch.equal(vit(xd), every)
        finally:
            vit.prune_last_block = True
        assert torch.equal(vit(xd), fwd)


def test_retrieval_cls_only_is_the_first_half(vit):
    xd = dev(_case_input("c64x88"))
    desc = vit.retrieval_features(xd)
    cls = vit.retrieval_features(xd, cls_only=True)
    assert desc.shape == (2, 768) and cls.shape == (2, 384)
    assert torch.equal(desc[:, :384], cls)
    rel("retrieval_cls_vs_dense", host(cls), host(vit.dense_features(xd, 1)[0][:, 0]), "c64x88")
    from sais_amd import retrieval
    odd = dev(R.frames(1, 70, 93, 811))                               # cropped to 64 x 88, not to 64 x 80
    assert torch.equal(retrieval.cls_features(vit)(odd), vit.retrieval_features(odd[:, :, :64, :88].contiguous(), cls_only=True))


def test_row_kernel_dispatch_at_eleven_frames(vit, g, ops):
    """11 x 785 = 8635 rows >= ROW_GEMM_MIN_M: the row-owning GEMMs with the LayerNorm epilogues; the two golden frames in front"""
    assert 11 * 785 >= ops.ROW_GEMM_MIN_M > 2 * 785
    name = "c224x224"
    x = np.concatenate([_case_input(name), R.frames(9, 224, 224, 812)])
    xd = dev(x)
    with torch.no_grad():
        fwd = vit(xd)
        rel("forward11", host(fwd[:2]), g[f"{name}_fwd"], name)
        dense = vit.dense_features(xd, 1)[0]
        rel("dense11", host(dense[:2])[:, R.rows(224, 224)], g[f"{name}_rows"][1], name)
        probe = vit.probe_features(xd, R.N_LAST)
        rel("probe11", host(probe[:2]), np.concatenate(list(g[f"{name}_cls"]), axis=1), name)
        assert torch.equal(vit(xd), fwd) and torch.equal(vit.dense_features(xd, 1)[0], dense)


def test_feature_extractor_replays_the_patch8_pass(vit):
    """sais_amd.inference.FeatureExtractor (extract_representations.py --patch_size 8): the captured pass, replayed on a full and
    on a padded batch, equals the eager pass on the same padded shapes bit for bit, and forward() within the feature bar"""
    from sais_amd.inference import FeatureExtractor
    x = dev(R.frames(6, 224, 224, 814))
    replayed = FeatureExtractor(vit, batch_size=4, use_graph=True, tail_batch=None)(x)
    eager = FeatureExtractor(vit, batch_size=4, use_graph=False, tail_batch=None)(x)
    assert replayed.shape == (6, 384) and torch.equal(replayed, eager)
    with torch.no_grad():
        rel("extractor_vs_forward", host(replayed), host(vit(x)), "c224x224")


# ------------------------------------------------------------------------------------------------ 6. one tool end to end
def test_visualize_attention_patch8(tmp_path):
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(813))
    yy, xx = np.mgrid[:64, :88]
    base = (np.stack([xx * 2.5, yy * 3.5, (xx + yy) * 1.5], -1) % 256).astype(np.float32)
    Image.fromarray(np.clip(base + 8 * rng.standard_normal((64, 88, 3)), 0, 255).astype(np.uint8)).save(tmp_path / "in.png")
    spec = importlib.util.spec_from_file_location(
        "vit8_visualize_attention", os.path.join(ROOT, "SAIS", "scripts", "dino-main", "visualize_attention.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--patch_size", "8", "--image_path", str(tmp_path / "in.png"), "--image_size", "64", "88", "--threshold", "0.6",
              "--output_dir", str(tmp_path / "out")])
    want = ["img.png"] + [f"attn-head{j}.png" for j in range(6)] + [f"mask_th0.6_head{j}.png" for j in range(6)]
    assert sorted(os.listdir(tmp_path / "out")) == sorted(want)
    for f in want:
        im = Image.open(tmp_path / "out" / f)
        assert im.size == (88, 64), f
        a = np.asarray(im)
        if f.startswith("mask"):                                      # 8 x 11 patches, each an 8 x 8 block
            assert im.mode == "L" and set(np.unique(a)) <= {0, 255} and 0 < (a == 255).mean() < 1
            assert np.array_equal(a, np.repeat(np.repeat(a[::8, ::8], 8, 0), 8, 1))
        elif f.startswith("attn"):
            assert np.array_equal(a, np.repeat(np.repeat(a[::8, ::8], 8, 0), 8, 1))
            assert len(np.unique(a[::8, ::8].reshape(-1, a.shape[-1]), axis=0)) > 8      # a map, not a constant
