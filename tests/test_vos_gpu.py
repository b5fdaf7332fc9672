"""Video object segmentation on a real MI355X: the streaming attention against an fp64 softmax, dense_features against the
reference's recorded get_intermediate_layers off 224 x 224, label propagation against the fp64 restatement of
tests/vos_ref.py and the reference's recorded outputs (tests/golden/make_golden_vos.py), the queue, the upsample / argmax tail
and the command line.

Bars (stated here, used below):
  * attention: the project's own for this operation (tests/test_kernels_gpu.py): out atol = rtol = 2e-2, lse atol = 1e-3
  * features: the project's single feature bar, 2e-2 * max|ref| (tests/test_model_gpu.py FEAT_REL; bf16 MFMA backbone)
  * propagation: vos_ref.PROP_TOL * max|segs| on non-fragile queries (derived there); fragile queries (the top-k cut within
    2 TAU of the next cosine) must be finite and inside the range of segs
  * labels: equal, except pixels whose two best channels lie within vos_ref.ARGMAX_MARGIN in fp64
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity
import synth
import vos_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT_REL = 2e-2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


@pytest.fixture(scope="module")
def vit():
    from sais_amd.vit import vit_small
    m = vit_small(patch_size=16)
    m.load_state_dict(synth.vit_state_dict(seed=0), strict=True)
    return m.to(DEV).eval()


# ------------------------------------------------------------------------------------------------ 1. streaming attention
def _attn_fp64(qkv, frames, ntok):
    t = qkv.double().view(frames, ntok, 3, 6, 64).permute(2, 0, 3, 1, 4)
    s = (t[0] @ t[1].transpose(-2, -1)) * 0.125
    out = (torch.softmax(s, -1) @ t[2]).transpose(1, 2).reshape(frames * ntok, 384)
    return out, torch.logsumexp(s, -1)


def _assert_close(got, ref, atol, rtol, name):
    err = (got.double() - ref.double()).abs()
    bad = err > atol + rtol * ref.double().abs()
    assert not bad.any(), f"{name}: max err {err.max().item():.3e}, {int(bad.sum())} bad"
    return err.max().item()


@pytest.mark.parametrize("frames,ntok", [(1, 25), (3, 171), (3, 197), (2, 274), (1, 1561), (2, 37)])
def test_streaming_attention_vs_fp64(frames, ntok):
    """one partial tile, a ragged tail, the resident kernel's two sizes, more than four tiles, the workload's own count"""
    from sais_amd import ops
    M = frames * ntok
    qkv = rnd(M, 1152, seed=40 + ntok, scale=1.5, dtype=torch.bfloat16)
    out = torch.full((M + 70, 384), float("nan"), dtype=torch.bfloat16, device=DEV)      # oversized: the tail must stay NaN
    lse = torch.full((frames, 6, ntok), float("nan"), device=DEV)
    ops.vit_attn_fwd_any(qkv, frames, ntok, out, lse)
    ref, ref_lse = _attn_fp64(qkv, frames, ntok)
    e_out = _assert_close(out[:M], ref, 2e-2, 2e-2, "out")
    e_lse = _assert_close(lse, ref_lse, 1e-3, 0.0, "lse")
    print(f"ntok {ntok}: out max err {e_out:.3e}, lse max err {e_lse:.3e}")
    parity.parity_log("vos_attn_any_lse_abs", e_lse, 1e-3)
    assert torch.isnan(out[M:]).all()
    if ntok in (197, 37):                                 # the LDS-resident kernel on the same input, under the same bars
        res, res_lse = torch.empty(M, 384, dtype=torch.bfloat16, device=DEV), torch.empty(frames, 6, ntok, device=DEV)
        ops.vit_attn_fwd(qkv, frames, res, res_lse, None, ntok=ntok)
        _assert_close(out[:M], res.float(), 2e-2, 2e-2, "out vs sais_vit_attn_fwd")
        _assert_close(lse, res_lse, 1e-3, 0.0, "lse vs sais_vit_attn_fwd")
    again, again_lse = torch.full_like(out, float("nan")), torch.empty_like(lse)
    ops.vit_attn_fwd_any(qkv, frames, ntok, again, again_lse)
    assert torch.equal(again[:M], out[:M]) and torch.equal(again_lse, lse)
    ops.vit_attn_fwd_any(qkv, frames, ntok, again, None)                                  # lse is optional
    assert torch.equal(again[:M], out[:M])


# ------------------------------------------------------------------------------------------------ 2. dense features
def test_dense_features_vs_golden(vit, golden):
    g = golden("vos")
    for name, H, W, n, seed in vos_ref.DENSE_CASES:
        x = vos_ref.dense_input(H, W, seed)
        assert np.array_equal(vos_ref.digest(x), g[f"{name}_sha256"])
        got = vit.dense_features(dev(x), n)
        ntok = 1 + (H // 16) * (W // 16)
        assert len(got) == n and all(t.shape == (2, ntok, 384) and t.dtype == torch.float32 for t in got)
        ref = g[name]
        for j in range(n):
            a = host(got[j]) if ntok <= 171 else host(got[j])[:, vos_ref.DENSE_ROWS]
            err, scale = float(np.abs(a.astype(np.float64) - ref[j]).max()), float(np.abs(ref[j]).max())
            print(f"{name} layer {j}: max err {err:.3e} = {err / scale:.3e} max|ref|")
            parity.parity_log("vos_dense_" + name, err / scale, FEAT_REL)
            assert err <= FEAT_REL * scale, (name, j, err, scale)


def test_dense_features_at_the_row_kernel_dispatch(vit, golden):
    """30 frames x 274 tokens = 8220 rows: the N = 384 GEMMs run on the row-owning kernel with the following LayerNorm in their
    epilogue, and the taps read the stream those launches left.  A frame's features do not depend on the frames beside it, so the
    two golden frames of d208x336, in front of 28 others, are held to their record at the bar of test_dense_features_vs_golden."""
    from sais_amd import ops
    name, H, W, n, seed = vos_ref.DENSE_CASES[1]
    x = dev(np.concatenate([vos_ref.dense_input(H, W, seed), vos_ref.dense_input(H, W, 233, frames=28)]))
    ntok = 1 + (H // 16) * (W // 16)
    assert (name, ntok, n) == ("d208x336", 274, 2) and x.shape[0] * ntok >= ops.ROW_GEMM_MIN_M
    got = vit.dense_features(x, n)
    assert len(got) == n and all(t.shape == (30, ntok, 384) and t.dtype == torch.float32 for t in got)
    ref = golden("vos")[name]
    for j in range(n):
        a = host(got[j][:2])[:, vos_ref.DENSE_ROWS]
        err, scale = float(np.abs(a.astype(np.float64) - ref[j]).max()), float(np.abs(ref[j]).max())
        print(f"{name} in 30 frames, layer {j}: max err {err:.3e} = {err / scale:.3e} max|ref|")
        parity.parity_log("vos_dense_rowkernel_" + name, err / scale, FEAT_REL)
        assert err <= FEAT_REL * scale, (name, j, err, scale)
    again = vit.dense_features(x, n)
    assert all(torch.equal(a, b) for a, b in zip(again, got))


def test_dense_features_at_224_and_forward_untouched(vit):
    x = synth.clips(seed=10, B=1, T=2)[0].to(DEV)
    with torch.no_grad():
        rep = vit(x)
    ref = host(vit.get_intermediate_layers(x, 1)[0])
    got = host(vit.dense_features(x, 1)[0])
    err, scale = float(np.abs(got.astype(np.float64) - ref).max()), float(np.abs(ref).max())
    print(f"224 x 224: streaming vs resident path max err {err:.3e} = {err / scale:.3e} max|ref|")
    parity.parity_log("vos_dense_224_vs_resident", err / scale, FEAT_REL)
    assert err <= FEAT_REL * scale
    vit.dense_features(x[:, :, :160, :208], 2)
    with torch.no_grad():
        assert torch.equal(vit(x), rep)


# ------------------------------------------------------------------------------------------------ 3. propagation
def _check_propagation(name, tar, ctx, segs, h, w, r, topk, recorded=None):
    from sais_amd import vos
    got = vos.label_propagation(dev(tar), dev(ctx), dev(segs), h, w, r, topk)
    assert got.shape == (segs.shape[1], h, w)
    a = host(got).reshape(segs.shape[1], h * w).astype(np.float64)
    ref = vos_ref.propagate(tar, ctx, segs, h, w, r, topk)
    frag = vos_ref.fragile_queries(tar, ctx, h, w, r, topk)
    assert frag.mean() <= vos_ref.FRAGILE_CAP
    bar = vos_ref.PROP_TOL * float(np.abs(segs).max())
    err = float(np.abs(a - ref)[:, ~frag].max())
    print(f"{name}: max err on non-fragile queries {err:.3e} (bar {bar:.3e}), {int(frag.sum())} fragile of {h * w}")
    parity.parity_log("vos_propagate_" + name, err, bar)
    assert err <= bar, (name, err, bar)
    assert np.isfinite(a).all() and a.min() >= segs.min() - 1e-6 and a.max() <= segs.max() + 1e-6
    if recorded is not None:                               # what the reference's own label_propagation gave (fp32)
        assert float(np.abs(a - recorded)[:, ~frag].max()) <= bar + 1e-5
    again = vos.label_propagation(dev(tar), dev(ctx), dev(segs), h, w, r, topk)
    assert torch.equal(again, got)


@pytest.mark.parametrize("case", vos_ref.GOLDEN_CASES, ids=[c[0] for c in vos_ref.GOLDEN_CASES])
def test_propagation_vs_fp64_and_golden(case, golden):
    name, h, w, nctx, C, r, topk, seed = case
    g = golden("vos")
    tar, ctx, segs = vos_ref.make_case(h, w, nctx, C, r, topk, seed)
    assert np.array_equal(vos_ref.digest(tar, ctx, segs), g[f"{name}_sha256"])
    _check_propagation(name, tar, ctx, segs, h, w, r, topk, recorded=g[f"{name}_out"])


def test_propagation_workload_grid():
    name, h, w, nctx, C, r, topk, seed = vos_ref.WORKLOAD_CASE
    _check_propagation(name, *vos_ref.make_case(h, w, nctx, C, r, topk, seed), h, w, r, topk)


def test_propagation_keeps_ties():
    """two pairs of context slots hold bit-identical features: every cosine occurs twice, the cut (topk = 5) falls inside a
    pair, and both twins stay — their masks differ, so dropping one shows"""
    name, h, w, nctx, C, r, topk, seed = vos_ref.TIE_CASE
    tar, ctx, segs = vos_ref.make_tie_case()
    assert np.array_equal(ctx[0], ctx[1]) and not np.array_equal(segs[0], segs[1])
    cos = vos_ref.cosines(tar, ctx)
    assert np.array_equal(cos[0], cos[1]) and np.array_equal(cos[2], cos[3])
    ref = vos_ref.propagate(tar, ctx, segs, h, w, r, topk)
    one = vos_ref.propagate(tar, ctx[[0, 2, 1, 3]], segs[[0, 2, 1, 3]], h, w, r, topk)
    assert np.abs(ref - one).max() < 1e-12                 # the restatement does not depend on the slot order either
    _check_propagation(name, tar, ctx, segs, h, w, r, topk)


# ------------------------------------------------------------------------------------------------ 4. the queue
def test_label_propagator_sequence(golden):
    from sais_amd import vos
    g, s = golden("vos"), vos_ref.SEQ
    feats, first = vos_ref.make_sequence()
    assert np.array_equal(vos_ref.digest(feats, first), g["seq_sha256"])
    h, w = s["h"], s["w"]
    prop = vos.LabelPropagator(dev(feats[0]), dev(first).view(s["C"], h, w), h, w, s["n_last_frames"], s["r"], s["topk"])
    orders = []
    for t in range(1, s["frames"]):
        orders.append(prop.context_order())
        seg = prop.step(dev(feats[t]))
        assert seg.shape == (s["C"], h, w)
        err = float(np.abs(host(seg).reshape(s["C"], -1) - g["seq_segs"][t - 1]).max())
        print(f"frame {t}: max err {err:.3e} (bar {t * 1e-3:.0e})")
        parity.parity_log(f"vos_sequence_frame{t}", err, t * 1e-3)
        assert err <= t * 1e-3, (t, err)
    assert orders == [[0], [0, 1], [0, 1, 2], [0, 2, 1]]     # first frame always first, then oldest to newest; the ring wraps


# ------------------------------------------------------------------------------------------------ 5. upsample + argmax
@pytest.mark.parametrize("case", vos_ref.UPSAMPLE_CASES, ids=[c[0] for c in vos_ref.UPSAMPLE_CASES])
def test_upsample_argmax_vs_golden(case, golden):
    from sais_amd import vos
    name, C, h, w, patch, seed, special = case
    g = golden("vos")
    seg = vos_ref.make_upsample_case(C, h, w, patch, seed, special)
    assert np.array_equal(vos_ref.digest(seg), g[f"{name}_sha256"])
    got = vos.upsample_argmax(dev(seg), patch)
    assert got.shape == (h * patch, w * patch) and got.dtype == torch.uint8
    _, near = vos_ref.upsample_argmax(seg, patch)
    assert near.mean() <= vos_ref.ARGMAX_EXCEPT_CAP
    diff = host(got) != g[f"{name}_labels"]
    print(f"{name}: {int(diff.sum())} pixels differ, {int(near.sum())} near-tie pixels excepted")
    assert not (diff & ~near).any()


# ------------------------------------------------------------------------------------------------ 6. argument errors
def test_argument_errors(vit):
    from sais_amd import vos
    from sais_amd._lib import SaisHipError
    bad = (ValueError, SaisHipError)
    with pytest.raises(bad):
        vit.dense_features(torch.zeros(1, 3, 64, 96), 1)                    # host tensor
    with pytest.raises(bad):
        vit.dense_features(torch.zeros(1, 3, 72, 96, device=DEV), 1)        # H not a multiple of 16
    with pytest.raises(bad):
        vit.dense_features(torch.zeros(1, 3, 16, 16 * 4097, device=DEV), 1)     # 4098 tokens
    with pytest.raises(bad):
        vit.dense_features(torch.zeros(1, 3, 64, 96, device=DEV), 13)
    h, w, n = 4, 5, 20
    feat = lambda *lead, d=384: torch.zeros(*lead, n, d, device=DEV) + 1.0
    seg = lambda nctx, C: torch.zeros(nctx, C, n, device=DEV)
    with pytest.raises(bad):
        vos.label_propagation(feat().cpu(), feat(2), seg(2, 3), h, w, 2, 5)      # host tensor
    with pytest.raises(bad):
        vos.label_propagation(feat(), feat(17), seg(17, 3), h, w, 2, 5)          # nctx = 17
    with pytest.raises(bad):
        vos.label_propagation(feat(), feat(2), seg(2, 65), h, w, 2, 5)           # C = 65
    with pytest.raises(bad):
        vos.label_propagation(feat(), feat(2), seg(2, 3), h, w, 2, 0)            # topk = 0
    with pytest.raises(bad):
        vos.label_propagation(feat(d=256), feat(2, d=256), seg(2, 3), h, w, 2, 5)     # feature dim 256
    with pytest.raises(bad):
        vos.upsample_argmax(torch.zeros(3, 4, 5), 16)                            # host tensor
    with pytest.raises(bad):
        vos.LabelPropagator(feat().cpu(), seg(1, 3)[0], h, w)


# ------------------------------------------------------------------------------------------------ 7. the command line
def test_cli_end_to_end(tmp_path):
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(7))
    data, H, W = tmp_path / "davis", 96, 160
    (data / "ImageSets" / "2017").mkdir(parents=True)
    (data / "ImageSets" / "2017" / "val.txt").write_text("vidA\nvidB\n")
    palette = np.zeros((256, 3), dtype=np.uint8)
    palette[1], palette[2] = (128, 0, 0), (0, 128, 0)
    ann = {}
    for v, shift in (("vidA", 0), ("vidB", 30)):
        (data / "JPEGImages" / "480p" / v).mkdir(parents=True)
        (data / "Annotations" / "480p" / v).mkdir(parents=True)
        yy, xx = np.mgrid[:H, :W]
        base = (np.stack([xx * 1.5, yy * 2.5, (xx + yy)], -1) % 256).astype(np.float32)
        for t in range(4):
            img = np.clip(np.roll(base, 4 * t + shift, axis=1) + 8 * rng.standard_normal((H, W, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(data / "JPEGImages" / "480p" / v / f"{t:05d}.jpg", quality=92)
        lab = np.zeros((H, W), dtype=np.uint8)
        lab[20:60, 30 + shift:80 + shift] = 1
        lab[50:90, 100:150] = 2
        im = Image.fromarray(lab)
        im.putpalette(palette.ravel())
        im.save(data / "Annotations" / "480p" / v / "00000.png")
        ann[v] = lab
    script = os.path.join(ROOT, "SAIS", "scripts", "dino-main", "eval_video_segmentation.py")

    def run(out):
        r = subprocess.run([sys.executable, script, "--data_path", str(data), "--output_dir", str(out), "--n_last_frames", "2",
                            "--size_mask_neighborhood", "3", "--bs", "3"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "random weights" in r.stdout
        return r.stdout
    run(tmp_path / "out1")
    run(tmp_path / "out2")
    for v in ("vidA", "vidB"):
        names = sorted(os.listdir(tmp_path / "out1" / v))
        assert names == [f"{t:05d}.png" for t in range(4)]
        for nm in names:
            im = Image.open(tmp_path / "out1" / v / nm)
            assert im.mode == "P" and im.size == (W, H)
            assert np.array_equal(np.asarray(im.getpalette()[:9], dtype=np.uint8), palette[:3].ravel())
            assert np.asarray(im).max() <= 2
            assert (tmp_path / "out1" / v / nm).read_bytes() == (tmp_path / "out2" / v / nm).read_bytes()
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out1" / v / "00000.png")), ann[v])
