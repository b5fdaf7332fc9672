"""Attention-map rendering on a real MI355X: the CLS row of the last block's softmax against an fp64 softmax, the resident
attention kernel and the reference's recorded get_last_selfattention off and on 224 x 224; the mass mask against the fp64
restatement of tests/attnviz_ref.py; heat maps and colour images against its f32 / matplotlib restatements and against what
the reference's VideoGenerator._inference recorded (tests/golden/make_golden_attnviz.py); the two command lines.

Bars (stated here, used below):
  * CLS probabilities: 1e-3 of the row maximum, the project's bar for fp32 softmax statistics (tests/test_kernels_gpu.py, lse);
    rows sum to 1 within 1e-5
  * attention maps of the backbone: ATTN_TOL = 2e-3 max-abs, the project's attention-map bar (tests/test_model_gpu.py)
  * masks: equal on every non-fragile element (attnviz_ref.fragile: cumulative share within n 2^-24 of the cut); at most
    attnviz_ref.FRAGILE_CAP fragile elements per row, asserted on the inputs before any comparison
  * heat maps: bit-equal; colours, JPEG bytes: equal
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import attnviz_ref as ar
import parity
import synth
import vos_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "SAIS", "scripts", "dino-main")
ATTN_TOL, PROB_REL = 2e-3, 1e-3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def vit():
    from sais_amd.vit import vit_small
    m = vit_small(patch_size=16)
    m.load_state_dict(synth.vit_state_dict(seed=0), strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def own_probs(vit):
    """cls_attention of the golden inputs, computed once: name -> f32 [2, 6, ntok] on the device"""
    return {name: vit.cls_attention(dev(vos_ref.dense_input(H, W, seed))) for name, H, W, seed in ar.CLS_CASES}


def grid_of(name):
    return next((H // 16, W // 16) for n, H, W, _ in ar.CLS_CASES if n == name)


# ------------------------------------------------------------------------------------------------ 1. sais_vit_cls_probs
@pytest.mark.parametrize("frames,ntok", [(1, 2), (1, 25), (3, 171), (3, 197), (2, 274), (1, 1561), (1, 4097)])
def test_cls_probs_vs_fp64(frames, ntok):
    from sais_amd import ops
    M = frames * ntok
    g = torch.Generator().manual_seed(300 + ntok)
    qkv = (torch.randn(M, 1152, generator=g) * 1.5).to(torch.bfloat16).to(DEV)
    q, k = qkv.view(frames, ntok, 1152)[:, 0, :384], qkv[:, 384:768]          # both in place: row strides ntok * 1152 and 1152
    buf = torch.full((frames * 6 * ntok + 70,), float("nan"), device=DEV)     # oversized: the tail must stay NaN
    probs = buf[:frames * 6 * ntok].view(frames, 6, ntok)
    ops.vit_cls_probs(q, k, frames, ntok, probs)
    ref = ar.cls_probs(host(qkv.float()), frames, ntok)
    got = host(probs).astype(np.float64)
    rel = float((np.abs(got - ref).max(-1) / ref.max(-1)).max())
    rowsum = float(np.abs(got.sum(-1) - 1).max())
    print(f"ntok {ntok}: max err / row max {rel:.3e}, |row sum - 1| {rowsum:.3e}")
    parity.parity_log("attnviz_cls_probs_rel_rowmax", rel, PROB_REL)
    parity.parity_log("attnviz_cls_probs_rowsum", rowsum, 1e-5)
    assert rel <= PROB_REL and rowsum <= 1e-5
    assert torch.isnan(buf[frames * 6 * ntok:]).all()
    again = torch.empty_like(probs)
    ops.vit_cls_probs(q, k, frames, ntok, again)
    assert torch.equal(again, probs)                                          # run to run
    if frames > 1:                                                            # a frame alone and inside the batch
        f = frames - 1
        alone = torch.empty(1, 6, ntok, device=DEV)
        ops.vit_cls_probs(q[f:f + 1], k[f * ntok:(f + 1) * ntok], 1, ntok, alone)
        assert torch.equal(alone[0], probs[f])
    if ntok == 197:                                                           # row 0 of the resident kernel's probabilities
        out, lse = torch.empty(M, 384, dtype=torch.bfloat16, device=DEV), torch.empty(frames, 6, ntok, device=DEV)
        full = torch.empty(frames, 6, ntok, ntok, device=DEV)
        ops.vit_attn_fwd(qkv, frames, out, lse, full, ntok=ntok)
        d = float((full[:, :, 0, :] - probs).abs().max())
        print(f"vs sais_vit_attn_fwd row 0: {d:.3e}")
        assert d <= ATTN_TOL


# ------------------------------------------------------------------------------------------------ 2. cls_attention
def test_cls_attention_vs_golden(vit, own_probs, golden):
    g = golden("attnviz")
    for name, H, W, seed in ar.CLS_CASES:
        assert np.array_equal(vos_ref.digest(vos_ref.dense_input(H, W, seed)), g[f"{name}_sha256"])
        got, ref = own_probs[name], g[f"{name}_probs"]
        assert got.shape == ref.shape and got.dtype == torch.float32
        err = float(np.abs(host(got).astype(np.float64) - ref).max())
        print(f"{name}: max err {err:.3e} (max probability {ref.max():.3e})")
        parity.parity_log("attnviz_cls_attention_" + name, err, ATTN_TOL)
        assert err <= ATTN_TOL, (name, err)
    x = dev(vos_ref.dense_input(224, 224, ar.CLS_CASES[2][3]))
    full = vit.get_last_selfattention(x)[:, :, 0, :]
    d = float((full - own_probs["c224x224"]).abs().max())
    print(f"224 x 224 vs get_last_selfattention: {d:.3e}")
    parity.parity_log("attnviz_cls_attention_vs_last_selfattention", d, ATTN_TOL)
    assert d <= ATTN_TOL
    assert torch.equal(vit.cls_attention(x), own_probs["c224x224"])           # run to run


def test_cls_attention_at_the_row_kernel_dispatch(vit, own_probs):
    """48 frames of 224 x 224 are 9456 >= 8192 rows: the N = 384 GEMMs run on the row-owning kernel and the last block's norm1
    comes out of block 10's fc2 epilogue instead of its own launch.  The first two frames agree with the small-batch pass."""
    from sais_amd import ops
    x2 = vos_ref.dense_input(224, 224, ar.CLS_CASES[2][3])
    x = np.concatenate([x2, vos_ref.dense_input(224, 224, 245, frames=46)])
    assert x.shape[0] * 197 >= ops.ROW_GEMM_MIN_M
    got = vit.cls_attention(dev(x))
    assert got.shape == (48, 6, 197)
    d = float((got[:2] - own_probs["c224x224"]).abs().max())
    rowsum = float((got.double().sum(-1) - 1).abs().max())
    print(f"row-kernel dispatch vs small batch: {d:.3e}; |row sum - 1| {rowsum:.3e}")
    parity.parity_log("attnviz_cls_attention_row_dispatch", d, ATTN_TOL)
    assert d <= ATTN_TOL and rowsum <= 1e-5


def test_cls_attention_argument_errors(vit):
    from sais_amd import _lib
    with pytest.raises(_lib.SaisHipError):
        vit.cls_attention(torch.zeros(1, 3, 64, 96))                          # host tensor
    with pytest.raises(ValueError):
        vit.cls_attention(torch.zeros(1, 3, 72, 96, device=DEV))              # H % 16
    with pytest.raises(ValueError):
        vit.cls_attention(torch.zeros(1, 3, 1024, 1040, device=DEV))          # 64 x 65 + 1 = 4161 tokens
    with pytest.raises(ValueError):
        vit.cls_attention(torch.zeros(3, 64, 96, device=DEV))


# ------------------------------------------------------------------------------------------------ 3. mass_mask
def synthetic_rows(n, seed, rows=6):
    """f32 [1, rows, 1 + n]: softmax rows of scores ~ 2 N(0, 1) behind a CLS column the mask must not read"""
    rng = np.random.Generator(np.random.PCG64(seed))
    e = np.exp(2.0 * rng.standard_normal((rows, n)))
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return np.concatenate([np.full((rows, 1), 0.5, np.float32), p], axis=1)[None]


def check_mask(probs, threshold, name):
    """probs f32 [F, R, 1 + n] (host): the device mask against the restatement, the strided view against a contiguous copy"""
    from sais_amd import attnviz, ops
    p = probs[:, :, 1:]
    frag = ar.fragile(p, threshold)
    assert frag.sum(-1).max() <= ar.FRAGILE_CAP, f"{name}: change the seed of this input, not the cap"
    d = dev(probs)
    keep = attnviz.mass_mask(d, threshold)
    assert keep.dtype == torch.uint8 and tuple(keep.shape) == p.shape
    bad = (host(keep) != ar.mass_mask(p, threshold)) & ~frag
    assert not bad.any(), f"{name} threshold {threshold}: {int(bad.sum())} non-fragile elements differ"
    assert torch.equal(attnviz.mass_mask(d, threshold), keep)                 # run to run
    flat, keep2 = d[:, :, 1:].contiguous(), torch.empty_like(keep)
    ops.attn_mass_mask(flat, p.shape[0] * p.shape[1], p.shape[2], threshold, keep2)
    assert torch.equal(keep2, keep)
    return int(frag.sum())


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 170, 1560, 4096])
def test_mass_mask_synthetic(n):
    """n = 1, 2; around one wave; a ragged row; the workload's size class; the limit (every sort stage, 16 elements per thread)"""
    probs = synthetic_rows(n, 400 + n)
    for threshold in ((0.6,) if n == 4096 else (0.1, 0.6, 0.95)):
        nfrag = check_mask(probs, threshold, f"n = {n}")
        print(f"n {n} threshold {threshold}: {nfrag} fragile elements")


def test_mass_mask_on_reference_probabilities(golden):
    from sais_amd import attnviz
    g = golden("attnviz")
    for name, _, _, _ in ar.CLS_CASES:
        for threshold in (0.1, 0.6, 0.95):
            check_mask(g[f"{name}_probs"], threshold, name)
    i = 0
    for name in ar.VIDEO_CASES:                         # the masks the reference's own f32 code made of the same rows
        keep = host(attnviz.mass_mask(dev(g[f"{name}_probs"]), ar.THRESHOLD))
        for fr in range(2):
            frag = ar.fragile(g[f"{name}_probs"][fr][:, 1:], ar.THRESHOLD)
            assert not ((keep[fr] != g[f"video_{i}_mask"]) & ~frag).any()
            i += 1


def test_mass_mask_ties_and_zero_rows():
    from sais_amd import attnviz
    t = ar.tie_rows()
    probs = np.concatenate([np.zeros((t.shape[0], 1), np.float32), t], axis=1)[None]
    frag = ar.fragile(t, ar.THRESHOLD)
    assert frag.sum(-1).max() <= ar.FRAGILE_CAP
    keep = host(attnviz.mass_mask(dev(probs), ar.THRESHOLD))[0]
    assert np.array_equal(keep[~frag], ar.mass_mask(t, ar.THRESHOLD)[~frag])  # equal values: ascending index order
    z = np.zeros((1, 3, 1 + 65), np.float32)
    z[0, 1, 1:] = 1.0 / 65
    z[:, :, 0] = 1.0                                    # (the CLS column is not part of the row)
    keep = host(attnviz.mass_mask(dev(z), 0.6))[0]
    assert keep[0].sum() == 0 and keep[2].sum() == 0 and keep[1].sum() > 0    # a zero row keeps nothing
    with pytest.raises(ValueError):
        attnviz.mass_mask(dev(z), 1.0)
    with pytest.raises(ValueError):
        attnviz.mass_mask(dev(z), 0.0)


# ------------------------------------------------------------------------------------------------ 4. render
@pytest.mark.parametrize("name", ["c64x96", "c160x272"])
@pytest.mark.parametrize("patch", [1, 16])
def test_render_own_probabilities(own_probs, name, patch):
    """the GPU's own probabilities and mask in, heat bit-equal to the f32 restatement, colours equal to matplotlib's rule"""
    from sais_amd import attnviz
    probs, (h, w) = own_probs[name], grid_of(name)
    keep = attnviz.mass_mask(probs, ar.THRESHOLD)
    heat, rgb = attnviz.render(probs, (h, w), threshold=ar.THRESHOLD, cmap="inferno", patch=patch)
    assert heat.shape == (2, h, w) and rgb.shape == (2, h * patch, w * patch, 3) and rgb.dtype == torch.uint8
    ref = ar.heat(host(probs)[:, :, 1:], host(keep)).reshape(2, h, w)
    assert np.array_equal(host(heat), ref)
    assert np.array_equal(host(rgb), ar.to_rgb(ref, attnviz.colormap_lut("inferno"), patch))
    heat2, rgb2 = attnviz.render(probs, (h, w), keep=keep, cmap="inferno", patch=patch)
    assert torch.equal(heat2, heat) and torch.equal(rgb2, rgb)                # the mask given == the mask made; run to run
    for j in range(6):                                                        # visualize_attention.py: one head, no mask
        hj, cj = attnviz.render(probs, (h, w), heads=j, cmap="viridis", patch=patch)
        assert np.array_equal(host(hj), host(probs)[:, j, 1:].reshape(2, h, w))
        assert np.array_equal(host(cj), ar.to_rgb(host(hj), attnviz.colormap_lut("viridis"), patch))
    h3, none = attnviz.render(probs, (h, w), heads=range(2, 5), cmap=None)    # a run of heads, heat only
    assert none is None and np.array_equal(host(h3), ar.heat(host(probs)[:, :, 1:], None, 2, 3).reshape(2, h, w))


def test_render_edge_maps():
    from sais_amd import attnviz
    lut = attnviz.colormap_lut("inferno")
    rng = np.random.Generator(np.random.PCG64(281))
    one = rng.random((3, 6, 2)).astype(np.float32)                            # grid 1 x 1: every map is constant
    heat, rgb = attnviz.render(dev(one), (1, 1), cmap="inferno", patch=16)
    assert np.array_equal(host(heat), ar.heat(one[:, :, 1:]).reshape(3, 1, 1))
    assert (host(rgb) == lut[0]).all() and rgb.shape == (3, 16, 16, 3)
    const = np.full((2, 6, 1 + 24), 0.04, np.float32)                         # a constant 4 x 6 map: index 0 everywhere
    const[1, :, 1:] = rng.random((6, 24)).astype(np.float32)                  # (and beside it a frame with its own range)
    heat, rgb = attnviz.render(dev(const), (4, 6), cmap="inferno", patch=16)
    ref = ar.heat(const[:, :, 1:]).reshape(2, 4, 6)
    assert np.array_equal(host(heat), ref) and np.array_equal(host(rgb), ar.to_rgb(ref, lut, 16))
    assert (host(rgb)[0] == lut[0]).all()
    edge = np.zeros((1, 1, 1 + 6), np.float32)                                # vmin, vmax and one ulp inside each
    lo, hi = np.float32(0.125), np.float32(0.8125)
    edge[0, 0, 1:] = [lo, np.nextafter(lo, hi), np.nextafter(hi, lo), hi, (lo + hi) / 2, lo]
    heat, rgb = attnviz.render(dev(edge), (1, 6), cmap="viridis", patch=1)
    assert np.array_equal(host(rgb), ar.to_rgb(host(heat), attnviz.colormap_lut("viridis"), 1))
    assert (host(rgb)[0, 0, 3] == attnviz.colormap_lut("viridis")[255]).all()
    big = np.concatenate([np.zeros((1, 2, 1), np.float32), rng.random((1, 2, 4096)).astype(np.float32)], axis=2)
    heat, rgb = attnviz.render(dev(big), (64, 64), cmap="inferno", patch=2)   # the limit: 16 min / max partials
    ref = ar.heat(big[:, :, 1:]).reshape(1, 64, 64)
    assert np.array_equal(host(heat), ref) and np.array_equal(host(rgb), ar.to_rgb(ref, lut, 2))
    with pytest.raises(ValueError):
        attnviz.render(dev(const), (4, 5))
    with pytest.raises(ValueError):
        attnviz.render(dev(const), (4, 6), patch=65)
    with pytest.raises(ValueError):
        attnviz.render(dev(const), (4, 6), heads=[0, 2])


def test_render_reproduces_the_reference_files(golden, tmp_path):
    """reference probabilities and the reference's own masks in: the heat map plt.imsave was given, bit for bit, and its JPEG"""
    from sais_amd import attnviz
    g = golden("attnviz")
    i = 0
    for name in ar.VIDEO_CASES:
        h, w = grid_of(name)
        keep = np.stack([g[f"video_{i + fr}_mask"] for fr in range(2)])
        heat, rgb = attnviz.render(dev(g[f"{name}_probs"]), (h, w), keep=dev(keep), cmap="inferno", patch=16)
        for fr in range(2):
            assert np.array_equal(host(heat)[fr], g[f"video_{i}_heat"]), (name, fr)
            attnviz.save_jpeg(str(tmp_path / "f.jpg"), rgb[fr])
            assert (tmp_path / "f.jpg").read_bytes() == g[f"video_{i}_jpeg"].tobytes(), (name, fr)
            i += 1


# ------------------------------------------------------------------------------------------------ 5. the command lines
def _frames(folder, sizes, seed):
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(seed))
    names = []
    for t, (H, W) in enumerate(sizes):
        yy, xx = np.mgrid[:H, :W]
        base = (np.stack([xx * 2.5 + 9 * t, yy * 3.5, (xx + yy) * 1.5], -1) % 256).astype(np.float32)
        img = np.clip(base + 8 * rng.standard_normal((H, W, 3)), 0, 255).astype(np.uint8)
        names.append(f"frame-{t:04d}.jpg")
        Image.fromarray(img).save(folder / names[-1], quality=92)
    return names


def test_video_generation_end_to_end(tmp_path):
    from PIL import Image
    from sais_amd import attnviz
    (tmp_path / "in").mkdir()
    names = _frames(tmp_path / "in", [(64, 96)] * 4, 291)
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "video_generation.py"), "--input_path", str(tmp_path / "in"),
                        "--output_path", str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "random (seeded) weights" in r.stdout
    try:
        import cv2  # noqa: F401
    except ImportError:
        assert "the video was not assembled" in r.stdout
    assert sorted(os.listdir(tmp_path / "out" / "attention")) == ["attn-" + n for n in names]
    args = types.SimpleNamespace(arch="vit_small", patch_size=16, pretrained_weights="", checkpoint_key="teacher")
    model = attnviz.build_model(args, torch.device(DEV))
    x = torch.stack([attnviz.load_frame(str(tmp_path / "in" / n)) for n in names]).to(DEV)
    _, rgb = attnviz.render(model.cls_attention(x), (4, 6), threshold=0.6, cmap="inferno", patch=16)
    for j, n in enumerate(names):
        im = Image.open(tmp_path / "out" / "attention" / ("attn-" + n))
        assert im.size == (96, 64) and im.mode == "RGB"
        attnviz.save_jpeg(str(tmp_path / "mine.jpg"), rgb[j])
        assert np.array_equal(np.asarray(im), np.asarray(Image.open(tmp_path / "mine.jpg"))), n


def test_visualize_attention_end_to_end(tmp_path):
    from PIL import Image
    (tmp_path / "in").mkdir()
    name = _frames(tmp_path / "in", [(160, 272)], 292)[0]
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "visualize_attention.py"), "--image_path", str(tmp_path / "in" / name),
                        "--image_size", "160", "272", "--threshold", "0.6", "--output_dir", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ["img.png"] + [f"attn-head{j}.png" for j in range(6)] + [f"mask_th0.6_head{j}.png" for j in range(6)]
    assert sorted(os.listdir(tmp_path / "out")) == sorted(want)
    for f in want:
        im = Image.open(tmp_path / "out" / f)
        assert im.size == (272, 160), f
        if f.startswith("mask"):
            a = np.asarray(im)
            assert im.mode == "L" and set(np.unique(a)) <= {0, 255} and 0 < (a == 255).mean() < 1
            assert np.array_equal(a, np.repeat(np.repeat(a[::16, ::16], 16, 0), 16, 1))
