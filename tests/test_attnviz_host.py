"""CPU-only half of the attention-rendering tests: tests/attnviz_ref.py is held to matplotlib itself and to what the reference's
own code recorded (tests/golden/make_golden_attnviz.py); the host helpers of sais_amd.attnviz (colormap tables, image files,
frame loading); the argument checks of the new library entries; the command lines."""
import ctypes
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

import attnviz_ref as ar
import vos_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "SAIS", "scripts", "dino-main")


def _mpl():
    mpl = pytest.importorskip("matplotlib", reason="matplotlib is the reference of the colormap restatement")
    mpl.use("Agg")
    return mpl


def _script(name):
    spec = importlib.util.spec_from_file_location("attnviz_cli_" + name, os.path.join(SCRIPTS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _adversarial_maps():
    rng = np.random.Generator(np.random.PCG64(271))
    rnd = rng.random((7, 9)).astype(np.float32)
    lo, hi = np.float32(0.125), np.float32(0.8125)
    edges = np.array([[lo, np.nextafter(lo, hi), np.nextafter(hi, lo), hi, (lo + hi) / 2, lo]], dtype=np.float32)
    steps = (np.float32(3.0) + np.arange(512, dtype=np.float32) * np.float32(7.0 / 511)).reshape(16, 32)     # every index, and
    tiny = (rng.random((5, 5)) * 1e-30).astype(np.float32)                                                     # their borders
    return {"constant": np.full((4, 6), 0.37, np.float32), "zero": np.zeros((3, 3), np.float32),
            "two_valued": np.where(rng.random((6, 5)) < 0.5, np.float32(0.2), np.float32(0.7)).astype(np.float32),
            "edges": edges, "random": rnd, "steps": steps, "tiny": tiny, "one": np.array([[0.5]], np.float32),
            "exp": np.exp(rng.standard_normal((10, 17)) * 3).astype(np.float32)}


@pytest.mark.parametrize("cmap", ["inferno", "viridis"])
def test_to_rgb_is_matplotlibs_to_rgba(cmap):
    _mpl()
    from matplotlib.cm import ScalarMappable
    from sais_amd import attnviz
    lut = attnviz.colormap_lut(cmap)
    for name, a in _adversarial_maps().items():
        ref = ScalarMappable(cmap=cmap).to_rgba(a, bytes=True)[..., :3]
        assert np.array_equal(ar.to_rgb(a[None], lut)[0], ref), name
    a = _adversarial_maps()["random"]
    big = ScalarMappable(cmap=cmap).to_rgba(np.repeat(np.repeat(a, 16, 0), 16, 1), bytes=True)[..., :3]
    assert np.array_equal(ar.to_rgb(a[None], lut, 16)[0], big)            # nearest upsampling commutes with the colormap


def test_colormap_tables():
    _mpl()
    from matplotlib import colormaps
    from sais_amd import _cmap_tables, attnviz
    for name in ("inferno", "viridis"):
        ref = colormaps[name](np.arange(256), bytes=True)[:, :3]          # integer input: the table rows themselves
        lut = attnviz.colormap_lut(name)
        assert lut.dtype == np.uint8 and lut.shape == (256, 3) and np.array_equal(lut, ref)
        bundled = np.frombuffer(bytes.fromhex(_cmap_tables.HEX[name]), dtype=np.uint8).reshape(256, 3)
        assert np.array_equal(bundled, ref), name


def test_image_files_equal_imsave(tmp_path):
    _mpl()
    import matplotlib.pyplot as plt
    from sais_amd import attnviz
    a = _adversarial_maps()["exp"]
    big = np.repeat(np.repeat(a, 16, 0), 16, 1)
    buf = io.BytesIO()
    plt.imsave(buf, arr=big, cmap="inferno", format="jpg")
    attnviz.save_jpeg(str(tmp_path / "a.jpg"), ar.to_rgb(a[None], attnviz.colormap_lut("inferno"), 16)[0])
    assert (tmp_path / "a.jpg").read_bytes() == buf.getvalue()
    buf = io.BytesIO()
    plt.imsave(buf, arr=big, format="png")                                # the default colormap: viridis
    attnviz.save_png(str(tmp_path / "a.png"), torch.from_numpy(ar.to_rgb(a[None], attnviz.colormap_lut("viridis"), 16)[0]))
    assert (tmp_path / "a.png").read_bytes() == buf.getvalue()
    with pytest.raises(ValueError):
        attnviz.save_jpeg(str(tmp_path / "b.jpg"), np.zeros((4, 4), np.uint8))


def test_restatements_reproduce_the_reference_records(golden):
    g = golden("attnviz")
    for name, H, W, seed in ar.CLS_CASES:
        assert np.array_equal(vos_ref.digest(vos_ref.dense_input(H, W, seed)), g[f"{name}_sha256"]), name
        p = g[f"{name}_probs"]
        assert p.shape == (2, 6, 1 + (H // 16) * (W // 16)) and np.abs(p.sum(-1) - 1).max() <= 1e-5
    i = 0
    for name in ar.VIDEO_CASES:
        for fr in range(2):
            p = g[f"{name}_probs"][fr][:, 1:]
            mask, heat = g[f"video_{i}_mask"], g[f"video_{i}_heat"]
            frag = ar.fragile(p, ar.THRESHOLD)
            assert frag.sum(-1).max() <= ar.FRAGILE_CAP
            assert not ((ar.mass_mask(p, ar.THRESHOLD) != mask) & ~frag).any(), (name, fr)
            got = ar.heat(p[None], mask[None])[0].reshape(heat.shape)
            assert got.dtype == np.float32 and np.array_equal(got, heat), (name, fr)       # bit for bit
            i += 1
    assert "tie_mask" not in g.files       # the reference's torch.sort is not stable: the tie rule stands on attnviz_ref alone


def test_golden_jpegs_are_the_colours_of_the_golden_heat_maps(golden, tmp_path):
    """the whole tail on the host: recorded heat map -> to_rgb -> save_jpeg == the file plt.imsave wrote in the reference run"""
    from sais_amd import attnviz
    g = golden("attnviz")
    for i in range(4):
        rgb = ar.to_rgb(g[f"video_{i}_heat"][None], attnviz.colormap_lut("inferno"), 16)[0]
        attnviz.save_jpeg(str(tmp_path / "f.jpg"), rgb)
        assert (tmp_path / "f.jpg").read_bytes() == g[f"video_{i}_jpeg"].tobytes(), i


def test_mass_mask_restatement_rules():
    t = ar.tie_rows()
    m = ar.mass_mask(t, 0.6)
    for row, keep in zip(t, m):                       # stable: among equal values the LATER indices are kept first
        for v in np.unique(row):
            k = keep[row == v]
            assert np.array_equal(k, np.sort(k)), (v, k)
    assert ar.mass_mask(np.zeros((2, 5), np.float32), 0.6).sum() == 0               # a zero row keeps nothing
    assert ar.mass_mask(np.array([[1.0]], np.float32), 0.1).tolist() == [[1]]
    p = np.array([[0.1, 0.2, 0.3, 0.4]], np.float32)
    assert ar.mass_mask(p, 0.6).tolist() == [[0, 0, 1, 1]] and ar.mass_mask(p, 0.95).tolist() == [[1, 1, 1, 1]]
    h = ar.heat(p.reshape(1, 2, 2), np.array([[[1, 0], [1, 1]]], np.uint8))
    assert np.array_equal(h, np.array([[np.float32(0.1) / np.float32(2) + np.float32(0.3) / np.float32(2),
                                        np.float32(0.0) + np.float32(0.4) / np.float32(2)]], np.float32))
    assert np.array_equal(ar.heat(p.reshape(1, 2, 2), None, 1, 1), p.reshape(1, 2, 2)[:, 1])     # one head: the map itself


def test_cls_probs_restatement():
    rng = np.random.Generator(np.random.PCG64(272))
    qkv = rng.standard_normal((2 * 5, 1152))
    p = ar.cls_probs(qkv, 2, 5)
    assert p.shape == (2, 6, 5) and np.abs(p.sum(-1) - 1).max() < 1e-12
    s = np.array([qkv[5, 64:128] @ qkv[5 + j, 384 + 64:384 + 128] for j in range(5)]) / 8       # frame 1, head 1
    assert np.allclose(p[1, 1], np.exp(s) / np.exp(s).sum(), rtol=1e-12)


def test_new_entries_reject_bad_arguments_without_a_gpu():
    from sais_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)

    def probs(q=p, k=p, out=p, ldq=384, ldk=1152, frames=1, ntok=25):
        return lib.sais_vit_cls_probs(q, ldq, k, ldk, frames, ntok, out, None)
    assert probs(q=None) == -1 and probs(k=None) == -1 and probs(out=None) == -1
    assert probs(ntok=1) == -1 and probs(ntok=4098) == -1 and probs(ntok=0) == -1
    assert probs(frames=0) == -1 and probs(frames=-1) == -1
    assert probs(ldk=1150) == -1 and probs(ldq=380) == -1 and probs(k=ctypes.c_void_p(66)) == -1

    def mask(src=p, keep=p, ldp=5000, rows=1, n=24, threshold=0.6):
        return lib.sais_attn_mass_mask(src, ldp, rows, n, threshold, keep, None)
    assert mask(src=None) == -1 and mask(keep=None) == -1
    assert mask(n=0) == -1 and mask(n=4097) == -1 and mask(rows=0) == -1 and mask(ldp=23) == -1
    assert mask(threshold=0.0) == -1 and mask(threshold=1.0) == -1 and mask(threshold=float("nan")) == -1

    def render(src=p, keep=None, lut=p, heat=p, rgb=p, ws=p, ldp=25, frames=1, nh=6, head0=0, nheads=6, h=4, w=6, n=24, patch=16):
        return lib.sais_attn_render(src, ldp, keep, frames, nh, head0, nheads, h, w, n, patch, lut, heat, rgb, ws, None)
    assert render(src=None) == -1 and render(heat=None) == -1 and render(lut=None) == -1 and render(ws=None) == -1
    assert render(h=4, w=5) == -1 and render(n=25) == -1                 # h * w != n
    assert render(patch=0) == -1 and render(patch=65) == -1
    assert render(head0=1) == -1 and render(nheads=0) == -1 and render(head0=-1, nheads=1) == -1 and render(frames=0) == -1
    assert render(h=65, w=64, n=4160, ldp=4161) == -1 and render(ldp=23) == -1


def test_host_tensors_raise_without_a_gpu():
    from sais_amd import _lib, attnviz
    from sais_amd.vit import vit_small
    with pytest.raises(ValueError):
        attnviz.mass_mask(torch.zeros(1, 6, 25), 0.6)
    with pytest.raises(ValueError):
        attnviz.render(torch.zeros(1, 6, 25), (4, 6))
    with pytest.raises(_lib.SaisHipError):
        vit_small(patch_size=16).cls_attention(torch.zeros(1, 3, 64, 96))


def test_resize_rule_and_frame_loading(tmp_path):
    from PIL import Image
    from sais_amd import attnviz
    assert attnviz.resize_size(848, 480, [240]) == (424, 240)             # (width, height): the short side becomes 240
    assert attnviz.resize_size(480, 848, 240) == (240, 424)
    assert attnviz.resize_size(853, 480, [100]) == (177, 100)             # int(100 * 853 / 480): truncated
    assert attnviz.resize_size(848, 480, [64, 96]) == (96, 64)            # two ints: (h, w)
    with pytest.raises(ValueError):
        attnviz.resize_size(10, 10, [1, 2, 3])
    rng = np.random.Generator(np.random.PCG64(273))
    a = rng.integers(0, 256, size=(70, 100, 3), dtype=np.uint8)
    Image.fromarray(a).save(tmp_path / "a.png")
    x = attnviz.load_frame(str(tmp_path / "a.png"))
    assert x.shape == (3, 64, 96) and x.dtype == torch.float32            # cropped to multiples of 16
    t = torch.from_numpy(a[:64, :96]).permute(2, 0, 1).float().div(255)   # ToTensor + Normalize in torch's own f32
    t = t.sub(torch.tensor(attnviz.MEAN).view(3, 1, 1)).div(torch.tensor(attnviz.STD).view(3, 1, 1))
    assert torch.equal(x, t)
    assert attnviz.load_frame(str(tmp_path / "a.png"), [32, 48]).shape == (3, 32, 48)
    u8 = attnviz.input_image_u8(x.numpy())
    ref = x.clone()
    lo, hi = float(ref.min()), float(ref.max())                            # make_grid's norm_ip + save_image's conversion
    ref.clamp_(min=lo, max=hi).sub_(lo).div_(max(hi - lo, 1e-5))
    ref = ref.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
    assert np.array_equal(u8, ref)
    Image.fromarray(a[:10]).save(tmp_path / "small.png")
    with pytest.raises(ValueError):
        attnviz.load_frame(str(tmp_path / "small.png"))                   # less than one patch


def test_video_generation_command_line(tmp_path, capsys):
    vg = _script("video_generation")
    args = vg.get_args_parser().parse_args(["--input_path", "frames"])
    assert (args.threshold, args.resize, args.video_only, args.fps, args.video_format) == (0.6, None, False, 30.0, "mp4")
    assert (args.arch, args.patch_size, args.pretrained_weights, args.checkpoint_key, args.output_path, args.bs) == \
        ("vit_small", 16, "", "teacher", "./", 8)
    args = vg.get_args_parser().parse_args(["--input_path", "x", "--resize", "480", "848", "--video_format", "avi", "--bs", "3",
                                            "--video_only", "--threshold", "0.3"])
    assert (args.resize, args.video_format, args.bs, args.video_only, args.threshold) == ([480, 848], "avi", 3, True, 0.3)
    with pytest.raises(SystemExit):
        vg.get_args_parser().parse_args([])                                # --input_path is required
    with pytest.raises(SystemExit):
        vg.main(["--input_path", str(tmp_path / "missing")])
    assert "doesn't exists" in capsys.readouterr().out
    if vg.import_cv2() is not None:
        return
    (tmp_path / "clip.mp4").write_bytes(b"not a video")
    with pytest.raises(SystemExit):                                        # a video file cannot be read without cv2
        vg.main(["--input_path", str(tmp_path / "clip.mp4"), "--output_path", str(tmp_path)])
    assert vg.NO_CV2_VIDEO_IN in capsys.readouterr().out
    (tmp_path / "attention").mkdir()
    vg.main(["--input_path", str(tmp_path / "attention"), "--output_path", str(tmp_path), "--video_only"])
    assert vg.NO_CV2_VIDEO_OUT in capsys.readouterr().out and not (tmp_path / "video.mp4").exists()


def test_visualize_attention_command_line(tmp_path, capsys):
    va = _script("visualize_attention")
    args = va.get_args_parser().parse_args(["--image_path", "a.png"])
    assert (tuple(args.image_size), args.threshold, args.output_dir, args.patch_size, args.arch) == ((480, 480), None, ".", 16,
                                                                                                     "vit_small")
    args = va.get_args_parser().parse_args(["--image_path", "a.png", "--image_size", "160", "272", "--threshold", "0.6"])
    assert (args.image_size, args.threshold) == ([160, 272], 0.6)
    with pytest.raises(SystemExit):
        va.get_args_parser().parse_args([])                                # --image_path is required: nothing is downloaded
    with pytest.raises(SystemExit):
        va.main(["--image_path", str(tmp_path / "missing.png")])
    assert "non valid" in capsys.readouterr().out
