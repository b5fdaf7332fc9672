"""CPU-only half of the video-segmentation tests: tests/vos_ref.py is pinned to what the reference's own functions recorded
(tests/golden/make_golden_vos.py), the host helpers of sais_amd.vos, and the argument checks of the new library entries."""
import ctypes

import numpy as np
import pytest
import torch

import vos_ref


def test_fp64_restatement_matches_the_reference_records(golden):
    g = golden("vos")
    for name, h, w, nctx, C, r, topk, seed in vos_ref.GOLDEN_CASES:
        tar, ctx, segs = vos_ref.make_case(h, w, nctx, C, r, topk, seed)
        assert np.array_equal(vos_ref.digest(tar, ctx, segs), g[f"{name}_sha256"]), name
        frag = vos_ref.fragile_queries(tar, ctx, h, w, r, topk)
        assert frag.mean() <= vos_ref.FRAGILE_CAP, name
        err = np.abs(vos_ref.propagate(tar, ctx, segs, h, w, r, topk) - g[f"{name}_out"])[:, ~frag].max()
        assert err <= 1e-5, (name, err)            # the reference's own fp32 arithmetic against fp64


def test_corner_queries_keep_their_whole_window():
    """r = 1, one context frame: a corner sees 4 < topk keys, every one of them is kept"""
    name, h, w, nctx, C, r, topk, seed = vos_ref.GOLDEN_CASES[1]
    tar, ctx, segs = vos_ref.make_case(h, w, nctx, C, r, topk, seed)
    out = vos_ref.propagate(tar, ctx, segs, h, w, r, topk)
    a = np.exp(vos_ref.cosines(tar, ctx)[0][:, 0] / 0.1)
    keys = [0, 1, w, w + 1]
    assert np.allclose(out[:, 0], (segs[0][:, keys] * a[keys]).sum(1) / a[keys].sum(), rtol=1e-12)


def test_sequence_restatement_matches_the_reference_queue(golden):
    g, s = golden("vos"), vos_ref.SEQ
    feats, first = vos_ref.make_sequence()
    assert np.array_equal(vos_ref.digest(feats, first), g["seq_sha256"])
    frag = []
    segs = vos_ref.run_sequence(feats, first, s["h"], s["w"], s["n_last_frames"], s["r"], s["topk"], frag)
    assert not any(frag)
    assert segs.shape == g["seq_segs"].shape and np.abs(segs - g["seq_segs"]).max() <= 1e-5


def test_upsample_restatement_matches_the_reference_records(golden):
    g = golden("vos")
    for name, C, h, w, patch, seed, special in vos_ref.UPSAMPLE_CASES:
        seg = vos_ref.make_upsample_case(C, h, w, patch, seed, special)
        assert np.array_equal(vos_ref.digest(seg), g[f"{name}_sha256"])
        labels, near = vos_ref.upsample_argmax(seg, patch)
        assert near.mean() <= vos_ref.ARGMAX_EXCEPT_CAP
        assert not ((labels != g[f"{name}_labels"]) & ~near).any(), name
    # a constant positive channel is 0 / 0 after norm_mask and wins every pixel, as torch.max does with a NaN
    assert (g["u1_labels"] == 2).all()


def test_target_size_rule():
    from sais_amd import vos
    assert vos.target_size(480, 854) == (480, 832)         # DAVIS 480p: 30 x 52 patches
    assert vos.target_size(854, 480) == (832, 480)
    assert vos.target_size(96, 160) == (480, 768)
    assert vos.target_size(1080, 1920) == (480, 832)
    assert vos.target_size(500, 500) == (480, 448)         # the long-side rule floors the square too


def test_to_one_hot():
    from sais_amd import vos
    y = torch.tensor([[[0, 2, 1], [1, 1, 0]]]).float()
    oh = vos.to_one_hot(y)
    assert oh.shape == (1, 3, 2, 3) and oh.dtype == torch.float32
    assert torch.equal(oh[0].argmax(0), y[0].long()) and torch.equal(oh.sum(1), torch.ones(1, 2, 3))
    assert vos.to_one_hot(y, 5).shape == (1, 5, 2, 3)


def test_palette_round_trip(tmp_path):
    from PIL import Image
    from sais_amd import vos
    palette = np.zeros((256, 3), dtype=np.uint8)
    palette[1], palette[2], palette[255] = (128, 0, 0), (0, 128, 0), (224, 224, 192)
    lab = np.zeros((96, 160), dtype=np.uint8)
    lab[10:40, 20:90] = 1
    lab[50:90, 100:150] = 2
    vos.imwrite_indexed(str(tmp_path / "a.png"), lab, palette)
    one_hot, seg_ori, pal = vos.read_seg(str(tmp_path / "a.png"), 16)
    assert np.array_equal(seg_ori, lab) and np.array_equal(pal, palette)
    assert one_hot.shape == (1, 3, 30, 48)                 # (480 / 16, 768 / 16)
    vos.imwrite_indexed(str(tmp_path / "b.png"), seg_ori, pal)
    assert (tmp_path / "a.png").read_bytes() == (tmp_path / "b.png").read_bytes()
    assert Image.open(tmp_path / "b.png").mode == "P"
    with pytest.raises(ValueError):
        vos.imwrite_indexed(str(tmp_path / "c.png"), np.zeros((4, 4, 3), np.uint8), palette)


def test_host_tensors_raise_without_a_gpu():
    from sais_amd import vos
    with pytest.raises(ValueError):
        vos.label_propagation(torch.zeros(20, 384), torch.zeros(2, 20, 384), torch.zeros(2, 3, 20), 4, 5, 2, 5)
    with pytest.raises(ValueError):
        vos.upsample_argmax(torch.zeros(3, 4, 5), 16)


def test_new_entries_reject_bad_arguments_without_a_gpu():
    from sais_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert lib.sais_vit_attn_fwd_any(None, 1152, 1, 171, None, 384, None, None) == -1
    assert lib.sais_vit_attn_fwd_any(p, 1152, 1, 1, p, 384, None, None) == -1            # ntok < 2
    assert lib.sais_vit_attn_fwd_any(p, 1152, 1, 4098, p, 384, None, None) == -1         # ntok > 4097
    assert lib.sais_vit_attn_fwd_any(p, 1150, 1, 171, p, 384, None, None) == -1          # row stride
    assert lib.sais_vit_attn_fwd_any(p, 1152, 0, 171, p, 384, None, None) == -1
    assert lib.sais_patchify_rect(None, 1, 160, 272, None, None) == -1
    assert lib.sais_patchify_rect(p, 1, 168, 272, p, None) == -1                         # H % 16
    assert lib.sais_patchify_rect(p, 1, 160, 0, p, None) == -1
    ok = dict(nctx=2, C=3, h=4, w=5, dim=384, radius=2, topk=5)

    def propagate(tar=p, **kw):
        a = dict(ok, **kw)
        return lib.sais_vos_propagate(tar, p, p, a["nctx"], a["C"], a["h"], a["w"], a["dim"], a["radius"], a["topk"], None, p, None)
    assert propagate(tar=None) == -1
    assert propagate(nctx=17) == -1 and propagate(nctx=0) == -1
    assert propagate(C=65) == -1 and propagate(C=0) == -1
    assert propagate(topk=0) == -1 and propagate(topk=17) == -1
    assert propagate(dim=256) == -1
    assert propagate(h=65, w=64) == -1                                                   # 4160 patches
    assert propagate(radius=-1) == -1
    order = (ctypes.c_int * 2)(0, 16)
    assert lib.sais_vos_propagate(p, p, p, 2, 3, 4, 5, 384, 2, 5, order, p, None) == -1  # slot out of range
    assert lib.sais_vos_upsample_argmax(None, 3, 4, 5, 16, None, None, None) == -1
    assert lib.sais_vos_upsample_argmax(p, 65, 4, 5, 16, p, p, None) == -1
    assert lib.sais_vos_upsample_argmax(p, 3, 4, 5, 0, p, p, None) == -1
    assert lib.sais_vos_upsample_argmax(p, 3, 65, 64, 16, p, p, None) == -1
