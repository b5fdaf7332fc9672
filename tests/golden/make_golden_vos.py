#!/usr/bin/env python3
"""Golden vectors of the video-segmentation path, produced by RUNNING THE REFERENCE's own functions on the CPU (build
container only: needs /root/reference).

    python tests/golden/make_golden_vos.py        # rewrites tests/golden/vos.npz

Reference entry points exercised (SAIS/scripts/dino-main/eval_video_segmentation.py): label_propagation (:113-150, with
restrict_neighborhood :85-99 and extract_feature :153-163), eval_video_tracking_davis (:38-82: the queue, the upsampling,
norm_mask :102-110 and the argmax) and vision_transformer.py's vit_small.get_intermediate_layers (:225-233, with
interpolate_pos_encoding :174-194) off 224 x 224.  The module imports cv2 and torchvision at the top: both are stubbed and
never touched on these paths; torch.Tensor.cuda is the identity; the module global `args` is set; a stub model hands out the
generated features (a frame is a constant image whose value is the frame's number).
  (i)   <case>_out: label_propagation on the cases of vos_ref.GOLDEN_CASES; inputs are regenerated from seeds and pinned by sha256
  (ii)  dense features of the reference ViT under synth.vit_state_dict(seed=0) for vos_ref.DENSE_CASES
  (iii) <case>_labels: F.interpolate + norm_mask + torch.max for vos_ref.UPSAMPLE_CASES
  (iv)  seq_segs: the soft mask of every frame of vos_ref.SEQ, captured from eval_video_tracking_davis's own queue
Every propagation output is compared with the fp64 restatement of vos_ref here, and the fragile-query caps are asserted."""
import os
import sys
import tempfile
import types

import numpy as np
import torch
from torch.nn import functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import synth  # noqa: E402
import vos_ref  # noqa: E402

REF = "/root/reference/SAIS/scripts"


def import_reference():
    for name in ("timm", "torchvision", "h5py", "cv2"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    tv = sys.modules["torchvision"]
    for sub in ("transforms", "models", "datasets"):
        m = types.ModuleType("torchvision." + sub)
        setattr(tv, sub, m)
        sys.modules["torchvision." + sub] = m
    tv.datasets.ImageFolder = object
    sys.path.insert(0, os.path.join(REF, "dino-main"))
    torch.Tensor.cuda = lambda self, *a, **k: self
    import eval_video_segmentation as evs
    import vision_transformer as vits
    return evs, vits


class StubModel:
    """get_intermediate_layers of a frame whose pixels all hold its number: [1, 1 + n, 384] with a zero CLS row"""

    def __init__(self, feats):
        self.feats = feats
        self.patch_embed = types.SimpleNamespace(patch_size=16)

    def get_intermediate_layers(self, x, n=1):
        f = torch.from_numpy(self.feats[int(x[0, 0, 0, 0])])
        return [torch.cat([torch.zeros(1, f.shape[1]), f])[None]]


def frame(idx, h, w):
    return torch.full((3, h * 16, w * 16), float(idx))


def golden_propagation(evs, out):
    for name, h, w, nctx, C, r, topk, seed in vos_ref.GOLDEN_CASES:
        tar, ctx, segs = vos_ref.make_case(h, w, nctx, C, r, topk, seed)
        out[f"{name}_sha256"] = vos_ref.digest(tar, ctx, segs)
        evs.args = args = types.SimpleNamespace(size_mask_neighborhood=r, topk=topk)
        model = StubModel([tar])
        with torch.no_grad():
            seg, feat_t, _ = evs.label_propagation(args, model, frame(0, h, w), [torch.from_numpy(c).T for c in ctx],
                                                   [torch.from_numpy(s).reshape(1, C, h, w) for s in segs])
        got = seg[0].reshape(C, h * w).numpy()
        assert np.array_equal(feat_t.T.numpy(), tar)
        ref64 = vos_ref.propagate(tar, ctx, segs, h, w, r, topk)
        nfrag = int(vos_ref.fragile_queries(tar, ctx, h, w, r, topk).sum())
        err = np.abs(got - ref64).max()
        print(f"{name}: reference vs fp64 restatement {err:.2e}; fragile queries {nfrag} of {h * w}")
        assert nfrag <= vos_ref.FRAGILE_CAP * h * w, "change the seed of this case (vos_ref.GOLDEN_CASES), not the cap"
        assert err <= 1e-5 or nfrag, err
        out[f"{name}_out"] = got.astype(np.float32)
    for case, maker in ((vos_ref.WORKLOAD_CASE, vos_ref.make_case), (vos_ref.TIE_CASE, lambda *a: vos_ref.make_tie_case())):
        name, h, w, nctx, C, r, topk, seed = case
        tar, ctx, _ = maker(h, w, nctx, C, r, topk, seed)
        nfrag = int(vos_ref.fragile_queries(tar, ctx, h, w, r, topk).sum())
        print(f"{name}: fragile queries {nfrag} of {h * w}")
        assert nfrag <= vos_ref.FRAGILE_CAP * h * w, "change the seed of this case, not the cap"


def golden_dense(vits, out):
    torch.manual_seed(0)
    model = vits.vit_small(patch_size=16, num_classes=0)
    model.load_state_dict(synth.vit_state_dict(seed=0), strict=True)
    model.eval()
    for name, H, W, n, seed in vos_ref.DENSE_CASES:
        x = vos_ref.dense_input(H, W, seed)
        out[f"{name}_sha256"] = vos_ref.digest(x)
        with torch.no_grad():
            inter = model.get_intermediate_layers(torch.from_numpy(x), n)
        a = np.stack([t.numpy() for t in inter])                          # [n, F, ntok, 384]
        assert a.shape[2] == 1 + (H // 16) * (W // 16)
        out[name] = a if a.shape[2] <= 171 else a[:, :, vos_ref.DENSE_ROWS]
        print(name, a.shape, "max|ref|", float(np.abs(a).max()))


def golden_upsample(evs, out):
    for name, C, h, w, patch, seed, special in vos_ref.UPSAMPLE_CASES:
        seg = vos_ref.make_upsample_case(C, h, w, patch, seed, special)
        out[f"{name}_sha256"] = vos_ref.digest(seg)
        up = F.interpolate(torch.from_numpy(seg)[None], scale_factor=patch, mode="bilinear", align_corners=False,
                           recompute_scale_factor=False)[0]               # :74
        _, lab = torch.max(evs.norm_mask(up), dim=0)                      # :75-76
        lab = lab.numpy().astype(np.uint8)
        mine, near = vos_ref.upsample_argmax(seg, patch)
        diff = (mine != lab) & ~near
        print(f"{name}: labels {np.bincount(lab.ravel())}, near-tie pixels {near.mean():.4f}, restatement differs on {int(diff.sum())}")
        assert near.mean() <= vos_ref.ARGMAX_EXCEPT_CAP, "change the seed of this case, not the cap"
        assert not diff.any()
        out[f"{name}_labels"] = lab


def golden_sequence(evs, out):
    s = vos_ref.SEQ
    h, w, C = s["h"], s["w"], s["C"]
    feats, first = vos_ref.make_sequence()
    out["seq_sha256"] = vos_ref.digest(feats, first)
    captured = []

    class Copy:                                   # `seg = copy.deepcopy(frame_tar_avg)` (:70) is what enters the queue
        @staticmethod
        def deepcopy(t):
            captured.append(t[0].reshape(C, h * w).numpy().copy())
            return t.clone()
    evs.copy = Copy
    evs.read_frame = lambda path, scale_size=[480]: (frame(int(os.path.basename(path).split(".")[0]), h, w), h * 16, w * 16)
    evs.imwrite_indexed = lambda *a, **k: None
    with tempfile.TemporaryDirectory() as tmp:
        evs.args = args = types.SimpleNamespace(size_mask_neighborhood=s["r"], topk=s["topk"], n_last_frames=s["n_last_frames"],
                                                patch_size=16, output_dir=tmp)
        evs.eval_video_tracking_davis(args, StubModel(list(feats)), [f"{i:05d}.jpg" for i in range(s["frames"])], "video",
                                      torch.from_numpy(first).reshape(1, C, h, w), np.zeros((h * 16, w * 16), np.uint8), None)
    got = np.stack(captured)
    frag = []
    ref64 = vos_ref.run_sequence(feats, first, h, w, s["n_last_frames"], s["r"], s["topk"], frag)
    print("sequence: reference vs fp64 restatement", float(np.abs(got - ref64).max()), "fragile per frame", frag)
    assert not any(frag), "the sequence must have no fragile query: change vos_ref.SEQ['seed']"
    assert np.abs(got - ref64).max() <= 1e-5
    out["seq_segs"] = got.astype(np.float32)


if __name__ == "__main__":
    evs, vits = import_reference()
    out = {}
    golden_propagation(evs, out)
    golden_dense(vits, out)
    golden_upsample(evs, out)
    golden_sequence(evs, out)
    np.savez_compressed(os.path.join(HERE, "vos.npz"), **out)
    print(len(out), "arrays,", os.path.getsize(os.path.join(HERE, "vos.npz")), "bytes")
