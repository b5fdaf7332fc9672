#!/usr/bin/env python3
"""Golden vectors of the attention-map rendering path, produced by RUNNING THE REFERENCE's own code on the CPU (build container
only: needs /root/reference).

    python tests/golden/make_golden_attnviz.py        # rewrites tests/golden/attnviz.npz

Reference entry points exercised: vision_transformer.py's vit_small.get_last_selfattention (:216-223) off and on 224 x 224, and
SAIS/scripts/dino-main/video_generation.py's VideoGenerator._inference (:150-241).  That module imports cv2, torchvision and
tqdm at the top: cv2 is stubbed (never touched on this path), torchvision.transforms gets working stand-ins for the three
transforms _inference calls without --resize (Compose, ToTensor, Normalize), tqdm is the identity when absent.
  (i)   <case>_probs: get_last_selfattention(x)[:, :, 0, :] of the reference ViT under synth.vit_state_dict(seed=0) on
        vos_ref.dense_input frames, for attnviz_ref.CLS_CASES; inputs are regenerated from seeds and pinned by sha256
  (ii)  video_*: _inference on two 64 x 96 and two 160 x 272 synthetic JPEG frames with a stub model that hands out the
        attention of (i); F.interpolate is wrapped to record the mask `th_attn` of every frame (its first call per frame),
        plt.imsave to record `arr`.  Kept: the masks, the heat maps at patch resolution (asserted to be their own nearest
        upsampling) and the bytes of the JPEG files plt.imsave wrote
  (iii) tie_mask: the threshold block on attnviz_ref.tie_rows() — visualize_attention.py:186-195 is inline script code, and
        _inference's lines :197-205 are identical — recorded only if the reference's CPU torch.sort ordered the ties as the stable
        rule says.  It does NOT (torch 2.x's CPU sort without stable=True permutes equal values; the generator prints what it
        found): the tie case is dropped from the golden file and the stable rule stands on attnviz_ref alone
Asserted here, on the CPU: every recorded case has at most attnviz_ref.FRAGILE_CAP fragile elements per (frame, head) row, and
the reference's f32 masks equal the fp64 restatement on every non-fragile element."""
import glob
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import attnviz_ref as ar  # noqa: E402
import synth  # noqa: E402
import vos_ref  # noqa: E402

REF = "/root/reference/SAIS/scripts"


class Compose:
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, x):
        for t in self.ts:
            x = t(x)
        return x


class ToTensor:
    def __call__(self, img):                     # torchvision.transforms.functional.to_tensor for an RGB PIL image
        a = torch.from_numpy(np.array(img, dtype=np.uint8, copy=True))
        return a.permute(2, 0, 1).contiguous().to(torch.float32).div(255)


class Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = torch.tensor(mean).view(-1, 1, 1), torch.tensor(std).view(-1, 1, 1)

    def __call__(self, t):
        return t.clone().sub_(self.mean).div_(self.std)


def import_reference():
    for name in ("timm", "torchvision", "h5py", "cv2"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["cv2"].VideoWriter_fourcc = lambda *a: 0
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.ModuleType("tqdm")
        sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    tv = sys.modules["torchvision"]
    for sub in ("transforms", "models", "datasets"):
        m = types.ModuleType("torchvision." + sub)
        setattr(tv, sub, m)
        sys.modules["torchvision." + sub] = m
    tv.datasets.ImageFolder = object
    tv.transforms.Compose, tv.transforms.ToTensor, tv.transforms.Normalize = Compose, ToTensor, Normalize
    sys.path.insert(0, os.path.join(REF, "dino-main"))
    import matplotlib
    matplotlib.use("Agg")
    import video_generation as vg
    import vision_transformer as vits
    return vg, vits


def golden_probs(vits, out):
    torch.manual_seed(0)
    model = vits.vit_small(patch_size=16, num_classes=0)
    model.load_state_dict(synth.vit_state_dict(seed=0), strict=True)
    model.eval()
    for name, H, W, seed in ar.CLS_CASES:
        x = vos_ref.dense_input(H, W, seed)
        out[f"{name}_sha256"] = vos_ref.digest(x)
        with torch.no_grad():
            a = model.get_last_selfattention(torch.from_numpy(x))
        assert a.shape == (2, 6, 1 + (H // 16) * (W // 16), 1 + (H // 16) * (W // 16))
        out[f"{name}_probs"] = a[:, :, 0, :].numpy().astype(np.float32)
        print(name, tuple(a.shape), "max CLS probability", float(a[:, :, 0, :].max()))


class StubModel:
    """get_last_selfattention: [1, 6, 1, ntok] holding the next recorded CLS row (all _inference reads is [0, :, 0, 1:])"""

    def __init__(self, rows):
        self.rows, self.calls = rows, 0

    def get_last_selfattention(self, img):
        r = self.rows[self.calls]
        self.calls += 1
        assert r.shape[1] == 1 + (img.shape[-2] // 16) * (img.shape[-1] // 16)
        return torch.from_numpy(r.copy())[None, :, None, :]


def run_inference(vg, rows, sizes):
    """VideoGenerator._inference over synthetic JPEG frames of `sizes` [(H, W)] with the CLS rows `rows` -> per frame
    (mask u8 [6, h w], heat f32 [h, w], JPEG bytes)."""
    masks, arrs = [], []
    real_interp, real_imsave = vg.nn.functional.interpolate, vg.plt.imsave
    state = {"n": 0}

    def interp(x, *a, **k):
        if state["n"] % 2 == 0:                   # the first of a frame's two calls upsamples th_attn
            masks.append(x[0].reshape(x.shape[1], -1).numpy().astype(np.uint8))
        state["n"] += 1
        return real_interp(x, *a, **k)

    def imsave(fname, arr, **k):
        arrs.append(np.array(arr, copy=True))
        return real_imsave(fname=fname, arr=arr, **k)

    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(261))
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "frames"), os.path.join(tmp, "attention")
        os.makedirs(src), os.makedirs(dst)
        for i, (H, W) in enumerate(sizes):
            Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(os.path.join(src, f"frame-{i:04d}.jpg"))
        gen = vg.VideoGenerator.__new__(vg.VideoGenerator)
        gen.args = types.SimpleNamespace(resize=None, patch_size=16, threshold=ar.THRESHOLD)
        gen.model = StubModel(rows)
        vg.nn.functional.interpolate, vg.plt.imsave = interp, imsave
        try:
            with torch.no_grad():
                gen._inference(src, dst)
        finally:
            vg.nn.functional.interpolate, vg.plt.imsave = real_interp, real_imsave
        files = sorted(glob.glob(os.path.join(dst, "attn-*.jpg")))
        jpegs = [np.frombuffer(open(f, "rb").read(), dtype=np.uint8) for f in files]
    assert len(masks) == len(arrs) == len(jpegs) == len(sizes)
    heats = []
    for a, (H, W) in zip(arrs, sizes):
        assert a.dtype == np.float32 and a.shape == (H, W)
        small = a[::16, ::16]
        assert np.array_equal(np.repeat(np.repeat(small, 16, 0), 16, 1), a)
        heats.append(np.ascontiguousarray(small))
    return masks, heats, jpegs


def check_masks(name, p, mask, threshold):
    """p f32 [rows, n], mask u8 [rows, n] of the reference: the fragile cap, and equality with the restatement off the fragile"""
    frag = ar.fragile(p, threshold)
    mine = ar.mass_mask(p, threshold)
    worst = int(frag.sum(-1).max())
    diff = (mine != mask) & ~frag
    print(f"{name}: fragile per row at most {worst}, restatement differs on {int(diff.sum())} non-fragile elements")
    assert worst <= ar.FRAGILE_CAP, "change the seed of this case (attnviz_ref), not the cap"
    return not diff.any()


def golden_video(vg, out):
    rows, sizes = [], []
    for name in ar.VIDEO_CASES:
        H, W = next((h, w) for n, h, w, _ in ar.CLS_CASES if n == name)
        for fr in range(2):
            rows.append(out[f"{name}_probs"][fr])
            sizes.append((H, W))
    masks, heats, jpegs = run_inference(vg, rows, sizes)
    for i, (r, m, a, j) in enumerate(zip(rows, masks, heats, jpegs)):
        assert check_masks(f"video frame {i}", r[:, 1:], m, ar.THRESHOLD)
        assert np.array_equal(ar.heat(r[None, :, 1:], m[None])[0].reshape(a.shape), a), "heat restatement"
        out[f"video_{i}_mask"], out[f"video_{i}_heat"], out[f"video_{i}_jpeg"] = m, a, j
        print(f"video frame {i}: heat {a.shape}, jpeg {j.size} bytes")


def golden_ties(vg, out):
    t = ar.tie_rows()
    rows = [np.concatenate([np.zeros((t.shape[0], 1), np.float32), t], axis=1)]
    masks, _, _ = run_inference(vg, rows, [(64, 96)])
    frag = ar.fragile(t, ar.THRESHOLD)
    stable = np.array_equal(ar.mass_mask(t, ar.THRESHOLD)[~frag], masks[0][~frag]) and int(frag.sum(-1).max()) <= ar.FRAGILE_CAP
    print("tie rows: the reference's torch.sort", "follows" if stable else "DOES NOT follow", "the stable rule;",
          "recorded" if stable else "dropped: the rule stands on attnviz_ref alone")
    if stable:
        out["tie_mask"] = masks[0]


if __name__ == "__main__":
    vg, vits = import_reference()
    out = {}
    golden_probs(vits, out)
    golden_video(vg, out)
    golden_ties(vg, out)
    np.savez_compressed(os.path.join(HERE, "attnviz.npz"), **out)
    print(len(out), "arrays,", os.path.getsize(os.path.join(HERE, "attnviz.npz")), "bytes")
