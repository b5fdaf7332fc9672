"""Cases, input generators, digests and the synthetic state dict of the patch-8 backbone tests (ViT-S/8: vit_small(patch_size=8),
dino-main/vision_transformer.py:243-247).  Shared by test_vit8_host.py, test_vit8_gpu.py and golden/make_golden_vit8.py; numpy
and torch on the CPU only."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import synth  # noqa: E402

PATCH, GRID0, NTOK0, DIM = 8, 28, 785, 384
FEAT_REL = 2e-2             # the project's one feature bar: |got - ref| <= FEAT_REL * max|ref|
ATTN_TOL = 2e-3             # max-abs bar of a softmax row (attnviz)
ROWSUM_TOL = 1e-5
N_LAST = 4                  # get_intermediate_layers(x, 4): the linear probe's n_last_blocks

# name, F, H, W, seed
CASES = [
    ("c64x88", 2, 64, 88, 801),         # 89 tokens: non-square, interpolated; a transposed grid shows here
    ("c224x224", 2, 224, 224, 802),     # 785 tokens: the positional table is the parameter itself
    ("c112x448", 1, 112, 448, 803),     # 784 patches, not square: interpolated
    ("c512x512", 1, 512, 512, 804),     # 4097 tokens: the cap
]


def ntok(H, W):
    return 1 + (H // PATCH) * (W // PATCH)


def rows(H, W):
    """The token rows of a case the golden file keeps (of the features and, past 100 tokens, of the positional table): the CLS
    row and patches on every border and in the middle of the (H/8, W/8) grid."""
    gw, n = W // PATCH, ntok(H, W)
    return sorted({0, 1, 2, gw, gw + 1, gw + 2, n // 2, n // 2 + 1, n - gw - 1, n - gw, n - 2, n - 1})


def frames(F, H, W, seed):
    """frames f32 [F, 3, H, W] ~ N(0, 1): normalised pixels"""
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((F, 3, H, W)).astype(np.float32)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def state_dict(seed=0):
    """synth.vit_state_dict(seed) with patch_embed.proj.weight [384, 3, 8, 8] and pos_embed [1, 785, 384] from the same kind of
    draws (N(0, 0.04^2) / N(0, 0.05^2)) of a generator of their own: every other tensor is the patch-16 fixture's."""
    sd = synth.vit_state_dict(seed=seed)
    g = torch.Generator(device="cpu")
    g.manual_seed(8000 + int(seed))
    sd["patch_embed.proj.weight"] = (torch.randn(DIM, 3, PATCH, PATCH, generator=g) * 0.04).float()
    sd["pos_embed"] = (torch.randn(1, NTOK0, DIM, generator=g) * 0.05).float()
    return sd


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit8.npz"))
