#!/usr/bin/env python3
"""Golden vectors of the patch-8 backbone, produced by RUNNING THE REFERENCE's own vision_transformer.vit_small(patch_size=8) on
the CPU (build container only: needs /root/reference).

    python tests/golden/make_golden_vit8.py        # rewrites tests/golden/vit8.npz

Reference entry points exercised (SAIS/scripts/dino-main/vision_transformer.py): VisionTransformer.forward (:209-214),
get_intermediate_layers (:225-233), get_last_selfattention (:216-223), interpolate_pos_encoding (:174-194) under
vit8_ref.state_dict(seed=0), for vit8_ref.CASES.  The module imports nothing this script has to stub beyond what
make_golden_vos.py stubs.  Per case: <name>_sha256 (the input), <name>_fwd = model(x) [F, 384], <name>_cls = the CLS rows of
get_intermediate_layers(x, 4) [4, F, 384], <name>_rows = the rows vit8_ref.rows of its last two [2, F, R, 384], <name>_attn =
get_last_selfattention(x)[:, :, 0, :] [F, 6, ntok], <name>_pos = the interpolated positional table (every row up to 100 tokens,
else the rows of vit8_ref.rows).  Also the reference's parameter count and state-dict shapes."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import vit8_ref  # noqa: E402

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
    import vision_transformer as vits
    return vits


if __name__ == "__main__":
    vits = import_reference()
    torch.manual_seed(0)
    model = vits.vit_small(patch_size=8, num_classes=0)
    out = {"param_count": np.array(sum(p.numel() for p in model.parameters()), dtype=np.int64),
           "num_patches": np.array(model.patch_embed.num_patches, dtype=np.int64)}
    sd0 = model.state_dict()
    out["sd_keys"] = np.array(list(sd0.keys()))
    out["sd_shapes"] = np.array([",".join(str(int(d)) for d in v.shape) for v in sd0.values()])
    model.load_state_dict(vit8_ref.state_dict(seed=0), strict=True)
    model.eval()
    for name, F, H, W, seed in vit8_ref.CASES:
        x = vit8_ref.frames(F, H, W, seed)
        n, keep = vit8_ref.ntok(H, W), vit8_ref.rows(H, W)
        out[f"{name}_sha256"] = vit8_ref.digest(x)
        xt = torch.from_numpy(x)
        with torch.no_grad():
            fwd = model(xt)
            inter = torch.stack(model.get_intermediate_layers(xt, vit8_ref.N_LAST))        # [4, F, ntok, 384]
            attn = model.get_last_selfattention(xt)[:, :, 0, :]
            pos = model.interpolate_pos_encoding(torch.zeros(1, n, vit8_ref.DIM), H, W)[0]
        assert inter.shape[2] == n and attn.shape == (F, 6, n) and pos.shape == (n, vit8_ref.DIM)
        assert torch.equal(fwd, inter[-1][:, 0])
        out[f"{name}_fwd"] = fwd.numpy()
        out[f"{name}_cls"] = inter[:, :, 0].numpy()
        out[f"{name}_rows"] = inter[-2:][:, :, keep].numpy()
        out[f"{name}_attn"] = attn.numpy().copy()
        out[f"{name}_pos"] = (pos if n <= 100 else pos[keep]).detach().numpy()
        print(name, tuple(inter.shape), "max|ref|", float(inter.abs().max()), "max attn", float(attn.max()), flush=True)
    path = os.path.join(HERE, "vit8.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes; parameters", int(out["param_count"]))
