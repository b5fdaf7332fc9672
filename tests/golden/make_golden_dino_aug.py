"""Records tests/golden/dino_aug.npz: the crops DataAugmentationDINO produced BEFORE its random draws were split from
its pixel work (sais_amd/dino_data.py at the commit that introduced sais_amd/jpeg.py).  Run from that commit:

    python tests/golden/make_golden_dino_aug.py

tests/test_augment_host.py replays the same seeds through today's code and compares bit for bit, generator state
included.  The images are synthetic (`image()` below); nothing else is read."""
import hashlib
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CASES = [  # name, (H, W), seed, local crops, global size, local size, calls
    ("landscape", (120, 160), 5, 3, 32, 16, 3),
    ("portrait", (97, 61), 11, 2, 24, 12, 2),
    ("elongated", (8, 400), 2, 2, 16, 8, 2),             # every RandomResizedCrop attempt fails: centre-crop fallback
]


def image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0) for c in range(3)], -1)
    return Image.fromarray(np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8))


def state_digest(rng):
    return np.frombuffer(hashlib.sha256(repr(rng.getstate()).encode()).digest(), dtype=np.uint8)


if __name__ == "__main__":
    from sais_amd.dino_data import DataAugmentationDINO
    out = {}
    for name, (h, w), seed, nloc, gs, ls, calls in CASES:
        aug = DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), nloc, seed=seed, global_size=gs, local_size=ls)
        img = image(h, w, seed)
        for k in range(calls):
            for i, c in enumerate(aug(img)):
                out[f"{name}_{k}_{i}"] = c.numpy()
        out[f"{name}_state"] = state_digest(aug.rng)
    np.savez_compressed(os.path.join(HERE, "dino_aug.npz"), **out)
    print(len(out), "arrays")
