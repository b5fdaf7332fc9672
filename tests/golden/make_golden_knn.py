#!/usr/bin/env python3
"""Golden counts of the weighted k-NN classifier, produced by RUNNING THE REFERENCE's own knn_classifier on the CPU
(build container only: needs /root/reference).

    python tests/golden/make_golden_knn.py        # rewrites tests/golden/knn.npz

Reference entry point exercised: SAIS/scripts/dino-main/eval_knn.py:143-182 (knn_classifier), on the inputs of
tests/knn_ref.py:GOLDEN_CASES at k in knn_ref.KS and T = 0.07.  eval_knn.py imports torchvision at the top, which is
stubbed (never touched on this path).  No input array is stored: knn.npz holds the top-1 / top-5 COUNTS per case and k and
a sha256 of the generated arrays, which the tests regenerate and compare."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import knn_ref  # noqa: E402

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
    tv.datasets.ImageFolder = object                 # base class of ReturnIndexDataset
    sys.path.insert(0, os.path.join(REF, "dino-main"))
    import eval_knn
    return eval_knn


if __name__ == "__main__":
    eval_knn = import_reference()
    out = {}
    for name, nt, nq, C, D, noise, seed in knn_ref.GOLDEN_CASES:
        train, train_labels, test, test_labels = knn_ref.make_case(nt, nq, C, D, noise, seed)
        out[f"{name}_sha256"] = knn_ref.digest(train, train_labels, test, test_labels)
        s = knn_ref.similarities(test, train)
        counts = []
        for k in knn_ref.KS:
            top1, top5 = eval_knn.knn_classifier(torch.from_numpy(train), torch.from_numpy(train_labels), torch.from_numpy(test),
                                                 torch.from_numpy(test_labels), k, knn_ref.T, num_classes=C)
            counts.append([round(top1 * nq / 100.0), round(top5 * nq / 100.0)])
            nfrag = int(knn_ref.fragile_rows(s, train_labels, test_labels, k, C).sum())
            print(f"{name} k={k}: top1 {counts[-1][0]} top5 {counts[-1][1]} of {nq}; fragile rows {nfrag} ({100.0 * nfrag / nq:.1f} %)")
            assert nfrag <= knn_ref.FRAGILE_CAP * nq, "change the seed of this case (knn_ref.GOLDEN_CASES), not the cap"
        out[f"{name}_counts"] = np.asarray(counts, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "knn.npz"), **out)
    print(len(out), "arrays")
