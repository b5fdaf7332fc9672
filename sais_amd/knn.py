"""Weighted k-NN evaluation of frozen features (dino-main/eval_knn.py) on the HIP kernels of csrc/knn.hip.

`knn_classifier` has the reference's signature and meaning (eval_knn.py:143-182) but never forms the [Nq, Nt] similarity
matrix and serves every k of `--nb_knn` from one search: sais_knn_search keeps the kmax best train rows per test row,
sais_knn_vote turns the neighbour list into the five best classes for each k.  There is no CPU fallback: host tensors
raise.  The dataset / transform / checkpoint helpers of the CLI (SAIS/scripts/dino-main/eval_knn.py) live here too.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib as L
from . import ops
from .model_io import backbone_state_dict  # noqa: F401  (its home; the name stays importable from here)

MAX_K, MAX_DIM, MAX_CLASSES, MAX_KS = 256, 1536, 4096, 8
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")     # torchvision's ImageFolder


def _features(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a device tensor (the k-NN path has no CPU fallback)")
    if t.dim() != 2 or t.shape[0] < 1:
        raise ValueError(f"{name}: expected [N, D], got {tuple(t.shape)}")
    if t.shape[1] % 64 or t.shape[1] > MAX_DIM:
        raise ValueError(f"{name}: D = {t.shape[1]} must be a multiple of 64 and at most {MAX_DIM}")
    return t.float().contiguous()


class KnnIndex:
    """The train side of the classifier: features [Nt, D] (L2-normalised rows) split once into their bf16x3 image, labels
    [Nt] (int64 or int32) in [0, num_classes).  train_labels = None: an index for `search` alone (sais_amd.retrieval)."""

    def __init__(self, train_features, train_labels=None, num_classes=1000):
        f = _features(train_features, "train_features")
        if train_labels is not None:
            if not isinstance(train_labels, torch.Tensor) or not train_labels.is_cuda:
                raise ValueError("train_labels: expected a device tensor")
            if train_labels.dim() != 1 or train_labels.shape[0] != f.shape[0] or train_labels.dtype not in (torch.int64, torch.int32):
                raise ValueError("train_labels: expected one int64 / int32 label per train row")
            if not 1 <= num_classes <= MAX_CLASSES:
                raise ValueError(f"num_classes must be in [1, {MAX_CLASSES}]")
            lo, hi = int(train_labels.min()), int(train_labels.max())
            if lo < 0 or hi >= num_classes:
                raise ValueError(f"train label {lo if lo < 0 else hi} outside [0, {num_classes})")
        self.nt, self.dim, self.num_classes = f.shape[0], f.shape[1], num_classes
        self.labels = None if train_labels is None else train_labels.to(torch.int32).contiguous()
        self.train3 = torch.empty(self.nt, 3 * self.dim, dtype=torch.bfloat16, device=f.device)
        ops.split_bf16x3(f, self.train3, True)
        self._ws = None

    def _workspace(self, nq, kmax):
        need = L.load().sais_knn_workspace_bytes(nq, self.nt, kmax)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.train3.device)
        return self._ws

    def search(self, test_features, kmax):
        """(values f32 [Nq, kmax], indices i32 [Nq, kmax]): the kmax largest dot products per test row, sorted by (value
        descending, train index ascending)."""
        q = _features(test_features, "test_features")
        if q.shape[1] != self.dim or q.device != self.train3.device:
            raise ValueError(f"test_features: expected [Nq, {self.dim}] on {self.train3.device}")
        kmax = int(kmax)
        if not 1 <= kmax <= MAX_K:
            raise ValueError(f"k = {kmax} must be in [1, {MAX_K}]")
        if kmax > self.nt:
            raise ValueError(f"k = {kmax} exceeds the {self.nt} train rows")
        nq = q.shape[0]
        val = torch.empty(nq, kmax, dtype=torch.float32, device=q.device)
        idx = torch.empty(nq, kmax, dtype=torch.int32, device=q.device)
        ws = self._workspace(nq, kmax)
        L.call("sais_knn_search", ops._p(q), ops._p(self.train3), 1, nq, self.nt, self.dim, kmax, ops._p(val), ops._p(idx),
               ops._p(ws), ws.numel(), ops._stream())
        return val, idx

    def vote(self, values, indices, ks, T, return_votes=False):
        """pred i32 [m, Nq, 5] (and votes f32 [m, Nq, num_classes]) for the ascending list `ks` from one neighbour list."""
        ks = [int(k) for k in ks]
        if self.labels is None:
            raise ValueError("this index was built without train_labels: it serves `search` only")
        if not 1 <= len(ks) <= MAX_KS or any(b <= a for a, b in zip(ks, ks[1:])) or ks[0] < 1 or ks[-1] > values.shape[1]:
            raise ValueError(f"ks = {ks}: 1 to {MAX_KS} strictly ascending values, the largest at most {values.shape[1]}")
        if not T > 0:
            raise ValueError("T must be positive")
        nq, kmax = values.shape
        pred = torch.empty(len(ks), nq, 5, dtype=torch.int32, device=values.device)
        votes = torch.empty(len(ks), nq, self.num_classes, dtype=torch.float32, device=values.device) if return_votes else None
        L.call("sais_knn_vote", ops._p(values), ops._p(indices), nq, kmax, ops._p(self.labels), self.nt, self.num_classes,
               float(T), (ctypes.c_int * len(ks))(*ks), len(ks), ops._p(pred), ops._p(votes), ops._stream())
        return (pred, votes) if return_votes else pred

    def classify(self, test_features, ks, T, return_votes=False):
        ks = [int(k) for k in ks]
        val, idx = self.search(test_features, max(ks))
        return self.vote(val, idx, ks, T, return_votes)


@torch.no_grad()
def knn_classifier(train_features, train_labels, test_features, test_labels, k, T, num_classes=1000):
    """eval_knn.py:143-182: (top1, top5) in per cent; top5 counts the first min(5, k) predictions.  `k` may be a list: one
    search then serves every k and a list of pairs comes back.  Any Nq >= 1."""
    many = isinstance(k, (list, tuple))
    ks = sorted(set(int(v) for v in (k if many else [k])))
    index = train_features if isinstance(train_features, KnnIndex) else KnnIndex(train_features, train_labels, num_classes)
    if not isinstance(test_labels, torch.Tensor) or not test_labels.is_cuda:
        raise ValueError("test_labels: expected a device tensor")
    results = {}
    for i in range(0, len(ks), MAX_KS):
        pred = index.classify(test_features, ks[i:i + MAX_KS], T)
        correct = pred.long().eq(test_labels.view(1, -1, 1).long())
        total = test_labels.shape[0]
        for j, kj in enumerate(ks[i:i + MAX_KS]):
            top1 = correct[j, :, :1].sum().item() * 100.0 / total
            top5 = correct[j, :, :min(5, kj)].sum().item() * 100.0 / total
            results[kj] = (top1, top5)
    return [results[int(v)] for v in k] if many else results[int(k)]


# ---------------------------------------------------------------------------------------------- CLI helpers (host side)
def list_image_folder(root):
    """torchvision's ImageFolder listing: (sorted class names, [(path, class position)]) with the files of each class in
    sorted walk order."""
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"no class folders under {root}")
    samples = []
    for ci, c in enumerate(classes):
        for d, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
            samples += [(os.path.join(d, f), ci) for f in sorted(files) if f.lower().endswith(IMG_EXTENSIONS)]
    return classes, samples


def eval_transform_geometry(w, h, resize=256, crop=224):
    """Resize(256) + CenterCrop(224) of torchvision on a w x h image: ((new_w, new_h), (left, top))."""
    if w <= h:
        nw, nh = resize, int(resize * h / w)
    else:
        nw, nh = int(resize * w / h), resize
    return (nw, nh), (int(round((nw - crop) / 2.0)), int(round((nh - crop) / 2.0)))


class EvalImageFolder(torch.utils.data.Dataset):
    """ReturnIndexDataset (eval_knn.py:185-188) with the eval transform restated on Pillow: Resize(256, bicubic),
    CenterCrop(224), ToTensor, Normalize(ImageNet)."""
    MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

    def __init__(self, root):
        self.classes, self.samples = list_image_folder(root)

    def __len__(self):
        return len(self.samples)

    @classmethod
    def transform(cls, img):
        from PIL import Image
        img = img.convert("RGB")
        (nw, nh), (left, top) = eval_transform_geometry(*img.size)
        if (nw, nh) != img.size:
            img = img.resize((nw, nh), Image.BICUBIC)
        img = img.crop((left, top, left + 224, top + 224))           # outside the image (sides < 224): zero fill, as CenterCrop pads
        a = np.asarray(img, dtype=np.float32) / 255.0
        a = (a - np.asarray(cls.MEAN, np.float32)) / np.asarray(cls.STD, np.float32)
        return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))

    def __getitem__(self, i):
        from PIL import Image
        with open(self.samples[i][0], "rb") as fh:
            return self.transform(Image.open(fh)), i


@torch.no_grad()
def extract_features(model, loader, device="cuda:0"):
    """Features [N, D] on the device in dataset order; `loader` yields (images, dataset indices)."""
    feats = None
    for samples, index in loader:
        out = model(samples.to(device, non_blocking=True)).float()
        if feats is None:
            feats = torch.zeros(len(loader.dataset), out.shape[-1], dtype=torch.float32, device=device)
        feats.index_copy_(0, index.to(device), out)
    return feats
