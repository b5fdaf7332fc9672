"""Linear probe on frozen features (dino-main/eval_linear.py) on the HIP kernels of csrc/probe.hip.

`LinearClassifier` is the reference's module (eval_linear.py:237-251).  `LinearProbe` trains up to 8 such heads that differ
only in learning rate from ONE backbone pass per step — the backbone pass dominates a step and has to be repeated every step
because the train transform is random — in three launches for any number of heads (logits, cross entropy, gradient + momentum
SGD; the weight gradient is never written to memory).  The heads run in the exact f32 MFMA arithmetic, without atomics: a run
is bit-reproducible.  There is no CPU fallback: host tensors raise.  The dataset / sampler / checkpoint helpers of the CLI
(SAIS/scripts/dino-main/eval_linear.py) live here too.
"""
import math
import random

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .dino_data import draw_crop_box
from .knn import EvalImageFolder, list_image_folder

MAX_HEADS, MAX_ROWS, MAX_CLASSES, MAX_DIM = 8, 1024, 4096, 1920


def _features(x, dim, name="features"):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise L.SaisHipError(f"{name}: expected a device tensor (the linear probe has no CPU fallback)")
    x = x.reshape(x.shape[0], -1)                                                  # eval_linear.py:248
    if x.shape[1] != dim:
        raise ValueError(f"{name}: expected [B, {dim}], got {tuple(x.shape)}")
    if not 1 <= x.shape[0] <= MAX_ROWS:
        raise ValueError(f"{name}: B = {x.shape[0]} must be in [1, {MAX_ROWS}]")
    return x.float().contiguous()


def _check_dims(dim, num_labels):
    if dim < 64 or dim % 64 or dim > MAX_DIM:
        raise ValueError(f"dim = {dim} must be a multiple of 64 and at most {MAX_DIM}")
    if not 1 <= num_labels <= MAX_CLASSES:
        raise ValueError(f"num_labels = {num_labels} must be in [1, {MAX_CLASSES}]")


def _logits(x, W, b, H, C, dim):
    Z = torch.empty(H, x.shape[0], C, dtype=torch.float32, device=x.device)
    L.call("sais_probe_logits", ops._p(x), ops._p(W), ops._p(b), H, x.shape[0], C, dim, ops._p(Z), ops._stream())
    return Z


class LinearClassifier(nn.Module):
    """Linear layer to train on top of frozen features (eval_linear.py:237-251): `linear.weight` [num_labels, dim] ~
    N(0, 0.01), `linear.bias` zero.  forward() computes the logits with sais_probe_logits under no_grad; training goes
    through LinearProbe, which owns the gradient and the optimiser step."""

    def __init__(self, dim, num_labels=1000):
        super().__init__()
        _check_dims(dim, num_labels)
        self.num_labels = num_labels
        self.linear = nn.Linear(dim, num_labels)
        self.linear.weight.data.normal_(mean=0.0, std=0.01)
        self.linear.bias.data.zero_()

    def forward(self, x):
        w, b = self.linear.weight, self.linear.bias
        if torch.is_grad_enabled() and (w.requires_grad or b.requires_grad or (isinstance(x, torch.Tensor) and x.requires_grad)):
            raise L.SaisHipError("LinearClassifier.forward is inference only (call it under torch.no_grad()): the heads are "
                                 "trained by sais_amd.linear.LinearProbe, whose kernels apply the gradient themselves")
        if not w.is_cuda:
            raise L.SaisHipError("LinearClassifier: move the module to the GPU (the linear probe has no CPU fallback)")
        x = _features(x, w.shape[1], "x")
        with torch.no_grad():
            return _logits(x, w.detach().float().contiguous(), b.detach().float().contiguous(), 1, self.num_labels, w.shape[1])[0]


def cosine_lr(base_lr, epochs, last_epoch, eta_min=0.0):
    """The learning rate torch.optim.lr_scheduler.CosineAnnealingLR(T_max=epochs, eta_min) holds after `last_epoch` calls of
    step(), by its own recursion (not the closed form: the two differ in the last bits)."""
    lr = base_lr
    for e in range(1, last_epoch + 1):
        if (e - 1 - epochs) % (2 * epochs) == 0:
            lr = lr + (base_lr - eta_min) * (1 - math.cos(math.pi / epochs)) / 2
        else:
            lr = (1 + math.cos(math.pi * e / epochs)) / (1 + math.cos(math.pi * (e - 1) / epochs)) * (lr - eta_min) + eta_min
    return lr


class LinearProbe:
    """H = len(lrs) heads [num_labels, dim] and their momentum buffers, stacked; the optimiser is torch.optim.SGD(lr,
    momentum, weight_decay=0) and the schedule CosineAnnealingLR(T_max=epochs, eta_min=0) of eval_linear.py:103-109, one
    pair per head.  `lrs` are the initial rates actually applied (after the linear scaling rule)."""

    def __init__(self, dim, num_labels, lrs, epochs, momentum=0.9, device="cuda:0", seed=None):
        _check_dims(dim, num_labels)
        lrs = [float(v) for v in lrs]
        if not 1 <= len(lrs) <= MAX_HEADS:
            raise ValueError(f"{len(lrs)} learning rates: 1 to {MAX_HEADS} heads")
        if any(not (v > 0 and math.isfinite(v)) for v in lrs) or not 0 <= momentum < 1 or epochs < 1:
            raise ValueError("lrs must be positive, momentum in [0, 1), epochs >= 1")
        device = torch.device(device)
        if device.type != "cuda":
            raise L.SaisHipError("LinearProbe: the linear probe has no CPU fallback")
        self.dim, self.num_labels, self.base_lrs, self.epochs, self.momentum = dim, num_labels, lrs, int(epochs), float(momentum)
        self.H, self.device = len(lrs), device
        self.last_epoch = 0
        self.lrs = list(lrs)
        gen = None if seed is None else torch.Generator().manual_seed(seed)
        # every head starts from the same draw (the heads differ only in learning rate), made as LinearClassifier does
        w0 = torch.empty(num_labels, dim).normal_(mean=0.0, std=0.01, generator=gen)
        self.W = w0.unsqueeze(0).repeat(self.H, 1, 1).to(device).contiguous()
        self.b = torch.zeros(self.H, num_labels, device=device)
        self.mW, self.mb = torch.zeros_like(self.W), torch.zeros_like(self.b)

    # ------------------------------------------------------------------ kernels
    def _targets(self, targets, B, check):
        if not isinstance(targets, torch.Tensor) or not targets.is_cuda:
            raise L.SaisHipError("targets: expected a device tensor")
        if targets.dim() != 1 or targets.shape[0] != B or targets.dtype not in (torch.int64, torch.int32):
            raise ValueError("targets: expected one int64 / int32 label per feature row")
        if check:
            lo, hi = int(targets.min()), int(targets.max())
            if lo < 0 or hi >= self.num_labels:
                raise ValueError(f"target {lo if lo < 0 else hi} outside [0, {self.num_labels})")
        return targets.to(torch.int32).contiguous()

    def _ce(self, x, t, train):
        H, B, C = self.H, x.shape[0], self.num_labels
        Z = _logits(x, self.W, self.b, H, C, self.dim)
        rows = torch.empty(H, B, dtype=torch.float32, device=x.device)
        loss = torch.empty(H, dtype=torch.float32, device=x.device)
        top5 = None if train else torch.empty(H, B, 5, dtype=torch.int32, device=x.device)
        L.call("sais_probe_ce", ops._p(Z), ops._p(t), H, B, C, 1 if train else 0, ops._p(rows), ops._p(top5),
               None if train else ops._p(loss), ops._stream())
        return Z, rows, loss, top5

    def _update(self, x, dZ, rows, loss):
        u = L.SaisProbeUpdate(ops._p(x), ops._p(dZ), ops._p(self.W), ops._p(self.b), ops._p(self.mW), ops._p(self.mb),
                              ops._p(rows), ops._p(loss), self.H, x.shape[0], self.num_labels, self.dim, self.momentum,
                              (L.c_float * 8)(*(self.lrs + [0.0] * (8 - self.H))))
        L.call("sais_probe_update", u, ops._stream())

    def step(self, features, targets, check_targets=True):
        """One optimiser step of every head on the batch (eval_linear.py:163-183) -> the heads' mean losses f32 [H] on the
        device.  Three launches.  check_targets = False skips the range check of the labels, the only host synchronisation
        (a caller that has the labels on the host checks them there)."""
        x = _features(features, self.dim)
        t = self._targets(targets, x.shape[0], check_targets)
        dZ, rows, loss, _ = self._ce(x, t, True)
        self._update(x, dZ, rows, loss)
        return loss

    @torch.no_grad()
    def evaluate(self, features, targets):
        """(loss_sum, top1, top5) per head over the rows of this batch: the summed cross entropy (float), the number of rows
        whose target is the best class and the number whose target is among the five best (utils.accuracy; with fewer
        than five classes all of them)."""
        x = _features(features, self.dim)
        t = self._targets(targets, x.shape[0], True)
        _, _, loss, top5 = self._ce(x, t, False)
        hit = top5.eq(t.view(1, -1, 1))
        top1 = hit[:, :, 0].sum(1).tolist()
        return [v * x.shape[0] for v in loss.double().tolist()], top1, hit.any(2).sum(1).tolist()

    def logits(self, features):
        """Z f32 [H, B, num_labels]."""
        return _logits(_features(features, self.dim), self.W, self.b, self.H, self.num_labels, self.dim)

    # ------------------------------------------------------------------ schedule, heads, checkpoints
    def scheduler_step(self):
        """CosineAnnealingLR.step() of every head (eval_linear.py:127)."""
        self.last_epoch += 1
        self.lrs = [cosine_lr(v, self.epochs, self.last_epoch) for v in self.base_lrs]

    def head(self, i):
        """Head i as a LinearClassifier (a copy of its weights)."""
        m = LinearClassifier(self.dim, self.num_labels)
        m.linear.weight.data = self.W[i].clone()
        m.linear.bias.data = self.b[i].clone()
        return m

    def state(self, i, epoch=None, best_acc=0.0):
        """Head i as the reference's checkpoint dict (eval_linear.py:141-148): `state_dict` carries the DistributedDataParallel
        prefix, `optimizer` / `scheduler` load into torch.optim.SGD / CosineAnnealingLR.  Tensors are on the host."""
        cpu = lambda t: t.detach().cpu().clone()
        group = dict(lr=self.lrs[i], momentum=self.momentum, dampening=0, weight_decay=0, nesterov=False, maximize=False,
                     foreach=None, differentiable=False, fused=None, initial_lr=self.base_lrs[i], params=[0, 1])
        return {"epoch": self.last_epoch if epoch is None else int(epoch),
                "state_dict": {"module.linear.weight": cpu(self.W[i]), "module.linear.bias": cpu(self.b[i])},
                "optimizer": {"state": {0: {"momentum_buffer": cpu(self.mW[i])}, 1: {"momentum_buffer": cpu(self.mb[i])}},
                              "param_groups": [group]},
                "scheduler": {"T_max": self.epochs, "eta_min": 0, "base_lrs": [self.base_lrs[i]], "last_epoch": self.last_epoch,
                              "_step_count": self.last_epoch + 1, "_get_lr_called_within_step": False,
                              "_last_lr": [self.lrs[i]]},
                "best_acc": best_acc}

    def load_weights(self, i, state_dict):
        """Weight and bias of head i from a LinearClassifier state_dict, with or without the `module.` prefix."""
        sd = {k.replace("module.", ""): v for k, v in state_dict.items()}
        w, b = sd["linear.weight"], sd["linear.bias"]
        if tuple(w.shape) != (self.num_labels, self.dim) or tuple(b.shape) != (self.num_labels,):
            raise ValueError(f"checkpoint head is {tuple(w.shape)}, expected {(self.num_labels, self.dim)}")
        self.W[i].copy_(w)
        self.b[i].copy_(b)

    def load_state(self, i, ckpt):
        """Restore head i from state(i) or from a checkpoint the reference wrote.  The schedule position is shared by the
        heads: every head of a run is loaded from the same epoch."""
        self.load_weights(i, ckpt["state_dict"])
        st = ckpt["optimizer"]["state"]
        for buf, k in ((self.mW, 0), (self.mb, 1)):
            m = st.get(k, {}).get("momentum_buffer")
            if m is None:                    # torch before its first step: no buffer yet; zeros give its first step
                buf[i].zero_()
            else:
                buf[i].copy_(m)
        sch = ckpt["scheduler"]
        if int(sch["T_max"]) != self.epochs:
            raise ValueError(f"checkpoint schedule has T_max = {sch['T_max']}, this run {self.epochs}")
        self.base_lrs[i] = float(sch["base_lrs"][0])
        self.last_epoch = int(sch["last_epoch"])
        self.lrs = [cosine_lr(v, self.epochs, self.last_epoch) for v in self.base_lrs]
        self.lrs[i] = float(ckpt["optimizer"]["param_groups"][0]["lr"])
        return {"epoch": ckpt.get("epoch", self.last_epoch), "best_acc": ckpt.get("best_acc", 0.0)}


# ---------------------------------------------------------------------------------------------- CLI helpers (host side)
def epoch_order(n, epoch, seed=0):
    """torch.utils.data.distributed.DistributedSampler(shuffle=True) at world size 1: randperm with generator seed
    `seed + epoch` (eval_linear.py:92, :124)."""
    g = torch.Generator()
    g.manual_seed(seed + epoch)
    return torch.randperm(n, generator=g).tolist()


class EpochSampler(torch.utils.data.Sampler):
    def __init__(self, n, seed=0):
        self.n, self.seed, self.epoch = n, seed, 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(epoch_order(self.n, self.epoch, self.seed))


class TrainImageFolder(torch.utils.data.Dataset):
    """ImageFolder with the train transform of eval_linear.py:85-90 restated on Pillow: RandomResizedCrop(224) (scale
    (0.08, 1), ratio (3/4, 4/3), bilinear), RandomHorizontalFlip, ToTensor, Normalize(ImageNet).  The draws of a sample
    come from a generator seeded by (seed, epoch, sample index): they do not depend on the worker count or on the order
    the samples are fetched in.  (The draws are not torchvision's stream: this transform is not parity-pinned.)"""
    MEAN, STD = EvalImageFolder.MEAN, EvalImageFolder.STD
    SCALE, RATIO = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)

    def __init__(self, root, seed=0):
        self.classes, self.samples = list_image_folder(root)
        self.seed, self.epoch = int(seed), 0

    def set_epoch(self, epoch):
        """Call before the DataLoader of an epoch is iterated (its workers copy the dataset then)."""
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.samples)

    def draw(self, i, W, H):
        """((left, top, right, bottom), flip) of sample i in the current epoch."""
        rng = random.Random((self.seed * 1000003 + self.epoch) * 2147483629 + i)
        box = draw_crop_box(rng, W, H, self.SCALE, self.RATIO)
        return box, rng.random() < 0.5

    @classmethod
    def apply(cls, img, box, flip):
        from PIL import Image
        img = img.convert("RGB").crop(box).resize((224, 224), Image.BILINEAR)
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        a = np.asarray(img, dtype=np.float32) / 255.0
        a = (a - np.asarray(cls.MEAN, np.float32)) / np.asarray(cls.STD, np.float32)
        return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))

    def __getitem__(self, i):
        from PIL import Image
        path, label = self.samples[i]
        with open(path, "rb") as fh:
            img = Image.open(fh)
            box, flip = self.draw(i, *img.size)
            return self.apply(img, box, flip), label


class LabelledEvalFolder(EvalImageFolder):
    """knn.EvalImageFolder yielding (image, label) as the reference's validation ImageFolder does (eval_linear.py:65-71)."""

    def __getitem__(self, i):
        return super().__getitem__(i)[0], self.samples[i][1]
