"""Host-side data pipeline of DINO pre-training: the frame dataset and the multi-crop augmentation that
SAIS/scripts/dino-main/main_dino.py builds from torchvision.transforms (`SurgDataset` :266-326,
`DataAugmentationDINO` :633-679, utils.GaussianBlur / Solarization utils.py:36-68).

This is CPU data-loader work in front of the GPU step (sais_amd/dino.py) and outside the measured path; torchvision is
not a dependency of this repo, so the transforms are written directly on Pillow with the semantics torchvision documents
for its PIL backend (RandomResizedCrop's area / log-ratio sampling with 10 attempts and a centre-crop fallback,
ColorJitter's random order of brightness / contrast / saturation / hue, ...).  The random draws come from one
`random.Random` per worker, not from torch's global generator: augmentation parity is distributional, not bitwise
(DESIGN.md §7)."""
import math
import os
import random
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

MEAN = np.array((0.485, 0.456, 0.406), dtype=np.float32).reshape(3, 1, 1)
STD = np.array((0.229, 0.224, 0.225), dtype=np.float32).reshape(3, 1, 1)


def to_normalized_tensor(img):
    """ToTensor() + Normalize(ImageNet mean / std) (main_dino.py:643-646)."""
    a = np.asarray(img.convert("RGB"), dtype=np.float32).transpose(2, 0, 1) / 255.0
    return torch.from_numpy((a - MEAN) / STD)


BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3                 # ColorJitter's ops, as numbered in ViewParams.order


@dataclass(frozen=True)
class ViewParams:
    """Every random decision of one view; pixels are not involved (the draws depend on the frame's W x H only)."""
    box: Tuple[int, int, int, int]           # left, top, right, bottom in the (border-cropped) image
    size: int                                # the view is size x size
    flip: bool
    jitter: bool
    order: Tuple[int, int, int, int]         # the jitter ops in the order they are applied
    brightness: float
    contrast: float
    saturation: float
    hue: float                               # the hue channel moves by int(hue * 255) mod 256
    gray: bool
    blur: Optional[float]                    # GaussianBlur radius
    solarize: bool

    @property
    def hue_shift(self):
        return int(self.hue * 255)


def draw_crop_box(rng, W, H, scale, ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """The box of transforms.RandomResizedCrop: area / log-ratio sampling, 10 attempts, centre-crop fallback."""
    area = W * H
    for _ in range(10):
        target = area * rng.uniform(scale[0], scale[1])
        ar = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w, h = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
        if 0 < w <= W and 0 < h <= H:
            top, left = rng.randint(0, H - h), rng.randint(0, W - w)
            return (left, top, left + w, top + h)
    r = W / H                                         # fallback: centre crop at the closest admissible ratio
    if r < ratio[0]:
        w, h = W, int(round(W / ratio[0]))
    elif r > ratio[1]:
        w, h = int(round(H * ratio[1])), H
    else:
        w, h = W, H
    left, top = (W - w) // 2, (H - h) // 2
    return (left, top, left + w, top + h)


def random_resized_crop(img, size, scale, rng, ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """transforms.RandomResizedCrop(size, scale=scale, interpolation=BICUBIC)."""
    W, H = img.size
    return img.crop(draw_crop_box(rng, W, H, scale, ratio)).resize((size, size), Image.BICUBIC)


def draw_color_jitter(rng, brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1):
    """The draws of transforms.ColorJitter: (order, brightness, contrast, saturation, hue)."""
    ops = [BRIGHTNESS, CONTRAST, SATURATION, HUE]
    rng.shuffle(ops)
    fb, fc = rng.uniform(1 - brightness, 1 + brightness), rng.uniform(1 - contrast, 1 + contrast)
    fs, fh = rng.uniform(1 - saturation, 1 + saturation), rng.uniform(-hue, hue)
    return tuple(ops), fb, fc, fs, fh


def apply_color_jitter(img, ops, fb, fc, fs, fh):
    for op in ops:
        if op == BRIGHTNESS:
            img = ImageEnhance.Brightness(img).enhance(fb)
        elif op == CONTRAST:
            img = ImageEnhance.Contrast(img).enhance(fc)
        elif op == SATURATION:
            img = ImageEnhance.Color(img).enhance(fs)
        else:
            h, s, v = img.convert("HSV").split()
            hh = (np.asarray(h, dtype=np.int16) + int(fh * 255)) % 256
            img = Image.merge("HSV", (Image.fromarray(hh.astype(np.uint8), "L"), s, v)).convert("RGB")
    return img


def color_jitter(img, rng, brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1):
    """transforms.ColorJitter: the four adjustments in a random order, factors uniform in [1 - x, 1 + x] ([-hue, hue])."""
    return apply_color_jitter(img, *draw_color_jitter(rng, brightness, contrast, saturation, hue))


def draw_view(rng, W, H, size, scale, blur_p, solarize_p=0.0):
    """Every draw of one view of a W x H image, in the order DataAugmentationDINO has always consumed the generator:
    crop attempts; flip; jitter gate, then shuffle + four factors only if it passed; grayscale gate; blur gate (<=), then
    the radius only if it passed; the solarize gate only when solarize_p is non-zero."""
    box = draw_crop_box(rng, W, H, scale)
    flip = rng.random() < 0.5
    jitter = rng.random() < 0.8
    order, fb, fc, fs, fh = draw_color_jitter(rng) if jitter else ((BRIGHTNESS, CONTRAST, SATURATION, HUE), 1.0, 1.0, 1.0, 0.0)
    gray = rng.random() < 0.2
    blur = rng.uniform(0.1, 2.0) if rng.random() <= blur_p else None            # utils.GaussianBlur: radius ~ U(0.1, 2)
    solarize = bool(solarize_p) and rng.random() < solarize_p                    # utils.Solarization
    return ViewParams(box, size, flip, jitter, order, fb, fc, fs, fh, gray, blur, solarize)


def apply_view_pillow(img, p):
    """The pixel half of a view: what `p` decided, applied to the RGB image with Pillow -> normalised [3,size,size]."""
    img = img.crop(p.box).resize((p.size, p.size), Image.BICUBIC)
    if p.flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if p.jitter:
        img = apply_color_jitter(img, p.order, p.brightness, p.contrast, p.saturation, p.hue)
    if p.gray:
        img = img.convert("L").convert("RGB")
    if p.blur is not None:
        img = img.filter(ImageFilter.GaussianBlur(radius=p.blur))
    if p.solarize:
        img = ImageOps.solarize(img)
    return to_normalized_tensor(img)


class DataAugmentationDINO:
    """main_dino.py:633-679: two global 224 x 224 views (blur p = 1.0 / blur p = 0.1 + solarize p = 0.2) and
    `local_crops_number` local 96 x 96 views (blur p = 0.5), each after flip / colour jitter (p = 0.8) / grayscale (p = 0.2)."""

    def __init__(self, global_crops_scale, local_crops_scale, local_crops_number, seed=None, global_size=224, local_size=96):
        self.gscale, self.lscale, self.local_crops_number = tuple(global_crops_scale), tuple(local_crops_scale), local_crops_number
        self.gsize, self.lsize = global_size, local_size
        self.seed = seed
        self._rng, self._rng_key = None, None

    @property
    def rng(self):
        """One random.Random per (process, DataLoader worker, epoch).  DataLoader workers are forked with a COPY of this
        object, re-forked every epoch from the parent's never-advancing state: a single generator made every worker draw
        the same crop / flip / jitter sequence and replay it every epoch.  torch gives each worker a seed
        `base_seed + worker_id` with a fresh base_seed per epoch (what torchvision's transforms draw from in the
        reference); the generator here is re-created from (seed, that worker seed) whenever it changes."""
        info = torch.utils.data.get_worker_info()
        key = (os.getpid(), None if info is None else (info.id, info.seed))
        if self._rng is None or key != self._rng_key:
            if info is None:
                self._rng = random.Random(self.seed)
            else:
                self._rng = random.Random(hash((self.seed, info.id, info.seed)) & 0xFFFFFFFFFFFF)
            self._rng_key = key
        return self._rng

    def _view_specs(self):
        return [(self.gsize, self.gscale, 1.0, 0.0), (self.gsize, self.gscale, 0.1, 0.2)] + \
            [(self.lsize, self.lscale, 0.5, 0.0)] * self.local_crops_number

    def draw(self, W, H):
        """The ViewParams of the 2 global + local_crops_number local views of one W x H image; no pixel is touched."""
        r = self.rng
        return [draw_view(r, W, H, *spec) for spec in self._view_specs()]

    def _view(self, image, size, scale, blur_p, solarize_p=0.0):
        return apply_view_pillow(image, draw_view(self.rng, image.size[0], image.size[1], size, scale, blur_p, solarize_p))

    def __call__(self, image):
        image = image.convert("RGB")
        return [self._view(image, *spec) for spec in self._view_specs()]


def border_box(W, H, fracs):
    """transforms.CenterCrop((hf * H, wf * W)) of SurgDataset as (left, top, width, height)."""
    hf, wf = fracs
    ch, cw = int(hf * H), int(wf * W)
    return int(round((W - cw) / 2.0)), int(round((H - ch) / 2.0)), cw, ch


class SurgDataset(torch.utils.data.Dataset):
    """Frames listed in `<data_path>/paths/<dataset>_Paths.csv` (columns `path`, `label`; Windows separators allowed),
    border-cropped to the central 0.8 x 0.8 (0.8 x 0.7 for the *_Gronau sets) before the transform — main_dino.py:266-326
    with its NS / VUA branch (every row is a training row; DINO needs no labels).  Returns (crops, label, dataset).

    With `gpu_augment` the workers only read the file and draw: an item is (file bytes, the header sais_jpeg_parse made
    of them as bytes or None, the ViewParams of its views, label, dataset), and `gpu_crops` turns a batch of those into
    the same crop list on the device."""

    def __init__(self, data_path, dataset_list, transform, frames_root="./SAIS", gpu_augment=False):
        import pandas as pd
        rows = []
        for name in dataset_list:
            df = pd.read_csv(os.path.join(data_path, "paths", "%s_Paths.csv" % name), index_col=0)
            for p, lab in zip(df["path"].tolist(), df["label"].tolist() if "label" in df else [0] * len(df)):
                rows.append((str(p).replace("\\", "/"), lab, name))
        self.rows, self.transform, self.frames_root = rows, transform, frames_root
        self.dataset = dataset_list[0]
        self.gpu_augment = gpu_augment

    def crop_fracs(self):
        return (0.8, 0.7) if self.dataset in ("NS_Gronau", "VUA_Gronau") else (0.8, 0.8)

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, idx):
        path, label, name = self.rows[idx]
        if self.gpu_augment:
            return self._raw_item(os.path.join(self.frames_root, path), label, name)
        with open(os.path.join(self.frames_root, path), "rb") as f:
            img = Image.open(f)
            img.load()
        W, H = img.size
        left, top, cw, ch = border_box(W, H, self.crop_fracs())      # transforms.CenterCrop((0.8 H, 0.8 W))
        img = img.crop((left, top, left + cw, top + ch))
        return self.transform(img), label, name

    def _raw_item(self, path, label, name):
        import io
        from . import jpeg
        with open(path, "rb") as f:
            blob = f.read()
        hdr = jpeg.parse_header(blob)
        if hdr is not None:
            W, H = hdr.width, hdr.height
        else:
            with Image.open(io.BytesIO(blob)) as img:                # reads the header only
                W, H = img.size
        _, _, cw, ch = border_box(W, H, self.crop_fracs())
        return blob, None if hdr is None else bytes(hdr), self.transform.draw(cw, ch), label, name


def collate_raw(batch):
    """collate_fn of the gpu_augment mode: (items, labels, datasets); the items go to gpu_crops as they are."""
    return batch, [b[3] for b in batch], [b[4] for b in batch]


def gpu_crops(items, decoder, augmenter, fracs):
    """A batch of gpu_augment items -> the crop list collate() makes of the Pillow path, on the device: one tensor
    [B,3,s,s] per view.  JpegDecoder takes one geometry per call and a dataset list mixes sources, so the files are
    grouped by geometry, decoded, augmented and scattered back into batch order.  A file the GPU decoder does not take
    is decoded by Pillow, converted to RGB as DataAugmentationDINO.__call__ does, and uploaded."""
    import io
    from . import jpeg
    dev = augmenter.device
    headers, host, groups = [], {}, {}
    for i, (blob, hdr, _, _, _) in enumerate(items):
        h = None if hdr is None else jpeg.SaisJpegHeader.from_buffer_copy(hdr)
        if h is None:
            with Image.open(io.BytesIO(blob)) as img:
                host[i] = np.array(img.convert("RGB"))
        headers.append(h)
        groups.setdefault((h.height, h.width) if h is not None else host[i].shape[:2], []).append(i)
    crops = None
    for (H, W), idx in groups.items():
        on_gpu = [i for i in idx if headers[i] is not None]
        if len(on_gpu) == len(idx):
            frames = decoder.decode([items[i][0] for i in idx], [headers[i] for i in idx])
        else:
            frames = torch.empty(len(idx), H, W, 3, dtype=torch.uint8, device=dev)
            if on_gpu:
                dec = decoder.decode([items[i][0] for i in on_gpu], [headers[i] for i in on_gpu])
                frames[torch.as_tensor([idx.index(i) for i in on_gpu], device=dev)] = dec
            for k, i in enumerate(idx):
                if i in host:
                    frames[k].copy_(torch.from_numpy(host[i]))
        views = augmenter(frames, [items[i][2] for i in idx], border_box(W, H, fracs))
        if len(groups) == 1:
            return views
        if crops is None:
            crops = [torch.empty(len(items), *v.shape[1:], dtype=v.dtype, device=dev) for v in views]
        where = torch.as_tensor(idx, device=dev)
        for c, v in zip(crops, views):
            c[where] = v
    return crops
