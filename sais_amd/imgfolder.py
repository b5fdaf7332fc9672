"""Image-folder batches on the MI355X: files of mixed sizes -> the normalised [B,3,h,w] tensor the Pillow datasets yield.

The evaluation tools read image folders (ImageNet, Copydays): dozens of geometries per batch.  Their Pillow datasets
(knn.EvalImageFolder, linear.TrainImageFolder, retrieval.ImgListDataset) decode and resample in DataLoader workers.  Here
the workers only read the file and parse its header (the pattern of dino_data.SurgDataset._raw_item), and GpuImageLoader
turns a batch of such items into the same tensor, bit for bit, with one pinned pack and one H2D copy, one
sais_jpeg_decode_mixed (csrc/jpeg.hip), one status read and one sais_image_transform (csrc/imgfolder.hip).

Three kinds of file are decoded by Pillow with .convert("RGB"), as the datasets do: files the parser refuses (progressive,
grayscale, CMYK, non-JPEG), files the GPU flags, and images the LDS fit predicate refuses.  The first two have their pixels
uploaded into the packed buffer, so their transform still runs on the device; the third goes through the Pillow transform
itself.  `stats` counts each path.  The Pillow path as a whole is chosen by the caller (the tools without --gpu_loader),
never from here."""
import ctypes
import io

import numpy as np
import torch

from . import _lib as L
from . import jpeg
from .augment import normalize_table  # noqa: F401  (the [3][256] table of `(a / 255 - MEAN) / STD`, re-exported)
from .knn import EvalImageFolder, eval_transform_geometry, list_image_folder
from .linear import TrainImageFolder

BILINEAR, BICUBIC = 0, 1                                           # SAIS_IMG_BILINEAR, SAIS_IMG_BICUBIC
XFORM_DTYPE = np.dtype([("src_offset", "<i8"), ("src_h", "<i4"), ("src_w", "<i4"), ("box", "<i4", 4), ("rw", "<i4"),
                        ("rh", "<i4"), ("win_left", "<i4"), ("win_top", "<i4"), ("filter", "<i4"), ("flip", "<i4"),
                        ("out_offset", "<i8")], align=True)
assert XFORM_DTYPE.itemsize == ctypes.sizeof(L.SaisImgXform)


# ------------------------------------------------------------------------------------------------ worker-side datasets
def _read(path):
    """(file bytes, header bytes of sais_jpeg_parse or None)."""
    with open(path, "rb") as fh:
        blob = fh.read()
    hdr = jpeg.parse_header(blob)
    return blob, None if hdr is None else bytes(hdr)


def _size(blob, hdr):
    """(W, H) from the parsed header, else from Pillow (reads the header only)."""
    if hdr is not None:
        h = jpeg.SaisJpegHeader.from_buffer_copy(hdr)
        return h.width, h.height
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as img:
        return img.size


class RawEvalFolder(torch.utils.data.Dataset):
    """knn.EvalImageFolder without the pixels: item = (bytes, header bytes or None, dataset index)."""

    def __init__(self, root):
        self.classes, self.samples = list_image_folder(root)

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return _read(self.samples[i][0]) + (i,)


class RawLabelledEvalFolder(RawEvalFolder):
    """linear.LabelledEvalFolder without the pixels: item = (bytes, header bytes or None, label)."""

    def __getitem__(self, i):
        return _read(self.samples[i][0]) + (self.samples[i][1],)


class RawTrainFolder(TrainImageFolder):
    """linear.TrainImageFolder without the pixels: item = (bytes, header bytes or None, label, box, flip) with the box and
    the flip of TrainImageFolder.draw (same seed, epoch and sample index: the same draws)."""

    def __getitem__(self, i):
        path, label = self.samples[i]
        blob, hdr = _read(path)
        box, flip = self.draw(i, *_size(blob, hdr))
        return blob, hdr, label, box, flip


class RawImgList(torch.utils.data.Dataset):
    """retrieval.ImgListDataset without the pixels: item = (bytes, header bytes or None, dataset index)."""

    def __init__(self, img_list):
        self.samples = list(img_list)

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return _read(self.samples[i]) + (i,)


def collate_raw(batch):
    """collate_fn of the raw datasets: (items as they are, LongTensor of their index or label)."""
    return batch, torch.tensor([b[2] for b in batch], dtype=torch.long)


# ------------------------------------------------------------------------------------------------ descriptor builders
# builder(item, w, h) -> (box, (rw, rh), (win_left, win_top), filter, flip); `out_hw` is the builder's output size
class _Builder:
    def __init__(self, fn, out_hw, pillow):
        self.fn, self.out_hw, self.pillow = fn, out_hw, pillow

    def __call__(self, item, w, h):
        return self.fn(item, w, h)


def eval_builder():
    """knn.EvalImageFolder.transform: Resize(256, bicubic), CenterCrop(224)."""
    def fn(item, w, h):
        (nw, nh), (left, top) = eval_transform_geometry(w, h)
        return (0, 0, w, h), (nw, nh), (left, top), BICUBIC, False
    return _Builder(fn, (224, 224), lambda item, img: EvalImageFolder.transform(img))


def train_builder():
    """linear.TrainImageFolder.apply: the item's box, bilinear to 224 x 224, the item's flip."""
    def fn(item, w, h):
        return tuple(item[3]), (224, 224), (0, 0), BILINEAR, bool(item[4])
    return _Builder(fn, (224, 224), lambda item, img: TrainImageFolder.apply(img, tuple(item[3]), bool(item[4])))


def square_builder(imsize):
    """retrieval.ImgListDataset(imsize): the whole image to imsize x imsize, bicubic."""
    imsize = int(imsize)

    def fn(item, w, h):
        return (0, 0, w, h), (imsize, imsize), (0, 0), BICUBIC, False

    def pillow(item, img):
        from PIL import Image
        from .retrieval import _to_tensor
        img = img.convert("RGB")
        if img.size != (imsize, imsize):
            img = img.resize((imsize, imsize), Image.BICUBIC)
        return _to_tensor(img)
    return _Builder(fn, (imsize, imsize), pillow)


# the whole image at its own size, a 1 x 1 window: always fits; the plan of GpuImageLoader.decode
_DECODE_ONLY = _Builder(lambda item, w, h: ((0, 0, w, h), (w, h), (0, 0), BILINEAR, False), (1, 1), None)


def descriptor(geometry, w, h, out_hw, src_offset=0, out_offset=0):
    """One SaisImgXform row (a tuple for XFORM_DTYPE) of a builder's answer for a w x h image."""
    box, (rw, rh), (wl, wt), filt, flip = geometry
    return (src_offset, h, w, tuple(int(v) for v in box), rw, rh, wl, wt, filt, int(flip), out_offset)


def fits(row, out_hw):
    """sais_image_transform_fits (a host function): does the descriptor's one-row band fit in LDS?"""
    d = L.SaisImgXform.from_buffer_copy(np.array([row], dtype=XFORM_DTYPE).tobytes())
    return bool(L.load().sais_image_transform_fits(ctypes.byref(d), out_hw[0], out_hw[1]))


def _pillow_rgb(blob):
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as img:
        return np.array(img.convert("RGB"))


# ------------------------------------------------------------------------------------------------ the batch plan (host only)
class BatchPlan:
    """Where every item of a batch goes.  gpu: decoded on the device; host: decoded by Pillow, pixels uploaded; pillow:
    the Pillow transform itself.  table rows exist for gpu + host items (`rows`, in batch order); src offsets address one
    buffer that holds the host-decoded pixels first (inside the upload) and the device-decoded images after it."""

    def __init__(self, items, builder):
        self.items, self.builder, self.out_hw = items, builder, builder.out_hw
        oh, ow = self.out_hw
        self.gpu, self.host, self.pillow, self.rows = [], {}, [], []
        self.headers, self.sizes = {}, {}
        for i, item in enumerate(items):
            blob, hdr = item[0], item[1]
            h = None if hdr is None else jpeg.SaisJpegHeader.from_buffer_copy(hdr)
            if h is None:
                rgb = _pillow_rgb(blob)
                w_, h_ = rgb.shape[1], rgb.shape[0]
            else:
                rgb, (w_, h_) = None, (h.width, h.height)
            row = descriptor(builder(item, w_, h_), w_, h_, self.out_hw, 0, i * 3 * oh * ow)
            if not fits(row, self.out_hw):
                self.pillow.append(i)
                continue
            self.sizes[i] = (w_, h_)
            self.rows.append((i, row))
            if h is None:
                self.host[i] = rgb
            else:
                self.gpu.append(i)
                self.headers[i] = h


# ------------------------------------------------------------------------------------------------ device back end
class _HipBackend:
    """The device half of GpuImageLoader: buffers, the two launches, the status read."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SaisHipError("GpuImageLoader needs a GPU device: the HIP path has no CPU fallback")
        L.load()
        self._lut = torch.from_numpy(normalize_table()).to(self.device)
        self._pinned = self._dev = self._ws = self._status = None

    def decode(self, plan):
        """Pack, copy, decode: the status of plan.gpu (numpy int32), after which the pinned buffer is free again."""
        al = lambda v: (v + 255) // 256 * 256                        # noqa: E731
        m, rows = len(plan.gpu), plan.rows
        # upload: [headers][decode offsets][descriptor table][JPEG files][host-decoded pixels]; then the decoded images
        o_hdr = 0
        o_off = al(o_hdr + m * jpeg.HDR_BYTES)
        o_tab = al(o_off + 8 * m)
        o_data = al(o_tab + XFORM_DTYPE.itemsize * len(rows))
        data_bytes = sum(len(plan.items[i][0]) for i in plan.gpu)
        o_pix = al(o_data + data_bytes)
        src = {}
        o = o_pix
        for i, rgb in plan.host.items():
            src[i] = o
            o = al(o + rgb.size)
        upload = o
        dec_off = []
        for i in plan.gpu:
            w, h = plan.sizes[i]
            src[i] = o
            dec_off.append(o - upload)
            o = al(o + 3 * w * h)
        total = o
        self._pinned = jpeg.grow(self._pinned, upload, pin_memory=True)
        self._dev = jpeg.grow(self._dev, total, device=self.device)
        base = self._pinned.data_ptr()
        pin = self._pinned.numpy()
        headers = (jpeg.SaisJpegHeader * max(m, 1))()
        fo = 0
        for k, i in enumerate(plan.gpu):
            blob = plan.items[i][0]
            hh = jpeg.SaisJpegHeader.from_buffer_copy(plan.headers[i])
            hh.scan_offset += fo
            headers[k] = hh
            ctypes.memmove(base + o_data + fo, blob, len(blob))
            fo += len(blob)
        ctypes.memmove(base + o_hdr, ctypes.addressof(headers), m * jpeg.HDR_BYTES)
        offs = np.asarray(dec_off, dtype=np.int64)
        pin[o_off:o_off + 8 * m] = offs.view(np.uint8)
        table = np.array([(src[i],) + r[1:] for i, r in rows], dtype=XFORM_DTYPE)
        pin[o_tab:o_tab + table.nbytes] = table.view(np.uint8).reshape(-1)
        for i, rgb in plan.host.items():
            pin[src[i]:src[i] + rgb.size] = rgb.reshape(-1)
        self._table, self._o_tab, self._total, self._src = table, o_tab, total, src
        status = np.zeros(0, np.int32)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            self._dev[:upload].copy_(self._pinned[:upload], non_blocking=True)
            if m:
                lib = L.load()
                need = lib.sais_jpeg_mixed_workspace_bytes(headers, m)
                if need == 0:
                    raise L.SaisHipError("sais_jpeg_mixed_workspace_bytes rejected the batch")
                self._ws = jpeg.grow(self._ws, need, device=self.device)
                if self._status is None or self._status.numel() < m:
                    self._status = torch.empty(max(m, 256), dtype=torch.int32, device=self.device)
                d = self._dev.data_ptr()
                self._last = (m, d + o_data, data_bytes, headers, d + o_hdr, offs, d + o_off, d + upload, total - upload)
                self.launch_decode(stream)
                status = self._status[:m].cpu().numpy()               # synchronises: the pinned buffer is free again
            else:
                stream.synchronize()
        return status

    def launch_decode(self, stream):
        """sais_jpeg_decode_mixed of the last packed batch, from the bytes already on the device, without synchronising."""
        m, data, data_bytes, headers, hdr_dev, offs, off_dev, out, out_bytes = self._last
        L.call("sais_jpeg_decode_mixed", m, data, data_bytes, headers, hdr_dev, offs.ctypes.data, off_dev,
               self._ws.data_ptr(), self._ws.numel(), out, out_bytes, self._status.data_ptr(), stream.cuda_stream)

    def upload(self, plan, i, rgb):
        """The pixels of a file the GPU flagged, into the slot its decode would have filled."""
        o = self._src[i]
        self._dev[o:o + rgb.size].copy_(torch.from_numpy(rgb.reshape(-1)))

    def image(self, plan, i):
        """A copy of the decoded image of item i of the last packed batch: uint8 [h,w,3] on the device."""
        w, h = plan.sizes[i]
        o = self._src[i]
        return self._dev[o:o + 3 * w * h].view(h, w, 3).clone()

    def launch_transform(self, out, stream):
        """sais_image_transform of the last packed batch into `out` (float32 [B,3,h,w]), without synchronising."""
        L.call("sais_image_transform", self._dev.data_ptr(), self._total, self._table.ctypes.data,
               self._dev.data_ptr() + self._o_tab, len(self._table), out.shape[2], out.shape[3], self._lut.data_ptr(),
               out.data_ptr(), out.numel(), stream.cuda_stream)

    def transform(self, plan, tensors):
        """[B,3,h,w] on the device: the table's images through the kernel, `tensors` (index -> Pillow-made tensor) copied in."""
        oh, ow = plan.out_hw
        out = torch.empty(len(plan.items), 3, oh, ow, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            if len(self._table):
                self.launch_transform(out, torch.cuda.current_stream(self.device))
            for i, t in tensors.items():
                out[i].copy_(t)
        return out


class GpuImageLoader:
    """loader(items, builder) -> float32 [B,3,h,w] on the device, equal bit for bit to the stacked items of the Pillow
    dataset the builder stands for.  eval / train / square are the three batch hooks of the tools.  stats: files decoded on
    the GPU; files the parser refused ("unsupported") and files the GPU flagged ("failed"), both decoded by Pillow and
    transformed on the device; images the fit predicate refused ("pillow_transform"), transformed by Pillow."""

    def __init__(self, device="cuda:0", backend=None):
        self.backend = backend if backend is not None else _HipBackend(device)
        self.stats = {"gpu": 0, "unsupported": 0, "failed": 0, "pillow_transform": 0}
        self._builders = {}

    def __call__(self, items, builder):
        if len(items) == 0:
            raise ValueError("GpuImageLoader needs at least one item")
        plan = BatchPlan(items, builder)
        status = self.backend.decode(plan)
        failed = [plan.gpu[k] for k in np.flatnonzero(status)]
        for i in failed:
            rgb = _pillow_rgb(items[i][0])
            if (rgb.shape[1], rgb.shape[0]) != plan.sizes[i]:
                raise ValueError(f"item {i}: Pillow decodes {rgb.shape[1]}x{rgb.shape[0]}, the header says "
                                 f"{plan.sizes[i][0]}x{plan.sizes[i][1]}")
            self.backend.upload(plan, i, rgb)
        tensors = {}
        for i in plan.pillow:
            from PIL import Image
            with Image.open(io.BytesIO(items[i][0])) as img:
                tensors[i] = builder.pillow(items[i], img)
        self.stats["gpu"] += len(plan.gpu) - len(failed)
        self.stats["failed"] += len(failed)
        self.stats["unsupported"] += len(plan.host)
        self.stats["pillow_transform"] += len(plan.pillow)
        self.last_plan = plan
        return self.backend.transform(plan, tensors)

    def decode(self, items):
        """The mixed decode alone, without any host decode: ([uint8 [h,w,3] device tensor, or None for an item the parser
        refused, per item], [status of sais_jpeg_decode_mixed, or None, per item])."""
        plan = BatchPlan(items, _DECODE_ONLY)
        status = self.backend.decode(plan)
        images, codes = [None] * len(items), [None] * len(items)
        for k, i in enumerate(plan.gpu):
            images[i], codes[i] = self.backend.image(plan, i), int(status[k])
        self.last_plan = plan
        return images, codes

    def _builder(self, key, make):
        if key not in self._builders:
            self._builders[key] = make()
        return self._builders[key]

    def eval(self, items):
        return self(items, self._builder("eval", eval_builder))

    def train(self, items):
        return self(items, self._builder("train", train_builder))

    def square(self, items, imsize):
        return self(items, self._builder(("square", int(imsize)), lambda: square_builder(imsize)))


class GpuBatches:
    """Wraps a DataLoader over a raw dataset (collate_raw): yields (device tensor, index or label tensor) as the Pillow
    loaders yield (host tensor, index or label tensor).  `dataset` is the raw dataset (samples, classes, set_epoch)."""

    def __init__(self, loader, hook):
        self.loader, self.hook, self.dataset = loader, hook, loader.dataset

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for items, tags in self.loader:
            yield self.hook(items), tags
