"""Image-folder batches on the MI355X: files of mixed sizes -> the normalised [B,3,h,w] tensor the Pillow datasets yield.

The evaluation tools read image folders (ImageNet, Copydays): dozens of geometries per batch.  Their Pillow datasets
(knn.EvalImageFolder, linear.TrainImageFolder, retrieval.ImgListDataset) decode and resample in DataLoader workers.  Here
the workers only read the file and parse its header (the pattern of dino_data.SurgDataset._raw_item), and GpuImageLoader
turns a batch of such items into the same tensor, bit for bit, with one pinned pack and one H2D copy, one
sais_jpeg_decode_mixed (csrc/jpeg.hip), one status read and one sais_image_transform (csrc/imgfolder.hip).
GpuImageLoader.thumbnail is the same path for retrieval.OxfordParisDataset (eval_image_retrieval.py): thumbnail(LANCZOS) keeps
the aspect ratio, so it returns one tensor per image, through one sais_thumbnail (csrc/thumbnail.hip).

Three kinds of file are decoded by Pillow with .convert("RGB"), as the datasets do: files the parser refuses (progressive,
grayscale, CMYK, non-JPEG), files the GPU flags, and images the LDS fit predicate refuses.  The first two have their pixels
uploaded into the packed buffer, so their transform still runs on the device; the third goes through the Pillow transform
itself.  `stats` counts each path.  The Pillow path as a whole is chosen by the caller (the tools without --gpu_loader),
never from here."""
import contextlib
import ctypes
import io
import math
import os

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
THUMB_DTYPE = np.dtype([("src_offset", "<i8"), ("src_h", "<i4"), ("src_w", "<i4"), ("fx", "<i4"), ("fy", "<i4"), ("rw", "<i4"),
                        ("rh", "<i4"), ("ws_offset", "<i8"), ("out_w", "<i4"), ("out_h", "<i4"), ("kx", "<i4"), ("ky", "<i4"),
                        ("cx_offset", "<i8"), ("cy_offset", "<i8"), ("out_offset", "<i8")], align=True)
assert THUMB_DTYPE.itemsize == ctypes.sizeof(L.SaisThumb)


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


class RawOxfordParis(torch.utils.data.Dataset):
    """retrieval.OxfordParisDataset without the pixels: the same gnd_<dataset>.pkl and sample order; item = (bytes, header
    bytes or None, dataset index)."""

    def __init__(self, dir_main, dataset, split):
        from .retrieval import OxfordParisDataset
        ref = OxfordParisDataset(dir_main, dataset, split)
        self.image_dir, self.cfg, self.gnd, self.samples = ref.image_dir, ref.cfg, ref.gnd, ref.samples

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return _read(os.path.join(self.image_dir, self.samples[i] + ".jpg")) + (i,)


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


# ------------------------------------------------------------------------------------------------ thumbnail(LANCZOS)
def _round_aspect(number, key):
    return max(min(math.floor(number), math.ceil(number), key=key), 1)


def thumbnail_geometry(w, h, imsize):
    """img.thumbnail((imsize, imsize), LANCZOS) of a plain w x h RGB Image (Pillow 12.2): None where the image is left
    untouched, else ((x, y), (fx, fy)): the aspect-preserving size of Image.thumbnail and the Image.reduce factors of
    Image.resize with reducing_gap = 2.0.  The reduced image is then resized with box = (0, 0, w / fx, h / fy): horizontal
    pass first, except where Image.resize takes its branch for tall, narrow images (thumbnail_vertical_first), which
    sais_thumbnail does not restate: ThumbPlan routes those to Pillow."""
    x = y = int(math.floor(imsize))
    if x >= w and y >= h:
        return None
    aspect = w / h
    if x / y >= aspect:
        x = _round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = _round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return (x, y), (int(w / x / 2.0) or 1, int(h / y / 2.0) or 1)


def thumbnail_vertical_first(rw, rh, out_h):
    """The last branch of Image.resize, on the size rw x rh of the image after the reduce: more than 100 times as high as
    wide and a lower output: the vertical pass runs first, as a resize of its own."""
    return rh > rw * 100 and out_h < rh


class RowCache(dict):
    """The coefficient rows per axis key, at most `limit` keys (a row is up to about 110 KB): filling a full cache empties
    it first.  A dataset of a few shapes never gets there; a folder of thousands of sizes stays bounded."""

    def __init__(self, limit=512):
        super().__init__()
        self.limit = limit

    def __setitem__(self, key, value):
        if key not in self and len(self) >= self.limit:
            self.clear()
        super().__setitem__(key, value)


def lanczos_rows(src_size, factor, out_size):
    """sais_lanczos_rows (a host function): the coefficient rows of one axis of src_size samples reduced by factor and
    resampled to out_size, as (ksize, int32 [out_size * 2 bounds | out_size * ksize coefficients]); (0, None) where Pillow
    skips the pass."""
    lib = L.load()
    k = lib.sais_lanczos_rows(src_size, factor, out_size, None, None, 0)
    if k < 0:
        raise ValueError(f"sais_lanczos_rows refused ({src_size}, {factor}, {out_size})")
    if k == 0:
        return 0, None
    buf = np.zeros(out_size * (2 + k), np.int32)
    if lib.sais_lanczos_rows(src_size, factor, out_size, buf.ctypes.data, buf[2 * out_size:].ctypes.data, k) != k:
        raise ValueError(f"sais_lanczos_rows refused ({src_size}, {factor}, {out_size})")
    return k, buf


def thumbnail_fits(row):
    """sais_thumbnail_fits (a host function) of one THUMB_DTYPE row."""
    d = L.SaisThumb.from_buffer_copy(np.array([row], dtype=THUMB_DTYPE).tobytes())
    return bool(L.load().sais_thumbnail_fits(ctypes.byref(d)))


def pillow_thumbnail(img, imsize):
    """retrieval.OxfordParisDataset's transform of an opened image: float32 [3, h, w]."""
    from PIL import Image
    from .retrieval import _to_tensor
    img = img.convert("RGB")
    img.thumbnail((imsize, imsize), Image.LANCZOS)
    return _to_tensor(img)


@contextlib.contextmanager
def _truncated_ok():
    """ImageFile.LOAD_TRUNCATED_IMAGES = True, as OxfordParisDataset sets it, for the time of one call."""
    from PIL import ImageFile
    before, ImageFile.LOAD_TRUNCATED_IMAGES = ImageFile.LOAD_TRUNCATED_IMAGES, True
    try:
        yield
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = before


def _pillow_rgb(blob):
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as img:
        return np.array(img.convert("RGB"))


# ------------------------------------------------------------------------------------------------ the batch plan (host only)
class BatchPlan:
    """Where every item of a batch goes.  gpu: decoded on the device; host: decoded by Pillow, pixels uploaded; pillow:
    the Pillow transform itself.  table rows exist for gpu + host items (`rows`, in batch order); src offsets address one
    buffer that holds the host-decoded pixels first (inside the upload) and the device-decoded images after it."""

    dtype, extra = XFORM_DTYPE, None          # the table's row type; int32 words that travel behind the table (ThumbPlan)

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


class ThumbPlan(BatchPlan):
    """BatchPlan of GpuImageLoader.thumbnail: one THUMB_DTYPE row per gpu / host item, each with its own output size
    (out_sizes[i] = (w, h), also for the pillow items), its slot in the float output (out_offset), its reduced image in
    the workspace and its two coefficient rows in `extra`.  `row_cache` maps an axis key (input size, factor, output size)
    to lanczos_rows' answer and is filled here; each distinct key of the batch is packed once."""
    dtype = THUMB_DTYPE

    def __init__(self, items, imsize, row_cache):
        self.items, self.imsize, self.out_hw = items, int(imsize), None
        self.gpu, self.host, self.pillow, self.rows = [], {}, [], []
        self.headers, self.sizes, self.out_sizes = {}, {}, {}
        al = lambda v: (v + 255) // 256 * 256                        # noqa: E731
        packed, words, ws, out = {}, [], 0, 0

        def axis(src, factor, size):
            key = (src, factor, size)
            if key not in row_cache:
                row_cache[key] = lanczos_rows(*key)
            k, buf = row_cache[key]
            if k and key not in packed:
                packed[key] = sum(len(b) for b in words)
                words.append(buf)
            return k, packed.get(key, 0)
        for i, item in enumerate(items):
            blob, hdr = item[0], item[1]
            h = None if hdr is None else jpeg.SaisJpegHeader.from_buffer_copy(hdr)
            if h is None:
                rgb = _pillow_rgb(blob)
                w_, h_ = rgb.shape[1], rgb.shape[0]
            else:
                rgb, (w_, h_) = None, (h.width, h.height)
            g = thumbnail_geometry(w_, h_, self.imsize)
            (x, y), (fx, fy) = g if g is not None else ((w_, h_), (1, 1))
            self.out_sizes[i] = (x, y)
            rw, rh = -(-w_ // fx), -(-h_ // fy)
            # what the entry refuses outright goes to Pillow before any coefficient row is computed for it: sides beyond its
            # limits, and the tall, narrow images whose vertical pass Image.resize runs first
            if max(x, y) > L.THUMB_MAX_OUT or max(w_, h_) > 65535 or thumbnail_vertical_first(rw, rh, y):
                self.pillow.append(i)
                continue
            (kx, cx), (ky, cy) = ((0, 0), (0, 0)) if g is None else (axis(w_, fx, x), axis(h_, fy, y))
            row = (0, h_, w_, fx, fy, rw, rh, ws if fx > 1 or fy > 1 else 0, x, y, kx, ky, cx, cy, out)
            if not thumbnail_fits(row):
                self.pillow.append(i)
                continue
            if fx > 1 or fy > 1:
                ws = al(ws + 3 * rw * rh)
            out += 3 * x * y
            self.sizes[i] = (w_, h_)
            self.rows.append((i, row))
            if h is None:
                self.host[i] = rgb
            else:
                self.gpu.append(i)
                self.headers[i] = h
        self.extra = np.concatenate(words) if words else np.zeros(1, np.int32)
        self.ws_bytes, self.out_elems = max(ws, 256), out


# ------------------------------------------------------------------------------------------------ device back end
class _HipBackend:
    """The device half of GpuImageLoader: buffers, the two launches, the status read."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SaisHipError("GpuImageLoader needs a GPU device: the HIP path has no CPU fallback")
        L.load()
        self._lut = torch.from_numpy(normalize_table()).to(self.device)
        self._pinned = self._dev = self._ws = self._status = self._thumb_ws = None

    def decode(self, plan):
        """Pack, copy, decode: the status of plan.gpu (numpy int32), after which the pinned buffer is free again."""
        al = lambda v: (v + 255) // 256 * 256                        # noqa: E731
        m, rows = len(plan.gpu), plan.rows
        # upload: [headers][decode offsets][descriptor table][extra words][JPEG files][host-decoded pixels]; then the decoded images
        o_hdr = 0
        o_off = al(o_hdr + m * jpeg.HDR_BYTES)
        o_tab = al(o_off + 8 * m)
        extra = plan.extra
        o_ext = al(o_tab + plan.dtype.itemsize * len(rows))          # int32 words behind the table (coefficient rows)
        o_data = al(o_ext + (0 if extra is None else extra.nbytes))
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
        table = np.array([(src[i],) + r[1:] for i, r in rows], dtype=plan.dtype)
        pin[o_tab:o_tab + table.nbytes] = table.view(np.uint8).reshape(-1)
        if extra is not None:
            pin[o_ext:o_ext + extra.nbytes] = extra.view(np.uint8)
        self._o_ext = o_ext
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

    def launch_thumbnail(self, plan, out, stream):
        """sais_thumbnail of the last packed batch (a ThumbPlan) into the flat float32 `out`, without synchronising."""
        L.call("sais_thumbnail", self._dev.data_ptr(), self._total, self._table.ctypes.data, self._dev.data_ptr() + self._o_tab,
               len(self._table), plan.extra.ctypes.data, self._dev.data_ptr() + self._o_ext, plan.extra.size,
               self._thumb_ws.data_ptr(), self._thumb_ws.numel(), self._lut.data_ptr(), out.data_ptr(), out.numel(),
               stream.cuda_stream)

    def thumbnail(self, plan, tensors):
        """[float32 [1,3,h_i,w_i] on the device per item]: the table's images through the kernels (views of one buffer),
        `tensors` (index -> Pillow-made tensor) uploaded."""
        out = torch.empty(max(plan.out_elems, 1), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            if len(self._table):
                need = L.load().sais_thumbnail_workspace_bytes(self._table.ctypes.data, len(self._table))
                if need == 0:
                    raise L.SaisHipError("sais_thumbnail_workspace_bytes rejected the batch")
                self._thumb_ws = jpeg.grow(self._thumb_ws, need, device=self.device)
                self.launch_thumbnail(plan, out, torch.cuda.current_stream(self.device))
            res = [None] * len(plan.items)
            for i, row in plan.rows:
                w, h = plan.out_sizes[i]
                res[i] = out[row[14]:row[14] + 3 * h * w].view(1, 3, h, w)
            for i, t in tensors.items():
                res[i] = t.to(self.device)[None]
        return res


class GpuImageLoader:
    """loader(items, builder) -> float32 [B,3,h,w] on the device, equal bit for bit to the stacked items of the Pillow
    dataset the builder stands for.  eval / train / square are the three batch hooks of the tools.  stats: files decoded on
    the GPU; files the parser refused ("unsupported") and files the GPU flagged ("failed"), both decoded by Pillow and
    transformed on the device; images the fit predicate refused ("pillow_transform"), transformed by Pillow."""

    def __init__(self, device="cuda:0", backend=None):
        self.backend = backend if backend is not None else _HipBackend(device)
        self.stats = {"gpu": 0, "unsupported": 0, "failed": 0, "pillow_transform": 0}
        self._builders = {}
        self.row_cache = RowCache()          # (input size, factor, output size) -> lanczos_rows' answer (thumbnail)

    def __call__(self, items, builder):
        if len(items) == 0:
            raise ValueError("GpuImageLoader needs at least one item")
        plan = BatchPlan(items, builder)
        return self.backend.transform(plan, self._decode(plan, builder.pillow))

    def _decode(self, plan, pillow):
        """Decodes the plan's files, uploads what the GPU flagged, counts every path: {index: tensor of pillow(item, img)}
        of the items that take the Pillow transform."""
        items = plan.items
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
                tensors[i] = pillow(items[i], img)
        self.stats["gpu"] += len(plan.gpu) - len(failed)
        self.stats["failed"] += len(failed)
        self.stats["unsupported"] += len(plan.host)
        self.stats["pillow_transform"] += len(plan.pillow)
        self.last_plan = plan
        return tensors

    def thumbnail(self, items, imsize):
        """[float32 [1,3,h_i,w_i] device tensor per item], each equal bit for bit to retrieval.OxfordParisDataset(imsize)'s
        sample of that file: convert("RGB"), thumbnail((imsize, imsize), LANCZOS), ToTensor, Normalize.  Truncated files
        decode as the dataset decodes them (LOAD_TRUNCATED_IMAGES).  What sais_thumbnail does not take (sides beyond its limits,
        a one-row band beyond LDS, the vertical-first order of tall, narrow images) is made by Pillow's thumbnail itself."""
        if len(items) == 0:
            raise ValueError("GpuImageLoader needs at least one item")
        imsize = int(imsize)
        with _truncated_ok():
            plan = ThumbPlan(items, imsize, self.row_cache)
            tensors = self._decode(plan, lambda item, img: pillow_thumbnail(img, imsize))
        return self.backend.thumbnail(plan, tensors)

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
