"""DINO multi-crop augmentation on the MI355X: decoded uint8 frames + drawn ViewParams -> the crop list.

Replaces the pixel half of DataAugmentationDINO (sais_amd/dino_data.py: apply_view_pillow, one image at a time in
DataLoader workers) with sais_augment_crop_resize + sais_augment_color (sais_amd/csrc/augment.hip).  For the same
ViewParams the tensors are bit-identical to the Pillow path.  There is no CPU fallback: the Pillow path is selected by
the caller (main_dino.py without --gpu_augment), never from here.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from .dino_data import MEAN, STD

VIEW_DTYPE = np.dtype([("frame", "<i4"), ("box", "<i4", 4), ("size", "<i4"), ("flip", "<i4"), ("jitter", "<i4"),
                       ("order", "<i4", 4), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"),
                       ("hue_shift", "<i4"), ("gray", "<i4"), ("blur", "<i4"), ("blur_radius", "<f4"), ("solarize", "<i4"),
                       ("reserved", "<i4"), ("u8_offset", "<i8"), ("out_offset", "<i8")], align=True)
assert VIEW_DTYPE.itemsize == ctypes.sizeof(L.SaisAugView)


def normalize_table():
    """[3][256] float32: the value to_normalized_tensor gives each byte of each channel, by its very expression."""
    a = np.broadcast_to(np.arange(256, dtype=np.float32).reshape(1, 256, 1), (3, 256, 1)) / 255.0
    return np.ascontiguousarray(((a - MEAN) / STD).reshape(3, 256))


def view_table(params):
    """params[n][j] = ViewParams of view j of frame n -> (table in view-major order j * N + n, sizes per view slot).
    u8_offset / out_offset lay the views out as [slot][frame] in one buffer each."""
    n, slots = len(params), len(params[0])
    if n == 0 or any(len(p) != slots for p in params):
        raise ValueError("every frame needs the same number of views")
    sizes = [params[0][j].size for j in range(slots)]
    rows, off = [], 0
    for j in range(slots):
        for i in range(n):
            p = params[i][j]
            if p.size != sizes[j]:
                raise ValueError(f"view {j}: sizes differ between frames")
            rows.append((i, p.box, p.size, p.flip, p.jitter, p.order, p.brightness, p.contrast, p.saturation,
                         p.hue_shift if p.jitter else 0, p.gray, p.blur is not None, p.blur or 0.0, p.solarize, 0, off, off))
            off += 3 * p.size * p.size
    return np.array(rows, dtype=VIEW_DTYPE), sizes


class DinoAugmenter:
    """augmenter(frames_u8, params, border) -> [tensor [N,3,s,s] per view slot], float32, normalised, on the device.
    The view table travels through a reused pinned buffer; the uint8 views between the two kernels live in a reused
    workspace.  `crop_resize` and `color` run the two halves on their own."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SaisHipError("DinoAugmenter needs a GPU device: the HIP path has no CPU fallback")
        L.load()
        self._lut = torch.from_numpy(normalize_table()).to(self.device)
        self._pinned = self._dev = self._ws = self._copied = self._last = None

    def _upload(self, table):
        """The table in device memory (stream-ordered copy from the pinned buffer)."""
        nbytes = table.nbytes
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty(2 * nbytes, dtype=torch.uint8, pin_memory=True)
            self._dev = torch.empty(2 * nbytes, dtype=torch.uint8, device=self.device)
        elif self._copied is not None:
            self._copied.synchronize()                               # the previous call's copy has left the buffer
        self._pinned[:nbytes].numpy()[:] = table.view(np.uint8).reshape(-1)
        self._dev[:nbytes].copy_(self._pinned[:nbytes], non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record(torch.cuda.current_stream(self.device))
        return self._dev.data_ptr()

    def _workspace(self, table):
        need = L.load().sais_augment_workspace_bytes(table.ctypes.data, len(table))
        if need == 0:
            raise L.SaisHipError("sais_augment_workspace_bytes rejected the view table")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    @staticmethod
    def _check_frames(frames):
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
            raise ValueError("frames must be a contiguous uint8 [N,H,W,3] tensor")

    def _crop_resize(self, frames, table, border, dev_table, ws, stream):
        border4 = (ctypes.c_int * 4)(*border)
        L.call("sais_augment_crop_resize", frames.data_ptr(), frames.shape[0], frames.shape[1], frames.shape[2], border4,
               table.ctypes.data, dev_table, len(table), ws.data_ptr(), ws.numel(), stream.cuda_stream)

    def _color(self, ws, table, dev_table, out, stream):
        L.call("sais_augment_color", ws.data_ptr(), ws.numel(), table.ctypes.data, dev_table, len(table),
               self._lut.data_ptr(), out.data_ptr(), out.numel(), stream.cuda_stream)

    @staticmethod
    def _split(buf, n, sizes, shape):
        out, off = [], 0
        for s in sizes:
            cnt = n * 3 * s * s
            out.append(buf[off:off + cnt].view(n, *shape(s)))
            off += cnt
        return out

    def __call__(self, frames_u8, params, border):
        """frames_u8: uint8 [N,H,W,3] on the device; params[n] = the ViewParams of frame n; border = (left, top, width,
        height) of SurgDataset's border crop, the frame the boxes refer to."""
        self._check_frames(frames_u8)
        if frames_u8.device != self.device or len(params) != frames_u8.shape[0]:
            raise ValueError("frames and params disagree (device or count)")
        table, sizes = view_table(params)
        n = frames_u8.shape[0]
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            dev_table, ws = self._upload(table), self._workspace(table)
            out = torch.empty(int(table["out_offset"][-1]) + 3 * sizes[-1] ** 2, dtype=torch.float32, device=self.device)
            self._last = (frames_u8, table, tuple(border), dev_table, ws, sizes)
            self._crop_resize(frames_u8, table, border, dev_table, ws, stream)
            self._color(ws, table, dev_table, out, stream)
        return self._split(out, n, sizes, lambda s: (3, s, s))

    def relaunch(self):
        """Both kernels again on the frames and the view table of the last call, which are still on the device, into a
        fresh output, on the current stream, without touching the host buffers.  For timing the device work alone
        (tools/dino_aug_bench.py)."""
        frames, table, border, dev_table, ws, sizes = self._last
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            out = torch.empty(int(table["out_offset"][-1]) + 3 * sizes[-1] ** 2, dtype=torch.float32, device=self.device)
            self._crop_resize(frames, table, border, dev_table, ws, stream)
            self._color(ws, table, dev_table, out, stream)
        return self._split(out, frames.shape[0], sizes, lambda s: (3, s, s))

    def crop_resize(self, frames_u8, params, border):
        """First half alone: [uint8 [N,s,s,3] per view slot] (a copy, not the workspace)."""
        self._check_frames(frames_u8)
        table, sizes = view_table(params)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            dev_table, ws = self._upload(table), self._workspace(table)
            self._crop_resize(frames_u8, table, border, dev_table, ws, stream)
            return self._split(ws.clone(), frames_u8.shape[0], sizes, lambda s: (s, s, 3))

    def color(self, views_u8, params):
        """Second half alone: views_u8 = [uint8 [N,s,s,3] per view slot] (already cropped and resized)."""
        table, sizes = view_table(params)
        if len(views_u8) != len(sizes) or any(tuple(v.shape) != (len(params), s, s, 3) or v.dtype != torch.uint8
                                              for v, s in zip(views_u8, sizes)):
            raise ValueError("views_u8 must hold one uint8 [N,s,s,3] tensor per view slot")
        n = len(params)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            dev_table = self._upload(table)
            ws = torch.cat([v.to(self.device).reshape(-1) for v in views_u8])
            out = torch.empty(ws.numel(), dtype=torch.float32, device=self.device)
            self._color(ws, table, dev_table, out, stream)
        return self._split(out, n, sizes, lambda s: (3, s, s))
