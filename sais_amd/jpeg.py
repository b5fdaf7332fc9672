"""Baseline-JPEG decode on the MI355X: compressed frames -> uint8 [N,H,W,3] on the device.

Replaces the host decode of SurgDataset.__getitem__ (dino-main/main_dino.py:295-316: Image.open + np.asarray) on the
feature-extraction path (extract_representations.py:158-162).  `sais_jpeg_decode` (sais_amd/csrc/jpeg.hip) is
bit-identical to Pillow + libjpeg-turbo for the files `sais_jpeg_parse` accepts: baseline / extended-sequential Huffman,
8 bit, YCbCr 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan.  Every other file, and every file whose entropy data the GPU
reports as corrupt or out of range, is decoded by Pillow into its slot: that host path is the only one for those inputs.
"""
import ctypes
import io

import numpy as np
import torch

from . import _lib as L

c_int, c_int64, c_uint16, c_uint8 = ctypes.c_int, ctypes.c_int64, ctypes.c_uint16, ctypes.c_uint8
UNSUPPORTED = -3                                                   # SAIS_JPEG_UNSUPPORTED


class SaisJpegHuff(ctypes.Structure):
    _fields_ = [("lookup", c_uint16 * 512), ("maxcode", ctypes.c_int32 * 18), ("valoffset", ctypes.c_int32 * 18),
                ("huffval", c_uint8 * 256)]


class SaisJpegHeader(ctypes.Structure):
    _fields_ = [("height", c_int), ("width", c_int), ("hsamp", c_int), ("vsamp", c_int), ("restart_interval", c_int),
                ("mcu_count", c_int), ("segments", c_int), ("qsel", c_int * 3), ("dcsel", c_int * 3),
                ("acsel", c_int * 3), ("scan_offset", c_int64), ("scan_bytes", c_int64),
                ("quant", (c_uint16 * 64) * 4), ("dc", SaisJpegHuff * 2), ("ac", SaisJpegHuff * 2)]


class SaisJpegBatch(ctypes.Structure):
    _fields_ = [("n", c_int), ("height", c_int), ("width", c_int), ("total_segments", c_int),
                ("total_scan_bytes", c_int64), ("data_bytes", c_int64)]


HDR_BYTES = ctypes.sizeof(SaisJpegHeader)


def parse_rc(blob):
    """sais_jpeg_parse on the host: (return code, header)."""
    h = SaisJpegHeader()
    rc = L.load().sais_jpeg_parse(blob, len(blob), ctypes.byref(h))
    return rc, h


def parse_header(blob):
    """The header of a file the GPU decodes, or None (the file stays with Pillow)."""
    rc, h = parse_rc(blob)
    return h if rc == 0 else None


class JpegModeError(ValueError):
    """A host-decoded file that is not RGB (the batch is uint8 [N,H,W,3])."""


def _host_decode(blob):
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as img:
        if img.mode != 'RGB':
            raise JpegModeError(f'mode {img.mode}; expected RGB')
        return np.asarray(img)


def grow(buf, nbytes, **kw):
    """A reused uint8 buffer of at least nbytes: `buf` itself, or a new one of at least twice its size (the decoder's, the
    encoder's and the image-folder loader's pinned, device and workspace buffers)."""
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 2 * (0 if buf is None else buf.numel())), dtype=torch.uint8, **kw)
    return buf


class JpegDecoder:
    """Decodes batches of one geometry.  The compressed bytes and the per-image headers go to the device in one copy
    from a reused pinned buffer; the workspace is reused too.  stats counts the files per path."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SaisHipError("JpegDecoder needs a GPU device: the HIP path has no CPU fallback")
        L.load()
        self._pinned = self._dev = self._ws = self._status = None
        self.stats = {"gpu": 0, "unsupported": 0, "failed": 0}

    def decode(self, blobs, headers=None):
        """blobs: list of JPEG file contents of one geometry -> uint8 [N,H,W,3] on the device.
        headers: their parse_header() results, when the caller has them already."""
        n = len(blobs)
        if n == 0:
            raise ValueError("decode() needs at least one file")
        if headers is None:
            headers = [parse_header(b) for b in blobs]
        gpu = [i for i in range(n) if headers[i] is not None]
        host = {i: _host_decode(blobs[i]) for i in range(n) if headers[i] is None}
        if gpu:
            H, W = headers[gpu[0]].height, headers[gpu[0]].width
        else:
            H, W = host[0].shape[:2]
        for i, h in enumerate(headers):
            shape = (h.height, h.width) if h is not None else host[i].shape[:2]
            if tuple(shape) != (H, W):
                raise ValueError(f"file {i}: {shape[0]}x{shape[1]}, the batch is {H}x{W}")
        out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=self.device)
        self.stats["unsupported"] += len(host)
        if gpu:
            failed = self._decode_gpu([blobs[i] for i in gpu], [headers[i] for i in gpu], out, gpu, H, W)
            self.stats["gpu"] += len(gpu) - len(failed)
            self.stats["failed"] += len(failed)
            for i in failed:
                host[i] = _host_decode(blobs[i])
        for i, a in host.items():
            if a.shape != (H, W, 3):
                raise ValueError(f"file {i}: decoded shape {a.shape}, the batch is {H}x{W}")
            out[i].copy_(torch.from_numpy(np.array(a)))
        return out

    def _decode_gpu(self, blobs, headers, out, index, H, W):
        m = len(blobs)
        data_off = (m * HDR_BYTES + 255) // 256 * 256
        offs, o = [], 0
        for b in blobs:
            offs.append(o)
            o += len(b)
        total = data_off + o
        self._pinned = grow(self._pinned, total, pin_memory=True)
        self._dev = grow(self._dev, total, device=self.device)
        base = self._pinned.data_ptr()
        for k, (b, h) in enumerate(zip(blobs, headers)):
            hh = SaisJpegHeader.from_buffer_copy(h)
            hh.scan_offset += offs[k]
            ctypes.memmove(base + k * HDR_BYTES, ctypes.addressof(hh), HDR_BYTES)
            ctypes.memmove(base + data_off + offs[k], b, len(b))
        bt = SaisJpegBatch(m, H, W, sum(h.segments for h in headers), sum(h.scan_bytes for h in headers), o)
        lib = L.load()
        need = lib.sais_jpeg_workspace_bytes(m, H, W, bt.total_scan_bytes, bt.total_segments)
        if need == 0:
            raise L.SaisHipError("sais_jpeg_workspace_bytes rejected the batch")
        self._ws = grow(self._ws, need, device=self.device)
        if self._status is None or self._status.numel() < m:
            self._status = torch.empty(max(m, 256), dtype=torch.int32, device=self.device)
        dst = out if m == out.shape[0] else torch.empty(m, H, W, 3, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            self._dev[:total].copy_(self._pinned[:total], non_blocking=True)
            self._last = (bt, m, H, W, data_off)
            self._launch(dst, stream)
            status = self._status[:m].cpu().numpy()              # synchronises: the pinned buffer is free again
        if dst is not out:
            out[torch.as_tensor(index, device=self.device)] = dst
        self.last_status = status
        return [index[k] for k in np.flatnonzero(status)]

    def _launch(self, out, stream):
        bt, _, _, _, data_off = self._last
        L.call("sais_jpeg_decode", ctypes.byref(bt), self._dev.data_ptr() + data_off, self._dev.data_ptr(),
               self._ws.data_ptr(), self._ws.numel(), out.data_ptr(), self._status.data_ptr(), stream.cuda_stream)

    def relaunch(self, out):
        """Decode the last GPU batch again from the bytes already on the device, into `out` (uint8 [m,H,W,3], m = the
        files of that batch the GPU took), on the current stream, without synchronising.  For timing the device
        decode alone (tools/jpeg_bench.py)."""
        _, m, H, W, _ = self._last
        if out.dtype != torch.uint8 or tuple(out.shape) != (m, H, W, 3) or not out.is_contiguous() \
                or out.device != self.device:
            raise ValueError(f"out must be a contiguous uint8 [{m},{H},{W},3] tensor on {self.device}")
        with torch.cuda.device(self.device):
            self._launch(out, torch.cuda.current_stream(self.device))
