"""Baseline-JPEG encode on the MI355X: uint8 [N,H,W,3] on the device -> the files Pillow writes, byte for byte.

The counterpart of sais_amd/jpeg.py for the images the project produces on the device (attention heat maps, colour-coded optical
flow).  `sais_jpeg_encode` (sais_amd/csrc/jpeg_enc.hip) writes the entropy-coded scan and the EOI marker of every image of a batch;
`header` builds the bytes before the scan on the host.  The forms are the ones `Image.save(format="jpeg")` takes at its defaults:
baseline, 8 bit, the Annex K Huffman tables, YCbCr 4:2:0 or 4:4:4, libjpeg's quality scaling.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from .jpeg import grow

# ITU-T T.81 Annex K: quantisation tables (natural order) and Huffman tables (code counts per length 1..16, symbols)
Q_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
          100, 103, 99)
Q_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) \
    + (99,) * 32
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_AC_LUMA = ("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a4344454647"
            "48494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9"
            "bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = ("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546"
              "4748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7"
              "b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
# (table class << 4 | id, counts, symbols) in the order the files carry them: DC0, AC0, DC1, AC1
HUFFMAN = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), bytes.fromhex(_AC_LUMA)),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), bytes.fromhex(_AC_CHROMA)),
)
SUBSAMPLING = {"4:4:4": 0, "4:2:0": 2, 0: 0, 2: 2}


class SaisJpegEncParams(ctypes.Structure):
    _fields_ = [("q", (ctypes.c_uint16 * 64) * 2), ("subsampling", ctypes.c_int)]


def quant_tables(quality):
    """The two quantisation tables (natural order, u16 [2, 64]) of jpeg_set_quality(quality, force_baseline=TRUE)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    t = (np.array([Q_LUMA, Q_CHROMA], dtype=np.int64) * scale + 50) // 100
    return np.clip(t, 1, 255).astype(np.uint16)


def _subsampling(subsampling):
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling = {subsampling!r}: only '4:2:0' (2) and '4:4:4' (0)")
    return SUBSAMPLING[subsampling]


def _dpi(dpi):
    if dpi is None:
        return None
    x, y = (int(round(v)) for v in dpi)
    if not (0 < x < 65536 and 0 < y < 65536):
        raise ValueError(f"dpi = {dpi!r}: two values in 1..65535")
    return x, y


def _segment(marker, payload):
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(height, width, quality=75, subsampling="4:2:0", dpi=None):
    """The bytes Image.save(format="jpeg", quality=..., subsampling=..., dpi=...) writes before the scan data of an RGB image."""
    sub = _subsampling(subsampling)
    height, width = int(height), int(width)
    if not (1 <= height <= 65535 and 1 <= width <= 65535):
        raise ValueError(f"{height} x {width}: each side in 1..65535")
    dpi = _dpi(dpi)
    units, (dx, dy) = (0, (1, 1)) if dpi is None else (1, dpi)
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0\x01\x01" + bytes((units,)) + dx.to_bytes(2, "big") + dy.to_bytes(2, "big") + b"\0\0")]
    for i, t in enumerate(quant_tables(quality)):
        out.append(_segment(0xDB, bytes((i,)) + bytes(int(t[z]) for z in ZIGZAG)))
    ysamp = 0x22 if sub == 2 else 0x11
    out.append(_segment(0xC0, b"\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") +
                        bytes((3, 1, ysamp, 0, 2, 0x11, 1, 3, 0x11, 1))))
    for tc_th, counts, symbols in HUFFMAN:
        out.append(_segment(0xC4, bytes((tc_th,)) + bytes(counts) + symbols))
    out.append(_segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))))
    return b"".join(out)


def encode_bound(height, width, subsampling="4:2:0"):
    """sais_jpeg_encode_bound: the worst-case bytes of one image's scan + EOI (a host function of the library)."""
    return int(L.load().sais_jpeg_encode_bound(int(height), int(width), _subsampling(subsampling)))


def check_options(**options):
    """Image.save keywords this encoder does not implement: a ValueError that names the option."""
    for name in ("optimize", "progressive"):
        if options.pop(name, False):
            raise ValueError(f"{name}: not supported (baseline files with the Annex K Huffman tables only)")
    if options.pop("restart_marker_blocks", 0) or options.pop("restart_marker_rows", 0):
        raise ValueError("restart intervals (restart_marker_blocks / restart_marker_rows): not supported")
    if options.pop("grayscale", False):
        raise ValueError("grayscale: not supported (three-component RGB input only)")
    if options:
        raise ValueError(f"unknown option(s) {sorted(options)}")


class JpegEncoder:
    """Encodes batches of one geometry.  The workspace, the output buffer and the pinned host buffer are reused across calls."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SaisHipError("JpegEncoder needs a GPU device: the HIP path has no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        L.load()
        self._ws = self._out = self._nbytes = self._pinned = None

    def _check(self, rgb):
        if not isinstance(rgb, torch.Tensor) or rgb.device != self.device or rgb.dtype != torch.uint8 or rgb.dim() != 4 \
                or rgb.shape[3] != 3 or rgb.shape[0] < 1 or not rgb.is_contiguous():
            raise ValueError(f"rgb: expected a contiguous u8 [N, H, W, 3] tensor on {self.device} (grayscale and host arrays "
                             "are not supported)")
        return tuple(rgb.shape[:3])

    def encode_to_device(self, rgb, quality=75, subsampling="4:2:0", out_stride=None, out=None, **options):
        """-> (out u8 [N, out_stride], nbytes i32 [N]) on the device, without synchronising: slot i holds nbytes[i] bytes, from the
        first entropy-coded byte through EOI, or nbytes[i] = -1 when they do not fit out_stride (default: the worst case).
        The two tensors are the encoder's own buffers: the next call overwrites them.  out: a contiguous u8 [N, out_stride]
        tensor of the caller's to write into instead; bytes of a slot past nbytes[i] are left as they were."""
        check_options(**options)
        n, H, W = self._check(rgb)
        sub = _subsampling(subsampling)
        if H > 65535 or W > 65535 or n > 65535:
            raise ValueError(f"{n} images of {H} x {W}: at most 65535 each")
        lib = L.load()
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.uint8 or out.dim() != 2 \
                    or out.shape[0] != n or not out.is_contiguous() or out_stride not in (None, out.shape[1]):
                raise ValueError(f"out: expected a contiguous u8 [{n}, out_stride] tensor on {self.device}")
            out_stride = out.shape[1]
        stride = int(lib.sais_jpeg_encode_bound(H, W, sub)) if out_stride is None else int(out_stride)
        if stride < 2:
            raise ValueError(f"out_stride = {out_stride}: at least 2 bytes")
        need = int(lib.sais_jpeg_encode_workspace_bytes(n, H, W, sub))
        if need == 0:
            raise L.SaisHipError("sais_jpeg_encode_workspace_bytes rejected the batch")
        p = SaisJpegEncParams()
        p.subsampling = sub
        for t, table in enumerate(quant_tables(quality)):
            for k in range(64):
                p.q[t][k] = int(table[k])
        self._ws = grow(self._ws, need, device=self.device)
        if out is None:
            self._out = grow(self._out, n * stride, device=self.device)
            out = self._out[:n * stride].view(n, stride)
        if self._nbytes is None or self._nbytes.numel() < n:
            self._nbytes = torch.empty(max(n, 256), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            L.call("sais_jpeg_encode", rgb.data_ptr(), n, H, W, ctypes.byref(p), self._ws.data_ptr(), self._ws.numel(),
                   out.data_ptr(), stride, self._nbytes.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        return out, self._nbytes[:n]

    def encode(self, rgb, quality=75, subsampling="4:2:0", dpi=None, **options):
        """-> a list of N `bytes`: the complete files Image.save(format="jpeg", quality, subsampling, dpi) writes for the images."""
        out, nbytes = self.encode_to_device(rgb, quality, subsampling, **options)
        n, H, W = tuple(rgb.shape[:3])
        head = header(H, W, quality, subsampling, dpi)
        lens = nbytes.cpu().numpy()                                       # copy 1: the lengths
        if (lens < 2).any():
            raise L.SaisHipError(f"sais_jpeg_encode: image {int(np.flatnonzero(lens < 2)[0])} did not fit its worst-case bound")
        longest = int(lens.max())
        self._pinned = grow(self._pinned, n * longest, pin_memory=True)
        host = self._pinned[:n * longest].view(n, longest)
        host.copy_(out[:, :longest])                                      # copy 2: the used bytes
        rows = host.numpy()
        return [head + rows[i, :lens[i]].tobytes() for i in range(n)]
