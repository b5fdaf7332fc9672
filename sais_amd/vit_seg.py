"""Host side of a backbone pass over frames of DIFFERENT sizes (csrc/attn_seg.hip): every frame is a segment of the stacked token
rows.  `SegPlan` is the pass's description, built once on the host: the segment table (one sais_vit_seg record per frame), the
tile table of the attention launch ((segment, first query) per workgroup) and the per-axis tap matrices of the positional
interpolation, in ONE buffer that reaches the device in one pinned copy.  No GPU code here: everything but `SegPlan.to_device`
runs without one.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L

PATCH, POS_SIDE, HEADS = 16, 14, 6
MAX_TOKENS = 4097                    # SAIS_VIT_ATTN_ANY_MAX_TOKENS
MAX_SEGMENTS = 65535
SEG_DTYPE = np.dtype([("row0", "<i4"), ("ntok", "<i4"), ("gh", "<i4"), ("gw", "<i4"), ("pix", "<i8"), ("tap_y", "<i4"),
                      ("tap_x", "<i4")])           # sais_vit_seg, 32 bytes
assert SEG_DTYPE.itemsize == ctypes.sizeof(L.SaisVitSeg) == 32

_AXIS = {}                           # grid side -> f32 [side, 14]: cached per SIDE, shared by every shape that has it


def axis_taps_f32(n0):
    """vit.pos_axis_matrix(14, n0) (interpolate_pos_encoding along one axis) as the kernel reads it, f32 [n0, 14], cached per
    grid side."""
    m = _AXIS.get(n0)
    if m is None:
        from .vit import pos_axis_matrix
        m = _AXIS[n0] = np.ascontiguousarray(pos_axis_matrix(POS_SIDE, n0), dtype=np.float32)
    return m


def attn_qtile(ntoks):
    """Queries per workgroup of the segmented attention: sais_vit_attn_fwd_any's rule on the total of the pass (64-query
    workgroups unless they would leave the chip short of two workgroups per CU: 6 heads x 64-query tiles >= 512)."""
    return 64 if HEADS * sum((n + 63) // 64 for n in ntoks) >= 512 else 32


def tile_table(ntoks, qtile):
    """int32 [ntiles, 2]: (segment, first query) of every workgroup, segments in order, queries in steps of qtile; the last tile
    of a segment may be partial.  No padding to the longest segment: a pass holds token counts that differ by 4x and more."""
    counts = [(n + qtile - 1) // qtile for n in ntoks]
    seg = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    first = np.cumsum([0] + counts[:-1])
    q0 = (np.arange(seg.size, dtype=np.int64) - np.repeat(first, counts)) * qtile
    return np.stack([seg, q0.astype(np.int32)], axis=1)


def segment_records(grids):
    """The sais_vit_seg records of frames with patch grids [(gh, gw), ...] stacked in that order (tap offsets unset: 0)."""
    rec = np.zeros(len(grids), dtype=SEG_DTYPE)
    row = pix = 0
    for s, (gh, gw) in enumerate(grids):
        ntok = 1 + gh * gw
        rec[s] = (row, ntok, gh, gw, pix, 0, 0)
        row, pix = row + ntok, pix + 3 * PATCH * PATCH * gh * gw
    return rec


class SegPlan:
    """One pass over frames with patch grids `grids` [(gh, gw), ...] (frames of equal shape are separate segments)."""

    def __init__(self, grids):
        grids = [(int(a), int(b)) for a, b in grids]
        if not 1 <= len(grids) <= MAX_SEGMENTS:
            raise ValueError(f"a pass takes 1 .. {MAX_SEGMENTS} frames, got {len(grids)}")
        for gh, gw in grids:
            if gh < 1 or gw < 1 or 1 + gh * gw > MAX_TOKENS:
                raise ValueError(f"a {gh} x {gw} patch grid is {1 + gh * gw} tokens; at most {MAX_TOKENS}")
        self.grids, self.nseg = grids, len(grids)
        self.segs = segment_records(grids)
        self.ntoks = [int(n) for n in self.segs["ntok"]]
        self.M = int(self.segs["row0"][-1]) + self.ntoks[-1]
        self.NP = self.M - self.nseg
        self.npix = 3 * PATCH * PATCH * self.NP
        # tap matrices: one per distinct grid side of the pass; a 14 x 14 frame takes the table itself (:177-178)
        sides, off, ntaps = {}, {}, 0
        for gh, gw in grids:
            if (gh, gw) != (POS_SIDE, POS_SIDE):
                for n in (gh, gw):
                    if n not in sides:
                        sides[n], off[n] = axis_taps_f32(n), ntaps
                        ntaps += n * POS_SIDE
        for s, (gh, gw) in enumerate(grids):
            self.segs["tap_y"][s], self.segs["tap_x"][s] = (-1, -1) if (gh, gw) == (POS_SIDE, POS_SIDE) else (off[gh], off[gw])
        self.ntaps = ntaps
        self.qtile = attn_qtile(self.ntoks)
        self.tiles = tile_table(self.ntoks, self.qtile)
        # one host buffer: segments | tiles | taps (each part 16-B aligned)
        a16 = lambda n: (n + 15) // 16 * 16
        self._o_tiles = a16(self.segs.nbytes)
        self._o_taps = self._o_tiles + a16(self.tiles.nbytes)
        self.host = np.zeros(self._o_taps + a16(4 * ntaps), dtype=np.uint8)
        self.host[:self.segs.nbytes] = self.segs.view(np.uint8)
        self.host[self._o_tiles:self._o_tiles + self.tiles.nbytes] = self.tiles.reshape(-1).view(np.uint8)
        if sides:
            self.host[self._o_taps:self._o_taps + 4 * ntaps] = np.concatenate([m.reshape(-1) for m in sides.values()]).view(np.uint8)
        self.dev = None

    def to_device(self, device):
        """The one copy of the pass: host buffer -> pinned -> device."""
        self.dev = torch.from_numpy(self.host).pin_memory().to(device, non_blocking=True)
        return self

    # host / device pointers of the three parts
    def _h(self, off):
        return ctypes.c_void_p(self.host.ctypes.data + off)

    def _d(self, off):
        return ctypes.c_void_p(self.dev.data_ptr() + off)

    segs_host = property(lambda self: self._h(0))
    segs_dev = property(lambda self: self._d(0))
    tiles_host = property(lambda self: self._h(self._o_tiles))
    tiles_dev = property(lambda self: self._d(self._o_tiles))
    taps_dev = property(lambda self: self._d(self._o_taps) if self.ntaps else None)

    @property
    def ntiles(self):
        return self.tiles.shape[0]
