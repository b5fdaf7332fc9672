"""Case lists and host restatements for the segmented ViT pass (csrc/attn_seg.hip, sais_amd/vit_seg.py): frames of different
sizes as segments of one stack of token rows.  Plain loops, numpy only, no GPU code: the tile table of the attention launch, the
per-axis positional interpolation in fp64, the segment layout.  Shared by test_vit_seg_host.py and test_vit_seg_gpu.py."""
import math

import numpy as np

NH, DM, PATCH, POS_SIDE = 6, 384, 16, 14
MAX_TOKENS = 4097
FEAT_REL = 2e-2             # the project's one feature bar: |got - ref| <= FEAT_REL * max|ref|

# ---------------------------------------------------------------------------------------------- case lists
# attention: token counts of one call (a lone pair, inside one key tile, both sides of 64, three tiles, the 224 x 224 count, a
# ragged 13th tile), in this order and in two permutations
ATTN_NTOKS = (2, 17, 63, 64, 65, 129, 197, 785)
ATTN_ORDERS = ((0, 1, 2, 3, 4, 5, 6, 7), (7, 0, 6, 1, 5, 2, 4, 3), (3, 4, 2, 7, 1, 0, 5, 6))
ATTN_MANY = (65,) * 90      # 90 x 2 x 6 = 1080 workgroups of 64 queries: above the 512 switch, the 64-query form
ATTN_CAP = (MAX_TOKENS,)    # one segment at the cap, alone
ATTN_LAYOUTS = ("rand", "planted", "offp", "offn", "same")      # the hard score layouts of tests/attn_ref.py the forward suites use
SENTINEL_ROWS = 128
# tile-table cases: the above and shapes of one multi_scale pass (token counts 4x apart)
TILE_CASES = (ATTN_NTOKS, ATTN_MANY, ATTN_CAP, (197, 101, 50), (2,), (32, 33, 64, 65, 4097, 2))
PATCHIFY_FRAMES = ((16, 16), (16, 48), (48, 16), (80, 112), (224, 224))     # (H, W) in one call
# model at depth 2: (frames, H, W) per list item
MODEL_LIST = ((1, 48, 80), (1, 224, 224), (2, 16, 16), (1, 160, 176), (1, 48, 80))
MODEL_BIG = ((46, 208, 240),)          # 46 x 196 = 9016 stacked rows: the fused GEMM + LayerNorm form (from 8192 on)
LAUNCH_3 = ((1, 32, 48), (1, 64, 64), (1, 48, 16))
LAUNCH_9 = LAUNCH_3 + ((1, 16, 16), (1, 80, 32), (1, 96, 64), (1, 32, 32), (1, 112, 48), (1, 16, 64))
MULTI_SCALE_SIZES = ((70, 100), (96, 64), (120, 90), (64, 64))              # (H, W) of four images, not multiples of 16
TOOL_SIZES = ((300, 200), (200, 300), (256, 256), (320, 180), (180, 320), (400, 250), (250, 400), (350, 350))    # (w, h) of the files


# ---------------------------------------------------------------------------------------------- restatements
def qtile(ntoks):
    """queries per workgroup: 64 iff the pass has >= 512 (head, 64-query tile) pairs, else 32"""
    n64 = 0
    for n in ntoks:
        n64 += (n + 63) // 64
    return 64 if NH * n64 >= 512 else 32


def tile_table(ntoks, qt):
    """[(segment, first query)] of every workgroup"""
    out = []
    for s, n in enumerate(ntoks):
        q = 0
        while q < n:
            out.append((s, q))
            q += qt
    return out


def coverage(tiles, ntoks, qt):
    """how often every query of every segment is owned by a tile: a list of int arrays (a correct table: all ones).  A tile
    outside its segment or off the qt grid raises."""
    cnt = [np.zeros(n, dtype=np.int64) for n in ntoks]
    for s, q0 in tiles:
        s, q0 = int(s), int(q0)
        if not 0 <= s < len(ntoks) or q0 % qt or not 0 <= q0 < ntoks[s]:
            raise ValueError(f"tile ({s}, {q0}) is not a tile of the pass")
        cnt[s][q0:q0 + qt] += 1
    return cnt


def covers_once(tiles, ntoks, qt):
    try:
        return all((c == 1).all() for c in coverage(tiles, ntoks, qt))
    except ValueError:
        return False


def layout(grids):
    """per frame (row0, ntok, gh, gw, pixel offset): token rows and packed [3, 16 gh, 16 gw] pixels, stacked in order"""
    out, row, pix = [], 0, 0
    for gh, gw in grids:
        ntok = 1 + gh * gw
        out.append((row, ntok, gh, gw, pix))
        row += ntok
        pix += 3 * (PATCH * gh) * (PATCH * gw)
    return out


def cubic(x, A=-0.75):
    x = abs(x)
    if x <= 1:
        return ((A + 2) * x - (A + 3)) * x * x + 1
    if x < 2:
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return 0.0


def axis_matrix(n0, side=POS_SIDE):
    """interpolate_pos_encoding along one axis in fp64, [n0, side]: bicubic, align_corners=False, scale (n0 + 0.1) / side, taps
    clamped at the border"""
    scale = (n0 + 0.1) / side
    assert int(math.floor(side * scale)) == n0
    M = np.zeros((n0, side))
    for i in range(n0):
        x = (i + 0.5) / scale - 0.5
        x0 = math.floor(x)
        for k in range(-1, 3):
            M[i, min(max(x0 + k, 0), side - 1)] += cubic(x - (x0 + k))
    return M


def pos_rows(pos, gh, gw):
    """fp64 positional rows [gh gw, 384] of a gh x gw grid from pos f64 [197, 384] (row 0 = CLS), and sum |m| |p| per element;
    a 14 x 14 grid takes the table itself"""
    p = np.asarray(pos, dtype=np.float64)[1:]
    if (gh, gw) == (POS_SIDE, POS_SIDE):
        return p.copy(), np.abs(p)
    m = np.kron(axis_matrix(gh), axis_matrix(gw))
    return m @ p, np.abs(m) @ np.abs(p)


# ---------------------------------------------------------------------------------------------- restated mistakes
def tile_table_drops_partial(ntoks, qt):
    """forgets the last partial tile of a segment (floor instead of ceil)"""
    return [(s, q) for s, n in enumerate(ntoks) for q in range(0, n - qt + 1, qt)]


def tile_table_padded(ntoks, qt):
    """a grid padded to the longest segment"""
    longest = max(ntoks)
    return [(s, q) for s in range(len(ntoks)) for q in range(0, longest, qt)]


def layout_swapped(grids):
    """gh and gw swapped in the record"""
    return [(r, n, gw, gh, p) for r, n, gh, gw, p in layout(grids)]


def layout_no_cls(grids):
    """row offsets that forget the CLS row of every frame"""
    out, row = [], 0
    for r, n, gh, gw, p in layout(grids):
        out.append((row, n, gh, gw, p))
        row += n - 1
    return out
