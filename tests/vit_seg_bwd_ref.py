"""Case lists and the host restatement for the BACKWARD of the segmented ViT pass (csrc/attn_seg.hip: sais_vit_attn_bwd_seg,
sais_vit_embed_bwd_seg): training on frames of different sizes in one pass.  numpy only, no GPU code.  Shared by
test_vit_seg_train_host.py and test_vit_seg_train_gpu.py; the segment layout, the tile table and the per-axis interpolation are
those of vit_seg_ref.py.

embed_bwd restates sais_vit_embed_bwd_seg in fp64, per segment through the two per-axis tap matrices (never the [hw, 196] map):
    dcls = dpos[0] = sum_s dx[row0_s],   dpos[1 + 14 a + b] = sum_s sum_y sum_x Ty_s[y][a] Tx_s[x][b] dx[row0_s + 1 + y gw + x]
and returns with it, per element of dpos, what an error bound needs: the NUMBER of non-zero terms and sum |Ty| |Tx| |dx|.
The bound of a sum of n terms accumulated one after the other in precision u (each product of the two taps rounded once, each of
the n partial sums rounded once, the total added to the value the buffer held and rounded once) is
    (n + 2) u sum |Ty Tx dx|  +  u |start|:
`bound(terms, mag, u, start)`.  Cutting the sum into runs that are added afterwards does not raise it: a run of n_k terms costs
n_k roundings of at most u sum_k, adding the r non-empty runs r - 1 more, and max n_k + r - 1 <= n.
"""
import numpy as np

import vit_seg_ref as R

U24, U53 = 2.0 ** -24, 2.0 ** -53

# ---------------------------------------------------------------------------------------------- case lists
# embedding backward: (frames, H, W) in one call: one patch, one row, one column, both axes interpolated, the table itself, and
# three frames of one shape
EMBED_FRAMES = ((1, 16, 16), (1, 16, 48), (1, 48, 16), (1, 80, 112), (1, 224, 224), (3, 32, 48))
# model at depth 2 under grad: (frames, H, W) per list item
MODEL_LIST = ((1, 32, 48), (2, 64, 64), (1, 224, 224), (1, 48, 112))
MODEL_BIG = ((30, 224, 224), (20, 176, 176))          # 30 x 197 + 20 x 122 = 8350 rows: the fused GEMM + LayerNorm form
# launch records: two lists of 41 stacked rows each (a record's tag may carry the row count), 2 shapes and 5 shapes
LAUNCH_2 = ((1, 32, 48), (2, 64, 64))
LAUNCH_5 = ((1, 32, 48), (1, 64, 64), (1, 48, 16), (1, 16, 16), (1, 80, 32))


def grids_of(spec):
    """[(gh, gw)] per frame of a (frames, H, W) list, in list order"""
    return [(h // R.PATCH, w // R.PATCH) for f, h, w in spec for _ in range(f)]


def rows_of(spec):
    return sum(f * (1 + (h // R.PATCH) * (w // R.PATCH)) for f, h, w in spec)


# ---------------------------------------------------------------------------------------------- the restatement
def embed_bwd(dx, grids, axis=R.axis_matrix):
    """dx f64 [M, C] (token rows of the segments of `grids`, stacked) -> (dcls [C], dpos [197, C], terms int [197], mag [197, C]).
    axis(n) -> the [n, 14] tap matrix of a grid side (fp64 by default; pass the f32-rounded one to restate the kernel's inputs)."""
    dx = np.asarray(dx, dtype=np.float64)
    C, S = dx.shape[1], R.POS_SIDE
    dpos, mag, terms = np.zeros((1 + S * S, C)), np.zeros((1 + S * S, C)), np.zeros(1 + S * S, dtype=np.int64)
    for row0, ntok, gh, gw, _ in R.layout(grids):
        dpos[0] += dx[row0]
        mag[0] += np.abs(dx[row0])
        terms[0] += 1
        g = dx[row0 + 1:row0 + ntok].reshape(gh, gw, C)
        if (gh, gw) == (S, S):                                  # the table itself: weight one
            ty = tx = np.eye(S)
        else:
            ty, tx = np.asarray(axis(gh), dtype=np.float64), np.asarray(axis(gw), dtype=np.float64)
        # out[a][b] = sum_y sum_x ty[y][a] tx[x][b] g[y][x]: over y first, then over x
        dpos[1:] += np.einsum("xb,axc->abc", tx, np.tensordot(ty.T, g, axes=1)).reshape(S * S, C)
        mag[1:] += np.einsum("xb,axc->abc", np.abs(tx), np.tensordot(np.abs(ty).T, np.abs(g), axes=1)).reshape(S * S, C)
        terms[1:] += np.outer(np.count_nonzero(ty, axis=0), np.count_nonzero(tx, axis=0)).reshape(-1)
    return dpos[0].copy(), dpos, terms, mag


def bound(terms, mag, u, start=None):
    """per element: (terms + 2) u mag + u |start| (see the module docstring); terms [197] or scalar, mag [197, C]"""
    b = (np.asarray(terms, dtype=np.float64).reshape(-1, 1) + 2) * u * mag
    return b if start is None else b + u * np.abs(start)


def patch_rows(grids):
    """the stacked-row index of every patch row, in segment order (what dpatch holds)"""
    return np.concatenate([np.arange(row0 + 1, row0 + ntok) for row0, ntok, *_ in R.layout(grids)])


def through_the_map(dx, grids):
    """the same gradient through the transposed [hw, 196] bicubic map per frame (autograd of interpolate_pos_encoding, what the
    resolution-group pass does): dpos [197, C] in fp64"""
    from sais_amd.vit import pos_interp_matrix
    dx = np.asarray(dx, dtype=np.float64)
    dpos = np.zeros((1 + R.POS_SIDE ** 2, dx.shape[1]))
    for row0, ntok, gh, gw, _ in R.layout(grids):
        dpos[0] += dx[row0]
        rows = dx[row0 + 1:row0 + ntok]
        dpos[1:] += rows if (gh, gw) == (R.POS_SIDE, R.POS_SIDE) else pos_interp_matrix(R.POS_SIDE, 16 * gh, 16 * gw).T @ rows
    return dpos


# ---------------------------------------------------------------------------------------------- restated mistakes
def embed_bwd_swapped(dx, grids):
    """gh and gw swapped when the patch rows of a segment are read as a grid"""
    dx = np.asarray(dx, dtype=np.float64)
    dpos = np.zeros((1 + R.POS_SIDE ** 2, dx.shape[1]))
    for row0, ntok, gh, gw, _ in R.layout(grids):
        dpos += embed_bwd(dx[row0:row0 + ntok], [(gw, gh)])[1]
    return dpos


def embed_bwd_cls_as_patch(dx, grids):
    """the CLS row counted as the first patch row (rows row0 .. row0 + hw - 1 instead of row0 + 1 .. row0 + hw)"""
    dx = np.asarray(dx, dtype=np.float64)
    dpos = np.zeros((1 + R.POS_SIDE ** 2, dx.shape[1]))
    for row0, ntok, gh, gw, _ in R.layout(grids):
        seg = dx[row0:row0 + ntok]
        dpos += embed_bwd(np.concatenate([seg[:1], seg[:-1]]), [(gh, gw)])[1]
    return dpos


def embed_bwd_drops_last(dx, grids):
    """the last segment left out of the sum"""
    if len(grids) == 1:
        return np.zeros((1 + R.POS_SIDE ** 2, np.asarray(dx).shape[1]))
    last = R.layout(grids)[-1][0]
    return embed_bwd(np.asarray(dx)[:last], grids[:-1])[1]
