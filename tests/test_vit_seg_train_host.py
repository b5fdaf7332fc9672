"""CPU-only half of the tests of TRAINING on frames of different sizes in one pass: the argument checks of the new library
entries through ctypes (nothing is launched), the fp64 restatement of sais_vit_embed_bwd_seg (tests/vit_seg_bwd_ref.py) against
the transposed bicubic map on every grid 1 .. 64 x 1 .. 64 with its own computed bound, that restated mistakes are caught, and the
MultiCropWrapper.segmented switch."""
import ctypes
import os

import numpy as np
import pytest

import vit_seg_bwd_ref as B
import vit_seg_ref as R


def _lib_loaded():
    import __graft_entry__ as ge
    from sais_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------- the C entries, no GPU
def test_bad_arguments_are_refused_without_a_gpu():
    from sais_amd import vit_seg as V
    lib = _lib_loaded()
    P = ctypes.c_void_p(4096)                                  # never dereferenced: every call below is refused before a launch
    plan = V.SegPlan([(3, 5), (14, 14), (1, 1)])
    M = plan.M
    WS = lib.sais_vit_attn_bwd_seg_workspace_bytes(M)
    assert WS == 24 * M and lib.sais_vit_attn_bwd_seg_workspace_bytes(0) == 0 == lib.sais_vit_attn_bwd_seg_workspace_bytes(-3)

    def table(**edit):
        segs = plan.segs.copy()
        for k, (i, v) in edit.items():
            segs[k][i] = v
        return segs

    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)

    def attn(qkv=P, ldq=1152, dout=P, lddo=384, out=P, ldout=384, lse=P, rows=M, segs=plan.segs_host, dsegs=P, nseg=plan.nseg,
             tiles=plan.tiles_host, dtiles=P, ntiles=plan.ntiles, dqkv=P, lddq=1152, ws=P, ws_bytes=WS):
        return lib.sais_vit_attn_bwd_seg(qkv, ldq, dout, lddo, out, ldout, lse, rows, segs, dsegs, nseg, tiles, dtiles, ntiles, dqkv,
                                         lddq, ws, ws_bytes, None)

    off_grid, outside, wrong_seg = plan.tiles.copy(), plan.tiles.copy(), plan.tiles.copy()
    off_grid[0, 1] = 16                                        # off the 32-row grid
    outside[-1, 1] = 32                                        # past the two tokens of the last segment
    wrong_seg[0, 0] = 3                                        # a segment the table does not have
    keep = [table(ntok=(2, 1)), table(ntok=(1, 4098)), table(row0=(1, 0))]
    refused = [
        attn(segs=None), attn(dsegs=None), attn(tiles=None), attn(dtiles=None),                       # null tables
        attn(qkv=None), attn(dout=None), attn(out=None), attn(lse=None), attn(dqkv=None), attn(ws=None),
        attn(nseg=0), attn(nseg=65536), attn(nseg=-1),                                                # nseg out of range
        attn(segs=ptr(keep[0])), attn(segs=ptr(keep[1])), attn(segs=ptr(keep[2])),                    # ntok 1, 4098; overlap
        attn(tiles=ptr(off_grid)), attn(tiles=ptr(outside)), attn(tiles=ptr(wrong_seg)),              # a tile outside its segment
        attn(ntiles=plan.ntiles - 1), attn(ntiles=plan.ntiles + 1),                                   # not sum ceil(ntok / q)
        attn(ldq=1156), attn(ldq=1144), attn(lddo=388), attn(lddo=376), attn(ldout=388), attn(ldout=376), attn(lddq=1156),
        attn(lddq=1144),                                                                              # misaligned / short strides
        attn(dsegs=ctypes.c_void_p(4104)), attn(dtiles=ctypes.c_void_p(4100)), attn(rows=M - 1),
        attn(ws_bytes=WS - 1),                                                                        # one byte short
    ]
    assert refused == [-1] * len(refused), refused

    def embed(dx=P, rows=M, taps=P, ntaps=plan.ntaps, segs=plan.segs_host, dsegs=P, nseg=plan.nseg, dcls=P, dpos=P, dpatch=P):
        return lib.sais_vit_embed_bwd_seg(dx, rows, taps, ntaps, segs, dsegs, nseg, dcls, dpos, dpatch, None)

    t_gap, t_tap, t_self = table(row0=(1, 17)), table(tap_x=(0, plan.ntaps)), table(tap_y=(0, -1), tap_x=(0, -1))
    refused = [embed(dx=None), embed(dcls=None), embed(dpos=None), embed(dpatch=None), embed(segs=None), embed(dsegs=None),
               embed(taps=None), embed(ntaps=plan.ntaps - 1), embed(nseg=0), embed(nseg=65536), embed(rows=M - 1),
               embed(dx=ctypes.c_void_p(4100)), embed(dpos=ctypes.c_void_p(4104)), embed(dpatch=ctypes.c_void_p(4098)),
               embed(segs=ptr(t_gap)),                         # a gap in the stack (dense)
               embed(segs=ptr(t_tap)),                         # a tap matrix outside the buffer
               embed(segs=ptr(t_self))]                        # "the table itself" off the 14 x 14 grid
    assert refused == [-1] * len(refused), refused

    def scatter(src=P, segs=plan.segs_host, dsegs=P, nseg=plan.nseg, dst=P, ldd=384, rows=M):
        return lib.sais_vit_cls_scatter_seg(src, segs, dsegs, nseg, dst, ldd, rows, None)

    refused = [scatter(src=None), scatter(dst=None), scatter(segs=None), scatter(dsegs=None), scatter(nseg=0), scatter(nseg=65536),
               scatter(ldd=380), scatter(ldd=386), scatter(rows=M - 1), scatter(segs=ptr(keep[1])),
               scatter(dst=ctypes.c_void_p(4100))]
    assert refused == [-1] * len(refused), refused

    def expand(src=P, nb=4, segs=plan.segs_host, dsegs=P, nseg=plan.nseg, out=P, rows=M):
        return lib.sais_vit_rows_expand_seg(src, nb, segs, dsegs, nseg, out, rows, None)

    refused = [expand(src=None), expand(out=None), expand(segs=None), expand(dsegs=None), expand(nb=0), expand(nseg=0),
               expand(rows=M - 1), expand(rows=M + 1), expand(segs=ptr(t_gap))]
    assert refused == [-1] * len(refused), refused


# ---------------------------------------------------------------------------------------------- the restatement
def _dx(grids, seed, C=3):
    M = R.layout(grids)[-1][0] + R.layout(grids)[-1][1]
    return np.random.default_rng(seed).standard_normal((M, C))


def test_restatement_equals_the_transposed_bicubic_map_on_every_grid():
    """grids 1 .. 64 on both axes (14 x 14 included): the per-axis form against pos_interp_matrix(14, H, W).T @ rows within 1e-12
    and within the two forms' own fp64 bounds (each (terms + 2) 2^-53 sum |Ty Tx dx|)"""
    worst = 0.0
    for gh in range(1, 65):
        for gw in range(1, 65):
            dx = _dx([(gh, gw)], 1000 * gh + gw)
            dcls, dpos, terms, mag = B.embed_bwd(dx, [(gh, gw)])
            want = B.through_the_map(dx, [(gh, gw)])
            err = np.abs(dpos - want)
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-12, (gh, gw, err.max())
            assert (err <= 2 * B.bound(terms, mag, B.U53) + 1e-300).all(), (gh, gw)
            assert np.array_equal(dcls, dx[0]) and np.array_equal(dpos[0], dx[0]) and terms[0] == 1
            assert terms[1:].max() <= gh * gw and terms[1:].sum() <= 16 * gh * gw           # at most 4 x 4 taps per patch
            if (gh, gw) == (14, 14):
                assert np.array_equal(dpos[1:], dx[1:]) and (terms[1:] == 1).all()
    print(f"per-axis form vs the transposed map, worst |d| = {worst:.3e}")


def test_restatement_on_the_case_list_and_its_bound():
    grids = B.grids_of(B.EMBED_FRAMES)
    dx = _dx(grids, 7, C=5)
    dcls, dpos, terms, mag = B.embed_bwd(dx, grids)
    want = B.through_the_map(dx, grids)
    assert np.abs(dpos - want).max() <= 1e-12
    assert np.array_equal(dcls, dpos[0]) and terms[0] == len(grids) == 8
    assert (terms[1:] >= 1).all()                                      # the 14 x 14 frame reaches every row of the table
    assert (mag >= np.abs(dpos) - 1e-12).all()
    # the f32 bound of the kernel is far above fp64 noise and far below the values: the GPU test can tell a wrong sum from rounding
    b32 = B.bound(terms, mag, B.U24)
    assert b32.max() < 1e-3 * np.abs(dpos).max() and b32.min() > 1e3 * B.bound(terms, mag, B.U53).min()
    assert B.patch_rows(grids).size == dx.shape[0] - len(grids)


@pytest.mark.parametrize("mistake", ["swapped", "cls_as_patch", "drops_last"])
def test_the_case_list_catches_restated_mistakes(mistake):
    """each mistake leaves the f32 bound of the device test by orders of magnitude on the device test's own list"""
    grids = B.grids_of(B.EMBED_FRAMES)
    dx = _dx(grids, 8, C=5)
    _, dpos, terms, mag = B.embed_bwd(dx, grids)
    wrong = getattr(B, "embed_bwd_" + mistake)(dx, grids)
    ratio = np.abs(wrong - dpos) / B.bound(terms, mag, B.U24)
    assert ratio.max() > 1e3, (mistake, ratio.max())
    if mistake == "swapped":                                            # square frames alone would not see it
        square = [(3, 3), (14, 14)]
        d2 = _dx(square, 9)
        assert np.abs(B.embed_bwd_swapped(d2, square) - B.embed_bwd(d2, square)[1]).max() <= 1e-12


def test_case_lists():
    from sais_amd import ops  # noqa: F401  (importable without a GPU)
    assert B.rows_of(B.MODEL_BIG) == 8350 and B.rows_of(B.MODEL_LIST) < 8192
    assert len({(h, w) for _, h, w in B.LAUNCH_2}) == 2 and len({(h, w) for _, h, w in B.LAUNCH_5}) == 5
    assert B.rows_of(B.LAUNCH_2) == B.rows_of(B.LAUNCH_5) == 41


# ---------------------------------------------------------------------------------------------- the switch
def _wrapper():
    from sais_amd import dino, vit
    return dino.MultiCropWrapper(vit.vit_small(patch_size=16, depth=1), dino.DINOHead(384, 1024))


def test_segmented_switch_and_the_graphed_step_refusal(monkeypatch):
    from sais_amd import dino
    monkeypatch.delenv("SAIS_DINO_SEGMENTED", raising=False)
    assert _wrapper().segmented is False
    monkeypatch.setenv("SAIS_DINO_SEGMENTED", "0")
    assert _wrapper().segmented is False
    monkeypatch.setenv("SAIS_DINO_SEGMENTED", "1")
    student = _wrapper()
    assert student.segmented is True
    with pytest.raises(NotImplementedError) as e:
        dino.GraphedTrainStep(student, _wrapper(), None, None, [])
    assert "segmented" in str(e.value) and ". " not in str(e.value)                # one sentence
    student.segmented = False
    step = dino.GraphedTrainStep(student, _wrapper(), None, None, [])
    student.segmented = True                                                       # set after construction: refused at capture
    with pytest.raises(NotImplementedError):
        step._capture(0)
