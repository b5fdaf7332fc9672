"""CPU-only half of the segmented-pass tests (frames of different sizes in one backbone pass): the host tables of
sais_amd/vit_seg.py against the plain restatements of tests/vit_seg_ref.py, the argument checks of the new library entries
(nothing is launched), the --mixed_batch flag of eval_image_retrieval.py, and that the case lists catch restated mistakes."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import vit_seg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grids(ntoks):
    """a patch grid per token count (1 x (n - 1): the attention reads the count only)"""
    return [(1, n - 1) for n in ntoks]


# ---------------------------------------------------------------------------------------------- tile table
@pytest.mark.parametrize("case", range(len(R.TILE_CASES)))
def test_tile_table_covers_every_query_once(case):
    from sais_amd import vit_seg as V
    ntoks = list(R.TILE_CASES[case])
    rng = np.random.default_rng(case)
    for order in [np.arange(len(ntoks)), rng.permutation(len(ntoks)), rng.permutation(len(ntoks))]:
        n = [ntoks[i] for i in order]
        for qt in (32, 64):                                    # both workgroup forms, whatever the rule would pick
            t = V.tile_table(n, qt)
            assert t.dtype == np.int32 and t.shape == (sum((k + qt - 1) // qt for k in n), 2)
            assert R.covers_once(t, n, qt)
            assert [tuple(r) for r in t.tolist()] == R.tile_table(n, qt)
        assert V.attn_qtile(n) == R.qtile(n)
        plan = V.SegPlan(_grids(n))
        assert plan.qtile == R.qtile(n) and R.covers_once(plan.tiles, n, plan.qtile) and plan.ntiles == len(plan.tiles)


def test_the_workgroup_form_switches_at_512_tiles():
    assert R.qtile(R.ATTN_NTOKS) == 32 and R.qtile(R.ATTN_MANY) == 64 and R.qtile(R.ATTN_CAP) == 32
    assert R.qtile((64,) * 85) == 32 and R.qtile((64,) * 86) == 64          # 6 x 85 = 510, 6 x 86 = 516
    from sais_amd import _lib, vit_seg as V
    lib = _lib_loaded()
    for ntoks in (R.ATTN_NTOKS, R.ATTN_MANY, R.ATTN_CAP, (64,) * 85, (64,) * 86):
        plan = V.SegPlan(_grids(ntoks))
        assert lib.sais_vit_seg_qtile(plan.segs_host, plan.nseg) == R.qtile(ntoks) == plan.qtile


# ---------------------------------------------------------------------------------------------- interpolation
def test_axis_matrices_multiply_out_to_the_bicubic_map():
    """grids 1 .. 64 on both axes: kron(axis(gh), axis(gw)) is pos_interp_matrix(14, H, W) within 1e-12, with the product's
    f64 matrices and with the restatement's"""
    from sais_amd.vit import pos_axis_matrix, pos_interp_matrix
    ours = {n: pos_axis_matrix(14, n) for n in range(1, 65)}
    ref = {n: R.axis_matrix(n) for n in range(1, 65)}
    worst = 0.0
    for n in range(1, 65):
        assert ours[n].shape == (n, 14)
        worst = max(worst, float(np.abs(ours[n] - ref[n]).max()))
        assert np.abs(ours[n].sum(1) - 1).max() <= 1e-12               # the taps of a sample sum to one
        assert (np.count_nonzero(ours[n], axis=1) <= 4).all()
    assert worst <= 1e-12
    for gh in range(1, 65):
        for gw in range(1, 65):
            K = pos_interp_matrix(14, 16 * gh, 16 * gw)
            assert K.shape == (gh * gw, 196)
            assert np.abs(np.kron(ref[gh], ref[gw]) - K).max() <= 1e-12, (gh, gw)


def test_tap_matrices_are_cached_per_grid_side():
    from sais_amd import vit_seg as V
    a = V.axis_taps_f32(23)
    assert a is V.axis_taps_f32(23) and a.dtype == np.float32 and a.shape == (23, 14)
    plan = V.SegPlan([(23, 5), (5, 23), (23, 23), (14, 14), (5, 5)])
    assert plan.ntaps == 14 * (23 + 5)                                 # two sides, five shapes
    s = plan.segs
    assert (s["tap_y"][0], s["tap_x"][0]) == (s["tap_x"][1], s["tap_y"][1]) == (s["tap_y"][2], s["tap_x"][4])
    assert (s["tap_y"][3], s["tap_x"][3]) == (-1, -1)                  # 14 x 14: the table itself
    taps = plan.host[plan._o_taps:plan._o_taps + 4 * plan.ntaps].view(np.float32)
    assert np.array_equal(taps[s["tap_y"][0]:s["tap_y"][0] + 23 * 14].reshape(23, 14), a)


# ---------------------------------------------------------------------------------------------- layout
def test_segment_records_match_the_restated_layout():
    from sais_amd import vit_seg as V
    grids = [(3, 5), (14, 14), (1, 1), (1, 1), (10, 11), (3, 5), (64, 64)]
    plan = V.SegPlan(grids)
    want = R.layout(grids)
    got = [tuple(int(plan.segs[k][i]) for k in ("row0", "ntok", "gh", "gw", "pix")) for i in range(len(grids))]
    assert got == want
    assert plan.M == want[-1][0] + want[-1][1] and plan.NP == plan.M - len(grids) and plan.npix == 768 * plan.NP
    assert plan.host[:32 * len(grids)].tobytes() == plan.segs.tobytes()
    with pytest.raises(ValueError):
        V.SegPlan([])
    with pytest.raises(ValueError):
        V.SegPlan([(64, 65)])                                           # 4161 tokens


# ---------------------------------------------------------------------------------------------- the lists catch mistakes
@pytest.mark.parametrize("mistake", ["drops_partial", "padded", "swapped", "no_cls"])
def test_the_list_catches_restated_mistakes(mistake):
    if mistake in ("drops_partial", "padded"):
        wrong = getattr(R, "tile_table_" + mistake)
        caught = [c for c in R.TILE_CASES for qt in (32, 64) if not R.covers_once(wrong(list(c), qt), list(c), qt)]
        assert len(caught) >= 3, (mistake, caught)                     # not one lucky case
        assert any(c == R.ATTN_NTOKS for c in caught)
        return
    from sais_amd import vit_seg as V
    wrong = getattr(R, "layout_" + mistake)
    lists = [[(h // 16, w // 16) for f, h, w in lst for _ in range(f)] for lst in (R.MODEL_LIST, R.LAUNCH_9)]
    lists.append([(h // 16, w // 16) for h, w in R.PATCHIFY_FRAMES])
    for grids in lists:
        plan = V.SegPlan(grids)
        got = [tuple(int(plan.segs[k][i]) for k in ("row0", "ntok", "gh", "gw", "pix")) for i in range(len(grids))]
        assert got == R.layout(grids) and got != wrong(grids), (mistake, grids)


# ---------------------------------------------------------------------------------------------- the C entries, no GPU
def _lib_loaded():
    import __graft_entry__ as ge
    from sais_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_bad_arguments_are_refused_without_a_gpu():
    from sais_amd import vit_seg as V
    lib = _lib_loaded()
    P = ctypes.c_void_p(4096)                                  # never dereferenced: every call below is refused before a launch
    grids = [(3, 5), (14, 14), (1, 1)]
    plan = V.SegPlan(grids)
    M = plan.M

    def table(**edit):
        """a host copy of the table with one field of one record changed"""
        segs = plan.segs.copy()
        for k, (i, v) in edit.items():
            segs[k][i] = v
        return segs, ctypes.c_void_p(segs.ctypes.data)

    def attn(qkv=P, ldq=1152, rows=M, segs=plan.segs_host, dsegs=P, nseg=plan.nseg, tiles=plan.tiles_host, dtiles=P,
             ntiles=plan.ntiles, out=P, ldo=384, lse=None):
        return lib.sais_vit_attn_fwd_seg(qkv, ldq, rows, segs, dsegs, nseg, tiles, dtiles, ntiles, out, ldo, lse, None)

    bad_tiles = plan.tiles.copy()
    bad_tiles[0, 1] = 16                                       # off the 32-query grid
    far_tiles = plan.tiles.copy()
    far_tiles[-1, 1] = 32                                      # past the two tokens of the last segment
    keep = [table(ntok=(2, 1))[0], table(ntok=(1, 4098))[0], table(row0=(1, 0))[0]]
    refused = [
        attn(segs=None), attn(dsegs=None), attn(tiles=None), attn(dtiles=None), attn(qkv=None), attn(out=None),
        attn(nseg=0), attn(nseg=65536), attn(nseg=-1),
        attn(segs=ctypes.c_void_p(keep[0].ctypes.data)),       # ntok 1
        attn(segs=ctypes.c_void_p(keep[1].ctypes.data)),       # ntok 4098
        attn(segs=ctypes.c_void_p(keep[2].ctypes.data)),       # overlapping rows
        attn(ldq=1156), attn(ldq=1144), attn(ldo=386), attn(ldo=380), attn(rows=M - 1),
        attn(dsegs=ctypes.c_void_p(4104)), attn(dtiles=ctypes.c_void_p(4100)),
        attn(ntiles=plan.ntiles - 1), attn(ntiles=plan.ntiles + 1),
        attn(tiles=ctypes.c_void_p(bad_tiles.ctypes.data)), attn(tiles=ctypes.c_void_p(far_tiles.ctypes.data)),
    ]
    assert refused == [-1] * len(refused), refused
    assert lib.sais_vit_seg_qtile(None, 3) == -1 and lib.sais_vit_seg_qtile(plan.segs_host, 0) == -1
    assert lib.sais_vit_seg_qtile(ctypes.c_void_p(keep[1].ctypes.data), 3) == -1

    def patchify(pix=P, npix=plan.npix, segs=plan.segs_host, dsegs=P, nseg=plan.nseg, out=P):
        return lib.sais_patchify_seg(pix, npix, segs, dsegs, nseg, out, None)

    t_pix, t_gap, t_grid = table(pix=(1, 2))[0], table(row0=(1, 17))[0], table(gw=(0, 4))[0]
    refused = [patchify(pix=None), patchify(out=None), patchify(segs=None), patchify(dsegs=None), patchify(nseg=0),
               patchify(nseg=65536), patchify(npix=plan.npix - 1), patchify(pix=ctypes.c_void_p(4100)),
               patchify(segs=ctypes.c_void_p(t_pix.ctypes.data)),       # pixel offset not a multiple of 4
               patchify(segs=ctypes.c_void_p(t_gap.ctypes.data)),       # a gap in the stack
               patchify(segs=ctypes.c_void_p(t_grid.ctypes.data))]      # ntok != 1 + gh gw
    assert refused == [-1] * len(refused), refused

    def embed(pe=P, cls=P, pos=P, taps=P, ntaps=plan.ntaps, segs=plan.segs_host, dsegs=P, nseg=plan.nseg, x=P, rows=M):
        return lib.sais_vit_embed_seg(pe, cls, pos, taps, ntaps, segs, dsegs, nseg, x, rows, None)

    t_tap, t_self = table(tap_x=(0, plan.ntaps))[0], table(tap_y=(0, -1), tap_x=(0, -1))[0]
    refused = [embed(pe=None), embed(cls=None), embed(pos=None), embed(x=None), embed(segs=None), embed(dsegs=None),
               embed(taps=None), embed(ntaps=plan.ntaps - 1), embed(nseg=0), embed(rows=M - 1), embed(x=ctypes.c_void_p(4100)),
               embed(segs=ctypes.c_void_p(t_tap.ctypes.data)),          # a tap matrix outside the buffer
               embed(segs=ctypes.c_void_p(t_self.ctypes.data)),         # "the table itself" off the 14 x 14 grid
               embed(segs=ctypes.c_void_p(t_gap.ctypes.data))]
    assert refused == [-1] * len(refused), refused

    def gather(x=P, ldx=384, rows=M, segs=plan.segs_host, dsegs=P, nseg=plan.nseg, out=P):
        return lib.sais_vit_cls_gather_seg(x, ldx, rows, segs, dsegs, nseg, out, None)

    refused = [gather(x=None), gather(out=None), gather(segs=None), gather(dsegs=None), gather(nseg=0), gather(nseg=65536),
               gather(ldx=380), gather(ldx=386), gather(rows=M - 1), gather(segs=ctypes.c_void_p(keep[1].ctypes.data))]
    assert refused == [-1] * len(refused), refused


# ---------------------------------------------------------------------------------------------- the tool's flag
def _tool():
    path = os.path.join(ROOT, "SAIS", "scripts", "dino-main", "eval_image_retrieval.py")
    spec = importlib.util.spec_from_file_location("eval_image_retrieval_seg", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mixed_batch_flag_and_its_two_exits():
    tool = _tool()
    p = tool.get_args_parser()
    assert p.parse_args([]).mixed_batch is False                        # with all defaults the tool is the parent's
    assert p.parse_args(["--mixed_batch", "true"]).mixed_batch is True
    assert p.parse_args(["--mixed_batch", "false", "--group_shapes", "true"]).group_shapes is True
    with pytest.raises(SystemExit) as e:
        tool.main(["--mixed_batch", "true"])
    assert "--mixed_batch true needs --gpu_loader true" in str(e.value.code) and str(e.value.code).count(".") == 0
    with pytest.raises(SystemExit) as e:
        tool.main(["--mixed_batch", "true", "--gpu_loader", "true", "--group_shapes", "true"])
    assert "exclude each other" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        tool.main(["--mixed_batch", "true", "--gpu_loader", "true", "--patch_size", "8"])
    assert "--patch_size 16 only" in str(e.value.code)


def test_thumbnail_batches_mixed_yields_one_list_per_loader_batch():
    import torch
    from sais_amd import retrieval

    class Loader(list):
        dataset = list(range(5))

    class Thumbs:
        def thumbnail(self, items, imsize):
            return [torch.zeros(1, 3, 16 + 16 * i, 32) for i in items]

    loader = Loader([([0, 1, 2], torch.tensor([0, 1, 2])), ([3, 4], torch.tensor([3, 4]))])
    got = list(retrieval.ThumbnailBatches(loader, Thumbs(), 64, mixed=True))
    assert [len(t) for t, _ in got] == [3, 2] and [i.tolist() for _, i in got] == [[0, 1, 2], [3, 4]]
    assert [tuple(t.shape) for t in got[1][0]] == [(1, 3, 64, 32), (1, 3, 80, 32)]
    with pytest.raises(ValueError):
        retrieval.ThumbnailBatches(loader, Thumbs(), 64, group_shapes=True, mixed=True)
    assert len(list(retrieval.ThumbnailBatches(loader, Thumbs(), 64))) == 5          # the default: one image per item
