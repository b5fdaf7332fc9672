"""The host plan of the frame preprocessing (`sais_preprocess_plan_describe`, the geometry half of plan_create) against the
plain-Python restatement of tests/preprocess_ref.py, and proof that the case table of test_preprocess_edges_gpu.py reaches
every horizontal arm, every band height and every boundary of the plan.  No GPU: describe makes no device call."""
import ctypes

import numpy as np
import pytest

import preprocess_ref as R
from oracle import preprocess_oracle as po

FRACTIONS = [(0.8, 0.8), (0.8, 0.7), (1.0, 1.0)]


def lib_describe(H, W, hf, wf):
    from sais_amd import _lib
    info = (ctypes.c_int * 10)(*([-7] * 10))
    rc = _lib.load().sais_preprocess_plan_describe(H, W, hf, wf, ctypes.cast(info, ctypes.c_void_p))
    assert rc in (0, -1), rc
    if rc:
        assert list(info) == [-7] * 10, "a refusal wrote into info"
        return None
    return tuple(info)


def lib_vfirst(cw, ch):
    from sais_amd import _lib
    return bool(_lib.load().sais_preprocess_vertical_first(cw, ch))


def check(H, W, hf, wf):
    want = R.describe(H, W, hf, wf)
    assert lib_describe(H, W, hf, wf) == want, (H, W, hf, wf, dict(zip(R.FIELDS, want or ())))
    return want


def frame_extent_for(crop, frac):
    """frame extents whose crop extent at `frac` is `crop` (none, one or two of them)"""
    n0 = int(round(crop / frac))
    return [n for n in range(max(1, n0 - 2), n0 + 3) if (R.crop_box(n, 8, frac, 1.0) or (0, 0, 0, -1))[3] == crop]


@pytest.mark.parametrize("hf,wf", FRACTIONS)
def test_describe_equals_the_restatement_at_small_sizes(hf, wf):
    for n in range(1, 401):
        check(n, 8, hf, wf)
        check(8, n, hf, wf)


@pytest.mark.parametrize("hf,wf", FRACTIONS)
def test_describe_equals_the_restatement_around_every_switch_over(hf, wf):
    switches, refused = R.band_switches()
    seen_bands, seen_refusal = set(), False
    for ch0 in [s[0] for s in switches] + [refused]:
        for ch in range(ch0 - 3, ch0 + 4):
            for H in frame_extent_for(ch, hf):
                got = check(H, 8, hf, wf)
                seen_refusal |= got is None
                if got:
                    assert got[3] == ch
                    seen_bands.add(got[6])
    assert seen_bands == {8, 4, 2, 1} and seen_refusal
    arms = set()
    for cw0, _ in R.arm_switches()[1:]:
        for cw in range(cw0 - 1, cw0 + 2):
            for W in frame_extent_for(cw, wf):
                got = check(8, W, hf, wf)
                assert got[2] == cw
                arms.add(R.arm(got[4]))
    assert arms == set(range(1, 10))


def test_refusals_return_the_codes_of_create():
    from sais_amd import _lib
    lib = _lib.load()
    info = (ctypes.c_int * 10)()
    p = ctypes.cast(info, ctypes.c_void_p)
    for args in ((0, 8, 0.8, 0.8), (8, 0, 0.8, 0.8), (-1, 8, 0.8, 0.8), (8, 8, 0.0, 0.8), (8, 8, 0.8, 1.5), (8, 8, float("nan"), 0.8),
                 (1, 8, 0.3, 0.8), (8, 1, 0.8, 0.4)):                  # the last two: a box that rounds to nothing
        assert lib.sais_preprocess_plan_describe(*args, p) == -1, args
    assert lib.sais_preprocess_plan_describe(8, 8, 0.8, 0.8, None) == -1
    _, refused = R.band_switches()
    assert lib.sais_preprocess_plan_describe(refused, 8, 1.0, 1.0, p) == -1
    assert lib.sais_preprocess_plan_describe(refused - 1, 8, 1.0, 1.0, p) == 0


def test_box_equals_the_oracle_including_exact_ties():
    sizes = [(h, w) for h in range(1, 130) for w in (1, 2, 5, 15, 45, 640)]
    sizes += [(h, 25) for h in range(5, 2000, 10)] + [(35, w) for w in range(5, 2000, 10)]     # (H - 0.8 H) / 2 = k + .5
    sizes += [(1080, 1920), (480, 854), (720, 1280), (1440, 2560), (2160, 3840)]
    ties = 0
    for hf, wf in FRACTIONS:
        for h, w in sizes:
            got = lib_describe(h, w, hf, wf)
            if got is None:
                assert R.crop_box(h, w, hf, wf) is None
                continue
            l, t, r, b = po.center_crop_box(w, h, hf, wf)
            assert (got[0], got[1], got[0] + got[2], got[1] + got[3]) == (l, t, r, b), (h, w, hf, wf)
            ties += hf == 0.8 and ((h - hf * h) / 2.) % 1 == 0.5
    assert ties >= 100                                                   # the tie sizes really are ties in double


def test_the_restated_switch_overs_are_the_documented_ones():
    """Written down from the restatement, so that a change of the thresholds (LDS budget, row bytes, tap grouping) shows."""
    assert R.arm_switches() == [(1, 1), (225, 2), (673, 3), (1121, 4), (1569, 5), (2017, 6), (2465, 7), (2913, 8), (3361, 9)]
    switches, refused = R.band_switches()
    assert switches[0] == (2143, 8, 4) and refused == 9634
    steps_up = [s for s in switches if s[2] > s[1]]                      # the band is not monotonic in the crop height
    assert (3856, 2, 4) in steps_up and (6424, 1, 2) in steps_up
    for ch, _, after in steps_up:
        assert R.band_plan(ch)[2] == 86, ch                             # max_rows lands exactly on the last row that fits
    assert 86 * R.ROW_BYTES + 16 + R.LUT_BYTES <= R.LDS_BUDGET < 87 * R.ROW_BYTES + 16 + R.LUT_BYTES


def test_every_arm_and_band_is_reached():
    """The GPU suite's case table, by `describe` of the library itself."""
    infos = {}
    for c in R.GPU_CASES:
        got = lib_describe(c.H, c.W, c.hf, c.wf)
        assert got is not None and got == tuple(c.info[k] for k in R.FIELDS), c
        infos[c.name] = dict(zip(R.FIELDS, got))
        infos[c.name]["vfirst"] = lib_vfirst(got[2], got[3])
        assert infos[c.name]["vfirst"] == c.info["vfirst"]
    hfirst = {n: i for n, i in infos.items() if not i["vfirst"]}           # the cases that run preprocess_kernel
    arms = {R.arm(i["kx"]) for i in hfirst.values()}
    assert arms == set(range(1, 10)), arms                               # G = 1..8 and the generic arm
    assert {i["band"] for i in hfirst.values()} == {8, 4, 2, 1}
    assert not any(i["vfirst"] for n, i in infos.items() if n.startswith("taps_"))
    # both sides of every arm switch-over, with W = cw
    for cw, a in R.arm_switches()[1:]:
        lo = [i for i in infos.values() if i["cw"] == cw - 1][0]
        hi = [i for i in infos.values() if i["cw"] == cw][0]
        assert (R.arm(lo["kx"]), R.arm(hi["kx"])) == (a - 1, a)
    assert any(i["cw"] >= 3809 for i in infos.values())
    assert R.arm(infos["taps_2560x16_at_0.8"]["kx"]) == 6 and R.arm(infos["taps_3840x16_at_0.8"]["kx"]) == 8
    # both sides of every band switch-over, the non-monotonic steps among them
    by_ch = {i["ch"]: i for n, i in hfirst.items() if n.startswith("band_")}
    tall = {i["ch"] for n, i in infos.items() if n.startswith("band_") and i["vfirst"]}
    assert tall == set(by_ch) and all(i["cw"] == 8 for n, i in infos.items() if n.startswith("band_") and i["vfirst"])
    switches, refused = R.band_switches()
    for ch, before, after in switches:
        assert (by_ch[ch - 1]["band"], by_ch[ch]["band"]) == (before, after), ch
    assert (by_ch[3855]["band"], by_ch[3856]["band"], by_ch[6423]["band"], by_ch[6424]["band"]) == (2, 4, 1, 2)
    # the last accepted crop height and the first refused one
    assert refused - 1 in by_ch and by_ch[refused - 1]["lds_bytes"] <= R.LDS_BUDGET
    rc = R.refused_case()
    assert rc.H == refused and lib_describe(rc.H, rc.W, rc.hf, rc.wf) is None
    assert all(c.H * c.W * 3 < 250_000 for c in R.BAND_CASES + [rc] if c.W == 8)
    assert all(c.H * c.W * 3 < 3_000_000 for c in R.BAND_CASES)
    # the byte-wise tail of load_dword, and a frame smaller than one dword
    assert {c.total_bytes % 4 for c in R.TAIL_CASES} == {1, 2, 3}
    assert any(c.total_bytes < 4 for c in R.TINY_CASES)
    # each kind of input on every arm and every band height
    for kind in R.KINDS:
        hit = [c.info for c, k in R.case_kinds() if k == kind]
        assert {R.arm(i["kx"]) for i in hit if not i["vfirst"]} == set(range(1, 10)), kind
        assert {i["band"] for i in hit if not i["vfirst"]} == {8, 4, 2, 1}, kind
        assert any(i["vfirst"] for i in hit), kind


def test_pass_order_rule_against_pillow():
    """Pillow resamples tall, narrow images vertical pass first; the intermediate image is uint8, so the order shows.  The rule
    of the plan (and of the oracle) against Pillow itself, on both sides of the switch at several widths, and where the
    height is enlarged."""
    from PIL import Image
    ties = 0
    for W, H in [(2, 223), (2, 225), (2, 201), (3, 300), (3, 301), (8, 800), (8, 801), (21, 2142), (22, 2142), (30, 3000), (30, 3001),
                 (96, 9600), (96, 9601), (96, 9633), (97, 9633), (300, 5), (5, 300), (7, 701)]:
        frame = R.make_frames("random", 1, H, W, seed=H + W)[0]
        pil = np.asarray(Image.fromarray(frame).resize((224, 224), Image.BILINEAR))
        assert lib_vfirst(W, H) == R.vertical_first(W, H) == po.vertical_first(W, H)
        assert np.array_equal(po.resize_bilinear_u8(frame), pil), (W, H)
        other = po.resample_axis0(np.ascontiguousarray(frame), 224) if not R.vertical_first(W, H) else None
        if other is not None:
            other = po.resample_axis0(np.ascontiguousarray(other.transpose(1, 0, 2)), 224).transpose(1, 0, 2)
            ties += np.array_equal(other, pil)
    assert ties == 0                                                     # at these sizes the other order is visibly different
    for cw in range(1, 120):
        for ch in (100 * cw - 1, 100 * cw, 100 * cw + 1, 224, 225):
            assert lib_vfirst(cw, ch) == R.vertical_first(cw, ch)
    assert not lib_vfirst(0, 500) and not lib_vfirst(-3, 500)
    assert R.narrowest_horizontal_first(9633) == 97 and not R.vertical_first(97, 9633) and R.vertical_first(96, 9633)


def test_pipeline_inputs():
    f = R.make_frames("flat", 2, 3, 4)
    assert f[0].min() == 255 and f[1].max() == 0
    s = R.make_frames("stripes", 2, 4, 4)
    assert np.array_equal(s[0, 0, :, 0], [255, 0, 255, 0]) and np.array_equal(s[1, :, 0, 0], [255, 0, 255, 0])
    assert np.array_equal(R.pil_pipeline(R.make_frames("random", 1, 61, 45)[0]), po.preprocess_frame(R.make_frames("random", 1, 61, 45)[0]))
