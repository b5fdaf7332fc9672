"""Reference side of the frame-preprocessing edge suites (sais_amd/csrc/preprocess.hip).

Two things live here, one copy each:
  * a plain-Python restatement of the host plan (crop box of torchvision 0.9.0's center_crop + PIL's Image.crop edge
    rounding, Pillow's per-axis bounds and ksize, the band loop with its LDS budget), which test_preprocess_edges_host.py
    holds against `sais_preprocess_plan_describe` field by field;
  * the Pillow pipeline the kernel must reproduce bit for bit (used by test_preprocess.py and both edge suites), and the
    case table of the GPU suite, derived from the restatement so that every case provably reaches the arm it is named for.

Nothing here imports the library: the case table must not depend on the code under test."""
import functools

import numpy as np

OUT = 224
ROW_BYTES = OUT * 3
LDS_BUDGET = 60 * 1024
LUT_BYTES = 3 * 256 * 4
FIELDS = ("left", "top", "cw", "ch", "kx", "ky", "band", "nbands", "max_rows", "lds_bytes")
GENERIC = 9                      # arm index of horizontal_pass_generic (kx > 32); arms 1..8 are horizontal_pass<G>


# ------------------------------------------------------------------------------------------------ the plan, restated
def crop_box(H, W, hf=0.8, wf=0.8):
    """(left, top, cw, ch) of CenterCrop((hf H, wf W)) followed by PIL's crop, round() = round-half-even; None if the
    rounded box leaves the frame or is empty (the plan refuses those)."""
    ch, cw = hf * H, wf * W
    top, left = int(round((H - ch) / 2.)), int(round((W - cw) / 2.))
    x0, y0, x1, y1 = (int(round(v)) for v in (left, top, left + cw, top + ch))
    if x0 < 0 or y0 < 0 or x1 > W or y1 > H or x1 <= x0 or y1 <= y0:
        return None
    return x0, y0, x1 - x0, y1 - y0


def ksize(n):
    """Resample.c precompute_coeffs, bilinear (support 1) from n samples to 224: int(ceil(support)) * 2 + 1."""
    support = max(n / OUT, 1.0)
    return int(np.ceil(support)) * 2 + 1


@functools.lru_cache(maxsize=None)
def axis_bounds(n):
    """Pillow's (xmin, count) of each of the 224 output indices of an axis of n samples."""
    scale = n / OUT
    support = max(scale, 1.0)
    out = []
    for xx in range(OUT):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n)
        out.append((xmin, xmax - xmin))
    return tuple(out)


def band_rows(ch, band):
    """(first crop row, row count) of each band of `band` output rows."""
    b = axis_bounds(ch)
    rows = []
    for b0 in range(0, OUT, band):
        part = b[b0:b0 + band]
        lo = min(p[0] for p in part)
        rows.append((lo, max(p[0] + p[1] for p in part) - lo))
    return rows


@functools.lru_cache(maxsize=None)
def band_plan(ch):
    """(band, nbands, max_rows, lds_bytes): the largest of 8, 4, 2, 1 output rows whose input rows fit the budget; None
    when one output row alone does not fit."""
    band = 8
    while True:
        max_rows = max(r[1] for r in band_rows(ch, band))
        if max_rows * ROW_BYTES + 16 + LUT_BYTES <= LDS_BUDGET or band == 1:
            break
        band >>= 1
    lds = ((max_rows * ROW_BYTES + 15) & ~15) + LUT_BYTES
    if lds > LDS_BUDGET:
        return None
    return band, (OUT + band - 1) // band, max_rows, lds


def describe(H, W, hf=0.8, wf=0.8):
    """The ten fields of sais_preprocess_plan_describe, or None where it returns SAIS_ERR_ARG."""
    box = crop_box(H, W, hf, wf)
    if box is None:
        return None
    bp = band_plan(box[3])
    if bp is None:
        return None
    return box + (ksize(box[2]), ksize(box[3])) + bp


def vertical_first(cw, ch):
    """Pillow resamples a box of more than 100 rows per column, its height being reduced, vertical pass first (observed on
    Pillow 12.2: test_preprocess_edges_host.py::test_pass_order_rule_against_pillow); the plan then runs
    preprocess_vfirst_kernel and none of preprocess_kernel's arms or bands."""
    return ch > OUT and ch > 100 * cw


def narrowest_horizontal_first(ch):
    """the smallest crop width at which a crop of ch rows still goes horizontal pass first"""
    return max(1, -(-ch // 100))


def arm(kx):
    """Which horizontal pass preprocess_kernel takes: G = 1..8, or GENERIC."""
    return (kx + 3) >> 2 if kx <= 32 else GENERIC


@functools.lru_cache(maxsize=None)
def arm_switches():
    """[(cw, arm)]: the smallest crop width of each arm, in order (arm 1 from cw = 1)."""
    out, cur = [], 0
    for cw in range(1, 4000):
        a = arm(ksize(cw))
        if a != cur:
            out.append((cw, a))
            cur = a
    return out


@functools.lru_cache(maxsize=None)
def band_switches():
    """([(ch, band before, band after)], first refused ch): every crop height at which the band differs from that of
    ch - 1, up to the refusal."""
    out, ch, cur = [], 1, band_plan(1)[0]
    while True:
        ch += 1
        bp = band_plan(ch)
        if bp is None:
            return out, ch
        if bp[0] != cur:
            out.append((ch, cur, bp[0]))
            cur = bp[0]


# ------------------------------------------------------------------------------------------------ the Pillow pipeline
def pil_pipeline(frame, hf=0.8, wf=0.8):
    """The reference's per-frame CPU pipeline with Pillow doing the work (torchvision 0.9.0 call sequence)."""
    import torch
    from PIL import Image

    from oracle import preprocess_oracle as po
    img = Image.fromarray(frame)
    w, h = img.size
    ch, cw = hf * h, wf * w
    top, left = int(round((h - ch) / 2.)), int(round((w - cw) / 2.))
    img = img.crop((left, top, left + cw, top + ch)).resize((224, 224), Image.BILINEAR)
    t = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float().div(255)
    return t.sub_(torch.tensor(po.MEAN)[:, None, None]).div_(torch.tensor(po.STD)[:, None, None]).numpy()


# ------------------------------------------------------------------------------------------------ inputs
KINDS = ("random", "flat", "stripes")


def make_frames(kind, F, H, W, seed=0):
    """uint8 [F, H, W, 3].  random: bytes; flat: frames alternate all 255 / all 0 (a coefficient row must sum so that 255
    stays 255); stripes: alternating 0 / 255 columns on even frames, rows on odd ones (the accumulator extremes)."""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    out = np.zeros((F, H, W, 3), np.uint8)
    for f in range(F):
        if kind == "flat":
            out[f] = 255 if f % 2 == 0 else 0
        elif f % 2 == 0:
            out[f, :, (seed + f // 2) % 2::2] = 255
        else:
            out[f, (seed + f // 2) % 2::2] = 255
    return out


# ------------------------------------------------------------------------------------------------ the GPU suite's cases
class Case:
    """One geometry of the GPU suite: `F` frames of H x W at fractions (hf, wf)."""

    def __init__(self, name, H, W, F=2, hf=1.0, wf=1.0):
        self.name, self.H, self.W, self.F, self.hf, self.wf = name, H, W, F, hf, wf

    @property
    def info(self):
        d = describe(self.H, self.W, self.hf, self.wf)
        if d is None:
            return None
        i = dict(zip(FIELDS, d))
        i["vfirst"] = vertical_first(i["cw"], i["ch"])
        return i

    @property
    def total_bytes(self):
        return self.F * self.H * self.W * 3

    def __repr__(self):
        return self.name


def _tap_cases():
    """width_frac = 1 (W = cw), H = 5: the last width of an arm and the first of the next, and one wide generic frame;
    then the two real geometries at 0.8."""
    sw = arm_switches()
    cases = []
    for cw, a in sw[1:]:
        cases.append(Case(f"taps_w{cw - 1}_arm{a - 1}", 5, cw - 1))
        cases.append(Case(f"taps_w{cw}_arm{a}", 5, cw))
    cases.append(Case("taps_w3811_generic", 5, 3811))
    cases.append(Case("taps_2560x16_at_0.8", 16, 2560, hf=0.8, wf=0.8))
    cases.append(Case("taps_3840x16_at_0.8", 16, 3840, hf=0.8, wf=0.8))
    return cases


def _band_cases():
    """height_frac = 1 (H = ch): the crop heights on both sides of every band switch-over and the tallest accepted one, each
    at W = 8 (Pillow goes vertical pass first there: preprocess_vfirst_kernel) and at the narrowest width that goes
    horizontal pass first (preprocess_kernel at that band height)."""
    sw, refused = band_switches()
    heights = {}
    for ch, before, after in sw:
        heights[ch - 1], heights[ch] = before, after
    cases = [Case(f"band_h{h}_b{b}", h, 8) for h, b in sorted(heights.items())]
    cases.append(Case(f"band_h{refused - 1}_last", refused - 1, 8))
    cases += [Case(f"{c.name}_w{narrowest_horizontal_first(c.H)}", c.H, narrowest_horizontal_first(c.H)) for c in list(cases)]
    return cases


def refused_case():
    return Case("band_first_refused", band_switches()[1], 8, F=1)


def _tiny_cases():
    cases = [Case(f"tiny_{h}x{w}_f{f}", h, w, F=f) for h, w in ((1, 1), (1, 7), (7, 1), (2, 3)) for f in (1, 3)]
    cases.append(Case("tiny_up_h_down_w", 3, 500))               # 3 -> 224 rows, 500 -> 224 columns
    cases.append(Case("tiny_down_h_up_w", 500, 3))
    return cases


def _tail_cases():
    """Total byte counts with residue 1, 2 and 3 mod 4: the last dword of the last row straddles the end of the frames."""
    return [Case("tail_res1", 3, 5, F=1), Case("tail_res2", 7, 5, F=2), Case("tail_res3", 5, 3, F=3),
            Case("tail_res3_wide", 3, 227, F=1)]


TAP_CASES, BAND_CASES, TINY_CASES, TAIL_CASES = _tap_cases(), _band_cases(), _tiny_cases(), _tail_cases()
GPU_CASES = TAP_CASES + BAND_CASES + TINY_CASES + TAIL_CASES


def case_kinds():
    """[(case, kind)]: every case with random bytes; flat and stripes on one case of every arm and every band height, and on
    the tiny and tail cases in turn."""
    out = [(c, "random") for c in GPU_CASES]
    seen = set()
    for c in TAP_CASES + BAND_CASES:
        i = c.info
        key = ("arm", arm(i["kx"])) if c in TAP_CASES else ("band", i["band"], i["vfirst"])
        if key not in seen:
            seen.add(key)
            out += [(c, "flat"), (c, "stripes")]
    for n, c in enumerate(TINY_CASES + TAIL_CASES):
        out.append((c, ("flat", "stripes")[n % 2]))
    return out
