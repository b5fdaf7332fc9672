"""Exact data, strided views, case lists and the restated launch plan for the TN (weight-gradient) GEMM edge tests (no GPU code;
imported by test_tn_ref_host.py and test_tn_edges_gpu.py).

  dW[N1,N2] += P[M,N1]^T . Q[M,N2],   db[N1] += colsum(P)

Three recipes make dW and db independent of the summation order, of the M-split and of atomics against slabs, so a kernel is
compared bit for bit with fp64, after one call and after two into the same dW / db:
  tern       P in {-2 .. 2}, Q in {-3 .. 3} (asymmetric: a transposed store shows), prior dW / db integers in [-5, 5]: every
             partial sum is an integer below 2^24.
  pow2       P, Q in {0, +-0.5, +-1, +-2}: products are multiples of 1/4, |sum| <= 4 M: non-integer bf16 codes, still exact.
  f32_round  fp32 operands c (1 + e), integer c in {-2 .. 2}, e in {0, -2^-10, +2^-10, +2^-9}: for e != 0 and c != 0 the value is
             no bf16 number and rounds to nearest at c, so the expected result is that of c.  Truncation gives c (1 - 2^-8)
             = 0.996 c wherever e < 0, rounding up c (1 + 2^-7) wherever e > 0.
The condition of each recipe (exact_bound / operand_condition) is asserted on the fp64 reference alone before a result is read.

The plan rules of csrc/tn_plan.hpp and ops._tn_nsplit are restated (tn_split, plan_bf16, plan_f32, default_nsplit) to CHOOSE
cases; every case also carries its form, M-splits and rows per split written out by hand, and test_tn_ref_host.py holds all
three against what the library's plan query answers, so a list that drifts off its form fails there."""
import collections
import os

import torch

import gemm_ref as G

NAN = G.NAN
TN_FORMS = ("XL_SLAB", "XL_ATOMIC", "WIDE_SLAB", "WIDE_ATOMIC", "TILE128", "F32_OWNER64", "F32_OWNER128", "F32_ATOMIC")   # enum TnForm
SLAB_FORMS = ("XL_SLAB", "WIDE_SLAB")
ENOUGH, NONE = 1 << 62, -1                         # slab offers: whatever the form needs (what ops offers) / no slab buffer

# ------------------------------------------------------------------------------------------------ the plan, restated
TK, WQ = 64, 384
XP, XQ, XK, XL_MIN_STEPS = 192, 384, 32, 48
TN_MIN_M, TN_ONE_ROUND = 8192, 256
F32_OWNER64_MAX_TILES = 200
XL_RING = 4                                        # stages of the XL form's LDS ring (gemm_tn_xl.hip, XNST)
SWITCHES = ("SAIS_TN_SLABS=1", "SAIS_TN_XL=0", "SAIS_TN_XL_SLABS=0")


def _cdiv(a, b):
    return -(-a // b)


def tn_split(M, nsplit):
    """tn_plan.hpp, tn_split: at most nsplit slices, a whole number of 64-row steps each -> (slices that hold rows, rows per slice)"""
    rows = _cdiv(_cdiv(M, nsplit), TK) * TK
    return _cdiv(M, rows), rows


def default_nsplit(M, items):
    """ops._tn_nsplit with nsplit = None"""
    tiles = sum((n1 // 128) * (n2 // 128) for n1, n2 in items)
    return max(1, min(_cdiv(M, 256), _cdiv(432, tiles)))


def plan_bf16(items, M, nsplit=None, switches="", slabs=True, aligned16=True):
    """tn_plan.hpp, tn_plan -> (form, M-splits, rows per split); `slabs`: the caller offers what the form needs"""
    assert switches in ("",) + SWITCHES
    old_slabs = switches == "SAIS_TN_SLABS=1"
    xl_on = not old_slabs and switches != "SAIS_TN_XL=0"
    xl_slabs = switches != "SAIS_TN_XL_SLABS=0"
    nsplit = default_nsplit(M, items) if nsplit is None else nsplit
    xl = xl_on and aligned16 and M % XK == 0 and M >= TN_MIN_M and all(n1 % XP == 0 and n2 % XQ == 0 for n1, n2 in items)
    wide = M % TK == 0 and M >= TN_MIN_M and all(n1 % 128 == 0 and n2 % WQ == 0 for n1, n2 in items)
    xt = sum((n1 // XP) * (n2 // XQ) for n1, n2 in items)
    wt = sum((n1 // 128) * (n2 // WQ) for n1, n2 in items)
    xns = max(1, TN_ONE_ROUND // xt) if xl and xt else 1
    if xl and xt and M // XK // xns >= XL_MIN_STEPS:
        return ("XL_SLAB" if slabs and xl_slabs and xns >= 2 else "XL_ATOMIC"), xns, M // XK // xns * XK
    if wide and wt:
        ns, rows = tn_split(M, max(1, TN_ONE_ROUND // wt))
        return ("WIDE_SLAB" if slabs and old_slabs and ns > 1 else "WIDE_ATOMIC"), ns, rows
    ns, rows = tn_split(M, nsplit)
    return "TILE128", ns, rows


def plan_f32(items, M, nsplit):
    """tn_plan.hpp, tn_plan_f32"""
    ns, rows = tn_split(M, nsplit)
    t128 = sum((n1 // 128) * (n2 // 128) for n1, n2 in items)
    return ("F32_OWNER64" if ns == 1 and t128 < F32_OWNER64_MAX_TILES else "F32_OWNER128" if ns == 1 else "F32_ATOMIC"), ns, rows


def xl_steps(M, ns):
    """gemm_tn_xl.hip: the 32-row steps of each M-split (the first M / 32 % ns splits take one more)"""
    base, rem = divmod(M // XK, ns)
    return [base + (1 if z < rem else 0) for z in range(ns)]


# ------------------------------------------------------------------------------------------------ the case lists
BLOCK = ((384, 1536), (1536, 384), (384, 384), (1152, 384))
KV = ((768, 384),)
TEMPORAL = ((384, 2048), (2048, 384), (384, 384), (1152, 384))
ONE = ((256, 128),)
THREE = ((256, 128), (128, 256), (128, 128))

# entry: single = ops.gemm_tn, grouped = ops.gemm_tn_grouped, null_slabs = sais_gemm_tn_grouped (no slab buffer);
# nsplit None = the default of ops._tn_nsplit; form, ns, rows: the plan, by hand (form None: the single fp32 entry has no plan form)
Case = collections.namedtuple("Case", "name entry f32 items M nsplit form ns rows")

# tn_split by hand: M -> nsplit -> (M-splits that hold rows, rows per split)
SMALL_SPLITS = {
    1: {1: (1, 64), 2: (1, 64), 3: (1, 64), 5: (1, 64)},
    63: {1: (1, 64), 2: (1, 64), 3: (1, 64), 5: (1, 64)},
    64: {1: (1, 64), 2: (1, 64), 3: (1, 64), 5: (1, 64)},
    65: {1: (1, 128), 2: (2, 64), 3: (2, 64), 5: (2, 64)},              # the caller's 3 and 5 splits do not fit: two of 64 rows
    127: {1: (1, 128), 2: (2, 64), 3: (2, 64), 5: (2, 64)},
    129: {1: (1, 192), 2: (2, 128), 3: (3, 64), 5: (3, 64)},
    333: {1: (1, 384), 2: (2, 192), 3: (3, 128), 5: (3, 128)},
}
TILE128_SMALL = [Case(f"t128_{entry}_m{M}_s{s}", entry, False, items, M, s, "TILE128", *SMALL_SPLITS[M][s])
                 for entry, items in (("single", ONE), ("grouped", THREE)) for M in SMALL_SPLITS for s in (1, 2, 3, 5)]
TILE128_LARGE = [
    Case("t128_blk_m8249", "grouped", False, BLOCK, 8192 + 57, None, "TILE128", 4, 2112),
    Case("t128_blk_m12640", "grouped", False, BLOCK, 12640, None, "TILE128", 4, 3200),
    Case("t128_n512_m8256", "grouped", False, ((384, 512),), 8256, None, "TILE128", 33, 256),         # N2 % 384 != 0 at M >= 8192
    Case("t128_blk_m15328", "grouped", False, BLOCK, 15328, None, "TILE128", 4, 3840),                # 479 steps: neither XL nor wide
]
WIDE_ATOMIC = [
    Case("wide_blk_m8192", "grouped", False, BLOCK, 8192, None, "WIDE_ATOMIC", 7, 1216),              # the last split holds 896 rows
    Case("wide_kv_m8256", "grouped", False, KV, 8256, None, "WIDE_ATOMIC", 33, 256),
    Case("wide_one_tile_m8192", "grouped", False, ((128, 384),), 8192, None, "WIDE_ATOMIC", 128, 64),
    Case("wide_one_tile_m8256", "grouped", False, ((128, 384),), 8256, None, "WIDE_ATOMIC", 129, 64),
    Case("wide_blk_m15296", "grouped", False, BLOCK, 15296, None, "WIDE_ATOMIC", 7, 2240),            # 478 steps / 10 = 47: XL refused
]
XL_SLAB = [
    Case("xl_blk_m15360", "grouped", False, BLOCK, 15360, None, "XL_SLAB", 10, 1536),                 # 48 steps each
    Case("xl_blk_m15392", "grouped", False, BLOCK, 15392, None, "XL_SLAB", 10, 1536),                 # 49 + 9 x 48
    Case("xl_blk_m16000", "grouped", False, BLOCK, 16000, None, "XL_SLAB", 10, 1600),                 # 50
    Case("xl_blk_m16320", "grouped", False, BLOCK, 16320, None, "XL_SLAB", 10, 1632),                 # 51
    Case("xl_blk3_m8192", "grouped", False, BLOCK * 3, 8192, None, "XL_SLAB", 3, 2720),               # 72 tiles: 86 + 85 + 85
    Case("xl_blk5_m8224", "grouped", False, BLOCK * 5, 8224, None, "XL_SLAB", 2, 4096),               # 120 tiles: 129 + 128
]
XL_RESIDUES = {"xl_blk_m15360": {0}, "xl_blk_m15392": {0, 1}, "xl_blk_m16000": {2}, "xl_blk_m16320": {3}, "xl_blk3_m8192": {1, 2},
               "xl_blk5_m8224": {0, 1}}                                                                # steps per split mod XL_RING
XL_ATOMIC = [
    Case("xla_blk6kv_m8224", "grouped", False, BLOCK * 6 + KV, 8224, None, "XL_ATOMIC", 1, 8224),     # 148 tiles, one owner each
    Case("xla_blk11_m8192", "grouped", False, BLOCK * 11, 8192, None, "XL_ATOMIC", 1, 8192),          # 264 tiles: more than one round
    Case("xla_nullslab_m15360", "null_slabs", False, BLOCK, 15360, None, "XL_ATOMIC", 10, 1536),
]
F32 = [Case(f"f32_own64_m{M}", "grouped", True, TEMPORAL, M, 1, "F32_OWNER64", 1, rows)
       for M, rows in ((1, 64), (13, 64), (64, 64), (65, 128), (264, 320))] + [
    Case("f32_own64_one_tile_m65", "grouped", True, ((128, 128),), 65, 1, "F32_OWNER64", 1, 128),
] + [Case(f"f32_own128_m{M}", "grouped", True, TEMPORAL * 2, M, 1, "F32_OWNER128", 1, rows)
     for M, rows in ((1, 64), (65, 128), (264, 320))] + [
    Case("f32_atomic_m65", "grouped", True, TEMPORAL, 65, 2, "F32_ATOMIC", 2, 64),
    Case("f32_atomic_m264", "grouped", True, TEMPORAL, 264, 2, "F32_ATOMIC", 2, 192),
    Case("f32_atomic_2x_m264", "grouped", True, TEMPORAL * 2, 264, 3, "F32_ATOMIC", 3, 128),
]
F32_SINGLE = [Case(f"f32_single_m{M}_s{s}", "single", True, ONE, M, s, None, *SMALL_SPLITS[M][s]) for M in (65, 333) for s in (1, 3)]

BF16_CASES = TILE128_SMALL + TILE128_LARGE + WIDE_ATOMIC + XL_SLAB + XL_ATOMIC
F32_CASES = F32 + F32_SINGLE
ALL_CASES = BF16_CASES + F32_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

# one case per form for pow2 and for the random data (WIDE_SLAB exists under SAIS_TN_SLABS=1 only: wide_blk_m8192 in that child)
ONE_PER_FORM = ("xl_blk_m15392", "xla_nullslab_m15360", "wide_blk_m8192", "t128_blk_m8249", "f32_own64_m264", "f32_own128_m65",
                "f32_atomic_m264")

# the BLOCK cases the alternate-switch children run, and their plan under each switch: M -> (form, M-splits, rows), by hand
ALT_CASES = ("wide_blk_m8192", "wide_blk_m15296", "xl_blk_m15360", "xl_blk_m15392")
ALT = {
    "SAIS_TN_SLABS=1": {8192: ("WIDE_SLAB", 7, 1216), 15296: ("WIDE_SLAB", 7, 2240), 15360: ("WIDE_SLAB", 7, 2240),
                        15392: ("TILE128", 4, 3904)},                       # 481 steps of 32: not a whole number of 64-row steps
    "SAIS_TN_XL=0": {8192: ("WIDE_ATOMIC", 7, 1216), 15296: ("WIDE_ATOMIC", 7, 2240), 15360: ("WIDE_ATOMIC", 7, 2240),
                     15392: ("TILE128", 4, 3904)},
    "SAIS_TN_XL_SLABS=0": {8192: ("WIDE_ATOMIC", 7, 1216), 15296: ("WIDE_ATOMIC", 7, 2240), 15360: ("XL_ATOMIC", 10, 1536),
                           15392: ("XL_ATOMIC", 10, 1536)},
}


def switches_from_env(env=None):
    """the switch setting of this process as a key of ALT ("" = defaults); anything else is not a setting these tests know"""
    env = os.environ if env is None else env
    sw = " ".join(f"{k}={v}" for k, v in sorted(env.items()) if k.startswith("SAIS_TN_"))
    assert sw in ("",) + SWITCHES, sw
    return sw


def expected_plan(case, switches=""):
    """(form, M-splits, rows per split) written by hand: the case's own under the defaults, the ALT table under a switch (fp32
    entries have no switch).  A case the table does not hold raises: it must not run under that switch."""
    if switches == "" or case.f32:
        return case.form, case.ns, case.rows
    assert case.name in ALT_CASES and case.items == BLOCK, case.name
    return ALT[switches][case.M]


# ------------------------------------------------------------------------------------------------ recipes
RECIPES = ("tern", "pow2", "f32_round")
RECIPE_MAX = {"tern": (2.0, 3.0, 1.0), "pow2": (2.0, 2.0, 0.25), "f32_round": (2.0, 2.0, 1.0)}      # max |p|, max |q|, unit of the sums
PRIOR_MAX = 5.0                                                                                       # prior dW / db: integers in [-5, 5]
POW2_VALUES = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
F32_ROUND_E = (0.0, -2.0 ** -10, 2.0 ** -10, 2.0 ** -9)
CALLS = 2


def exact_bound(recipe, M, calls=CALLS):
    """the largest magnitude any partial sum of dW or db can reach, in units of the recipe: below 2^24 = exact in f32 in any order"""
    pmax, qmax, unit = RECIPE_MAX[recipe]
    return (pmax * max(qmax, 1.0) * M * calls + PRIOR_MAX) / unit


def _gen(device, seed):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return g


def operand(recipe, role, M, N, seed, device, f32=False):
    """-> (values as the kernel reads them, what they mean in fp64).  role "p" | "q"."""
    g = _gen(device, seed)
    ri = lambda lo, hi: torch.randint(lo, hi + 1, (M, N), generator=g, device=device)
    if recipe == "tern":
        v = ri(-2, 2) if role == "p" else ri(-3, 3)
        v = v.float() if f32 else v.to(torch.bfloat16)
        return v, v.double()
    if recipe == "pow2":
        v = torch.tensor(POW2_VALUES, device=device)[ri(0, 6)]
        v = v if f32 else v.to(torch.bfloat16)
        return v, v.double()
    if recipe == "f32_round":
        assert f32
        c = ri(-2, 2).float()
        e = torch.tensor(F32_ROUND_E, device=device)[ri(0, 3)]
        return c * (1.0 + e), c.double()
    if recipe == "randn":
        v = torch.randn(M, N, generator=g, device=device)
        return (v if f32 else v.to(torch.bfloat16)), v.to(torch.bfloat16).double()
    raise KeyError(recipe)


def truncate_bf16(x):
    """fp32 -> bf16 by dropping the low 16 bits (what a staging that forgot to round would do)"""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def operand_condition(recipe, values, meaning):
    """the recipe's claim about its operands, on the data itself"""
    vals = set(meaning.unique().tolist())
    if recipe == "tern":
        return vals <= set(range(-3, 4)) and torch.equal(values.double(), meaning)
    if recipe == "pow2":
        return vals <= set(POW2_VALUES) and torch.equal(values.double(), meaning)
    if recipe == "f32_round":
        off = (values.double() != meaning)
        rounds = torch.equal(values.to(torch.bfloat16).double(), meaning)                      # to nearest: c
        not_bf16 = bool((values.to(torch.bfloat16).float() != values)[off].all())
        trunc = truncate_bf16(values).double()
        return (vals <= set(range(-2, 3)) and rounds and not_bf16 and float(off.double().mean()) > 0.4 and
                float((trunc != meaning).double().mean()) > 0.1 and
                bool(torch.equal(trunc[trunc != meaning], (meaning * (1 - 2.0 ** -8))[trunc != meaning])))
    raise KeyError(recipe)


def reference_condition(recipe, ref, M, calls=CALLS):
    """on the fp64 reference alone: a multiple of the recipe's unit, and the bound on every partial sum is below 2^24"""
    unit = RECIPE_MAX[recipe][2]
    return bool(torch.equal(torch.round(ref / unit), ref / unit)) and exact_bound(recipe, M, calls) < 2 ** 24


# ------------------------------------------------------------------------------------------------ strided views
ROWS_BEHIND = 64                                   # NaN rows behind row M - 1 of P and Q
# (pad, first column) of P and of Q: the leading dimension is N + pad, the base 16-B aligned and not 128-B aligned.  The grouped fp32
# entry takes ld % 4 == 0 (N + 12 is no multiple of 8); the single entries check ld % 8 for both operand types.
PADS = {("bf16", "grouped"): ((24, 8), (40, 16)), ("bf16", "single"): ((24, 8), (40, 16)), ("bf16", "null_slabs"): ((24, 8), (40, 16)),
        ("f32", "grouped"): ((12, 4), (20, 8)), ("f32", "single"): ((24, 4), (40, 8))}
DW_BORDER = 4                                      # integer columns left and right of the dW slice; guard elements around db


def distinct(items):
    """the item shapes of a launch without repetitions, in order: repeated shapes (k x BLOCK) share their P / Q, never their dW"""
    return tuple(dict.fromkeys(items))


class Operands:
    """P / Q of every distinct shape of a launch as views into NaN-surrounded buffers, with P^T Q and colsum(P) in fp64 of what the
    values MEAN (f32_round: of c).  Computed once per (case shape list, M, recipe), never written."""

    def __init__(self, items, M, recipe, f32, entry, device, seed=0):
        pads = PADS[("f32" if f32 else "bf16", entry)]
        self.M, self.recipe, self.by_shape, self.buffers = M, recipe, {}, []
        for i, (n1, n2) in enumerate(distinct(items)):
            pv, pm = operand(recipe, "p", M, n1, 7919 * M + 31 * i + seed, device, f32)
            qv, qm = operand(recipe, "q", M, n2, 7919 * M + 31 * i + 17 + seed, device, f32)
            if recipe != "randn":
                assert operand_condition(recipe, pv, pm) and operand_condition(recipe, qv, qm), (recipe, n1, n2)
            p, pbuf = G.padded(pv, *pads[0], rows_extra=ROWS_BEHIND)
            q, qbuf = G.padded(qv, *pads[1], rows_extra=ROWS_BEHIND)
            for t, (pad, off) in ((p, pads[0]), (q, pads[1])):
                assert t.data_ptr() % 16 == 0 and t.data_ptr() % 128 != 0 and t.stride(0) == t.shape[1] + pad > t.shape[1]
            self.buffers += [pbuf, qbuf]
            self.by_shape[(n1, n2)] = (p, q, pm.t() @ qm, pm.sum(0))


class Outputs:
    """dW as a column slice of a wider f32 buffer with integer border columns, db as a slice with guard elements: one per ITEM"""

    def __init__(self, items, device, seed=1):
        g = _gen(device, 1000 + seed)
        self.items = []
        for n1, n2 in items:
            wide = torch.randint(-5, 6, (n1, n2 + 2 * DW_BORDER), generator=g, device=device).float()
            dbuf = None if n1 == n2 else torch.randint(-5, 6, (n1 + 2 * DW_BORDER,), generator=g, device=device).float()
            self.items.append(dict(wide=wide, dW=wide[:, DW_BORDER:DW_BORDER + n2], wide0=wide.clone(), dbuf=dbuf,
                                   db=None if dbuf is None else dbuf[DW_BORDER:DW_BORDER + n1],
                                   dbuf0=None if dbuf is None else dbuf.clone()))

    def check(self, items, operands, calls, exact=True):
        """after `calls` launches: dW == dW0 + calls P^T Q and db == db0 + calls colsum(P) in fp64, bit for bit; border columns and
        guards unchanged; nothing but finite numbers.  Returns the (dW, db) pairs for bit-identity checks."""
        recipe, M = operands.recipe, operands.M
        for shape, o in zip(items, self.items):
            _, _, ptq, colsum = operands.by_shape[shape]
            b = DW_BORDER
            want = o["wide0"][:, b:-b].double() + calls * ptq
            assert reference_condition(recipe, want, M, calls), (shape, "dW reference")
            assert bool(torch.isfinite(o["dW"]).all()), (shape, "a NaN or inf arrived in dW")
            assert torch.equal(o["dW"].double(), want), (shape, calls, "dW", _first_diff(o["dW"].double(), want))
            assert torch.equal(o["wide"][:, :b], o["wide0"][:, :b]) and torch.equal(o["wide"][:, -b:], o["wide0"][:, -b:]), \
                (shape, "columns beside the dW slice were written")
            if o["db"] is not None:
                want = o["dbuf0"][b:-b].double() + calls * colsum
                assert reference_condition(recipe, want, M, calls), (shape, "db reference")
                assert torch.equal(o["db"].double(), want), (shape, calls, "db", _first_diff(o["db"].double(), want))
                assert torch.equal(o["dbuf"][:b], o["dbuf0"][:b]) and torch.equal(o["dbuf"][-b:], o["dbuf0"][-b:]), \
                    (shape, "guard elements of db were written")
        return [(o["dW"].clone(), None if o["db"] is None else o["db"].clone()) for o in self.items]


def _first_diff(got, want):
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()[0].tolist()
    return f"{int(bad.sum())} differ, first at {idx}: {got[tuple(idx)].item()} != {want[tuple(idx)].item()}"


def launch_items(items, operands, outputs):
    """[(p, q, dW, db)] as ops.gemm_tn_grouped takes them"""
    return [operands.by_shape[shape][:2] + (o["dW"], o["db"]) for shape, o in zip(items, outputs.items)]


# ------------------------------------------------------------------------------------------------ the launch, restated
MUTATIONS = ("unmasked_tail", "drop_last_step", "bias_twice", "transposed_store", "truncate", "border_written")


def model_launch(items, M, rows, mutate=None):
    """What one grouped launch computes, in fp64 torch over M-splits of `rows` rows and 64-row steps, reading the operands through
    their buffers the way a kernel does.  items: [(p, q, dW, db)] views.  The mutations are errors the GPU lists have to notice."""
    assert mutate is None or mutate in MUTATIONS
    for p, q, dW, db in items:
        rd = (lambda t: truncate_bf16(t.float())) if mutate == "truncate" else (lambda t: t.to(torch.bfloat16))
        acc = torch.zeros(dW.shape, dtype=torch.float64)
        accb = torch.zeros(dW.shape[0], dtype=torch.float64)
        for mbeg in range(0, M, rows):
            mend = min(M, mbeg + rows)
            nsteps = _cdiv(mend - mbeg, TK)
            for st in range(nsteps):
                if mutate == "drop_last_step" and mend == M and st == nsteps - 1 and nsteps > 1:
                    continue
                lo = mbeg + st * TK
                hi = lo + TK if mutate == "unmasked_tail" else min(lo + TK, mend)
                view = lambda t: t.as_strided((hi - lo, t.shape[1]), t.stride(), t.storage_offset() + lo * t.stride(0))
                pp, qq = rd(view(p)).double(), rd(view(q)).double()
                acc += pp.t() @ qq
                accb += pp.sum(0) * (2 if mutate == "bias_twice" else 1)
        if mutate == "transposed_store" and dW.shape[0] == dW.shape[1]:
            acc = acc.t()
        if mutate == "border_written":
            dW.as_strided((dW.shape[0], 1), dW.stride(), dW.storage_offset() + dW.shape[1]).add_(1.0)     # the column right of the slice
        dW += acc.float()
        if db is not None:
            db += accb.float()


# ------------------------------------------------------------------------------------------------ the library's plan query
def plan_query(lib, arr, nitems, M, nsplit, offer, f32):
    """sais_gemm_tn_plan_ (a host function: no launch) -> (return code, (form, M-splits, rows per split), workgroups, slab bytes)"""
    import ctypes
    fn = lib.sais_gemm_tn_plan_
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
    fn.restype = ctypes.c_int
    out = (ctypes.c_int64 * 6)(-1, 0, 0, 0, 0, 0)
    rc = fn(arr, nitems, M, nsplit, offer, int(bool(f32)), out)
    return rc, (TN_FORMS[out[0]] if out[0] >= 0 else None, out[2], out[3]), out[4], out[5]


def case_query(case):
    """(nsplit, offer) of the plan query that describes the launch a case makes"""
    nsplit = default_nsplit(case.M, case.items) if case.nsplit is None else case.nsplit
    return nsplit, (NONE if case.entry == "null_slabs" or case.f32 else ENOUGH)
