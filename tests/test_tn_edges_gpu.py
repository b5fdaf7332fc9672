"""The TN (weight-gradient) GEMMs — sais_gemm_tn, sais_gemm_tn_grouped / _ws, sais_gemm_tn_grouped_f32, sais_gemm_tn_f32 — in every
launch form of csrc/tn_plan.hpp (TnForm), at the ragged M, short last M-splits and ring residues where each can go wrong, with
free row strides, on a real MI355X.

Exact cases use the recipes of tests/tn_ref.py (`tern`, `pow2`, `f32_round`): the condition that makes the fp64 reference
independent of the summation order is asserted on the reference first, then dW and db must be torch.equal to
dW0 + k P^T Q and db0 + k colsum(P) after k = 1 and k = 2 calls into the same buffers.  P and Q are column slices of wider
buffers that hold NaN beside the slice and in 64 rows behind row M - 1; dW and db lie between integer border columns / guard
elements that must not change.  Every case first asserts, through the plan query (a host call), that it takes the form written
beside it in tn_ref.py.  Random data runs once per form against fp64 under the bars of test_kernels_gpu.py (test_gemm_tn,
test_gemm_tn_grouped_f32_accumulates_owned_or_atomic), unchanged; observed / bar goes to parity_log("tn_edge_<form>_...")."""
import ctypes
import functools
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import parity
import tn_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.fixture(scope="module")
def ops():
    from sais_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from sais_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _sw():
    """"" or the switch an alternate-form child runs under (read when a test runs, not when the file is collected)"""
    return T.switches_from_env()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=2)
def _operands(shapes, M, recipe, f32, entry):
    """P, Q and the fp64 references of a launch: computed once per (distinct shapes, M, recipe), never written"""
    return T.Operands(shapes, M, recipe, f32, entry, DEV)


def _case_operands(case, recipe):
    return _operands(T.distinct(case.items), case.M, recipe, case.f32, case.entry if case.f32 else "grouped")


def _array(ops, L, items):
    return (L.SaisTnItem * len(items))(*[ops._tn_item(*it) for it in items])


def _assert_plan(ops, L, case, items):
    """the launch about to be made takes the form the case names (host call, no launch); returns the form"""
    arr = _array(ops, L, items)
    nsplit, offer = T.case_query(case)
    rc, plan, _, slab = T.plan_query(L.load(), arr, len(items), case.M, nsplit, offer, case.f32)
    want = T.expected_plan(case, _sw())
    if want[0] is None:                                  # the single fp32 entry: tn_split alone
        plan = (None,) + plan[1:]
    assert rc == 0 and plan == want, (case.name, _sw(), rc, plan, want)
    if case.entry == "grouped" and not case.f32:         # what ops.gemm_tn_grouped will offer is what that form uses
        assert slab == L.load().sais_gemm_tn_grouped_slab_bytes(arr, len(items), case.M) and (slab > 0) == (plan[0] in T.SLAB_FORMS)
    return plan[0]


def _launch(ops, L, case, items):
    if case.entry == "single":
        (p, q, dW, db), = items
        ops.gemm_tn(p, q, dW, db, nsplit=case.nsplit)
    elif case.entry == "grouped":
        ops.gemm_tn_grouped(items, case.M, nsplit=case.nsplit)
    else:                                                # the public entry without a slab buffer: the form's atomics
        L.call("sais_gemm_tn_grouped", _array(ops, L, items), len(items), case.M, T.case_query(case)[0], _stream())


def _exact(ops, L, case, recipe):
    opnd = _case_operands(case, recipe)
    runs = []
    for rep in range(2):
        outs = T.Outputs(case.items, DEV)                # the same prior dW / db every time
        items = T.launch_items(case.items, opnd, outs)
        form = _assert_plan(ops, L, case, items)
        got = []
        for calls in (1, 2):
            _launch(ops, L, case, items)
            got.append(outs.check(case.items, opnd, calls))
        runs.append(got)
        if form not in T.SLAB_FORMS:
            break
    if len(runs) == 2:                                   # slabs + fixed-order finish: the whole sequence again, bit-identical
        for a, b in zip(runs[0], runs[1]):
            for (w1, b1), (w2, b2) in zip(a, b):
                assert torch.equal(w1, w2) and (b1 is None or torch.equal(b1, b2)), (case.name, "second sequence differs")
    return form


def _ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("case", T.BF16_CASES, ids=_ids(T.BF16_CASES))
def test_exact_tern(ops, L, case):
    """every bf16 case of the lists: the 128 x 128 kernel (single entry and grouped, masked and LDS-DMA tiles) at M in 1 .. 333
    with 1, 2, 3, 5 caller splits and at large ragged M; the 128 x 384 kernel with a short last split, one-tile launches of 128 /
    129 one-step splits and just under the XL threshold; the XL form at 48, 48 / 49, 50, 51 steps per split (all four residues of
    its four-stage ring), with 72 and 120 tiles, as one-owner atomics over 148 and 264 tiles, and behind a NULL slab pointer"""
    _exact(ops, L, case, "tern")


@pytest.mark.parametrize("case", T.F32_CASES, ids=_ids(T.F32_CASES))
def test_exact_tern_f32(ops, L, case):
    """the fp32-operand forms: 64-row owner tiles, 128-row owner tiles (264 tiles: two temporal layers in one launch), atomics, and
    the single entry, at M in 1 .. 333 (a one-row second step at 65)"""
    _exact(ops, L, case, "tern")


@pytest.mark.parametrize("case", T.F32_CASES, ids=_ids(T.F32_CASES))
def test_exact_f32_operands_are_rounded_to_nearest(ops, L, case):
    """c (1 + e) is no bf16 number and rounds to c: the result must be that of c, bit for bit.  Truncation gives 0.996 c where e < 0."""
    _exact(ops, L, case, "f32_round")


POW2 = [T.BY_NAME[n] for n in T.ONE_PER_FORM]


@pytest.mark.parametrize("case", POW2, ids=_ids(POW2))
def test_exact_pow2(ops, L, case):
    """one case per form on {0, +-0.5, +-1, +-2}: non-integer bf16 codes, sums in multiples of 1/4"""
    _exact(ops, L, case, "pow2")


# ------------------------------------------------------------------------------------------------ random
@pytest.mark.parametrize("case", POW2, ids=_ids(POW2))
def test_random(ops, L, case):
    """seeded randn (bf16, or fp32 with the reference on p.bfloat16()), one case per form, one call: the bars of test_gemm_tn and
    test_gemm_tn_grouped_f32_accumulates_owned_or_atomic, 2e-3 sqrt(M) + 1e-4 |ref| for dW and 1e-3 sqrt(M) for db"""
    opnd = _case_operands(case, "randn")
    outs = T.Outputs(case.items, DEV)
    items = T.launch_items(case.items, opnd, outs)
    form = _assert_plan(ops, L, case, items)
    _launch(ops, L, case, items)
    b, M, rw, rb = T.DW_BORDER, case.M, 0.0, 0.0
    for shape, o in zip(case.items, outs.items):
        _, _, ptq, colsum = opnd.by_shape[shape]
        want = o["wide0"][:, b:-b].double() + ptq
        rw = max(rw, float(((o["dW"].double() - want).abs() / (2e-3 * math.sqrt(M) + 1e-4 * want.abs())).max()))
        assert torch.equal(o["wide"][:, :b], o["wide0"][:, :b]) and torch.equal(o["wide"][:, -b:], o["wide0"][:, -b:])
        if o["db"] is not None:
            want = o["dbuf0"][b:-b].double() + colsum
            rb = max(rb, float(((o["db"].double() - want).abs() / (1e-3 * math.sqrt(M))).max()))
            assert torch.equal(o["dbuf"][:b], o["dbuf0"][:b]) and torch.equal(o["dbuf"][-b:], o["dbuf0"][-b:])
    print(f"\n{case.name} ({form}): dW {rw:.3e} of the bar, db {rb:.3e} of the bar")
    parity.parity_log(f"tn_edge_{form.lower()}_dW", rw, 1.0)
    parity.parity_log(f"tn_edge_{form.lower()}_db", rb, 1.0)
    assert rw <= 1.0 and rb <= 1.0 and math.isfinite(rw) and math.isfinite(rb), (case.name, form, rw, rb)


# ------------------------------------------------------------------------------------------------ alternate switches
@pytest.mark.parametrize("switches", T.SWITCHES)
def test_alternate_switches_pass_the_block_cases(switches):
    """The switches are read once per process: the exact BLOCK cases at M = 8192, 15 296, 15 360, 15 392 (and the random ones among
    them) in a child process with the switch set.  The forms the child expects — WIDE_SLAB, WIDE_ATOMIC, XL_ATOMIC, TILE128 —
    are tn_ref.ALT, checked on the CPU by test_tn_ref_host.py::test_alternate_switch_table."""
    sel = "(test_exact_tern or test_random) and (" + " or ".join(T.ALT_CASES) + ")"
    env = {k: v for k, v in os.environ.items() if not k.startswith("SAIS_TN_")}
    env.update(kv.split("=") for kv in switches.split())
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-k", sel], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    nrandom = len(set(T.ALT_CASES) & set(T.ONE_PER_FORM))
    m = re.search(r"(\d+) passed", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) == len(T.ALT_CASES) + nrandom, r.stdout[-2500:] + r.stderr[-500:]
    ratios = re.findall(r"^(\w+) \((\w+)\): dW (\S+) of the bar, db (\S+) of the bar", r.stdout, flags=re.M)
    assert len(ratios) == nrandom and {form for _, form, _, _ in ratios} <= {f for f, _, _ in T.ALT[switches].values()}, r.stdout[-2500:]
    for _, form, rw, rb in ratios:                       # the child's session has its own log: carry its figures into this one
        parity.parity_log(f"tn_edge_{form.lower()}_dW", float(rw), 1.0)
        parity.parity_log(f"tn_edge_{form.lower()}_db", float(rb), 1.0)


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections(ops, L):
    """every entry returns SAIS_ERR_ARG before any launch and leaves dW / db bit-unchanged; the same arguments without the defect
    are accepted (so each refusal is that of the defect)"""
    lib, st = L.load(), _stream()
    M, SENT = 65, 7.0
    ptr = lambda t: t.data_ptr()
    src = {False: torch.ones(M + 64, 512, dtype=torch.bfloat16, device=DEV), True: torch.ones(M + 64, 512, device=DEV)}
    dW, db = torch.full((256, 256), SENT, device=DEV), torch.full((256,), SENT, device=DEV)
    dW_ok, db_ok = torch.zeros(256, 256, device=DEV), torch.zeros(256, device=DEV)

    def item(f32, ok=False, **kw):
        d = dict(P=ptr(src[f32]), ldp=512, Q=ptr(src[f32]), ldq=512, N1=256, N2=128, dW=ptr(dW_ok if ok else dW), ldw=256,
                 db=ptr(db_ok if ok else db))
        d.update(kw)
        return L.SaisTnItem(**d)

    def grouped(entry, items, n=None, M_=M, nsplit=1):
        arr = (L.SaisTnItem * max(1, len(items)))(*items) if items is not None else None
        n = len(items) if n is None else n
        extra = (None, 0) if entry == "sais_gemm_tn_grouped_ws" else ()
        return getattr(lib, entry)(arr, n, M_, nsplit, *extra, st)

    def single(entry, f32, ok=False, M_=M, nsplit=1, **kw):
        it = item(f32, ok, **kw)
        return getattr(lib, entry)(it.P, it.ldp, it.Q, it.ldq, M_, it.N1, it.N2, it.dW, it.ldw, it.db, nsplit, st)

    item_defects = {False: dict(N1=192, N2=192, ldp=516, ldq=516, P=None, Q=None, dW=None),        # ld % 8 != 0
                    True: dict(N1=192, N2=192, ldp=514, ldq=514, P=None, Q=None, dW=None)}         # ld % 4 != 0
    for entry, f32 in (("sais_gemm_tn_grouped", False), ("sais_gemm_tn_grouped_ws", False), ("sais_gemm_tn_grouped_f32", True)):
        assert grouped(entry, [item(f32, ok=True)]) == 0, entry
        for field, bad in item_defects[f32].items():
            assert grouped(entry, [item(f32, **{field: bad})]) == ERR_ARG, (entry, field)
            assert grouped(entry, [item(f32), item(f32, **{field: bad})]) == ERR_ARG, (entry, field, "second item")
        assert grouped(entry, [item(f32)], n=0) == ERR_ARG and grouped(entry, None, n=1) == ERR_ARG, entry
        assert grouped(entry, [item(f32)] * (L.TN_MAX_ITEMS + 1)) == ERR_ARG, (entry, "49 items")
        assert grouped(entry, [item(f32)], nsplit=0) == ERR_ARG and grouped(entry, [item(f32)], M_=0) == ERR_ARG, entry
    for entry, f32 in (("sais_gemm_tn", False), ("sais_gemm_tn_f32", True)):
        assert single(entry, f32, ok=True) == 0, entry
        for field, bad in item_defects[f32].items():
            assert single(entry, f32, **{field: bad}) == ERR_ARG, (entry, field)
        assert single(entry, f32, nsplit=0) == ERR_ARG and single(entry, f32, M_=0) == ERR_ARG, entry
    with pytest.raises(L.SaisHipError):                                                   # and through the wrapper: it raises
        ops.gemm_tn_grouped([(src[False][:M, :192], src[False][:M, :384], dW[:192, :], None)], M)

    # the slab workspace of BLOCK at M = 15 360 (XL_SLAB, 10 splits): a pointer that is not 16-B aligned, an offer one byte short
    if _sw() == "":
        Mx = 15360
        big = torch.ones(Mx, 1536, dtype=torch.bfloat16, device=DEV)
        outs = [torch.full((n1, n2), SENT, device=DEV) for n1, n2 in T.BLOCK]
        arr = (L.SaisTnItem * 4)(*[L.SaisTnItem(P=ptr(big), ldp=1536, Q=ptr(big), ldq=1536, N1=n1, N2=n2, dW=ptr(o), ldw=n2, db=None)
                                   for (n1, n2), o in zip(T.BLOCK, outs)])
        need = lib.sais_gemm_tn_grouped_slab_bytes(arr, 4, Mx)
        assert need == 240 * (192 * 384 * 4 + 4 * 32 * 32 * 4)
        ws = torch.empty(need + 64, dtype=torch.uint8, device=DEV)
        assert ws.data_ptr() % 16 == 0
        assert lib.sais_gemm_tn_grouped_ws(arr, 4, Mx, 4, ctypes.c_void_p(ws.data_ptr() + 4), need, st) == ERR_ARG
        assert lib.sais_gemm_tn_grouped_ws(arr, 4, Mx, 4, ctypes.c_void_p(ws.data_ptr()), need - 1, st) == ERR_ARG
        torch.cuda.synchronize()
        assert all(bool((o == SENT).all()) for o in outs)
    torch.cuda.synchronize()
    assert bool((dW == SENT).all()) and bool((db == SENT).all())
    assert float(dW_ok[0, 0]) == 5 * M and float(db_ok[0]) == 5 * M                       # the five accepted launches did run
