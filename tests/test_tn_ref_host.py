"""The exact-data recipes of tests/tn_ref.py hold at every shape test_tn_edges_gpu.py runs, and every case of its lists takes the
launch form written beside it (CPU only).  Each case carries its form, M-splits and rows per split by hand; here they are held
against the library's own plan query (sais_gemm_tn_plan_: the function the size query and the launches call; a child process per
switch setting, the switches are read once per process) and against the rules restated in tn_ref.py, so a list that drifts off its
form fails here instead of passing on another kernel on the GPU.  This file run as a script with --plan-child is that child."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import tn_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE, SLAB_BYTES_15360 = 4096, 240 * (192 * 384 * 4 + 4 * 32 * 32 * 4)       # an aligned stand-in pointer; BLOCK's XL slabs at 10 splits

# plan only (nothing is launched at such a base): name -> (items, M, P / Q base pointer, offer) -> return code, plan by hand
EXTRA = {
    "aligned16": ((T.BLOCK, 15360, BASE, T.ENOUGH), (0, ("XL_SLAB", 10, 1536))),
    "aligned8": ((T.BLOCK, 15360, BASE + 8, T.ENOUGH), (0, ("WIDE_ATOMIC", 7, 2240))),         # 8-B aligned only: leaves the XL form
    "exact_offer": ((T.BLOCK, 15360, BASE, SLAB_BYTES_15360), (0, ("XL_SLAB", 10, 1536))),
    "short_offer": ((T.BLOCK, 15360, BASE, SLAB_BYTES_15360 - 1), (-1, ("XL_ATOMIC", 10, 1536))),   # refused: one byte short
}


def _queries(switches):
    """[(key, items, M, nsplit, offer, f32, base pointer)] of one child"""
    if switches:
        return [(n, T.BY_NAME[n].items, T.BY_NAME[n].M, T.case_query(T.BY_NAME[n])[0], T.ENOUGH, 0, BASE) for n in T.ALT_CASES]
    rows = [(c.name, c.items, c.M) + T.case_query(c) + (int(c.f32), BASE) for c in T.ALL_CASES]
    return rows + [(k, items, M, T.default_nsplit(M, items), offer, 0, ptr) for k, ((items, M, ptr, offer), _) in EXTRA.items()]


def _plan_child(switches):
    sys.path.insert(0, ROOT)
    from sais_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    got = {}
    for key, shapes, M, nsplit, offer, f32, ptr in _queries(switches):
        items = (_lib.SaisTnItem * len(shapes))()
        for it, (n1, n2) in zip(items, shapes):
            it.P, it.Q, it.dW, it.N1, it.N2, it.ldp, it.ldq, it.ldw = ptr, ptr, BASE, n1, n2, n1, n2, n2
        rc, plan, wg, slab = T.plan_query(lib, items, len(shapes), M, nsplit, offer, f32)
        got[key] = [rc, list(plan), wg, slab]
    print(json.dumps(got))


_ANSWERS = {}


def answers(switches):
    """what the library's plan query says in a process with `switches` set, per query key"""
    if switches not in _ANSWERS:
        import __graft_entry__ as ge
        from sais_amd import _lib
        if not os.path.exists(_lib.LIB_PATH):
            ge.build()
        env = {k: v for k, v in os.environ.items() if not k.startswith("SAIS_TN_")}
        env.update(kv.split("=") for kv in switches.split())
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plan-child", switches], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
        _ANSWERS[switches] = {k: (v[0], tuple(v[1]), v[2], v[3]) for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()}
    return _ANSWERS[switches]


# ------------------------------------------------------------------------------------------------ recipes
@pytest.mark.parametrize("recipe", T.RECIPES)
def test_exactness_bound_at_every_case(recipe):
    """evaluated on the bound max|p| max|q| M calls + max|dW0| (in units of 1 or 1/4), not on the data: below 2^24 at every M"""
    cases = T.F32_CASES if recipe == "f32_round" else T.ALL_CASES
    worst = max(T.exact_bound(recipe, c.M) for c in cases)
    print(f"{recipe}: largest bound {worst:.0f} = 2^{torch.log2(torch.tensor(worst)).item():.1f} over {len(cases)} cases")
    assert worst < 2 ** 24 and max(c.M for c in T.ALL_CASES) == 16320
    assert T.exact_bound("tern", 16320) == 2 * 3 * 16320 * 2 + 5 and T.exact_bound("pow2", 16320) == 4 * (2 * 2 * 16320 * 2 + 5)


@pytest.mark.parametrize("recipe,f32", [("tern", False), ("tern", True), ("pow2", False), ("f32_round", True)])
def test_recipe_conditions_on_data(recipe, f32):
    """the value sets, the asymmetry of tern, the rounding claims of f32_round, and an f32 chain over the rows in three orders equal
    to the fp64 reference bit for bit"""
    M, n1, n2 = 333, 128, 256
    p, pm = T.operand(recipe, "p", M, n1, 5, "cpu", f32)
    q, qm = T.operand(recipe, "q", M, n2, 6, "cpu", f32)
    assert T.operand_condition(recipe, p, pm) and T.operand_condition(recipe, q, qm)
    assert p.dtype == (torch.float32 if f32 else torch.bfloat16)
    if recipe == "tern":
        assert set(pm.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0} and set(qm.unique().tolist()) == set(map(float, range(-3, 4)))
    if recipe == "pow2":
        assert set(pm.unique().tolist()) == set(T.POW2_VALUES)
    if recipe == "f32_round":
        x = torch.tensor([1 - 2.0 ** -10, 2 + 2.0 ** -8, -1 - 2.0 ** -9])
        assert T.truncate_bf16(x).tolist() == [1 - 2.0 ** -8, 2.0, -1.0] and x.to(torch.bfloat16).tolist() == [1.0, 2.0, -1.0]
        assert not T.operand_condition(recipe, pm.float(), pm)              # data that IS bf16 does not satisfy the recipe
    ref = pm.t() @ qm
    assert T.reference_condition(recipe, ref, M, 1) and not torch.equal(ref[:128, :128], ref[:128, :128].t())
    rd = lambda t: t.to(torch.bfloat16).float()
    for order in (list(range(M)), list(range(M))[::-1], torch.randperm(M, generator=torch.Generator().manual_seed(1)).tolist()):
        acc = torch.zeros(n1, n2)
        for chunk in torch.tensor(order).split(37):
            acc = acc + rd(p[chunk]).t() @ rd(q[chunk])
        assert torch.equal(acc.double(), ref)


# ------------------------------------------------------------------------------------------------ plans
def test_case_lists_take_their_forms():
    """every case: the hand-written (form, M-splits, rows per split) == the library's plan == the restated rules"""
    got = answers("")
    for c in T.ALL_CASES:
        nsplit, _ = T.case_query(c)
        rc, plan, wg, slab = got[c.name]
        restated = T.plan_f32(c.items, c.M, nsplit) if c.f32 else T.plan_bf16(c.items, c.M, nsplit, slabs=c.entry != "null_slabs")
        want = (c.form, c.ns, c.rows)
        if c.form is None:                                   # the single fp32 entry: tn_split alone
            plan, restated = (None,) + plan[1:], (None,) + restated[1:]
        assert rc == 0 and plan == want == restated, (c.name, rc, plan, want, restated)
        assert (slab > 0) == (c.form in T.SLAB_FORMS), (c.name, slab)
        if c.form == "TILE128" and c.entry == "grouped":
            assert wg == c.ns * sum((a // 128) * (b // 128) for a, b in c.items)
    # what the table of the issue names
    assert T.BY_NAME["t128_grouped_m65_s5"][-2:] == (2, 64) and T.BY_NAME["t128_grouped_m129_s5"][-2:] == (3, 64)
    assert 8192 - 6 * 1216 == 896 and got["xla_blk11_m8192"][2] == 264 > T.TN_ONE_ROUND and got["xla_blk6kv_m8224"][2] == 148
    assert got["f32_own128_m65"][2] == 264 and got["f32_own64_m65"][2] == 264 and got["f32_own64_one_tile_m65"][2] == 2


def test_boundary_m_takes_three_kernels():
    """15 296 (478 steps over 10 splits: 47 each, refused), 15 328 (479: refused, and no whole number of 64-row steps) and 15 360 (48)"""
    got = answers("")
    assert [got[n][1][0] for n in ("wide_blk_m15296", "t128_blk_m15328", "xl_blk_m15360")] == ["WIDE_ATOMIC", "TILE128", "XL_SLAB"]
    assert (15296 // 32 // 10, 15328 // 32 // 10, 15360 // 32 // 10) == (47, 47, 48) == (T.XL_MIN_STEPS - 1,) * 2 + (T.XL_MIN_STEPS,)


@pytest.mark.parametrize("switches", T.SWITCHES)
def test_alternate_switch_table(switches):
    """the forms the GPU children expect for BLOCK at M = 8192, 15 296, 15 360, 15 392 under each switch"""
    got = answers(switches)
    for n in T.ALT_CASES:
        c = T.BY_NAME[n]
        want = T.expected_plan(c, switches)
        assert got[n][0] == 0 and got[n][1] == want == T.plan_bf16(c.items, c.M, None, switches=switches), (switches, n, got[n], want)
    forms = {got[n][1][0] for n in T.ALT_CASES}
    assert forms == {"SAIS_TN_SLABS=1": {"WIDE_SLAB", "TILE128"}, "SAIS_TN_XL=0": {"WIDE_ATOMIC", "TILE128"},
                     "SAIS_TN_XL_SLABS=0": {"WIDE_ATOMIC", "XL_ATOMIC"}}[switches]
    with pytest.raises(AssertionError):
        T.expected_plan(T.BY_NAME["t128_blk_m8249"], switches)                 # a case outside the table must not run under a switch


def test_lists_cover_every_form_and_ring_residue():
    got = answers("")
    forms = {got[c.name][1][0] for c in T.ALL_CASES} | {answers("SAIS_TN_SLABS=1")[n][1][0] for n in T.ALT_CASES}
    print("forms:", sorted(forms))
    assert forms == set(T.TN_FORMS) and len(T.TN_FORMS) == 8
    assert {got[n][1][0] for n in T.ONE_PER_FORM} == set(T.TN_FORMS) - {"WIDE_SLAB"}
    residues = set()
    for c in T.XL_SLAB:
        steps = T.xl_steps(c.M, c.ns)
        assert sum(steps) * 32 == c.M and min(steps) * 32 == c.rows and min(steps) >= T.XL_MIN_STEPS
        assert {s % T.XL_RING for s in steps} == T.XL_RESIDUES[c.name], (c.name, steps)
        residues |= T.XL_RESIDUES[c.name]
    print("XL steps per split mod 4:", sorted(residues))
    assert residues == {0, 1, 2, 3}
    assert T.xl_steps(8192, 3) == [86, 85, 85] and T.xl_steps(8224, 2) == [129, 128] and T.xl_steps(15392, 10) == [49] + [48] * 9
    # every list has an item without db and one with; N2 = 384 and N2 = 1536 both carry one (db is absent iff N1 == N2)
    for lst in (T.TILE128_SMALL, T.TILE128_LARGE, T.WIDE_ATOMIC, T.XL_SLAB, T.XL_ATOMIC, T.F32):
        shapes = {s for c in lst for s in c.items}
        assert any(a == b for a, b in shapes) and any(a != b for a, b in shapes)
    assert {(1536, 384), (384, 1536)} <= set(T.BLOCK)


def test_alignment_and_short_offer_plans():
    """plan only: a P / Q base that is 8-B but not 16-B aligned leaves the XL form; an offer one byte short is refused"""
    got = answers("")
    for key, (_, (rc, plan)) in EXTRA.items():
        assert got[key][0] == rc and got[key][1] == plan, (key, got[key])
    assert got["exact_offer"][3] == SLAB_BYTES_15360 == got["xl_blk_m15360"][3] and got["short_offer"][3] == 0
    assert T.plan_bf16(T.BLOCK, 15360, aligned16=False) == EXTRA["aligned8"][1][1]
    hdr = open(os.path.join(ROOT, "include", "sais_hip.h")).read()
    assert "P and Q must be 16-B aligned" in hdr


# ------------------------------------------------------------------------------------------------ the checks notice
def _verdict(case_name, recipe, mutate):
    c = T.BY_NAME[case_name]
    ops_ = T.Operands(c.items, c.M, recipe, c.f32, c.entry, "cpu")
    outs = T.Outputs(c.items, "cpu")
    items = T.launch_items(c.items, ops_, outs)
    try:
        for k in (1, 2):
            T.model_launch(items, c.M, c.rows, mutate=mutate)
            outs.check(c.items, ops_, k)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("mutate,case_name,recipe", [
    ("unmasked_tail", "t128_grouped_m65_s2", "tern"),          # the one-row second step reads 63 NaN rows
    ("drop_last_step", "t128_grouped_m129_s1", "tern"),
    ("bias_twice", "t128_grouped_m65_s2", "pow2"),
    ("transposed_store", "t128_grouped_m63_s1", "tern"),       # the (128, 128) item: P != Q, so P^T Q is not symmetric
    ("border_written", "t128_grouped_m1_s1", "tern"),
    ("truncate", "f32_own64_one_tile_m65", "f32_round"),
])
def test_the_gpu_checks_notice(mutate, case_name, recipe):
    """the launch restated in fp64 torch (tn_ref.model_launch) passes the GPU test's own check (Outputs.check, one call and two) on a
    named case of the lists, and fails it with the error put in"""
    assert _verdict(case_name, recipe, None)
    assert not _verdict(case_name, recipe, mutate)


def test_views_are_what_the_issue_asks():
    c = T.BY_NAME["t128_grouped_m65_s2"]
    ops_ = T.Operands(c.items, c.M, "tern", False, "grouped", "cpu")
    views = [t for p, q, _, _ in ops_.by_shape.values() for t in (p, q)]
    for t, buf in zip(views, ops_.buffers):
        assert t.stride(0) == buf.shape[1] > t.shape[1] and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0 and t.data_ptr() % 128 != 0
        assert buf.shape[0] == c.M + T.ROWS_BEHIND and bool(torch.isnan(buf[c.M:]).all())
        assert int(torch.isnan(buf).sum()) == buf.numel() - t.numel()                 # NaN everywhere but inside the view
    f = T.Operands(((128, 128),), 65, "f32_round", True, "grouped", "cpu")
    p, q, _, _ = f.by_shape[(128, 128)]
    assert p.stride(0) % 4 == 0 and p.stride(0) % 8 != 0 and q.stride(0) % 8 != 0           # the grouped fp32 entry takes ld % 4
    s = T.Operands(T.ONE, 65, "f32_round", True, "single", "cpu").by_shape[(256, 128)]
    assert s[0].stride(0) % 8 == 0 and s[1].stride(0) % 8 == 0
    outs = T.Outputs(c.items, "cpu")
    assert [o["db"] is None for o in outs.items] == [False, False, True]
    assert all(o["dW"].stride(0) == o["dW"].shape[1] + 2 * T.DW_BORDER and o["dW"].storage_offset() == T.DW_BORDER for o in outs.items)
    assert len({o["dW"].data_ptr() for o in T.Outputs(T.BLOCK * 3, "cpu").items}) == 12        # items never share dW
    assert len(T.Operands(T.BLOCK * 3, 64, "tern", False, "grouped", "cpu").by_shape) == 4       # repeated shapes share P / Q


if __name__ == "__main__" and "--plan-child" in sys.argv:
    _plan_child(sys.argv[-1])
