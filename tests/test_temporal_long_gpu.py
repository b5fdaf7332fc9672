"""The streaming temporal attention (csrc/tattn_long.hip) and the encoder past 96 tokens on a real MI355X.

Kernel level: references are fp64 (tests/temporal_long_ref.py, which restates the bounds of temporal_ref.py for S > 96 and
which test_temporal_long_host.py proves sound and sharp on the CPU); every output buffer is oversized and NaN-filled: what a
kernel owns must be non-NaN and inside its bar, everything else must still be NaN.  The map needs no pre-zeroing and is
bit-reproducible (fixed-order head sum), as are ctx and dqkv.  Model level: the reference's own outputs
(tests/golden/temporal_long.npz, written by tests/golden/make_golden_temporal_long.py) under the bars of test_model_gpu.py,
gradients against fp64 autograd of the oracle with the exported dropout masks and the forward's ReLU gates.
Worst observed / bar ratios go to parity.parity_log("temporal_long_...")."""
import functools
import math

import numpy as np
import pytest
import torch

import parity
import synth
import temporal_long_ref as LR
import temporal_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
LOGIT_TOL, ATTN_TOL, FEAT_REL, GRAD_REL = 1e-3, 2e-3, 2e-2, 4e-2          # the bars of test_model_gpu.py / test_dropout_gpu.py


@pytest.fixture(scope="module")
def ops():
    from sais_amd import ops as o
    return o


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def log(name, value, bar):
    value, bar = float(value), float(bar)
    r = value / bar if bar > 0 else (0.0 if value == 0 else float("inf"))
    r = r if math.isfinite(r) else float("inf")
    parity.parity_log("temporal_long_" + name, r, 1.0)
    return r


def guarded(n, *tail):
    """a NaN buffer with 3 guard rows in front of and behind the n rows handed to the kernel -> (whole, the n rows)"""
    whole = nan(n + 6, *tail)
    return whole, whole[3:n + 3]


def inside(whole, n):
    assert torch.isnan(whole[:3]).all() and torch.isnan(whole[n + 3:]).all(), "wrote outside its rows"
    assert torch.isfinite(whole[3:n + 3]).all(), "left NaN / inf in what it owns"
    return whole[3:n + 3]


def _fwd(ops, qkv, padu, S, want_avg, p=0.0, rng=None, site=0, fn=None):
    B = padu.shape[0]
    wc, ctx = guarded(B * S, 384)
    wa, avg = guarded(B, S, S) if want_avg else (None, None)
    (fn or ops.temporal_attn_fwd_long)(qkv, padu, B, S, ctx, avg, p, rng, site)
    return inside(wc, B * S), inside(wa, B) if want_avg else None


def _bwd(ops, qkv, padu, S, dctx, p=0.0, rng=None, site=0):
    B = padu.shape[0]
    wd, dqkv = guarded(B * S, 1152)
    ops.temporal_attn_bwd_long(qkv, padu, B, S, dctx, dqkv, p, rng, site)
    return inside(wd, B * S)


def _check_fwd(tag, name, got, ref):
    ratios = LR.attn_ratios_long({k: v.cpu() for k, v in got.items()}, ref)
    rs = {k: log(f"fwd_{k}_{tag}", v, LR.fwd_bar_long(name, k)) for k, v in ratios.items()}
    print(f"{tag}: " + ", ".join(f"{k} {v:.3f} of the bar" for k, v in rs.items()))
    assert all(r <= 1.0 for r in rs.values()), (tag, rs)


def _check_bwd(tag, got, ref, bars, pad):
    rel = R.rel_l2_parts(got.cpu(), ref)
    rs = [log(f"bwd_{part}_{tag}", g, b) for part, g, b in zip(("dq", "dk", "dv"), rel, bars)]
    print(f"{tag}: " + ", ".join(f"{part} {g:.3e} (bar {b:.3e})" for part, g, b in zip(("dq", "dk", "dv"), rel, bars)))
    assert all(r <= 1.0 for r in rs), (tag, rel, bars)
    B, S = pad.shape
    if pad.any():
        assert float(got.cpu().view(B, S, 3, 384)[:, :, 1:][pad].abs().max()) == 0.0, "dk / dv of a masked key"


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", R.LAYOUTS)
@pytest.mark.parametrize("S", LR.S_LONG)
def test_attn_fwd_long(ops, S, name):
    """one pass without the map and two passes with it, every layout at every tile edge and at the cap"""
    assert LR.tiles(S) == (S + 63) // 64
    qkv, pad, ref = LR.fwd_ref(name, S)
    qd, padu = qkv.to(DEV), pad.to(torch.uint8).to(DEV)
    ctx, avg = _fwd(ops, qd, padu, S, True)
    ctx1, none = _fwd(ops, qd, padu, S, False)
    assert none is None
    _check_fwd(f"{name}_S{S}", name, dict(avg=avg, ctx=ctx, ctx1=ctx1), ref)
    if pad.any():
        assert float(avg.cpu()[pad[:, None, :].expand(-1, S, -1)].abs().max()) == 0.0
    ctx_b, avg_b = _fwd(ops, qd, padu, S, True)                 # bit-reproducible, the map included: no atomics
    assert torch.equal(ctx_b, ctx) and torch.equal(avg_b, avg)
    assert torch.equal(_fwd(ops, qd, padu, S, False)[0], ctx1)


@pytest.mark.parametrize("S,p,site", LR.DROP_CASES_LONG)
def test_attn_long_dropout(ops, S, p, site):
    """the keep mask is the library's own (sais_dropout_mask at the same state and site), element ((b 4 + h) S + i) S + j;
    forward (both forms) and backward draw it; a second site draws another"""
    qkv, pad, dctx = LR.bwd_case_long("rand", S)
    qd, padu, dd = qkv.to(DEV), pad.to(torch.uint8).to(DEV), dctx.to(DEV)
    B = pad.shape[0]
    rng = ops.rng_state(1234 + S, DEV)
    keep = ops.dropout_mask(B * 4 * S * S, p, rng, site, DEV).view(B, 4, S, S).bool()
    frac = float(keep.float().mean())
    assert abs(frac - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / keep.numel()), frac
    ref = LR.attn_fp64_long(qkv, pad, keep.cpu(), p)
    ctx, avg = _fwd(ops, qd, padu, S, True, p, rng, site)
    ctx1, _ = _fwd(ops, qd, padu, S, False, p, rng, site)
    _check_fwd(f"rand_S{S}_p{p}_site{site}", "rand", dict(avg=avg, ctx=ctx, ctx1=ctx1), ref)
    dropped = ~keep.cpu().any(1)                                # an entry every head dropped is exactly 0 in the map
    assert float(avg.cpu()[dropped].abs().max() if dropped.any() else 0.0) == 0.0
    got = _bwd(ops, qd, padu, S, dd, p, rng, site)
    _check_bwd(f"rand_S{S}_p{p}_site{site}", got, R.attn_bwd_fp64(qkv, pad, dctx, keep.cpu(), p), LR.bwd_bars_long("rand", S, p), pad)
    assert torch.equal(_bwd(ops, qd, padu, S, dd, p, rng, site), got)
    other = ops.dropout_mask(B * 4 * S * S, p, rng, 7 - site, DEV).view(B, 4, S, S).bool()
    assert not torch.equal(other, keep)
    assert not torch.equal(_fwd(ops, qd, padu, S, False, p, rng, 7 - site)[0], ctx1)


# ------------------------------------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=None)
def _plain_ref(name, S):
    qkv, pad, dctx = LR.bwd_case_long(name, S)
    return R.attn_bwd_fp64(qkv, pad, dctx)


@pytest.mark.parametrize("name", R.BWD_LAYOUTS)
@pytest.mark.parametrize("S", LR.S_LONG)
def test_attn_bwd_long(ops, S, name):
    """dctx plain and as three raw slabs a gapped stride apart (NaN in the gaps), each against fp64 autograd on what it holds"""
    qkv, pad, dctx = LR.bwd_case_long(name, S)
    qd, padu = qkv.to(DEV), pad.to(torch.uint8).to(DEV)
    M = pad.shape[0] * S
    bars = LR.bwd_bars_long(name, S)
    got = _bwd(ops, qd, padu, S, dctx.to(DEV))
    _check_bwd(f"{name}_S{S}_plain", got, _plain_ref(name, S), bars, pad)
    assert torch.equal(_bwd(ops, qd, padu, S, dctx.to(DEV)), got)
    _, _, buf, _, ref3 = LR.bwd_ref(name, S)
    bufd = buf.to(DEV)
    slabs = R.slab_view(bufd, M)
    assert slabs.stride(0) == M * 384 + 64 and slabs.data_ptr() == bufd.data_ptr()
    g3 = _bwd(ops, qd, padu, S, slabs)
    _check_bwd(f"{name}_S{S}_slabs3", g3, ref3, bars, pad)
    assert torch.isnan(bufd[:, M * 384:]).all()


# ------------------------------------------------------------------------------------------------ the two forms agree
@pytest.mark.parametrize("S", (33, 96))
def test_long_and_resident_forms_agree(ops, S):
    """the same inputs through tattn.hip and tattn_long.hip: they sum in different orders, so not bit-equal, but each is inside
    its own bar of its own bound around the same fp64 values, hence within the sum of both of each other"""
    pad = R.masks(S)
    qkv = R.layouts("rand", pad, R.case_seed("rand", S))
    qd, padu = qkv.to(DEV), pad.to(torch.uint8).to(DEV)
    B = pad.shape[0]
    rs, rl = R.attn_fp64(qkv, pad), LR.attn_fp64_long(qkv, pad)
    ctx_l, avg_l = _fwd(ops, qd, padu, S, True)
    ctx_s, avg_s = _fwd(ops, qd, padu, S, True, fn=ops.temporal_attn_fwd)
    tol_ctx = R.fwd_bar("rand", "ctx") * R.ctx_bound(rs) + LR.fwd_bar_long("rand", "ctx") * LR.ctx_bound_long(rl)
    tol_avg = R.fwd_bar("rand", "avg") * R.avg_bound(rs) + LR.fwd_bar_long("rand", "avg") * R.avg_bound(rl)
    r_ctx = log(f"agree_ctx_S{S}", float(((ctx_l - ctx_s).cpu().double().abs() / tol_ctx).max()), 1.0)
    r_avg = log(f"agree_avg_S{S}", float(((avg_l - avg_s).cpu().double().abs() / tol_avg).max()), 1.0)
    assert r_ctx <= 1.0 and r_avg <= 1.0, (r_ctx, r_avg)
    _, _, dctx = R.bwd_case("rand", S)
    dd = dctx.to(DEV)
    g_l = _bwd(ops, qd, padu, S, dd)
    g_s = nan(B * S, 1152)
    ops.temporal_attn_bwd(qd, padu, B, S, dd, g_s)
    ref = R.attn_bwd_fp64(qkv, pad, dctx)
    for i, (part, bs, bl) in enumerate(zip(("dq", "dk", "dv"), R.bwd_bars("rand", S), LR.bwd_bars_long("rand", S))):
        sl = slice(384 * i, 384 * (i + 1))
        d = float((g_l[:, sl] - g_s[:, sl]).double().norm()) / float(ref[:, sl].norm())
        assert log(f"agree_{part}_S{S}", d, bs + bl) <= 1.0, (part, d, bs, bl)


# ------------------------------------------------------------------------------------------------ rejections
def test_long_rejections_launch_nothing(ops):
    from sais_amd._lib import SaisHipError
    S, B = 97, 2
    pad = torch.zeros(B, S, dtype=torch.uint8, device=DEV)
    qkv = torch.randn(B * 2002, 1152, device=DEV)
    dctx = torch.randn(2, B * S * 384 + 2, device=DEV)
    rng = ops.rng_state(5, DEV)
    ctx, avg, dqkv = nan(B * 2002, 384), nan(B, S, S), nan(B * 2002, 1152)
    pad_big = torch.zeros(B, 2002, dtype=torch.uint8, device=DEV)
    need = ops.temporal_attn_long_bwd_workspace_bytes(B, S)
    assert need == LR.bwd_workspace_bytes(B, S) and ops.temporal_attn_long_bwd_workspace_bytes(B, 2002) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    plain = dctx[0, :B * S * 384].view(B * S, 384)
    bad = [
        lambda: ops.temporal_attn_fwd_long(qkv, pad, B, 0, ctx, avg),
        lambda: ops.temporal_attn_fwd_long(qkv, pad_big, B, 2002, ctx, None),
        lambda: ops.temporal_attn_fwd_long(qkv, pad, B, S, ctx, avg, 1.0, rng, 0),
        lambda: ops.temporal_attn_fwd_long(qkv, pad, B, S, ctx, avg, 0.1, None, 0),
        lambda: ops.temporal_attn_bwd_long(qkv, pad, B, 0, plain, dqkv, ws=ws),
        lambda: ops.temporal_attn_bwd_long(qkv, pad_big, B, 2002, plain, dqkv, ws=ws),
        lambda: ops.temporal_attn_bwd_long(qkv, pad, B, S, plain, dqkv, 1.0, rng, 0, ws=ws),
        lambda: ops.temporal_attn_bwd_long(qkv, pad, B, S, plain, dqkv, 0.1, None, 0, ws=ws),
        lambda: ops.temporal_attn_bwd_long(qkv, pad, B, S, torch.as_strided(dctx, (2, B * S, 384), (B * S * 384 + 2, 384, 1)), dqkv, ws=ws),
        lambda: ops.temporal_attn_bwd_long(qkv, pad, B, S, plain, dqkv, ws=ws[:need - 1]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(SaisHipError):
            call()
        torch.cuda.synchronize()
        assert torch.isnan(ctx).all() and torch.isnan(avg).all() and torch.isnan(dqkv).all(), i
    ops.temporal_attn_bwd_long(qkv, pad, B, S, plain, dqkv, ws=ws)              # the exact size is enough
    assert torch.isfinite(dqkv[:B * S]).all() and torch.isnan(dqkv[B * S:]).all()


# ------------------------------------------------------------------------------------------------ model
def _model(modal="RGB-Flow", p=0.0, train=False):
    from sais_amd.temporal import fullModel
    m = fullModel('reps', 2, 'in_vs_out', 384, 'ViT', modalities=modal)
    m.load_state_dict(synth.temporal_state_dict(seed=1), strict=True)
    m.dropout_p = p
    m = m.to(DEV)
    return m.train() if train else m.eval()


def _inputs(lens, seeds):
    B, T = len(lens), max(lens)
    x, f = synth.reps(seed=seeds[0], B=B, T=T), synth.reps(seed=seeds[1], B=B, T=T)
    for b, n in enumerate(lens):
        x[b, :, n:] = 0
        f[b, :, n:] = 0
    return x, f, synth.padding_mask(lens)


def maxabs(a, b):
    return float(np.abs(a.detach().float().cpu().numpy() - np.asarray(b)).max())


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-12))


def test_layer_calls_equal_the_per_launch_path(ops):
    """sais_temporal_layer_fwd / _bwd at (B, S) = (2, 131) pick the streaming kernels and issue the launches of the per-launch
    Python path: embeddings, loss and the map bit for bit (the map too: no atomics here), gradients as the existing layer-call
    test holds them (the deferred dW launch groups the layers' GEMMs differently)."""
    import sais_amd.temporal as TM
    from sais_amd.loss import calcNCELoss
    lens = [130, 97]
    x, f, pad = _inputs(lens, (910, 911))
    lab = synth.labels(seed=912, B=2)

    def run(layer_calls):
        old = TM._LAYER_CALLS
        TM._LAYER_CALLS = layer_calls
        try:
            m = _model("RGB", 0.1, train=True)
            m.dropout_seed = 31
            xg = x.to(DEV).requires_grad_(True)
            protos = torch.nn.ParameterDict({k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in synth.prototypes(2, 2).items()})
            emb, attn = m(xg, None, lens, lens, 'Prototypes', pad.to(DEV), None, None)
            loss = calcNCELoss(0, emb, lab, ["v0", "v1"], protos, None)
            loss.backward()
            return emb.detach(), attn.detach(), float(loss.detach()), m.flat.grad.clone(), xg.grad.clone()
        finally:
            TM._LAYER_CALLS = old

    a, b = run(True), run(False)
    assert tuple(a[1].shape) == (2, 131, 131)
    assert torch.equal(a[0], b[0]) and a[2] == b[2] and torch.equal(a[1], b[1])
    assert float(b[3].abs().max()) > 0
    for u, v in zip(a[3:], b[3:]):
        assert float((u - v).norm() / v.norm()) <= 1e-6


GOLDEN_CASES = (("RGB-Flow", "r130_97", [130, 97]), ("RGB", "r96", [96]), ("Flow", "r100", [100]), ("RGB-Flow", "r2000", [2000]))
MAP_ROWS = (0, 1, 1000, 2000)


@pytest.mark.parametrize("modal,cname,lens", GOLDEN_CASES)
def test_long_forward_vs_golden(ops, golden, modal, cname, lens):
    """the reference's own fullModel on the CPU (make_golden_temporal_long.py) under the bars of test_model_gpu.py"""
    from oracle import sais_oracle as O
    from sais_amd.loss import cosine_logits_and_probs
    g = golden("temporal_long")
    key = f"{modal}/{cname}/"
    T = max(lens)
    x, f, pad = _inputs(lens, (100 + T, 200 + T))
    m = _model(modal)
    use_x, use_f = modal != "Flow", modal != "RGB"
    with torch.no_grad():
        emb, attn = m(x.to(DEV) if use_x else None, f.to(DEV) if use_f else None, lens, lens, 'Prototypes',
                      pad.to(DEV) if use_x else None, pad.to(DEV) if use_f else None, None)
    ref = g[key + "emb"]
    e = log(f"golden_emb_{cname}", maxabs(emb, ref), FEAT_REL * np.abs(ref).max())
    got_map = attn[:, list(MAP_ROWS)] if T == 2000 else attn
    a = log(f"golden_attn_{cname}", maxabs(got_map, g[key + "attn"]), ATTN_TOL)
    protos = torch.nn.ParameterDict({k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in synth.prototypes(2, 2).items()})
    sim, _ = cosine_logits_and_probs(emb, protos)
    s = log(f"golden_logits_{cname}", maxabs(sim, O.cosine_logits(torch.from_numpy(ref), synth.prototypes(2, 2)).numpy()), LOGIT_TOL)
    assert e <= 1.0 and a <= 1.0 and s <= 1.0, (cname, e, a, s)
    assert tuple(attn.shape) == (len(lens), T + 1, T + 1) and torch.isfinite(attn).all()


def test_long_tta_list_vs_golden_and_merged_pass(ops, golden):
    """a TTA list T = (130, 127, 124), B = 2: against the reference, and the merged pass against the per-version passes within
    the tolerances of test_tta_merged_pass_equals_per_version_passes"""
    from sais_amd import temporal as tmod
    g = golden("temporal_long")
    m = _model("RGB-Flow")
    xs, fs, pads, lens_l = [], [], [], []
    for v, T in enumerate((130, 127, 124)):
        xs.append(synth.reps(seed=300 + v, B=2, T=T).to(DEV))
        fs.append(synth.reps(seed=400 + v, B=2, T=T).to(DEV))
        pads.append(synth.padding_mask([T, T]).to(DEV))
        lens_l.append([T, T])
    old = tmod._TTA_MERGE
    try:
        with torch.no_grad():
            tmod._TTA_MERGE = True
            e1, a1 = m(xs, fs, lens_l, lens_l, 'Prototypes', pads, pads, None)
            tmod._TTA_MERGE = False
            e0, a0 = m(xs, fs, lens_l, lens_l, 'Prototypes', pads, pads, None)
    finally:
        tmod._TTA_MERGE = old
    for embs, attn in ((e1, a1), (e0, a0)):
        for v in range(3):
            ref = g[f"TTA/emb{v}"]
            assert log(f"golden_tta_emb{v}", maxabs(embs[v], ref), FEAT_REL * np.abs(ref).max()) <= 1.0
        assert log("golden_tta_attn", maxabs(attn, g["TTA/attn"]), ATTN_TOL) <= 1.0
    assert a1.shape == a0.shape
    for v in range(3):
        assert maxabs(e1[v], e0[v].cpu().numpy()) <= 1e-4
    assert maxabs(a1, a0.cpu().numpy()) <= 1e-5


def test_long_gradients_vs_fp64_oracle(ops):
    """lens [130, 97], RGB-Flow, train() with dropout 0.1: every parameter gradient, dx and df against fp64 autograd of
    oracle.temporal_forward fed the exported masks and the forward's ReLU gates; the bar of the existing temporal gradient test
    (GRAD_REL).  Position rows 97 .. 129 receive a gradient, rows past 130 none."""
    from oracle import sais_oracle as O
    from sais_amd.loss import calcNCELoss
    lens = [130, 97]
    B, T, S = 2, 130, 131
    x, f, pad = _inputs(lens, (920, 921))
    m = _model("RGB-Flow", 0.1, train=True)
    m.dropout_seed = 77
    xg, fg = x.to(DEV).requires_grad_(True), f.to(DEV).requires_grad_(True)
    protos = torch.nn.ParameterDict({k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in synth.prototypes(2, 2).items()})
    lab = synth.labels(seed=912, B=B, nclasses=2)
    emb, attn = m(xg, fg, lens, lens, 'Prototypes', pad.to(DEV), pad.to(DEV), None)
    calcNCELoss(0, emb, lab, ["v0", "v1"], protos, None).backward()
    st = m.last_dropout_state
    drop = {"rgb": [{k: v.cpu() for k, v in lm.items()} for lm in m.dropout_masks(st, B, S, stream=0)],
            "flow": [{k: v.cpu() for k, v in lm.items()} for lm in m.dropout_masks(st, B, S, stream=1)]}
    sd = {k: v.double().clone().requires_grad_(True) for k, v in synth.temporal_state_dict(seed=1).items()}
    pr = {k: v.double().clone().requires_grad_(True) for k, v in synth.prototypes(2, 2).items()}
    xr, fr = x.double().requires_grad_(True), f.double().requires_grad_(True)
    # the ReLU gates of the same pass: put the state one draw back, so that the helper's forward draws `st` again.  A gate
    # reads closed where the FFN dropout zeroed a positive unit; the oracle multiplies by the same mask there, so value and
    # gradient are 0 either way (such units show in ig.mismatches, which is therefore not asserted on)
    m._rng.copy_(st)
    m._rng[1] -= 1
    gates = parity.hip_temporal_gates(m, xg, fg, pad.to(DEV), pad.to(DEV))
    assert m.last_dropout_state.tolist() == st.tolist()
    with O.imposed_gates(gates) as ig:
        e_ref, a_ref = O.temporal_forward(sd, xr, fr, pad, pad, "RGB-Flow", drop=drop, p=m.dropout_p)
        O.nce_loss(e_ref, lab, pr).backward()
    assert not ig.gates, "the oracle took fewer ReLUs than the forward has"
    assert log("grad_attn", maxabs(attn, a_ref.detach().numpy()), ATTN_TOL) <= 1.0
    P = dict(m.named_parameters())
    errs = {"dx": rel_l2(xg.grad, xr.grad), "df": rel_l2(fg.grad, fr.grad)}
    for n, q in P.items():
        if sd[n].grad is None or float(sd[n].grad.abs().max()) == 0.0:
            continue
        errs[n] = rel_l2(q.grad, sd[n].grad)
    for k in protos.keys():
        errs["proto" + k] = rel_l2(protos[k].grad, pr[k].grad)
    log("grad_worst", max(errs.values()), GRAD_REL)
    print("worst gradients vs fp64 at the same masks and gates:", sorted(errs.items(), key=lambda kv: -kv[1])[:4])
    bad = {k: v for k, v in errs.items() if v > GRAD_REL}
    assert not bad, bad
    for t in range(97, 130):
        assert float(P[f"frame_pos_embeddings.{t}"].grad.abs().max()) > 0.0, t
    for t in (130, 131, 1999):
        assert float(P[f"frame_pos_embeddings.{t}"].grad.abs().max()) == 0.0, t


@pytest.mark.parametrize("p", [0.1, 0.0])
def test_long_graph_replay(ops, p):
    """forward + backward of one T = 130 train-mode pass captured under torch.cuda.graph: two replays give finite, different
    dropout draws (the state advances inside the graph); with dropout_p = 0 the outputs (loss, embeddings, map) are bit-equal"""
    from sais_amd.graph import GraphedStep
    from sais_amd.loss import calcNCELoss, label_columns
    from sais_amd.optim import SGD
    lens = [130, 130]
    x, _, pad = _inputs(lens, (930, 931))
    xd, padd = x.to(DEV), pad.to(DEV)
    m = _model("RGB", p, train=True)
    protos = torch.nn.ParameterDict({k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in synth.prototypes(2, 2).items()})
    cols = label_columns(synth.labels(seed=912, B=2), protos, DEV)
    opt = SGD(list(m.parameters()) + list(protos.values()), lr=0.0, engines=[m])
    out = {}

    def step():
        opt.zero_grad()
        emb, attn = m(xd, None, lens, lens, 'Prototypes', padd, None, None)
        loss = calcNCELoss(0, emb, cols, ["v0", "v1"], protos, None)
        loss.backward()
        opt.step()
        out["emb"], out["attn"] = emb.detach(), attn.detach()
        return loss

    graphed = GraphedStep(step, warmup=2)
    res = []
    for _ in range(2):
        loss = float(graphed().detach())
        res.append((loss, out["emb"].clone(), out["attn"].clone(), m.flat.grad.clone()))
    for r in res:
        assert math.isfinite(r[0]) and all(bool(torch.isfinite(t).all()) for t in r[1:])
    assert float(res[0][3].abs().max()) > 0
    if p > 0:
        assert res[0][0] != res[1][0] and not torch.equal(res[0][2], res[1][2])
    else:
        assert res[0][0] == res[1][0]
        assert torch.equal(res[0][1], res[1][1]), "embeddings differ between replays"
        assert torch.equal(res[0][2], res[1][2]), "attention maps differ between replays"
        # the weight gradients are not held bit for bit: the LayerNorm backward of the encoder adds its per-workgroup dgamma /
        # dbeta with float atomics (row384.hpp), at any S; the bar of the layer-call tests
        assert float((res[0][3] - res[1][3]).norm() / res[1][3].norm()) <= 1e-6
