"""GPU: copy detection and image retrieval (sais_amd/retrieval.py, VisionTransformer.retrieval_features, csrc/retrieval.hip) against
the fp64 restatement of tests/retrieval_ref.py and the results of the reference's own functions (tests/golden/retrieval.npz,
golden/make_golden_retrieval.py).

Bars.  GeM: 4 x the largest error of the same expression evaluated in numpy f32 on the same inputs (another summation order,
hence the margin).  The kernel test measures the error in units of the column's normed magnitude (retrieval_ref.gem_scale says
why an error relative to the GeM value is a lottery at these sizes: a first version of this test used it, and both the kernel
and numpy f32 moved by factors of 5 between cases, 1.4e-6 to 1.6e-5 for the kernel against numpy f32's 1.7e-6 to 9.1e-6) and,
beside it, the plain absolute error under the same factor, so that the scaled measure is seen not to be the looser one; the
model test pools given normed tokens, sums of positive terms, and keeps the relative error.
Covariance: |cov_ij - fp64| <= N 2^-24 (sum_k |x_ki x_kj|) / N, the sequential-summation bound of an f32 fma chain; the mean likewise with sum_k |x_kj|.  (The bound is the one the feature was specified with.  The kernel rounds N
times in the chain, up to splits - 1 times adding the splits and once dividing, so its worst case over all data is (N + splits) 2^-24
of the FIRST row's term and less of every later one: the bound holds with room wherever no single row carries the sum, and is met
to 0.95 - 1.00 at N = 1, where one rounding stands against a bound of one rounding (the division by 1 is exact).  A seed under
which one of N > 1 rows dominates an element to a few parts in N could exceed it by construction, not by a fault.)
Whitening: 4 x the reference's own f32 error against fp64, stored in the golden file, on the query x database similarities (never on whitened coordinates, which depend on the eigenvector basis).  Ranks:
equality with numpy's stable argsort.  Resize: 8 x 2^-24 x max |x| against the reference's recorded multi_scale inputs."""
import functools
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity
import retrieval_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
D = 384


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def rel_err(a, ref):
    return float((np.abs(a.astype(np.float64) - ref) / np.abs(ref)).max())


# ------------------------------------------------------------------------------------------------------------------ 1. GeM
def gem_kernel(x, gamma, beta, stride_pad=64, ldy=2 * D + 32):
    """sais_vit_cls_gem_norm on x [F, ntok, 384] laid out with frame_stride = ntok * 384 + stride_pad and the given ldy; returns
    (y [F, 768] host, CLS rows by sais_layernorm_fwd host)."""
    from sais_amd import _lib as L, ops
    F, ntok, _ = x.shape
    fs = ntok * D + stride_pad
    buf = torch.full((F, fs), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :ntok * D] = dev(x.reshape(F, -1))
    g, b = dev(gamma), dev(beta)
    y = torch.full((F, ldy), float("nan"), dtype=torch.float32, device=DEV)
    L.call("sais_vit_cls_gem_norm", ops._p(buf), fs, F, ntok, D, ops._p(g), ops._p(b), R.LN_EPS, R.GEM_CLAMP, ops._p(y), ldy,
           ops._stream())
    cls = torch.empty(F, D, dtype=torch.float32, device=DEV)
    ops.layernorm_fwd(buf, F, fs, g, b, R.LN_EPS, y32=cls)
    torch.cuda.synchronize()
    assert torch.isnan(y[:, 2 * D:]).all(), "wrote past 768 columns"
    return y[:, :2 * D].cpu().numpy(), cls.cpu().numpy()


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("ntok", [2, 16, 197, 401])
def test_gem_kernel(frames, ntok):
    x, gamma, beta = R.make_tokens(frames, ntok, 1000 + ntok)
    y, cls = gem_kernel(x, gamma, beta)
    ref = R.gem_descriptor(x, gamma, beta)
    f32 = R.gem_descriptor(x, gamma, beta, dtype=np.float32)
    assert np.isfinite(y).all()
    assert (y[:, :D].view(np.int32) == cls.view(np.int32)).all(), "CLS half differs from sais_layernorm_fwd"
    np.testing.assert_allclose(y[:, :D], ref[:, :D], rtol=0, atol=2e-5 * max(1.0, float(np.abs(ref[:, :D]).max())))
    # the halves are concatenated, and a column that is negative in every patch row gives exactly the clamp value
    assert np.abs(ref[:, D + 5] / R.GEM_CLAMP - 1).max() < 1e-14 and (y[:, D + 5] == np.float32(R.GEM_CLAMP)).all()
    # one token at 50 in column 9 of frame 0: mean = 50^4 / (ntok - 1) + the others
    normed = R.layernorm(x, gamma, beta)
    assert abs(normed[0, 1, 9] - 50.0) < 1e-3 and ref[0, D + 9] >= 50.0 / (ntok - 1) ** 0.25 * (1 - 1e-6)
    scale = R.gem_scale(x, gamma, beta)                      # error in units of the column's normed magnitude: see gem_scale
    err = lambda a: float((np.abs(a[:, D:].astype(np.float64) - ref[:, D:]) / scale).max())
    bar, got = 4 * err(f32), err(y)
    print(f"GeM F={frames} ntok={ntok}: max error / column scale {got:.3e}, numpy f32 {bar / 4:.3e}, bar {bar:.3e}; "
          f"relative to the value: {rel_err(y[:, D:], ref[:, D:]):.3e}, numpy f32 {rel_err(f32[:, D:], ref[:, D:]):.3e}")
    parity.parity_log(f"retrieval_gem_scaled_ntok{ntok}", got, bar)
    assert got <= bar
    # and the plain, unscaled absolute error under the same factor: the scaled measure is not a looser one
    plain = lambda a: float(np.abs(a[:, D:].astype(np.float64) - ref[:, D:]).max())
    print(f"GeM F={frames} ntok={ntok}: max absolute error {plain(y):.3e}, numpy f32 {plain(f32):.3e}, bar {4 * plain(f32):.3e}")
    parity.parity_log(f"retrieval_gem_abs_ntok{ntok}", plain(y), 4 * plain(f32))
    assert plain(y) <= 4 * plain(f32)
    y2, _ = gem_kernel(x, gamma, beta)
    assert (y.view(np.int32) == y2.view(np.int32)).all(), "two calls differ"


@functools.lru_cache(maxsize=None)
def backbone():
    from sais_amd.vit import vit_small
    torch.manual_seed(7)
    return vit_small(patch_size=16, num_classes=0).to(DEV).eval()


@pytest.mark.parametrize("F,H,W", [(2, 320, 320), (1, 224, 160)])
def test_retrieval_features(F, H, W):
    model = backbone()
    x = torch.randn(F, 3, H, W, generator=torch.Generator().manual_seed(H + W)).to(DEV)
    feats = model.retrieval_features(x)
    again = model.retrieval_features(x)
    tokens = model.dense_features(x, 1)[0]
    torch.cuda.synchronize()
    assert tuple(feats.shape) == (F, 2 * D) and feats.dtype == torch.float32
    assert tuple(tokens.shape) == (F, 1 + (H // 16) * (W // 16), D)
    assert torch.equal(feats, again), "two calls differ"
    only = model.retrieval_features(x, cls_only=True)
    assert tuple(only.shape) == (F, D) and torch.equal(only, feats[:, :D]), "cls_only differs from the descriptor's first half"
    y, t = feats.cpu().numpy(), tokens.cpu().numpy()
    assert (y[:, :D].view(np.int32) == t[:, 0].view(np.int32)).all(), "CLS half differs from dense_features"
    ref = R.gem_from_normed(t)
    p = np.maximum(t[:, 1:], np.float32(R.GEM_CLAMP))
    p2 = p * p
    f32 = np.sqrt(np.sqrt((p2 * p2).mean(1, dtype=np.float32)))
    bar = 4 * rel_err(f32, ref[:, D:])
    got = rel_err(y[:, D:], ref[:, D:])
    print(f"retrieval_features {F}x{H}x{W}: max relative error {got:.3e}, numpy f32 {bar / 4:.3e}, bar {bar:.3e}")
    parity.parity_log(f"retrieval_features_gem_rel_{H}x{W}", got, bar)
    assert got <= bar


# ------------------------------------------------------------------------------------------------------------------ 2. covariance
def colmean_cov(X, ldx):
    from sais_amd import _lib as L, ops
    N, Dm = X.shape
    buf = torch.full((N, ldx), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :Dm] = dev(X)
    need = L.load().sais_colmean_cov_workspace_bytes(N, Dm)
    assert need > 0
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV)
    mean = torch.full((Dm,), float("nan"), dtype=torch.float32, device=DEV)
    cov = torch.full((Dm, Dm), float("nan"), dtype=torch.float32, device=DEV)
    L.call("sais_colmean_cov", ops._p(buf), ldx, N, Dm, ops._p(mean), ops._p(cov), ops._p(ws), need, ops._stream())
    torch.cuda.synchronize()
    return mean.cpu().numpy(), cov.cpu().numpy()


@pytest.mark.parametrize("Dm", [64, 128, 768])
@pytest.mark.parametrize("N", [1, 63, 64, 1000, 4099])
def test_colmean_cov(N, Dm):
    rng = np.random.Generator(np.random.PCG64(31 * N + Dm))
    X = (rng.standard_normal((N, Dm)) * np.exp(rng.uniform(-1, 1, Dm)) + 0.5 * rng.standard_normal(Dm)).astype(np.float32)
    ldx = Dm + 4 * (N % 3)
    mean, cov = colmean_cov(X, ldx)
    assert np.isfinite(mean).all() and np.isfinite(cov).all(), "elements left unwritten"
    assert (cov.view(np.int32) == cov.T.view(np.int32)).all(), "cov is not bit-symmetric"
    rmean, rcov, absprod, abssum = R.colmean_cov(X)
    cov_bound = N * R.U24 * absprod / N
    mean_bound = N * R.U24 * abssum / N
    ec, em = np.abs(cov.astype(np.float64) - rcov), np.abs(mean.astype(np.float64) - rmean)
    worst_c, worst_m = float((ec / cov_bound).max()), float((em / mean_bound).max())
    print(f"cov N={N} D={Dm}: max error / bound = {worst_c:.3e} (cov), {worst_m:.3e} (mean); max |cov error| {ec.max():.3e}")
    parity.parity_log("retrieval_cov_err_over_bound", worst_c, 1.0)
    parity.parity_log("retrieval_mean_err_over_bound", worst_m, 1.0)
    assert (ec <= cov_bound).all() and (em <= mean_bound).all()
    mean2, cov2 = colmean_cov(X, ldx)
    assert (cov.view(np.int32) == cov2.view(np.int32)).all() and (mean.view(np.int32) == mean2.view(np.int32)).all()


def test_center_rows():
    from sais_amd import ops
    rng = np.random.Generator(np.random.PCG64(5))
    X, m = rng.standard_normal((37, 768)).astype(np.float32), rng.standard_normal(768).astype(np.float32)
    buf = torch.zeros(37, 772, dtype=torch.float32, device=DEV)
    buf[:, :768] = dev(X)
    ops.center_rows_(buf[:, :768], dev(m))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:, :768] == X - m).all() and (out[:, 768:] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ 3. whitening
@pytest.mark.parametrize("case", R.WHITEN_CASES, ids=[c[0] for c in R.WHITEN_CASES])
def test_whitening_vs_fp64(golden, case):
    from sais_amd import retrieval
    name, N, Dm, ndb, nq, seed = case
    g = golden("retrieval")
    W, db, q = R.make_whiten_case(N, Dm, ndb, nq, seed)
    assert (R.digest(W, db, q) == g[f"whiten_{name}_sha256"]).all(), "generated inputs differ from the recorded ones"
    pca = retrieval.PCAWhitening(Dm, 0.5).fit(dev(W))
    fq, fd = pca.apply(dev(q)), pca.apply(dev(db))
    torch.cuda.synchronize()
    fq, fd = fq.cpu().numpy().astype(np.float64), fd.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose((fq * fq).sum(1), 1.0, atol=1e-5)
    s64 = R.whitened_similarity(W, db, q, Dm)
    bar = 4 * float(g[f"whiten_{name}_ref_err"])
    got = float(np.abs(fq @ fd.T - s64).max())
    print(f"whitening {name}: max |sim - fp64| = {got:.3e}, reference f32 {bar / 4:.3e}, bar {bar:.3e}")
    parity.parity_log(f"retrieval_whiten_{name}_abs", got, bar)
    assert got <= bar
    # the reference's own f32 similarities are as far from fp64 as recorded (the bar is what it claims to be)
    assert abs(float(np.abs(g[f"whiten_{name}_sim"].astype(np.float64) - s64).max()) - bar / 4) <= 1e-9
    # copy-detection search on the whitened descriptors: the first hit agrees with fp64 wherever fp64 is decided by more than 2^-15
    val, idx = retrieval.copy_detection_topk(dev(fq.astype(np.float32)), dev(fd.astype(np.float32)), 20)
    idx = idx.cpu().numpy()
    top2 = np.sort(s64, axis=1)[:, -2:]
    decided = top2[:, 1] - top2[:, 0] > 2.0 ** -15
    assert decided.sum() >= nq // 2 and (idx[decided, 0] == s64.argmax(1)[decided]).all()


# ------------------------------------------------------------------------------------------------------------------ 4. ranks
def rank_rows(nq, ndb, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    sim = rng.standard_normal((nq, ndb)).astype(np.float32)
    kinds = ["random", "duplicates", "zeros", "equal", "random", "duplicates", "random"]
    for q in range(nq):
        kind = kinds[q % len(kinds)] if nq > 1 else "duplicates"
        if kind == "duplicates":
            sim[q] = np.round(sim[q] * 2) / 2                         # a handful of distinct values
        elif kind == "zeros":
            sim[q] = np.where(rng.integers(0, 2, ndb) == 1, np.float32(0.0), np.float32(-0.0))
            sim[q, ::5] = np.round(rng.standard_normal(len(sim[q, ::5])))
        elif kind == "equal":
            sim[q] = np.float32(0.25)
    return sim, rng


@pytest.mark.parametrize("ndb", [1, 255, 256, 257, 5003])
@pytest.mark.parametrize("nq,sizes", [(1, (0,)), (1, (1,)), (1, (300,)), (7, (300, 300, 1, 300, 0, 1, 300))])
def test_rank_positions(nq, ndb, sizes):
    from sais_amd import retrieval
    sim, rng = rank_rows(nq, ndb, 17 * ndb + nq + sum(sizes))
    lists = [rng.integers(0, ndb, n) for n in sizes]
    if sizes[0] == 300 and ndb >= 300:
        lists[0] = rng.permutation(ndb)[:300]                          # distinct items too
    ld = ndb + 3
    buf = torch.full((nq, ld), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :ndb] = dev(sim)
    got = retrieval.rank_positions(buf[:, :ndb], lists)
    down = buf[:, :ndb].cpu().numpy()
    assert (down.view(np.int32) == sim.view(np.int32)).all()
    assert len(got) == nq
    for q in range(nq):
        want = R.positions_of(down[q], lists[q])
        assert got[q].dtype == np.int64 and got[q].shape == want.shape
        assert (got[q] == want).all(), f"query {q}: {np.flatnonzero(got[q] != want)[:5]}"
    if nq == 7 and ndb > 1:
        assert len(np.unique(sim[1])) < ndb and np.signbit(sim[2]).any() and (sim[2] == 0).sum() > ndb // 2 and len(np.unique(sim[3])) == 1
    again = retrieval.rank_positions(buf[:, :ndb], lists)
    assert all((a == b).all() for a, b in zip(got, again))


def test_rank_positions_errors():
    from sais_amd import retrieval
    sim = torch.zeros(2, 10, device=DEV)
    with pytest.raises(ValueError):
        retrieval.rank_positions(sim, [[0]])
    with pytest.raises(ValueError):
        retrieval.rank_positions(sim, [[0], [10]])
    with pytest.raises(ValueError):
        retrieval.rank_positions(sim, [[-1], [0]])


def test_map_vs_reference(golden):
    from sais_amd import retrieval
    g = golden("retrieval")
    nq, ndb, seed = R.MAP_CASE
    sim, gnd = R.make_map_case(nq, ndb, seed)
    assert (R.digest(sim, *[x[k] for x in gnd for k in ("easy", "hard", "junk")]) == g["map_sha256"]).all()
    (mapM, mprM), (mapH, mprH) = retrieval.evaluate_revisited(dev(sim), gnd, R.KAPPAS)
    assert abs(mapM - float(g["map_M"])) <= 1e-12 and abs(mapH - float(g["map_H"])) <= 1e-12
    np.testing.assert_allclose(mprM, g["pr_M"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(mprH, g["pr_H"], rtol=0, atol=1e-12)
    for tag, gt in zip("MH", retrieval.revisited_protocols(gnd)):
        _, aps, _, prs = retrieval.compute_map(retrieval.rank_positions(dev(sim), retrieval.gnd_lists(gt)), gt, R.KAPPAS)
        np.testing.assert_allclose(aps, g[f"aps_{tag}"], rtol=0, atol=1e-12, equal_nan=True)
        np.testing.assert_allclose(prs, g[f"prs_{tag}"], rtol=0, atol=1e-12, equal_nan=True)


def test_similarity_pads_the_database():
    from sais_amd import retrieval
    rng = np.random.Generator(np.random.PCG64(3))
    q, db = R.unit_rows(rng.standard_normal((5, 384))).astype(np.float32), R.unit_rows(rng.standard_normal((131, 384))).astype(np.float32)
    s = retrieval.similarity(dev(q), dev(db)).cpu().numpy()
    assert s.shape == (5, 131)
    assert np.abs(s - q.astype(np.float64) @ db.astype(np.float64).T).max() <= 2.0 ** -16


# ------------------------------------------------------------------------------------------------------------------ 5. resize
def test_resize_and_multi_scale(golden):
    from sais_amd import retrieval
    g = golden("retrieval")
    H, W, seed = R.FRAME_CASE
    frame = R.make_frame(H, W, seed)
    assert (R.digest(frame) == g["frame_sha256"]).all()
    tol = 8 * R.U24 * float(np.abs(frame).max())
    x = dev(frame)
    for i, s in enumerate(R.SCALES):
        if i == 0:
            continue
        y = retrieval.resize_bilinear(x, s).cpu().numpy()
        ref = g[f"multi_scale_in{i}"]
        assert y.shape == ref.shape
        err = float(np.abs(y.astype(np.float64) - ref).max())
        print(f"resize scale {s:.4f}: {y.shape[-2:]} max |d| = {err:.3e} (bar {tol:.3e})")
        parity.parity_log("retrieval_resize_abs_over_bar", err / tol, 1.0)
        assert err <= tol
    # three frames in one call give the same bits per frame
    many = retrieval.resize_bilinear(x.expand(3, -1, -1, -1).contiguous(), R.SCALES[1])
    one = retrieval.resize_bilinear(x, R.SCALES[1])
    assert all(torch.equal(many[i], one[0]) for i in range(3))
    # multi_scale: the model sees the three scales cropped to whole patches; mean over the scales, then the norm of the whole tensor
    seen = []

    def model(t):
        seen.append(t.clone())
        return torch.stack([t.mean(), t.abs().mean(), t.std(), t.max()]).reshape(1, 4)
    v = retrieval.multi_scale(x, model)
    assert [tuple(t.shape[-2:]) for t in seen] == [(32, 48), (16, 32), (16, 16)]
    for i, t in enumerate(seen):
        assert np.abs(t.cpu().numpy().astype(np.float64) - R.crop16(g[f"multi_scale_in{i}"])).max() <= tol
    mean = sum(model(t) for t in list(seen)) / 3
    assert torch.allclose(v, mean / mean.norm(), atol=1e-6) and abs(float(v.norm()) - 1.0) < 1e-6


# ------------------------------------------------------------------------------------------------------------------ 6. CLIs
def _jpeg(path, px, quality=90):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.clip(px, 0, 255).astype(np.uint8)).save(path, quality=quality)


def _picture(rng, h, w, i):
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 90 * np.sin(xx / (3.0 + 2 * i) + i)[..., None] * np.cos(yy / (2.0 + i))[..., None] * np.array([1.0, 0.6, -0.8])
    return base + 40 * (i % 3) - 30 + rng.normal(0, 6, (h, w, 3))


def _run(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "SAIS", "scripts", "dino-main", script), "--num_workers", "2", *args],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_cli_copy_detection(tmp_path):
    from sais_amd import retrieval
    rng = np.random.Generator(np.random.PCG64(21))
    root = str(tmp_path / "copydays")
    pics = [_picture(rng, 80, 100, i) for i in range(3)]
    for i, p in enumerate(pics):
        _jpeg(os.path.join(root, "original", f"20{i}000.jpg"), p)
        _jpeg(os.path.join(root, "jpegqual", "10", f"20{i}000.jpg"), p, quality=10)
    _jpeg(os.path.join(root, "strong", "200001.jpg"), pics[0][::-1] * 0.8 + 20)
    _jpeg(os.path.join(root, "strong", "202001.jpg"), np.roll(pics[2], 9, axis=1) + rng.normal(0, 25, pics[2].shape))
    for i in range(2):
        _jpeg(str(tmp_path / "distractors" / f"d{i}.jpg"), _picture(rng, 64, 64, 5 + i))
    for i in range(4):
        _jpeg(str(tmp_path / "whitening" / f"w{i}.jpg"), _picture(rng, 72, 90, 8 + i))
    dump = tmp_path / "feats"
    out = _run("eval_copy_detection.py", "--data_path", root, "--distractors_path", str(tmp_path / "distractors"),
               "--whitening_path", str(tmp_path / "whitening"), "--imsize", "72", "--batch_size_per_gpu", "4",
               "--dump_features", str(dump))
    assert "random weights" in out and "Using distractors..." in out and "keeping" in out
    assert "Extraction of queries features done. Shape: torch.Size([8, 768])" in out
    assert "Extraction of database and distractors features done. Shape: torch.Size([5, 768])" in out
    q, db = torch.load(dump / "queries.pth").numpy().astype(np.float64), torch.load(dump / "database.pth").numpy().astype(np.float64)
    assert q.shape == (8, 768) and db.shape == (5, 768)
    np.testing.assert_allclose((db * db).sum(1), 1.0, atol=1e-5)
    blocks = retrieval.copydays_blocks(root)
    assert [(n, len(f)) for n, f in blocks] == [("original", 3), ("strong", 2), ("jpegqual/10", 3)]
    s = q @ db.T
    want, j0 = [], 0
    for name, files in blocks:
        aps = []
        for k, f in enumerate(files):
            positives = [k] if name != "strong" else [j for j, b in enumerate(blocks[0][1]) if b[:4] == f[:4]]
            order = R.stable_order(s[j0 + k])[:20]
            aps.append(R.trapezoid_ap([r for r, b in enumerate(order) if b in positives], len(positives)))
        want.append("eval on %s mAP=%.3f" % (name, sum(aps) / len(files)))
        j0 += len(files)
    assert re.findall(r"^eval on .*$", out, flags=re.M) == want


def test_cli_image_retrieval(tmp_path):
    rng = np.random.Generator(np.random.PCG64(22))
    root = tmp_path / "data"
    names = {"q0": (120, 80), "q1": (80, 120), "d0": (120, 80), "d1": (100, 100), "d2": (80, 120), "d3": (120, 90), "d4": (96, 72),
             "d5": (110, 80)}
    for i, (n, (w, h)) in enumerate(names.items()):
        _jpeg(str(root / "roxford5k" / "jpg" / f"{n}.jpg"), _picture(rng, h, w, i % 4))
    cfg = {"imlist": [f"d{i}" for i in range(6)], "qimlist": ["q0", "q1"],
           "gnd": [{"easy": [0, 4], "hard": [3], "junk": [5]}, {"easy": [2], "hard": [1, 5], "junk": []}]}
    with open(root / "roxford5k" / "gnd_roxford5k.pkl", "wb") as f:
        pickle.dump(cfg, f)
    dump = tmp_path / "feats"
    out = _run("eval_image_retrieval.py", "--data_path", str(root), "--dataset", "roxford5k", "--imsize", "96", "--multiscale", "1",
               "--dump_features", str(dump))
    assert "random weights" in out and "train: 6 imgs / query: 2 imgs" in out
    tr, qf = torch.load(dump / "trainfeat.pth").numpy().astype(np.float64), torch.load(dump / "queryfeat.pth").numpy().astype(np.float64)
    assert tr.shape == (6, 384) and qf.shape == (2, 384)
    np.testing.assert_allclose((tr * tr).sum(1), 1.0, atol=1e-5)
    s = qf @ tr.T
    order = np.stack([R.stable_order(s[q]) for q in range(2)], axis=1)
    (mM, _, pM, _), (mH, _, pH, _) = [R.map_from_order(order, g) for g in R.protocols(cfg["gnd"])]
    want = ['>> {}: mAP M: {}, H: {}'.format("roxford5k", np.around(mM * 100, decimals=2), np.around(mH * 100, decimals=2)),
            '>> {}: mP@k{} M: {}, H: {}'.format("roxford5k", np.array([1, 5, 10]), np.around(pM * 100, decimals=2),
                                                np.around(pH * 100, decimals=2))]
    assert re.findall(r"^>> .*$", out, flags=re.M) == want
