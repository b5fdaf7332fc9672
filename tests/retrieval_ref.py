"""fp64 restatement of the descriptor evaluations (dino-main/eval_copy_detection.py, eval_image_retrieval.py, utils.PCA /
compute_map / multi_scale) and the input generators of their tests.  Shared by test_retrieval_host.py, test_retrieval_gpu.py and
golden/make_golden_retrieval.py; numpy only.  Nothing here is copied from the reference: each function states what the reference
computes in this project's own words (vectorised where the reference loops), and golden/retrieval.npz — produced by running the
reference's own functions — is what test_retrieval_host.py holds these restatements to."""
import hashlib

import numpy as np

GEM_CLAMP = float(np.float32(1e-6))          # clamp(min=1e-6) on an f32 tensor
LN_EPS = 1e-6
SCALES = (1, 1 / 2 ** (1 / 2), 1 / 2)
KAPPAS = (1, 5, 10)
U24 = 2.0 ** -24                             # unit roundoff of f32

# name, N (whitening rows), D, database rows, query rows, seed
WHITEN_CASES = [
    ("well", 500, 128, 150, 40, 201),        # well conditioned
    ("deficient", 96, 128, 150, 40, 202),    # rank 96 < 128: the eigenvalue floor decides 32 directions
]
MAP_CASE = (7, 300, 301)                     # queries, database images, seed
FRAME_CASE = (37, 50, 302)                   # H, W, seed of the multi_scale frame [1, 3, H, W]
COPYDAYS_CASE = 303                          # seed of the rank lists for the Holidays AP


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------ GeM
def layernorm(x, gamma, beta, eps=LN_EPS, dtype=np.float64):
    x = x.astype(dtype)
    mu = x.mean(-1, keepdims=True, dtype=dtype)
    var = ((x - mu) ** 2).mean(-1, keepdims=True, dtype=dtype)
    return (x - mu) / np.sqrt(var + dtype(eps)) * gamma.astype(dtype) + beta.astype(dtype)


def gem_descriptor(x, gamma, beta, eps=LN_EPS, clamp=GEM_CLAMP, dtype=np.float64):
    """x [F, ntok, d] -> [F, 2 d]: the CLS row of the LayerNorm, then the fourth root of the mean fourth power of the patch rows
    clamped from below, concatenated.  dtype = np.float32 evaluates the same expression in numpy f32 (the yardstick of the
    device's error: same formula, another summation order)."""
    y = layernorm(x, gamma, beta, eps, dtype)
    p = np.maximum(y[:, 1:], dtype(clamp))
    p2 = p * p
    m = (p2 * p2).mean(1, dtype=dtype)
    return np.concatenate([y[:, 0], np.sqrt(np.sqrt(m))], axis=1)


def gem_scale(x, gamma, beta, eps=LN_EPS):
    """[F, d]: per frame and column max over the patch tokens of |xhat gamma| + |beta|, the magnitude of what enters norm(x) =
    xhat gamma + beta.  The yardstick of a GeM error: the power mean is monotone and 1-Lipschitz in the sup norm, so its error
    is at most the largest error of a normed patch value, which is a few units of roundoff of THIS magnitude.  An error
    relative to the GeM value itself is not a usable measure: where xhat gamma and beta cancel (or where all but a few tokens
    clamp and the few left are such remainders) the value is small and every f32 evaluation is far off in relative terms, so
    the largest relative error over some hundred columns is a draw of the smallest remainder, not a property of the code."""
    xh = layernorm(x, np.ones(x.shape[-1]), np.zeros(x.shape[-1]), eps)
    return (np.abs(xh[:, 1:]) * np.abs(gamma.astype(np.float64))).max(1) + np.abs(beta.astype(np.float64))


def gem_from_normed(y, clamp=GEM_CLAMP):
    """The same descriptor from an already normalised token tensor [F, ntok, d] (dense_features' output), in fp64."""
    y = y.astype(np.float64)
    p = np.maximum(y[:, 1:], clamp)
    return np.concatenate([y[:, 0], ((p ** 2) ** 2).mean(1) ** 0.25], axis=1)


def make_tokens(frames, ntok, seed, d=384, hard=True):
    """(x f32 [frames, ntok, d], gamma, beta): residual-stream-like tokens and LayerNorm weights.  hard: column 5 is about -8
    after the norm in every row (gamma 0.01, beta -8), so every patch row clamps and the GeM value is the clamp; column 9 has ONE
    patch token at 50 after the norm: token 1 of frame 0 gets an outlier in x (its normalised value is then close to
    sqrt(d - 1)) and gamma[9] is set so that gamma[9] * that value = 50, with beta[9] = 0."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.standard_normal((frames, ntok, d)) * rng.uniform(0.5, 3.0, (1, 1, d)) + rng.standard_normal((1, 1, d))).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, d).astype(np.float32)
    beta = (0.3 * rng.standard_normal(d)).astype(np.float32)
    if hard:
        gamma[5], beta[5] = 0.01, -8.0
        x[0, 1, 9] = 1.0e4
        xh = layernorm(x[0, 1][None], np.ones(d), np.zeros(d))[0, 9]
        gamma[9], beta[9] = np.float32(50.0 / xh), 0.0
    return x, gamma, beta


# ------------------------------------------------------------------------------------------------------------ covariance, whitening
def colmean_cov(X):
    """(mean [D], X^T X / N [D, D], sum_k |x_ki x_kj| [D, D], sum_k |x_kj| [D]) in fp64; the second moment is NOT centred."""
    X = X.astype(np.float64)
    n = X.shape[0]
    A = np.abs(X)
    return X.mean(0), X.T @ X / n, A.T @ A, A.sum(0)


def pca_whitening(cov, dim, whit=0.5):
    """The whitening operator [dim, D] of a second-moment matrix: eigenvalues below 1e-5 of the largest are raised to it, the `dim`
    largest directions are kept in descending order, each scaled by eigenvalue^-whit."""
    w, v = np.linalg.eigh(cov)
    w = np.maximum(w, w.max() * 1e-5)
    keep = np.argsort(w)[::-1][:dim]
    return (v[:, keep] / w[keep] ** whit).T


def unit_rows(x):
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)


def whitened_similarity(W, db, q, dim, whit=0.5):
    """fp64: centre database and queries by the mean of the whitening set W, whiten with the operator of W's uncentred second
    moment, L2-normalise the rows, return queries x database^T [nq, ndb]."""
    mean, cov, _, _ = colmean_cov(W)
    P = pca_whitening(cov, dim, whit)
    f = lambda x: unit_rows((x.astype(np.float64) - mean) @ P.T)
    return f(q) @ f(db).T


def make_whiten_case(N, D, ndb, nq, seed):
    """(W [N, D], database [ndb, D], queries [nq, D]) f32: anisotropic Gaussian features with a common offset; database and
    queries are mixtures of whitening rows plus a little isotropic noise, queries are noisy copies of database rows."""
    rng = np.random.Generator(np.random.PCG64(seed))
    scale = np.exp(rng.uniform(-1.0, 1.0, D))
    offset = 0.5 * rng.standard_normal(D)
    W = (rng.standard_normal((N, D)) * scale + offset).astype(np.float32)
    mix = rng.standard_normal((ndb, N)) / np.sqrt(N)
    db = (mix @ (W.astype(np.float64) - offset) + offset + 0.05 * rng.standard_normal((ndb, D))).astype(np.float32)
    src = rng.integers(0, ndb, nq)
    q = (db[src] + 0.2 * scale * rng.standard_normal((nq, D))).astype(np.float32)
    return W, db, q


# ------------------------------------------------------------------------------------------------------------ ranks, AP, mAP
def stable_order(s):
    """argsort(-s) with equal values in ascending index order"""
    return np.argsort(-np.asarray(s), kind="stable")


def positions_of(s, items):
    """0-based positions of `items` in stable_order(s): pos[j] = #{i : s[i] > s[j] or (s[i] == s[j] and i < j)}"""
    inv = np.empty(len(s), dtype=np.int64)
    inv[stable_order(s)] = np.arange(len(s))
    return inv[np.asarray(items, dtype=np.int64)]


def trapezoid_ap(ranks, nres):
    """Area under the precision-recall polyline of one query: positive number j (0-based) found at 0-based rank r contributes
    the trapezoid between precision j / r (1 at r = 0) and (j + 1) / (r + 1), of width 1 / nres.  Both of the reference's AP
    functions (Holidays' score_ap_from_ranks_1 and utils.compute_ap) are this sum."""
    r = np.asarray(ranks, dtype=np.float64)
    j = np.arange(len(r), dtype=np.float64)
    left = np.where(r == 0, 1.0, j / np.where(r == 0, 1.0, r))
    return float(((left + (j + 1) / (r + 1)) / (2.0 * nres)).sum())


def map_from_order(order, gnd, kappas=KAPPAS):
    """order [ndb, nq]: column q = database indices by descending similarity.  Per query with a non-empty `ok`: drop the junk
    images from the list, AP of the positions of the positives in what remains (trapezoids, nres = len(ok)); precision at k =
    (positives within the first kq) / kq with kq = min(k, 1-based position of the last positive).  Queries with an empty `ok`
    count nowhere.  Returns (mAP, APs [nq] with NaN for skipped queries, mean P@k [len(kappas)], P@k [nq, len(kappas)])."""
    nq = len(gnd)
    aps, prs = np.full(nq, np.nan), np.full((nq, len(kappas)), np.nan)
    for q, g in enumerate(gnd):
        ok = np.asarray(g["ok"], dtype=np.int64).reshape(-1)
        if ok.size == 0:
            continue
        col = order[:, q]
        junk = np.isin(col, np.asarray(g.get("junk", []), dtype=np.int64))
        kept = col[~junk]
        pos = np.flatnonzero(np.isin(kept, ok))
        aps[q] = trapezoid_ap(pos, ok.size)
        for j, k in enumerate(kappas):
            kq = min(int(pos.max()) + 1, k)
            prs[q, j] = float((pos < kq).sum()) / kq
    used = ~np.isnan(aps)
    return float(aps[used].sum() / used.sum()), aps, prs[used].sum(0) / used.sum(), prs


def protocols(gnd):
    """Medium: easy and hard are positives, junk is junk.  Hard: hard are positives, junk and easy are junk."""
    cat = lambda *a: np.concatenate([np.asarray(v, dtype=np.int64).reshape(-1) for v in a])
    return ([{"ok": cat(g["easy"], g["hard"]), "junk": cat(g["junk"])} for g in gnd],
            [{"ok": cat(g["hard"]), "junk": cat(g["junk"], g["easy"])} for g in gnd])


def make_map_case(nq, ndb, seed):
    """(sim f32 [nq, ndb] with distinct values, gnd: per query disjoint easy / hard / junk index lists).  Query 0: its junk images
    get the largest similarities (junk ranked before every positive); query 3: no positives at all (skipped under both
    protocols); query 5: easy images only (skipped under Hard alone)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sim = rng.permutation(nq * ndb).reshape(nq, ndb).astype(np.float32) / np.float32(nq * ndb) - np.float32(0.5)
    gnd = []
    for q in range(nq):
        picks = rng.permutation(ndb)
        ne, nh, nj = (int(v) for v in rng.integers(3, 12, 3))
        g = {"easy": picks[:ne], "hard": picks[ne:ne + nh], "junk": picks[ne + nh:ne + nh + nj]}
        if q == 3:
            g["easy"], g["hard"] = picks[:0], picks[:0]
        if q == 5:
            g["hard"] = picks[:0]
        gnd.append({k: np.sort(v).astype(np.int64) for k, v in g.items()})
        # positives well above the median, so that precision at k is not trivially zero
        boost = np.concatenate([gnd[q]["easy"], gnd[q]["hard"]])
        sim[q, boost] += np.float32(0.4) * rng.uniform(0, 1, boost.size).astype(np.float32)
    sim[0, gnd[0]["junk"]] = np.float32(2.0) + np.arange(gnd[0]["junk"].size, dtype=np.float32)
    return sim, gnd


def make_copydays_ranks(seed, n=12):
    """[(ascending ranks of the retrieved positives, number of positives)]: Holidays-AP inputs, some with rank 0, some with
    positives that were not retrieved, one with none retrieved."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = [([0], 1), ([], 1), ([19], 1), ([0, 1, 2], 3)]
    for _ in range(n):
        nres = int(rng.integers(1, 6))
        found = int(rng.integers(0, nres + 1))
        out.append((sorted(int(v) for v in rng.choice(20, found, replace=False)), nres))
    return out


# ------------------------------------------------------------------------------------------------------------ bilinear resize
def scaled_size(h, w, s):
    return int(np.floor(float(h) * s)), int(np.floor(float(w) * s))


def _axis(size, out, s):
    """Source indices and weight of the second neighbour along one axis.  The weights are part of the operator's definition and
    torch computes them in f32: coordinate = f32(1 / s) (dst + 0.5) - 0.5 as one fused multiply-add (a single rounding to f32),
    clamped at 0; the second neighbour is clamped at the border."""
    r = np.float64(np.float32(1.0 / s))
    c = np.maximum((r * (np.arange(out) + 0.5) - 0.5).astype(np.float32), np.float32(0))
    i0 = np.minimum(c.astype(np.int64), size - 1)
    i1 = np.minimum(i0 + 1, size - 1)
    return i0, i1, (c - i0.astype(np.float32)).astype(np.float64)


def resize_bilinear(x, s):
    """x [F, C, H, W] -> fp64 [F, C, floor(H s), floor(W s)], align_corners = False, the scale factor as given."""
    H, W = x.shape[-2:]
    ho, wo = scaled_size(H, W, s)
    y0, y1, ly = _axis(H, ho, s)
    x0, x1, lx = _axis(W, wo, s)
    x = x.astype(np.float64)
    rows = lambda yi: x[..., yi, :][..., x0] * (1 - lx) + x[..., yi, :][..., x1] * lx
    return rows(y0) * (1 - ly)[:, None] + rows(y1) * ly[:, None]


def crop16(x):
    return x[..., :x.shape[-2] // 16 * 16, :x.shape[-1] // 16 * 16]


def make_frame(H, W, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal((1, 3, H, W)) * 1.2).astype(np.float32)
