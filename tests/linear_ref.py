"""fp64 restatement of the linear probe (dino-main/eval_linear.py:103-109, 163-183, 206-221, 237-251), the input generator of
its tests and the rounding bounds they assert.  Shared by test_linear_gpu.py, test_linear_host.py and
golden/make_golden_linear.py; numpy only.

Bounds.  EPS = 2^-24 is the unit roundoff of fp32.  For a dot product of length K accumulated in fp32 IN ANY ORDER, plus one
more addition (the bias), the standard bound is |fl(x.w + b) - (x.w + b)| <= (K + 2) EPS (|x|.|w| + |b|) to first order
(Higham, Accuracy and Stability of Numerical Algorithms, 3.1).  `logit_bound` is that, per element.  The bounds of the cross
entropy and of the update are propagated from it below; none is tuned to what a kernel gives."""
import hashlib
import math

import numpy as np

EPS = 2.0 ** -24
MOMENTUM = 0.9
FRAGILE_CAP = 0.05
#        name     C     Dm    B    sep   lr    epochs steps eval seed
CASES = [
    ("c10", 10, 1536, 37, 0.08, 0.05, 4, 6, 200, 201),
    ("c1000", 1000, 1536, 128, 1.0, 0.05, 2, 4, 256, 202),
    ("c3", 3, 768, 16, 0.1, 0.1, 3, 5, 64, 203),
]
W_SAMPLE_ROWS = 16           # rows of the final W kept for the large case


def case_spec(name):
    return next(c for c in CASES if c[0] == name)


def make_case(name):
    """dict(C, Dm, lr, epochs, W0 f32 [C, Dm], batches = [[(x f32 [b, Dm], y i64 [b]) per step] per epoch], eval = (x, y)):
    class centres ~ N(0, I), x = sep centre[y] + N(0, I), labels uniform; PCG64.  The last batch of every epoch has B // 3
    rows (the tail batch of a DataLoader without drop_last)."""
    _, C, Dm, B, sep, lr, epochs, steps, n_eval, seed = case_spec(name)
    rng = np.random.Generator(np.random.PCG64(seed))
    centres = rng.standard_normal((C, Dm))
    W0 = (0.01 * rng.standard_normal((C, Dm))).astype(np.float32)          # LinearClassifier's init, drawn here

    def part(n):
        y = rng.integers(0, C, n).astype(np.int64)
        return (sep * centres[y] + rng.standard_normal((n, Dm))).astype(np.float32), y
    batches = [[part(B if s + 1 < steps else max(1, B // 3)) for s in range(steps)] for _ in range(epochs)]
    return dict(name=name, C=C, Dm=Dm, B=B, lr=lr, epochs=epochs, W0=W0, batches=batches, eval=part(n_eval))


def digest(case):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(case["W0"]).tobytes())
    for ep in case["batches"]:
        for x, y in ep:
            h.update(np.ascontiguousarray(x).tobytes())
            h.update(np.ascontiguousarray(y).tobytes())
    h.update(np.ascontiguousarray(case["eval"][0]).tobytes())
    h.update(np.ascontiguousarray(case["eval"][1]).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- features (eval_linear.py:166-170)
def probe_features(normed, avgpool=False):
    """normed: the n arrays [F, 197, 384] of get_intermediate_layers, oldest first -> the classifier input.  With avgpool
    the reference's cat(..., dim=-1).reshape INTERLEAVES (column 2 j = CLS[j], 2 j + 1 = patch mean[j]) and only n = 1
    passes its torch.cat."""
    out = np.concatenate([a[:, 0] for a in normed], axis=-1)
    if avgpool:
        if len(normed) != 1:
            raise ValueError("torch.cat: sizes of tensors must match except in dimension 2")
        out = np.stack([out, normed[-1][:, 1:].mean(axis=1)], axis=-1).reshape(out.shape[0], -1)
    return out


# ---------------------------------------------------------------------------------------------- the heads
def logits(x, W, b):
    return x.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)


def logit_bound(x, W, b):
    K = x.shape[1]
    return (K + 2) * EPS * (np.abs(x).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(b).astype(np.float64))


def cross_entropy(z, y):
    """(loss_rows [B], lse [B], dz [B, C] = (softmax - onehot) / B) in fp64."""
    mx = z.max(axis=1, keepdims=True)
    lse = (mx + np.log(np.exp(z - mx).sum(axis=1, keepdims=True)))[:, 0]
    p = np.exp(z - lse[:, None])
    p[np.arange(len(y)), y] -= 1.0
    return lse - z[np.arange(len(y)), y], lse, p / len(y)


def ce_bounds(z, y, zb):
    """Bounds of a fp32 cross entropy evaluated on logits that are within zb (elementwise) of z.
    delta = max over a row of zb.  lse is 1-Lipschitz in the sup norm, so it moves by at most delta and loss_row = lse - z[y]
    by at most 2 delta; log softmax moves by at most 2 delta as well.  The fp32 evaluation adds `arith` to every exponent
    (absolute): the roundings of z - lse and of lse = max + log(sum) (EPS (|z| + |lse| + 2)), the relative error of a sum of
    C positive terms in any order (C EPS), and 8 EPS for expf / logf themselves (a few ulp each).
    -> (loss_row bound [B], dz bound [B, C], loss-mean bound)."""
    B, C = z.shape
    rows, lse, dz = cross_entropy(z, y)
    delta = zb.max(axis=1)
    arith = EPS * (np.abs(z) + np.abs(lse)[:, None] + C + 10)
    row_b = 2 * delta + arith[np.arange(B), y] + EPS * np.abs(rows)
    p = np.exp(z - lse[:, None])
    dz_b = (p * np.expm1(2 * delta[:, None] + arith) + 2 * EPS * np.abs(dz) * B) / B
    mean_b = row_b.mean() + (B + 1) * EPS * np.abs(rows).mean()            # B additions in row order, one division
    return row_b, dz_b, mean_b


def top5(z):
    """[B, 5] classes by (value descending, class ascending): torch.topk's order on distinct values, a stable sort's on ties;
    slots >= C hold -1."""
    out = np.full((z.shape[0], 5), -1, dtype=np.int64)
    for r in range(z.shape[0]):
        o = np.argsort(-z[r], kind="stable")[:5]
        out[r, :len(o)] = o
    return out


def update_bounds(x, dz, W, b, mW, mb, lr, mu=MOMENTUM):
    """One sais_probe_update on exactly these inputs, in fp64, and the bounds of a fp32 evaluation:
    G = dz^T x is a dot product of length B: (B + 2) EPS |dz|^T |x|;  m' = mu m + G adds two roundings, W' = W - lr m' two more."""
    x64, dz64 = x.astype(np.float64), dz.astype(np.float64)
    B = x.shape[0]
    G, gb = dz64.T @ x64, dz64.sum(axis=0)
    Gb = (B + 2) * EPS * (np.abs(dz64).T @ np.abs(x64))
    gbb = (B + 2) * EPS * np.abs(dz64).sum(axis=0)
    out = {}
    for key, p, m, g, gbound in (("W", W, mW, G, Gb), ("b", b, mb, gb, gbb)):
        m1 = mu * m.astype(np.float64) + g
        p1 = p.astype(np.float64) - lr * m1
        mbound = gbound + 2 * EPS * (mu * np.abs(m) + np.abs(g)) + EPS * np.abs(m1)
        out[key] = (p1, lr * mbound + 2 * EPS * (np.abs(p) + lr * np.abs(m1)) + EPS * np.abs(p1))
        out["m" + key] = (m1, mbound)
    return out


def cosine_lrs(base_lr, epochs, n):
    """lr of epochs 0 .. n - 1 under CosineAnnealingLR(T_max=epochs, eta_min=0), by torch's recursion."""
    out, lr = [], base_lr
    for e in range(n):
        if e > 0:
            if (e - 1 - epochs) % (2 * epochs) == 0:
                lr = lr + base_lr * (1 - math.cos(math.pi / epochs)) / 2
            else:
                lr = (1 + math.cos(math.pi * e / epochs)) / (1 + math.cos(math.pi * (e - 1) / epochs)) * lr
        out.append(lr)
    return out


def trajectory(case, mu=MOMENTUM):
    """The whole run in fp64: dict(loss [epochs * steps], lr [epochs], W, b, eval_loss, top1, top5 (counts), z_eval)."""
    W, b = case["W0"].astype(np.float64), np.zeros(case["C"])
    mW, mb = np.zeros_like(W), np.zeros_like(b)
    lrs = cosine_lrs(case["lr"], case["epochs"], case["epochs"])
    losses = []
    for ep, lr in zip(case["batches"], lrs):
        for x, y in ep:
            x64 = x.astype(np.float64)
            rows, _, dz = cross_entropy(x64 @ W.T + b, y)
            losses.append(rows.mean())
            mW = mu * mW + dz.T @ x64
            mb = mu * mb + dz.sum(axis=0)
            W = W - lr * mW
            b = b - lr * mb
    xe, ye = case["eval"]
    z = xe.astype(np.float64) @ W.T + b
    t5 = top5(z)
    return dict(loss=np.asarray(losses), lr=np.asarray(lrs), W=W, b=b, eval_loss=cross_entropy(z, ye)[0].mean(),
                top1=int((t5[:, 0] == ye).sum()), top5=int((t5 == ye[:, None]).any(axis=1).sum()), z_eval=z)


def fragile_rows(z, y, zb):
    """Boolean [n]: eval rows whose top-1 or top-5 verdict can change when every logit moves by at most zb: the margin
    between the target and the class it would have to pass (or be passed by) at rank 1 or rank min(5, C) is below
    2 x bound."""
    n, C = z.shape
    out = np.zeros(n, dtype=bool)
    for r in range(n):
        t = y[r]
        others = np.delete(np.arange(C), t)
        gap = np.abs(z[r, others] - z[r, t])
        lim = zb[r, others] + zb[r, t]                    # both logits may move: |difference| moves by at most their sum
        close = gap < lim
        if not close.any():
            continue
        above = int((z[r, others] > z[r, t]).sum())
        lo, hi = above - int((close & (z[r, others] > z[r, t])).sum()), above + int((close & (z[r, others] <= z[r, t])).sum())
        out[r] = any(lo < k <= hi for k in ((1, 5) if C >= 5 else (1,)))
    return out
