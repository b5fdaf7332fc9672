"""fp64 restatement of the weighted k-NN classifier (dino-main/eval_knn.py:143-182), the input generator of the k-NN tests
and the analysis of which rows' verdict rounding can move.  Shared by test_knn_gpu.py, test_knn_host.py and
golden/make_golden_knn.py; numpy only."""
import hashlib

import numpy as np

TAU = 2.0 ** -15            # bf16x3 dot products of unit vectors: 2^-17 documented, x 4 for accumulation order
T = 0.07
KS = (10, 20, 100, 200)
GOLDEN_CASES = [            # name, nt, nq, C, D, noise, seed
    ("c10", 1000, 137, 10, 384, 1.0, 101),
    ("c37", 4133, 229, 37, 384, 1.0, 102),
    ("c37_noisy", 4133, 229, 37, 384, 2.0, 103),
    ("c1000", 1500, 100, 1000, 384, 1.0, 104),
]
FRAGILE_CAP = 0.05


def make_case(nt, nq, C, D, noise, seed):
    """(train f32 [nt, D], train labels i64, test f32 [nq, D], test labels i64): C class centres ~ N(0, I), feature =
    0.25 centre[label] + noise N(0, I), L2-normalised in fp32; labels uniform."""
    rng = np.random.Generator(np.random.PCG64(seed))
    centres = rng.standard_normal((C, D))

    def part(n):
        labels = rng.integers(0, C, n).astype(np.int64)
        f = (0.25 * centres[labels] + noise * rng.standard_normal((n, D))).astype(np.float32)
        f /= np.sqrt((f * f).sum(1, dtype=np.float32, keepdims=True))
        return f, labels
    train, train_labels = part(nt)
    test, test_labels = part(nq)
    return train, train_labels, test, test_labels


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def similarities(test, train):
    return test.astype(np.float64) @ train.astype(np.float64).T


def order_desc(v):
    """stable descending argsort: equal values keep the lower index first (torch.sort(descending=True) on the CPU)"""
    return np.argsort(-v, kind="stable")


def votes_of(val, idx, labels, k, C, temp=T):
    """fp64 votes [C] of one row from a neighbour list"""
    v = np.zeros(C)
    np.add.at(v, labels[idx[:k]], np.exp(val[:k].astype(np.float64) / temp))
    return v


def classify(s, train_labels, test_labels, k, C, temp=T):
    """(top1 count, top5 count) of the fp64 classifier on the similarity matrix s [nq, nt]"""
    top1 = top5 = 0
    for r in range(s.shape[0]):
        nb = order_desc(s[r])[:k]
        pred = order_desc(votes_of(s[r][nb], np.arange(k), train_labels[nb], k, C, temp))
        top1 += int(pred[0] == test_labels[r])
        top5 += int(test_labels[r] in pred[:min(5, k)])
    return top1, top5


def fragile_rows(s, train_labels, test_labels, k, C, temp=T, tau=TAU, rel=1e-3):
    """Boolean [nq]: rows whose top-1 or top-5 verdict can change when every similarity moves by at most tau: neighbours
    within tau of the k-th largest value are in or out, votes scale by (1 +- rel) (tau / T with margin); a row is fragile
    if the target's rank can cross 1 or min(5, k).  Ties at exactly zero vote are resolved by class index."""
    out = np.zeros(s.shape[0], dtype=bool)
    cls = np.arange(C)
    for r in range(s.shape[0]):
        sk = np.sort(s[r])[-k]
        sure, maybe = s[r] > sk + tau, np.abs(s[r] - sk) <= tau
        if sure.sum() + maybe.sum() == k:            # exactly as many candidates as open places: all of them are in
            sure, maybe = sure | maybe, np.zeros_like(maybe)
        w = np.exp(s[r] / temp)
        lo, hi = np.zeros(C), np.zeros(C)
        np.add.at(lo, train_labels[sure], w[sure] * (1 - rel))
        np.add.at(hi, train_labels[sure | maybe], w[sure | maybe] * (1 + rel))
        t = int(test_labels[r])
        surely = (lo > hi[t]) | ((hi[t] == 0) & (hi == 0) & (cls < t))
        possibly = (hi > lo[t]) | ((hi == lo[t]) & ((hi > 0) | (cls < t)))
        surely[t] = possibly[t] = False
        rmin, rmax = int(surely.sum()), int((possibly | surely).sum())
        out[r] = any(rmin < n <= rmax for n in (1, min(5, k)))
    return out


def check_search(val, idx, s, kmax, tau=TAU):
    """The search contract on one case: val / idx [nq, kmax] from the kernel, s [nq, nt] fp64.  Returns the largest
    |val - s[idx]| seen."""
    nq, nt = s.shape
    assert val.shape == (nq, kmax) and idx.shape == (nq, kmax)
    assert idx.min() >= 0 and idx.max() < nt
    worst = 0.0
    for r in range(nq):
        assert len(set(idx[r].tolist())) == kmax, f"row {r}: repeated index"
        sk = np.sort(s[r])[-kmax]
        got = s[r][idx[r]]
        assert got.min() >= sk - tau, f"row {r}: returned {got.min()} below the k-th value {sk}"
        rest = np.ones(nt, dtype=bool)
        rest[idx[r]] = False
        if rest.any():
            assert s[r][rest].max() <= sk + tau, f"row {r}: missed {s[r][rest].max()} above the k-th value {sk}"
        err = np.abs(val[r].astype(np.float64) - got).max()
        worst = max(worst, float(err))
        assert err <= tau / 2, f"row {r}: |val - fp64| = {err}"
        assert (np.diff(val[r]) <= 0).all(), f"row {r}: values not sorted"
    return worst
