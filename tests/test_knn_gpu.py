"""GPU: weighted k-NN evaluation (sais_amd/knn.py on csrc/knn.hip) against the fp64 restatement of tests/knn_ref.py and the
reference's own counts (tests/golden/knn.npz, golden/make_golden_knn.py)."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import knn_ref
import parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TAU = knn_ref.TAU


@functools.lru_cache(maxsize=None)
def case(nt, nq, C, D, noise, seed):
    arrays = knn_ref.make_case(nt, nq, C, D, noise, seed)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def golden_case(name):
    _, nt, nq, C, D, noise, seed = next(c for c in knn_ref.GOLDEN_CASES if c[0] == name)
    train, tl, test, sl = case(nt, nq, C, D, noise, seed)
    return train, tl, test, sl, knn_ref.similarities(test, train), C


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def search(train, test, kmax, labels=None, C=1000):
    from sais_amd.knn import KnnIndex
    labels = np.zeros(len(train), np.int64) if labels is None else labels
    index = KnnIndex(dev(train), dev(labels), C)
    val, idx = index.search(dev(test), kmax)
    torch.cuda.synchronize()
    return index, val, idx


def check(train, test, kmax, name):
    _, val, idx = search(train, test, kmax)
    worst = knn_ref.check_search(val.cpu().numpy(), idx.cpu().numpy(), knn_ref.similarities(test, train), kmax)
    print(f"{name}: max |val - fp64| = {worst:.3e} (bar {TAU / 2:.3e})")
    parity.parity_log("knn_search_abs", worst, TAU / 2)


# ------------------------------------------------------------------------------------------------------------- 1. search
@pytest.mark.parametrize("nt,nq,D,kmax", [(1000, 137, 384, 200), (4133, 229, 384, 200), (257, 100, 64, 256), (200, 3, 384, 200),
                                          (129, 1, 384, 1)])
def test_search_vs_fp64(nt, nq, D, kmax):
    train, _, test, _ = case(nt, nq, 10, D, 1.0, 7)
    check(train, test, kmax, f"search {nt}x{nq}x{D} k={kmax}")


def test_search_f32_train_equals_split_index():
    """the entry takes the train side as f32 too and splits it while staging: same bits as the pre-split index"""
    import ctypes
    from sais_amd import _lib as L, ops
    train, _, test, _ = case(1000, 137, 10, 384, 1.0, 7)
    _, val, idx = search(train, test, 200)
    tr, q = dev(train), dev(test)
    val2, idx2 = torch.empty_like(val), torch.empty_like(idx)
    ws = torch.empty(L.load().sais_knn_workspace_bytes(137, 1000, 200), dtype=torch.uint8, device=DEV)
    L.call("sais_knn_search", ops._p(q), ops._p(tr), 0, 137, 1000, 384, 200, ops._p(val2), ops._p(idx2), ops._p(ws), ws.numel(),
           ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(val, val2) and torch.equal(idx, idx2)


# --------------------------------------------------------------------------------- 2. every column passes the threshold
@pytest.mark.parametrize("descending", [False, True])
def test_search_monotone_train_order(descending):
    train, _, test, _ = case(4133, 229, 10, 384, 1.0, 7)
    order = np.argsort(knn_ref.similarities(test[:1], train)[0], kind="stable")
    train = train[order[::-1] if descending else order]
    check(train, test, 200, "search, similarities to row 0 " + ("descending" if descending else "ascending"))


# --------------------------------------------------------------------------------------------------------------- 3. ties
def test_ties_bit_equal_and_lowest_indices_kept():
    base, _, test, _ = case(64, 40, 10, 384, 1.0, 11)
    rng = np.random.Generator(np.random.PCG64(12))
    src = rng.permutation(np.repeat(np.arange(64), 8))              # train row i is a copy of base[src[i]]
    train = base[src]
    kmax = 20                                                       # 2 groups of 8 and 4 of the third group
    _, val, idx = search(train, test, kmax)
    val, idx = val.cpu().numpy(), idx.cpu().numpy()
    knn_ref.check_search(val, idx, knn_ref.similarities(test, train), kmax)
    bits = val.view(np.int32)
    cut = 0
    for r in range(len(test)):
        by_src = {}
        for v, i in zip(bits[r], idx[r]):
            by_src.setdefault(int(src[i]), []).append((int(v), int(i)))
        for s, items in by_src.items():
            assert len({v for v, _ in items}) == 1, f"row {r}: copies of vector {s} differ in value"
        for j in range(kmax - 1):
            if bits[r][j] == bits[r][j + 1]:
                assert idx[r][j] < idx[r][j + 1], f"row {r}: equal values not in index order at {j}"
        # the group that kmax cuts through keeps its lowest train indices
        same = np.flatnonzero(src == src[idx[r][-1]]).tolist()
        kept = sorted(int(i) for i in idx[r] if src[i] == src[idx[r][-1]])
        assert kept == same[:len(kept)], f"row {r}: kept {kept} of {same}"
        cut += len(kept) < 8
    assert cut > 0


# --------------------------------------------------------------------------------------------------------------- 4. vote
@pytest.mark.parametrize("name", ["c10", "c1000"])
def test_vote(name):
    train, tl, test, sl, s, C = golden_case(name)
    ks = list(knn_ref.KS)
    index, val, idx = search(train, test, max(ks), tl, C)
    pred, votes = index.vote(val, idx, ks, knn_ref.T, return_votes=True)
    pred32 = index.vote(val, idx, ks, knn_ref.T)
    torch.cuda.synchronize()
    assert torch.equal(pred, pred32)
    v_np, i_np, p_np, w_np = val.cpu().numpy(), idx.cpu().numpy(), pred.cpu().numpy(), votes.cpu().numpy()
    worst = 0.0
    for j, k in enumerate(ks):
        single_pred, single_votes = index.vote(val, idx, [k], knn_ref.T, return_votes=True)
        assert torch.equal(single_pred[0], pred[j]) and torch.equal(single_votes[0], votes[j]), f"k={k}: multi-k differs from single-k"
        few = 0
        for r in range(len(test)):
            ref = knn_ref.votes_of(v_np[r], i_np[r], tl, k, C)
            err = np.abs(w_np[j, r] - ref).max() / ref.max()
            worst = max(worst, float(err))
            assert err <= 5e-5, f"k={k} row {r}: vote error {err} of the largest vote"
            assert (p_np[j, r] == knn_ref.order_desc(w_np[j, r])[:5]).all(), f"k={k} row {r}: pred is not the stable argsort"
            few += int((w_np[j, r] > 0).sum() < 5)
        if name == "c10" and k == 10:
            assert few > 0                          # the class-index tie-break among unvoted classes decides these rows' top-5
        print(f"{name} k={k}: rows with fewer than 5 voted classes: {few}")
    print(f"{name}: max vote error / largest vote = {worst:.3e} (bar 5e-5)")
    parity.parity_log("knn_vote_rel", worst, 5e-5)
    # int32 labels give the same index as int64 labels
    from sais_amd.knn import KnnIndex
    p2 = KnnIndex(dev(train), dev(tl.astype(np.int32)), C).classify(dev(test), ks, knn_ref.T)
    assert torch.equal(p2, pred)


# ------------------------------------------------------------------------------------------------- 5. against the reference
@pytest.mark.parametrize("name", [c[0] for c in knn_ref.GOLDEN_CASES])
def test_counts_vs_reference(golden, name):
    from sais_amd.knn import knn_classifier
    g = golden("knn")
    train, tl, test, sl, s, C = golden_case(name)
    assert (knn_ref.digest(train, tl, test, sl) == g[f"{name}_sha256"]).all(), "generated inputs differ from the recorded ones"
    nq = len(test)
    res = knn_classifier(dev(train), dev(tl), dev(test), dev(sl), list(knn_ref.KS), knn_ref.T, num_classes=C)
    for j, k in enumerate(knn_ref.KS):
        nfrag = int(knn_ref.fragile_rows(s, tl, sl, k, C).sum())
        assert nfrag <= knn_ref.FRAGILE_CAP * nq
        got = [round(res[j][0] * nq / 100.0), round(res[j][1] * nq / 100.0)]
        ref = g[f"{name}_counts"][j]
        print(f"{name} k={k}: top1 {got[0]} (ref {ref[0]}), top5 {got[1]} (ref {ref[1]}), fragile rows {nfrag}")
        assert isinstance(res[j][0], float) and isinstance(res[j][1], float)
        assert abs(got[0] - ref[0]) <= nfrag and abs(got[1] - ref[1]) <= nfrag
    one = knn_classifier(dev(train), dev(tl), dev(test), dev(sl), 20, knn_ref.T, num_classes=C)
    assert one == res[1]


# ------------------------------------------------------------------------------------------------------- 6. determinism
def test_determinism_and_index_reuse():
    from sais_amd.knn import KnnIndex
    train, tl, test, sl, s, C = golden_case("c37")
    other = case(1000, 137, 10, 384, 1.0, 7)[2]
    ks = list(knn_ref.KS)

    def run(index, q):
        val, idx = index.search(dev(q), 200)
        pred, votes = index.vote(val, idx, ks, knn_ref.T, return_votes=True)
        return [t.clone() for t in (val, idx, pred, votes)]
    index = KnnIndex(dev(train), dev(tl), C)
    a, b = run(index, test), run(index, test)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = run(index, other)                                            # reused across test sets (different Nq: other workspace)
    a2 = run(index, test)
    assert all(torch.equal(x, y) for x, y in zip(a, a2))
    assert all(torch.equal(x, y) for x, y in zip(c, run(KnnIndex(dev(train), dev(tl), C), other)))


# ---------------------------------------------------------------------------------------------------- 7. argument errors
def test_argument_errors():
    from sais_amd._lib import SaisHipError
    from sais_amd.knn import KnnIndex, knn_classifier
    train, tl, test, sl = case(200, 3, 10, 384, 1.0, 7)
    err = (ValueError, SaisHipError)
    args = (dev(train), dev(tl), dev(test), dev(sl))
    with pytest.raises(err):
        knn_classifier(*args, 201, 0.07, num_classes=10)             # k > Nt
    with pytest.raises(err):
        knn_classifier(*args, 257, 0.07, num_classes=10)
    big = case(300, 3, 10, 384, 1.0, 7)
    with pytest.raises(err):
        knn_classifier(dev(big[0]), dev(big[1]), dev(big[2]), dev(big[3]), 257, 0.07, num_classes=10)      # k = 257 <= Nt
    with pytest.raises(err):
        KnnIndex(dev(train[:, :100].copy()), dev(tl), 10)            # D = 100
    bad = tl.copy()
    bad[5] = 10
    with pytest.raises(err):
        KnnIndex(dev(train), dev(bad), 10)                           # label == num_classes
    with pytest.raises(err):
        KnnIndex(torch.from_numpy(train.copy()), torch.from_numpy(tl.copy()), 10)      # host tensors
    with pytest.raises(err):
        KnnIndex(dev(train), dev(tl), 10).search(torch.from_numpy(test.copy()), 5)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 8. CLI end to end
def test_cli_end_to_end(tmp_path):
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(5))
    for part, n in (("train", 8), ("val", 4)):
        for c in range(3):
            d = tmp_path / "data" / part / f"class_{c}"
            d.mkdir(parents=True)
            for i in range(n):
                px = np.clip(rng.normal(60 + 60 * c, 40, (72, 96, 3)), 0, 255).astype(np.uint8)
                Image.fromarray(px).save(d / f"img_{i:02d}.jpg", quality=90)
    script = os.path.join(ROOT, "SAIS", "scripts", "dino-main", "eval_knn.py")
    dump = tmp_path / "feats"

    def run(*extra):
        r = subprocess.run([sys.executable, script, "--num_workers", "2", "--batch_size_per_gpu", "16", *extra], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout
    out = run("--data_path", str(tmp_path / "data"), "--nb_knn", "5", "10", "100", "--dump_features", str(dump))
    lines = re.findall(r"^(\d+)-NN classifier result: Top1: ([\d.]+), Top5: ([\d.]+)$", out, flags=re.M)
    assert [int(l[0]) for l in lines] == [5, 10]
    assert all(0.0 <= float(v) <= 100.0 for l in lines for v in l[1:])
    assert "100-NN classifier skipped" in out and "random weights" in out
    shapes = {"trainfeat.pth": (24, 384), "testfeat.pth": (12, 384), "trainlabels.pth": (24,), "testlabels.pth": (12,)}
    for f, shape in shapes.items():
        t = torch.load(dump / f)
        assert tuple(t.shape) == shape
        if t.dim() == 2:
            assert torch.allclose(t.norm(dim=1), torch.ones(shape[0]), atol=1e-5)
    assert torch.load(dump / "trainlabels.pth").tolist() == [c for c in range(3) for _ in range(8)]
    again = run("--load_features", str(dump), "--nb_knn", "5", "10", "100")
    assert re.findall(r"^\d+-NN classifier result.*$", again, flags=re.M) == re.findall(r"^\d+-NN classifier result.*$", out, flags=re.M)
