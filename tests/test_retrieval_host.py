"""CPU-only: the fp64 restatement of the copy-detection / image-retrieval evaluations (tests/retrieval_ref.py) against the results
of the reference's own functions (tests/golden/retrieval.npz, written by golden/make_golden_retrieval.py), the host functions of
sais_amd.retrieval against both, the crop rule, the dataset listings and the argument errors of the new entries."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from tests import retrieval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "retrieval.npz"))


@pytest.fixture(scope="module")
def map_case():
    nq, ndb, seed = R.MAP_CASE
    sim, gnd = R.make_map_case(nq, ndb, seed)
    assert (R.digest(sim, *[g[k] for g in gnd for k in ("easy", "hard", "junk")]) == G["map_sha256"]).all()
    return sim, gnd


def test_map_restatement_matches_reference(map_case):
    sim, gnd = map_case
    order = np.stack([R.stable_order(sim[q]) for q in range(sim.shape[0])], axis=1)
    for tag, g in zip("MH", R.protocols(gnd)):
        m, aps, pr, prs = R.map_from_order(order, g)
        assert abs(m - float(G[f"map_{tag}"])) <= 1e-12
        np.testing.assert_allclose(aps, G[f"aps_{tag}"], rtol=0, atol=1e-12, equal_nan=True)
        np.testing.assert_allclose(pr, G[f"pr_{tag}"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(prs, G[f"prs_{tag}"], rtol=0, atol=1e-12, equal_nan=True)
    assert np.isnan(G["aps_M"]).sum() == 1 and np.isnan(G["aps_H"]).sum() == 2          # the empty-`ok` queries


def test_host_map_matches_reference_and_restatement(map_case):
    from sais_amd import retrieval
    sim, gnd = map_case
    order = np.stack([R.stable_order(sim[q]) for q in range(sim.shape[0])], axis=1)
    for tag, (g, mine) in zip("MH", zip(retrieval.revisited_protocols(gnd), R.protocols(gnd))):
        for a, b in zip(g, mine):
            assert (a["ok"] == b["ok"]).all() and (a["junk"] == b["junk"]).all()
        lists = retrieval.gnd_lists(g)
        positions = [R.positions_of(sim[q], lists[q]) for q in range(len(g))]
        m, aps, pr, prs = retrieval.compute_map(positions, g, R.KAPPAS)
        rm, raps, rpr, rprs = R.map_from_order(order, g)
        for got, ref, gold in ((m, rm, G[f"map_{tag}"]), (aps, raps, G[f"aps_{tag}"]), (pr, rpr, G[f"pr_{tag}"]),
                               (prs, rprs, G[f"prs_{tag}"])):
            np.testing.assert_allclose(got, gold, rtol=0, atol=1e-12, equal_nan=True)
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12, equal_nan=True)


def test_ap_formulas():
    from sais_amd import retrieval
    cases = R.make_copydays_ranks(R.COPYDAYS_CASE)
    assert len(cases) == len(G["copydays_ap"]) == len(G["compute_ap"])
    for (ranks, nres), gold_h, gold_u in zip(cases, G["copydays_ap"], G["compute_ap"]):
        mine = R.trapezoid_ap(ranks, nres)
        assert abs(mine - gold_h) <= 1e-12 and abs(mine - gold_u) <= 1e-12
        assert abs(retrieval.average_precision_from_ranks(ranks, nres) - gold_h) <= 1e-12
        assert abs(retrieval.compute_ap(np.asarray(ranks), nres) - gold_u) <= 1e-12
    assert G["copydays_ap"][0] == 1.0 and G["copydays_ap"][1] == 0.0


@pytest.mark.parametrize("case", R.WHITEN_CASES, ids=[c[0] for c in R.WHITEN_CASES])
def test_whitening_restatement(case):
    name, N, D, ndb, nq, seed = case
    W, db, q = R.make_whiten_case(N, D, ndb, nq, seed)
    assert (R.digest(W, db, q) == G[f"whiten_{name}_sha256"]).all()
    s64 = R.whitened_similarity(W, db, q, D)
    err = float(np.abs(G[f"whiten_{name}_sim"].astype(np.float64) - s64).max())
    print(f"{name}: reference f32 vs fp64 restatement {err:.3e} (stored {float(G[f'whiten_{name}_ref_err']):.3e})")
    assert err <= 1e-3 and abs(err - float(G[f"whiten_{name}_ref_err"])) <= 1e-9
    floored = int((np.linalg.eigvalsh(R.colmean_cov(W)[1]) < 1e-5 * np.linalg.eigvalsh(R.colmean_cov(W)[1]).max()).sum())
    assert (floored > 0) == (name == "deficient")
    # the host half of PCAWhitening on the fp64 second moment gives the restatement's operator up to the sign of each direction
    from sais_amd import retrieval
    p = retrieval.PCAWhitening(D, 0.5)
    cov = R.colmean_cov(W)[1]
    p.train_pca(cov.copy())
    P = R.pca_whitening(cov, D)
    np.testing.assert_allclose(np.abs(p.dvt.T @ p.dvt), np.abs(P.T @ P), rtol=0, atol=1e-9 * np.abs(P.T @ P).max())
    assert 99.99 < p.energy <= 100.0 + 1e-9


def test_resize_restatement_and_multi_scale():
    H, W, seed = R.FRAME_CASE
    frame = R.make_frame(H, W, seed)
    assert (R.digest(frame) == G["frame_sha256"]).all()
    tol = 8 * R.U24 * float(np.abs(frame).max())
    ins = [frame.astype(np.float64)] + [R.resize_bilinear(frame, s) for s in R.SCALES[1:]]
    for i, mine in enumerate(ins):
        assert mine.shape == G[f"multi_scale_in{i}"].shape
        assert np.abs(mine - G[f"multi_scale_in{i}"]).max() <= tol
    assert [a.shape[-2:] for a in ins] == [(37, 50), (26, 35), (18, 25)]
    from sais_amd import retrieval
    for s in R.SCALES:
        assert retrieval.scaled_size(H, W, s) == R.scaled_size(H, W, s)


def test_crop_rule():
    from sais_amd import retrieval
    assert retrieval.cropped_size(224, 224) == (224, 224)
    assert retrieval.cropped_size(37, 50) == (32, 48) and retrieval.cropped_size(26, 35) == (16, 32)
    assert retrieval.cropped_size(18, 25) == (16, 16) and retrieval.cropped_size(159, 223) == (144, 208)
    with pytest.raises(ValueError):
        retrieval.cropped_size(15, 64)
    x = torch.arange(3 * 37 * 50, dtype=torch.float32).reshape(1, 3, 37, 50)
    y = retrieval.crop_to_patches(x)
    assert tuple(y.shape) == (1, 3, 32, 48) and y.is_contiguous() and torch.equal(y, x[:, :, :32, :48])       # right and bottom go
    z = torch.zeros(2, 3, 32, 64)
    assert retrieval.crop_to_patches(z) is z
    with pytest.raises(ValueError):
        retrieval.crop_to_patches(torch.zeros(3, 32, 32))
    assert (R.crop16(np.zeros((1, 3, 37, 50))).shape == np.array((1, 3, 32, 48))).all()


def _jpeg(path, w, h, seed):
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(seed))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path, quality=90)


def test_dataset_listings(tmp_path):
    from sais_amd import retrieval
    root = str(tmp_path)
    for i, n in enumerate(("2001.jpg", "2000.jpg", "2002.jpg")):
        _jpeg(os.path.join(root, "cd", "original", n), 40 + i, 30, i)
    for i, n in enumerate(("200001.jpg", "200002.jpg", "200201.jpg", "notes.txt")):
        _jpeg(os.path.join(root, "cd", "strong", n), 33, 47, 10 + i) if n.endswith(".jpg") else open(os.path.join(root, "cd", "strong", n), "w").close()
    for n in ("2000.jpg", "2001.jpg", "2002.jpg"):
        _jpeg(os.path.join(root, "cd", "crops", "10", n), 20, 20, 20)
    blocks = retrieval.copydays_blocks(os.path.join(root, "cd"))
    assert [b[0] for b in blocks] == ["original", "strong", "crops/10"]
    assert blocks[0][1] == ["2000.jpg", "2001.jpg", "2002.jpg"] and blocks[1][1] == ["200001.jpg", "200002.jpg", "200201.jpg"]
    with pytest.raises(FileNotFoundError):
        retrieval.copydays_blocks(os.path.join(root, "cd", "crops"))
    # 3 + 3 + 3 queries against the 3 originals (+ 2 distractors): strong queries 0, 1 match original 0, query 2 original 2
    idx = np.array([[0, 1, 2], [1, 0, 2], [3, 4, 2],                  # original: rank 0, rank 0, rank 2
                    [0, 1, 2], [4, 3, 0], [1, 0, 3],                  # strong: rank 0, rank 2, not retrieved
                    [2, 1, 0], [1, 2, 0], [4, 3, 1]])                 # crops/10: rank 2, rank 0, not retrieved
    got = retrieval.copydays_map(idx, blocks)
    want = [("original", (1.0 + 1.0 + R.trapezoid_ap([2], 1)) / 3), ("strong", (1.0 + R.trapezoid_ap([2], 1) + 0.0) / 3),
            ("crops/10", (R.trapezoid_ap([2], 1) + 1.0 + 0.0) / 3)]
    assert [g[0] for g in got] == [w[0] for w in want]
    np.testing.assert_allclose([g[1] for g in got], [w[1] for w in want], rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        retrieval.copydays_map(idx[:-1], blocks)
    # flat image lists: extension filter, sorted
    open(os.path.join(root, "cd", "original", "readme.md"), "w").close()
    assert [os.path.basename(p) for p in retrieval.list_images(os.path.join(root, "cd", "original"))] == ["2000.jpg", "2001.jpg", "2002.jpg"]
    ds = retrieval.ImgListDataset(retrieval.list_images(os.path.join(root, "cd", "strong")), 48)
    img, i = ds[1]
    assert len(ds) == 3 and i == 1 and tuple(img.shape) == (3, 48, 48) and img.dtype == torch.float32
    # revisited Oxford: thumbnail keeps the aspect ratio, the longer side becomes imsize
    for n, (w, h) in {"q0": (80, 40), "d0": (30, 60), "d1": (64, 64)}.items():
        _jpeg(os.path.join(root, "ro", "roxford5k", "jpg", n + ".jpg"), w, h, 30)
    cfg = {"imlist": ["d0", "d1"], "qimlist": ["q0"], "gnd": [{"easy": [1], "hard": [], "junk": [0]}]}
    with open(os.path.join(root, "ro", "roxford5k", "gnd_roxford5k.pkl"), "wb") as f:
        pickle.dump(cfg, f)
    dq = retrieval.OxfordParisDataset(os.path.join(root, "ro"), "roxford5k", "query", imsize=40)
    dt = retrieval.OxfordParisDataset(os.path.join(root, "ro"), "roxford5k", "train", imsize=40)
    assert len(dq) == 1 and len(dt) == 2 and dt.gnd == cfg["gnd"] and dt.cfg == cfg and dq.samples == ["q0"]
    assert tuple(dq[0][0].shape) == (3, 20, 40) and tuple(dt[0][0].shape) == (3, 40, 20) and tuple(dt[1][0].shape) == (3, 40, 40)
    with pytest.raises(ValueError):
        retrieval.OxfordParisDataset(root, "oxford", "query")


def test_argument_errors():
    from sais_amd import _lib, retrieval
    from sais_amd.vit import vit_small
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    assert lib.sais_vit_cls_gem_norm(None, 197 * 384, 2, 197, 384, None, None, 1e-6, 1e-6, None, 768, None) == -1
    for fs, frames, ntok, dim, ldy, pmin in ((197 * 384, 0, 197, 384, 768, 1e-6), (197 * 384, 1, 1, 384, 768, 1e-6),
                                             (197 * 384, 1, 197, 256, 768, 1e-6), (100, 1, 197, 384, 768, 1e-6),
                                             (197 * 384, 1, 197, 384, 767, 1e-6), (197 * 384, 1, 197, 384, 768, 0.0)):
        assert lib.sais_vit_cls_gem_norm(p, fs, frames, ntok, dim, p, p, 1e-6, pmin, p, ldy, None) == -1, (fs, frames, ntok, dim, ldy)
    # one plan behind the size query and the launch: tiles on or above the diagonal x row splits of whole 32-row steps
    assert lib.sais_colmean_cov_workspace_bytes(20000, 768) == (13 * 78 * 4096 + 13 * 768) * 4      # 13 splits of 1568 rows
    assert lib.sais_colmean_cov_workspace_bytes(1000, 64) == (8 * 4096 + 8 * 64) * 4                # 8 splits of 128 rows
    assert lib.sais_colmean_cov_workspace_bytes(1, 64) == (4096 + 64) * 4
    assert lib.sais_colmean_cov_workspace_bytes(4099, 1536) == (3 * 300 * 4096 + 3 * 1536) * 4      # 3 splits of 1376 rows
    for n, d in ((0, 64), (10, 0), (10, 96), (10, 1600)):
        assert lib.sais_colmean_cov_workspace_bytes(n, d) == 0
        assert lib.sais_colmean_cov(p, max(d, 64), n, d, p, p, p, 1 << 30, None) == -1
    assert lib.sais_colmean_cov(None, 64, 10, 64, p, p, p, 1 << 30, None) == -1
    assert lib.sais_colmean_cov(p, 64, 10, 64, p, p, p, (4096 + 64) * 4 - 1, None) == -1            # workspace too small
    assert lib.sais_colmean_cov(p, 60, 10, 64, p, p, p, 1 << 30, None) == -1                        # ldx < D
    assert lib.sais_center_rows(None, 64, 4, 64, p, None) == -1 and lib.sais_center_rows(p, 64, 4, 62, p, None) == -1
    assert lib.sais_rank_positions(None, 10, 1, 10, p, p, p, None) == -1 and lib.sais_rank_positions(p, 9, 1, 10, p, p, p, None) == -1
    assert lib.sais_rank_positions(p, 10, 0, 10, p, p, p, None) == -1
    assert lib.sais_resize_bilinear_f32(None, 1, 37, 50, 0.5, p, 18, 25, None) == -1
    assert lib.sais_resize_bilinear_f32(p, 1, 37, 50, 0.5, p, 19, 25, None) == -1                   # not floor(H s)
    assert lib.sais_resize_bilinear_f32(p, 1, 37, 50, 0.0, p, 18, 25, None) == -1
    # host tensors raise: there is no CPU fallback
    x = torch.zeros(4, 128)
    with pytest.raises(_lib.SaisHipError):
        retrieval.PCAWhitening(128).fit(x)
    with pytest.raises(_lib.SaisHipError):
        retrieval.rank_positions(x, [[0]] * 4)
    with pytest.raises(_lib.SaisHipError):
        retrieval.copy_detection_topk(x, x)
    with pytest.raises(_lib.SaisHipError):
        retrieval.resize_bilinear(torch.zeros(1, 3, 32, 32), 0.5)
    with pytest.raises(_lib.SaisHipError):
        retrieval.multi_scale(torch.zeros(1, 3, 32, 32), lambda t: t)
    with pytest.raises(_lib.SaisHipError):
        vit_small(patch_size=16).retrieval_features(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError):
        retrieval.PCAWhitening(128).apply(x)
