#!/usr/bin/env python3
"""Golden results of the copy-detection / image-retrieval evaluations, produced by RUNNING THE REFERENCE's own functions on the
CPU (build container only: needs /root/reference).

    python tests/golden/make_golden_retrieval.py        # rewrites tests/golden/retrieval.npz

Reference entry points exercised (SAIS/scripts/dino-main), on the inputs of tests/retrieval_ref.py:
  utils.compute_map / utils.compute_ap (utils.py:709-813) on the MAP_CASE similarity matrix under the Medium and Hard groupings
      of eval_image_retrieval.py:184-197, with the rank matrix it builds (argsort of -sim along the database axis);
  score_ap_from_ranks_1 (eval_copy_detection.py:97-125) on the rank lists of make_copydays_ranks;
  utils.PCA(dim, whit=0.5).train_pca / apply inside the pipeline of eval_copy_detection.py:276-295 (mean of the whitening set,
      uncentred covariance by torch.mm, centre, whiten, F.normalize, torch.mm) on the two WHITEN_CASES, all in f32 on the CPU;
  utils.multi_scale (utils.py:816-830) with a stub model that records its three inputs, on the FRAME_CASE frame.
eval_copy_detection.py imports torchvision at the top, which is stubbed (never touched on these paths).

GeM: the reference's lines (eval_copy_detection.py:166-175) sit inside extract_features, which calls .cuda() and a distributed
all_gather, so they cannot run here.  The fp64 restatement retrieval_ref.gem_descriptor alone stands for GeM in the tests.

No input array is stored: retrieval.npz holds results and a sha256 of the generated inputs, which the tests regenerate and
compare.  The script asserts what keeps the tests honest: on the whitening cases the reference's own f32 similarities lie within
1e-3 of the fp64 restatement (otherwise change the seed of the case in retrieval_ref.WHITEN_CASES, not the bar)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import retrieval_ref as R  # noqa: E402

REF = "/root/reference/SAIS/scripts"


def import_reference():
    for name in ("timm", "torchvision", "h5py", "cv2"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    tv = sys.modules["torchvision"]
    for sub in ("transforms", "models", "datasets"):
        m = types.ModuleType("torchvision." + sub)
        setattr(tv, sub, m)
        sys.modules["torchvision." + sub] = m
    tv.datasets.ImageFolder = object
    sys.path.insert(0, os.path.join(REF, "dino-main"))
    import eval_copy_detection
    import utils
    return eval_copy_detection, utils


class Recorder(torch.nn.Module):
    """model(inp) of utils.multi_scale: keeps every input, returns a feature that depends on it"""

    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x):
        self.seen.append(x.clone())
        return torch.stack([x.mean(), x.abs().mean(), x.std(), x.max()]).reshape(1, 4)


if __name__ == "__main__":
    ecd, utils = import_reference()
    out = {}

    # ---- mAP / precision at k
    nq, ndb, seed = R.MAP_CASE
    sim, gnd = R.make_map_case(nq, ndb, seed)
    out["map_sha256"] = R.digest(sim, *[g[k] for g in gnd for k in ("easy", "hard", "junk")])
    ranks = np.argsort(-sim.T, axis=0, kind="stable")                  # [ndb, nq], as torch.argsort(-sim, dim=0) of :176
    for tag, g in zip("MH", R.protocols(gnd)):
        m, aps, pr, prs = utils.compute_map(ranks, g, list(R.KAPPAS))
        out[f"map_{tag}"], out[f"aps_{tag}"], out[f"pr_{tag}"], out[f"prs_{tag}"] = np.float64(m), aps, pr, prs
        print(f"compute_map {tag}: mAP {m:.6f}  mP@k {pr}  skipped {int(np.isnan(aps).sum())}")
        mine = R.map_from_order(ranks, g)
        assert abs(mine[0] - m) < 1e-12 and np.allclose(mine[2], pr, atol=1e-12, rtol=0)
    assert np.isnan(out["aps_M"]).sum() == 1 and np.isnan(out["aps_H"]).sum() == 2
    out["compute_ap"] = np.asarray([utils.compute_ap(np.asarray(r), n) for r, n in R.make_copydays_ranks(R.COPYDAYS_CASE)])

    # ---- Holidays AP
    out["copydays_ap"] = np.asarray([ecd.score_ap_from_ranks_1(r, n) for r, n in R.make_copydays_ranks(R.COPYDAYS_CASE)])

    # ---- whitening
    for name, N, D, ndb, nq, seed in R.WHITEN_CASES:
        W, db, q = R.make_whiten_case(N, D, ndb, nq, seed)
        out[f"whiten_{name}_sha256"] = R.digest(W, db, q)
        feats, database, queries = torch.from_numpy(W), torch.from_numpy(db.copy()), torch.from_numpy(q.copy())
        mean_feature = torch.mean(feats, dim=0)
        database -= mean_feature
        queries -= mean_feature
        pca = utils.PCA(dim=D, whit=0.5)
        cov = torch.mm(feats.T, feats) / feats.shape[0]
        pca.train_pca(cov.cpu().numpy())
        database, queries = pca.apply(database), pca.apply(queries)
        database = torch.nn.functional.normalize(database, dim=1, p=2)
        queries = torch.nn.functional.normalize(queries, dim=1, p=2)
        s32 = torch.mm(queries, database.T).numpy()
        s64 = R.whitened_similarity(W, db, q, D)
        err = float(np.abs(s32.astype(np.float64) - s64).max())
        floored = int((np.linalg.eigvalsh(R.colmean_cov(W)[1]) < 1e-5 * np.linalg.eigvalsh(R.colmean_cov(W)[1]).max()).sum())
        print(f"whitening {name}: reference f32 vs fp64 restatement max |d sim| = {err:.3e}; floored eigenvalues {floored}")
        assert err <= 1e-3, "change the seed of this case (retrieval_ref.WHITEN_CASES), not the bar"
        assert (floored > 0) == (N < D)
        out[f"whiten_{name}_sim"] = s32
        out[f"whiten_{name}_ref_err"] = np.float64(err)

    # ---- multi_scale
    H, Wd, seed = R.FRAME_CASE
    frame = R.make_frame(H, Wd, seed)
    out["frame_sha256"] = R.digest(frame)
    rec = Recorder()
    v = utils.multi_scale(torch.from_numpy(frame), rec)
    assert len(rec.seen) == 3
    out["multi_scale_out"] = v.numpy()
    for i, t in enumerate(rec.seen):
        out[f"multi_scale_in{i}"] = t.numpy()
        mine = frame.astype(np.float64) if i == 0 else R.resize_bilinear(frame, R.SCALES[i])
        d = float(np.abs(mine - t.numpy()).max())
        print(f"multi_scale input {i}: {tuple(t.shape)}  restatement max |d| = {d:.3e}")
        assert mine.shape == tuple(t.shape) and d <= 8 * R.U24 * float(np.abs(frame).max())

    np.savez_compressed(os.path.join(HERE, "retrieval.npz"), **out)
    print(len(out), "arrays")
