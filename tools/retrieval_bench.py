#!/usr/bin/env python3
"""Copy-detection / image-retrieval kernels (VisionTransformer.retrieval_features, csrc/retrieval.hip) on the GPU, with HIP events.

After a warm-up of every timed call, in `--rounds` interleaved rounds of `--iters` calls each (the median round is reported, the
spread as min / max), one JSON line per group, appended to --out (default profiles/retrieval_bench.jsonl):
  * descriptor: retrieval_features at 16 frames of 320 x 320 (eval_copy_detection.py's default batch) and at one 224 x 160 frame
    (a thumbnail of eval_image_retrieval.py), each next to dense_features(x, 1) + the reference's GeM lines in torch on its output
    (what the descriptor costs without the fused kernel), and sais_vit_cls_gem_norm alone with its bytes per second (the residual
    stream read once, the descriptor written);
  * covariance: sais_colmean_cov at 20 000 x 768 against torch.mm(X.T, X) / N plus torch.mean on the same card and data (rocBLAS
    f32), with the FLOP rate of the tiles actually computed (on or above the diagonal) and the largest difference of the two;
  * ranks: sais_rank_positions at 70 x 4 993 and 70 x 1 000 000 with 300 listed items per query against torch.argsort(-sim, dim=1)
    on the same data — the reference sorts the whole database and then looks the listed items up on the host, which is not timed —
    with the positions checked against the argsort at the smaller size."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(legs, rounds, iters):
    import torch
    for fn in legs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters)
    rec = {}
    for name, v in times.items():
        rec[name] = round(statistics.median(v), 4)
        rec[name.replace("_ms", "_minmax_ms")] = [round(min(v), 4), round(max(v), 4)]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        sys.exit("retrieval_bench.py measures on the GPU: no device found")
    from sais_amd import _lib as L, ops, retrieval
    from sais_amd.vit import vit_small
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=gen, device=dev)
    torch.manual_seed(0)
    model = vit_small(patch_size=16, num_classes=0).to(dev).eval()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")

    def torch_gem(x):                                   # eval_copy_detection.py:166-175 on dense_features' output
        feats = model.dense_features(x, 1)[0]
        b, h, w = x.shape[0], x.shape[2] // 16, x.shape[3] // 16
        p = feats[:, 1:, :].reshape(b, h, w, 384).clamp(min=1e-6).permute(0, 3, 1, 2)
        p = torch.nn.functional.avg_pool2d(p.pow(4), (h, w)).pow(1. / 4).reshape(b, -1)
        return torch.cat((feats[:, 0, :], p), dim=1)

    # ---- descriptor
    f = model._engine(dev)
    for F, H, W in ((16, 320, 320), (1, 224, 160)):
        x = rn(F, 3, H, W)
        ntok = 1 + (H // 16) * (W // 16)
        xs = rn(F * ntok, 384)
        y = torch.empty(F, 768, device=dev)
        g, b = f.w32("norm.weight"), f.w32("norm.bias")
        rec = dict(tool="retrieval_bench", group="descriptor", rounds=args.rounds, iters=args.iters, frame=f"{H}x{W}", frames=F,
                   tokens=ntok)
        rec.update(timed({
            "retrieval_features_ms": lambda: model.retrieval_features(x),
            "dense_plus_torch_gem_ms": lambda: torch_gem(x),
            "retrieval_features_aa_ms": lambda: model.retrieval_features(x),
            "cls_gem_norm_ms": lambda: ops.vit_cls_gem_norm(xs, F, ntok, g, b, 1e-6, y),
        }, args.rounds, args.iters))
        rec["cls_gem_norm_gbps"] = round((F * ntok * 384 + F * 768) * 4 / rec["cls_gem_norm_ms"] / 1e6, 1)
        a, t = model.retrieval_features(x), torch_gem(x)
        rec["max_rel_diff_vs_torch_gem"] = float(((a - t).abs() / t.abs().clamp(min=1e-6)).max())
        emit(rec)

    # ---- covariance
    N, Dm = 20000, 768
    X = rn(N, Dm) * torch.exp(rn(1, Dm) * 0.5) + 0.3 * rn(1, Dm)
    mean, cov = torch.empty(Dm, device=dev), torch.empty(Dm, Dm, device=dev)
    rec = dict(tool="retrieval_bench", group="covariance", rounds=args.rounds, iters=args.iters, N=N, D=Dm,
               workspace_bytes=int(L.load().sais_colmean_cov_workspace_bytes(N, Dm)))
    rec.update(timed({
        "colmean_cov_ms": lambda: ops.colmean_cov(X, mean, cov),
        "torch_mm_mean_ms": lambda: (torch.mm(X.T, X) / N, torch.mean(X, dim=0)),
        "colmean_cov_aa_ms": lambda: ops.colmean_cov(X, mean, cov),
    }, args.rounds, args.iters))
    tiles = (Dm // 64) * (Dm // 64 + 1) // 2
    rec["colmean_cov_tflops_computed_tiles"] = round(2.0 * N * tiles * 64 * 64 / rec["colmean_cov_ms"] / 1e9, 2)
    ops.colmean_cov(X, mean, cov)
    tc = torch.mm(X.T, X) / N
    rec["max_abs_diff_vs_torch_mm"] = float((cov - tc).abs().max())
    rec["max_abs_cov"] = float(tc.abs().max())
    rec["bit_symmetric"] = bool(torch.equal(cov, cov.T))
    emit(rec)

    # ---- ranks
    for nq, ndb in ((70, 4993), (70, 1000000)):
        sim = rn(nq, ndb)
        rng = np.random.Generator(np.random.PCG64(ndb))
        lists = [rng.permutation(ndb)[:300] for _ in range(nq)]
        items = torch.from_numpy(np.concatenate(lists).astype(np.int32)).to(dev)
        off = torch.from_numpy((np.arange(nq + 1) * 300).astype(np.int32)).to(dev)
        pos = torch.empty(nq * 300, dtype=torch.int32, device=dev)
        rec = dict(tool="retrieval_bench", group="ranks", rounds=args.rounds, iters=args.iters, queries=nq, database=ndb,
                   items_per_query=300)
        rec.update(timed({
            "rank_positions_ms": lambda: ops.rank_positions(sim, off, items, pos),
            "torch_argsort_ms": lambda: torch.argsort(-sim, dim=1),
            "rank_positions_aa_ms": lambda: ops.rank_positions(sim, off, items, pos),
        }, args.rounds, args.iters if ndb < 100000 else max(1, args.iters // 2)))
        rec["rank_positions_gcompares_per_s"] = round(nq * 300.0 * ndb / rec["rank_positions_ms"] / 1e6, 1)
        if ndb < 100000:
            ops.rank_positions(sim, off, items, pos)
            s = sim.cpu().numpy()
            want = np.concatenate([np.argsort(np.argsort(-s[q], kind="stable"), kind="stable")[lists[q]] for q in range(nq)])
            rec["positions_equal_stable_argsort"] = bool((pos.cpu().numpy() == want).all())
        emit(rec)


if __name__ == "__main__":
    main()
