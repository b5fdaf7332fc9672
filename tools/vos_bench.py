#!/usr/bin/env python3
"""Video object segmentation path (VisionTransformer.dense_features, sais_amd.vos) on the GPU, with HIP events.

Measured, after a warm-up of every timed shape, in `--rounds` interleaved rounds of `--iters` calls each (the median round is
reported, the spread as min / max):
  * dense_features at 480 x 832 (1561 tokens), F = 1 and F = 6, random ViT-S/16 weights
  * the streaming attention (sais_vit_attn_fwd_any) against the LDS-resident kernel (sais_vit_attn_fwd) at ntok = 197, and the
    streaming attention alone at 1561 tokens
  * one propagation step at 30 x 52, nctx = 8, r = 12, topk = 5, C = 3 (normalised features in place) against the reference's
    formulation (eval_video_segmentation.py:113-150: bmm + dense mask + topk + mm) written out in torch on the same card; the
    two results are compared on the timed inputs
  * the upsample / norm_mask / argmax tail at 30 x 52, patch 16, against F.interpolate + the per-channel loop + torch.max
One JSON line per run, appended to profiles/vos_bench.jsonl with --append."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_propagation(tar_n, ctx_n, segs, mask, topk):
    """label_propagation (:125-149) on normalised features: tar_n [n, d], ctx_n [nctx, n, d], segs [nctx, C, n], mask [n, n]"""
    import torch
    nctx, C, n = segs.shape
    aff = torch.exp(torch.bmm(tar_n.unsqueeze(0).expand(nctx, -1, -1), ctx_n.transpose(1, 2)) / 0.1)      # [nctx, q, key]
    aff = aff * mask.unsqueeze(0)
    aff = aff.transpose(2, 1).reshape(-1, n)
    tk_val, _ = torch.topk(aff, dim=0, k=topk)
    aff[aff < tk_val.min(dim=0)[0]] = 0
    aff = aff / aff.sum(dim=0, keepdim=True)
    return torch.mm(segs.transpose(0, 1).reshape(C, nctx * n), aff)


def torch_tail(seg, patch):
    import torch
    up = torch.nn.functional.interpolate(seg[None], scale_factor=patch, mode="bilinear", align_corners=False,
                                         recompute_scale_factor=False)[0]
    for c in range(up.shape[0]):
        if up[c].max() > 0:
            m = up[c] - up[c].min()
            up[c] = m / m.max()
    return torch.max(up, dim=0)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--append", action="store_true", help="append the JSON line to profiles/vos_bench.jsonl")
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        sys.exit("vos_bench.py measures on the GPU: no device found")
    from sais_amd import ops, vos
    from sais_amd.vit import vit_small
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=gen, device=dev)
    model = vit_small(patch_size=16).to(dev).eval()
    H, W, h, w, n, nctx, C, r, topk, patch = 480, 832, 30, 52, 1560, 8, 3, 12, 5, 16

    x1, x6 = rn(1, 3, H, W), rn(6, 3, H, W)
    qkv197, qkv1561 = (rn(64 * 197, 1152) * 1.5).bfloat16(), (rn(1561, 1152) * 1.5).bfloat16()
    o197, o1561 = torch.empty(64 * 197, 384, dtype=torch.bfloat16, device=dev), torch.empty(1561, 384, dtype=torch.bfloat16, device=dev)
    base = rn(n, 384)
    tar_n = vos.normalize_rows(base + 0.5 * rn(n, 384))
    ctx_n = vos.normalize_rows((base[None] + 0.5 * rn(nctx, n, 384)).view(nctx * n, 384)).view(nctx, n, 384)
    segs = torch.softmax(2 * rn(nctx, C, n), dim=1).contiguous()
    yy, xx = torch.arange(n, device=dev) // w, torch.arange(n, device=dev) % w
    mask = (((yy[:, None] - yy[None]).abs() <= r) & ((xx[:, None] - xx[None]).abs() <= r)).float()
    seg = torch.softmax(2 * rn(C, h, w), dim=0).contiguous()

    legs = {
        "dense_features_f1_ms": lambda: model.dense_features(x1, 1),
        "dense_features_f6_ms": lambda: model.dense_features(x6, 1),
        "attn_any_197x64_ms": lambda: ops.vit_attn_fwd_any(qkv197, 64, 197, o197),
        "attn_resident_197x64_ms": lambda: ops.vit_attn_fwd(qkv197, 64, o197, ntok=197),
        "attn_any_1561x1_ms": lambda: ops.vit_attn_fwd_any(qkv1561, 1, 1561, o1561),
        "propagate_ms": lambda: vos.propagate_normalized(tar_n, ctx_n, segs, h, w, r, topk),
        "propagate_torch_ms": lambda: torch_propagation(tar_n, ctx_n, segs, mask, topk),
        "tail_ms": lambda: vos.upsample_argmax(seg, patch),
        "tail_torch_ms": lambda: torch_tail(seg, patch),
    }
    for fn in legs.values():                                   # warm-up of every timed shape
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                               # interleaved: every leg once per round
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.iters)
    rec = dict(tool="vos_bench", rounds=args.rounds, iters=args.iters, frame="480x832", tokens=1561, grid="30x52", nctx=nctx,
               radius=r, topk=topk, classes=C)
    for k, v in times.items():
        rec[k] = round(statistics.median(v), 4)
        rec[k.replace("_ms", "_minmax_ms")] = [round(min(v), 4), round(max(v), 4)]
    a, b = vos.propagate_normalized(tar_n, ctx_n, segs, h, w, r, topk), torch_propagation(tar_n, ctx_n, segs, mask, topk)
    d = (a - b).abs().amax(dim=0)                              # per query: the two differ where f32 cosines order a near-tie at
    rec["propagate_max_abs_diff_vs_torch"] = float(d.max())    # the top-k cut differently (the kernel is held to fp64 by the tests)
    rec["propagate_median_abs_diff_vs_torch"] = float(d.median())
    rec["propagate_queries_off_vs_torch"] = [int((d > 1e-3).sum()), n]
    rec["tail_label_agreement_vs_torch"] = float((vos.upsample_argmax(seg, patch).long() == torch_tail(seg.clone(), patch)).float().mean())
    # 4 F heads ntok^2 64 operations per attention call
    rec["attn_any_1561x1_tflops"] = round(4.0 * 6 * 1561 * 1561 * 64 / rec["attn_any_1561x1_ms"] / 1e9, 1)
    rec["attn_any_197x64_tflops"] = round(4.0 * 64 * 6 * 197 * 197 * 64 / rec["attn_any_197x64_ms"] / 1e9, 1)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.append:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "vos_bench.jsonl"), "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
