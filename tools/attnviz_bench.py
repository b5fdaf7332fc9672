#!/usr/bin/env python3
"""Attention-map rendering path (VisionTransformer.cls_attention, sais_amd.attnviz) on the GPU, with HIP events.

Per shape — 480 x 848 (1591 tokens) with F = 1 and F = 16, 224 x 224 with F = 64 — after a warm-up of every timed call, in
`--rounds` interleaved rounds of `--iters` calls each (the median round is reported, the spread as min / max):
  * cls_attention, twice (the two legs run the same code: their difference is the run's A/A spread), and dense_features(x, 1)
    at the same shape as the yardstick of the pass: cls_attention does strictly less (no V, attention, proj, MLP of the last
    block), so it should not be slower beyond 2 x the A/A spread; `cls_vs_dense_ok` says whether that held
  * sais_vit_cls_probs alone, mass_mask, render (threshold given as a ready mask: the render launches alone)
  * the scripts' own formulation of the tail (video_generation.py:195-238: sort, normalise, cumsum, compare, argsort, the
    head loop, two nearest interpolations, the product, the head mean) written out in torch on the same card, per frame as the
    script runs it; its masks and heat maps are compared with the kernels' on the timed inputs
  * the host-side matplotlib colormap (ScalarMappable.to_rgba(bytes=True) of one upsampled map) separately, as host wall time
One JSON line per shape, appended to --out (default profiles/attnviz_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(480, 848, 1), (480, 848, 16), (224, 224, 64)]


def torch_tail(probs, h, w, threshold, patch=16):
    """One frame at a time, as the script: probs f32 [F, 6, 1 + hw] -> (masks bool [F, 6, hw], maps f32 [F, h patch, w patch])"""
    import torch
    masks, maps = [], []
    for f in range(probs.shape[0]):
        att = probs[f, :, 1:]
        nh = att.shape[0]
        val, idx = torch.sort(att)
        val = val / torch.sum(val, dim=1, keepdim=True)
        th = torch.cumsum(val, dim=1) > (1 - threshold)
        back = torch.argsort(idx)
        for head in range(nh):
            th[head] = th[head][back[head]]
        masks.append(th.clone())
        up = lambda t: torch.nn.functional.interpolate(t.reshape(1, nh, h, w), scale_factor=patch, mode="nearest")[0]
        a = up(att) * up(th.float())
        maps.append(sum(a[i] * 1 / nh for i in range(nh)))
    return torch.stack(masks), torch.stack(maps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attnviz_bench.jsonl"))
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        sys.exit("attnviz_bench.py measures on the GPU: no device found")
    from sais_amd import attnviz, ops
    from sais_amd.vit import vit_small
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=gen, device=dev)
    torch.manual_seed(0)
    model = vit_small(patch_size=16).to(dev).eval()
    threshold = 0.6
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for H, W, F in SHAPES:
        h, w = H // 16, W // 16
        ntok = 1 + h * w
        x = rn(F, 3, H, W)
        qkv = (rn(F * ntok, 1152) * 1.5).bfloat16()
        q, k = qkv.view(F, ntok, 1152)[:, 0, :384], qkv[:, 384:768]
        pbuf = torch.empty(F, 6, ntok, device=dev)
        probs = model.cls_attention(x)
        keep = attnviz.mass_mask(probs, threshold)
        legs = {
            "cls_attention_ms": lambda: model.cls_attention(x),
            "dense_features_ms": lambda: model.dense_features(x, 1),
            "cls_attention_aa_ms": lambda: model.cls_attention(x),
            "cls_probs_ms": lambda: ops.vit_cls_probs(q, k, F, ntok, pbuf),
            "mass_mask_ms": lambda: attnviz.mass_mask(probs, threshold),
            "render_ms": lambda: attnviz.render(probs, (h, w), keep=keep, cmap="inferno", patch=16),
            "tail_torch_ms": lambda: torch_tail(probs, h, w, threshold),
        }
        for fn in legs.values():                                   # warm-up of every timed shape
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        for _ in range(args.rounds):                               # interleaved: every leg once per round
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.iters)
        rec = dict(tool="attnviz_bench", rounds=args.rounds, iters=args.iters, frame=f"{H}x{W}", frames=F, tokens=ntok,
                   threshold=threshold)
        for name, v in times.items():
            rec[name] = round(statistics.median(v), 4)
            rec[name.replace("_ms", "_minmax_ms")] = [round(min(v), 4), round(max(v), 4)]
        spread = abs(rec["cls_attention_ms"] - rec["cls_attention_aa_ms"])
        rec["aa_spread_ms"] = round(spread, 4)
        rec["cls_vs_dense_ok"] = bool(min(rec["cls_attention_ms"], rec["cls_attention_aa_ms"]) <= rec["dense_features_ms"] + 2 * spread)
        rec["kernel_tail_ms"] = round(rec["mass_mask_ms"] + rec["render_ms"], 4)
        # K once (bf16), the probabilities once
        rec["cls_probs_gbps"] = round(F * ntok * (768 + 24) / rec["cls_probs_ms"] / 1e6, 1)
        tm, tmap = torch_tail(probs, h, w, threshold)
        heat, rgb = attnviz.render(probs, (h, w), keep=keep, cmap="inferno", patch=16)
        rec["mask_elements_off_vs_torch"] = [int((tm != keep.bool()).sum()), int(keep.numel())]     # f32 cumsum at the cut, tie order
        same = tm == keep.bool()
        small = tmap[:, ::16, ::16]
        ok = same.all(dim=1).view(F, h, w)                          # compare the maps where all six masks agree
        rec["heat_max_abs_diff_vs_torch"] = float(((small - heat).abs() * ok).max())
        try:
            import matplotlib
            matplotlib.use("Agg")
            from matplotlib.cm import ScalarMappable
            arr = tmap[0].cpu().numpy()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                ScalarMappable(cmap="inferno").to_rgba(arr, bytes=True)
                ts.append((time.perf_counter() - t0) * 1e3)
            rec["host_matplotlib_colormap_per_frame_ms"] = round(statistics.median(ts), 3)
        except ImportError:
            rec["host_matplotlib_colormap_per_frame_ms"] = None
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
