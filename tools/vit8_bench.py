#!/usr/bin/env python3
"""The patch-8 backbone (vit_small(patch_size=8), inference) on the GPU, with HIP events.

Measured, after a warm-up of every timed shape, in `--rounds` interleaved rounds of `--iters` calls each (the median round is
reported, the spread as min / max), random ViT-S/8 weights:
  * model(x) at 64 x 224 x 224 (785 tokens: the extraction pass of k-NN, linear probe and retrieval) with the CLS-only last
    block (sais_vit_attn_cls_fwd_any) and with every row of the last block computed (prune_last_block = False)
  * dense_features and cls_attention at 1 x 480 x 480 (3601 tokens)
  * the two kernels of csrc/vit8.hip alone: sais_patchify_rect8 at 64 x 224 x 224, sais_vit_attn_cls_fwd_any at 64 x 785 and
    1 x 4097, beside the streaming attention over every query (sais_vit_attn_fwd_any) on the same qkv
One JSON line per run, appended to profiles/vit8_bench.jsonl with --append."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--append", action="store_true", help="append the JSON line to profiles/vit8_bench.jsonl")
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        sys.exit("vit8_bench.py measures on the GPU: no device found")
    from sais_amd import ops
    from sais_amd.vit import vit_small
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=gen, device=dev)
    bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)
    model = vit_small(patch_size=8).to(dev).eval()
    x64, x480 = rn(64, 3, 224, 224), rn(1, 3, 480, 480)
    qkv785, qkv4097 = (rn(64 * 785, 1152) * 1.5).bfloat16(), (rn(4097, 1152) * 1.5).bfloat16()
    patches, c785, c4097, o785, o4097 = bf(64 * 784, 192), bf(64, 384), bf(1, 384), bf(64 * 785, 384), bf(4097, 384)

    def forward(prune):
        model.prune_last_block = prune
        with torch.no_grad():
            return model(x64)

    legs = {
        "forward_64x224_cls_tail_ms": lambda: forward(True),
        "forward_64x224_every_row_ms": lambda: forward(False),
        "dense_features_480x480_ms": lambda: model.dense_features(x480, 1),
        "cls_attention_480x480_ms": lambda: model.cls_attention(x480),
        "patchify_rect8_64x224_ms": lambda: ops.patchify_rect8(x64, patches),
        "attn_cls_any_785x64_ms": lambda: ops.vit_attn_cls_fwd_any(qkv785, 64, 785, c785),
        "attn_any_785x64_ms": lambda: ops.vit_attn_fwd_any(qkv785, 64, 785, o785),
        "attn_cls_any_4097x1_ms": lambda: ops.vit_attn_cls_fwd_any(qkv4097, 1, 4097, c4097),
        "attn_any_4097x1_ms": lambda: ops.vit_attn_fwd_any(qkv4097, 1, 4097, o4097),
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
    model.prune_last_block = True
    rec = dict(tool="vit8_bench", rounds=args.rounds, iters=args.iters, patch=8, forward="64x224x224 (785 tokens)",
               dense="1x480x480 (3601 tokens)")
    for k, v in times.items():
        rec[k] = round(statistics.median(v), 4)
        rec[k.replace("_ms", "_minmax_ms")] = [round(min(v), 4), round(max(v), 4)]
    # the kernels' own traffic: pixels in + patches out; K and V of every token once
    rec["patchify_rect8_gbps"] = round(64 * 3 * 224 * 224 * 6 / rec["patchify_rect8_64x224_ms"] / 1e6, 1)
    rec["attn_cls_any_785x64_gbps"] = round(64 * 785 * 768 * 2 / rec["attn_cls_any_785x64_ms"] / 1e6, 1)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.append:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "vit8_bench.jsonl"), "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
