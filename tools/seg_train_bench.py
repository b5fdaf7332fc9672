#!/usr/bin/env python3
"""What ONE segmented training pass over frames of different sizes costs (VisionTransformer.forward on a list under grad,
csrc/attn_seg.hip: sais_vit_attn_bwd_seg / sais_vit_embed_bwd_seg) against the resolution-group pass, forward + backward of the
12-block ViT-S/16, HIP events around the two calls, synthetic pixels.  The method of tools/mixed_batch_bench.py.

(a)  64 frames with the aspect ratios of tools/mixed_batch_bench.py's folder at imsize 224 (long side 224, the short side cut to a
     multiple of 16 as every backbone call does: the distinct shapes that leaves are counted in the record), as resolution groups
     (one group per shape, the yardstick) and as one segmented pass;
(a48) the same with 64 frames in 48 distinct shapes (long sides 224 / 208 / 192, short sides 80 .. 208), where nearly every frame
     is a group of its own;
(b)  the DINO student's crops at batch 64, 2 x 224 x 224 + 8 x 96 x 96 per image, as the default resident groups, as streaming
     groups and as segments.
Every leg runs TWICE per round (A/A: the spread of identical work), --rounds interleaved rounds after a warm-up round, medians
with [min, max].  A segmented leg includes building its host tables (one SegPlan per call, as forward(list) does).  One JSON
line, appended to --out.  Reads nothing outside the repository."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASPECTS = 48


def thumb_shapes(n, imsize=224):
    """(H, W) of n frames: mixed_batch_bench's aspect ratios (long side 800, short side 300 + 10 j, orientation alternating)
    scaled to long side imsize, both sides cut to multiples of 16"""
    out = []
    for i in range(n):
        j = i % ASPECTS
        short = max(16, int(round(imsize * (300 + 10 * j) / 800.0)) // 16 * 16)
        out.append((short, imsize) if j % 2 == 0 else (imsize, short))
    return out


def distinct_shapes(n, count=48):
    """n frames in `count` distinct (H, W): long sides 224 / 208 / 192 x short sides 80 .. 208 x two orientations"""
    pool = [(s, l) if o == 0 else (l, s) for l in (224, 208, 192) for s in range(80, 209, 16) for o in (0, 1) if s < l]
    pool = pool[:count]
    assert len(set(pool)) == count, len(set(pool))
    return [pool[i % count] for i in range(n)]


def summary(rec, name, v):
    rec[name + "_ms"] = round(statistics.median(v), 3)
    rec[name + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64, help="images per batch of leg (b); 0 skips the leg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_train_bench.jsonl"))
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from sais_amd.vit import vit_small
    dev = torch.device("cuda:0")
    model = vit_small(patch_size=16, depth=args.depth).to(dev).train()
    model._engine(dev)
    gen = torch.Generator().manual_seed(0)

    def frames_of(shapes):
        return [torch.randn(1, 3, h, w, generator=gen).to(dev) for h, w in shapes]

    def stacks_of(frames):
        groups = {}
        for t in frames:
            groups.setdefault(tuple(t.shape[2:]), []).append(t)
        return [torch.cat(g) for g in groups.values()]

    def group_pass(stacks, streaming):
        def run():
            with torch.no_grad():
                reps, saved = model._forward_kernels(stacks if len(stacks) > 1 else stacks[0], save=True, streaming=streaming)
                model._backward_kernels(saved, torch.ones_like(reps))
        return run

    def seg_pass(items):
        def run():
            with torch.no_grad():
                reps, saved = model._forward_kernels(items, save=True, streaming=True, seg=model._seg_plan(items))
                model._backward_kernels(saved, torch.ones_like(reps))
        return run

    def measure(rec, legs):
        calls = {}
        for name, f in legs.items():
            calls[name], calls[name + "_again"] = f, f
        for f in legs.values():                                     # warm-up round
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for name, f in calls.items():
                model.flat.grad.zero_()
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                f()
                ev1.record()
                torch.cuda.synchronize()
                times[name].append(ev0.elapsed_time(ev1))
        for name, v in times.items():
            summary(rec, name, v)
        for name in legs:
            rec[name + "_aa_pct"] = round(100.0 * abs(rec[name + "_ms"] - rec[name + "_again_ms"]) / rec[name + "_ms"], 2)

    def versus(rec, seg, base):
        gain = 100.0 * (rec[base + "_ms"] - rec[seg + "_ms"]) / rec[base + "_ms"]
        rec[f"{seg}_vs_{base}_pct"] = round(gain, 2)
        rec[f"{seg}_faster_than_{base}"] = bool(gain > rec[seg + "_aa_pct"] + rec[base + "_aa_pct"])
        rec[f"{seg}_slower_than_{base}"] = bool(-gain > rec[seg + "_aa_pct"] + rec[base + "_aa_pct"])

    rec = dict(frames=args.frames, rounds=args.rounds, depth=args.depth)
    for leg, shapes in (("a", thumb_shapes(args.frames)), ("a48", distinct_shapes(args.frames))):
        frames = frames_of(shapes)
        stacks = stacks_of(frames)
        rec[leg + "_shapes"] = len(stacks)
        rec[leg + "_rows"] = sum(1 + (h // 16) * (w // 16) for h, w in shapes)
        measure(rec, {leg + "_groups": group_pass(stacks, True), leg + "_segmented": seg_pass(frames)})
        versus(rec, leg + "_segmented", leg + "_groups")
        print(json.dumps({k: v for k, v in rec.items() if k.startswith(leg + "_")}), flush=True)
        del frames, stacks
    if args.batch:
        B = args.batch
        crops = [torch.randn(B, 3, 224, 224, generator=gen).to(dev) for _ in range(2)] + \
                [torch.randn(B, 3, 96, 96, generator=gen).to(dev) for _ in range(8)]
        stacks = [torch.cat(crops[:2]), torch.cat(crops[2:])]
        rec["b_batch"], rec["b_rows"] = B, 2 * B * 197 + 8 * B * 37
        measure(rec, {"b_resident_groups": group_pass(stacks, False), "b_streaming_groups": group_pass(stacks, True),
                      "b_segmented": seg_pass(crops)})
        versus(rec, "b_segmented", "b_resident_groups")
        versus(rec, "b_segmented", "b_streaming_groups")
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
