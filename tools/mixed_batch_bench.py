#!/usr/bin/env python3
"""What one segmented backbone pass over thumbnails of many shapes buys (VisionTransformer.retrieval_features on a list,
csrc/attn_seg.hip; eval_image_retrieval.py --mixed_batch true) against the tool's two other ways to run the backbone behind
--gpu_loader: one call per image, and --group_shapes.  The method of tools/thumbnail_bench.py, on a synthetic roxford5k folder the
tool writes: --files JPEGs of 48 aspect ratios (long side 800), so that the thumbnails of a loader batch mostly find no partner of
their shape; the number of distinct thumbnail shapes is printed per imsize.

(a) the backbone alone on ONE loader batch of --loader_batch thumbnails already on the device, HIP events, three ways:
      single    one retrieval_features call per thumbnail
      grouped   one call per group of equal shapes (what --group_shapes stacks)
      mixed     one segmented pass over the list
(b) the extraction loop retrieval.extract_features(cls_features(vit_small), ThumbnailBatches(...)) over all files, wall clock,
    in the three modes;
(c) the same with multi_scale.
Every leg runs TWICE per round (A/A: the spread of identical work), --rounds interleaved rounds after a warm-up round, medians with
[min, max].  The yardsticks are the two older modes in the same run on the same card.  One JSON line per imsize, appended to --out."""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASPECTS = 48


def write_folder(root, n, seed=0):
    rng = np.random.default_rng(seed)
    d = os.path.join(root, "roxford5k", "jpg")
    os.makedirs(d, exist_ok=True)
    names = []
    for i in range(n):
        j = i % ASPECTS
        long_side, short = 800, 300 + 10 * j
        w, h = (long_side, short) if j % 2 == 0 else (short, long_side)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([128 + 90 * np.sin(xx / (29.0 + i % 7) + c) * np.cos(yy / (17.0 + i % 5)) for c in range(3)], -1)
        a = np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
        names.append("img%04d" % i)
        Image.fromarray(a).save(os.path.join(d, names[-1] + ".jpg"), quality=(75, 90)[i // 2 % 2])
    with open(os.path.join(root, "roxford5k", "gnd_roxford5k.pkl"), "wb") as fh:
        pickle.dump({"imlist": names, "qimlist": names[:1], "gnd": [{"easy": [0], "hard": [], "junk": []}]}, fh)


def summary(rec, name, v):
    rec[name + "_ms"] = round(statistics.median(v), 3)
    rec[name + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]


def aa(rec, name):
    """A/A spread of a leg in percent of its median: |median(first) - median(again)|"""
    rec[name + "_aa_pct"] = round(100.0 * abs(rec[name + "_ms"] - rec[name + "_again_ms"]) / rec[name + "_ms"], 2)
    return rec[name + "_aa_pct"]


def verdict(rec, leg):
    """the segmented pass against --group_shapes: faster by more than the two legs' A/A spreads, or not"""
    g, m = rec[f"{leg}_grouped_ms"], rec[f"{leg}_mixed_ms"]
    gain = 100.0 * (g - m) / g
    rec[f"{leg}_mixed_vs_grouped_pct"] = round(gain, 2)
    rec[f"{leg}_mixed_faster_than_grouped"] = bool(gain > rec[f"{leg}_grouped_aa_pct"] + rec[f"{leg}_mixed_aa_pct"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--imsize", type=int, nargs="+", default=[224, 512])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--loader_batch", type=int, default=64)
    ap.add_argument("--multiscale", type=int, default=1, help="0: skip leg (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_batch_bench.jsonl"))
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from sais_amd import imgfolder, retrieval
    from sais_amd.vit import vit_small
    dev = torch.device("cuda:0")
    model = vit_small(patch_size=16, num_classes=0).to(dev).eval()
    cls = retrieval.cls_features(model)
    ms = lambda x: retrieval.multi_scale(x, cls)                    # noqa: E731
    with tempfile.TemporaryDirectory() as root:
        write_folder(root, args.files)
        raw = imgfolder.RawOxfordParis(root, "roxford5k", "train")
        items, _ = imgfolder.collate_raw([raw[i] for i in range(len(raw))])
        for imsize in args.imsize:
            loader = imgfolder.GpuImageLoader(dev)
            thumbs = loader.thumbnail(items, imsize)
            shapes = {tuple(t.shape[2:]) for t in thumbs}
            print(f"imsize {imsize}: {len(thumbs)} thumbnails in {len(shapes)} distinct shapes", flush=True)
            assert len(shapes) >= 32 or args.files < 64, len(shapes)
            rec = dict(files=len(items), imsize=imsize, shapes=len(shapes), loader_batch=args.loader_batch, rounds=args.rounds)

            # (a) the backbone on one loader batch, HIP events
            batch = thumbs[:args.loader_batch]
            groups = {}
            for t in batch:
                groups.setdefault(tuple(t.shape[2:]), []).append(t)
            stacks = [torch.cat(g) for g in groups.values()]
            rec["batch_shapes"], rec["batch_tokens"] = len(stacks), sum(1 + (t.shape[2] // 16) * (t.shape[3] // 16) for t in batch)
            legs = {"single": lambda: [cls(t) for t in batch], "grouped": lambda: [cls(s) for s in stacks],
                    "mixed": lambda: cls(batch)}
            calls = {}
            for name, f in legs.items():
                calls["backbone_" + name], calls["backbone_" + name + "_again"] = f, f
            for f in legs.values():
                f()
            torch.cuda.synchronize()
            times = {k: [] for k in calls}
            for _ in range(args.rounds):
                for name, f in calls.items():
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                    f()
                    ev1.record()
                    torch.cuda.synchronize()
                    times[name].append(ev0.elapsed_time(ev1))
            for name, v in times.items():
                summary(rec, name, v)
            for name in legs:
                aa(rec, "backbone_" + name)
            verdict(rec, "backbone")
            one = torch.cat([cls(t) for t in batch])
            rec["backbone_mixed_max_abs_diff_vs_single"] = float((cls(batch) - one).abs().max())

            # (b), (c) the extraction loop in the three modes
            def loop(group, mixed):
                return retrieval.ThumbnailBatches(torch.utils.data.DataLoader(
                    raw, batch_size=args.loader_batch, num_workers=args.workers, collate_fn=imgfolder.collate_raw), loader,
                    imsize, group, mixed=mixed)
            modes = {"single": (False, False), "grouped": (True, False), "mixed": (False, True)}
            for leg, fn in (("extract", cls), ("extract_ms", ms))[:2 if args.multiscale else 1]:
                loops = {}
                for name, (g, m) in modes.items():
                    loops[f"{leg}_{name}"] = loops[f"{leg}_{name}_again"] = (g, m)
                feats, wall = {}, {k: [] for k in loops}
                for r in range(args.rounds + 1):                     # round 0 is the warm-up
                    for name, (g, m) in loops.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        feats[name] = retrieval.extract_features(fn, loop(g, m), dev)
                        torch.cuda.synchronize()
                        if r:
                            wall[name].append((time.perf_counter() - t0) * 1e3)
                for name, v in wall.items():
                    summary(rec, name, v)
                for name in modes:
                    aa(rec, f"{leg}_{name}")
                verdict(rec, leg)
                unit = lambda x: x / x.norm(dim=1, keepdim=True)      # noqa: E731
                rec[f"{leg}_mixed_max_abs_diff_vs_single_unit_rows"] = float(
                    (unit(feats[f"{leg}_mixed"]) - unit(feats[f"{leg}_single"])).abs().max())
            line = json.dumps(rec)
            print(line, flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
