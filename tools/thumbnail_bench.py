#!/usr/bin/env python3
"""The retrieval loader on the GPU (GpuImageLoader.thumbnail, csrc/thumbnail.hip) against retrieval.OxfordParisDataset on
Pillow, on a synthetic roxford5k folder the tool writes: --files JPEGs, 1024x768 and 768x1024 at quality 75 / 90 (what ROxford
and RParis mostly hold) and a few of other sizes, for --imsize 224 and 512.

(a) the loader.  HIP events around each call, after a warm-up of every call, in --rounds interleaved rounds of --iters calls;
    the median round with [min, max], and `loader_call` twice per round (A/A) so that the spread of identical work shows:
      thumbnail        sais_thumbnail alone (reduce + resample launches), decoded images already on the device
      loader_call      GpuImageLoader.thumbnail(items): plan, pinned pack, H2D, decode, status read, sais_thumbnail
    and, with the wall clock, OxfordParisDataset through a DataLoader of --workers processes on this host (second pass, the
    workers already running, one sixteenth of the files per worker batch).
(b) the extraction loop, retrieval.extract_features(cls_features(vit_small), ...) over the same files, wall clock, --rounds
    interleaved rounds, median with [min, max]: the Pillow loader at batch 1 with --workers workers (what the tool runs
    without switches), --gpu_loader per image, --gpu_loader --group_shapes (--loader_batch files per decode call).
The loader's images are checked against the dataset's bit for bit.  One JSON line per imsize, appended to --out."""
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
OTHER = [(500, 375), (640, 480), (800, 1067), (1600, 1200)]


def write_folder(root, n, seed=0):
    rng = np.random.default_rng(seed)
    d = os.path.join(root, "roxford5k", "jpg")
    os.makedirs(d, exist_ok=True)
    names = []
    for i in range(n):
        w, h = OTHER[i // 16 % len(OTHER)] if i % 16 == 15 else ((1024, 768), (768, 1024))[i % 2]
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([128 + 90 * np.sin(xx / (29.0 + i % 7) + c) * np.cos(yy / (17.0 + i % 5)) for c in range(3)], -1)
        a = np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
        names.append("img%04d" % i)
        Image.fromarray(a).save(os.path.join(d, names[-1] + ".jpg"), quality=(75, 90)[i // 2 % 2])
    with open(os.path.join(root, "roxford5k", "gnd_roxford5k.pkl"), "wb") as fh:
        pickle.dump({"imlist": names, "qimlist": names[:1], "gnd": [{"easy": [0], "hard": [], "junk": []}]}, fh)


def keep(batch):
    return batch


def summary(rec, name, v):
    rec[name + "_ms"] = round(statistics.median(v), 3)
    rec[name + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--imsize", type=int, nargs="+", default=[224, 512])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--loader_batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thumbnail_bench.jsonl"))
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from sais_amd import imgfolder, retrieval
    from sais_amd.vit import vit_small
    dev = torch.device("cuda:0")
    model = vit_small(patch_size=16, num_classes=0).to(dev).eval()
    fn = retrieval.cls_features(model)
    with tempfile.TemporaryDirectory() as root:
        write_folder(root, args.files)
        raw = imgfolder.RawOxfordParis(root, "roxford5k", "train")
        items, _ = imgfolder.collate_raw([raw[i] for i in range(len(raw))])
        for imsize in args.imsize:
            ref = retrieval.OxfordParisDataset(root, "roxford5k", "train", imsize=imsize)
            loader = imgfolder.GpuImageLoader(dev)
            thumbs = loader.thumbnail(items, imsize)                 # warm-up, sizes the buffers
            for i in range(0, len(items), max(1, len(items) // 16)):
                assert torch.equal(thumbs[i][0].cpu(), ref[i][0]), i
            assert loader.stats["gpu"] == len(items), loader.stats
            be, plan = loader.backend, loader.last_plan
            out = torch.empty(plan.out_elems, dtype=torch.float32, device=dev)
            stream = torch.cuda.current_stream(dev)
            calls = {"thumbnail": lambda: be.launch_thumbnail(plan, out, stream),
                     "loader_call": lambda: loader.thumbnail(items, imsize),
                     "loader_call_again": lambda: loader.thumbnail(items, imsize)}
            for f in calls.values():
                f()
            torch.cuda.synchronize()
            times = {k: [] for k in calls}
            for _ in range(args.rounds):
                for name, f in calls.items():
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                    for _ in range(args.iters):
                        f()
                    ev1.record()
                    torch.cuda.synchronize()
                    times[name].append(ev0.elapsed_time(ev1) / args.iters)
            rec = dict(files=len(items), imsize=imsize, shapes=len({tuple(t.shape) for t in thumbs}), axis_rows=len(loader.row_cache),
                       mean_file_kb=round(sum(len(it[0]) for it in items) / len(items) / 1024, 1), iters=args.iters,
                       rounds=args.rounds, bit_exact=True)
            for name, v in times.items():
                summary(rec, name, v)
            rec["aa_spread_pct"] = round(100.0 * abs(rec["loader_call_ms"] - rec["loader_call_again_ms"]) / rec["loader_call_ms"], 2)
            rec["loader_fps"] = round(len(items) / rec["loader_call_ms"] * 1e3)

            # (a) the Pillow dataset in worker processes: a DataLoader batch is made by one worker
            if args.workers > 0:
                dl = torch.utils.data.DataLoader(ref, batch_size=max(1, len(items) // args.workers), num_workers=args.workers,
                                                 persistent_workers=True, collate_fn=keep)
                for _ in dl:
                    pass
                t0 = time.perf_counter()
                n = sum(len(b) for b in dl)
                rec["pillow_workers"] = args.workers
                rec["pillow_loader_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                rec["pillow_loader_fps"] = round(n / rec["pillow_loader_ms"] * 1e3)
                del dl

            # (b) the extraction loop, three ways
            def pillow_loop():
                return torch.utils.data.DataLoader(ref, batch_size=1, num_workers=args.workers, pin_memory=True)

            def gpu_loop(group):
                return retrieval.ThumbnailBatches(torch.utils.data.DataLoader(
                    raw, batch_size=args.loader_batch, num_workers=args.workers, collate_fn=imgfolder.collate_raw), loader,
                    imsize, group)
            loops = {"extract_pillow": pillow_loop, "extract_gpu_loader": lambda: gpu_loop(False),
                     "extract_gpu_loader_again": lambda: gpu_loop(False), "extract_grouped": lambda: gpu_loop(True)}
            feats, wall = {}, {k: [] for k in loops}
            for r in range(args.rounds + 1):                         # round 0 is the warm-up
                for name, make in loops.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    feats[name] = retrieval.extract_features(fn, make(), dev)
                    torch.cuda.synchronize()
                    if r:
                        wall[name].append((time.perf_counter() - t0) * 1e3)
            for name, v in wall.items():
                summary(rec, name, v)
            rec["extract_aa_spread_pct"] = round(100.0 * abs(rec["extract_gpu_loader_ms"] - rec["extract_gpu_loader_again_ms"])
                                                 / rec["extract_gpu_loader_ms"], 2)
            rec["extract_gpu_equals_pillow"] = bool(torch.equal(feats["extract_pillow"], feats["extract_gpu_loader"]))
            rec["extract_grouped_max_abs_diff"] = float((feats["extract_grouped"] - feats["extract_gpu_loader"]).abs().max())
            line = json.dumps(rec)
            print(line, flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
