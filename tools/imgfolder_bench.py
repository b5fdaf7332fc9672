#!/usr/bin/env python3
"""Image-folder batches on the GPU (sais_amd.imgfolder) against the Pillow loader, on a synthetic folder the tool writes.

The folder: --batch JPEG files of the sizes an image folder mixes (500x375, 375x500, 500x333, 640x480, 1024x768 and a few
2048x1536), quality 75 and 90, 4:2:0 and 4:4:4, all in one class folder.  Timed with HIP events around each call, after a
warm-up of every call, in --rounds interleaved rounds of --iters calls each; the median round is reported with the spread
(min / max over rounds), and `loader_call` is measured twice per round (A/A) so that the spread of identical work is visible:
  mixed_decode     sais_jpeg_decode_mixed alone, compressed bytes already on the device
  transform        sais_image_transform alone (the eval transform), decoded images already on the device
  loader_call      GpuImageLoader.eval(items): plan, pinned pack, H2D, decode, status read, transform
  grouped_call     the same batch through the per-geometry grouping of dino_data.gpu_crops: one JpegDecoder.decode (one status
                   read) and one transform launch per (H, W)
  model            model(x) on the batch
and, with the wall clock, EvalImageFolder through a DataLoader of 16 worker processes on this host (second pass over the
folder, the workers already running, one sixteenth of the batch per worker).  The loader's batch is checked against
EvalImageFolder bit for bit.  One JSON line, appended to --out (default profiles/imgfolder_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(500, 375), (375, 500), (500, 333), (640, 480), (1024, 768)]
LARGE = (2048, 1536)


def write_folder(root, n, large=4, seed=0):
    rng = np.random.default_rng(seed)
    d = os.path.join(root, "c0")
    os.makedirs(d, exist_ok=True)
    for i in range(n):
        w, h = LARGE if i % (n // large) == n // large - 1 else SIZES[i % len(SIZES)]
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([128 + 90 * np.sin(xx / (29.0 + i % 7) + c) * np.cos(yy / (17.0 + i % 5)) for c in range(3)], -1)
        a = np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(d, "img%04d.jpg" % i), quality=(75, 90)[i // 2 % 2], subsampling=(2, 0)[i % 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imgfolder_bench.jsonl"))
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from sais_amd import _lib as L, imgfolder, jpeg
    from sais_amd.knn import EvalImageFolder
    from sais_amd.vit import vit_small
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as root:
        write_folder(root, args.batch)
        ref = EvalImageFolder(root)
        raw = imgfolder.RawEvalFolder(root)
        items, _ = imgfolder.collate_raw([raw[i] for i in range(len(raw))])
        loader = imgfolder.GpuImageLoader(dev)
        x = loader.eval(items)                                       # warm-up, sizes the buffers
        for i in range(0, len(items), max(1, len(items) // 16)):
            assert torch.equal(x[i].cpu(), ref[i][0]), i
        assert loader.stats["gpu"] == len(items), loader.stats
        be = loader.backend
        out = torch.empty_like(x)

        # the per-geometry grouping of gpu_crops, with this tool's transform
        headers = [jpeg.SaisJpegHeader.from_buffer_copy(it[1]) for it in items]
        groups = {}
        for i, h in enumerate(headers):
            groups.setdefault((h.height, h.width), []).append(i)
        dec = jpeg.JpegDecoder(dev)
        lut = torch.from_numpy(imgfolder.normalize_table()).to(dev)
        build = imgfolder.eval_builder()

        def grouped():
            stream = torch.cuda.current_stream(dev)
            for (h, w), idx in groups.items():
                frames = dec.decode([items[i][0] for i in idx], [headers[i] for i in idx])
                rows = [imgfolder.descriptor(build(None, w, h), w, h, (224, 224), k * 3 * h * w, i * 3 * 224 * 224)
                        for k, i in enumerate(idx)]
                table = np.array(rows, dtype=imgfolder.XFORM_DTYPE)
                table_d = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
                L.call("sais_image_transform", frames.data_ptr(), frames.numel(), table.ctypes.data, table_d.data_ptr(),
                       len(idx), 224, 224, lut.data_ptr(), out.data_ptr(), out.numel(), stream.cuda_stream)
            return out

        assert torch.equal(grouped(), x)
        model = vit_small(patch_size=16, num_classes=0).to(dev).eval()
        stream = torch.cuda.current_stream(dev)
        calls = {
            "mixed_decode": lambda: be.launch_decode(stream),
            "transform": lambda: be.launch_transform(out, stream),
            "loader_call": lambda: loader.eval(items),
            "loader_call_again": lambda: loader.eval(items),
            "grouped_call": grouped,
            "model": lambda: model(x),
        }
        loader.eval(items)                                           # the replayed launches refer to this batch
        with torch.no_grad():
            for fn in calls.values():
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in calls}
            for _ in range(args.rounds):
                for name, fn in calls.items():
                    if name in ("mixed_decode", "transform"):
                        loader.eval(items)                           # (untimed) the device buffers hold this batch again
                        torch.cuda.synchronize()
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                    for _ in range(args.iters):
                        fn()
                    ev1.record()
                    torch.cuda.synchronize()
                    times[name].append(ev0.elapsed_time(ev1) / args.iters)
        assert torch.equal(loader.eval(items), x)

        # a DataLoader batch is made by one worker: batches of batch / workers images keep every worker busy
        pillow_ms = None
        if args.workers > 0:                                         # --workers 0: no Pillow leg (under a profiler)
            dl = torch.utils.data.DataLoader(ref, batch_size=max(1, args.batch // args.workers), num_workers=args.workers,
                                             persistent_workers=True)
            for _ in dl:
                pass
            t0 = time.perf_counter()
            n = sum(b[0].shape[0] for b in dl)
            pillow_ms = (time.perf_counter() - t0) * 1e3
            del dl

    B = len(items)
    rec = dict(batch=B, geometries=len(groups), mean_file_kb=round(sum(len(it[0]) for it in items) / B / 1024, 1),
               iters=args.iters, rounds=args.rounds, bit_exact=True)
    for name, v in times.items():
        rec[name + "_ms"] = round(statistics.median(v), 3)
        rec[name + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
    rec["aa_spread_pct"] = round(100.0 * abs(rec["loader_call_ms"] - rec["loader_call_again_ms"]) / rec["loader_call_ms"], 2)
    rec["loader_fps"] = round(B / rec["loader_call_ms"] * 1e3)
    rec["grouped_fps"] = round(B / rec["grouped_call_ms"] * 1e3)
    rec["model_fps"] = round(B / rec["model_ms"] * 1e3)
    if pillow_ms is not None:
        rec["pillow_workers"] = args.workers
        rec["pillow_loader_ms"] = round(pillow_ms, 1)
        rec["pillow_loader_fps"] = round(n / pillow_ms * 1e3)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
