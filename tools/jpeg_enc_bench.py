#!/usr/bin/env python3
"""GPU JPEG encode (sais_amd.jpeg_enc) against Pillow's encoder on the images the project writes.

Shapes: 16 and 64 rendered 480 x 848 inferno heat maps (attnviz.render on seeded attention), 256 colour-coded flow maps of
224 x 224 (raft.flow_to_rgb on seeded smooth flow fields), 64 frames of 1280 x 720 decoded from tools/jpeg_bench.py's corpus.
Per shape, `--rounds` interleaved rounds of: JpegEncoder.encode_to_device alone (HIP events around `--iters` calls), the same
again (the A/A pair: its spread is the noise floor of the figures), JpegEncoder.encode including its two device-to-host copies
(host clock; the call ends synchronised), Pillow's Image.save into memory over 16 threads, and over 16 worker processes (pool
start-up not timed; torch and the GPU stay in the parent).  Medians over the rounds.  The timed batch is checked against Pillow
byte for byte.  `--video N` adds one video_generation run over N synthetic 480 x 848 frames and times its write step per frame,
for the batch writer (attnviz.save_jpegs) and for the per-frame loop it replaced (rgb.cpu().numpy() + attnviz.save_jpeg per frame,
restated here), each after a device synchronise.  One JSON line per record, appended to --out."""
import argparse
import importlib.util
import io
import json
import multiprocessing as mp
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DPI = (100, 100)


def _save_one(job):
    a, dpi = job
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="jpeg", **({"dpi": dpi} if dpi else {}))
    return buf.getvalue()


def pillow_threads_ms(jobs, threads=16):
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(_save_one, jobs))
        return (time.perf_counter() - t0) * 1e3


def heat_maps(frames, dev, seed=0):
    import torch
    from sais_amd import attnviz
    g = torch.Generator().manual_seed(seed)
    probs = torch.softmax(3 * torch.randn(frames, 6, 1 + 30 * 53, generator=g), dim=2)
    return attnviz.render(probs.to(dev), (30, 53), threshold=0.6, cmap="inferno", patch=16)[1]


def flow_maps(n, dev, seed=1):
    import torch
    from sais_amd.raft import flow_image_uint8_device, flow_to_rgb
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(n, 2, 8, 8, generator=g) * 6
    flow = torch.nn.functional.interpolate(coarse, size=(224, 224), mode="bicubic", align_corners=False).to(dev)
    return torch.stack([flow_image_uint8_device(flow_to_rgb(f)) for f in flow])


def decoded_frames(n, dev):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import jpeg_bench
    from sais_amd.jpeg import JpegDecoder
    return JpegDecoder(dev).decode(jpeg_bench.corpus(720, 1280, 75, 2, n))


def bench_shape(name, rgb, dpi, enc, args, pool):
    import torch
    n, H, W = tuple(rgb.shape[:3])
    host = rgb.cpu().numpy()
    jobs = [(host[i], dpi) for i in range(n)]
    files = enc.encode(rgb, dpi=dpi)                                     # warm-up, sizes the buffers, exactness check
    want = [_save_one(j) for j in jobs]
    assert files == want, name
    list(pool.map(_save_one, jobs[:16]))                                 # every worker has imported Pillow
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def device_ms():
        ev[0].record()
        for _ in range(args.iters):
            enc.encode_to_device(rgb)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / args.iters

    rows = {k: [] for k in ("dev_a", "dev_b", "e2e", "threads", "procs")}
    for _ in range(args.rounds):
        rows["dev_a"].append(device_ms())
        t0 = time.perf_counter()
        enc.encode(rgb, dpi=dpi)
        rows["e2e"].append((time.perf_counter() - t0) * 1e3)
        rows["threads"].append(pillow_threads_ms(jobs))
        t0 = time.perf_counter()
        list(pool.map(_save_one, jobs, chunksize=max(1, n // 64)))
        rows["procs"].append((time.perf_counter() - t0) * 1e3)
        rows["dev_b"].append(device_ms())
    med = {k: statistics.median(v) for k, v in rows.items()}
    return dict(shape=name, frames=n, height=H, width=W, dpi=bool(dpi), rounds=args.rounds, iters=args.iters,
                mean_file_kb=round(sum(map(len, files)) / n / 1024, 1),
                encode_to_device_ms=round(med["dev_a"], 4), encode_to_device_ms_again=round(med["dev_b"], 4),
                aa_spread_pct=round(abs(med["dev_a"] - med["dev_b"]) / med["dev_a"] * 100, 2),
                encode_to_device_ms_min_max=[round(min(rows["dev_a"] + rows["dev_b"]), 4), round(max(rows["dev_a"] + rows["dev_b"]), 4)],
                encode_incl_copies_ms=round(med["e2e"], 3), pillow_16_threads_ms=round(med["threads"], 3),
                pillow_16_processes_ms=round(med["procs"], 3),
                per_frame_us=dict(encode_to_device=round(med["dev_a"] / n * 1e3, 2), encode_incl_copies=round(med["e2e"] / n * 1e3, 2),
                                  pillow_16_threads=round(med["threads"] / n * 1e3, 2), pillow_16_processes=round(med["procs"] / n * 1e3, 2)),
                byte_exact=True)


def bench_video(frames, args):
    """video_generation over `frames` synthetic 480 x 848 frames, twice: the write step per frame with the batch writer and with
    the per-frame Pillow loop; the files of the two runs are compared."""
    import torch
    from sais_amd import attnviz
    spec = importlib.util.spec_from_file_location("vg_bench", os.path.join(ROOT, "SAIS", "scripts", "dino-main", "video_generation.py"))
    vg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vg)
    batch_writer = attnviz.save_jpegs
    spent = []

    def timed(fn):
        def run(fnames, rgb):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(fnames, rgb)
            spent.append(time.perf_counter() - t0)
        return run

    def per_frame_loop(fnames, rgb):
        rgb = rgb.cpu().numpy()
        for j, fname in enumerate(fnames):
            attnviz.save_jpeg(fname, rgb[j])

    rec = dict(shape="video_generation write step", frames=frames, height=480, width=848, bs=8)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "in"))
        rng = np.random.Generator(np.random.PCG64(7))
        yy, xx = np.mgrid[:480, :848]
        for t in range(frames):
            base = (np.stack([xx * 0.6 + 9 * t, yy * 0.9, (xx + yy) * 0.4], -1) % 256).astype(np.float32)
            Image.fromarray(np.clip(base + 8 * rng.standard_normal(base.shape), 0, 255).astype(np.uint8)).save(
                os.path.join(tmp, "in", f"frame-{t:04d}.jpg"), quality=92)
        outs = {}
        for key, fn in (("warm_up", batch_writer), ("save_jpegs", batch_writer), ("save_jpeg_loop", per_frame_loop),
                        ("save_jpegs_again", batch_writer)):
            spent.clear()
            attnviz.save_jpegs = timed(fn)
            try:
                vg.main(["--input_path", os.path.join(tmp, "in"), "--output_path", os.path.join(tmp, key)])
            finally:
                attnviz.save_jpegs = batch_writer
            folder = os.path.join(tmp, key, "attention")
            outs[key] = [open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))]
            if key != "warm_up":
                rec[key + "_ms_per_frame"] = round(sum(spent) / frames * 1e3, 4)
        rec["files_identical"] = outs["save_jpegs"] == outs["save_jpeg_loop"] == outs["save_jpegs_again"] and len(outs["save_jpegs"]) == frames
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="heat16,heat64,flow256,frames64")
    ap.add_argument("--video", type=int, default=64, help="frames of the video_generation run (0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_enc_bench.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_enc_bench needs the GPU: nothing is timed without one")
    from sais_amd.jpeg_enc import JpegEncoder
    dev = torch.device("cuda:0")
    enc = JpegEncoder(dev)
    make = {"heat16": lambda: (heat_maps(16, dev), DPI), "heat64": lambda: (heat_maps(64, dev), DPI),
            "flow256": lambda: (flow_maps(256, dev), None), "frames64": lambda: (decoded_frames(64, dev), None)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh, ProcessPoolExecutor(16, mp_context=mp.get_context("spawn")) as pool:
        for name in [s for s in args.shapes.split(",") if s]:
            rgb, dpi = make[name]()
            rec = bench_shape(name, rgb.contiguous(), dpi, enc, args, pool)
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            fh.flush()
        if args.video:
            rec = bench_video(args.video, args)
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
