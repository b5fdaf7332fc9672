#!/usr/bin/env python3
"""DINO multi-crop loader on the GPU (sais_amd.jpeg + sais_amd.augment) against the Pillow loader, on a seeded
in-memory corpus.

For each case (1280x720 / 1920x1080, q75 4:2:0) it encodes `--batch` distinct frames, draws 2 global + 8 local views per
frame with a seeded DataAugmentationDINO and reports, per batch:
  * augment alone: both kernels from HIP events, frames and view table resident on the device;
  * decode + augment: wall clock of dino_data.gpu_crops from the file bytes, including the packing of the files, the view
    table and the H2D copies;
  * the Pillow loader (decode + border crop + ten views per frame, as SurgDataset.__getitem__ does in DataLoader
    workers) over `--procs` worker processes on this host: the speed reference.
Every timed GPU batch is compared with the crops of the Pillow loader bit for bit (digests per view).  With --step-ms
(the step time of `bench.py --workload dino` for the same batch) it adds the ratio loader / step.  One JSON line per case."""
import argparse
import hashlib
import io
import json
import multiprocessing as mp
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
FRACS = (0.8, 0.8)


def _pillow_one(job):
    """What a DataLoader worker of the default path does for one frame; optionally a digest per view."""
    from sais_amd.dino_data import apply_view_pillow, border_box
    blob, params, digest = job
    img = Image.open(io.BytesIO(blob))
    img.load()
    left, top, cw, ch = border_box(*img.size, FRACS)
    img = img.crop((left, top, left + cw, top + ch)).convert('RGB')
    views = [apply_view_pillow(img, p) for p in params]
    return [hashlib.sha1(v.numpy().tobytes()).hexdigest() for v in views] if digest else len(views)


def pillow_loader(blobs, params, procs):
    """(frames/s of the Pillow loader over `procs` processes, digests[frame][view]); pool start-up not timed."""
    with ProcessPoolExecutor(procs, mp_context=mp.get_context('spawn')) as ex:
        list(ex.map(_pillow_one, [(blobs[0], params[0], False)] * procs))
        t0 = time.perf_counter()
        list(ex.map(_pillow_one, [(b, p, False) for b, p in zip(blobs, params)]))
        dt = time.perf_counter() - t0
        digests = list(ex.map(_pillow_one, [(b, p, True) for b, p in zip(blobs, params)]))
    return len(blobs) / dt, digests


def digests_of(crops):
    host = [c.cpu().numpy() for c in crops]
    return [[hashlib.sha1(np.ascontiguousarray(h[i]).tobytes()).hexdigest() for h in host] for i in range(host[0].shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--procs', type=int, default=16)
    ap.add_argument('--cases', default='720,1080')
    ap.add_argument('--step-ms', type=float, default=None, help='DINO step time for the same batch (bench.py --workload dino)')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file')
    args = ap.parse_args()
    import torch
    from jpeg_bench import corpus
    from sais_amd.augment import DinoAugmenter
    from sais_amd.dino_data import DataAugmentationDINO, border_box, gpu_crops
    from sais_amd.jpeg import JpegDecoder, parse_header
    dev = torch.device('cuda:0')
    dec, aug = JpegDecoder(dev), DinoAugmenter(dev)
    for case in args.cases.split(','):
        h, w = (720, 1280) if int(case) == 720 else (1080, 1920)
        blobs = corpus(h, w, 75, 2, args.batch)
        t = DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), 8, seed=1)
        params = [t.draw(*border_box(w, h, FRACS)[2:]) for _ in blobs]
        items = [(b, bytes(parse_header(b)), p, 0, 'bench') for b, p in zip(blobs, params)]
        pillow_fps, want = pillow_loader(blobs, params, args.procs)

        for _ in range(args.warmup):
            crops = gpu_crops(items, dec, aug, FRACS)
        assert digests_of(crops) == want, 'GPU crops differ from the Pillow loader'
        first = [c.clone() for c in crops]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            crops = gpu_crops(items, dec, aug, FRACS)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(crops, first))             # = the batch checked against Pillow
        e2e_with_check = (time.perf_counter() - t0) * 1e3 / args.iters
        t0 = time.perf_counter()
        for _ in range(args.iters):
            crops = gpu_crops(items, dec, aug, FRACS)
        torch.cuda.synchronize()
        e2e_ms = (time.perf_counter() - t0) * 1e3 / args.iters
        assert all(torch.equal(a, b) for a, b in zip(crops, first))

        for _ in range(args.warmup):
            aug.relaunch()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(args.iters):
            crops = aug.relaunch()
        ev1.record()
        torch.cuda.synchronize()
        aug_ms = ev0.elapsed_time(ev1) / args.iters
        assert all(torch.equal(a, b) for a, b in zip(crops, first))

        m = len(blobs)
        rec = dict(case=f'{w}x{h} q75 4:2:0', batch=m, views='2x224 + 8x96', mean_file_kb=round(sum(map(len, blobs)) / m / 1024, 1),
                   augment_ms_frames_on_device=round(aug_ms, 3), augment_fps_frames_on_device=round(m / aug_ms * 1e3),
                   decode_augment_ms=round(e2e_ms, 3), decode_augment_fps=round(m / e2e_ms * 1e3),
                   decode_augment_ms_synchronised_and_compared=round(e2e_with_check, 3),
                   pillow_loader_procs=args.procs, pillow_loader_fps=round(pillow_fps, 1),
                   pillow_loader_ms_per_batch=round(m / pillow_fps * 1e3, 1), bit_exact=True,
                   fallbacks=int(dec.stats['failed'] + dec.stats['unsupported']))
        rec['speedup_vs_pillow_loader'] = round(rec['decode_augment_fps'] / pillow_fps, 1)
        if args.step_ms:
            rec['step_ms'] = args.step_ms
            rec['loader_over_step'] = round(e2e_ms / args.step_ms, 3)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
