#!/usr/bin/env python3
"""GPU JPEG decode (sais_amd.jpeg) against Pillow on a seeded in-memory corpus.

For each case (1280x720 / 1920x1080, q75 / q95, 4:2:0 / 4:4:4) it encodes `--batch` distinct frames with Pillow and
reports, per batch: the sais_jpeg_decode time from HIP events with the compressed bytes already on the device, the time
of JpegDecoder.decode including packing and the H2D copy, decode + preprocess frames/s, and Pillow decode frames/s on
this host with 1 and 16 threads and with 16 worker processes (torch and the GPU stay in the parent).  The timed batch is
checked against Pillow bit for bit.  One JSON line per case."""
import argparse
import io
import json
import multiprocessing as mp
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def corpus(h, w, q, ss, n, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(xx / 37.0 + c) * np.cos(yy / 23.0) for c in range(3)], -1)
    noise = rng.normal(0, 6, (h, w, 3))
    out = []
    for i in range(n):
        a = np.clip(np.roll(base, 5 * i, axis=1) + np.roll(noise, 11 * i, axis=0), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(a).save(b, 'JPEG', quality=q, subsampling=ss)
        out.append(b.getvalue())
    return out


def _decode_one(b):
    return np.asarray(Image.open(io.BytesIO(b))).shape


def pillow_rate_processes(blobs, procs):
    """Pillow decode frames/s over `procs` fresh worker processes (no GIL between decodes; pool start-up not timed)."""
    with ProcessPoolExecutor(procs, mp_context=mp.get_context('spawn')) as ex:
        list(ex.map(_decode_one, blobs[:procs]))
        t0 = time.perf_counter()
        list(ex.map(_decode_one, blobs, chunksize=4))
        return len(blobs) / (time.perf_counter() - t0)


def pillow_rate(blobs, threads, reps=1):
    def one(b):
        return np.asarray(Image.open(io.BytesIO(b)))
    t0 = time.perf_counter()
    for _ in range(reps):
        if threads == 1:
            for b in blobs:
                one(b)
        else:
            with ThreadPoolExecutor(threads) as ex:
                list(ex.map(one, blobs))
    return reps * len(blobs) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--cases', default='720:75:2,720:95:2,720:75:0,720:95:0,1080:75:2,1080:95:2,1080:75:0,1080:95:0')
    ap.add_argument('--pillow-frames', type=int, default=64)
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from sais_amd.jpeg import JpegDecoder, parse_header
    from sais_amd.preprocess import FramePreprocessor
    dev = torch.device('cuda:0')
    dec = JpegDecoder(dev)
    for case in args.cases.split(','):
        hh, q, ss = (int(v) for v in case.split(':'))
        h, w = (720, 1280) if hh == 720 else (1080, 1920)
        blobs = corpus(h, w, q, ss, args.batch)
        hdrs = [parse_header(b) for b in blobs]
        assert all(x is not None for x in hdrs)
        pre = FramePreprocessor(h, w, device=dev)
        out = dec.decode(blobs, hdrs)                              # warm-up, sizes the buffers, exactness check
        for i in range(0, args.batch, max(1, args.batch // 16)):
            assert np.array_equal(out[i].cpu().numpy(), np.asarray(Image.open(io.BytesIO(blobs[i])))), i
        assert dec.last_status.sum() == 0
        # device-only time: replay the launch on the bytes dec.decode() left on the device
        m = len(blobs)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(args.iters):
            dec.relaunch(out)
        ev1.record()
        torch.cuda.synchronize()
        dev_ms = ev0.elapsed_time(ev1) / args.iters
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            dec.decode(blobs, hdrs)
        torch.cuda.synchronize()
        e2e_ms = (time.perf_counter() - t0) * 1e3 / args.iters
        t0 = time.perf_counter()
        for _ in range(args.iters):
            pre(dec.decode(blobs, hdrs))
        torch.cuda.synchronize()
        dp_ms = (time.perf_counter() - t0) * 1e3 / args.iters
        again = dec.decode(blobs, hdrs)
        assert torch.equal(again, out)
        pf = blobs[:args.pillow_frames]
        rec = dict(case=f'{w}x{h} q{q} {"4:2:0" if ss == 2 else "4:4:4"}', batch=m,
                   mean_file_kb=round(sum(map(len, blobs)) / m / 1024, 1),
                   gpu_decode_ms_bytes_on_device=round(dev_ms, 3), gpu_decode_fps_bytes_on_device=round(m / dev_ms * 1e3),
                   decode_incl_pack_h2d_ms=round(e2e_ms, 3), decode_incl_pack_h2d_fps=round(m / e2e_ms * 1e3),
                   decode_preprocess_fps=round(m / dp_ms * 1e3),
                   pillow_fps_1t=round(pillow_rate(pf, 1)), pillow_fps_16t=round(pillow_rate(pf * 4, 16)),
                   pillow_fps_16p=round(pillow_rate_processes(pf * 4, 16)),
                   bit_exact=True, fallbacks=int(dec.stats['failed'] + dec.stats['unsupported']))
        rec['speedup_vs_pillow_16t'] = round(rec['decode_preprocess_fps'] / rec['pillow_fps_16t'], 1)
        rec['speedup_vs_pillow_16p'] = round(rec['decode_preprocess_fps'] / rec['pillow_fps_16p'], 1)
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
