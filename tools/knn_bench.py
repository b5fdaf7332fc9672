#!/usr/bin/env python3
"""Weighted k-NN evaluation (sais_amd.knn) against the reference formulation in torch on the same GPU.

For each shape (Nt train rows x Nq test rows, D = 384, synthetic L2-normalised features, `--classes` labels) it times with
HIP events, after a warm-up of the same shape: KnnIndex build (the bf16x3 split of the train side), search (kmax = the
largest k) and vote (every k in one pass), and the reference's formulation (eval_knn.py:143-182: per chunk of test rows
`mm` + `topk` + one-hot scatter + weighted sum + `sort`, repeated once per k).  The two paths' top-1 predictions are
compared on the timed inputs.  One JSON line per shape; bf16x3 work is counted as 3 x 2 Nq Nt D operations."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def features(n, d, classes, gen, dev):
    import torch
    labels = torch.randint(0, classes, (n,), generator=gen, device=dev)
    centres = torch.randn(classes, d, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    f = 0.25 * centres[labels] + torch.randn(n, d, generator=gen, device=dev)
    return torch.nn.functional.normalize(f, dim=1, p=2), labels


def torch_formulation(train_t, train_labels, test, k, T, num_classes, chunk):
    """eval_knn.py:143-182 with the test rows in chunks of `chunk`; returns the top-5 predictions [Nq, 5]"""
    import torch
    preds = []
    one_hot = torch.zeros(chunk * k, num_classes, device=test.device)
    for i in range(0, test.shape[0], chunk):
        f = test[i:i + chunk]
        b = f.shape[0]
        distances, indices = torch.mm(f, train_t).topk(k, largest=True, sorted=True)
        neighbors = torch.gather(train_labels.view(1, -1).expand(b, -1), 1, indices)
        oh = one_hot[:b * k].zero_()
        oh.scatter_(1, neighbors.view(-1, 1), 1)
        w = distances.clone().div_(T).exp_()
        probs = torch.sum(torch.mul(oh.view(b, -1, num_classes), w.view(b, -1, 1)), 1)
        preds.append(probs.sort(1, True)[1][:, :5])
    return torch.cat(preds)


def timed(fn, iters):
    import torch
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(iters):
        out = fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / iters, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='65536:8192,65536:50000,1281167:8192,1281167:50000', help='Nt:Nq,...')
    ap.add_argument('--dim', type=int, default=384)
    ap.add_argument('--ks', type=int, nargs='+', default=[10, 20, 100, 200])
    ap.add_argument('--classes', type=int, default=1000)
    ap.add_argument('--temperature', type=float, default=0.07)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--chunk', type=int, default=500, help='test rows per chunk of the torch formulation (50 000 // 100)')
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from sais_amd.knn import KnnIndex
    if not torch.cuda.is_available():
        sys.exit("knn_bench.py measures on the GPU: no device found")
    dev = torch.device('cuda:0')
    ks, T, C = sorted(args.ks), args.temperature, args.classes
    for shape in args.shapes.split(','):
        nt, nq = (int(v) for v in shape.split(':'))
        gen = torch.Generator(device=dev).manual_seed(nt + nq)
        train, train_labels = features(nt, args.dim, C, gen, dev)
        test, _ = features(nq, args.dim, C, gen, dev)
        index = KnnIndex(train, train_labels, C)                       # warm-up of every timed call at this shape
        val, idx = index.search(test, ks[-1])
        index.vote(val, idx, ks, T)
        train_t = train.t()
        for k in ks:
            torch_formulation(train_t, train_labels, test[:2 * args.chunk], k, T, C, args.chunk)
        torch.cuda.synchronize()
        build_ms, index = timed(lambda: KnnIndex(train, train_labels, C), args.iters)
        search_ms, (val, idx) = timed(lambda: index.search(test, ks[-1]), args.iters)
        vote_ms, pred = timed(lambda: index.vote(val, idx, ks, T), args.iters)
        torch_ms, torch_pred = [], []
        for k in ks:
            ms, p = timed(lambda: torch_formulation(train_t, train_labels, test, k, T, C, args.chunk), args.iters)
            torch_ms.append(ms)
            torch_pred.append(p)
        agree = [float((pred[j, :, 0].long() == torch_pred[j][:, 0]).float().mean()) for j in range(len(ks))]
        ops = 3 * 2.0 * nq * nt * args.dim
        native = search_ms + vote_ms
        rec = dict(nt=nt, nq=nq, dim=args.dim, ks=ks, classes=C, iters=args.iters,
                   index_build_ms=round(build_ms, 3), search_ms=round(search_ms, 3), vote_ms=round(vote_ms, 3),
                   search_bf16_tflops=round(ops / search_ms / 1e9, 1),
                   workspace_mb=round(index._ws.numel() / 2 ** 20, 1),
                   torch_ms_per_k=[round(v, 3) for v in torch_ms], torch_total_ms=round(sum(torch_ms), 3),
                   native_total_ms=round(native, 3), speedup_vs_torch=round(sum(torch_ms) / native, 2),
                   top1_agreement_per_k=[round(a, 5) for a in agree])
        print(json.dumps(rec), flush=True)
        del index, train, test, train_t, val, idx


if __name__ == '__main__':
    main()
