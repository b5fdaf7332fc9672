#!/usr/bin/env python3
"""What the linear probe (sais_amd.linear, VisionTransformer.probe_features) costs per training step on the GPU.

Shape: B = 128 frames of 224 x 224, Dm = 1536 (n_last_blocks 4), C = 1000 classes, H in {1, 8} heads.  HIP events; the
series of one comparison are INTERLEAVED round by round (A, A', B, A, A', B, ...) after a warm-up of every timed call, and
the medians over the rounds are reported.
  (a) features: `probe_features(x, 4)` against `model(x)`, which is the forward this tree had before the probe existed (the
      new path adds three CLS-row LayerNorm launches and nothing else).  `model(x)` is timed TWICE per round (A and A'): the
      difference of the two medians is the run-to-run spread.  The three LayerNorm launches are timed on their own.
      Criterion recorded as `within`: probe - parent <= 2 x spread + the three launches.
  (b) heads: one LinearProbe.step (three launches for all H heads) against the torch formulation on the same GPU, H x
      (nn.Linear + CrossEntropyLoss + backward + optim.SGD(momentum 0.9).step) (eval_linear.py:173-183).  No threshold.
One JSON line per comparison, appended to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, iters):
    import torch
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / iters


def interleaved(fns, rounds, iters):
    """{name: median ms per call} with the series taken in turn within every round"""
    for fn in fns.values():
        fn()
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            samples[k].append(timed(fn, iters))
    return {k: statistics.median(v) for k, v in samples.items()}, {k: (min(v), max(v)) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--classes', type=int, default=1000)
    ap.add_argument('--n_last_blocks', type=int, default=4)
    ap.add_argument('--heads', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linear_bench.jsonl'))
    args = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        sys.exit("linear_bench.py measures on the GPU: no device found")
    from sais_amd import ops
    from sais_amd.linear import LinearProbe
    from sais_amd.vit import NTOK, D, vit_small
    dev = torch.device('cuda:0')
    B, C, n = args.batch, args.classes, args.n_last_blocks
    Dm = D * n
    torch.manual_seed(0)
    model = vit_small(patch_size=16, num_classes=0).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, 3, 224, 224, generator=gen, device=dev)
    out = open(args.out, 'a')

    # ---- (a) features
    f = model._engine(dev)
    stream = torch.randn(B * NTOK, D, generator=gen, device=dev)
    feats = torch.empty(B, Dm, device=dev)

    def three_ln():
        for j in range(n - 1):
            ops.layernorm_fwd(stream, B, NTOK * D, f.w32("norm.weight"), f.w32("norm.bias"), 1e-6, y32=feats[:, j * D:], ldy32=Dm)
    with torch.no_grad():
        med, rng = interleaved({"parent_a": lambda: model(x), "parent_b": lambda: model(x),
                                "probe": lambda: model.probe_features(x, n), "cls_ln": three_ln}, args.rounds, args.iters)
        same = torch.equal(model.probe_features(x, n)[:, -D:], model(x))
    parent = 0.5 * (med["parent_a"] + med["parent_b"])
    spread = abs(med["parent_a"] - med["parent_b"])
    extra = med["probe"] - parent
    rec = dict(what="features", batch=B, n_last_blocks=n, rounds=args.rounds, iters=args.iters,
               parent_forward_ms=[round(med["parent_a"], 4), round(med["parent_b"], 4)], aa_spread_ms=round(spread, 4),
               probe_features_ms=round(med["probe"], 4), cls_layernorm_launches_ms=round(med["cls_ln"], 4),
               extra_ms=round(extra, 4), allowed_ms=round(2 * spread + med["cls_ln"], 4),
               within=bool(extra <= 2 * spread + med["cls_ln"]), last_slot_bit_equal_forward=bool(same),
               min_max_ms={k: [round(a, 4), round(b, 4)] for k, (a, b) in rng.items()})
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")

    # ---- (b) heads
    feat = torch.randn(B, Dm, generator=gen, device=dev)
    target = torch.randint(0, C, (B,), generator=gen, device=dev)
    for H in args.heads:
        probe = LinearProbe(Dm, C, [0.01 * (h + 1) for h in range(H)], 100, device=dev, seed=0)
        heads = [torch.nn.Linear(Dm, C).to(dev) for _ in range(H)]
        opts = [torch.optim.SGD(m.parameters(), 0.01 * (h + 1), momentum=0.9, weight_decay=0) for h, m in enumerate(heads)]
        ce = torch.nn.CrossEntropyLoss()

        def torch_step():
            for m, o in zip(heads, opts):
                loss = ce(m(feat), target)
                o.zero_grad()
                loss.backward()
                o.step()
        med, rng = interleaved({"native": lambda: probe.step(feat, target, check_targets=False), "torch": torch_step},
                               args.rounds, 4 * args.iters)
        flops = H * 2 * 2.0 * B * Dm * C
        rec = dict(what="heads", batch=B, dim=Dm, classes=C, heads=H, rounds=args.rounds, iters=4 * args.iters,
                   native_step_ms=round(med["native"], 4), torch_step_ms=round(med["torch"], 4),
                   speedup_vs_torch=round(med["torch"] / med["native"], 2), native_f32_tflops=round(flops / med["native"] / 1e9, 2),
                   share_of_probe_step=round(med["native"] / (med["native"] + parent), 4),
                   min_max_ms={k: [round(a, 4), round(b, 4)] for k, (a, b) in rng.items()})
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
    out.close()


if __name__ == '__main__':
    main()
