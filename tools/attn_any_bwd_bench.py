#!/usr/bin/env python3
"""Times of the streaming attention backward (csrc/attn_any_bwd.hip) -> profiles/attn_any_bwd_bench.jsonl, one JSON line per record.

Method (HIP events): `--rounds` interleaved rounds (at least 5), every leg once per round with `--iters` back-to-back calls
between two events; the median round is reported, the min / max of the rounds next to it, and per leg its A/A spread: each leg is
timed twice per round under two names that run the same code, |a - b| / min(a, b) of the two medians is what a difference below
it means nothing.
Records:
  64 frames x 197 tokens: sais_vit_attn_bwd_any against the resident sais_vit_attn_bwd on the same qkv, dout, out and lse
  1561 tokens x {1, 6} frames (480 x 832) and 785 x 16: forward + backward of the streaming pair (sais_vit_attn_fwd_any with lse,
      then sais_vit_attn_bwd_any) against F.scaled_dot_product_attention with autograd in bf16 on [frames, 6, ntok, 64] tensors
  one ViT-S/16 forward + backward (12 blocks, DropPath off) at 6 x 480 x 832"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3                       # us per call


def run_legs(legs, rounds, iters):
    """legs: name -> fn; every leg runs as `name` and `name_again` in every round"""
    both = {}
    for k, fn in legs.items():
        both[k], both[k + "_again"] = fn, fn
    for fn in legs.values():                                      # warm-up: code objects, allocator, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in both}
    for _ in range(rounds):
        for k, fn in both.items():
            ts[k].append(timed(fn, iters))
    med = {k: round(statistics.median(v), 2) for k, v in ts.items()}
    return ({k: med[k] for k in legs}, {k: [round(min(ts[k]), 2), round(max(ts[k]), 2)] for k in legs},
            {k: round(abs(med[k] - med[k + "_again"]) / min(med[k], med[k + "_again"]), 4) for k in legs})


def _inputs(frames, ntok):
    g = torch.Generator().manual_seed(ntok)
    qkv = (torch.randn(frames * ntok, 1152, generator=g) * 1.5).to(torch.bfloat16).to(DEV)
    dout = torch.randn(frames * ntok, 384, generator=g).to(torch.bfloat16).to(DEV)
    out = torch.empty(frames * ntok, 384, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(frames, 6, ntok, device=DEV)
    dqkv = torch.empty(frames * ntok, 1152, dtype=torch.bfloat16, device=DEV)
    return qkv, dout, out, lse, dqkv


def resident_record(ops, rounds, iters):
    frames, ntok = 64, 197
    qkv, dout, out, lse, dqkv = _inputs(frames, ntok)
    ops.vit_attn_fwd(qkv, frames, out, lse, None, ntok=ntok)
    legs = {"bwd_any": lambda: ops.vit_attn_bwd_any(qkv, dout, out, lse, frames, ntok, dqkv),
            "bwd_resident": lambda: ops.vit_attn_bwd(qkv, dout, out, lse, None, frames, dqkv, ntok=ntok)}
    med, spread, aa = run_legs(legs, rounds, iters)
    return dict(record="bwd_vs_resident", frames=frames, ntok=ntok, rounds=rounds, iters=iters, us=med, min_max_us=spread,
                aa_spread=aa, any_over_resident=round(med["bwd_any"] / med["bwd_resident"], 3))


def sdpa_record(ops, frames, ntok, rounds, iters):
    qkv, dout, out, lse, dqkv = _inputs(frames, ntok)
    q, k, v = (qkv.view(frames, ntok, 3, 6, 64)[:, :, i].transpose(1, 2).contiguous().requires_grad_(True) for i in range(3))
    w = dout.view(frames, ntok, 6, 64).transpose(1, 2).contiguous()

    def ours():
        ops.vit_attn_fwd_any(qkv, frames, ntok, out, lse)
        ops.vit_attn_bwd_any(qkv, dout, out, lse, frames, ntok, dqkv)

    def sdpa():
        q.grad = k.grad = v.grad = None
        F.scaled_dot_product_attention(q, k, v).backward(w)
    med, spread, aa = run_legs({"stream_fwd_bwd": ours, "sdpa_fwd_bwd": sdpa,
                                "stream_bwd": lambda: ops.vit_attn_bwd_any(qkv, dout, out, lse, frames, ntok, dqkv)}, rounds, iters)
    return dict(record="fwd_bwd_vs_sdpa", frames=frames, ntok=ntok, rounds=rounds, iters=iters, us=med, min_max_us=spread,
                aa_spread=aa, sdpa_over_stream=round(med["sdpa_fwd_bwd"] / med["stream_fwd_bwd"], 3))


def vit_record(rounds):
    from sais_amd import vit
    torch.manual_seed(0)
    model = vit.vit_small(patch_size=16).to(DEV).train()
    x = torch.randn(6, 3, 480, 832, device=DEV)

    def step():
        model.zero_grad()
        model(x).sum().backward()
    med, spread, aa = run_legs({"vit_fwd_bwd": step}, rounds, 3)
    return dict(record="vit_fwd_bwd", frames=6, H=480, W=832, ntok=1561, depth=12, rounds=rounds,
                ms=round(med["vit_fwd_bwd"] / 1e3, 3), min_max_ms=[round(t / 1e3, 3) for t in spread["vit_fwd_bwd"]],
                aa_spread=aa["vit_fwd_bwd"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_any_bwd_bench.jsonl"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds: at least 5 interleaved rounds")
    from sais_amd import ops
    recs = [resident_record(ops, args.rounds, args.iters)]
    recs += [sdpa_record(ops, f, n, args.rounds, args.iters) for f, n in ((1, 1561), (6, 1561), (16, 785))]
    recs.append(vit_record(args.rounds))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in recs:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
