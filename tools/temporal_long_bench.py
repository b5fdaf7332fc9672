#!/usr/bin/env python3
"""Times of the streaming temporal attention (csrc/tattn_long.hip) -> profiles/temporal_long_bench.jsonl, one JSON line per shape.

Method (HIP events): `--rounds` interleaved rounds, every leg once per round with `--iters` back-to-back calls between two
events; the median round is reported and the A/A spread next to it (the long forward without map is timed as two legs that run
the same code: |a - b| / min(a, b) of their medians is what a difference below it means nothing).
Legs per shape (B, S): forward without map, forward with map, backward (dctx plain), of
  long      sais_temporal_attn_fwd_long / _bwd_long
  resident  sais_temporal_attn_fwd / _bwd, at S <= 96 only: the number that says where the switch sits
  torch     F.multi_head_attention_forward(need_weights=True) in fp32 with identity projections and autograd (forward + map;
            backward = autograd of a sum against fixed weights, the forward's time subtracted is NOT done: the leg is fwd + bwd)
Shapes: S in {96, 97, 256, 512, 1024, 2001}; B = 8 up to 512, then 2 and 1.
Last line: one whole fullModel train step (forward + NCE loss + backward + sgd_step) at B = 2, T = 1000, RGB-Flow."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"
SHAPES = ((8, 96), (8, 97), (8, 256), (8, 512), (2, 1024), (1, 2001))


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3                       # us per call


def run_legs(legs, rounds, iters):
    for fn in legs.values():                                      # warm-up: code objects, LDS attributes, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ts[k].append(timed(fn, iters))
    return {k: round(statistics.median(v), 2) for k, v in ts.items()}, {k: [round(min(v), 2), round(max(v), 2)] for k, v in ts.items()}


def shape_record(ops, B, S, rounds, iters):
    g = torch.Generator().manual_seed(S)
    qkv = torch.randn(B * S, 1152, generator=g).to(DEV)
    pad = torch.zeros(B, S, dtype=torch.uint8, device=DEV)
    dctx = torch.randn(B * S, 384, generator=g).to(DEV)
    ctx, avg, dqkv = (torch.empty(*s, device=DEV) for s in ((B * S, 384), (B, S, S), (B * S, 1152)))
    ws = torch.empty(ops.temporal_attn_long_bwd_workspace_bytes(B, S), dtype=torch.uint8, device=DEV)
    legs = {
        "long_fwd": lambda: ops.temporal_attn_fwd_long(qkv, pad, B, S, ctx, None),
        "long_fwd_again": lambda: ops.temporal_attn_fwd_long(qkv, pad, B, S, ctx, None),
        "long_fwd_map": lambda: ops.temporal_attn_fwd_long(qkv, pad, B, S, ctx, avg),
        "long_bwd": lambda: ops.temporal_attn_bwd_long(qkv, pad, B, S, dctx, dqkv, ws=ws),
    }
    if S <= 96:
        legs.update({
            "resident_fwd": lambda: ops.temporal_attn_fwd(qkv, pad, B, S, ctx, None),
            "resident_fwd_map": lambda: ops.temporal_attn_fwd(qkv, pad, B, S, ctx, avg),
            "resident_bwd": lambda: ops.temporal_attn_bwd(qkv, pad, B, S, dctx, dqkv),
        })
    # torch: [S, B, 384] inputs, identity in / out projections so that the work is the attention core
    q, k, v = (qkv.view(B, S, 3, 384)[:, :, i].transpose(0, 1).contiguous().requires_grad_(True) for i in range(3))
    eye, zero = torch.eye(384, device=DEV), torch.zeros(384, device=DEV)
    w = dctx.view(B, S, 384).transpose(0, 1).contiguous()

    def torch_fwd():
        return F.multi_head_attention_forward(q, k, v, 384, 4, None, None, None, None, False, 0.0, eye, zero, training=False,
                                              key_padding_mask=pad.bool(), need_weights=True, use_separate_proj_weight=True,
                                              q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye)

    def torch_fwd_bwd():
        out, _ = torch_fwd()
        q.grad = k.grad = v.grad = None
        (out * w).sum().backward()

    def torch_fwd_nograd():
        with torch.no_grad():
            torch_fwd()
    legs.update({"torch_fwd_map": torch_fwd_nograd, "torch_fwd_bwd": torch_fwd_bwd})
    med, spread = run_legs(legs, rounds, iters)
    aa = abs(med["long_fwd"] - med["long_fwd_again"]) / min(med["long_fwd"], med["long_fwd_again"])
    rec = dict(B=B, S=S, rounds=rounds, iters=iters, us=med, min_max_us=spread, aa_spread=round(aa, 4),
               torch_fwd_map_over_long=round(med["torch_fwd_map"] / med["long_fwd_map"], 3),
               torch_fwd_bwd_over_long=round(med["torch_fwd_bwd"] / (med["long_fwd_map"] + med["long_bwd"]), 3))
    if S <= 96:
        rec.update(long_over_resident={k: round(med["long_" + k] / med["resident_" + k], 3) for k in ("fwd", "fwd_map", "bwd")})
    return rec


def train_step_record(rounds):
    import synth
    from sais_amd.loss import calcNCELoss
    from sais_amd.optim import SGD
    from sais_amd.temporal import fullModel
    B, T = 2, 1000
    m = fullModel('reps', 2, 'in_vs_out', 384, 'ViT', modalities="RGB-Flow")
    m.load_state_dict(synth.temporal_state_dict(seed=1), strict=True)
    m = m.to(DEV).train()
    x, f = synth.reps(seed=1, B=B, T=T).to(DEV), synth.reps(seed=2, B=B, T=T).to(DEV)
    pad = synth.padding_mask([T, T]).to(DEV)
    protos = torch.nn.ParameterDict({k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in synth.prototypes(2, 2).items()})
    lab = synth.labels(seed=3, B=B)
    opt = SGD(list(m.parameters()) + list(protos.values()), lr=1e-3, engines=[m])

    def step():
        opt.zero_grad()
        emb, _ = m(x, f, [T, T], [T, T], 'Prototypes', pad, pad, None)
        calcNCELoss(0, emb, lab, ["v0", "v1"], protos, None).backward()
        opt.step()
    med, spread = run_legs({"step": step, "step_again": step}, rounds, 3)
    return dict(train_step=dict(B=B, T=T, modalities="RGB-Flow"), ms=round(med["step"] / 1e3, 3),
                min_max_ms=[round(v / 1e3, 3) for v in spread["step"]],
                aa_spread=round(abs(med["step"] - med["step_again"]) / min(med.values()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_long_bench.jsonl"))
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from sais_amd import ops
    recs = [shape_record(ops, B, S, args.rounds, args.iters) for B, S in SHAPES]
    if not args.no_step:
        recs.append(train_step_record(args.rounds))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in recs:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
