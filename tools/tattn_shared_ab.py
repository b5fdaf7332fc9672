#!/usr/bin/env python3
"""A/B of the temporal attention kernels (csrc/tattn.hip, csrc/tattn_long.hip) between two builds of libsais_hip.so on the GPU
(LABNOTES R31.1).  The library is chosen by SAIS_HIP_LIB, which is read once per process: one `dump` per library, then `equal`.
    dump <out.pt>                 every output of the four entry points on the seeded cases of tests/temporal_ref.py (layouts rand,
                                  peaky, planted; masks of mask_patterns): resident S in {1, 17, 33, 96} at B = 3, p = 0 and 0.1, backward
                                  plain and as three gapped slabs; streaming S in {97, 129, 257} at B = 2 and S = 2001 at B = 1, both
                                  forward forms, backward
    equal <a.pt> <b.pt> <json>    torch.equal on every ctx, dqkv and streaming map; the resident map (a float-atomic sum of four head
                                  terms <= 1/4 each) within 6 x 2^-24 absolute, the roundings of its three additions in either order.
                                  Writes {outputs, differ}; exit status 1 if any differs"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

RESIDENT_MAP_BAR = 6 * 2.0 ** -24


def _pad(S, B):
    """the last B patterns of mask_patterns(S) (repeated where S has fewer); at the cap the ragged sequence of long_masks"""
    import temporal_long_ref as LR
    import temporal_ref as R
    if S == LR.LONG_MAX_S:
        return LR.long_masks(S)
    rows = R.masks(S)
    return rows[[max(0, rows.shape[0] - B + i) for i in range(B)]]


def dump(out):
    import torch
    import temporal_ref as R
    from sais_amd import ops
    saved = []
    for S, B, form in [(S, 3, "resident") for S in (1, 17, 33, 96)] + [(97, 2, "long"), (129, 2, "long"), (257, 2, "long"), (2001, 1, "long")]:
        fwd, bwd = (ops.temporal_attn_fwd, ops.temporal_attn_bwd) if form == "resident" else (ops.temporal_attn_fwd_long, ops.temporal_attn_bwd_long)
        pad = _pad(S, B)
        pad8 = pad.to(torch.uint8).cuda()
        for name in R.BWD_LAYOUTS:
            qkv = R.layouts(name, pad, R.case_seed(name, S)).cuda()
            total = torch.randn(B * S, R.DM, generator=torch.Generator().manual_seed(S + 1))
            slabs = R.slab_view(R.split_slabs(total, 3, 8, S + 2)[0].cuda(), B * S)
            for p in (0.0, 0.1):
                st = ops.rng_state(11, "cuda") if p else None
                tag = f"{form} {name} S={S} p={p}"
                for want_map in (False, True):
                    ctx, avg = torch.zeros(B * S, R.DM, device="cuda"), torch.zeros(B, S, S, device="cuda")
                    fwd(qkv, pad8, B, S, ctx, avg if want_map else None, p, st, 3)
                    saved.append((f"{tag} ctx map={want_map}", ctx.cpu()))
                    if want_map:
                        saved.append((f"{tag} map", avg.cpu()))
                for label, dctx in (("plain", total.cuda()), ("3 slabs", slabs)):
                    dqkv = torch.zeros(B * S, 3 * R.DM, device="cuda")
                    bwd(qkv, pad8, B, S, dctx, dqkv, p, st, 3)
                    saved.append((f"{tag} dqkv {label}", dqkv.cpu()))
    torch.cuda.synchronize()
    torch.save(saved, out)
    print(f"{len(saved)} outputs")


def equal(a, b, out):
    import torch
    ta, tb = torch.load(a), torch.load(b)
    differ = [f"only one side has {n}" for n in {n for n, _ in ta} ^ {n for n, _ in tb}]
    for (n, x), (_, y) in zip(ta, tb):
        if n.startswith("resident") and n.endswith(" map"):
            worst = float((x - y).abs().max())
            same = worst <= RESIDENT_MAP_BAR
        else:
            worst, same = float("nan"), torch.equal(x, y)
        if not same:
            differ.append(n)
            print(f"{n}: differs (max |a - b| = {worst:.3g})")
    rec = dict(outputs=len(ta), differ=len(differ), names=differ, resident_map_bar=RESIDENT_MAP_BAR)
    with open(out, "w") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))
    sys.exit(1 if differ or not ta else 0)


if __name__ == "__main__":
    {"dump": dump, "equal": equal}[sys.argv[1]](*sys.argv[2:])
