#!/usr/bin/env python3
"""A/B of the grouped weight-gradient dispatch between two builds of libsais_hip.so on the GPU (LABNOTES R19.1).  The library is
chosen by SAIS_HIP_LIB, the form switches (SAIS_TN_XL, SAIS_TN_XL_SLABS, SAIS_TN_SLABS) by the environment: one process per
(library, switch setting), because both are read once per process.
    rows <out.pt>        every launchable row of the plan table of tests/test_abi.py for the switches in the environment, once, with
                         small-integer operands (every sum exact in fp32 in any order); saves every dW / db.  Under
                         `rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/dw_plan_ab.py rows ...` the same run
                         gives the launch sequence
    blocks <out.pt> [frames] [depth] [groups] [prune]   sais_vit_block_bwd (one dW launch per block) and sais_vit_blocks_dw (one per two blocks) inside a
                         depth-3 ViT at (frames = 64, 197), and sais_temporal_layer_bwd at B = 8, S = 33 with dropout 0.1 and 0:
                         features and every gradient.  Bit-reproducible where the dW launches take a slab form: 256 frames, or 64
                         under SAIS_TN_SLABS=1 (fp32 atomics otherwise: equal up to summation order only).  `256 6 5 1`: five blocks + the
                         pruned block's k / v item are 124 tiles x 2 splits = 248 partial tiles, more than the 240 of a workspace's slab
                         region: the launch sais_vit_blocks_dw makes with fp32 atomics instead
    time                 HIP events, median of 7 turns: the block's dW launch and the 41-item launch at M = 50 432 (one JSON line)
    equal <a.pt> <b.pt> [regex] [tol]   torch.equal on every saved tensor (whose label matches), or relative l2 <= tol; exit status 1 otherwise
    trace <dirA> <dirB>  (kernel name, grid, workgroup size) sequences of two rocprofv3 kernel traces; exit status 1 if they differ"""
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]


def _items(shapes, M, f32, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    dt = torch.float32 if f32 else torch.bfloat16
    ops_in, items = {}, []
    for i, (n1, n2) in enumerate(shapes):
        if (n1, n2) not in ops_in:                                     # repeated blocks share their operands, never their outputs
            ops_in[n1, n2] = (torch.randint(-2, 3, (M, n1), generator=g, device="cuda").to(dt),
                              torch.randint(-3, 4, (M, n2), generator=g, device="cuda").to(dt))
        p, q = ops_in[n1, n2]
        dW = torch.randint(-5, 6, (n1, n2), generator=g, device="cuda").float()
        items.append((p, q, dW, torch.zeros(n1, device="cuda") if i % 2 == 0 else None))
    return items


def rows(out):
    import torch
    from sais_amd import _lib as L, ops
    from tests.test_abi import PLAN_TABLE, NONE
    key = " ".join(f"{k}={os.environ[k]}" for k in ("SAIS_TN_XL", "SAIS_TN_XL_SLABS", "SAIS_TN_SLABS") if k in os.environ)
    saved = []
    for r, ((shapes, M, nsplit, offer, f32), want) in enumerate(PLAN_TABLE[key]):
        if want[0] != 0:
            continue                                                   # rows that are refused: host test only
        items = _items(shapes, M, f32, 100 + r)
        if f32 or offer != NONE:
            ops.gemm_tn_grouped(items, M, nsplit)                      # offers what sais_gemm_tn_grouped_slab_bytes asks for
        else:
            arr = (L.SaisTnItem * len(items))(*[ops._tn_item(*it) for it in items])
            tiles = sum((n1 // 128) * (n2 // 128) for n1, n2 in shapes)
            L.call("sais_gemm_tn_grouped", arr, len(items), M, ops._tn_nsplit(nsplit, M, tiles), ops._stream())
        torch.cuda.synchronize()
        saved += [(f"row {r} item {i} {'dW' if j == 0 else 'db'}", t.cpu()) for i, it in enumerate(items) for j, t in enumerate(it[2:]) if t is not None]
        del items
    torch.save(saved, out)
    print(f"{key or 'default'}: {len(saved)} tensors")


def blocks(out, frames="64", depth="3", groups="1,2", prune="0"):
    import torch
    import synth
    from sais_amd.vit import vit_small
    from sais_amd.temporal import fullModel
    from sais_amd.loss import calcNCELoss
    dev, saved = torch.device("cuda", 0), []
    for G in groups.split(","):
        os.environ["SAIS_DW_GROUP"] = G
        v = vit_small(patch_size=16, drop_path_rate=0.2, depth=int(depth))
        v.load_state_dict(synth.vit_state_dict(seed=0, depth=int(depth)), strict=True)
        v = v.to(dev).train()
        v.block_calls, v.prune_last_block, v.drop_path_seed = True, prune == "1", 9
        x = synth.clips(seed=961, B=1, T=int(frames))[0].to(dev)
        w = synth.reps(seed=962, B=1, T=int(frames))[0, 0].to(dev)
        feat = v(x)
        (feat * w).sum().backward()
        saved += [(f"vit G={G} features", feat.detach().cpu())] + [(f"vit G={G} d {n}", v.flat.g(n).cpu()) for n in v.flat.names]
    B, T = 8, 32
    lens = [32, 20, 32, 7, 32, 32, 15, 32]
    xr, fr = synth.reps(seed=910, B=B, T=T), synth.reps(seed=911, B=B, T=T)
    for b, n in enumerate(lens):
        xr[b, :, n:] = 0
        fr[b, :, n:] = 0
    pad, lab = synth.padding_mask(lens).to(dev), synth.labels(seed=912, B=B)
    for train in (True, False):
        m = fullModel('reps', 2, 'in_vs_out', 384, 'ViT', modalities="RGB-Flow")
        m.load_state_dict(synth.temporal_state_dict(seed=1), strict=True)
        m = m.to(dev)
        m = m.train() if train else m.eval()
        m.dropout_seed = 31
        xg, fg = xr.to(dev).requires_grad_(True), fr.to(dev).requires_grad_(True)
        protos = torch.nn.ParameterDict({k: torch.nn.Parameter(t.clone().to(dev)) for k, t in synth.prototypes(2, 2).items()})
        emb, _ = m(xg, fg, lens, lens, 'Prototypes', pad, pad, None)
        calcNCELoss(0, emb, lab, [f"v{b}" for b in range(B)], protos, None).backward()
        tag = f"temporal p={0.1 if train else 0}"
        saved += [(f"{tag} embedding", emb.detach().cpu()), (f"{tag} d x", xg.grad.cpu()), (f"{tag} d f", fg.grad.cpu())]
        saved += [(f"{tag} d {n}", m.flat.g(n).cpu()) for n in m.flat.names]
    torch.save(saved, out)
    print(f"blocks: {len(saved)} tensors")


def time_launches():
    import torch
    from sais_amd import ops
    from tests.test_abi import BLOCK, KV
    M, res = 50432, {}
    for label, shapes in (("block", BLOCK), ("41 items", BLOCK * 10 + KV)):
        items = _items(shapes, M, False, 7)
        for _ in range(3):
            ops.gemm_tn_grouped(items, M)
        us = []
        for _ in range(7):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            ops.gemm_tn_grouped(items, M)
            e.record()
            torch.cuda.synchronize()
            us.append(1e3 * s.elapsed_time(e))
        res[label] = round(statistics.median(us), 2)
        del items
    print(json.dumps(res))


def equal(a, b, only="", tol="0"):
    import torch
    ta, tb = [[(n, t) for n, t in torch.load(f) if re.search(only, n)] for f in (a, b)]
    diff = abs(len(ta) - len(tb))
    for (n, x), (_, y) in zip(ta, tb):
        rel = 0.0 if torch.equal(x, y) else float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-300))
        if rel > float(tol) or (rel != rel):
            diff += 1
            print(f"{n}: relative l2 difference {rel:.3g}")
    print(f"{len(ta)} tensors{' matching ' + only if only else ''}, {diff} differ")
    sys.exit(1 if diff or not ta else 0)


def _dispatches(d):
    seq = []
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        recs = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        seq += [(r["Kernel_Name"],) + tuple(int(r[k]) for k in sorted(r) if k.startswith(("Grid_Size", "Workgroup_Size"))) for r in recs]
    return [s for s in seq if re.search("gemm_tn|xl_finish|tn_slab_finish", s[0])]    # the dW launches (the rest is torch's fills)


def trace(da, db):
    a, b = _dispatches(da), _dispatches(db)
    diff = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
    print(f"{len(a)} / {len(b)} dW launches, {diff} differ")
    sys.exit(1 if diff or not a else 0)


if __name__ == "__main__":
    {"rows": rows, "blocks": blocks, "time": time_launches, "equal": equal, "trace": trace}[sys.argv[1]](*sys.argv[2:])
