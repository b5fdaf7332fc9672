#!/usr/bin/env python3
"""Golden vectors of the temporal encoder past 96 tokens, from the reference's own fullModel on the CPU -> temporal_long.npz.

Runs only where the reference checkout is (make_golden.py: import_reference, build_full); the GPU box sees the .npz alone.
fullModel('reps', 2, 'in_vs_out', 384, 'ViT', self_attention=True) under synth.temporal_state_dict(seed=1), eval():
  RGB-Flow  lens [130, 97]   ragged in one batch
  RGB       lens [96]        S = 97, the first length past the resident kernels
  Flow      lens [100]
  RGB-Flow  lens [2000]      the position table's last row; the map rows MAP_ROWS only (the whole map is 16 MB)
  TTA list  T = (130, 127, 124), B = 2 (prepare_model.py:331-346); the map is version 0's
Inputs: synth.reps(seed = 100 + T / 200 + T) zero-padded past each length, as make_golden.golden_temporal builds them; the TTA
versions synth.reps(seed = 300 + v / 400 + v)."""
import os

import numpy as np
import torch

import make_golden as MG
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = (("RGB-Flow", "r130_97", [130, 97]), ("RGB", "r96", [96]), ("Flow", "r100", [100]), ("RGB-Flow", "r2000", [2000]))
MAP_ROWS = [0, 1, 1000, 2000]


def main():
    _, prepare_model, _ = MG.import_reference()
    g = {}
    models = {}
    for modal, cname, lens in CASES:
        m = models.setdefault(modal, MG.build_full(prepare_model, 2, modal))
        B, T = len(lens), max(lens)
        x, f = synth.reps(seed=100 + T, B=B, T=T), synth.reps(seed=200 + T, B=B, T=T)
        for b, n in enumerate(lens):
            x[b, :, n:] = 0
            f[b, :, n:] = 0
        pad = synth.padding_mask(lens)
        with torch.no_grad():
            emb, attn = m(x.clone(), f.clone(), lens, lens, 'Prototypes', pad.clone(), pad.clone(), None)
        key = f"{modal}/{cname}/"
        g[key + "lens"] = np.array(lens)
        g[key + "emb"] = emb.numpy()
        g[key + "attn"] = (attn[:, MAP_ROWS] if T == 2000 else attn).numpy()
    m = models["RGB-Flow"]
    xs, fs, pads, lens_l = [], [], [], []
    for v, T in enumerate((130, 127, 124)):
        xs.append(synth.reps(seed=300 + v, B=2, T=T))
        fs.append(synth.reps(seed=400 + v, B=2, T=T))
        pads.append(synth.padding_mask([T, T]))
        lens_l.append([T, T])
    with torch.no_grad():
        embs, attn = m([t.clone() for t in xs], [t.clone() for t in fs], lens_l, lens_l, 'Prototypes', [p.clone() for p in pads],
                       [p.clone() for p in pads], None)
    for v in range(3):
        g[f"TTA/emb{v}"] = embs[v].numpy()
    g["TTA/attn"] = attn.numpy()
    np.savez_compressed(os.path.join(HERE, "temporal_long.npz"), **g)
    print("temporal_long.npz keys", len(g), "bytes", os.path.getsize(os.path.join(HERE, "temporal_long.npz")))


if __name__ == "__main__":
    main()
