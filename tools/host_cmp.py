#!/usr/bin/env python3
"""Do two builds of libsais_hip.so answer the same on the host?  No GPU needed: the slab-workspace sizing rule of the grouped
weight-gradient launch under its environment switches, the block workspace sizes, and the return codes of the sais_gemm_* entries for bad arguments
(the calls of tests/test_abi.py).  Every (library, environment) pair runs in a child process of its own, because the
switches are read once per process.
    tools/host_cmp.py <libA.so> <libB.so>      exit status 1 on any difference"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = ((384, 1536), (1536, 384), (384, 384), (1152, 384))
KV = ((768, 384),)
# the edges of every regime of the grouped dW launch: 192 x 384 tiles (N1 % 192, N2 % 384, M % 32, >= 48 steps per split, one or
# several splits), 128 x 384 tiles (M % 64, M >= 8192), 128 x 128 tiles; more items than SAIS_TN_MAX_ITEMS
ITEM_SETS = {"vit block": BLOCK, "two items": ((384, 384), (1152, 384)), "N2 % 384 != 0": ((384, 1536), (1536, 512)),
             "k/v only": KV, "6 blocks + k/v": BLOCK * 6 + KV, "10 blocks + k/v": BLOCK * 10 + KV, "49 items": ((384, 384),) * 49,
             "fc1 + fc2": BLOCK[:2], "N1 % 192 != 0": ((128, 384),)}
MS = (300, 3152, 8192, 12608, 12640, 50432, 100864)
WS_SHAPES = ((64, 197), (256, 197), (16, 37), (8, 16), (204, 16))          # (frames, ntok) for sais_workspace_bytes, all four ops
ENVS = ({}, {"SAIS_TN_XL": "0"}, {"SAIS_TN_XL": "8"}, {"SAIS_TN_XL_SLABS": "0"}, {"SAIS_TN_SLABS": "1"})


def child():
    sys.path.insert(0, ROOT)
    from sais_amd import _lib
    lib = ctypes.CDLL(os.environ["SAIS_HIP_LIB"])
    for name, args in _lib.SIGNATURES.items():
        if name.startswith(("sais_gemm_", "sais_splitk")):
            getattr(lib, name).argtypes = args
    lib.sais_gemm_tn_grouped_slab_bytes.restype = ctypes.c_size_t
    out = {}
    for label, shapes in ITEM_SETS.items():
        items = (_lib.SaisTnItem * len(shapes))()
        for it, (n1, n2) in zip(items, shapes):
            it.N1, it.N2 = n1, n2
        for M in MS:
            out[f"slab_bytes {label} M={M}"] = lib.sais_gemm_tn_grouped_slab_bytes(items, len(shapes), M)
    lib.sais_workspace_bytes.restype = ctypes.c_size_t
    for frames, ntok in WS_SHAPES:
        for op in range(4):
            out[f"workspace_bytes op={op} ({frames}, {ntok})"] = lib.sais_workspace_bytes(op, frames, ntok)
    items = (_lib.SaisTnItem * 4)()
    out["slab_bytes NULL items"] = lib.sais_gemm_tn_grouped_slab_bytes(None, 4, 50432)
    out["slab_bytes 0 items"] = lib.sais_gemm_tn_grouped_slab_bytes(items, 0, 50432)
    g = _lib.SaisGemm()
    out["gemm_nt(NULL)"] = lib.sais_gemm_nt(None, None)
    out["gemm_nt(zeroed)"] = lib.sais_gemm_nt(ctypes.byref(g), None)
    out["gemm_nt_f32(NULL)"] = lib.sais_gemm_nt_f32(None, None)
    out["gemm_nt_f32(zeroed)"] = lib.sais_gemm_nt_f32(ctypes.byref(g), None)
    g.A = g.B = g.out = 16
    g.M, g.N, g.K, g.lda, g.ldb, g.ldo = 256, 384, 384, 384, 384, 384
    for epi, what in ((99, "unknown epilogue"), (_lib.EPI_BIAS_GELU_GRAD_BF16, "GELU' without out2"), (_lib.EPI_MUL_BF16, "MUL without aux")):
        g.epilogue = epi
        out[f"gemm_nt({what})"] = lib.sais_gemm_nt(ctypes.byref(g), None)
    g.epilogue, g.N = _lib.EPI_BIAS_BF16, 100
    out["gemm_nt(N % 128)"] = lib.sais_gemm_nt(ctypes.byref(g), None)
    out["gemm_nt_f32(N % 128)"] = lib.sais_gemm_nt_f32(ctypes.byref(g), None)
    out["gemm_ln_fwd(NULL)"] = lib.sais_gemm_ln_fwd(None, None)
    out["gemm_ln_bwd(zeroed)"] = lib.sais_gemm_ln_bwd(ctypes.byref(_lib.SaisGemmLn()), None)
    out["gemm_tn(NULL)"] = lib.sais_gemm_tn(None, 384, None, 384, 256, 384, 384, None, 384, None, 4, None)
    out["gemm_tn_f32(NULL)"] = lib.sais_gemm_tn_f32(None, 384, None, 384, 256, 384, 384, None, 384, None, 4, None)
    out["gemm_tn(N1 % 128)"] = lib.sais_gemm_tn(16, 384, 16, 384, 256, 100, 384, 16, 384, None, 4, None)
    out["gemm_tn(nsplit 0)"] = lib.sais_gemm_tn(16, 384, 16, 384, 256, 384, 384, 16, 384, None, 0, None)
    out["gemm_tn_grouped(NULL)"] = lib.sais_gemm_tn_grouped(None, 4, 50432, 7, None)
    out["gemm_tn_grouped(NULL P)"] = lib.sais_gemm_tn_grouped(items, 4, 50432, 7, None)
    out["gemm_tn_grouped(5 items)"] = lib.sais_gemm_tn_grouped(items, 5, 50432, 7, None)
    out["gemm_tn_grouped_ws(NULL)"] = lib.sais_gemm_tn_grouped_ws(None, 4, 50432, 7, None, 0, None)
    out["gemm_tn_grouped_ws(M 0)"] = lib.sais_gemm_tn_grouped_ws(items, 4, 0, 7, None, 0, None)
    out["gemm_tn_grouped_f32(NULL)"] = lib.sais_gemm_tn_grouped_f32(None, 4, 264, 1, None)
    out["gemm_tn_grouped_f32(NULL P)"] = lib.sais_gemm_tn_grouped_f32(items, 4, 264, 1, None)
    out["splitk_finish(NULL)"] = lib.sais_splitk_finish(None, 2, 4, 384, 384, None, None, None, 0, None, 0, None, 0, None)
    print(json.dumps(out))


def main():
    libs = [os.path.abspath(p) for p in sys.argv[1:3]]
    bad = 0
    for env in ENVS:
        res = []
        for lib in libs:
            e = {k: v for k, v in os.environ.items() if not k.startswith("SAIS_")}
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(e, SAIS_HIP_LIB=lib, **env),
                               capture_output=True, text=True, check=True)
            res.append(json.loads(r.stdout.strip().splitlines()[-1]))
        label = " ".join(f"{k}={v}" for k, v in env.items()) or "(no switch)"
        for k in res[0]:
            same = res[0][k] == res[1].get(k)
            bad += not same
            print(f"{label:20s} {k:40s} {res[0][k]:>12} {res[1].get(k):>12} {'same' if same else 'DIFFERENT'}")
    print(f"{bad} differences")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
