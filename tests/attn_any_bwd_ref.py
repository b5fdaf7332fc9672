"""Cases, derived bars and the launcher's published rule for the streaming attention backward (csrc/attn_any_bwd.hip).  Shared by
test_attn_any_bwd_host.py (which recomputes the table and shows that the list catches restated mistakes, on the CPU) and
test_attn_any_bwd_gpu.py; torch only.  The reference (attn_bwd_fp64), the emulation of the kernel's arithmetic (emulate_bwd: the
streaming kernels round where the resident one does), the layouts and the bar rule are attn_ref's; nothing is added to it.

Cases.  Token counts around the 64-row tile (63, 64, 65), two tiles plus one row (129) and a ragged third tile (145), each with
the six backward layouts at 3 frames; the knobs: planted 0.5, up / down 2.0, the others attn_ref's defaults.  Where the emulation
alone is outside the 1.5e-2 bar of the backward the case is not listed, the bar is never raised: at 2 tokens every layout but
rand is far outside (up to 1.7e-1: two keys leave dQ and dK a difference of two roundings), at 17 tokens offp sits at 1.46e-2 —
those two counts take rand only.  rand alone at 785 (a patch-8 frame's count, 13 tiles) and at 4097 tokens (the cap), 1 frame.
"""
import torch

import attn_ref as R

MULT = {"rand": None, "planted": 0.5, "up": 2.0, "down": 2.0, "offp": None, "offn": None}
TILE_NTOK = (63, 64, 65, 129, 145)
# (layout, tokens, frames)
CASES = [(name, ntok, 3) for ntok in TILE_NTOK for name in R.BWD_LAYOUTS] + \
        [("rand", 2, 3), ("rand", 17, 3), ("rand", 785, 1), ("rand", 4097, 1)]

# emulate_bwd against attn_bwd_fp64 (rel-L2 per part dq, dk, dv), measured on the CPU; test_attn_any_bwd_host.py recomputes them
EMU = {
    ("rand", 63): [2.931e-03, 2.827e-03, 2.309e-03],
    ("planted", 63): [2.814e-03, 2.659e-03, 2.118e-03],
    ("up", 63): [1.235e-02, 2.439e-03, 2.328e-03],
    ("down", 63): [1.294e-02, 2.490e-03, 2.325e-03],
    ("offp", 63): [1.301e-02, 2.791e-03, 2.340e-03],
    ("offn", 63): [1.304e-02, 2.796e-03, 2.340e-03],
    ("rand", 64): [2.871e-03, 2.762e-03, 2.305e-03],
    ("planted", 64): [2.824e-03, 2.681e-03, 2.122e-03],
    ("up", 64): [1.236e-02, 2.415e-03, 2.300e-03],
    ("down", 64): [1.300e-02, 2.454e-03, 2.295e-03],
    ("offp", 64): [1.291e-02, 2.724e-03, 2.357e-03],
    ("offn", 64): [1.294e-02, 2.730e-03, 2.358e-03],
    ("rand", 65): [2.856e-03, 2.755e-03, 2.322e-03],
    ("planted", 65): [2.766e-03, 2.637e-03, 2.106e-03],
    ("up", 65): [1.292e-02, 2.376e-03, 2.375e-03],
    ("down", 65): [1.276e-02, 2.408e-03, 2.377e-03],
    ("offp", 65): [1.320e-02, 2.699e-03, 2.348e-03],
    ("offn", 65): [1.324e-02, 2.706e-03, 2.347e-03],
    ("rand", 129): [2.869e-03, 2.737e-03, 2.315e-03],
    ("planted", 129): [2.525e-03, 2.428e-03, 2.624e-03],
    ("up", 129): [1.306e-02, 2.369e-03, 2.354e-03],
    ("down", 129): [1.280e-02, 2.388e-03, 2.355e-03],
    ("offp", 129): [1.302e-02, 2.732e-03, 2.320e-03],
    ("offn", 129): [1.303e-02, 2.735e-03, 2.321e-03],
    ("rand", 145): [2.773e-03, 2.630e-03, 2.310e-03],
    ("planted", 145): [2.522e-03, 2.412e-03, 2.427e-03],
    ("up", 145): [1.262e-02, 2.382e-03, 2.323e-03],
    ("down", 145): [1.343e-02, 2.422e-03, 2.323e-03],
    ("offp", 145): [1.312e-02, 2.612e-03, 2.320e-03],
    ("offn", 145): [1.314e-02, 2.626e-03, 2.317e-03],
    ("rand", 2): [6.915e-03, 6.458e-03, 2.022e-03],
    ("rand", 17): [3.239e-03, 3.185e-03, 2.272e-03],
    ("rand", 785): [2.647e-03, 2.499e-03, 2.358e-03],
    ("rand", 4097): [2.617e-03, 2.431e-03, 2.342e-03],
}


def stream_bwd_waves(frames, ntok):
    """Waves per workgroup of BOTH launches of sais_vit_attn_bwd_any (attn_any_bwd.hip: the forward's rule, 64-row workgroups iff
    there are >= 512 of them, else 32-row ones)."""
    return 4 if frames * R.NH * ((ntok + 63) // 64) >= 512 else 2


def case(name, ntok, frames=3):
    """qkv bf16 [frames ntok, 1152], dout bf16 [frames ntok, 384] (CPU); the seeds of attn_ref.bwd_case"""
    qkv = R.layouts(name, frames, ntok, R.BWD_SEED + ntok, MULT[name])
    g = torch.Generator().manual_seed(R.BWD_SEED + 1000 + ntok)
    return qkv, torch.randn(frames * ntok, R.DM, generator=g).to(torch.bfloat16)


def bars(name, ntok):
    """attn_ref.bwd_bars' rule on this file's table: per part min(1.5e-2, 4 x the emulation's rel-L2 against fp64), floored at the
    rand layout's emulated value of that token count.  The 4 x covers MFMA accumulation order and the hardware exp2."""
    return [max(min(1.5e-2, 4.0 * e), r) for e, r in zip(EMU[(name, ntok)], EMU[("rand", ntok)])]
