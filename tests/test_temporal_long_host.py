"""CPU-only: the bounds of tests/temporal_long_ref.py are sound (the fp32 restatement of tattn_long.hip stays inside them on
every layout, length and dropout case), sharp (every deliberate error leaves the bar by 10 x somewhere), its recorded tables are
what the restatements give, and its launcher rules are the sources'."""
import ctypes
import functools
import os
import re

import pytest
import torch

import temporal_long_ref as LR
import temporal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@functools.lru_cache(maxsize=None)
def _r_emu(name):
    return LR.r_emu_long(name)


@pytest.mark.parametrize("name", R.LAYOUTS)
def test_bounds_are_sound_and_r_emu_is_what_is_recorded(name):
    """every S of S_LONG with its masks at p = 0 and, for rand, DROP_CASES_LONG with host_keep masks"""
    got = _r_emu(name)
    assert set(got) == {"P", "avg", "ctx", "ctx1"}
    for k, v in got.items():
        assert v <= 1.0, (name, k, v)
        assert "%.3e" % v == "%.3e" % LR.R_EMU_LONG[name][k], (name, k, v, LR.R_EMU_LONG[name][k])
        assert 0 < LR.fwd_bar_long(name, k) <= 1.0


def test_bwd_emu_is_what_is_recorded():
    assert set(LR.BWD_EMU_LONG) == set(LR.BWD_KEYS)
    for key in LR.BWD_KEYS:
        got = LR.bwd_emu_case_long(*key)
        assert ["%.3e" % v for v in got] == ["%.3e" % v for v in LR.BWD_EMU_LONG[key]], (key, got)
        assert all(b > 0 for b in LR.bwd_bars_long(*key))


def test_restatement_equals_the_plain_formula_where_nothing_is_tiled():
    """one key tile: the online recurrence has a single step, so emulate_long is R.emulate up to the order of two products"""
    pad = R.masks(33)
    qkv = R.layouts("rand", pad, R.case_seed("rand", 33))
    a, b = LR.emulate_long(qkv, pad), R.emulate(qkv, pad)
    for k in ("P", "avg", "ctx"):
        assert float((a[k] - b[k]).abs().max()) <= 4 * R.EPS * float(b[k].abs().max()), k
    assert float((a["ctx1"] - b["ctx"]).abs().max()) <= 8 * R.EPS * float(b["ctx"].abs().max())


def _fwd_excess(mutate, name, S, keep=None, p=0.0):
    """worst ratio / bar over the quantities of one case under a mutation"""
    qkv, pad = LR.long_case(name, S)
    ref = LR.attn_fp64_long(qkv, pad, keep, p)
    r = LR.attn_ratios_long(LR.emulate_long(qkv, pad, keep, p, mutate), ref)
    return max(v / LR.fwd_bar_long(name, k) for k, v in r.items())


def _bwd_excess(mutate, name, S, p=0.0):
    qkv, pad, buf, keep, ref = LR.bwd_ref(name, S, p)
    got = LR.emulate_bwd_long(qkv, pad, R.slab_view(buf, qkv.shape[0]), keep, p, mutate)
    return max(g / b for g, b in zip(R.rel_l2_parts(got, ref), LR.bwd_bars_long(name, S, p)))


@pytest.mark.parametrize("mutate", [m for m in LR.MUTATIONS_LONG if m != "mask_index_32bit"])
def test_bounds_are_sharp(mutate):
    """every mutation exceeds the bar by at least 10 x on at least one case, forward or backward"""
    worst = 0.0
    if mutate == "drop_last_slab":
        worst = _bwd_excess(mutate, "rand", 129)
    elif mutate in ("mask_off_by_one", "tile_tail_unmasked"):
        worst = max(_fwd_excess(mutate, "rand", 97), _bwd_excess(mutate, "rand", 97))
    elif mutate == "stale_rescale":
        worst = max(_fwd_excess(mutate, n, S) for n in ("rand", "peaky") for S in (129, 257))
        assert _bwd_excess(mutate, "peaky", 257) >= 10.0
    else:                                                       # the dropout mutations
        S, p = 97, 0.5
        keep = R.host_keep(LR.long_masks(S).shape[0], S, p, 7097)
        worst = _fwd_excess(mutate, "rand", S, keep, p)
    print(mutate, "exceeds the bar by", worst)
    assert worst >= 10.0, (mutate, worst)


def test_mask_index_is_64_bit():
    """4 x 2001^2 x B crosses 2^32 at B = 269: the last element of the largest batch below fits 32 bits, the first past it does
    not, and the sources build the index in 64 bits"""
    S = LR.LONG_MAX_S
    assert LR.mask_index(267, 3, S - 1, S - 1, S) < 2 ** 32 <= LR.mask_index(268, 3, S - 1, S - 1, S)
    assert 4 * S * S * 268 < 2 ** 32 <= 4 * S * S * 269
    assert LR.mask_index(268, 3, S - 1, S - 1, S, bits=32) != LR.mask_index(268, 3, S - 1, S - 1, S)
    assert LR.mask_index(1, 2, 3, 4, 97) == ((1 * 4 + 2) * 97 + 3) * 97 + 4
    src = _src("sais_amd", "csrc", "tattn_frag.hpp")
    assert "base(((unsigned long long)b * TH + h) * S_ * S_)" in src and "base + (unsigned long long)q * S + key" in src
    # the one dropout rule serves the resident and the streaming kernels: neither file draws a mask of its own
    assert src.count("philox_keep(") == 1
    for name in ("tattn.hip", "tattn_long.hip"):
        assert "philox_keep(" not in _src("sais_amd", "csrc", name), name


def test_long_launcher_rules_match_the_sources():
    import __graft_entry__ as ge
    from sais_amd import _lib, temporal
    hdr, src = _src("include", "sais_hip.h"), _src("sais_amd", "csrc", "tattn_long.hip")
    top = int(re.search(r"#define SAIS_TEMPORAL_LONG_MAX_S (\d+)", hdr).group(1))
    assert top == max(LR.S_LONG) == LR.LONG_MAX_S == temporal.NPOS + 1 == _lib.TEMPORAL_LONG_MAX_S
    assert LR.tiles(top) is not None and LR.tiles(top + 1) is None and LR.tiles(0) is None
    assert int(re.search(r"constexpr int LT = (\d+);", src).group(1)) == LR.TILE
    assert [LR.tiles(S) for S in (1, 64, 65, 128, 129, 2001)] == [1, 1, 2, 2, 3, 32]
    # every multiple of the staging tile that S_LONG is meant to straddle is in it
    assert {128, 129}.issubset(LR.S_LONG) and 257 in LR.S_LONG
    assert int(re.search(r"#define SAIS_TEMPORAL_MAX_S_FWD (\d+)", hdr).group(1)) == _lib.TEMPORAL_MAX_S == min(LR.S_LONG) - 1
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("sais_temporal_attn_long_bwd_workspace_bytes", "sais_temporal_attn_fwd_long", "sais_temporal_attn_bwd_long"):
        assert hasattr(lib, name), name
    lib = _lib.load()
    for B, S in ((1, 1), (5, 97), (1, 2001), (269, 2001)):
        assert lib.sais_temporal_attn_long_bwd_workspace_bytes(B, S) == LR.bwd_workspace_bytes(B, S)
    assert lib.sais_temporal_attn_long_bwd_workspace_bytes(1, 2002) == 0 and lib.sais_temporal_attn_long_bwd_workspace_bytes(0, 97) == 0
    # the layer workspace grows past 96 tokens by what the streaming backward needs and is unchanged up to it
    up = lambda b: (b + 255) // 256 * 256
    bwd = lambda B, S: lib.sais_workspace_bytes(_lib.OP_TEMPORAL_LAYER_BWD, B, S)
    assert bwd(2, 131) - bwd(131, 2) == up(LR.bwd_workspace_bytes(2, 131))         # the same M = 262 rows with / without S > 96
    assert bwd(8, 33) == bwd(3, 88) and bwd(1, 96) == bwd(2, 48)
    # bad arguments come back before any launch (no GPU here)
    p16 = ctypes.c_void_p(16)
    assert lib.sais_temporal_attn_fwd_long(None, None, 1, 97, None, None, 0.0, None, 0, None) == -1
    assert lib.sais_temporal_attn_fwd_long(p16, p16, 1, 2002, p16, None, 0.0, None, 0, None) == -1
    assert lib.sais_temporal_attn_fwd_long(p16, p16, 1, 97, p16, None, 0.1, None, 0, None) == -1
    assert lib.sais_temporal_attn_bwd_long(p16, p16, 1, 97, p16, 1, 6, p16, 0.0, None, 0, p16, 1 << 30, None) == -1
    assert lib.sais_temporal_attn_bwd_long(p16, p16, 1, 97, p16, 1, 0, p16, 0.0, None, 0, p16, LR.bwd_workspace_bytes(1, 97) - 1, None) == -1
