"""CPU only.  The table behind the bars of attn_any_bwd_ref is reproduced and every case is inside its own bar; the case list
catches three restated mistakes of a streaming backward by a factor of ten; sais_vit_attn_bwd_any refuses bad arguments before
any launch and its workspace query is monotone; the two crop-size switches of main_dino.py."""
import argparse
import ctypes
import importlib.util
import os

import pytest
import torch

import attn_any_bwd_ref as B
import attn_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
MISTAKES = ("tail_unmasked", "no_delta", "no_dk_scale")


_REF = {}


def _ref(name, ntok, frames):
    """(qkv, dout, fp64 reference) of a case, computed once"""
    key = (name, ntok, frames)
    if key not in _REF:
        qkv, dout = B.case(name, ntok, frames)
        _REF[key] = (qkv, dout, R.attn_bwd_fp64(qkv, dout, frames, ntok))
    return _REF[key]


def test_case_list_is_the_stated_one():
    assert len(B.CASES) == 5 * 6 + 4 and len(set(B.CASES)) == len(B.CASES) and set(B.EMU) == {(n, t) for n, t, _ in B.CASES}
    assert {t for _, t, _ in B.CASES} == {63, 64, 65, 129, 145, 2, 17, 785, 4097}
    assert all(f == (1 if t in (785, 4097) else 3) for _, t, f in B.CASES)
    assert all(n == "rand" for n, t, _ in B.CASES if t in (2, 17, 785, 4097))
    assert B.MULT == {"rand": None, "planted": 0.5, "up": 2.0, "down": 2.0, "offp": None, "offn": None}
    # both forms of the launcher are within reach of small shapes, and the rule is the forward's
    assert B.stream_bwd_waves(3, 129) == 2 and B.stream_bwd_waves(30, 129) == 4 and B.stream_bwd_waves(29, 129) == 4
    assert all(B.stream_bwd_waves(f, t) == R.stream_waves(f, t) for f in (1, 3, 28, 29, 86) for t in (2, 64, 65, 129, 4097))


@pytest.mark.parametrize("name,ntok,frames", B.CASES, ids=[f"{n}-{t}x{f}" for n, t, f in B.CASES])
def test_table_is_reproduced_and_inside_the_bars(name, ntok, frames):
    """emulate_bwd against fp64 autograd gives the recorded values (to 2 %: thread count and BLAS); each is inside its own bar,
    which follows the stated rule and is never above 1.5e-2"""
    qkv, dout, ref = _ref(name, ntok, frames)
    emu = R.rel_l2_parts(R.emulate_bwd(qkv, dout, frames, ntok), ref)
    rec, bars = B.EMU[(name, ntok)], B.bars(name, ntok)
    print(f"{name} {ntok}: emulated " + ", ".join(f"{e:.3e}" for e in emu) + " bars " + ", ".join(f"{b:.3e}" for b in bars))
    for e, r, b, rr in zip(emu, rec, bars, B.EMU[("rand", ntok)]):
        assert abs(e - r) <= 0.02 * r
        assert e <= b and r <= b <= 1.5e-2
        assert b == max(min(1.5e-2, 4 * r), rr)


def _restated(qkv, dout, frames, ntok, mistake=None):
    """attn_ref.emulate_bwd written out again with one deliberate error of a streaming backward:
      tail_unmasked  the keys that pad the last 64-row tile keep their score: they are copies of the last key (clamped loads) with
                     zero V rows, so each adds P_last (0 - delta) K_last to dQ
      no_delta       dS = P dP
      no_dk_scale    dK = dS^T Q without the 1/8"""
    assert mistake is None or mistake in MISTAKES
    bf = lambda x: x.to(torch.bfloat16).float()
    q, k, v = (x.float() for x in R.heads(qkv, frames, ntok))
    do = dout.float().reshape(frames, ntok, R.NH, R.HD).permute(0, 2, 1, 3)
    c = R.SCALE * R.LOG2E
    s = q @ k.transpose(-2, -1)
    m = s.amax(-1, keepdim=True)
    e = torch.exp2((s - m) * c)
    z = e.sum(-1, keepdim=True)
    out = bf((bf(e) @ v) / z)
    lse = m * R.SCALE + z.log()
    p = torch.exp2(s * c - lse * R.LOG2E)
    delta = (do * out).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-2, -1) - (0.0 if mistake == "no_delta" else delta))
    dv = bf(p).transpose(-2, -1) @ do
    dk = (bf(ds).transpose(-2, -1) @ q) * (1.0 if mistake == "no_dk_scale" else R.SCALE)
    dq = (bf(ds) @ k) * R.SCALE
    if mistake == "tail_unmasked":
        npad = -ntok % 64
        dq = dq + npad * bf(p[..., -1:] * (0.0 - delta)) * k[..., -1:, :] * R.SCALE
    g = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4)
    return g.reshape(frames * ntok, 3 * R.DM).to(torch.bfloat16)


def test_restatement_is_the_emulation():
    qkv, dout, _ = _ref("rand", 65, 3)
    assert torch.equal(_restated(qkv, dout, 3, 65), R.emulate_bwd(qkv, dout, 3, 65))


@pytest.mark.parametrize("mistake", MISTAKES)
def test_the_list_catches_restated_mistakes(mistake):
    """each mistake exceeds a bar of a listed case by >= 10 x (65 tokens: 63 pad keys in the second tile)"""
    worst = 0.0
    for name, ntok, frames in [("rand", 65, 3), ("planted", 129, 3)]:
        qkv, dout, ref = _ref(name, ntok, frames)
        got = R.rel_l2_parts(_restated(qkv, dout, frames, ntok, mistake), ref)
        print(mistake, name, ntok, got, B.bars(name, ntok))
        worst = max(worst, max(g / b for g, b in zip(got, B.bars(name, ntok))))
    assert worst >= 10.0, (mistake, worst)


# ---------------------------------------------------------------------------------------------- the C entry, no GPU
def _lib():
    import __graft_entry__ as ge
    from sais_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_bad_arguments_are_refused_without_a_gpu():
    lib = _lib()
    P = ctypes.c_void_p(4096)                                  # never dereferenced: every call below is refused before a launch
    need = lib.sais_vit_attn_bwd_any_workspace_bytes

    def call(qkv=P, ldq=1152, dout=P, lddo=384, out=P, ldout=384, lse=P, frames=2, ntok=65, dqkv=P, lddq=1152, ws=P, nbytes=None):
        nbytes = need(max(frames, 1), max(ntok, 1)) if nbytes is None else nbytes
        return lib.sais_vit_attn_bwd_any(qkv, ldq, dout, lddo, out, ldout, lse, frames, ntok, dqkv, lddq, ws, nbytes, None)
    for bad in (dict(ntok=1), dict(ntok=4098), dict(frames=0), dict(frames=65536), dict(frames=-1)):
        assert call(**bad) == -1, bad
    for name in ("ldq", "lddq"):
        assert call(**{name: 1156}) == -1 and call(**{name: 1144}) == -1, name          # not a multiple of 8 / below the row width
    for name in ("lddo", "ldout"):
        assert call(**{name: 388}) == -1 and call(**{name: 376}) == -1, name
    assert call(nbytes=need(2, 65) - 1) == -1 and call(nbytes=0) == -1
    for name in ("qkv", "dout", "out", "lse", "dqkv", "ws"):
        assert call(**{name: None}) == -1, name


def test_workspace_query_is_monotone():
    need = _lib().sais_vit_attn_bwd_any_workspace_bytes
    assert need(1, 2) >= 1 * 6 * 2 * 4 and need(65535, 4097) >= 65535 * 6 * 4097 * 4 and need(0, 65) == 0 and need(2, 0) == 0
    frames, ntoks = (1, 2, 3, 64, 65, 1000, 65535), (2, 3, 63, 64, 65, 197, 1561, 4097)
    for a, b in zip(frames, frames[1:]):
        assert all(need(a, t) <= need(b, t) for t in ntoks)
    for s, t in zip(ntoks, ntoks[1:]):
        assert all(need(f, s) <= need(f, t) for f in frames)


# ---------------------------------------------------------------------------------------------- main_dino.py
def _load_cli():
    path = os.path.join(os.path.dirname(HERE), "SAIS", "scripts", "dino-main", "main_dino.py")
    spec = importlib.util.spec_from_file_location("sais_main_dino_anyres", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_crop_size_switches(capsys):
    mod = _load_cli()
    cli = mod.get_cli_parser()
    a = cli.parse_args([])
    assert (a.global_crops_size, a.local_crops_size) == (224, 96)
    ref_flags = {o for act in mod.get_args_parser()._actions for o in act.option_strings}
    assert "--global_crops_size" not in ref_flags and "--local_crops_size" not in ref_flags
    a = cli.parse_args(["--global_crops_size", "128", "--local_crops_size", "64"])
    assert (a.global_crops_size, a.local_crops_size) == (128, 64)
    assert cli.parse_args(["--global_crops_size", "1024"]).global_crops_size == 1024         # 4097 tokens
    for bad in (["--local_crops_size", "100"], ["--local_crops_size", "0"], ["--global_crops_size", "-16"],
                ["--global_crops_size", "1040"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    assert "multiple of 16" in capsys.readouterr().err
    with pytest.raises(argparse.ArgumentTypeError):
        mod.crop_size("100")


def test_build_loader_hands_the_sizes_to_the_transform(monkeypatch):
    mod = _load_cli()
    seen = {}

    class FakeDataset(torch.utils.data.Dataset):
        def __init__(self, data_path, datasets, transform, frames_root="./SAIS", gpu_augment=False):
            seen["transform"], seen["gpu_augment"] = transform, gpu_augment

        def __len__(self):
            return 4

        def __getitem__(self, i):
            return [torch.zeros(3, 16, 16)], 0, "x"
    monkeypatch.setattr(mod, "SurgDataset", FakeDataset)
    args = mod.get_cli_parser().parse_args(["--global_crops_size", "128", "--local_crops_size", "64", "--num_workers", "0",
                                            "--batch_size_per_gpu", "2"])
    args.rank, args.world_size = 0, 1
    mod.build_loader(args, torch.device("cpu"))
    t = seen["transform"]
    assert (t.gsize, t.lsize) == (128, 64) and not seen["gpu_augment"]
    assert [spec[0] for spec in t._view_specs()] == [128, 128] + [64] * args.local_crops_number
    views = t.draw(640, 480)                                   # the draws the GPU augmenter sizes its views from
    assert [v.size for v in views] == [128, 128] + [64] * args.local_crops_number
    # the GPU augmenter holds views up to 224 pixels: beyond it, one clear sentence instead of a refused kernel argument
    args = mod.get_cli_parser().parse_args(["--global_crops_size", "256", "--gpu_augment", "true"])
    args.rank, args.world_size = 0, 1
    with pytest.raises(SystemExit, match="--gpu_augment makes views of at most 224 x 224 pixels"):
        mod.build_loader(args, torch.device("cpu"))
