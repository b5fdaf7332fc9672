"""ViT-S/16 training at any frame size (streaming attention forward + sais_vit_attn_bwd_any around the size-generic rest of the
launch list): features and every parameter gradient against the fp64 oracle at depth 2, under the project's own bars (features
within 2e-2 max|ref|, gradients within 2e-2 rel-L2; the DINO step under the bars of test_dino_gpu.py's step tests); which
attention a pass takes; the eager DINO step and main_dino.py at other crop sizes."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import synth  # noqa: E402
from parity import parity_log  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEPTH = 2


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _model(drop_path=0.0, seed=22):
    from sais_amd import vit
    sd = synth.vit_state_dict(seed=seed, depth=DEPTH)
    model = vit.vit_small(patch_size=16, depth=DEPTH, drop_path_rate=drop_path)
    model.load_state_dict(sd)
    return model.to(DEV).train(), sd


# 16 tokens; 111 tokens (the CLS-only last block stays: <= 200); 211 tokens (the last block on every row); 128 x 64 tokens = 8192 rows:
# the row-owning GEMMs with LayerNorm epilogues and the grouped weight-gradient launch, with DropPath
@pytest.mark.parametrize("frames,H,W,drop_path,pruned", [(3, 48, 80, 0.0, True), (2, 160, 176, 0.0, True), (2, 224, 240, 0.0, False),
                                                         (128, 112, 144, 0.1, True)])
def test_single_group_gradients_vs_oracle(frames, H, W, drop_path, pruned):
    from oracle import dino_oracle as do
    from sais_amd import ops
    model, sd = _model(drop_path)
    ntok = 1 + (H // 16) * (W // 16)
    assert (frames * ntok >= ops.ROW_GEMM_MIN_M) == (frames == 128)
    x = rnd(frames, 3, H, W, seed=40 + frames).to(DEV)
    wv = rnd(frames, 384, seed=14)
    model.zero_grad()
    rep = model(x)
    saved = rep.grad_fn.saved                                     # (the autograd node is the ctx of _ViTFn)
    assert saved["streaming"] and bool(saved["pruned"]) == pruned
    (rep * wv.to(DEV)).sum().backward()
    dp = None
    if drop_path > 0:
        dp = model.last_droppath_scales.view(2 * DEPTH, frames, ntok)[:, :, 0].double().cpu()
        assert (dp == 0).any()
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ref = do.vit_forward_res(leaves, x.double().cpu(), depth=DEPTH, droppath=dp)
    (ref * wv.double()).sum().backward()
    ferr = (rep.detach().double().cpu() - ref.detach()).abs().max().item() / ref.abs().max().item()
    worst = max(rel(p.grad, leaves[n].grad) for n, p in model.named_parameters())
    print(f"{frames} x {H} x {W}: features {ferr:.3e} of max|ref|, worst gradient rel-L2 {worst:.3e}")
    parity_log(f"vit_anyres_feat_{H}x{W}", ferr, 2e-2)
    parity_log(f"vit_anyres_grad_rel_l2_{H}x{W}", worst, 2e-2)
    assert ferr < 2e-2
    for n, p in model.named_parameters():
        e = rel(p.grad, leaves[n].grad)
        assert e < 2e-2, (n, e)


@pytest.mark.parametrize("sizes", [((2, 128), (4, 64)), ((1, 224), (3, 64))], ids=["128+64", "224+64"])
def test_multi_group_pass_vs_oracle(sizes):
    """rows of both resolutions stacked in ONE streaming pass (what the multi-crop student runs), a 224 x 224 group included"""
    from oracle import dino_oracle as do
    model, sd = _model()
    imgs = [rnd(f, 3, s, s, seed=50 + s).to(DEV) for f, s in sizes]
    wv = rnd(sum(f for f, _ in sizes), 384, seed=15)
    with torch.no_grad():
        groups = [model._check_input(im, "forward") for im in imgs]
        model._engine(groups[0].device)
        assert model.streaming_pass(groups) and not model.streaming_pass([torch.empty(1, 3, 224, 224), torch.empty(1, 3, 96, 96)])
        rep, saved = model._forward_kernels(groups, save=True, streaming=model.streaming_pass(groups))
        assert saved["streaming"] and all(lg is not None for lg in saved["blocks"][0]["lse"])
        model.flat.grad.zero_()
        model._backward_kernels(saved, wv.to(DEV))
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ref = torch.cat([do.vit_forward_res(leaves, im.double().cpu(), depth=DEPTH) for im in imgs])
    (ref * wv.double()).sum().backward()
    ferr = (rep.double().cpu() - ref.detach()).abs().max().item() / ref.abs().max().item()
    parity_log("vit_anyres_multigroup_feat", ferr, 2e-2)
    assert ferr < 2e-2
    worst = 0.0
    for n, _ in model.named_parameters():
        e = rel(model.flat.g(n), leaves[n].grad)
        worst = max(worst, e)
        assert e < 2e-2, (n, e)
    parity_log("vit_anyres_multigroup_grad_rel_l2", worst, 2e-2)


def test_which_attention_a_training_pass_takes():
    """under ops.TIMER (the per-launch list): 224 x 224 keeps the resident pair, 64 x 96 takes the streaming pair"""
    from sais_amd import ops
    model, _ = _model()
    tags = {}
    for name, shape in (("resident", (2, 3, 224, 224)), ("streaming", (2, 3, 64, 96))):
        ops.TIMER = ops.KernelTimer()
        try:
            model.zero_grad()
            model(rnd(*shape, seed=60).to(DEV)).sum().backward()
            torch.cuda.synchronize()
            tags[name] = set(ops.TIMER.recs)
        finally:
            ops.TIMER = None
    assert "vit_attn_bwd" in tags["resident"] and "vit_attn_fwd" in tags["resident"]
    assert not {"vit_attn_bwd_any", "vit_attn_fwd_any"} & tags["resident"]
    assert "vit_attn_bwd_any" in tags["streaming"] and "vit_attn_fwd_any" in tags["streaming"]
    assert not {"vit_attn_bwd", "vit_attn_fwd"} & tags["streaming"]


def test_refusals_that_stay():
    from sais_amd import vit
    model, _ = _model()
    for shape in ((1, 3, 72, 96), (1, 3, 16, 16 * 4097), (1, 3, 0, 64), (3, 64, 64)):
        with pytest.raises(ValueError):
            model(torch.zeros(*shape, device=DEV))
    with torch.no_grad(), pytest.raises(ValueError):              # without gradients forward() keeps its two sizes
        model(torch.zeros(1, 3, 64, 96, device=DEV))
    with pytest.raises(NotImplementedError, match="training runs on patch 16"):
        vit.vit_small(patch_size=8, depth=1).to(DEV)(torch.zeros(1, 3, 64, 64, device=DEV))


def test_dino_train_step_at_128_64_vs_oracle():
    """one eager dino.train_step at global 128 / local 64 (65 and 17 tokens) against oracle.dino_oracle.train_step: loss, centre,
    pre-clip gradients and their norms under the bars of test_dino_gpu.py's step tests"""
    from oracle import dino_oracle as do
    from sais_amd import dino
    out_dim, n_local, B = 1024, 2, 2
    sd = {"backbone." + k: v for k, v in synth.vit_state_dict(seed=23, depth=DEPTH).items()}
    sd.update({"head." + k: v for k, v in synth.dino_head_state_dict(seed=24, out_dim=out_dim).items()})
    student, teacher = dino.build_student_teacher(out_dim=out_dim, drop_path_rate=0.0, device=DEV, depth=DEPTH)
    student.load_state_dict(sd)
    teacher.load_state_dict(student.state_dict())
    student.train()
    loss_mod = dino.DINOLoss(out_dim, n_local + 2, 0.04, 0.07, 3, 10).to(DEV)
    opt = dino.DINOOptimizer(student, teacher)
    crops = synth.dino_crops(seed=340, B=B, n_local=n_local, gsize=128, lsize=64)
    assert [tuple(c.shape) for c in crops] == [(B, 3, 128, 128)] * 2 + [(B, 3, 64, 64)] * n_local
    lr_s, wd_s, mom_s = np.full(4, 1e-4), np.full(4, 0.05), np.full(4, 0.9)
    loss, norms = dino.train_step(student, teacher, loss_mod, opt, [c.to(DEV) for c in crops], 0, 1, lr_s, wd_s, mom_s,
                                  clip_grad=0.05, freeze_last_layer=0)
    st = do.TrainState(sd)
    ref = do.train_step(st, crops, 0, 1, lr_s, wd_s, mom_s, loss_mod.teacher_temp_schedule, 0.05, 0, n_local, depth=DEPTH)
    lerr = abs(loss.item() - ref["loss"]) / ref["loss"]
    parity_log("vit_anyres_step_loss_rel", lerr, 2e-3)
    assert math.isfinite(loss.item()) and lerr < 2e-3
    assert (loss_mod.center.double().cpu() - st.center).abs().max().item() < 2e-3
    names = [n for n, p in student.named_parameters() if p.requires_grad]
    got_n, ref_n = norms.double().cpu().numpy(), np.array([ref["norms"][n] for n in names])
    assert got_n.shape == ref_n.shape
    nerr = np.abs(got_n - ref_n) / np.maximum(ref_n, 1e-12)
    parity_log("vit_anyres_step_grad_norm_rel", float(nerr.max()), 5e-2)
    assert nerr.max() < 5e-2, [n for n, e in zip(names, nerr) if e > 5e-2]
    worst = 0.0
    for who, mod in (("backbone.", student.backbone), ("head.", student.head)):
        for n, p in mod.named_parameters():
            if p.requires_grad:
                e = rel(mod.flat.g(n), ref["grads"][who + n])
                worst = max(worst, e)
                assert e < 3e-2, (who + n, e)
    parity_log("vit_anyres_step_grad_rel_l2", worst, 3e-2)


def test_main_dino_cli_at_128_64_trains_and_resumes(tmp_path):
    """main_dino.py --global_crops_size 128 --local_crops_size 64 on 8 synthetic frames: two iterations (one epoch of two batches),
    a finite loss, and a second invocation that resumes from checkpoint.pth (its probe pass runs at the chosen global size)"""
    import pandas as pd
    from PIL import Image
    root = os.path.dirname(HERE)
    rng = np.random.default_rng(1)
    frames = tmp_path / "frames" / "Images" / "vidA"
    frames.mkdir(parents=True)
    (tmp_path / "paths").mkdir()
    rows = []
    for i in range(8):
        Image.fromarray(rng.integers(0, 256, (270, 480, 3), dtype=np.uint8)).save(frames / f"frames_{i:08d}.jpg")
        rows.append((f"Images\\vidA\\frames_{i:08d}.jpg", "vidA"))
    pd.DataFrame(rows, columns=["path", "label"]).to_csv(tmp_path / "paths" / "VUA_Paths.csv")
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "SAIS", "scripts", "dino-main", "main_dino.py"), "--data_path", str(tmp_path),
           "--frames_root", str(tmp_path / "frames"), "--datasets", "VUA", "--output_dir", str(out), "--batch_size_per_gpu", "4",
           "--local_crops_number", "2", "--out_dim", "1024", "--warmup_epochs", "1", "--num_workers", "0",
           "--saveckp_freq", "1", "--lr", "0.01", "--global_crops_size", "128", "--local_crops_size", "64"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(30800 + os.getpid() % 1000), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd + ["--epochs", "1"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Starting DINO training" in r.stdout and "[0/2]" in r.stdout and os.path.exists(out / "checkpoint0000.pth")
    log = [json.loads(l) for l in open(out / "log.txt")]
    assert [l["epoch"] for l in log] == [0] and math.isfinite(log[0]["train_loss"]) and log[0]["train_loss"] > 0
    ck = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and (ck["args"].global_crops_size, ck["args"].local_crops_size) == (128, 64)
    r = subprocess.run(cmd + ["--epochs", "2"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "resumed from" in r.stdout and "at epoch 1" in r.stdout
    log = [json.loads(l) for l in open(out / "log.txt")]
    assert [l["epoch"] for l in log] == [0, 1] and math.isfinite(log[1]["train_loss"])


def test_gpu_augment_takes_its_view_sizes_from_the_transform():
    """--gpu_augment at other crop sizes: the augmenter sizes its views from the transform's draws, so 128 / 64 views come out equal
    to the Pillow loader's bit for bit (past 224 pixels build_loader exits: test_attn_any_bwd_host.py)"""
    import io
    from PIL import Image
    from test_jpeg_host import encode, frame
    from sais_amd import jpeg
    from sais_amd.augment import DinoAugmenter
    from sais_amd.dino_data import DataAugmentationDINO, apply_view_pillow, border_box, gpu_crops
    fracs, geoms = (0.8, 0.8), [(270, 480), (216, 384), (270, 480)]
    blobs = [encode(frame(h, w, 12, seed=i), quality=85, subsampling=(2, 0)[i % 2]) for i, (h, w) in enumerate(geoms)]
    t = DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), 2, seed=4, global_size=128, local_size=64)
    params = [t.draw(*border_box(w, h, fracs)[2:]) for h, w in geoms]
    assert [p.size for p in params[0]] == [128, 128, 64, 64]
    items = [(b, bytes(jpeg.parse_header(b)), p, 0, "VUA") for b, p in zip(blobs, params)]
    got = gpu_crops(items, jpeg.JpegDecoder("cuda:0"), DinoAugmenter("cuda:0"), fracs)
    assert [tuple(g.shape) for g in got] == [(3, 3, 128, 128)] * 2 + [(3, 3, 64, 64)] * 2
    for i, (b, p) in enumerate(zip(blobs, params)):
        img = Image.open(io.BytesIO(b))
        left, top, cw, ch = border_box(*img.size, fracs)
        img = img.crop((left, top, left + cw, top + ch)).convert("RGB")
        for j, view in enumerate(p):
            assert torch.equal(got[j][i].cpu(), apply_view_pillow(img, view)), (i, j)
