"""CPU-only: host side of the linear probe (the fp64 oracle against the reference's recorded trajectories, CLI flags, lr
schedule, checkpoint layout, train transform, argument checks of the new entry points)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import linear_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in linear_ref.CASES]


def load_cli():
    path = os.path.join(ROOT, "SAIS", "scripts", "dino-main", "eval_linear.py")
    spec = importlib.util.spec_from_file_location("sais_eval_linear", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", NAMES)
def test_fp64_oracle_reproduces_reference_trajectory(golden, name):
    """guards the oracle itself: linear_ref.trajectory against what the reference's classes recorded"""
    g = golden("linear")
    case = linear_ref.make_case(name)
    assert (linear_ref.digest(case) == g[f"{name}_sha256"]).all(), "generated inputs differ from the recorded ones"
    o = linear_ref.trajectory(case)
    assert np.abs(o["loss"] - g[f"{name}_loss"]).max() <= 1e-9
    assert abs(o["eval_loss"] - float(g[f"{name}_eval_loss"])) <= 1e-9
    counts = g[f"{name}_counts"]
    assert o["top1"] == counts[0]
    assert o["top5"] == counts[1] if case["C"] >= 5 else counts[1] == -1
    rows = g[f"{name}_w_rows"]
    w_ref = case["W0"][rows].astype(np.float64) + g[f"{name}_dw"]
    assert np.linalg.norm(o["W"][rows] - w_ref) <= float(g[f"{name}_e_ref_w"]) / 4 * np.linalg.norm(w_ref)       # storage rounding
    assert np.abs(o["b"] - g[f"{name}_b"]).max() <= 1e-12
    # the properties the cases were chosen for
    n = len(case["eval"][1])
    assert int(g[f"{name}_fragile"]) <= 2
    assert 0.20 * n < counts[0] < 0.95 * n


def test_feature_layout_interleaves():
    rng = np.random.default_rng(0)
    normed = [rng.standard_normal((2, 197, 384)) for _ in range(4)]
    f = linear_ref.probe_features(normed)
    assert f.shape == (2, 1536) and np.array_equal(f[:, 384:768], normed[1][:, 0])
    a = linear_ref.probe_features(normed[-1:], avgpool=True)
    assert a.shape == (2, 768)
    assert np.array_equal(a[:, 0::2], normed[-1][:, 0]) and np.allclose(a[:, 1::2], normed[-1][:, 1:].mean(1))
    with pytest.raises(ValueError):
        linear_ref.probe_features(normed, avgpool=True)


def test_top5_tie_rule():
    z = np.array([[1.0, 3.0, 3.0, 0.0, 3.0, 2.0, 2.0], [5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0]])
    assert linear_ref.top5(z).tolist() == [[1, 2, 4, 5, 6], [0, 1, 2, 3, 4]]
    assert linear_ref.top5(np.array([[0.0, 1.0, 1.0]])).tolist() == [[1, 2, 0, -1, -1]]
    t = torch.from_numpy(z)
    assert torch.sort(t, dim=1, descending=True, stable=True).indices[:, :5].tolist() == linear_ref.top5(z).tolist()


def test_cli_flags_match_the_reference():
    mod = load_cli()
    ns = vars(mod.get_args_parser().parse_args([]))
    want = dict(n_last_blocks=4, avgpool_patchtokens=False, arch='vit_small', patch_size=16, pretrained_weights='',
                checkpoint_key='teacher', epochs=100, lr=0.001, batch_size_per_gpu=128, dist_url='env://', local_rank=0,
                data_path='/path/to/imagenet/', num_workers=10, val_freq=1, output_dir='.', num_labels=1000, evaluate=False)
    assert {k: v for k, v in ns.items() if k not in mod.EXTRA_FLAGS} == want
    assert set(ns) - set(want) == set(mod.EXTRA_FLAGS)
    ns = mod.get_args_parser().parse_args(["--lr", "0.01", "0.1", "--avgpool_patchtokens", "true", "--evaluate"])
    assert ns.lr == [0.01, 0.1] and ns.avgpool_patchtokens is True and ns.evaluate is True
    ns = mod.get_args_parser().parse_args(["--arch", "vit_base"])
    with pytest.raises(NotImplementedError, match="--arch vit_small --patch_size 16"):
        mod.build_model(ns, "cpu")
    assert mod.checkpoint_paths(mod.get_args_parser().parse_args(["--output_dir", "o"]), [0.001]) == ["o/checkpoint.pth.tar"]
    assert mod.checkpoint_paths(mod.get_args_parser().parse_args(["--output_dir", "o"]), [0.01, 0.1]) == \
        ["o/checkpoint_lr0.01.pth.tar", "o/checkpoint_lr0.1.pth.tar"]


@pytest.mark.parametrize("name", NAMES)
def test_lr_schedule_matches_the_recorded_one(golden, name):
    from sais_amd.linear import cosine_lr
    g = golden("linear")
    _, _, _, _, _, lr, epochs, _, _, _ = linear_ref.case_spec(name)
    ref = g[f"{name}_lr"]
    got = np.array([cosine_lr(lr, epochs, e) for e in range(epochs)])
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(np.array(linear_ref.cosine_lrs(lr, epochs, epochs)) - ref).max() <= 1e-12 * np.abs(ref).max()
    # against torch's scheduler itself, through T_max and past it
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr, momentum=0.9)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, epochs, eta_min=0)
    for e in range(2 * epochs + 3):
        assert abs(cosine_lr(lr, epochs, e) - opt.param_groups[0]["lr"]) <= 1e-12 * lr, e
        opt.step()
        sch.step()


class _HostProbe:
    """The checkpoint half of LinearProbe on host tensors (LinearProbe's constructor needs the GPU; state / load_state do not)."""

    def __new__(cls, dim, C, lrs, epochs):
        from sais_amd.linear import LinearProbe
        p = object.__new__(LinearProbe)
        p.dim, p.num_labels, p.base_lrs, p.epochs, p.momentum, p.H = dim, C, list(lrs), epochs, 0.9, len(lrs)
        p.last_epoch, p.lrs = 0, list(lrs)
        gen = torch.Generator().manual_seed(3)
        p.W = torch.randn(p.H, C, dim, generator=gen)
        p.b = torch.randn(p.H, C, generator=gen)
        p.mW, p.mb = torch.randn(p.H, C, dim, generator=gen), torch.randn(p.H, C, generator=gen)
        return p


def test_checkpoint_layout_round_trip_and_torch_compatibility():
    from sais_amd.linear import LinearClassifier
    a = _HostProbe(64, 5, [0.05, 0.2], 7)
    for _ in range(3):
        a.scheduler_step()
    ck = a.state(1, epoch=3, best_acc=61.5)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "scheduler", "best_acc"}
    assert set(ck["state_dict"]) == {"module.linear.weight", "module.linear.bias"}
    assert ck["epoch"] == 3 and ck["best_acc"] == 61.5
    # round trip into another probe
    b = _HostProbe(64, 5, [0.05, 0.2], 7)
    b.W.zero_(); b.b.zero_(); b.mW.zero_(); b.mb.zero_()
    got = b.load_state(1, ck)
    assert got == {"epoch": 3, "best_acc": 61.5} and b.last_epoch == 3 and b.lrs[1] == a.lrs[1]
    for name in ("W", "b", "mW", "mb"):
        assert torch.equal(getattr(a, name)[1], getattr(b, name)[1]), name
    # the reference resumes from our file: DistributedDataParallel(LinearClassifier) + SGD + CosineAnnealingLR (utils.py
    # restart_from_checkpoint calls load_state_dict on each)
    clf = LinearClassifier(64, 5)
    wrapped = torch.nn.Module()
    wrapped.module = clf
    wrapped.load_state_dict(ck["state_dict"], strict=True)
    opt = torch.optim.SGD(clf.parameters(), 0.2, momentum=0.9, weight_decay=0)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 7, eta_min=0)
    opt.load_state_dict(ck["optimizer"])
    sch.load_state_dict(ck["scheduler"])
    assert opt.param_groups[0]["lr"] == a.lrs[1] and sch.last_epoch == 3
    assert torch.equal(opt.state[clf.linear.weight]["momentum_buffer"], a.mW[1])
    sch.step()
    a.scheduler_step()
    assert abs(opt.param_groups[0]["lr"] - a.lrs[1]) <= 1e-15
    # ... and the reverse: what torch writes loads here (also before its first step: no momentum buffer yet)
    ref_ck = {"epoch": 4, "state_dict": wrapped.state_dict(), "optimizer": opt.state_dict(), "scheduler": sch.state_dict(),
              "best_acc": 70.0}
    c = _HostProbe(64, 5, [0.2], 7)
    assert c.load_state(0, ref_ck)["epoch"] == 4 and c.last_epoch == 4
    assert torch.equal(c.mW[0], a.mW[1]) and abs(c.lrs[0] - a.lrs[1]) <= 1e-15
    fresh = torch.optim.SGD(clf.parameters(), 0.2, momentum=0.9)
    ref_ck["optimizer"] = fresh.state_dict()
    c.load_state(0, ref_ck)
    assert not c.mW[0].any() and not c.mb[0].any()
    with pytest.raises(ValueError):
        _HostProbe(64, 6, [0.2], 7).load_state(0, ck)


def test_linear_classifier_init_and_guards():
    from sais_amd._lib import SaisHipError
    from sais_amd.linear import LinearClassifier, LinearProbe
    torch.manual_seed(0)
    m = LinearClassifier(384 * 4)
    assert m.linear.weight.shape == (1000, 1536) and not m.linear.bias.any()
    assert abs(float(m.linear.weight.detach().std()) - 0.01) < 2e-4
    with pytest.raises(SaisHipError, match="LinearProbe"):
        m(torch.zeros(2, 1536))                                    # a gradient would be required
    with torch.no_grad(), pytest.raises(SaisHipError):
        m(torch.zeros(2, 1536))                                    # host tensors
    for bad in (dict(dim=100), dict(dim=1984), dict(num_labels=0), dict(num_labels=4097)):
        with pytest.raises(ValueError):
            LinearClassifier(**{"dim": 384, **bad})
    with pytest.raises(ValueError):
        LinearProbe(384, 10, [0.1] * 9, 5)                         # H = 9
    with pytest.raises(ValueError):
        LinearProbe(384, 10, [0.0], 5)
    with pytest.raises(SaisHipError):
        LinearProbe(384, 10, [0.1], 5, device="cpu")


def test_train_image_folder(tmp_path):
    from PIL import Image
    from sais_amd.linear import EpochSampler, TrainImageFolder, epoch_order
    rng = np.random.default_rng(1)
    for c in range(2):
        (tmp_path / f"c{c}").mkdir()
        for i in range(5):
            Image.fromarray(rng.integers(0, 256, (60 + 7 * i, 90 - 5 * i, 3), dtype=np.uint8)).save(tmp_path / f"c{c}" / f"{i}.png")
    ds = TrainImageFolder(str(tmp_path), seed=3)
    assert len(ds) == 10
    flips = []
    for e in range(3):
        ds.set_epoch(e)
        for i in range(10):
            W, H = 90 - 5 * (i % 5), 60 + 7 * (i % 5)
            (l, t, r, b), flip = ds.draw(i, W, H)
            assert 0 <= l < r <= W and 0 <= t < b <= H
            area, ratio = (r - l) * (b - t) / (W * H), (r - l) / (b - t)
            assert 0.06 <= area <= 1.0 and 0.7 <= ratio <= 1.4
            flips.append(flip)
    assert 5 <= sum(flips) <= 25
    ds.set_epoch(1)
    x, y = ds[7]
    assert x.shape == (3, 224, 224) and x.dtype == torch.float32 and y == 1
    assert torch.equal(ds[7][0], x)                                # a function of (seed, epoch, index) only
    ds.set_epoch(2)
    assert not torch.equal(ds[7][0], x)
    assert not torch.equal(TrainImageFolder(str(tmp_path), seed=4)[7][0], ds[7][0])
    # the flip mirrors
    img = Image.open(tmp_path / "c0" / "0.png")
    box = (5, 6, 70, 50)
    assert torch.equal(TrainImageFolder.apply(img, box, True), TrainImageFolder.apply(img, box, False).flip(-1))
    # draws independent of the worker count
    ds.set_epoch(1)
    sampler = EpochSampler(len(ds))
    sampler.set_epoch(1)
    runs = []
    for workers in (0, 2):
        loader = torch.utils.data.DataLoader(ds, sampler=sampler, batch_size=4, num_workers=workers)
        runs.append([(xb.clone(), yb.clone()) for xb, yb in loader])
    assert [len(r) for r in runs] == [3, 3]
    for (xa, ya), (xb, yb) in zip(*runs):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    # DistributedSampler's order at world size 1
    want = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=1, rank=0)
    want.set_epoch(1)
    assert list(want) == epoch_order(len(ds), 1) == list(sampler)


def test_new_entries_reject_bad_arguments():
    from sais_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert lib.sais_probe_logits(None, None, None, 1, 4, 10, 384, None, None) == -1
    for H, B, C, Dm in ((0, 4, 10, 384), (9, 4, 10, 384), (1, 0, 10, 384), (1, 1025, 10, 384), (1, 4, 0, 384), (1, 4, 4097, 384),
                        (1, 4, 10, 100), (1, 4, 10, 0), (1, 4, 10, 1984)):
        assert lib.sais_probe_logits(p, p, p, H, B, C, Dm, p, None) == -1, (H, B, C, Dm)
    assert lib.sais_probe_ce(None, None, 1, 4, 10, 1, None, None, None, None) == -1
    assert lib.sais_probe_ce(p, p, 9, 4, 10, 1, p, p, p, None) == -1
    assert lib.sais_probe_ce(p, p, 1, 1025, 10, 1, p, p, p, None) == -1
    assert lib.sais_probe_ce(p, p, 1, 4, 4097, 1, p, p, p, None) == -1
    assert lib.sais_probe_ce(p, p, 1, 4, 10, 0, p, None, p, None) == -1            # eval mode writes top5 and loss
    assert lib.sais_probe_ce(p, p, 1, 4, 10, 0, p, p, None, None) == -1

    def upd(**kw):
        a = dict(X=16, dZ=16, W=16, b=16, mW=16, mb=16, loss_rows=16, loss=16, H=1, B=4, C=10, Dm=384, momentum=0.9)
        a.update(kw)
        lr = a.pop("lr", [0.1] * 8)
        return _lib.SaisProbeUpdate(lr=(ctypes.c_float * 8)(*lr), **a)
    assert lib.sais_probe_update(None, None) == -1
    for bad in (dict(X=None), dict(dZ=None), dict(W=None), dict(mb=None), dict(H=9), dict(B=1025), dict(C=0), dict(Dm=96),
                dict(Dm=1984), dict(momentum=-0.1), dict(momentum=1.0), dict(lr=[-0.1] + [0.1] * 7), dict(lr=[float("nan")] + [0.1] * 7),
                dict(loss=None), dict(loss_rows=None)):
        assert lib.sais_probe_update(ctypes.byref(upd(**bad)), None) == -1, bad
    assert lib.sais_vit_cls_avgpool_norm(None, 197 * 384, 2, 197, 384, None, None, 1e-6, None, 768, None) == -1
    for fs, frames, ntok, dim, ldy in ((197 * 384, 0, 197, 384, 768), (197 * 384, 2, 1, 384, 768), (197 * 384, 2, 197, 768, 768),
                                       (196 * 384, 2, 197, 384, 768), (197 * 384, 2, 197, 384, 384)):
        assert lib.sais_vit_cls_avgpool_norm(p, fs, frames, ntok, dim, p, p, 1e-6, p, ldy, None) == -1, (fs, frames, ntok, dim, ldy)
