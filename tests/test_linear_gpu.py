"""Linear probe on a real MI355X: probe_features / get_intermediate_layers against the reference's recorded features, the three
head kernels against the fp64 restatement of tests/linear_ref.py within its derived rounding bounds, bit-reproducibility, and
whole trajectories against what the reference's own classes recorded (tests/golden/make_golden_linear.py).

Bars (stated here, used below):
  * features: the project's single feature bar, 2e-2 * max|ref| (tests/test_model_gpu.py FEAT_REL; bf16 MFMA backbone)
  * logits / cross entropy / update: linear_ref's bounds, elementwise (fp32 accumulation in any order, derived, not tuned)
  * trajectories: 16 x the reference's OWN fp32-vs-fp64 error stored in the golden file (one fmaf chain of K = 1536 against
    the CPU's blocked summation: sqrt(1536 / 8) ~ 14, rounded up)
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import linear_ref
import parity
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT_REL = 2e-2
ROWS = [0, 1, 100, 196]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def maxabs(a, b):
    return float(np.abs(host(a).astype(np.float64) - np.asarray(b, dtype=np.float64)).max())


@pytest.fixture(scope="module")
def vit():
    from sais_amd.vit import vit_small
    m = vit_small(patch_size=16, drop_path_rate=0.1)
    m.load_state_dict(synth.vit_state_dict(seed=0), strict=True)
    return m.to(DEV).eval()


def make_probe(C, Dm, lrs, epochs=4, W=None, b=None):
    from sais_amd.linear import LinearProbe
    p = LinearProbe(Dm, C, lrs, epochs, device=DEV, seed=1)
    if W is not None:
        p.W.copy_(dev(W) if isinstance(W, np.ndarray) else W)
    if b is not None:
        p.b.copy_(dev(b) if isinstance(b, np.ndarray) else b)
    return p


# ------------------------------------------------------------------------------------------------ 1. features, F = 2
def test_features_vs_golden_unfused(vit, golden):
    from sais_amd._lib import SaisHipError
    g = golden("linear")
    x = synth.clips(seed=10, B=1, T=2)[0].to(DEV)
    with torch.no_grad():
        rep = vit(x)
    f4, f1, fa = vit.probe_features(x, 4), vit.probe_features(x, 1), vit.probe_features(x, 1, avgpool=True)
    inter = vit.get_intermediate_layers(x, 4)
    assert f4.shape == (2, 1536) and f1.shape == (2, 384) and fa.shape == (2, 768) and len(inter) == 4
    assert all(t.shape == (2, 197, 384) and t.dtype == torch.float32 for t in inter)
    for name, got in (("feat_n4", f4), ("feat_n1", f1), ("feat_n1_avgpool", fa)):
        ref = g[name]
        err, bar = maxabs(got, ref), FEAT_REL * np.abs(ref).max()
        parity.parity_log("linear_" + name, err / np.abs(ref).max(), FEAT_REL)
        assert err <= bar, (name, err, bar)
    for j in range(4):
        ref = g["normed_rows"][j]
        assert maxabs(inter[j][:, ROWS], ref) <= FEAT_REL * np.abs(ref).max(), j
    # the last slot IS forward()'s output: the same CLS-only tail, bit for bit
    assert torch.equal(f4[:, -384:], rep) and torch.equal(f1, rep)
    # the slots are the CLS rows of get_intermediate_layers; the interleaved mean
    bar = FEAT_REL * np.abs(g["feat_n4"]).max()
    for j in range(4):
        assert maxabs(f4[:, 384 * j:384 * (j + 1)], host(inter[j][:, 0])) <= bar, j
    assert maxabs(fa[:, 0::2], host(inter[-1][:, 0])) <= bar
    assert maxabs(fa[:, 1::2], host(inter[-1][:, 1:]).astype(np.float64).mean(axis=1)) <= bar
    assert len(vit.get_intermediate_layers(x, 1)) == 1
    with pytest.raises(ValueError):
        vit.probe_features(x, 4, avgpool=True)
    with pytest.raises(SaisHipError):
        vit.probe_features(x.cpu(), 4)
    with pytest.raises(SaisHipError):
        vit.get_intermediate_layers(x.cpu(), 4)
    with pytest.raises(ValueError):
        vit.probe_features(x, 13)
    assert torch.equal(vit(x), rep)                       # the public forward is untouched by the taps


# ------------------------------------------------------------------------------------------------ 2. features, F = 44
def test_features_fused_path(vit, golden):
    from sais_amd import ops
    g = golden("linear")
    F = 44
    assert F * 197 >= ops.ROW_GEMM_MIN_M > 2 * 197        # this batch takes the fused / block-call path, test 1 does not
    x = torch.cat([synth.clips(seed=10, B=1, T=2)[0], synth.clips(seed=12, B=1, T=F - 2)[0]]).to(DEV)
    ref = g["feat_n4"]
    bar = FEAT_REL * np.abs(ref).max()
    with torch.no_grad():
        rep = vit(x)
    inter = vit.get_intermediate_layers(x, 4)
    for j in range(4):
        r = g["normed_rows"][j]
        assert maxabs(inter[j][:2, ROWS], r) <= FEAT_REL * np.abs(r).max(), j
    for n in (1, 2, 4):
        f = vit.probe_features(x, n)
        assert f.shape == (F, 384 * n)
        err = maxabs(f[:2], ref[:, -384 * n:])
        parity.parity_log("linear_feat_fused", err / np.abs(ref).max(), FEAT_REL)
        assert err <= bar, (n, err, bar)
        assert torch.equal(f[:, -384:], rep)
        for j in range(n):
            assert maxabs(f[:, 384 * j:384 * (j + 1)], host(inter[4 - n + j][:, 0])) <= bar, (n, j)
    fa = vit.probe_features(x, 1, avgpool=True)
    assert maxabs(fa[:2], g["feat_n1_avgpool"]) <= FEAT_REL * np.abs(g["feat_n1_avgpool"]).max()
    assert maxabs(fa[:, 1::2], host(inter[-1][:, 1:]).astype(np.float64).mean(axis=1)) <= bar


# ------------------------------------------------------------------------------------------------ 3. logits / CE / top-5
def head_inputs(B, C, Dm, H, seed, ties=True):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((B, Dm)).astype(np.float32)
    W = (0.05 * rng.standard_normal((H, C, Dm))).astype(np.float32)
    b = (0.1 * rng.standard_normal((H, C))).astype(np.float32)
    if ties and C >= 4:                                  # duplicated classifier rows: exactly equal logits
        for h in range(H):
            W[h, C - 1], b[h, C - 1] = W[h, 1], b[h, 1]
            W[h, C // 2], b[h, C // 2] = W[h, 1], b[h, 1]
    y = rng.integers(0, C, B).astype(np.int64)
    return x, W, b, y


@pytest.mark.parametrize("B,C,Dm,H", [(1, 2, 384, 1), (37, 5, 384, 2), (128, 10, 1536, 1), (200, 1000, 1536, 2), (37, 1000, 384, 1),
                                      (200, 2, 1536, 8), (1, 1000, 1536, 1), (128, 65, 448, 3)])
def test_logits_ce_top5_vs_fp64(B, C, Dm, H):
    x, W, b, y = head_inputs(B, C, Dm, H, 1000 + B + C)
    p = make_probe(C, Dm, [0.1] * H, W=W, b=b)
    xd, td = dev(x), dev(y)
    Z = host(p.logits(xd))
    Ze, rows_e, loss_e, top5 = p._ce(xd, p._targets(td, B, True), False)
    assert np.array_equal(host(Ze), Z)                                       # eval mode leaves the logits alone
    dZ, rows_t, _, none = p._ce(xd, p._targets(td, B, True), True)
    assert none is None and torch.equal(rows_t, rows_e)
    top5, rows, loss, dZ = host(top5), host(rows_e), host(loss_e), host(dZ)
    for h in range(H):
        z64 = linear_ref.logits(x, W[h], b[h])
        zb = linear_ref.logit_bound(x, W[h], b[h])
        err = np.abs(Z[h] - z64)
        parity.parity_log("linear_logits_vs_bound", float((err / zb).max()), 1.0)
        assert (err <= zb).all(), (h, float((err / zb).max()))
        rows64, _, dz64 = linear_ref.cross_entropy(z64, y)
        row_b, dz_b, mean_b = linear_ref.ce_bounds(z64, y, zb)
        assert (np.abs(rows[h] - rows64) <= row_b).all(), float((np.abs(rows[h] - rows64) / row_b).max())
        assert abs(loss[h] - rows64.mean()) <= mean_b
        assert (np.abs(dZ[h] - dz64) <= dz_b).all(), float((np.abs(dZ[h] - dz64) / dz_b).max())
        # top-5: the stable order of the kernel's OWN logits; slots >= C are -1
        assert np.array_equal(top5[h], linear_ref.top5(Z[h].astype(np.float64))), h
        assert (top5[h][:, min(C, 5):] == -1).all() and (top5[h][:, :min(C, 5)] >= 0).all()
        if C >= 4:
            assert (Z[h][:, 1] == Z[h][:, C - 1]).all() and (Z[h][:, 1] == Z[h][:, C // 2]).all()       # the ties are real
    # evaluate(): counts from the same top-5
    ls, t1, t5 = p.evaluate(xd, td)
    for h in range(H):
        assert t1[h] == int((top5[h][:, 0] == y).sum()) and t5[h] == int((top5[h] == y[:, None]).any(axis=1).sum())
        assert abs(ls[h] - float(loss[h]) * B) <= 1e-6 * max(1.0, abs(ls[h]))


# ------------------------------------------------------------------------------------------------ 4. one update step
@pytest.mark.parametrize("B", [1, 37, 200])
def test_update_step_vs_fp64(B):
    C, Dm, H, lrs = 1000, 384, 2, [0.05, 0.3]
    x, W, b, y = head_inputs(B, C, Dm, H, 2000 + B, ties=False)
    p = make_probe(C, Dm, lrs, W=W, b=b)
    for step in (1, 2):                                   # step 2: the momentum buffer is live
        x, _, _, y = head_inputs(B, C, Dm, H, 2000 + B + 7 * step, ties=False)
        xd = dev(x)
        before = {k: host(getattr(p, k)).copy() for k in ("W", "b", "mW", "mb")}
        dZ, rows, loss, _ = p._ce(xd, p._targets(dev(y), B, True), True)
        dz, rws = host(dZ).copy(), host(rows).copy()
        p._update(xd, dZ, rows, loss)
        after = {k: host(getattr(p, k)) for k in ("W", "b", "mW", "mb")}
        assert np.array_equal(host(dZ), dz)               # the update reads dZ only
        for h in range(H):
            want = linear_ref.update_bounds(x, dz[h], before["W"][h], before["b"][h], before["mW"][h], before["mb"][h], lrs[h])
            for k in ("W", "b", "mW", "mb"):
                ref, bound = want[k]
                err = np.abs(after[k][h] - ref)
                assert (err <= bound).all(), (step, h, k, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.abs(after["W"][h] - before["W"][h]).max() > 0
            m = rws[h].astype(np.float64).mean()
            assert abs(float(host(loss)[h]) - m) <= (B + 1) * linear_ref.EPS * np.abs(rws[h]).mean() + linear_ref.EPS * abs(m)


# ------------------------------------------------------------------------------------------------ 5. reproducibility
def run_steps(p, batches):
    losses = [p.step(dev(x), dev(y)) for x, y in batches]
    return torch.stack(losses)


def test_heads_are_independent_and_rows_too():
    C, Dm, B = 1000, 1536, 200
    lrs = [0.01, 0.05, 0.2]
    x, W, b, y = head_inputs(B, C, Dm, 1, 31)
    batches = [head_inputs(n, C, Dm, 1, 40 + i)[::3] for i, n in enumerate((B, 37, 1))]
    p3 = make_probe(C, Dm, lrs, W=np.repeat(W, 3, axis=0), b=np.repeat(b, 3, axis=0))
    l3 = run_steps(p3, batches)
    for h, lr in enumerate(lrs):
        p1 = make_probe(C, Dm, [lr], W=W, b=b)
        l1 = run_steps(p1, batches)
        assert torch.equal(l1[:, 0], l3[:, h])
        for k in ("W", "b", "mW", "mb"):
            assert torch.equal(getattr(p1, k)[0], getattr(p3, k)[h]), (h, k)
    # a row's logits and top-5 depend on nothing but the row
    xd, td = dev(x), dev(y)
    Z, _, _, top5 = p3._ce(xd, p3._targets(td, B, True), False)
    for r in (0, 63, 64, 137, 199):
        z1, _, _, t1 = p3._ce(xd[r:r + 1].contiguous(), p3._targets(td[r:r + 1], 1, True), False)
        assert torch.equal(z1[:, 0], Z[:, r]) and torch.equal(t1[:, 0], top5[:, r]), r
    pa = make_probe(C, Dm, lrs[:1], W=W, b=b)
    assert torch.equal(pa.logits(xd)[0], make_probe(C, Dm, lrs, W=np.repeat(W, 3, axis=0), b=np.repeat(b, 3, axis=0)).logits(xd)[1])


# ------------------------------------------------------------------------------------------------ 6. trajectories
def run_case(case, epochs=None, probe=None, start=0):
    p = probe or make_probe(case["C"], case["Dm"], [case["lr"]], epochs=case["epochs"], W=case["W0"][None],
                            b=np.zeros((1, case["C"]), np.float32))
    losses = []
    for ep in case["batches"][start:epochs]:
        losses += [p.step(dev(x), dev(y)) for x, y in ep]
        p.scheduler_step()
    return p, (host(torch.stack(losses))[:, 0].astype(np.float64) if losses else np.zeros(0))


@pytest.mark.parametrize("name", [c[0] for c in linear_ref.CASES])
def test_trajectory_vs_reference_golden(golden, name):
    g = golden("linear")
    case = linear_ref.make_case(name)
    assert (linear_ref.digest(case) == g[f"{name}_sha256"]).all()
    p, losses = run_case(case)
    p2, losses2 = run_case(case)
    assert np.array_equal(losses, losses2) and torch.equal(p.W, p2.W) and torch.equal(p.b, p2.b)      # two runs: bit-equal
    e_loss, e_w = float(g[f"{name}_e_ref_loss"]), float(g[f"{name}_e_ref_w"])
    d_loss = float(np.abs(losses - g[f"{name}_loss"]).max())
    rows = g[f"{name}_w_rows"]
    w_ref = case["W0"][rows].astype(np.float64) + g[f"{name}_dw"]
    d_w = float(np.linalg.norm(host(p.W[0]).astype(np.float64)[rows] - w_ref) / np.linalg.norm(w_ref))
    print(f"{name}: max|loss - loss64| = {d_loss:.3e} ({d_loss / e_loss:.2f} e_ref_loss), rel L2 W = {d_w:.3e} ({d_w / e_w:.2f} e_ref_w)")
    parity.parity_log("linear_traj_loss", d_loss / e_loss, 16.0)
    parity.parity_log("linear_traj_w", d_w / e_w, 16.0)
    assert d_loss <= 16 * e_loss, (d_loss, e_loss)
    assert d_w <= 16 * e_w, (d_w, e_w)
    assert [p.lrs[0]] == [pytest.approx(linear_ref.cosine_lrs(case["lr"], case["epochs"], case["epochs"] + 1)[-1], abs=1e-15)]
    xe, ye = case["eval"]
    ls, t1, t5 = p.evaluate(dev(xe), dev(ye))
    counts, nfrag = g[f"{name}_counts"], int(g[f"{name}_fragile"])
    assert abs(t1[0] - counts[0]) <= nfrag, (t1, counts, nfrag)
    if case["C"] >= 5:
        assert abs(t5[0] - counts[1]) <= nfrag, (t5, counts, nfrag)
    else:
        assert t5[0] == len(ye)                           # fewer than five classes: every target is among them
    assert abs(ls[0] / len(ye) - float(g[f"{name}_eval_loss"])) <= 16 * e_loss


# ------------------------------------------------------------------------------------------------ 7. resume
def test_resume_is_bit_exact(tmp_path):
    case = linear_ref.make_case("c10")
    straight, _ = run_case(case)
    first, _ = run_case(case, epochs=2)
    torch.save(first.state(0, epoch=2, best_acc=12.5), tmp_path / "checkpoint.pth.tar")
    ck = torch.load(tmp_path / "checkpoint.pth.tar", map_location="cpu", weights_only=False)
    second = make_probe(case["C"], case["Dm"], [case["lr"]], epochs=case["epochs"])
    assert second.load_state(0, ck) == {"epoch": 2, "best_acc": 12.5}
    run_case(case, probe=second, start=2)
    assert second.lrs == straight.lrs and second.last_epoch == straight.last_epoch == 4
    for k in ("W", "b", "mW", "mb"):
        assert torch.equal(getattr(second, k), getattr(straight, k)), k
    # head(i) is the reference's module and computes the same logits
    xe = dev(case["eval"][0])
    with torch.no_grad():
        assert torch.equal(straight.head(0).to(DEV)(xe), straight.logits(xe)[0])


# ------------------------------------------------------------------------------------------------ 8. argument errors
def test_argument_errors():
    from sais_amd._lib import SaisHipError
    from sais_amd.linear import LinearClassifier, LinearProbe
    err = (ValueError, SaisHipError)
    x, W, b, y = head_inputs(8, 10, 384, 1, 5)
    p = make_probe(10, 384, [0.1], W=W, b=b)
    w_before = p.W.clone()
    with pytest.raises(err):
        p.step(torch.from_numpy(x), dev(y))                                   # host features
    with pytest.raises(err):
        p.step(dev(x), torch.from_numpy(y))                                   # host targets
    bad = y.copy()
    bad[3] = 10
    with pytest.raises(err):
        p.step(dev(x), dev(bad))                                              # label == C
    with pytest.raises(err):
        p.evaluate(dev(x), dev(-bad))
    with pytest.raises(err):
        p.step(dev(x[:, :320].copy()), dev(y))                                # mismatched dims
    with pytest.raises(err):
        p.step(dev(x), dev(y[:7]))
    with pytest.raises(err):
        p.step(dev(x), dev(y.astype(np.float32)))
    with pytest.raises(err):
        p.step(dev(np.zeros((1025, 384), np.float32)), dev(np.zeros(1025, np.int64)))      # B = 1025
    with pytest.raises(err):
        LinearProbe(384, 10, [0.1] * 9, 5, device=DEV)                         # H = 9
    with pytest.raises(err):
        LinearProbe(100, 10, [0.1], 5, device=DEV)
    m = LinearClassifier(384, 10).to(DEV)
    with pytest.raises(SaisHipError, match="LinearProbe"):
        m(dev(x))                                                             # a gradient would be required
    with torch.no_grad():
        with pytest.raises(err):
            m(dev(x[:, :320].copy()))
        assert m(dev(x)).shape == (8, 10)
    torch.cuda.synchronize()
    assert torch.equal(p.W, w_before)                                         # nothing was launched


# ------------------------------------------------------------------------------------------------ 9. CLI end to end
def test_cli_end_to_end(tmp_path):
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(5))
    for part, n in (("train", 8), ("val", 4)):
        for c in range(3):
            d = tmp_path / "data" / part / f"class_{c}"
            d.mkdir(parents=True)
            for i in range(n):
                px = np.clip(rng.normal(60 + 60 * c, 40, (72, 96, 3)), 0, 255).astype(np.uint8)
                Image.fromarray(px).save(d / f"img_{i:02d}.jpg", quality=90)
    script = os.path.join(ROOT, "SAIS", "scripts", "dino-main", "eval_linear.py")
    out_dir = tmp_path / "out"

    def run(*extra, ok=True):
        r = subprocess.run([sys.executable, script, "--num_workers", "2", "--batch_size_per_gpu", "16", "--num_labels", "3",
                            "--data_path", str(tmp_path / "data"), "--output_dir", str(out_dir), *extra], capture_output=True,
                           text=True, timeout=600)
        assert (r.returncode == 0) == ok, r.stdout + r.stderr
        return r.stdout + r.stderr
    missing = run("--evaluate", ok=False)
    assert "not found" in missing and "--linear_weights" in missing
    out = run("--epochs", "2", "--lr", "0.01", "0.1")
    assert "random weights" in out and "Data loaded with 24 train and 12 val imgs." in out
    assert len(re.findall(r"^Accuracy at epoch [01] of the network on the 12 test images \(lr 0\.0?1\): [\d.]+%$", out, flags=re.M)) == 4
    assert len(re.findall(r"^Max accuracy so far \(lr 0\.0?1\): [\d.]+%$", out, flags=re.M)) == 4
    final = re.search(r"^Top-1 test accuracy: ([\d.]+)$", out, flags=re.M)
    assert final and "Training of the supervised linear classifier on frozen features completed." in out
    logs = [json.loads(l) for l in (out_dir / "log.txt").read_text().splitlines()]
    assert len(logs) == 4 and [(l["epoch"], l["lr0"]) for l in logs] == [(0, 0.01), (0, 0.1), (1, 0.01), (1, 0.1)]
    for l in logs:
        assert list(l) == ["train_loss", "train_lr", "epoch", "test_loss", "test_acc1", "lr0"]            # no acc5 with 3 labels
        assert np.isfinite(l["train_loss"]) and 0.0 <= l["test_acc1"] <= 100.0
        assert l["train_lr"] == pytest.approx(l["lr0"] * 16 / 256 * (1.0 if l["epoch"] == 0 else 0.5))
    assert float(final.group(1)) == pytest.approx(max(l["test_acc1"] for l in logs), abs=0.05)
    for v in ("0.01", "0.1"):
        ck = torch.load(out_dir / f"checkpoint_lr{v}.pth.tar", map_location="cpu", weights_only=False)
        assert ck["epoch"] == 2 and set(ck["state_dict"]) == {"module.linear.weight", "module.linear.bias"}
        assert ck["state_dict"]["module.linear.weight"].shape == (3, 1536)
        assert ck["scheduler"]["last_epoch"] == 2 and ck["optimizer"]["param_groups"][0]["momentum"] == 0.9
    # a second invocation resumes at the end of the schedule: nothing left to train, nothing appended
    again = run("--epochs", "2", "--lr", "0.01", "0.1")
    assert "resuming at epoch 2" in again and "Accuracy at epoch" not in again
    assert len((out_dir / "log.txt").read_text().splitlines()) == 4
    # --evaluate reproduces the last epoch's accuracy from the run's own files
    ev = run("--evaluate", "--lr", "0.01", "0.1")
    accs = re.findall(r"^Accuracy of the network on the 12 test images \(lr (0\.0?1)\): ([\d.]+)%$", ev, flags=re.M)
    assert [a[0] for a in accs] == ["0.01", "0.1"]
    for (v, acc), l in zip(accs, logs[2:]):
        assert float(acc) == pytest.approx(l["test_acc1"], abs=0.05)
    gone = run("--evaluate", "--linear_weights", str(out_dir / "no_such_file.pth.tar"), ok=False)
    assert "no such file" in gone
