#!/usr/bin/env python3
"""Golden vectors of the linear probe, produced by RUNNING THE REFERENCE's own classes on the CPU (build container only:
needs /root/reference).

    python tests/golden/make_golden_linear.py        # rewrites tests/golden/linear.npz

(i) Features: the reference vit_small (vision_transformer.py:225-233, get_intermediate_layers) with synth.vit_state_dict(seed=0)
on synth.clips(seed=10, B=1, T=2)[0] (the inputs of vit.npz), joined exactly as eval_linear.py:166-170 does, for (n = 4,
avgpool False), (n = 1, False), (n = 1, True), plus token rows ROWS of the 4 normed outputs; n = 4 with avgpool must raise
in the reference's torch.cat.
(ii) Trajectories: eval_linear.py's LinearClassifier, torch.optim.SGD(momentum 0.9, weight_decay 0), CosineAnnealingLR,
nn.CrossEntropyLoss and utils.accuracy, driven as eval_linear.py:103-109, 163-183, 206-221 on the cases of
tests/linear_ref.py (the classifier's initial weight is the case's W0), in fp64 and in fp32.  Stored per case: the fp64
loss of every step, the lr of every epoch, the final W (16 sampled rows for c1000; as W - W0 in fp32) and b, the eval loss and top-1 / top-5
counts, a sha256 of the generated inputs, and the reference's OWN fp32 error e_ref_loss = max |loss32 - loss64|,
e_ref_w = relative L2 of W32 - W64 over the stored rows: the yardstick of the GPU trajectory test.  eval_linear.py imports torchvision at the top,
which is stubbed (never touched on this path)."""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import linear_ref  # noqa: E402
import synth  # noqa: E402

REF = "/root/reference/SAIS/scripts"
ROWS = [0, 1, 100, 196]


def import_reference():
    for name in ("timm", "torchvision", "h5py", "cv2"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    tv = sys.modules["torchvision"]
    for sub in ("transforms", "models", "datasets"):
        m = types.ModuleType("torchvision." + sub)
        setattr(tv, sub, m)
        sys.modules["torchvision." + sub] = m
    tv.datasets.ImageFolder = object
    sys.path.insert(0, os.path.join(REF, "dino-main"))
    import eval_linear
    import utils
    import vision_transformer as vits
    return eval_linear, utils, vits


def join(inter, avgpool):
    """eval_linear.py:166-170, verbatim."""
    output = torch.cat([x[:, 0] for x in inter], dim=-1)
    if avgpool:
        output = torch.cat((output.unsqueeze(-1), torch.mean(inter[-1][:, 1:], dim=1).unsqueeze(-1)), dim=-1)
        output = output.reshape(output.shape[0], -1)
    return output


def golden_features(vits, out):
    torch.manual_seed(0)
    model = vits.vit_small(patch_size=16, num_classes=0)
    model.load_state_dict(synth.vit_state_dict(seed=0), strict=True)
    model.eval()
    x = synth.clips(seed=10, B=1, T=2)[0]
    with torch.no_grad():
        inter4 = model.get_intermediate_layers(x, 4)
        inter1 = model.get_intermediate_layers(x, 1)
        out["feat_n4"] = join(inter4, False).numpy()
        out["feat_n1"] = join(inter1, False).numpy()
        out["feat_n1_avgpool"] = join(inter1, True).numpy()
        try:
            join(inter4, True)
            raise AssertionError("the reference joined n = 4 with avgpool")
        except RuntimeError as e:
            print("n = 4 with avgpool raises in the reference:", str(e).splitlines()[0])
        out["normed_rows"] = np.stack([t[:, ROWS].numpy() for t in inter4])          # [4, F, len(ROWS), 384]
    # the oracle's layout against the reference's
    full = [t.numpy() for t in inter4]
    assert np.array_equal(linear_ref.probe_features(full), out["feat_n4"])
    assert np.allclose(linear_ref.probe_features(full[-1:], True), out["feat_n1_avgpool"], atol=1e-6)


def run_reference(eval_linear, utils, case, dtype):
    """eval_linear.py:103-109 (optimiser, scheduler), :163-183 (train step), :206-221 (validation)."""
    C = case["C"]
    clf = eval_linear.LinearClassifier(case["Dm"], num_labels=C)
    clf.linear.weight.data.copy_(torch.from_numpy(case["W0"]))
    clf = clf.to(dtype)
    optimizer = torch.optim.SGD(clf.parameters(), case["lr"], momentum=0.9, weight_decay=0)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, case["epochs"], eta_min=0)
    losses, lrs = [], []
    for ep in case["batches"]:
        clf.train()
        lrs.append(optimizer.param_groups[0]["lr"])
        for x, y in ep:
            output = clf(torch.from_numpy(x).to(dtype))
            loss = nn.CrossEntropyLoss()(output, torch.from_numpy(y))
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            losses.append(loss.item())
        scheduler.step()
    clf.eval()
    xe, ye = case["eval"]
    with torch.no_grad():
        output = clf(torch.from_numpy(xe).to(dtype))
        loss = nn.CrossEntropyLoss()(output, torch.from_numpy(ye)).item()
        n = len(ye)
        if C >= 5:
            acc1, acc5 = utils.accuracy(output, torch.from_numpy(ye), topk=(1, 5))
            counts = [round(acc1.item() * n / 100.0), round(acc5.item() * n / 100.0)]
        else:
            acc1, = utils.accuracy(output, torch.from_numpy(ye), topk=(1,))
            counts = [round(acc1.item() * n / 100.0), -1]
    return dict(loss=np.asarray(losses, dtype=np.float64), lr=np.asarray(lrs, dtype=np.float64),
                W=clf.linear.weight.detach().double().numpy(), b=clf.linear.bias.detach().double().numpy(), eval_loss=loss,
                counts=np.asarray(counts, dtype=np.int64), optimizer=optimizer, scheduler=scheduler)


if __name__ == "__main__":
    eval_linear, utils, vits = import_reference()
    out = {}
    golden_features(vits, out)
    mid = False
    for spec in linear_ref.CASES:
        name = spec[0]
        case = linear_ref.make_case(name)
        r64 = run_reference(eval_linear, utils, case, torch.float64)
        r32 = run_reference(eval_linear, utils, case, torch.float32)
        assert (r64["counts"] == r32["counts"]).all(), "fp32 and fp64 counts differ: change the seed of this case"
        o = linear_ref.trajectory(case)                                   # the numpy oracle against the reference, both fp64
        assert np.abs(o["loss"] - r64["loss"]).max() <= 1e-9 and np.abs(o["W"] - r64["W"]).max() <= 1e-12
        assert np.allclose(o["lr"], r64["lr"], rtol=1e-14, atol=0)
        xe, ye = case["eval"]
        zb = linear_ref.logit_bound(xe, r64["W"], r64["b"])
        nfrag = int(linear_ref.fragile_rows(o["z_eval"], ye, zb).sum())
        n = len(ye)
        assert nfrag <= linear_ref.FRAGILE_CAP * n, "change the seed of this case (linear_ref.CASES), not the cap"
        assert nfrag <= 2, "change the seed, not the cap"
        mid |= 0.20 * n < r64["counts"][0] < 0.95 * n
        rows = np.arange(case["C"]) if case["C"] <= 16 else np.linspace(0, case["C"] - 1, linear_ref.W_SAMPLE_ROWS).astype(np.int64)
        e_loss = float(np.abs(r32["loss"] - r64["loss"]).max())
        e_w = float(np.linalg.norm((r32["W"] - r64["W"])[rows]) / np.linalg.norm(r64["W"][rows]))      # on the stored rows
        # fp64 W as its fp32-rounded difference to the (fp32, regenerated) W0: half the bytes, |rounding| <= 2^-24 |W - W0|
        dw = (r64["W"][rows] - case["W0"][rows].astype(np.float64)).astype(np.float32)
        w_back = case["W0"][rows].astype(np.float64) + dw
        store_err = float(np.linalg.norm(w_back - r64["W"][rows]) / np.linalg.norm(r64["W"][rows]))
        assert store_err <= e_w / 4, (store_err, e_w)                  # under 2 % of the 16 e_ref_w bar
        out.update({f"{name}_sha256": linear_ref.digest(case), f"{name}_loss": r64["loss"], f"{name}_lr": r64["lr"],
                    f"{name}_w_rows": rows, f"{name}_dw": dw, f"{name}_b": r64["b"],
                    f"{name}_eval_loss": np.float64(r64["eval_loss"]), f"{name}_counts": r64["counts"],
                    f"{name}_e_ref_loss": np.float64(e_loss), f"{name}_e_ref_w": np.float64(e_w),
                    f"{name}_fragile": np.int64(nfrag)})
        print(f"{name}: top1 {r64['counts'][0]} top5 {r64['counts'][1]} of {n}; fragile rows {nfrag}; "
              f"e_ref_loss {e_loss:.3g} e_ref_w {e_w:.3g}; final loss {r64['loss'][-1]:.4f}")
    assert mid, "no case ends with top-1 strictly between 20 % and 95 %: change a seed"
    np.savez_compressed(os.path.join(HERE, "linear.npz"), **out)
    print(len(out), "arrays,", os.path.getsize(os.path.join(HERE, "linear.npz")), "bytes")
