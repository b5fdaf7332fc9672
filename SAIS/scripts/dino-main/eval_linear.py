#!/usr/bin/env python3
"""Linear probe of a DINO checkpoint on MI355X — the command line, log lines, log.txt and checkpoint files of the
reference's SAIS/scripts/dino-main/eval_linear.py, driving sais_amd.linear (hand-written gfx950 kernels: the frozen backbone's
features from VisionTransformer.probe_features, the classifier heads in exact f32 MFMA arithmetic, no library on the path).

    python SAIS/scripts/dino-main/eval_linear.py --data_path <root with train/ and val/ class folders> \
        --pretrained_weights <output_dir>/checkpoint.pth [--checkpoint_key teacher] [--lr 0.001 | --lr 0.0003 0.001 0.003]

Kept: every flag and default, the linear scaling rule lr * batch / 256, SGD(momentum 0.9, no weight decay) under
CosineAnnealingLR(epochs), the train transform (RandomResizedCrop 224, horizontal flip) and the eval transform (Resize 256
bicubic, CenterCrop 224), DistributedSampler's epoch order at world size 1, `--val_freq`, one JSON line per epoch in
log.txt with the keys train_loss, train_lr, epoch, test_loss, test_acc1, test_acc5 (acc5 only with --num_labels >= 5),
checkpoint.pth.tar in the reference's layout with resume, the lines "Accuracy at epoch ...", "Max accuracy so far" and the
final "Top-1 test accuracy".
Differences: only `--arch vit_small` with `--patch_size 16` or `8`.  `--lr` takes one OR SEVERAL values: the backbone pass, which
dominates a step, then serves one head per value (at most 8).  One value behaves and names its files exactly as the
reference; with several, head i is saved as checkpoint_lr<value>.pth.tar, log.txt gets one line per head and epoch with
an extra `lr0` key (the head's --lr value) and the final line reports the best head.  One process (WORLD_SIZE > 1 exits);
`--dist_url` / `--local_rank` are accepted and ignored.  No download: without `--pretrained_weights` the backbone keeps
its random weights and the script says so; `--evaluate` reads `--linear_weights PATH` (a checkpoint of this script or of
the reference) or the checkpoint in `--output_dir`, and exits with a message if neither exists.  The random draws of the
train transform are this script's own (`--seed`), not torchvision's stream.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from sais_amd import imgfolder, linear  # noqa: E402
from sais_amd.model_io import bool_flag, load_dino_backbone  # noqa: E402


def get_args_parser():
    parser = argparse.ArgumentParser('Evaluation with linear classification on ImageNet')
    parser.add_argument('--n_last_blocks', default=4, type=int, help="""Concatenate [CLS] tokens
        for the `n` last blocks. We use `n=4` when evaluating ViT-Small and `n=1` with ViT-Base.""")
    parser.add_argument('--avgpool_patchtokens', default=False, type=bool_flag,
        help="""Whether ot not to concatenate the global average pooled features to the [CLS] token.
        We typically set this to False for ViT-Small and to True with ViT-Base.""")
    parser.add_argument('--arch', default='vit_small', type=str, help='Architecture')
    parser.add_argument('--patch_size', default=16, type=int, help='Patch resolution of the model.')
    parser.add_argument('--pretrained_weights', default='', type=str, help="Path to pretrained weights to evaluate.")
    parser.add_argument("--checkpoint_key", default="teacher", type=str, help='Key to use in the checkpoint (example: "teacher")')
    parser.add_argument('--epochs', default=100, type=int, help='Number of epochs of training.')
    parser.add_argument("--lr", default=0.001, type=float, nargs='+', help="""Learning rate at the beginning of
        training (highest LR used during training). The learning rate is linearly scaled
        with the batch size, and specified here for a reference batch size of 256.
        Several values train one head each from the same backbone pass.""")
    parser.add_argument('--batch_size_per_gpu', default=128, type=int, help='Per-GPU batch-size')
    parser.add_argument("--dist_url", default="env://", type=str, help="Accepted and ignored.")
    parser.add_argument("--local_rank", default=0, type=int, help="Accepted and ignored.")
    parser.add_argument('--data_path', default='/path/to/imagenet/', type=str)
    parser.add_argument('--num_workers', default=10, type=int, help='Number of data loading workers per GPU.')
    parser.add_argument('--val_freq', default=1, type=int, help="Epoch frequency for validation.")
    parser.add_argument('--output_dir', default=".", help='Path to save logs and checkpoints')
    parser.add_argument('--num_labels', default=1000, type=int, help='Number of labels for linear classifier')
    parser.add_argument('--evaluate', dest='evaluate', action='store_true', help='evaluate model on validation set')
    # not in the reference
    parser.add_argument('--linear_weights', default='', type=str, help="With --evaluate: the classifier checkpoint to read.")
    parser.add_argument('--seed', default=0, type=int, help="Seed of the train transform's draws and of the heads' init.")
    parser.add_argument('--gpu_loader', default=False, type=bool_flag,
                        help="""Decode and transform the images on the GPU (sais_amd/imgfolder.py): the workers only read the
        files.  The batches are bit-identical to the Pillow loader's.""")
    return parser


EXTRA_FLAGS = ("linear_weights", "seed", "gpu_loader")


def build_model(args, dev):
    model = load_dino_backbone(args, dev)
    print(f"Model {args.arch} built.")
    return model


def lr_tag(v):
    return repr(float(v))


def checkpoint_paths(args, lrs):
    if len(lrs) == 1:
        return [os.path.join(args.output_dir, "checkpoint.pth.tar")]
    return [os.path.join(args.output_dir, f"checkpoint_lr{lr_tag(v)}.pth.tar") for v in lrs]


def check_labels(target, num_labels):
    if target.numel() and (int(target.min()) < 0 or int(target.max()) >= num_labels):
        sys.exit(f"a label outside [0, {num_labels}) came from the dataset: set --num_labels to the number of class folders")


def train(model, probe, loader, epoch, n, avgpool, dev):
    """One epoch (eval_linear.py:153-192) -> {'loss': [per head], 'lr': [per head]}: the averages over the steps."""
    total, steps = torch.zeros(probe.H, device=dev), 0
    for it, (inp, target) in enumerate(loader):
        check_labels(target, probe.num_labels)                      # on the host, where the labels are: no device sync
        feats = model.probe_features(inp.to(dev, non_blocking=True), n, avgpool)
        total += probe.step(feats, target.to(dev, non_blocking=True), check_targets=False)
        steps += 1
        if it % 20 == 0:
            print(f"Epoch: [{epoch}]  [{it}/{len(loader)}]  lr: {probe.lrs[0]:.6f}")
    stats = {"loss": (total / max(steps, 1)).tolist(), "lr": list(probe.lrs)}
    print("Averaged stats:", "  ".join(f"loss[{i}]: {v:.6f}" for i, v in enumerate(stats["loss"])))
    return stats


@torch.no_grad()
def validate_network(val_loader, model, probe, n, avgpool, dev):
    """eval_linear.py:195-234 -> per head {'loss', 'acc1'[, 'acc5']}: loss is the average of the batch means, the
    accuracies are weighted by batch size, as the reference's MetricLogger does."""
    H = probe.H
    loss, top1, top5, count, batches = [0.0] * H, [0] * H, [0] * H, 0, 0
    for inp, target in val_loader:
        check_labels(target, probe.num_labels)
        feats = model.probe_features(inp.to(dev, non_blocking=True), n, avgpool)
        ls, t1, t5 = probe.evaluate(feats, target.to(dev, non_blocking=True))
        B = inp.shape[0]
        for h in range(H):
            loss[h] += ls[h] / B
            top1[h] += t1[h]
            top5[h] += t5[h]
        count, batches = count + B, batches + 1
    out = []
    for h in range(H):
        s = {"loss": loss[h] / max(batches, 1), "acc1": 100.0 * top1[h] / max(count, 1)}
        if probe.num_labels >= 5:
            s["acc5"] = 100.0 * top5[h] / max(count, 1)
            print('* Acc@1 {:.3f} Acc@5 {:.3f} loss {:.3f}'.format(s["acc1"], s["acc5"], s["loss"]))
        else:
            print('* Acc@1 {:.3f} loss {:.3f}'.format(s["acc1"], s["loss"]))
        out.append(s)
    return out


def eval_linear(args):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("eval_linear.py runs as one process on one GPU: multi-rank training of the heads is not implemented "
                 "(start it without a distributed launcher)")
    base = args.lr if isinstance(args.lr, (list, tuple)) else [args.lr]
    if not 1 <= len(base) <= linear.MAX_HEADS or len(set(base)) != len(base):
        sys.exit(f"--lr takes 1 to {linear.MAX_HEADS} distinct values")
    print("\n".join("%s: %s" % (k, str(v)) for k, v in sorted(dict(vars(args)).items())))
    dev = torch.device("cuda:0")
    n, avgpool = args.n_last_blocks, args.avgpool_patchtokens
    if avgpool and n != 1:
        sys.exit("--avgpool_patchtokens true needs --n_last_blocks 1 (the reference's torch.cat fails otherwise)")
    embed_dim = 384 * (n + int(avgpool))
    if embed_dim > linear.MAX_DIM:
        sys.exit(f"--n_last_blocks {n}: the heads take at most {linear.MAX_DIM} features")

    paths = checkpoint_paths(args, base)
    files = None
    if args.evaluate:                             # which classifier files: decided before anything is built
        if args.linear_weights:
            if not os.path.isfile(args.linear_weights):
                sys.exit(f"--linear_weights {args.linear_weights}: no such file")
            if len(base) != 1:
                sys.exit("--evaluate with --linear_weights evaluates one head: give one --lr value (or none)")
            files = [args.linear_weights]
        else:
            files = paths
            missing = [p for p in files if not os.path.isfile(p)]
            if missing:
                sys.exit(f"--evaluate: {missing[0]} not found and no --linear_weights given (there is nothing to download)")

    torch.manual_seed(args.seed)                  # (a backbone without --pretrained_weights is the same in every invocation)
    model = build_model(args, dev)
    lrs = [v * args.batch_size_per_gpu / 256. for v in base]                       # linear scaling rule, world size 1
    probe = linear.LinearProbe(embed_dim, args.num_labels, lrs, args.epochs, momentum=0.9, device=dev, seed=args.seed)

    gpu_loader = imgfolder.GpuImageLoader(dev) if args.gpu_loader else None
    if gpu_loader is not None:
        dataset_val = imgfolder.RawLabelledEvalFolder(os.path.join(args.data_path, "val"))
        val_loader = imgfolder.GpuBatches(torch.utils.data.DataLoader(
            dataset_val, batch_size=args.batch_size_per_gpu, num_workers=args.num_workers, collate_fn=imgfolder.collate_raw),
            gpu_loader.eval)
    else:
        dataset_val = linear.LabelledEvalFolder(os.path.join(args.data_path, "val"))
        val_loader = torch.utils.data.DataLoader(dataset_val, batch_size=args.batch_size_per_gpu, num_workers=args.num_workers,
                                                 pin_memory=True)
    if args.evaluate:
        for i, p in enumerate(files):
            ckpt = torch.load(p, map_location="cpu", weights_only=False)
            probe.load_weights(i, ckpt["state_dict"] if "state_dict" in ckpt else ckpt)
        for v, s in zip(base, validate_network(val_loader, model, probe, n, avgpool, dev)):
            tag = "" if len(base) == 1 else f" (lr {lr_tag(v)})"
            print(f"Accuracy of the network on the {len(dataset_val)} test images{tag}: {s['acc1']:.1f}%")
        return

    if gpu_loader is not None:
        dataset_train = imgfolder.RawTrainFolder(os.path.join(args.data_path, "train"), seed=args.seed)
        sampler = linear.EpochSampler(len(dataset_train))
        train_loader = imgfolder.GpuBatches(torch.utils.data.DataLoader(
            dataset_train, sampler=sampler, batch_size=args.batch_size_per_gpu, num_workers=args.num_workers,
            collate_fn=imgfolder.collate_raw), gpu_loader.train)
    else:
        dataset_train = linear.TrainImageFolder(os.path.join(args.data_path, "train"), seed=args.seed)
        sampler = linear.EpochSampler(len(dataset_train))
        train_loader = torch.utils.data.DataLoader(dataset_train, sampler=sampler, batch_size=args.batch_size_per_gpu,
                                                   num_workers=args.num_workers, pin_memory=True)
    print(f"Data loaded with {len(dataset_train)} train and {len(dataset_val)} val imgs.")

    # Optionally resume from a checkpoint (every head of the run, or none)
    start_epoch, best_acc = 0, [0.0] * probe.H
    if all(os.path.isfile(p) for p in paths):
        for i, p in enumerate(paths):
            print("Found checkpoint at {}".format(p))
            got = probe.load_state(i, torch.load(p, map_location="cpu", weights_only=False))
            start_epoch, best_acc[i] = int(got["epoch"]), float(got["best_acc"])
        print(f"=> resuming at epoch {start_epoch}")

    os.makedirs(args.output_dir, exist_ok=True)
    for epoch in range(start_epoch, args.epochs):
        sampler.set_epoch(epoch)
        dataset_train.set_epoch(epoch)
        train_stats = train(model, probe, train_loader, epoch, n, avgpool, dev)
        probe.scheduler_step()
        logs = [{"train_loss": train_stats["loss"][h], "train_lr": train_stats["lr"][h], "epoch": epoch} for h in range(probe.H)]
        if epoch % args.val_freq == 0 or epoch == args.epochs - 1:
            test_stats = validate_network(val_loader, model, probe, n, avgpool, dev)
            for h in range(probe.H):
                tag = "" if probe.H == 1 else f" (lr {lr_tag(base[h])})"
                print(f"Accuracy at epoch {epoch} of the network on the {len(dataset_val)} test images{tag}: "
                      f"{test_stats[h]['acc1']:.1f}%")
                best_acc[h] = max(best_acc[h], test_stats[h]["acc1"])
                print(f'Max accuracy so far{tag}: {best_acc[h]:.2f}%')
                logs[h].update({f"test_{k}": v for k, v in test_stats[h].items()})
        with (Path(args.output_dir) / "log.txt").open("a") as f:
            for h in range(probe.H):
                if probe.H > 1:
                    logs[h]["lr0"] = base[h]
                f.write(json.dumps(logs[h]) + "\n")
        for h, p in enumerate(paths):
            torch.save(probe.state(h, epoch=epoch + 1, best_acc=best_acc[h]), p)
    best = max(range(probe.H), key=lambda h: best_acc[h])
    if probe.H > 1:
        print(f"Best head: lr {lr_tag(base[best])}")
    print("Training of the supervised linear classifier on frozen features completed.\n"
          "Top-1 test accuracy: {acc:.1f}".format(acc=best_acc[best]))


if __name__ == '__main__':
    eval_linear(get_args_parser().parse_args())
