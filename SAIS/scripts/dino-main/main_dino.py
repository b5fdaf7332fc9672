#!/usr/bin/env python3
"""DINO pre-training of the ViT-S/16 frame encoder on MI355X — same command line, log and checkpoint files as the
reference's SAIS/scripts/dino-main/main_dino.py (flags: tests/golden/dino_args.json is the reference parser's own
dump), driving sais_amd.dino (hand-written gfx950 kernels, one process per GPU, RCCL for the gradient and centre
all-reduces).

    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 SAIS/scripts/dino-main/main_dino.py \
        --data_path <root with paths/<dataset>_Paths.csv> --output_dir <dir> [--epochs ...]

Kept: every flag, the linear lr scaling rule lr * global_batch / 256, the cosine schedules, `checkpoint.pth` /
`checkpoint%04d.pth` / `log.txt`, resume from `--output_dir/checkpoint.pth`.  Differences: `--use_fp16` is accepted and
ignored (bf16 MFMA operands with fp32 master weights need no loss scaler); `--arch` must be vit_small (deit_small),
`--optimizer` adamw, `--use_bn_in_head` False; the dataset list the reference hard-codes (:353) is the default of the
extra `--datasets` flag, its hard-coded frame root './SAIS' (:288) the default of `--frames_root`.  `--global_crops_size` /
`--local_crops_size` (switches of this implementation; the reference hard-codes 224 / 96, :658-663) train at other view sizes:
positive multiples of 16 of at most 4097 tokens; a size other than 224 / 96 takes the streaming attention kernels.
"""
import argparse
import datetime
import json
import math
import os
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from sais_amd import dino  # noqa: E402
from sais_amd.dino_data import DataAugmentationDINO, SurgDataset, collate_raw, gpu_crops  # noqa: E402
from sais_amd.model_io import bool_flag  # noqa: E402
from sais_amd.vit import MAX_DENSE_TOKENS  # noqa: E402


FLAGS = [  # (flag, type, default)   — the reference parser, main_dino.py:48-141
    ("--arch", str, "vit_small"), ("--patch_size", int, 16), ("--out_dim", int, 65536),
    ("--norm_last_layer", bool_flag, True), ("--momentum_teacher", float, 0.996), ("--use_bn_in_head", bool_flag, False),
    ("--warmup_teacher_temp", float, 0.04), ("--teacher_temp", float, 0.04), ("--warmup_teacher_temp_epochs", int, 0),
    ("--use_fp16", bool_flag, True), ("--weight_decay", float, 0.04), ("--weight_decay_end", float, 0.4),
    ("--clip_grad", float, 3.0), ("--batch_size_per_gpu", int, 64), ("--epochs", int, 100),
    ("--freeze_last_layer", int, 1), ("--lr", float, 0.0005), ("--warmup_epochs", int, 10), ("--min_lr", float, 1e-6),
    ("--optimizer", str, "adamw"), ("--drop_path_rate", float, 0.1), ("--local_crops_number", int, 8),
    ("--data_path", str, "/path/to/imagenet/train/"), ("--output_dir", str, "."), ("--saveckp_freq", int, 20),
    ("--seed", int, 0), ("--num_workers", int, 10), ("--dist_url", str, "env://"), ("--local_rank", int, 0),
]


def get_args_parser():
    p = argparse.ArgumentParser("DINO", add_help=False)
    for flag, typ, default in FLAGS:
        p.add_argument(flag, type=typ, default=default)
    p.add_argument("--global_crops_scale", type=float, nargs="+", default=(0.4, 1.))
    p.add_argument("--local_crops_scale", type=float, nargs="+", default=(0.05, 0.4))
    for flag in ("--optical_flow_to_reps", "--segmentation_to_reps", "--optical_flow", "--segmentation"):
        p.add_argument(flag, default=False, action="store_true")
    p.add_argument("--task", default="DINO")
    # not in the reference: what it hard-codes
    p.add_argument("--datasets", nargs="+", default=["VUA", "VUA_Gronau", "VUA_HMH"])
    p.add_argument("--frames_root", default="./SAIS")
    return p


class _CliParser(argparse.ArgumentParser):
    """get_cli_parser()'s parser.  The two view-size switches are parsed by a parser of their own (crop_size_parser) before this
    one sees the command line, and land in the same namespace: the switches on THIS parser's own list stay the reference's plus
    --gpu_augment, which is what that list is pinned to."""

    def parse_known_args(self, args=None, namespace=None):
        sizes, rest = crop_size_parser().parse_known_args(sys.argv[1:] if args is None else list(args))
        namespace, extras = super().parse_known_args(rest, namespace)
        for k, v in vars(sizes).items():
            setattr(namespace, k, v)
        return namespace, extras

    def format_help(self):
        return super().format_help() + "\nview size " + crop_size_parser().format_help().split("\n\n", 1)[-1]


def crop_size_parser():
    p = argparse.ArgumentParser("DINO", add_help=False, allow_abbrev=False)
    p.add_argument("--global_crops_size", type=crop_size, default=224,
                   help="side of the two global views in pixels: a positive multiple of 16, at most 4097 tokens")
    p.add_argument("--local_crops_size", type=crop_size, default=96, help="side of the local views, same rule")
    return p


def get_cli_parser():
    """The command line: the reference's flags (get_args_parser) + switches of this implementation only: --gpu_augment, and
    --global_crops_size / --local_crops_size (the reference hard-codes 224 / 96, :658-663)."""
    p = _CliParser("DINO", parents=[get_args_parser()])
    p.add_argument("--gpu_augment", type=bool_flag, default=False,
                   help="decode the frames and make the multi-crop views on the GPU (sais_amd.jpeg + sais_amd.augment): "
                        "same views as the default Pillow loader for the same seed, bit for bit")
    return p


def crop_size(text):
    """A view side the patch-16 backbone trains on: a positive multiple of 16 with 1 + (side / 16)^2 <= 4097 tokens."""
    side = int(text)
    if side < 16 or side % 16 or 1 + (side // 16) ** 2 > MAX_DENSE_TOKENS:
        raise argparse.ArgumentTypeError(f"{text}: a crop size is a positive multiple of 16 of at most {MAX_DENSE_TOKENS} tokens "
                                         f"(at most {16 * math.isqrt(MAX_DENSE_TOKENS - 1)} pixels)")
    return side


def init_distributed(args):
    """utils.init_distributed_mode (utils.py:468-500): torchrun / launch env, else a single process."""
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:
        args.rank, args.world_size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        args.gpu = int(os.environ.get("LOCAL_RANK", args.local_rank))
    else:
        args.rank, args.gpu, args.world_size = 0, 0, 1
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
    torch.cuda.set_device(args.gpu)
    dist.init_process_group("nccl", init_method=args.dist_url, world_size=args.world_size, rank=args.rank,
                            device_id=torch.device("cuda", args.gpu))
    dist.barrier()


AUG_MAX_SIZE = 224          # SAIS_AUG_MAX_SIZE (include/sais_hip.h): the largest view sais_augment_crop_resize makes


def collate(batch):
    crops = [torch.stack([b[0][i] for b in batch]) for i in range(len(batch[0][0]))]
    return crops, [b[1] for b in batch], [b[2] for b in batch]


def build_loader(args, dev):
    """(dataset, sampler, loader, to_device): to_device turns the first element of a batch into the crop list on `dev`.
    Default: DataLoader workers decode and augment with Pillow, the tensors are copied.  --gpu_augment: the workers read
    the files and draw the views' parameters; decode and pixel work happen here, on the GPU, serially with the step."""
    gpu_augment = getattr(args, "gpu_augment", False)
    gsize, lsize = getattr(args, "global_crops_size", 224), getattr(args, "local_crops_size", 96)
    # the GPU augmenter takes its view sizes from the transform's draws, up to the side its kernels hold (SAIS_AUG_MAX_SIZE)
    if gpu_augment and max(gsize, lsize) > AUG_MAX_SIZE:
        sys.exit(f"--gpu_augment makes views of at most {AUG_MAX_SIZE} x {AUG_MAX_SIZE} pixels: use the default Pillow loader for "
                 f"--global_crops_size {gsize} --local_crops_size {lsize}")
    transform = DataAugmentationDINO(args.global_crops_scale, args.local_crops_scale, args.local_crops_number,
                                     seed=args.seed * 1000 + args.rank, global_size=gsize, local_size=lsize)
    dataset = SurgDataset(args.data_path, args.datasets, transform, frames_root=args.frames_root, gpu_augment=gpu_augment)
    sampler = torch.utils.data.DistributedSampler(dataset, num_replicas=args.world_size, rank=args.rank, shuffle=True)
    loader = torch.utils.data.DataLoader(dataset, sampler=sampler, batch_size=args.batch_size_per_gpu,
                                         num_workers=args.num_workers, pin_memory=not gpu_augment, drop_last=True,
                                         collate_fn=collate_raw if gpu_augment else collate)
    if gpu_augment:
        from sais_amd.augment import DinoAugmenter
        from sais_amd.jpeg import JpegDecoder
        decoder, augmenter = JpegDecoder(dev), DinoAugmenter(dev)
        return dataset, sampler, loader, lambda items: gpu_crops(items, decoder, augmenter, dataset.crop_fracs())
    return dataset, sampler, loader, lambda crops: [im.to(dev, non_blocking=True) for im in crops]


def train_dino(args):
    init_distributed(args)
    torch.manual_seed(args.seed)
    main = args.rank == 0
    if args.arch.replace("deit", "vit") != "vit_small" or args.patch_size != 16 or args.optimizer != "adamw" or args.use_bn_in_head:
        raise NotImplementedError("MI355X path: --arch vit_small --patch_size 16 --optimizer adamw --use_bn_in_head false")
    dev = torch.device("cuda", args.gpu)
    dataset, sampler, loader, to_device = build_loader(args, dev)
    if main:
        print(f"Data loaded: there are {len(dataset)} images.")
    student, teacher = dino.build_student_teacher(args.out_dim, args.drop_path_rate, args.norm_last_layer, dev)
    for m in (student, teacher):                                     # DDP's start-up broadcast: every rank = rank 0
        for t in list(m.parameters()) + list(m.buffers()):
            dist.broadcast(t.data, 0)
    dino_loss = dino.DINOLoss(args.out_dim, args.local_crops_number + 2, args.warmup_teacher_temp, args.teacher_temp,
                              args.warmup_teacher_temp_epochs, args.epochs).to(dev)
    optimizer = dino.DINOOptimizer(student, teacher)
    niter = len(loader)
    lr_schedule = dino.cosine_scheduler(args.lr * (args.batch_size_per_gpu * args.world_size) / 256., args.min_lr,
                                        args.epochs, niter, warmup_epochs=args.warmup_epochs)
    wd_schedule = dino.cosine_scheduler(args.weight_decay, args.weight_decay_end, args.epochs, niter)
    momentum_schedule = dino.cosine_scheduler(args.momentum_teacher, 1, args.epochs, niter)
    start_epoch = 0
    ckpt_path = os.path.join(args.output_dir, "checkpoint.pth")
    if os.path.isfile(ckpt_path):                                    # utils.restart_from_checkpoint
        ck = torch.load(ckpt_path, map_location="cpu", weights_only=False)
        with torch.no_grad():                                        # flat buffers exist after one forward
            probe = [torch.zeros(1, 3, args.global_crops_size, args.global_crops_size, device=dev)] * 2
            student(probe), teacher(probe)
        start_epoch = dino.load_checkpoint(ck, student, teacher, optimizer, dino_loss)
        if main:
            print(f"=> resumed from {ckpt_path} at epoch {start_epoch}")
    t_start = time.time()
    if main:
        print("Starting DINO training !")
    for epoch in range(start_epoch, args.epochs):
        sampler.set_epoch(epoch)
        total, count, t0 = torch.zeros((), device=dev), 0, time.time()
        finite = torch.ones((), device=dev)                          # device-side AND of isfinite(loss), every iteration
        for i, (images, _, _) in enumerate(loader):
            it = niter * epoch + i
            images = to_device(images)
            loss, _ = dino.train_step(student, teacher, dino_loss, optimizer, images, it, epoch, lr_schedule, wd_schedule,
                                      momentum_schedule, clip_grad=args.clip_grad, freeze_last_layer=args.freeze_last_layer)
            total += loss
            finite *= torch.isfinite(loss).to(finite.dtype)
            count += 1
            if i % 10 == 0:                                          # the reference logs every 10 iterations
                lv = loss.item()
                if not math.isfinite(lv):
                    print("Loss is {}, stopping training".format(lv))
                    sys.exit(1)
                if main:
                    print(f"Epoch: [{epoch}/{args.epochs}]  [{i}/{niter}]  loss: {lv:.6f}  lr: {lr_schedule[it]:.6f}  "
                          f"wd: {wd_schedule[it]:.6f}  {(time.time() - t0) / (i + 1):.4f} s / it")
        dist.all_reduce(total)
        dist.all_reduce(finite, op=dist.ReduceOp.MIN)
        if finite.item() == 0:                                       # the reference checks every iteration (main_dino.py:540-542);
            print("Loss went non-finite in epoch {}, stopping training".format(epoch))   # here: before checkpoint.pth is
            sys.exit(1)                                              # overwritten with poisoned weights
        stats = {"loss": (total / max(count * args.world_size, 1)).item(), "lr": float(lr_schedule[min(it, len(lr_schedule) - 1)]),
                 "wd": float(wd_schedule[min(it, len(wd_schedule) - 1)])} if count else {}
        if main:
            save = dino.checkpoint_dict(student, teacher, optimizer, dino_loss, epoch + 1, args)
            torch.save(save, ckpt_path)
            if args.saveckp_freq and epoch % args.saveckp_freq == 0:
                torch.save(save, os.path.join(args.output_dir, f"checkpoint{epoch:04}.pth"))
            with open(os.path.join(args.output_dir, "log.txt"), "a") as f:
                f.write(json.dumps({**{f"train_{k}": v for k, v in stats.items()}, "epoch": epoch}) + "\n")
        dist.barrier()
    if main:
        print("Training time {}".format(str(datetime.timedelta(seconds=int(time.time() - t_start)))))
    dist.destroy_process_group()


if __name__ == "__main__":
    args = get_cli_parser().parse_args()
    os.makedirs(args.output_dir, exist_ok=True)
    train_dino(args)
