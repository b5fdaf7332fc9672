#!/usr/bin/env python3
"""Weighted k-NN evaluation of a DINO checkpoint on MI355X — the command line, result lines and feature dump files of the
reference's SAIS/scripts/dino-main/eval_knn.py, driving sais_amd.knn (hand-written gfx950 kernels: no similarity matrix in
memory, one search for every k of --nb_knn).

    python SAIS/scripts/dino-main/eval_knn.py --data_path <root with train/ and val/ class folders> \
        --pretrained_weights <output_dir>/checkpoint.pth [--checkpoint_key teacher] [--nb_knn 10 20 100 200]

Kept: every flag, `ImageFolder` listing rules, the eval transform (Resize 256 bicubic, CenterCrop 224, ImageNet
normalisation; on Pillow in the DataLoader workers), `--checkpoint_key` and the `module.` / `backbone.` prefix handling,
the four `--dump_features` / `--load_features` files, and the line "{k}-NN classifier result: Top1: .., Top5: ..".
Differences: only `--arch vit_small` with `--patch_size 16` or `8`; without `--pretrained_weights` the weights stay random and the
script says so (no download); one process (WORLD_SIZE > 1 exits); `--dist_url` / `--local_rank` are accepted and
ignored; a k larger than the train set is reported and skipped; any number of test rows works.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from sais_amd import imgfolder, knn  # noqa: E402
from sais_amd.model_io import bool_flag, load_dino_backbone  # noqa: E402


def get_args_parser():
    parser = argparse.ArgumentParser('Evaluation with weighted k-NN on ImageNet')
    parser.add_argument('--batch_size_per_gpu', default=128, type=int, help='Per-GPU batch-size')
    parser.add_argument('--nb_knn', default=[10, 20, 100, 200], nargs='+', type=int,
                        help='Number of NN to use. 20 is usually working the best.')
    parser.add_argument('--temperature', default=0.07, type=float, help='Temperature used in the voting coefficient')
    parser.add_argument('--pretrained_weights', default='', type=str, help="Path to pretrained weights to evaluate.")
    parser.add_argument('--use_cuda', default=True, type=bool_flag,
                        help="Accepted for compatibility: the features always stay on the GPU.")
    parser.add_argument('--arch', default='vit_small', type=str, help='Architecture')
    parser.add_argument('--patch_size', default=16, type=int, help='Patch resolution of the model.')
    parser.add_argument("--checkpoint_key", default="teacher", type=str,
                        help='Key to use in the checkpoint (example: "teacher")')
    parser.add_argument('--dump_features', default=None, help='Path where to save computed features, empty for no saving')
    parser.add_argument('--load_features', default=None,
                        help="If the features have already been computed, where to find them.")
    parser.add_argument('--num_workers', default=10, type=int, help='Number of data loading workers per GPU.')
    parser.add_argument("--dist_url", default="env://", type=str, help="Accepted and ignored.")
    parser.add_argument("--local_rank", default=0, type=int, help="Accepted and ignored.")
    parser.add_argument('--data_path', default='/path/to/imagenet/', type=str)
    return parser


def get_cli_parser():
    """The command line: the reference's flags (get_args_parser) + switches of this implementation only."""
    parser = argparse.ArgumentParser('Evaluation with weighted k-NN on ImageNet', parents=[get_args_parser()],
                                     conflict_handler='resolve')          # -h comes with the parent
    parser.add_argument('--gpu_loader', default=False, type=bool_flag,
                        help="""Decode and transform the images on the GPU (sais_amd/imgfolder.py): the workers only read the
        files.  The batches are bit-identical to the Pillow loader's.""")
    return parser


def build_model(args, dev):
    print(f"Model {args.arch} {args.patch_size}x{args.patch_size} built.")
    return load_dino_backbone(args, dev)


def extract_feature_pipeline(args, dev):
    loaders = []
    gpu_loader = imgfolder.GpuImageLoader(dev) if getattr(args, "gpu_loader", False) else None
    for part in ("train", "val"):
        if gpu_loader is not None:
            ds = imgfolder.RawEvalFolder(os.path.join(args.data_path, part))
            loaders.append(imgfolder.GpuBatches(torch.utils.data.DataLoader(
                ds, batch_size=args.batch_size_per_gpu, num_workers=args.num_workers, drop_last=False, shuffle=False,
                collate_fn=imgfolder.collate_raw), gpu_loader.eval))
            continue
        ds = knn.EvalImageFolder(os.path.join(args.data_path, part))
        loaders.append(torch.utils.data.DataLoader(ds, batch_size=args.batch_size_per_gpu, num_workers=args.num_workers,
                                                   pin_memory=True, drop_last=False, shuffle=False))
    print(f"Data loaded with {len(loaders[0].dataset)} train and {len(loaders[1].dataset)} val imgs.")
    model = build_model(args, dev)
    print("Extracting features for train set...")
    train_features = knn.extract_features(model, loaders[0], dev)
    print("Extracting features for val set...")
    test_features = knn.extract_features(model, loaders[1], dev)
    train_features = torch.nn.functional.normalize(train_features, dim=1, p=2)
    test_features = torch.nn.functional.normalize(test_features, dim=1, p=2)
    train_labels = torch.tensor([s[-1] for s in loaders[0].dataset.samples]).long()
    test_labels = torch.tensor([s[-1] for s in loaders[1].dataset.samples]).long()
    if args.dump_features:
        os.makedirs(args.dump_features, exist_ok=True)
        torch.save(train_features.cpu(), os.path.join(args.dump_features, "trainfeat.pth"))
        torch.save(test_features.cpu(), os.path.join(args.dump_features, "testfeat.pth"))
        torch.save(train_labels.cpu(), os.path.join(args.dump_features, "trainlabels.pth"))
        torch.save(test_labels.cpu(), os.path.join(args.dump_features, "testlabels.pth"))
    return train_features, test_features, train_labels, test_labels


def main(argv=None):
    args = get_cli_parser().parse_args(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("eval_knn.py runs as one process on one GPU: multi-rank feature extraction is not implemented "
                 "(start it without a distributed launcher)")
    print("\n".join("%s: %s" % (k, str(v)) for k, v in sorted(dict(vars(args)).items())))
    dev = torch.device("cuda:0")
    if args.load_features:
        load = lambda n: torch.load(os.path.join(args.load_features, n), map_location="cpu")
        train_features, test_features = load("trainfeat.pth"), load("testfeat.pth")
        train_labels, test_labels = load("trainlabels.pth"), load("testlabels.pth")
    else:
        train_features, test_features, train_labels, test_labels = extract_feature_pipeline(args, dev)
    train_features, test_features = train_features.to(dev), test_features.to(dev)
    train_labels, test_labels = train_labels.to(dev), test_labels.to(dev)

    print("Features are ready!\nStart the k-NN classification.")
    nt = train_features.shape[0]
    ks = []
    for k in args.nb_knn:
        if k > nt or k > knn.MAX_K or k < 1:
            print(f"{k}-NN classifier skipped: k must be in [1, {min(nt, knn.MAX_K)}] ({nt} train images)")
        else:
            ks.append(k)
    if ks:
        num_classes = max(1000, int(train_labels.max()) + 1)
        index = knn.KnnIndex(train_features, train_labels, num_classes)
        for k, (top1, top5) in zip(ks, knn.knn_classifier(index, None, test_features, test_labels, ks, args.temperature)):
            print(f"{k}-NN classifier result: Top1: {top1}, Top5: {top5}")


if __name__ == '__main__':
    main()
