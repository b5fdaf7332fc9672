#!/usr/bin/env python3
"""Image retrieval on revisited Oxford / Paris with a DINO checkpoint on MI355X — the command line and result lines of the
reference's SAIS/scripts/dino-main/eval_image_retrieval.py, driving sais_amd.retrieval (hand-written gfx950 kernels: the backbone
at every image's own resolution, the bilinear rescaling of --multiscale, and the ranks of the listed positives and junk images
instead of an argsort of the whole database).

    python SAIS/scripts/dino-main/eval_image_retrieval.py --data_path <revisited_paris_oxford root> --dataset roxford5k \
        --pretrained_weights <checkpoint.pth> [--multiscale 1] [--imsize 224]

Kept: every flag, `gnd_<dataset>.pkl`, `img.thumbnail((imsize, imsize), LANCZOS)` + ImageNet normalisation (on Pillow in the
DataLoader workers), batch size 1 (images keep their aspect ratio, so their sizes differ), the Medium / Hard groupings, and the
lines ">> <dataset>: mAP M: .., H: .." and ">> <dataset>: mP@k[ 1  5 10] M: .., H: ..".
Differences: only `--arch vit_small` with `--patch_size 16` or `8` (anything else is refused with a message); without `--pretrained_weights`
the weights stay random and the script says so (no download of the Google-Landmarks checkpoint); one process (WORLD_SIZE > 1
exits, as eval_knn.py here); `--dist_url` / `--local_rank` / `--use_cuda` are accepted and ignored; sides that are no multiple of
16 are cropped at the right and bottom to the multiple below, which is what the reference's patch embedding computes; equal
similarities rank in ascending database index; `--dump_features <dir>` (new) saves the normalised features;
`--gpu_loader true` (new) decodes the files and makes the thumbnails on the GPU (sais_amd/imgfolder.py: the workers only read
the files, `--gpu_loader_batch` of them per decode call), bit-identical to the Pillow loader's, and `--group_shapes true` (new,
with `--gpu_loader true` only) hands the thumbnails of one such batch that share a shape to the backbone together;
`--mixed_batch true` (new, with `--gpu_loader true` only, patch 16, not with `--group_shapes true`) hands ALL thumbnails of one
such batch to the backbone in one segmented pass, whatever their shapes.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from sais_amd import imgfolder, retrieval  # noqa: E402
from sais_amd.model_io import bool_flag, load_dino_backbone  # noqa: E402


def get_args_parser():
    parser = argparse.ArgumentParser('Image Retrieval on revisited Paris and Oxford')
    parser.add_argument('--data_path', default='/path/to/revisited_paris_oxford/', type=str)
    parser.add_argument('--dataset', default='roxford5k', type=str, choices=['roxford5k', 'rparis6k'])
    parser.add_argument('--multiscale', default=False, type=bool_flag)
    parser.add_argument('--imsize', default=224, type=int, help='Image size')
    parser.add_argument('--pretrained_weights', default='', type=str, help="Path to pretrained weights to evaluate.")
    parser.add_argument('--use_cuda', default=True, type=bool_flag,
                        help="Accepted for compatibility: the features always stay on the GPU.")
    parser.add_argument('--arch', default='vit_small', type=str, help='Architecture (vit_small only)')
    parser.add_argument('--patch_size', default=16, type=int, help='Patch resolution of the model (16 or 8).')
    parser.add_argument("--checkpoint_key", default="teacher", type=str,
                        help='Key to use in the checkpoint (example: "teacher")')
    parser.add_argument('--num_workers', default=10, type=int, help='Number of data loading workers per GPU.')
    parser.add_argument("--dist_url", default="env://", type=str, help="Accepted and ignored.")
    parser.add_argument("--local_rank", default=0, type=int, help="Accepted and ignored.")
    parser.add_argument('--dump_features', default=None, help='Directory for trainfeat.pth / queryfeat.pth (normalised features)')
    parser.add_argument('--gpu_loader', default=False, type=bool_flag,
                        help="""Decode the images and make the thumbnails on the GPU (sais_amd/imgfolder.py): the workers only
        read the files.  The images are bit-identical to the Pillow loader's.""")
    parser.add_argument('--gpu_loader_batch', default=64, type=int, help='Files per decode call of --gpu_loader.')
    parser.add_argument('--group_shapes', default=False, type=bool_flag,
                        help="""With --gpu_loader true: thumbnails of one loader batch that share a shape go through the
        backbone together instead of one by one.""")
    parser.add_argument('--mixed_batch', default=False, type=bool_flag,
                        help="""With --gpu_loader true: all thumbnails of one loader batch, whatever their shapes, go through
        the backbone in one segmented pass (patch 16 only; not together with --group_shapes true).""")
    return parser


def main(argv=None):
    args = get_args_parser().parse_args(argv)
    if args.group_shapes and not args.gpu_loader:
        sys.exit("--group_shapes true needs --gpu_loader true: the Pillow loader yields one image per batch")
    if args.mixed_batch and not args.gpu_loader:
        sys.exit("--mixed_batch true needs --gpu_loader true: the Pillow loader yields one image per batch")
    if args.mixed_batch and args.group_shapes:
        sys.exit("--mixed_batch true and --group_shapes true exclude each other: choose one way to batch the thumbnails")
    if args.mixed_batch and args.patch_size != 16:
        sys.exit("--mixed_batch true runs on --patch_size 16 only: the segmented pass is not built for patch 8")
    if args.gpu_loader_batch < 1:
        sys.exit("--gpu_loader_batch must be at least 1")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("eval_image_retrieval.py runs as one process on one GPU: multi-rank feature extraction is not implemented "
                 "(start it without a distributed launcher)")
    if args.arch.replace("deit", "vit") != "vit_small" or args.patch_size not in (16, 8):
        sys.exit(f"Architecture {args.arch} / patch size {args.patch_size} not supported: this path runs --arch vit_small "
                 "--patch_size 16 or 8 only")
    print("\n".join("%s: %s" % (k, str(v)) for k, v in sorted(dict(vars(args)).items())))
    dev = torch.device("cuda:0")

    # ============ preparing data ... ============
    if args.gpu_loader:
        gpu_loader = imgfolder.GpuImageLoader(dev)
        dataset_train = imgfolder.RawOxfordParis(args.data_path, args.dataset, split="train")
        dataset_query = imgfolder.RawOxfordParis(args.data_path, args.dataset, split="query")
        loader = lambda ds: retrieval.ThumbnailBatches(torch.utils.data.DataLoader(
            ds, batch_size=args.gpu_loader_batch, num_workers=args.num_workers, drop_last=False, shuffle=False,
            collate_fn=imgfolder.collate_raw), gpu_loader, args.imsize, args.group_shapes, mixed=args.mixed_batch)
    else:
        dataset_train = retrieval.OxfordParisDataset(args.data_path, args.dataset, split="train", imsize=args.imsize)
        dataset_query = retrieval.OxfordParisDataset(args.data_path, args.dataset, split="query", imsize=args.imsize)
        loader = lambda ds: torch.utils.data.DataLoader(ds, batch_size=1, num_workers=args.num_workers, pin_memory=True,
                                                        drop_last=False, shuffle=False)
    print(f"train: {len(dataset_train)} imgs / query: {len(dataset_query)} imgs")

    # ============ building network ... ============
    print(f"Model {args.arch} {args.patch_size}x{args.patch_size} built.")
    model = load_dino_backbone(args, dev)
    cls = retrieval.cls_features(model)
    fn = (lambda x: retrieval.multi_scale(x, cls)) if args.multiscale else cls

    # Step 1: extract features, normalize
    train_features = retrieval.l2_normalize(retrieval.extract_features(fn, loader(dataset_train), dev))
    query_features = retrieval.l2_normalize(retrieval.extract_features(fn, loader(dataset_query), dev))
    if args.gpu_loader:
        print("gpu loader:", gpu_loader.stats)
    if args.dump_features:
        os.makedirs(args.dump_features, exist_ok=True)
        torch.save(train_features.cpu(), os.path.join(args.dump_features, "trainfeat.pth"))
        torch.save(query_features.cpu(), os.path.join(args.dump_features, "queryfeat.pth"))

    # Step 2: similarity (query x database); Step 3: evaluate from the ranks of the listed images
    sim = retrieval.similarity(query_features, train_features)
    ks = [1, 5, 10]
    (mapM, mprM), (mapH, mprH) = retrieval.evaluate_revisited(sim, dataset_train.gnd, ks)
    print('>> {}: mAP M: {}, H: {}'.format(args.dataset, np.around(mapM * 100, decimals=2), np.around(mapH * 100, decimals=2)))
    print('>> {}: mP@k{} M: {}, H: {}'.format(args.dataset, np.array(ks), np.around(mprM * 100, decimals=2),
                                              np.around(mprH * 100, decimals=2)))


if __name__ == '__main__':
    main()
