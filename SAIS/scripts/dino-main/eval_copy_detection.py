#!/usr/bin/env python3
"""Copy detection on Copydays with a DINO checkpoint on MI355X — the command line and result lines of the reference's
SAIS/scripts/dino-main/eval_copy_detection.py, driving sais_amd.retrieval (hand-written gfx950 kernels: the CLS | GeM descriptor
without the normed token tensor, exact-f32 whitening statistics, a top-20 search without the similarity matrix).

    python SAIS/scripts/dino-main/eval_copy_detection.py --data_path <copydays root> --pretrained_weights <checkpoint.pth> \
        [--whitening_path <dir>] [--distractors_path <dir>] [--imsize 320]

Kept: every flag, the block order of CopydaysDataset, `Resize((imsize, imsize), bicubic)` + ImageNet normalisation (on Pillow in
the DataLoader workers), the optional distractors and whitening sets, the printed lines ("Extraction of ... features done.
Shape: ...", "Using distractors...", "keeping .. % of the energy", "eval on <block> mAP=..").
Differences: only `--arch vit_small` with `--patch_size 16` or `8` (the defaults here; anything else is refused with a message); without
`--pretrained_weights` the weights stay random and the script says so (no download); one process (WORLD_SIZE > 1 exits, as
eval_knn.py here); `--dist_url` / `--local_rank` / `--use_cuda` are accepted and ignored; the block sizes come from the directory
listing (157 per block and 229 for `strong` on the real data, which the reference hard-codes), blocks that are absent are left
out; directory listings of distractors and whitening images are sorted; an `--imsize` that is no multiple of 16 is cropped at the
right and bottom to the multiple below, which is what the reference's patch embedding computes; a database smaller than 20 images
is searched to its size; `--dump_features <dir>` (new) saves the final query and database descriptors.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from sais_amd import imgfolder, retrieval  # noqa: E402
from sais_amd.model_io import bool_flag, load_dino_backbone  # noqa: E402


def get_args_parser():
    parser = argparse.ArgumentParser('Copy detection on Copydays')
    parser.add_argument('--data_path', default='/path/to/copydays/', type=str,
                        help="See https://lear.inrialpes.fr/~jegou/data.php#copydays")
    parser.add_argument('--whitening_path', default='/path/to/whitening_data/', type=str,
                        help="""Path to directory with images used for computing the whitening operator.
        In the paper: 20k random images from YFCC100M.""")
    parser.add_argument('--distractors_path', default='/path/to/distractors/', type=str,
                        help="Path to directory with distractors images. In the paper: 10k random images from YFCC100M.")
    parser.add_argument('--imsize', default=320, type=int, help='Image size (square image)')
    parser.add_argument('--batch_size_per_gpu', default=16, type=int, help='Per-GPU batch-size')
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
    parser.add_argument('--dump_features', default=None, help='Directory for queries.pth / database.pth (final descriptors)')
    return parser


def get_cli_parser():
    """The command line: the reference's flags (get_args_parser) + switches of this implementation only."""
    parser = argparse.ArgumentParser('Copy detection on Copydays', parents=[get_args_parser()],
                                     conflict_handler='resolve')          # -h comes with the parent
    parser.add_argument('--gpu_loader', default=False, type=bool_flag,
                        help="""Decode and transform the images on the GPU (sais_amd/imgfolder.py): the workers only read the
        files.  The batches are bit-identical to the Pillow loader's.""")
    return parser


_gpu_loader = {}                                                   # device -> the GpuImageLoader of --gpu_loader (its buffers are reused)


def extract(image_list, model, args, dev):
    if getattr(args, "gpu_loader", False):
        if dev not in _gpu_loader:
            _gpu_loader[dev] = imgfolder.GpuImageLoader(dev)
        loader = imgfolder.GpuBatches(torch.utils.data.DataLoader(
            imgfolder.RawImgList(image_list), batch_size=args.batch_size_per_gpu, num_workers=args.num_workers, drop_last=False,
            shuffle=False, collate_fn=imgfolder.collate_raw), lambda items: _gpu_loader[dev].square(items, args.imsize))
        return retrieval.extract_features(retrieval.descriptor_features(model), loader, dev)
    ds = retrieval.ImgListDataset(image_list, args.imsize)
    loader = torch.utils.data.DataLoader(ds, batch_size=args.batch_size_per_gpu, num_workers=args.num_workers, drop_last=False,
                                         shuffle=False)
    return retrieval.extract_features(retrieval.descriptor_features(model), loader, dev)


def main(argv=None):
    args = get_cli_parser().parse_args(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("eval_copy_detection.py runs as one process on one GPU: multi-rank feature extraction is not implemented "
                 "(start it without a distributed launcher)")
    if args.arch.replace("deit", "vit") != "vit_small" or args.patch_size not in (16, 8):
        sys.exit(f"Architecture {args.arch} / patch size {args.patch_size} not supported: this path runs --arch vit_small "
                 "--patch_size 16 or 8 only")
    print("\n".join("%s: %s" % (k, str(v)) for k, v in sorted(dict(vars(args)).items())))
    dev = torch.device("cuda:0")
    print(f"Model {args.arch} {args.patch_size}x{args.patch_size} built.")
    model = load_dino_backbone(args, dev)

    blocks = retrieval.copydays_blocks(args.data_path)
    paths = lambda name, files: [os.path.join(args.data_path, name, f) for f in files]

    # ============ Extract features ... ============
    queries = torch.cat([extract(paths(name, files), model, args, dev) for name, files in blocks])
    print(f"Extraction of queries features done. Shape: {queries.shape}")
    database = [extract(paths(*blocks[0]), model, args, dev)]
    if os.path.isdir(args.distractors_path):
        print("Using distractors...")
        database.append(extract(retrieval.list_images(args.distractors_path), model, args, dev))
    database = torch.cat(database)
    print(f"Extraction of database and distractors features done. Shape: {database.shape}")

    # ============ Whitening ... ============
    if os.path.isdir(args.whitening_path):
        print(f"Extracting features on images from {args.whitening_path} for learning the whitening operator.")
        features_for_whitening = extract(retrieval.list_images(args.whitening_path), model, args, dev)
        pca = retrieval.PCAWhitening(dim=database.shape[-1], whit=0.5).fit(features_for_whitening)
        database, queries = pca.apply(database), pca.apply(queries)          # centre, whiten, l2 normalize
    else:
        database, queries = retrieval.l2_normalize(database), retrieval.l2_normalize(queries)

    # ============ Copy detection ... ============
    if args.dump_features:
        os.makedirs(args.dump_features, exist_ok=True)
        torch.save(queries.cpu(), os.path.join(args.dump_features, "queries.pth"))
        torch.save(database.cpu(), os.path.join(args.dump_features, "database.pth"))
    distances, indices = retrieval.copy_detection_topk(queries, database, 20)
    for name, m in retrieval.copydays_map(indices.cpu().numpy(), blocks):
        print("eval on %s mAP=%.3f" % (name, m))


if __name__ == '__main__':
    main()
