#!/usr/bin/env python3
"""Self-attention maps of one image, per head, on MI355X — the command line and output files of the reference's
SAIS/scripts/dino-main/visualize_attention.py, driving VisionTransformer.cls_attention and sais_amd.attnviz (hand-written gfx950
kernels: the CLS row of the last block's softmax at any image size, the mass threshold, colormap + upsampling).

    python SAIS/scripts/dino-main/visualize_attention.py --image_path <image> --output_dir <dir> \
        --pretrained_weights <checkpoint.pth> [--checkpoint_key teacher] [--image_size 480 480] [--threshold 0.6]

Writes <output_dir>/img.png (the input as the network saw it, rescaled to its own range), attn-head<j>.png for the six heads
(matplotlib's default colormap, viridis, each map normalised on its own) and, with --threshold t, mask_th<t>_head<j>.png.

Decisions where this script differs from the reference:
  * --image_path is required.  The reference downloads a default image when it is missing; this script never touches the network.
  * Masks.  The reference draws each thresholded map over the image with display_instances (skimage contours, a random colour per
    call).  skimage is not a dependency and random colours cannot be compared: mask_th<t>_head<j>.png is the plain binary
    mask, white where the head keeps its attention mass, upsampled x 16.  Equal attention values are ordered by index (the
    stable rule); the reference's torch.sort leaves that order unspecified.
  * img.png is make_grid(normalize=True, scale_each=True) + save_image's arithmetic for one image, written by Pillow
    (torchvision is not a dependency); attn-head<j>.png is written by Pillow with the keywords plt.imsave passes on, and equals
    plt.imsave's file byte for byte when matplotlib is installed (its Software text chunk names matplotlib's version: without
    matplotlib the chunk is left out and viridis comes from the bundled table).
  * --image_size is Pillow's bilinear filter on the decoded image under torchvision's size rule (one int: the short side; two:
    h w); torchvision's Resize antialiases: this step is PARITY-UNPINNED.
  * Checkpoints.  Loaded as eval_knn.py does; without --pretrained_weights the weights stay random (seeded: the same in every
    run) and the script says so.  No download.  Only --arch vit_small with --patch_size 16 or 8; --patch_size defaults to 16 (the
    reference's default is 8: ViT-S/8, inference only here).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from sais_amd import attnviz  # noqa: E402


def get_args_parser():
    parser = argparse.ArgumentParser("Visualize Self-Attention maps")
    parser.add_argument("--arch", default="vit_small", type=str, choices=["vit_tiny", "vit_small", "vit_base"],
                        help="backbone (this path: vit_small only)")
    parser.add_argument("--patch_size", default=16, type=int, help="patch size of the backbone (this path: 16 or 8)")
    parser.add_argument("--pretrained_weights", default="", type=str, help="checkpoint file of the backbone")
    parser.add_argument("--checkpoint_key", default="teacher", type=str, help="entry of the checkpoint dict that holds the weights")
    parser.add_argument("--image_path", required=True, type=str, help="the image to visualise")
    parser.add_argument("--image_size", default=(480, 480), type=int, nargs="+", help="resize the image first: SHORT_SIDE, or H W")
    parser.add_argument("--output_dir", default=".", help="where the PNG files go")
    parser.add_argument("--threshold", type=float, default=None,
                        help="also write the masks that keep this share of each head's attention mass, in (0, 1)")
    return parser


@torch.no_grad()
def main(argv=None, dev=None):
    args = get_args_parser().parse_args(argv)
    if not os.path.isfile(args.image_path):
        print(f"Provided image path {args.image_path} is non valid.")
        sys.exit(1)
    dev = torch.device("cuda:0") if dev is None else dev
    model = attnviz.build_model(args, dev)
    img = attnviz.load_frame(args.image_path, list(args.image_size), args.patch_size)
    h, w = img.shape[1] // args.patch_size, img.shape[2] // args.patch_size
    probs = model.cls_attention(img[None].to(dev))
    os.makedirs(args.output_dir, exist_ok=True)
    attnviz.save_image_png(os.path.join(args.output_dir, "img.png"), attnviz.input_image_u8(img.numpy()))
    for j in range(probs.shape[1]):
        fname = os.path.join(args.output_dir, f"attn-head{j}.png")
        _, rgb = attnviz.render(probs, (h, w), heads=j, cmap="viridis", patch=args.patch_size)
        attnviz.save_png(fname, rgb[0])
        print(f"{fname} saved.")
    if args.threshold is not None:
        keep = attnviz.mass_mask(probs, args.threshold)[0].view(-1, h, w).cpu()
        for j in range(keep.shape[0]):
            fname = os.path.join(args.output_dir, f"mask_th{args.threshold}_head{j}.png")
            attnviz.save_mask_png(fname, keep[j], args.patch_size)
            print(f"{fname} saved.")


if __name__ == "__main__":
    main()
