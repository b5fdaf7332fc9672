#!/usr/bin/env python3
"""DAVIS-style video object segmentation with frozen DINO patch features on MI355X — the command line and directory layout
of the reference's SAIS/scripts/dino-main/eval_video_segmentation.py, driving VisionTransformer.dense_features and
sais_amd.vos (hand-written gfx950 kernels: streaming attention at 1561 tokens, label propagation without the affinity
matrix, upsampling + argmax).

    python SAIS/scripts/dino-main/eval_video_segmentation.py --data_path <davis root> --output_dir <dir> \
        --pretrained_weights <output_dir>/checkpoint.pth [--checkpoint_key teacher] [--n_last_frames 7] \
        [--size_mask_neighborhood 12] [--topk 5] [--bs 6]

Reads <data_path>/ImageSets/2017/val.txt, <data_path>/JPEGImages/480p/<video>/*.jpg and the first annotation
<data_path>/Annotations/480p/<video>/<first frame>.png; writes <output_dir>/<video>/<frame>.png, indexed PNGs of the
frames' original size (the first one is the annotation itself).  Scoring (J&F) is left to the DAVIS toolkit, as in the reference.

Decisions where this script differs from the reference:
  * Network.  The reference downloads its colour palette with urlopen.  This script takes the palette of the first annotation
    PNG of each video (Image.getpalette()) and never touches the network.
  * Frame reading.  cv2 is not a dependency: frames are read with Pillow and resized (bilinear) to the reference's (th, tw)
    rule (:197-214: short side 480, long side floored to a multiple of 64), normalised with the reference's constants, its
    std of 0.228 for red included (:244).  Pillow's filter is not cv2.resize's: this step is PARITY-UNPINNED.
  * --bs.  The reference parses it and ignores it.  Features do not depend on the propagation, so this script extracts the
    dense features of --bs frames per ViT pass and then propagates frame by frame.
  * Checkpoints.  Loaded as eval_knn.py does (sais_amd.model_io.load_dino_backbone); without --pretrained_weights the weights stay
    random (seeded: the same in every run) and the script says so (no download).  Only --arch vit_small, --patch_size 16 or 8.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from sais_amd import vos  # noqa: E402
from sais_amd.model_io import load_dino_backbone  # noqa: E402


def get_args_parser():
    parser = argparse.ArgumentParser('Evaluation with video object segmentation on DAVIS 2017')
    parser.add_argument('--pretrained_weights', default='', type=str, help="Path to pretrained weights to evaluate.")
    parser.add_argument('--arch', default='vit_small', type=str, help='Architecture (vit_small only).')
    parser.add_argument('--patch_size', default=16, type=int, help='Patch resolution of the model.')
    parser.add_argument("--checkpoint_key", default="teacher", type=str, help='Key to use in the checkpoint (example: "teacher")')
    parser.add_argument('--output_dir', default=".", help='Path where to save segmentations')
    parser.add_argument('--data_path', default='/path/to/davis/', type=str)
    parser.add_argument("--n_last_frames", type=int, default=7, help="number of preceeding frames")
    parser.add_argument("--size_mask_neighborhood", default=12, type=int,
                        help="We restrict the set of source nodes considered to a spatial neighborhood of the query node")
    parser.add_argument("--topk", type=int, default=5, help="accumulate label from top k neighbors")
    parser.add_argument("--bs", type=int, default=6, help="Frames per ViT pass, try to reduce if OOM")
    return parser


def build_model(args, dev):
    print(f"Model {args.arch} {args.patch_size}x{args.patch_size} built.")
    return load_dino_backbone(args, dev, seed=0, freeze=True)


@torch.no_grad()
def extract_features(model, frame_list, bs, dev):
    """Patch features f32 [frames, h w, 384] on the device (extract_feature, :153-163: the CLS token is dropped), --bs frames per
    pass; also (h, w) and the frames' original (height, width)."""
    feats, sizes = [], []
    for i in range(0, len(frame_list), max(1, bs)):
        frames = [vos.read_frame(p) for p in frame_list[i:i + max(1, bs)]]
        sizes += [(oh, ow) for _, oh, ow in frames]
        x = torch.stack([f for f, _, _ in frames]).to(dev)
        feats.append(model.dense_features(x, 1)[0][:, 1:].contiguous())
    feats = torch.cat(feats)
    patch = model.patch_embed.patch_size
    return feats, x.shape[2] // patch, x.shape[3] // patch, sizes


@torch.no_grad()
def eval_video_tracking_davis(args, model, frame_list, video_dir, first_seg, seg_ori, color_palette, dev):
    """eval_video_tracking_davis (:38-82)."""
    from PIL import Image
    video_folder = os.path.join(args.output_dir, video_dir.rstrip("/").split('/')[-1])
    os.makedirs(video_folder, exist_ok=True)
    feats, h, w, sizes = extract_features(model, frame_list, args.bs, dev)
    vos.imwrite_indexed(os.path.join(video_folder, "00000.png"), seg_ori, color_palette)
    prop = vos.LabelPropagator(feats[0], first_seg[0].to(dev), h, w, args.n_last_frames, args.size_mask_neighborhood, args.topk)
    for cnt in range(1, len(frame_list)):
        seg = prop.step(feats[cnt])
        labels = vos.upsample_argmax(seg, args.patch_size).cpu().numpy()
        ori_h, ori_w = sizes[cnt]
        labels = np.array(Image.fromarray(labels).resize((ori_w, ori_h), 0))
        frame_nm = frame_list[cnt].split('/')[-1].replace(".jpg", ".png")
        vos.imwrite_indexed(os.path.join(video_folder, frame_nm), labels, color_palette)


def main(argv=None):
    args = get_args_parser().parse_args(argv)
    print("\n".join("%s: %s" % (k, str(v)) for k, v in sorted(dict(vars(args)).items())))
    dev = torch.device("cuda:0")
    model = build_model(args, dev)
    video_list = open(os.path.join(args.data_path, "ImageSets/2017/val.txt")).readlines()
    for i, video_name in enumerate(video_list):
        video_name = video_name.strip()
        if not video_name:
            continue
        print(f'[{i}/{len(video_list)}] Begin to segmentate video {video_name}.')
        video_dir = os.path.join(args.data_path, "JPEGImages/480p/", video_name)
        frame_list = vos.read_frame_list(video_dir)
        seg_path = frame_list[0].replace("JPEGImages", "Annotations").replace("jpg", "png")
        first_seg, seg_ori, palette = vos.read_seg(seg_path, args.patch_size)
        eval_video_tracking_davis(args, model, frame_list, video_dir, first_seg, seg_ori, palette, dev)


if __name__ == '__main__':
    main()
