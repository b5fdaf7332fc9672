#!/usr/bin/env python3
"""Self-attention heat maps of video frames, and the video made of them, on MI355X — the command line and folder layout of the
reference's SAIS/scripts/dino-main/video_generation.py (the DINO script the SAIS author edited: the thresholded maps are
multiplied into the attention, :229), driving VisionTransformer.cls_attention and sais_amd.attnviz (hand-written gfx950 kernels:
the CLS row of the last block's softmax at any frame size, the mass threshold, the head mean + colormap + upsampling).

    python SAIS/scripts/dino-main/video_generation.py --input_path <folder of *.jpg | video file> --output_path <dir> \
        --pretrained_weights <checkpoint.pth> [--checkpoint_key teacher] [--threshold 0.6] \
        [--resize 480 | --resize 480 848] [--bs 8] [--fps 30] [--video_format mp4] [--video_only]

A folder of frames gives <output_path>/attention/attn-<name>.jpg for every <name>.jpg, in sorted order, then
<output_path>/video.<fmt>; a video file is first split into <output_path>/frames/frame-NNNN.jpg.

Decisions where this script differs from the reference:
  * cv2 is not a dependency.  It is imported only where a video container is read or written.  Without it a video-file input
    exits with a message, and a folder input writes the attention frames and says that the video was not assembled (and
    --video_only has nothing it can do).  With it, frame extraction and the video.<fmt> assembly are the reference's.
  * --bs (new): frames per ViT pass.  Consecutive frames of equal size share a pass; the reference runs one frame at a time.
  * Arithmetic.  The attention is the CLS row only (no [6, N, N] tensor); mass threshold, head mean, normalisation, colormap and
    nearest upsampling run on the device, and so does the JPEG encode (sais_amd.jpeg_enc: the file Pillow writes with the
    keywords plt.imsave passes on, one batch per call): given the same attention the file is the reference's byte for byte
    (tests/test_attnviz_gpu.py, tests/test_jpeg_enc_gpu.py).  matplotlib is optional (the `inferno`
    table is bundled).  Equal attention values are ordered by index (the stable rule); the reference's torch.sort leaves that
    order unspecified.
  * --resize is Pillow's bilinear filter on the decoded image under torchvision's size rule (one int: the short side; two:
    h w), not torchvision's antialiased tensor resize: this step is PARITY-UNPINNED.
  * Checkpoints.  Loaded as eval_knn.py does; without --pretrained_weights the weights stay random (seeded: the same in every
    run) and the script says so.  No download.  Only --arch vit_small with --patch_size 16 or 8; --patch_size defaults to 16 (the
    reference's default is 8: ViT-S/8, inference only here).
"""
import argparse
import glob
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from sais_amd import attnviz  # noqa: E402

NO_CV2_VIDEO_IN = "cv2 (opencv-python) is not installed: a video file cannot be read. Extract the frames to a folder of *.jpg " \
                  "and pass that folder as --input_path."
NO_CV2_VIDEO_OUT = "cv2 (opencv-python) is not installed: the attention frames are written, the video was not assembled."


def import_cv2():
    try:
        import cv2
    except ImportError:
        return None
    return cv2


def extract_frames(cv2, video, folder):
    """Every frame of a video file as <folder>/frame-NNNN.jpg (the reference's names) -> the container's frame rate."""
    cap = cv2.VideoCapture(video)
    fps = cap.get(cv2.CAP_PROP_FPS)
    print(f"Video: {video} ({fps} fps)")
    print(f"Extracting frames to {folder}")
    count = 0
    while True:
        ok, bgr = cap.read()
        if not ok:
            break
        cv2.imwrite(os.path.join(folder, f"frame-{count:04}.jpg"), bgr)
        count += 1
    cap.release()
    return fps


def assemble_video(cv2, files, path, fps, fmt):
    """The attention JPEGs `files`, in order, as one mp4 (MP4V) or avi (XVID) file."""
    import numpy as np
    from PIL import Image
    writer = None
    for name in files:
        with Image.open(name) as im:
            rgb = np.array(im.convert("RGB"))
        if writer is None:
            size = (rgb.shape[1], rgb.shape[0])
            print(f"Generating video {size} to {path}")
            writer = cv2.VideoWriter(path, cv2.VideoWriter_fourcc(*{"mp4": "MP4V", "avi": "XVID"}[fmt]), fps, size)
        writer.write(cv2.cvtColor(rgb, cv2.COLOR_RGB2BGR))
    if writer is not None:
        writer.release()
    print("Done")


class VideoGenerator:
    def __init__(self, args, dev=None):
        self.args, self.dev, self.model = args, dev, None

    def run(self):
        a = self.args
        if a.input_path is None or not os.path.exists(a.input_path):
            print(f"Provided input path {a.input_path} doesn't exists.")
            sys.exit(1)
        cv2 = import_cv2()
        if a.video_only:                              # --input_path is the folder of attention images; no model is needed
            self._video(cv2, a.input_path)
            return
        frames_folder = a.input_path
        if os.path.isfile(a.input_path):
            if cv2 is None:
                print(NO_CV2_VIDEO_IN)
                sys.exit(1)
            frames_folder = os.path.join(a.output_path, "frames")
            os.makedirs(frames_folder, exist_ok=True)
            a.fps = extract_frames(cv2, a.input_path, frames_folder)
        attention_folder = os.path.join(a.output_path, "attention")
        os.makedirs(attention_folder, exist_ok=True)
        self.dev = torch.device("cuda:0") if self.dev is None else self.dev
        self.model = attnviz.build_model(a, self.dev)
        self._inference(frames_folder, attention_folder)
        self._video(cv2, attention_folder)

    def _video(self, cv2, folder):
        if cv2 is None:
            print(NO_CV2_VIDEO_OUT)
            return
        a = self.args
        assemble_video(cv2, sorted(glob.glob(os.path.join(folder, "attn-*.jpg"))),
                       os.path.join(a.output_path, "video." + a.video_format), a.fps, a.video_format)

    @torch.no_grad()
    def _inference(self, inp, out):
        print(f"Generating attention images to {out}")
        paths = sorted(glob.glob(os.path.join(inp, "*.jpg")))
        load = lambda path: attnviz.load_frame(path, self.args.resize, self.args.patch_size)
        bs, i, nxt = max(1, self.args.bs), 0, None
        while i < len(paths):
            batch, nxt = [load(paths[i]) if nxt is None else nxt], None
            while len(batch) < bs and i + len(batch) < len(paths):           # consecutive frames of equal size share a pass
                nxt = load(paths[i + len(batch)])
                if nxt.shape != batch[0].shape:
                    break                                                    # (it opens the next pass)
                batch.append(nxt)
                nxt = None
            x = torch.stack(batch).to(self.dev)
            probs = self.model.cls_attention(x)
            _, rgb = attnviz.render(probs, (x.shape[2] // self.args.patch_size, x.shape[3] // self.args.patch_size), threshold=self.args.threshold, cmap="inferno",
                                    patch=self.args.patch_size)
            attnviz.save_jpegs([os.path.join(out, "attn-" + os.path.basename(paths[i + j])) for j in range(len(batch))], rgb)
            i += len(batch)


def get_args_parser():
    parser = argparse.ArgumentParser("Generation self-attention video")
    parser.add_argument("--arch", default="vit_small", type=str, choices=["vit_tiny", "vit_small", "vit_base"],
                        help="backbone (this path: vit_small only)")
    parser.add_argument("--patch_size", default=16, type=int, help="patch size of the backbone (this path: 16 or 8)")
    parser.add_argument("--pretrained_weights", default="", type=str, help="checkpoint file of the backbone")
    parser.add_argument("--checkpoint_key", default="teacher", type=str, help="entry of the checkpoint dict that holds the weights")
    parser.add_argument("--input_path", required=True, type=str,
                        help="a video file, a folder of frames (*.jpg), or with --video_only a folder of attention images")
    parser.add_argument("--output_path", default="./", type=str, help="where frames/, attention/ and video.<fmt> go")
    parser.add_argument("--threshold", type=float, default=0.6, help="share of the attention mass the maps keep, in (0, 1)")
    parser.add_argument("--resize", default=None, type=int, nargs="+", help="resize the frames first: SHORT_SIDE, or H W")
    parser.add_argument("--video_only", action="store_true", help="only assemble video.<fmt> from attention images")
    parser.add_argument("--fps", default=30.0, type=float, help="frame rate of the output video (a video input sets it)")
    parser.add_argument("--video_format", default="mp4", type=str, choices=["mp4", "avi"], help="container of the output video")
    parser.add_argument("--bs", default=8, type=int, help="frames per ViT pass (consecutive frames of equal size share a pass)")
    return parser


def main(argv=None):
    args = get_args_parser().parse_args(argv)
    VideoGenerator(args).run()


if __name__ == "__main__":
    main()
