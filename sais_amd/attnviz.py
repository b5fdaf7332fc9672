"""Attention-map rendering (dino-main/video_generation.py, visualize_attention.py) on the HIP kernels of csrc/attnviz.hip.

`VisionTransformer.cls_attention` gives the CLS row of the last block's softmax, f32 [F, 6, 1 + hw], at any frame size.  Here:
`mass_mask` is the scripts' "keep xx% of the mass" block (video_generation.py:197-205) without sort / cumsum / argsort / the head
loop, `render` their tail (:207-241) — the masked head mean, min / max normalisation, the colormap and the nearest x patch
upsampling — as one heat map at patch resolution and one colour image per frame.  There is no CPU fallback: host tensors raise.
The image writers (`save_jpeg`, `save_png`: Pillow with the keywords plt.imsave passes on, so the files equal plt.imsave's byte
for byte; `save_jpegs`: the same JPEG files for a batch on the device, encoded there by sais_amd.jpeg_enc) and the frame loading of the two command-line scripts live here too; matplotlib is optional.
"""
import numpy as np
import torch

from . import ops
from .model_io import load_dino_backbone

MAX_N, RENDER_WS_FLOATS = 4096, 32                  # SAIS_ATTN_MASK_MAX_N, SAIS_ATTN_RENDER_WS_FLOATS
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # video_generation.py:163-165, visualize_attention.py:168
_LUTS = {}
_ENCODERS = {}                                     # device -> JpegEncoder (save_jpegs)


def _probs(probs):
    if not isinstance(probs, torch.Tensor) or not probs.is_cuda:
        raise ValueError("probs: expected a device tensor (the rendering path has no CPU fallback)")
    if probs.dim() != 3 or probs.dtype != torch.float32 or probs.shape[2] < 2 or probs.stride(2) != 1 or \
            (probs.shape[0] > 1 and probs.stride(0) != probs.shape[1] * probs.stride(1)):    # row = frame * heads + head
        raise ValueError(f"probs: expected f32 [F, heads, 1 + hw] as cls_attention returns it, got {tuple(probs.shape)} {probs.dtype}")
    if probs.shape[2] - 1 > MAX_N:
        raise ValueError(f"{probs.shape[2] - 1} patches: at most {MAX_N}")
    return probs[:, :, 1:]                        # "we keep only the output patch attention" (:195): a strided view, no copy


@torch.no_grad()
def mass_mask(probs, threshold):
    """probs f32 [F, heads, 1 + hw] on the device (cls_attention's output) -> keep u8 [F, heads, hw]: per (frame, head), the patch
    tokens that hold the top `threshold` share of the patch attention's mass — ascending stable order, kept iff the inclusive
    cumulative share is > 1 - threshold (video_generation.py:197-205)."""
    p = _probs(probs)
    threshold = float(threshold)
    if not 0.0 < threshold < 1.0:
        raise ValueError(f"threshold = {threshold} must be in (0, 1)")
    F, nh, n = p.shape
    keep = torch.empty(F, nh, n, dtype=torch.uint8, device=p.device)
    ops.attn_mass_mask(p, F * nh, n, threshold, keep)
    return keep


def _head_range(heads, nh):
    if heads is None:
        return 0, nh
    if isinstance(heads, int):
        head0, nheads = heads, 1
    else:
        hs = [int(h) for h in heads]
        if not hs or hs != list(range(hs[0], hs[0] + len(hs))):
            raise ValueError(f"heads = {heads}: one head or a run of consecutive heads")
        head0, nheads = hs[0], len(hs)
    if head0 < 0 or head0 + nheads > nh:
        raise ValueError(f"heads {head0} .. {head0 + nheads - 1} of {nh}")
    return head0, nheads


@torch.no_grad()
def render(probs, grid, threshold=None, heads=None, cmap="inferno", patch=16, keep=None):
    """probs f32 [F, heads, 1 + hw] on the device, grid = (h, w) -> (heat f32 [F, h, w], rgb u8 [F, h patch, w patch, 3]).
    heat = the mean over `heads` (None: all; an int: that head alone, which is the map itself; or consecutive heads) of the
    patch attention, masked by `keep` (u8 [F, heads, hw]) or by mass_mask(probs, threshold) when either is given
    (video_generation.py:229-238 in numpy's f32 arithmetic).  rgb = what plt.imsave(cmap=cmap) makes of heat upsampled x patch
    by nearest: every frame normalised by its own minimum and maximum.  cmap: a name (colormap_lut) or a u8 [256, 3] table;
    None: heat only, rgb is None."""
    p = _probs(probs)
    F, nh, n = p.shape
    h, w = int(grid[0]), int(grid[1])
    patch = int(patch)
    if h < 1 or w < 1 or h * w != n:
        raise ValueError(f"grid {h} x {w} does not hold {n} patches")
    if not 1 <= patch <= 64:
        raise ValueError(f"patch = {patch} must be in [1, 64]")
    head0, nheads = _head_range(heads, nh)
    if keep is not None and threshold is not None:
        raise ValueError("give threshold or keep, not both")
    if threshold is not None:
        keep = mass_mask(probs, threshold)
    if keep is not None:
        if not keep.is_cuda or keep.dtype != torch.uint8 or tuple(keep.shape) != (F, nh, n):
            raise ValueError(f"keep: expected a device u8 [{F}, {nh}, {n}] tensor")
        keep = keep.contiguous()
    dev = p.device
    heat = torch.empty(F, h, w, dtype=torch.float32, device=dev)
    rgb = lut = ws = None
    if cmap is not None:
        lut = cmap if isinstance(cmap, torch.Tensor) else torch.from_numpy(colormap_lut(cmap))
        if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
            raise ValueError("cmap: a colormap name or a u8 [256, 3] table")
        lut = lut.to(dev).contiguous()
        rgb = torch.empty(F, h * patch, w * patch, 3, dtype=torch.uint8, device=dev)
        ws = torch.empty(F * RENDER_WS_FLOATS, dtype=torch.float32, device=dev)
    ops.attn_render(p, keep, F, nh, head0, nheads, h, w, patch, lut, heat, rgb, ws)
    return heat, rgb


# ---------------------------------------------------------------------------------------------- colormaps, image files (host)
def colormap_lut(name):
    """u8 [256, 3]: the byte table Colormap.__call__(bytes=True) looks colours up in — matplotlib's own when it is importable,
    else the copy bundled with the package (`inferno` and `viridis`, written by tools/make_cmap_tables.py)."""
    if name not in _LUTS:
        try:
            from matplotlib import colormaps
        except ImportError:
            from ._cmap_tables import HEX
            if name not in HEX:
                raise ValueError(f"colormap {name!r}: without matplotlib only {sorted(HEX)} are available") from None
            lut = np.frombuffer(bytes.fromhex(HEX[name]), dtype=np.uint8).reshape(256, 3).copy()
        else:
            cm = colormaps[name]
            if cm.N != 256:
                raise ValueError(f"colormap {name!r} has {cm.N} entries: the kernel takes 256")
            if not cm._isinit:
                cm._init()
            lut = (cm._lut[:256, :3] * 255).astype(np.uint8)
        _LUTS[name] = lut
    return _LUTS[name]


def _image(rgb):
    from PIL import Image
    a = rgb.cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"expected a u8 [H, W, 3] image, got {a.dtype} {a.shape}")
    return Image, np.ascontiguousarray(a)


def save_jpeg(fname, rgb):
    """The file plt.imsave(fname, arr, cmap=..., format='jpg') writes for the colours `rgb` u8 [H, W, 3] of arr: imsave pastes
    its opaque RGBA image on an RGB background and saves with format='jpeg', dpi=(100, 100) (matplotlib.image.imsave)."""
    Image, a = _image(rgb)
    Image.fromarray(a).save(fname, format="jpeg", dpi=(100, 100))


def save_jpegs(fnames, rgb):
    """save_jpeg for a batch that is on the device: rgb u8 [F, H, W, 3] is encoded there (sais_amd.jpeg_enc) and fnames[j] gets
    the file save_jpeg(fnames[j], rgb[j]) writes, byte for byte."""
    if not isinstance(rgb, torch.Tensor) or not rgb.is_cuda:
        raise ValueError("rgb: expected a device tensor (save_jpeg writes a host array)")
    fnames = list(fnames)
    if rgb.dim() != 4 or rgb.shape[0] != len(fnames):
        raise ValueError(f"{len(fnames)} file names for images of shape {tuple(rgb.shape)}")
    if rgb.device not in _ENCODERS:
        from .jpeg_enc import JpegEncoder
        _ENCODERS[rgb.device] = JpegEncoder(rgb.device)
    for fname, blob in zip(fnames, _ENCODERS[rgb.device].encode(rgb.contiguous(), dpi=(100, 100))):
        with open(fname, "wb") as fh:
            fh.write(blob)


def save_png(fname, rgb):
    """The file plt.imsave(fname, arr, format='png') writes: the RGBA image (alpha 255) with dpi=(100, 100) and, as imsave adds
    it, a Software text chunk naming matplotlib's version — added here only when matplotlib is importable."""
    Image, a = _image(rgb)
    from PIL import PngImagePlugin
    rgba = np.concatenate([a, np.full(a.shape[:2] + (1,), 255, np.uint8)], axis=2)
    info = PngImagePlugin.PngInfo()
    try:
        import matplotlib
        info.add_text("Software", f"Matplotlib version{matplotlib.__version__}, https://matplotlib.org/")
    except ImportError:
        pass
    Image.fromarray(rgba).save(fname, format="png", dpi=(100, 100), pnginfo=info)


def save_image_png(fname, rgb):
    """A u8 [H, W, 3] image as a plain RGB PNG, as torchvision's save_image writes one."""
    Image, a = _image(rgb)
    Image.fromarray(a).save(fname, format="png")


def save_mask_png(fname, mask, patch=16):
    """A binary mask [h, w] as a black / white PNG upsampled x patch by nearest."""
    from PIL import Image
    m = mask.cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    m = np.repeat(np.repeat((m != 0).astype(np.uint8) * 255, patch, axis=0), patch, axis=1)
    Image.fromarray(m).save(fname, format="png")


def input_image_u8(x):
    """make_grid(img, normalize=True, scale_each=True) + save_image's conversion (visualize_attention.py:204) for ONE image:
    x f32 [3, H, W] normalised -> u8 [H, W, 3]: minus its minimum, divided by max(its range, 1e-5), times 255 plus 0.5, clamped,
    truncated — in f32."""
    x = np.asarray(x, dtype=np.float32)
    lo, hi = float(x.min()), float(x.max())
    y = (np.clip(x, np.float32(lo), np.float32(hi)) - np.float32(lo)) / np.float32(max(hi - lo, 1e-5))
    y = np.clip(y * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(y.transpose(1, 2, 0))


# ---------------------------------------------------------------------------------------------- frame loading (host)
def resize_size(width, height, size):
    """torchvision's Resize size rule -> (new width, new height): one int sets the SHORT side (the long one scaled with it,
    truncated), two ints are (h, w)."""
    size = [int(s) for s in (size if isinstance(size, (list, tuple)) else [size])]
    if len(size) == 2:
        return size[1], size[0]
    if len(size) != 1:
        raise ValueError("resize takes one or two integers")
    short, long = (width, height) if width <= height else (height, width)
    new_short, new_long = size[0], int(size[0] * long / short)
    return (new_short, new_long) if width <= height else (new_long, new_short)


def load_frame(path, resize=None, patch=16):
    """An image file -> f32 [3, H, W] (host) as both scripts prepare it: RGB, optionally resized, ToTensor (/ 255), Normalize
    with the reference's constants, cropped at the bottom / right to multiples of `patch`.  The optional resize is Pillow's
    bilinear filter under torchvision's size rule; torchvision's own filter (antialiased, on the tensor in video_generation.py,
    on the PIL image in visualize_attention.py) is not available to compare with: this step is PARITY-UNPINNED.  Without
    resize the result is the reference's bit for bit."""
    from PIL import Image
    with open(path, "rb") as fh:
        img = Image.open(fh).convert("RGB")
    if resize is not None:
        img = img.resize(resize_size(img.width, img.height, resize), Image.BILINEAR)
    a = np.asarray(img, dtype=np.uint8).astype(np.float32) / 255
    a = (a - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    H, W = a.shape[0] - a.shape[0] % patch, a.shape[1] - a.shape[1] % patch
    if H < patch or W < patch:
        raise ValueError(f"{path}: {a.shape[1]} x {a.shape[0]} pixels are less than one {patch} x {patch} patch")
    return torch.from_numpy(np.ascontiguousarray(a[:H, :W].transpose(2, 0, 1)))


def build_model(args, dev):
    """The backbone of the two scripts: frozen, and seeded so that it is the same in every run without --pretrained_weights."""
    return load_dino_backbone(args, dev, seed=0, freeze=True, random="random (seeded)")
