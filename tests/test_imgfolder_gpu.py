"""GPU: sais_jpeg_decode_mixed equals Pillow and the one-geometry decoder per file; sais_image_transform equals the Pillow
datasets' tensors bit for bit on raw arrays; GpuImageLoader equals the stacked items of EvalImageFolder, TrainImageFolder and
ImgListDataset on a folder of mixed files."""
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgfolder_ref as R  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"


def _jpeg(w, h, seed=0, **kw):
    buf = io.BytesIO()
    Image.fromarray(R.make_image(w, h, seed)).save(buf, "JPEG", **kw)
    return buf.getvalue()


def _items(blobs):
    from sais_amd import jpeg
    out = []
    for i, b in enumerate(blobs):
        h = jpeg.parse_header(b)
        out.append((b, None if h is None else bytes(h), i))
    return out


# ------------------------------------------------------------------------------------------------ mixed decode
def _mixed_files():
    """(w, h) with no single image the largest on both axes; every sampling; a restart interval; two qualities."""
    return [_jpeg(1, 1, quality=75), _jpeg(8, 8, quality=75), _jpeg(7, 9, quality=75, subsampling=2),
            _jpeg(33, 17, quality=75, subsampling=1), _jpeg(16, 16, quality=75, subsampling=0),
            _jpeg(40, 24, quality=75, restart_marker_blocks=2), _jpeg(9, 70, quality=75), _jpeg(70, 9, quality=75),
            _jpeg(64, 48, quality=95)]


@gpu
def test_mixed_decode_matches_pillow_and_the_uniform_decoder():
    from sais_amd import imgfolder, jpeg
    blobs = _mixed_files()
    assert jpeg.parse_header(blobs[5]).restart_interval == 2 and jpeg.parse_header(blobs[5]).segments > 1
    assert [(jpeg.parse_header(b).hsamp, jpeg.parse_header(b).vsamp) for b in blobs[2:5]] == [(2, 2), (2, 1), (1, 1)]
    loader = imgfolder.GpuImageLoader(DEV)
    images, status = loader.decode(_items(blobs))
    assert status == [0] * len(blobs) and loader.stats == {"gpu": 0, "unsupported": 0, "failed": 0, "pillow_transform": 0}
    single = jpeg.JpegDecoder(DEV)
    for i, b in enumerate(blobs):
        want = np.asarray(Image.open(io.BytesIO(b)))
        assert np.array_equal(images[i].cpu().numpy(), want), i
        assert torch.equal(images[i], single.decode([b])[0]), i
    assert single.stats["gpu"] == len(blobs)
    # the same batch in reversed order
    rev, status = loader.decode(_items(blobs[::-1]))
    assert status == [0] * len(blobs)
    for i in range(len(blobs)):
        assert torch.equal(rev[len(blobs) - 1 - i], images[i]), i
    # a truncated file in the middle: flagged, its neighbours intact
    cut = list(blobs)
    cut[4] = blobs[8][:len(blobs[8]) - jpeg.parse_header(blobs[8]).scan_bytes // 2]
    assert jpeg.parse_header(cut[4]) is not None
    got, status = loader.decode(_items(cut))
    assert status[4] != 0 and [s for k, s in enumerate(status) if k != 4] == [0] * (len(blobs) - 1)
    for i in range(len(blobs)):
        if i != 4:
            assert torch.equal(got[i], images[i]), i


# ------------------------------------------------------------------------------------------------ transform on raw arrays
def _run_transform(images, geometries, out_hw, order=None, lut=None):
    """One sais_image_transform launch over raw uint8 arrays; image i writes output slot order[i].  -> float32 [n,3,h,w].
    lut: a [3][256] float32 table in place of the normalisation table."""
    from sais_amd import _lib as L, imgfolder
    oh, ow = out_hw
    n = len(images)
    order = list(range(n)) if order is None else order
    rows, off = [], 0
    for img, g, slot in zip(images, geometries, order):
        rows.append(imgfolder.descriptor(g, img.shape[1], img.shape[0], out_hw, off, slot * 3 * oh * ow))
        off += (img.size + 255) // 256 * 256
    table = np.array(rows, dtype=imgfolder.XFORM_DTYPE)
    src = np.zeros(off, np.uint8)
    for img, row in zip(images, rows):
        src[row[0]:row[0] + img.size] = img.reshape(-1)
    src_d = torch.from_numpy(src).to(DEV)
    table_d = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)
    lut = torch.from_numpy(imgfolder.normalize_table() if lut is None else lut).to(DEV)
    out = torch.full((n, 3, oh, ow), float("nan"), dtype=torch.float32, device=DEV)
    L.call("sais_image_transform", src_d.data_ptr(), src_d.numel(), table.ctypes.data, table_d.data_ptr(), n, oh, ow,
           lut.data_ptr(), out.data_ptr(), out.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu()


@gpu
def test_crop_resize_and_image_transform_share_one_resampler():
    """The two kernels built on the band of resample.hpp give the same bytes, and those of the numpy restatement.  S = 17 ends
    crop_resize's second band (16 rows) after one row while image_transform takes it in one band; S = 33 ends the last band
    of both after one row (bands of 16 and 32); S = 96 is 6 and 3 full bands, once upscaling from 3 x 2 pixels; S = 1 is a
    single output byte."""
    from sais_amd.augment import DinoAugmenter
    from sais_amd.dino_data import ViewParams
    img = R.make_image(131, 97)
    frames = torch.from_numpy(img[None]).to(DEV)
    aug = DinoAugmenter(DEV)
    identity = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.float32), (3, 256)))
    for box, s in [((0, 0, 131, 97), 1), ((0, 0, 131, 97), 17), ((2, 1, 130, 96), 33), ((5, 5, 45, 35), 96), ((0, 0, 3, 2), 96)]:
        view = ViewParams(box=box, size=s, flip=False, jitter=False, order=(0, 1, 2, 3), brightness=1.0, contrast=1.0,
                          saturation=1.0, hue=0.0, gray=False, blur=None, solarize=False)
        cropped = aug.crop_resize(frames, [[view]], (0, 0, 131, 97))[0][0].cpu()
        out = _run_transform([img], [(box, (s, s), (0, 0), R.BICUBIC, False)], (s, s), lut=identity)[0]
        assert tuple(cropped.shape) == (s, s, 3) and cropped.dtype == torch.uint8
        assert torch.equal(out.to(torch.uint8).permute(1, 2, 0), cropped), (box, s)
        assert torch.equal(out, out.to(torch.uint8).to(torch.float32)), (box, s)         # whole bytes: the cast dropped nothing
        want = torch.from_numpy(R.window_u8(img, box, s, s, 0, 0, s, s, R.BICUBIC))
        assert torch.equal(cropped, want), (box, s)


@gpu
def test_transform_matches_the_pillow_datasets():
    from sais_amd import imgfolder
    from sais_amd.knn import EvalImageFolder
    from sais_amd.linear import TrainImageFolder
    images, geometries, want = [], [], []
    ev, tr = imgfolder.eval_builder(), imgfolder.train_builder()
    for w, h in R.EVAL_SIZES:
        img = R.make_image(w, h)
        images.append(img)
        geometries.append(ev(None, w, h))
        want.append(EvalImageFolder.transform(Image.fromarray(img)))
    for (w, h), box in R.TRAIN_BOXES:
        for flip in (False, True):
            img = R.make_image(w, h, seed=1)
            images.append(img)
            geometries.append(tr((b"", None, 0, box, flip), w, h))
            want.append(TrainImageFolder.apply(Image.fromarray(img), box, flip))
    # a window touching two borders of the resampled image, both filters; the second mirrored
    img = R.make_image(150, 97, seed=3)
    for filt, pil in ((R.BICUBIC, Image.BICUBIC), (R.BILINEAR, Image.BILINEAR)):
        full = np.asarray(Image.fromarray(img).crop((5, 3, 140, 90)).resize((260, 231), pil))
        images += [img, img]
        geometries += [((5, 3, 140, 90), (260, 231), (36, 7), filt, False), ((5, 3, 140, 90), (260, 231), (0, 0), filt, True)]
        want += [torch.from_numpy(R.to_tensor(full[7:, 36:])), torch.from_numpy(R.to_tensor(full[:224, :224][:, ::-1]))]
    n = len(images)
    order = [(7 * i + 3) % n for i in range(n)]                      # permuted output offsets (7 and n = 19 are coprime)
    assert sorted(order) == list(range(n))
    out = _run_transform(images, geometries, (224, 224), order)
    for i in range(n):
        assert torch.equal(out[order[i]], want[i]), (i, images[i].shape, geometries[i])


@gpu
def test_transform_flip_at_odd_and_even_widths_and_320():
    from sais_amd import imgfolder
    from sais_amd.retrieval import _to_tensor
    # flip at an odd and an even output width, rectangular output
    for ow, oh in ((223, 117), (224, 118), (1, 1)):
        img = R.make_image(97, 61, seed=ow)
        pil = Image.fromarray(img).crop((3, 2, 95, 60)).resize((ow, oh), Image.BILINEAR).transpose(Image.FLIP_LEFT_RIGHT)
        out = _run_transform([img], [((3, 2, 95, 60), (ow, oh), (0, 0), R.BILINEAR, True)], (oh, ow))
        assert torch.equal(out[0], _to_tensor(pil)), (ow, oh)
    # the copy-detection transform: 320 x 320 (more than one band per image, a downscale and an upscale in one launch)
    sq = imgfolder.square_builder(320)
    images = [R.make_image(w, h, seed=2) for (w, h), _ in R.SQUARE_SIZES] + [R.make_image(700, 90, seed=4), R.make_image(320, 320, 5)]
    out = _run_transform(images, [sq(None, im.shape[1], im.shape[0]) for im in images], (320, 320))
    for i, im in enumerate(images):
        assert torch.equal(out[i], sq.pillow(None, Image.fromarray(im))), im.shape


@gpu
def test_refused_descriptor_launches_nothing():
    from sais_amd import _lib as L, imgfolder
    img = R.make_image(300, 200)
    good = imgfolder.descriptor(imgfolder.eval_builder()(None, 300, 200), 300, 200, (224, 224), 0, 0)
    bad = good[:6] + (good[6] + 200,) + good[7:9] + (0, 3 * 224 * 224)                  # window leaves the resampled image
    table = np.array([good, bad], dtype=imgfolder.XFORM_DTYPE)
    assert table[1]["win_left"] == good[6] + 200 and table[1]["rw"] == good[4]
    src = torch.from_numpy(img.reshape(-1).copy()).to(DEV)
    table_d = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)
    lut = torch.from_numpy(imgfolder.normalize_table()).to(DEV)
    out = torch.full((2, 3, 224, 224), -7.0, dtype=torch.float32, device=DEV)
    rc = L.load().sais_image_transform(src.data_ptr(), src.numel(), table.ctypes.data, table_d.data_ptr(), 2, 224, 224,
                                       lut.data_ptr(), out.data_ptr(), out.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == -7.0).all())
    # the kernel skips a descriptor its device copy shows to be out of range, and serves the others
    ok_host = np.array([good, good[:10] + (3 * 224 * 224,)], dtype=imgfolder.XFORM_DTYPE)
    rc = L.load().sais_image_transform(src.data_ptr(), src.numel(), ok_host.ctypes.data, table_d.data_ptr(), 2, 224, 224,
                                       lut.data_ptr(), out.data_ptr(), out.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    from sais_amd.knn import EvalImageFolder
    assert rc == 0 and bool((out[1] == -7.0).all())
    assert torch.equal(out[0].cpu(), EvalImageFolder.transform(Image.fromarray(img)))


# ------------------------------------------------------------------------------------------------ end to end
def _write_folder(root):
    """Two class folders: ten baseline JPEGs of different size, quality and sampling, a progressive and a grayscale JPEG,
    a PNG.  -> the names of the three files the parser refuses."""
    specs = [(500, 375, 75, 2), (375, 500, 90, 0), (500, 333, 75, 1), (640, 480, 90, 2), (97, 131, 75, 2), (224, 224, 95, 0),
             (256, 300, 75, 2), (31, 20, 90, 0), (333, 211, 75, 1), (320, 320, 90, 2)]
    for k, (w, h, q, ss) in enumerate(specs):
        d = os.path.join(root, "c%d" % (k % 2))
        os.makedirs(d, exist_ok=True)
        Image.fromarray(R.make_image(w, h, seed=k)).save(os.path.join(d, "img%02d.jpg" % k), quality=q, subsampling=ss)
    Image.fromarray(R.make_image(300, 200, seed=20)).save(os.path.join(root, "c0", "prog.jpg"), quality=80, progressive=True)
    Image.fromarray(R.make_image(210, 280, seed=21)[:, :, 1]).save(os.path.join(root, "c1", "gray.jpg"), quality=80)
    Image.fromarray(R.make_image(123, 345, seed=22)).save(os.path.join(root, "c1", "pic.png"))
    return {"prog.jpg", "gray.jpg", "pic.png"}


@gpu
def test_loader_equals_the_pillow_datasets(tmp_path):
    from sais_amd import imgfolder
    from sais_amd.knn import EvalImageFolder
    from sais_amd.linear import TrainImageFolder
    from sais_amd.retrieval import ImgListDataset
    root = str(tmp_path)
    refused = _write_folder(root)
    loader = imgfolder.GpuImageLoader(DEV)

    def host_files(plan, samples):
        return {os.path.basename(samples[i][0] if isinstance(samples[i], tuple) else samples[i]) for i in plan.host}

    ref = EvalImageFolder(root)
    raw = imgfolder.RawEvalFolder(root)
    assert raw.samples == ref.samples and len(raw) == 13
    items, tags = imgfolder.collate_raw([raw[i] for i in range(len(raw))])
    got = loader.eval(items)
    assert got.is_cuda and torch.equal(got.cpu(), torch.stack([ref[i][0] for i in range(len(ref))]))
    assert tags.tolist() == list(range(13))
    assert loader.stats == {"gpu": 10, "unsupported": 3, "failed": 0, "pillow_transform": 0}
    assert host_files(loader.last_plan, ref.samples) == refused

    ref = TrainImageFolder(root, seed=3)
    raw = imgfolder.RawTrainFolder(root, seed=3)
    for epoch in (0, 2):
        ref.set_epoch(epoch)
        raw.set_epoch(epoch)
        items, tags = imgfolder.collate_raw([raw[i] for i in range(len(raw))])
        got = loader.train(items)
        assert torch.equal(got.cpu(), torch.stack([ref[i][0] for i in range(len(ref))])), epoch
        assert tags.tolist() == [ref[i][1] for i in range(len(ref))]
    assert host_files(loader.last_plan, ref.samples) == refused

    paths = [p for p, _ in ref.samples][::-1]
    ref = ImgListDataset(paths, 320)
    raw = imgfolder.RawImgList(paths)
    items, tags = imgfolder.collate_raw([raw[i] for i in range(len(raw))])
    got = loader.square(items, 320)
    assert tuple(got.shape) == (13, 3, 320, 320)
    assert torch.equal(got.cpu(), torch.stack([ref[i][0] for i in range(len(ref))]))
    assert host_files(loader.last_plan, paths) == refused
    assert loader.stats == {"gpu": 40, "unsupported": 12, "failed": 0, "pillow_transform": 0}

    # through a DataLoader and the batch hook, as the tools run it
    dl = torch.utils.data.DataLoader(imgfolder.RawEvalFolder(root), batch_size=5, num_workers=0, collate_fn=imgfolder.collate_raw)
    ref = EvalImageFolder(root)
    batches = imgfolder.GpuBatches(dl, loader.eval)
    assert len(batches) == 3 and len(batches.dataset) == 13
    for x, index in batches:
        assert torch.equal(x.cpu(), torch.stack([ref[int(i)][0] for i in index]))
