"""CPU: the numpy restatement of the image-folder transforms (tests/imgfolder_ref.py) equals Pillow bit for bit; the
descriptor builders, the host-side refusals of sais_image_transform, the loader's routing and the tools' switch."""
import ctypes
import importlib.util
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imgfolder_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref_tensor(img, geometry, out_hw):
    box, (rw, rh), (wl, wt), filt, flip = geometry
    return R.to_tensor(R.window_u8(img, box, rw, rh, wl, wt, out_hw[1], out_hw[0], filt, flip))


# ------------------------------------------------------------------------------------------------ arithmetic against Pillow
def test_normalize_table_is_the_datasets_expression():
    from sais_amd import imgfolder
    from sais_amd.knn import EvalImageFolder
    assert np.array_equal(R.normalize_table(), imgfolder.normalize_table())
    a = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    want = (a.astype(np.float32) / 255.0 - np.asarray(EvalImageFolder.MEAN, np.float32)) / np.asarray(EvalImageFolder.STD, np.float32)
    assert np.array_equal(R.to_tensor(a), want.transpose(2, 0, 1))


@pytest.mark.parametrize("wh", R.EVAL_SIZES)
def test_eval_transform_matches_pillow(wh):
    from sais_amd import imgfolder
    from sais_amd.knn import EvalImageFolder, eval_transform_geometry
    w, h = wh
    img = R.make_image(w, h)
    (nw, nh), (left, top) = eval_transform_geometry(w, h)
    assert 0 <= left <= nw - 224 and 0 <= top <= nh - 224            # the window lies inside the resampled image
    geometry = imgfolder.eval_builder()(None, w, h)
    assert geometry == ((0, 0, w, h), (nw, nh), (left, top), R.BICUBIC, False)
    got = _ref_tensor(img, geometry, (224, 224))
    assert np.array_equal(got, EvalImageFolder.transform(Image.fromarray(img)).numpy())


@pytest.mark.parametrize("case", R.TRAIN_BOXES)
@pytest.mark.parametrize("flip", [False, True])
def test_train_transform_matches_pillow(case, flip):
    from sais_amd import imgfolder
    from sais_amd.linear import TrainImageFolder
    (w, h), box = case
    img = R.make_image(w, h, seed=1)
    geometry = imgfolder.train_builder()((b"", None, 0, box, flip), w, h)
    assert geometry == (box, (224, 224), (0, 0), R.BILINEAR, flip)
    got = _ref_tensor(img, geometry, (224, 224))
    assert np.array_equal(got, TrainImageFolder.apply(Image.fromarray(img), box, flip).numpy())


@pytest.mark.parametrize("case", R.SQUARE_SIZES)
def test_square_transform_matches_pillow(case, tmp_path):
    from sais_amd import imgfolder
    from sais_amd.retrieval import ImgListDataset
    (w, h), imsize = case
    img = R.make_image(w, h, seed=2)
    path = str(tmp_path / "a.png")
    Image.fromarray(img).save(path)
    geometry = imgfolder.square_builder(imsize)(None, w, h)
    assert geometry == ((0, 0, w, h), (imsize, imsize), (0, 0), R.BICUBIC, False)
    got = _ref_tensor(img, geometry, (imsize, imsize))
    assert np.array_equal(got, ImgListDataset([path], imsize)[0][0].numpy())


def test_window_touching_two_borders_matches_pillow():
    img = R.make_image(150, 97, seed=3)
    for filt, pil in ((R.BICUBIC, Image.BICUBIC), (R.BILINEAR, Image.BILINEAR)):
        full = np.asarray(Image.fromarray(img).crop((5, 3, 140, 90)).resize((260, 231), pil))
        got = R.window_u8(img, (5, 3, 140, 90), 260, 231, 260 - 224, 231 - 224, 224, 224, filt)     # right and bottom borders
        assert np.array_equal(got, full[7:, 36:])
        got = R.window_u8(img, (5, 3, 140, 90), 260, 231, 0, 0, 224, 224, filt, flip=True)          # left and top borders
        assert np.array_equal(got, full[:224, :224][:, ::-1])


# ------------------------------------------------------------------------------------------------ builders
def test_train_items_carry_the_draws_of_the_pillow_dataset(tmp_path):
    from sais_amd import imgfolder
    from sais_amd.linear import TrainImageFolder
    os.makedirs(tmp_path / "c0")
    Image.fromarray(R.make_image(123, 77)).save(str(tmp_path / "c0" / "a.jpg"), quality=90)
    Image.fromarray(R.make_image(60, 91)).save(str(tmp_path / "c0" / "b.png"))
    raw, ref = imgfolder.RawTrainFolder(str(tmp_path), seed=5), TrainImageFolder(str(tmp_path), seed=5)
    for epoch in (0, 3):
        raw.set_epoch(epoch)
        ref.set_epoch(epoch)
        for i, (w, h) in enumerate(((123, 77), (60, 91))):
            blob, hdr, label, box, flip = raw[i]
            assert (box, flip) == ref.draw(i, w, h) and label == 0
            assert (hdr is None) == (i == 1) and blob == open(ref.samples[i][0], "rb").read()
    items, tags = imgfolder.collate_raw([raw[0], raw[1]])
    assert len(items) == 2 and tags.dtype == torch.long and tags.tolist() == [0, 0]
    ev = imgfolder.RawEvalFolder(str(tmp_path))
    assert ev[1][2] == 1 and ev[1][1] is None and len(ev) == 2
    assert imgfolder.RawLabelledEvalFolder(str(tmp_path))[1][2] == 0
    assert imgfolder.RawImgList(p for p, _ in ref.samples)[0][2] == 0


# ------------------------------------------------------------------------------------------------ refusals (no launch: no GPU needed)
def _table(rows):
    from sais_amd import imgfolder
    return np.array(rows, dtype=imgfolder.XFORM_DTYPE)


def _transform_rc(rows, out_hw=(224, 224), src_bytes=1 << 30, out_elems=1 << 30):
    from sais_amd import _lib
    t = _table(rows)
    fake = ctypes.c_void_p(4096)                                     # never dereferenced: every case here is refused first
    return _lib.load().sais_image_transform(fake, src_bytes, t.ctypes.data, fake, len(t), out_hw[0], out_hw[1], fake, fake,
                                            out_elems, None)


def test_table_check_refuses_bad_descriptors():
    from sais_amd import imgfolder
    good = imgfolder.descriptor(((0, 0, 300, 200), (341, 256), (58, 16), R.BICUBIC, False), 300, 200, (224, 224))

    def rep(**kw):
        d = dict(zip(imgfolder.XFORM_DTYPE.names, good))
        d.update(kw)
        return tuple(d[k] for k in imgfolder.XFORM_DTYPE.names)
    assert imgfolder.fits(good, (224, 224))
    bad = [rep(win_left=341 - 224 + 1), rep(win_top=256 - 224 + 1), rep(win_left=-1), rep(rw=223),        # window outside
           rep(box=(10, 10, 10, 50)), rep(box=(10, 50, 20, 50)), rep(box=(0, 0, 301, 200)), rep(box=(-1, 0, 300, 200)),  # box
           rep(filter=2), rep(src_offset=-1), rep(out_offset=-1), rep(src_h=0)]
    for row in bad:
        assert _transform_rc([good, row]) == -1, row
    assert _transform_rc([good], src_bytes=300 * 200 * 3 - 1) == -1 and _transform_rc([good], out_elems=3 * 224 * 224 - 1) == -1
    assert _transform_rc([good], out_hw=(513, 224)) == -1 and _transform_rc([good], out_hw=(224, 0)) == -1
    assert _transform_rc([rep(rw=320, rh=320, win_left=0, win_top=0)], out_hw=(320, 320), out_elems=3 * 320 * 320 - 1) == -1
    # the LDS fit: a one-row band of a 60000-to-256 bicubic downscale holds 60000 / 256 * 4 + 1 taps per output column
    huge = imgfolder.descriptor(((0, 0, 60000, 60000), (256, 256), (16, 16), R.BICUBIC, False), 60000, 60000, (224, 224))
    assert not imgfolder.fits(huge, (224, 224))
    assert _transform_rc([good, huge], src_bytes=1 << 40) == -1
    assert imgfolder.fits(imgfolder.descriptor(((0, 0, 4000, 3000), (341, 256), (58, 16), R.BICUBIC, False), 4000, 3000,
                                               (224, 224)), (224, 224))


def test_mixed_decode_entry_refuses_bad_batches():
    from sais_amd import _lib, jpeg
    lib = _lib.load()
    buf = io.BytesIO()
    Image.fromarray(R.make_image(40, 24)).save(buf, "JPEG", quality=90)
    h = jpeg.parse_header(buf.getvalue())
    hs = (jpeg.SaisJpegHeader * 2)(h, h)
    need = lib.sais_jpeg_mixed_workspace_bytes(hs, 2)
    assert need > 0 and lib.sais_jpeg_mixed_workspace_bytes(hs, 0) == 0 and lib.sais_jpeg_mixed_workspace_bytes(None, 2) == 0
    # the workspace grows with the sum of the images' sizes: a large image among small ones costs one large slot
    big = jpeg.SaisJpegHeader.from_buffer_copy(h)
    big.height, big.width = 3000, 4000
    small_n = 64
    many = (jpeg.SaisJpegHeader * (small_n + 1))(*([h] * small_n + [big]))
    one_big = lib.sais_jpeg_mixed_workspace_bytes((jpeg.SaisJpegHeader * 1)(big), 1)
    assert lib.sais_jpeg_mixed_workspace_bytes(many, small_n + 1) < one_big + small_n * need
    fake = ctypes.c_void_p(4096)
    offs = (ctypes.c_int64 * 2)(0, 40 * 24 * 3)

    def rc(n=2, data_bytes=1 << 20, offsets=offs, ws=need, out_bytes=2 * 40 * 24 * 3):
        return lib.sais_jpeg_decode_mixed(n, fake, data_bytes, hs, fake, offsets, fake, fake, ws, fake, out_bytes, fake, None)
    assert rc(n=0) == -1 and rc(ws=need - 1) == -1 and rc(out_bytes=2 * 40 * 24 * 3 - 1) == -1
    assert rc(offsets=(ctypes.c_int64 * 2)(0, -1)) == -1 and rc(data_bytes=2 * h.scan_bytes - 1) == -1


# ------------------------------------------------------------------------------------------------ routing
class StubBackend:
    """Stands in for the device half: reports the files it is told to flag, records what it is given."""

    def __init__(self, flag=()):
        self.flag, self.uploaded, self.plans = set(flag), [], []

    def decode(self, plan):
        self.plans.append(plan)
        return np.array([8 if i in self.flag else 0 for i in plan.gpu], np.int32)

    def upload(self, plan, i, rgb):
        self.uploaded.append((i, rgb.shape))

    def transform(self, plan, tensors):
        self.tensors = tensors
        return torch.zeros(len(plan.items), 3, *plan.out_hw)


def _jpeg(w, h, **kw):
    buf = io.BytesIO()
    Image.fromarray(R.make_image(w, h)).save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_loader_routing_and_stats():
    from sais_amd import imgfolder, jpeg
    from sais_amd.knn import EvalImageFolder
    png = io.BytesIO()
    Image.fromarray(R.make_image(50, 40)).save(png, "PNG")
    gray = io.BytesIO()
    Image.fromarray(R.make_image(33, 47)[:, :, 0]).save(gray, "JPEG")
    blobs = [_jpeg(64, 48, quality=90), _jpeg(31, 77, quality=75, progressive=True), png.getvalue(), _jpeg(100, 30, quality=75),
             gray.getvalue(), _jpeg(9000, 16, quality=30), _jpeg(20, 20, quality=75)]
    items = []
    for i, b in enumerate(blobs):
        h = jpeg.parse_header(b)
        items.append((b, None if h is None else bytes(h), i))
    assert [it[1] is None for it in items] == [False, True, True, False, True, False, False]
    stub = StubBackend(flag={3})
    loader = imgfolder.GpuImageLoader(backend=stub)
    out = loader.eval(items)
    assert tuple(out.shape) == (7, 3, 224, 224)
    plan = stub.plans[0]
    # 9000 x 16 -> Resize(256) makes 144000 x 256: an upscale, a few taps per output index.  The fit predicate refuses nothing here
    assert plan.gpu == [0, 3, 5, 6] and sorted(plan.host) == [1, 2, 4] and plan.pillow == []
    assert stub.uploaded == [(3, (30, 100, 3))]
    assert loader.stats == {"gpu": 3, "unsupported": 3, "failed": 1, "pillow_transform": 0}
    assert [i for i, _ in plan.rows] == [0, 1, 2, 3, 4, 5, 6]
    assert [r[10] for _, r in plan.rows] == [i * 3 * 224 * 224 for i in range(7)]
    # an image the fit predicate refuses goes through the Pillow transform itself, whichever decoder it would have had
    wide = _jpeg(30000, 8, quality=20)
    h = jpeg.parse_header(wide)
    assert h is not None
    stub2 = StubBackend()
    loader2 = imgfolder.GpuImageLoader(backend=stub2)
    loader2.square([items[0], (wide, bytes(h), 1), items[2]], 64)
    plan = stub2.plans[0]
    assert plan.gpu == [0] and sorted(plan.host) == [2] and plan.pillow == [1]
    assert loader2.stats == {"gpu": 1, "unsupported": 1, "failed": 0, "pillow_transform": 1}
    want = imgfolder.square_builder(64).pillow(None, Image.open(io.BytesIO(wide)))
    assert list(stub2.tensors) == [1] and torch.equal(stub2.tensors[1], want)
    assert torch.equal(imgfolder.eval_builder().pillow(None, Image.open(io.BytesIO(blobs[0]))),
                       EvalImageFolder.transform(Image.open(io.BytesIO(blobs[0]))))
    with pytest.raises(ValueError):
        loader.eval([])


# ------------------------------------------------------------------------------------------------ the tools' switch
@pytest.mark.parametrize("name", ["eval_knn", "eval_linear", "eval_copy_detection"])
def test_gpu_loader_flag_parses_and_defaults_to_false(name):
    path = os.path.join(ROOT, "SAIS", "scripts", "dino-main", name + ".py")
    spec = importlib.util.spec_from_file_location("sais_imgfolder_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cli = getattr(mod, "get_cli_parser", mod.get_args_parser)()
    assert cli.parse_args([]).gpu_loader is False
    assert cli.parse_args(["--gpu_loader", "true"]).gpu_loader is True
    assert cli.parse_args(["--gpu_loader", "false"]).gpu_loader is False
    with pytest.raises(SystemExit):
        cli.parse_args(["--gpu_loader", "maybe"])
