"""CPU: the numpy restatement of img.thumbnail((imsize, imsize), LANCZOS) (tests/thumb_ref.py) equals Pillow bit for bit, step
by step; the C host coefficient rows equal the restatement's; the host-side refusals of sais_thumbnail and its companions; the
routing of GpuImageLoader.thumbnail with a fake backend; the switches of eval_image_retrieval.py."""
import ctypes
import importlib.util
import io
import os
import pickle
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thumb_ref as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(fx, fy) for fx in range(1, 9) for fy in range(1, 9)]


def _pillow_thumb(img, imsize):
    p = Image.fromarray(img)
    p.thumbnail((imsize, imsize), Image.LANCZOS)
    return np.asarray(p)


# ------------------------------------------------------------------------------------------------ restatement against Pillow
@pytest.mark.parametrize("whs", T.GEOMETRIES)
def test_thumbnail_matches_pillow(whs):
    from sais_amd import imgfolder
    w, h, imsize = whs
    img = T.make_image(w, h)
    want = _pillow_thumb(img, imsize)
    g = T.geometry(w, h, imsize)
    assert g == imgfolder.thumbnail_geometry(w, h, imsize)
    assert (g is None) == (want.shape[:2] == (h, w))
    if g is not None:
        assert g[0] == (want.shape[1], want.shape[0])
    assert np.array_equal(T.thumbnail_u8(img, imsize), want)


def test_geometry_list_is_what_it_says():
    """The list's cases are the paths they are there for."""
    G = {whs: T.geometry(*whs) for whs in T.GEOMETRIES}
    assert G[(12, 9, 16)] is None
    assert G[(63, 47, 16)] == ((16, 12), (1, 1)) and G[(63, 16, 16)][1] == (1, 2)
    assert G[(67, 45, 16)][1] == (2, 2) and (67 / 2, 45 / 2) == (33.5, 22.5)
    for whs in ((100, 7, 24), (40, 30, 10)):
        assert G[whs][1][0] != G[whs][1][1]
    assert G[(255, 3, 16)] == ((16, 1), (7, 1))
    assert G[(130, 97, 8)][1] == (8, 8) and G[(97, 130, 8)][1] == (8, 8)
    assert G[(17, 1, 16)] == ((16, 1), (1, 1)) and G[(1, 17, 16)] == ((1, 16), (1, 1))
    assert G[(64, 64, 16)] == ((16, 16), (2, 2)) and G[(1023, 767, 224)] == ((224, 168), (2, 2))
    # the largest ksize of the list: 25 on both axes of 63 x 47 -> 16 x 12
    assert T.lanczos_rows(63, 63.0, 16)[1].shape[1] == 25 and T.lanczos_rows(47, 47.0, 12)[1].shape[1] == 25
    # one axis unchanged: its pass is skipped
    assert not T.needs_pass(1, 1.0, 1) and T.needs_pass(17, 17.0, 16)


@pytest.mark.parametrize("multiple", [True, False])
def test_reduce_matches_pillow(multiple):
    for fx, fy in PAIRS:
        w, h = (fx * 6, fy * 5) if multiple else (fx * 6 + fx // 2, fy * 5 + fy - 1)
        img = T.make_image(w, h, seed=1)
        want = np.asarray(Image.fromarray(img).reduce((fx, fy)))
        assert want.shape[:2] == (-(-h // fy), -(-w // fx))
        assert np.array_equal(T.reduce(img, fx, fy), want), (fx, fy, w, h)
    img = T.make_image(130, 97, seed=1)
    assert np.array_equal(T.reduce(img, 16, 16), np.asarray(Image.fromarray(img).reduce((16, 16))))


def test_decomposition_is_pillows_own():
    """thumbnail == reduce + resize with the fractional box, in Pillow itself."""
    for w, h, imsize in T.GEOMETRIES:
        g = T.geometry(w, h, imsize)
        if g is None:
            continue
        (x, y), (fx, fy) = g
        p = Image.fromarray(T.make_image(w, h))
        r = p.reduce((fx, fy)) if fx > 1 or fy > 1 else p
        got = np.asarray(r.resize((x, y), Image.LANCZOS, box=(0, 0, w / fx, h / fy)))
        assert np.array_equal(got, _pillow_thumb(T.make_image(w, h), imsize))


def test_random_sweep_matches_pillow():
    rng = np.random.default_rng(20261020)
    kinds = set()
    for _ in range(1000):
        w, h, imsize = int(rng.integers(1, 301)), int(rng.integers(1, 301)), int(rng.integers(1, 65))
        img = T.make_image(w, h, seed=2)
        assert np.array_equal(T.thumbnail_u8(img, imsize), _pillow_thumb(img, imsize)), (w, h, imsize)
        g = T.geometry(w, h, imsize)
        kinds.add(None if g is None else (g[1][0] > 1, g[1][1] > 1, w % g[1][0] != 0, h % g[1][1] != 0))
    assert None in kinds and len(kinds) >= 8                          # untouched, and most factor / partial-edge combinations


@pytest.mark.parametrize("whs", T.TALL)
def test_tall_narrow_images_take_the_vertical_pass_first(whs):
    """Image.resize's last branch: the reduced image more than 100 times as high as wide, a lower output."""
    from sais_amd import imgfolder
    w, h, imsize = whs
    (x, y), (fx, fy) = T.geometry(w, h, imsize)
    rw, rh = -(-w // fx), -(-h // fy)
    assert T.vertical_first(rw, rh, y) and imgfolder.thumbnail_vertical_first(rw, rh, y)
    img = T.make_image(w, h, seed=3)
    assert np.array_equal(T.thumbnail_u8(img, imsize), _pillow_thumb(img, imsize))


def test_vertical_first_is_not_horizontal_first_and_switches_at_100():
    img = T.make_image(3, 1980, seed=3)
    a = T.reduce(img, 1, 2)
    h_first = T._pass_axis0(T._pass_axis0(a.transpose(1, 0, 2), *T.lanczos_rows(3, 3.0, 1)).transpose(1, 0, 2),
                            *T.lanczos_rows(990, 990.0, 431))
    assert not np.array_equal(h_first, _pillow_thumb(img, 431))       # the order shows in the bytes
    assert not T.vertical_first(5, 500, 100) and T.vertical_first(5, 501, 100) and not T.vertical_first(5, 501, 501)
    for h in (500, 501, 510):                                         # both sides of the switch, no reduce
        img = T.make_image(5, h, seed=3)
        assert np.array_equal(T.thumbnail_u8(img, 300), _pillow_thumb(img, 300)), h
    rng = np.random.default_rng(7)
    taken = 0
    for _ in range(60):
        w, h, imsize = int(rng.integers(1, 9)), int(rng.integers(200, 1200)), int(rng.integers(8, 600))
        img = T.make_image(w, h, seed=4)
        assert np.array_equal(T.thumbnail_u8(img, imsize), _pillow_thumb(img, imsize)), (w, h, imsize)
        g = T.geometry(w, h, imsize)
        taken += g is not None and T.vertical_first(-(-w // g[1][0]), -(-h // g[1][1]), g[0][1])
    assert 10 <= taken <= 55


def test_box_end_is_a_c_float():
    """_imaging.c parses the box with "(ffff)": 123 / 5 = 24.6 reaches Resample.c as 24.6f.  With the double the rows differ."""
    a = T.lanczos_rows(25, float(np.float32(24.6)), 12)[1]
    b = T.lanczos_rows(25, 24.6, 12)[1]
    assert not np.array_equal(a, b)
    img = T.make_image(248, 123, seed=2)
    assert np.array_equal(T.thumbnail_u8(img, 25), _pillow_thumb(img, 25))


# ------------------------------------------------------------------------------------------------ the C host rows
def test_c_rows_equal_the_restatement():
    from sais_amd import imgfolder
    axes = 0
    for w, h, imsize in T.GEOMETRIES:
        g = T.geometry(w, h, imsize)
        if g is None:
            continue
        (x, y), (fx, fy) = g
        for src, f, out in ((w, fx, x), (h, fy, y)):
            k, buf = imgfolder.lanczos_rows(src, f, out)
            n_in, in1 = -(-src // f), float(np.float32(src / f))
            if not T.needs_pass(n_in, in1, out):
                assert (k, buf) == (0, None)
                continue
            bounds, coef = T.lanczos_rows(n_in, in1, out)
            assert k == coef.shape[1] and k <= 25
            assert np.array_equal(buf[:2 * out].reshape(out, 2), bounds), (src, f, out)
            assert np.array_equal(buf[2 * out:].reshape(out, k), coef), (src, f, out)
            axes += 1
    assert axes == 26
    from sais_amd import _lib
    lib = _lib.load()
    assert lib.sais_lanczos_rows(0, 1, 4, None, None, 0) == -1 and lib.sais_lanczos_rows(8, 0, 4, None, None, 0) == -1
    assert lib.sais_lanczos_rows(8, 1, 0, None, None, 0) == -1 and lib.sais_lanczos_rows(65536, 1, 4, None, None, 0) == -1
    buf = np.zeros(64, np.int32)
    assert lib.sais_lanczos_rows(8, 1, 4, buf.ctypes.data, buf[8:].ctypes.data, 12) == -1        # ksize is 13
    assert lib.sais_lanczos_rows(8, 1, 4, buf.ctypes.data, None, 13) == -1


# ------------------------------------------------------------------------------------------------ refusals (no launch: no GPU needed)
def _good():
    """67 x 45 at imsize 16: factors (2, 2), a partial last column and row."""
    from sais_amd import imgfolder
    (x, y), (fx, fy) = T.geometry(67, 45, 16)
    kx, bx = imgfolder.lanczos_rows(67, fx, x)
    ky, by = imgfolder.lanczos_rows(45, fy, y)
    row = (0, 45, 67, fx, fy, 34, 23, 0, x, y, kx, ky, 0, len(bx), 0)
    return row, np.concatenate([bx, by])


def _rep(row, **kw):
    from sais_amd import imgfolder
    d = dict(zip(imgfolder.THUMB_DTYPE.names, row))
    d.update(kw)
    return tuple(d[k] for k in imgfolder.THUMB_DTYPE.names)


def _rc(rows, coef, n=None, src_bytes=1 << 30, ws_bytes=1 << 30, out_elems=1 << 30, coef_ints=None, null=()):
    from sais_amd import _lib, imgfolder
    t = np.array(rows, dtype=imgfolder.THUMB_DTYPE)
    fake = ctypes.c_void_p(4096)                                     # never dereferenced: every case here is refused first
    ptr = {k: (None if k in null else fake) for k in ("src", "table_dev", "coef_dev", "ws", "lut", "out")}
    return _lib.load().sais_thumbnail(ptr["src"], src_bytes, None if "table" in null else t.ctypes.data, ptr["table_dev"],
                                      len(t) if n is None else n, None if "coef" in null else coef.ctypes.data, ptr["coef_dev"],
                                      len(coef) if coef_ints is None else coef_ints, ptr["ws"], ws_bytes, ptr["lut"], ptr["out"],
                                      out_elems, None)


def test_entries_refuse_each_bad_field():
    from sais_amd import _lib, imgfolder
    lib = _lib.load()
    good, coef = _good()
    x, y, kx, ky = good[8], good[9], good[10], good[11]
    assert imgfolder.thumbnail_fits(good)
    bad = [_rep(good, out_w=0), _rep(good, out_h=1025), _rep(good, out_w=1025), _rep(good, src_w=65536, rw=32768),
           _rep(good, src_h=0), _rep(good, fx=0), _rep(good, fy=-1), _rep(good, rw=33), _rep(good, rh=24),
           _rep(good, fx=65535, fy=2, rw=1, rh=23),                                                     # fx * fy above 65536
           _rep(good, src_offset=-1), _rep(good, ws_offset=-1), _rep(good, cx_offset=-1), _rep(good, cy_offset=-1),
           _rep(good, cy_offset=len(coef) - y * (2 + ky) + 1), _rep(good, out_offset=-1), _rep(good, kx=-1), _rep(good, ky=-1),
           _rep(good, kx=0), _rep(good, ky=0),                                                          # a skipped pass keeps the size
           _rep(good, cx_offset=len(coef) - x * (2 + kx) + 1), _rep(good, out_w=1024, ky=60)]            # rows past the buffer; LDS
    for k, row in enumerate(bad):
        assert _rc([good, row], coef) == -1, (k, row)
    geometry_only = [r for r in bad if r[0] == 0 and r[7] == 0 and r[12] == 0 and r[13] == good[13] and r[14] == 0]
    assert len(geometry_only) == 15
    for row in geometry_only:
        assert not imgfolder.thumbnail_fits(row), row
        t = np.array([good, row], dtype=imgfolder.THUMB_DTYPE)
        assert lib.sais_thumbnail_workspace_bytes(t.ctypes.data, 2) == 0 or row[8] == 1024          # the LDS fit is not its business
    assert lib.sais_thumbnail_fits(None) == 0
    # buffers one unit short, n outside 1..65535, null pointers
    assert _rc([good], coef, src_bytes=45 * 67 * 3 - 1) == -1 and _rc([good], coef, ws_bytes=34 * 23 * 3 - 1) == -1
    assert _rc([good], coef, out_elems=3 * x * y - 1) == -1 and _rc([good], coef, coef_ints=len(coef) - 1) == -1
    assert _rc([good], coef, n=0) == -1 and _rc([good], coef, n=65536) == -1 and _rc([good], coef, n=-1) == -1
    for name in ("src", "table", "table_dev", "coef", "coef_dev", "ws", "lut", "out"):
        assert _rc([good], coef, null=(name,)) == -1, name
    # coefficient rows the kernel could not follow: a tap past the reduced image, a negative first index, too many taps, a band
    # whose rows go backwards
    for pos, val in ((2 * (x - 1), 34), (0, -1), (1, kx + 1), (len(coef) - y * (2 + ky), 22), (len(coef) - y * (2 + ky) + 1, 0)):
        c = coef.copy()
        c[pos] = val
        assert _rc([good], c) == -1, (pos, val)
    # the workspace query: the end of the furthest reduced image, never 0 for a valid table
    t = np.array([good, _rep(good, ws_offset=4096)], dtype=imgfolder.THUMB_DTYPE)
    assert lib.sais_thumbnail_workspace_bytes(t.ctypes.data, 2) == 4096 + 34 * 23 * 3
    copy = np.array([(0, 9, 12, 1, 1, 12, 9, 0, 12, 9, 0, 0, 0, 0, 0)], dtype=imgfolder.THUMB_DTYPE)     # untouched: a copy
    assert lib.sais_thumbnail_workspace_bytes(copy.ctypes.data, 1) == 256 and imgfolder.thumbnail_fits(tuple(copy[0]))
    assert lib.sais_thumbnail_workspace_bytes(None, 1) == 0 and lib.sais_thumbnail_workspace_bytes(t.ctypes.data, 0) == 0
    assert lib.sais_thumbnail_workspace_bytes(t.ctypes.data, 65536) == 0
    # the widest output with the largest ksize fits: one-row bands
    wide = (0, 40, 4030, 1, 1, 4030, 40, 0, 1024, 10, 25, 25, 0, 0, 0)
    assert imgfolder.thumbnail_fits(wide) and not imgfolder.thumbnail_fits(_rep(wide, ky=60))


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

    def thumbnail(self, plan, tensors):
        self.tensors = tensors
        return [torch.zeros(1, 3, plan.out_sizes[i][1], plan.out_sizes[i][0]) for i in range(len(plan.items))]


def _jpeg(w, h, seed=0, **kw):
    buf = io.BytesIO()
    Image.fromarray(T.make_image(w, h, seed)).save(buf, "JPEG", **kw)
    return buf.getvalue()


def _items(blobs):
    from sais_amd import jpeg
    out = []
    for i, b in enumerate(blobs):
        h = jpeg.parse_header(b)
        out.append((b, None if h is None else bytes(h), i))
    return out


def test_thumbnail_routing_stats_and_row_cache(monkeypatch):
    from PIL import ImageFile
    from sais_amd import imgfolder
    monkeypatch.setattr(ImageFile, "LOAD_TRUNCATED_IMAGES", False)    # OxfordParisDataset sets it for the process
    gray = io.BytesIO()
    Image.fromarray(T.make_image(50, 70)[:, :, 0]).save(gray, "JPEG")
    whole = _jpeg(128, 96, quality=90)
    blobs = [_jpeg(128, 96, quality=90), _jpeg(96, 128, quality=75), _jpeg(128, 96, seed=1, progressive=True), gray.getvalue(),
             _jpeg(20, 24, quality=75), whole[:len(whole) * 9 // 10], _jpeg(96, 128, seed=3, quality=75),
             _jpeg(6000, 4, quality=30)]
    items = _items(blobs)
    assert [it[1] is None for it in items] == [False, False, True, True, False, False, False, False]
    stub = StubBackend(flag={5})
    loader = imgfolder.GpuImageLoader(backend=stub)
    assert ImageFile.LOAD_TRUNCATED_IMAGES is False
    out = loader.thumbnail(items, 32)
    assert ImageFile.LOAD_TRUNCATED_IMAGES is False                   # set for the call only
    plan = stub.plans[0]
    assert isinstance(plan, imgfolder.BatchPlan) and plan.dtype is imgfolder.THUMB_DTYPE
    assert plan.gpu == [0, 1, 4, 5, 6, 7] and sorted(plan.host) == [2, 3] and plan.pillow == []
    assert stub.uploaded == [(5, (96, 128, 3))]                       # the truncated file, decoded as the dataset decodes it
    assert loader.stats == {"gpu": 5, "unsupported": 2, "failed": 1, "pillow_transform": 0}
    assert [tuple(t.shape) for t in out] == [(1, 3, 24, 32), (1, 3, 32, 24), (1, 3, 24, 32), (1, 3, 32, 23), (1, 3, 24, 20),
                                             (1, 3, 24, 32), (1, 3, 32, 24), (1, 3, 1, 32)]
    # rows: 128 -> 32 and 96 -> 24 serve the landscape and the portrait files; the gray file and the strip add theirs; the small
    # file is untouched and has none
    assert set(loader.row_cache) == {(128, 2, 32), (96, 2, 24), (50, 1, 23), (70, 1, 32), (6000, 93, 32), (4, 2, 1)}
    assert loader.row_cache[(4, 2, 1)][0] == 13 and loader.row_cache[(128, 2, 32)][0] == 13
    rows = dict(plan.rows)
    assert rows[0][10:14] == rows[2][10:14] and rows[1][12] == rows[0][13] and rows[1][13] == rows[0][12]     # shared, swapped
    assert rows[4][3:7] == (1, 1, 20, 24) and rows[4][10:12] == (0, 0)
    assert [rows[i][14] for i in range(8)] == list(np.cumsum([0] + [3 * t.shape[2] * t.shape[3] for t in out[:-1]]))
    assert len(plan.extra) == sum(len(loader.row_cache[k][1]) for k in loader.row_cache)
    # a second batch of the same two shapes computes nothing new
    before = {k: id(v[1]) for k, v in loader.row_cache.items()}
    loader.thumbnail(items[:2] + items[6:7], 32)
    assert {k: id(v[1]) for k, v in loader.row_cache.items()} == before
    assert len(stub.plans[1].extra) == 32 * (2 + 13) + 24 * (2 + 13)
    # a descriptor the fit predicate refuses goes through Pillow's thumbnail itself
    stub2 = StubBackend()
    loader2 = imgfolder.GpuImageLoader(backend=stub2)
    tall = _jpeg(8, 3000, quality=30)
    loader2.thumbnail(_items([blobs[0], tall, blobs[3]]), 2000)
    plan = stub2.plans[0]
    assert plan.gpu == [0] and sorted(plan.host) == [2] and plan.pillow == [1] and plan.out_sizes[1] == (5, 2000)
    assert loader2.stats == {"gpu": 1, "unsupported": 1, "failed": 0, "pillow_transform": 1}
    want = Image.open(io.BytesIO(tall)).convert("RGB")
    want.thumbnail((2000, 2000), Image.LANCZOS)
    assert list(stub2.tensors) == [1] and np.array_equal(stub2.tensors[1].numpy(), T.to_tensor(np.asarray(want)))
    with pytest.raises(ValueError):
        loader.thumbnail([], 32)


def test_tall_narrow_files_go_to_pillow():
    """4 x 600 at imsize 500 -> 3 x 500 without a reduce: Image.resize runs the vertical pass first, which sais_thumbnail does
    not restate.  The library refuses the descriptor and the plan routes the file to Pillow's thumbnail itself."""
    from sais_amd import imgfolder
    assert imgfolder.thumbnail_geometry(4, 600, 500) == ((3, 500), (1, 1)) and imgfolder.thumbnail_vertical_first(4, 600, 500)
    kx, bx = imgfolder.lanczos_rows(4, 1, 3)
    ky, by = imgfolder.lanczos_rows(600, 1, 500)
    row = (0, 600, 4, 1, 1, 4, 600, 0, 3, 500, kx, ky, 0, len(bx), 0)
    assert not imgfolder.thumbnail_fits(row) and _rc([row], np.concatenate([bx, by])) == -1
    assert imgfolder.thumbnail_fits(_rep(row, src_h=400, rh=400, out_h=333))          # 100 times as high: still the GPU's
    tall = _jpeg(4, 600, quality=90)
    stub = StubBackend()
    loader = imgfolder.GpuImageLoader(backend=stub)
    loader.thumbnail(_items([_jpeg(128, 96, quality=90), tall]), 500)
    plan = stub.plans[0]
    assert plan.gpu == [0] and plan.pillow == [1] and plan.out_sizes[1] == (3, 500)
    assert loader.stats == {"gpu": 1, "unsupported": 0, "failed": 0, "pillow_transform": 1}
    want = Image.open(io.BytesIO(tall)).convert("RGB")
    want.thumbnail((500, 500), Image.LANCZOS)
    assert list(stub.tensors) == [1] and np.array_equal(stub.tensors[1].numpy(), T.to_tensor(np.asarray(want)))
    assert (600, 1, 500) not in loader.row_cache                      # no rows were computed for it


def test_row_cache_is_bounded():
    from sais_amd import imgfolder
    c = imgfolder.RowCache(limit=3)
    for k in range(3):
        c[k] = k
    c[1] = "again"
    assert len(c) == 3
    c[9] = 9
    assert dict(c) == {9: 9}
    assert imgfolder.GpuImageLoader(backend=StubBackend()).row_cache.limit == 512


def test_raw_dataset_and_adapters(tmp_path):
    from sais_amd import imgfolder, retrieval
    root = tmp_path / "roxford5k"
    os.makedirs(root / "jpg")
    names = ["b_img", "a_img", "c_img"]
    for k, n in enumerate(names):
        Image.fromarray(T.make_image(40 + 8 * k, 30)).save(str(root / "jpg" / (n + ".jpg")), quality=90)
    with open(root / "gnd_roxford5k.pkl", "wb") as fh:
        pickle.dump({"imlist": names, "qimlist": names[:1], "gnd": [{"easy": [0], "hard": [], "junk": []}]}, fh)
    raw = imgfolder.RawOxfordParis(str(tmp_path), "roxford5k", "train")
    ref = retrieval.OxfordParisDataset(str(tmp_path), "roxford5k", "train", imsize=16)
    assert raw.samples == ref.samples == names and raw.gnd == ref.gnd and len(raw) == 3
    assert len(imgfolder.RawOxfordParis(str(tmp_path), "roxford5k", "query")) == 1
    blob, hdr, idx = raw[2]
    assert idx == 2 and hdr is not None and blob == open(root / "jpg" / "c_img.jpg", "rb").read()

    class Gpu:
        def thumbnail(self, items, imsize):
            return [torch.full((1, 3, 2 + it[2] % 2, 4), float(it[2])) for it in items]
    loader = torch.utils.data.DataLoader(raw, batch_size=3, collate_fn=imgfolder.collate_raw)
    single = list(retrieval.ThumbnailBatches(loader, Gpu(), 16))
    assert [tuple(s.shape) for s, _ in single] == [(1, 3, 2, 4), (1, 3, 3, 4), (1, 3, 2, 4)]
    assert [i.tolist() for _, i in single] == [[0], [1], [2]]
    grouped = list(retrieval.ThumbnailBatches(loader, Gpu(), 16, group_shapes=True))
    assert [tuple(s.shape) for s, _ in grouped] == [(2, 3, 2, 4), (1, 3, 3, 4)]
    assert [i.tolist() for _, i in grouped] == [[0, 2], [1]] and grouped[0][0][1, 0, 0, 0] == 2.0
    assert len(retrieval.ThumbnailBatches(loader, Gpu(), 16)) == 1 and retrieval.ThumbnailBatches(loader, Gpu(), 16).dataset is raw


# ------------------------------------------------------------------------------------------------ the tool's switches
def _tool():
    path = os.path.join(ROOT, "SAIS", "scripts", "dino-main", "eval_image_retrieval.py")
    spec = importlib.util.spec_from_file_location("sais_thumb_eval_image_retrieval", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flags_parse_and_default():
    cli = _tool().get_args_parser()
    a = cli.parse_args([])
    assert a.gpu_loader is False and a.gpu_loader_batch == 64 and a.group_shapes is False
    a = cli.parse_args(["--gpu_loader", "true", "--gpu_loader_batch", "8", "--group_shapes", "true"])
    assert a.gpu_loader is True and a.gpu_loader_batch == 8 and a.group_shapes is True
    with pytest.raises(SystemExit):
        cli.parse_args(["--group_shapes", "maybe"])


def test_group_shapes_needs_the_gpu_loader():
    with pytest.raises(SystemExit) as e:
        _tool().main(["--group_shapes", "true"])
    assert "--gpu_loader true" in str(e.value)
    with pytest.raises(SystemExit):
        _tool().main(["--gpu_loader", "true", "--gpu_loader_batch", "0"])
