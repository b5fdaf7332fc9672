"""GPU: sais_thumbnail (csrc/thumbnail.hip) against Pillow bit for bit, the reduce kernel alone against Image.reduce,
GpuImageLoader.thumbnail against retrieval.OxfordParisDataset item for item, and eval_image_retrieval.py with --gpu_loader
(identical features and result lines) and --group_shapes (both dumps under the feature bar of tests/test_retrieval_gpu.py).

Every expected value is Pillow's own (Image.thumbnail, Image.reduce) through the dataset's ToTensor + Normalize; the comparisons
are torch.equal.  The numpy restatement these kernels follow is held against Pillow in tests/test_thumbnail_host.py."""
import functools
import io
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity  # noqa: E402
import retrieval_ref as R  # noqa: E402
import thumb_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
PAIRS = [(fx, fy) for fx in range(1, 9) for fy in range(1, 9)]


# ------------------------------------------------------------------------------------------------ one launch over raw arrays
def _thumb_row(w, h, imsize, rows, words):
    """(THUMB_DTYPE row without offsets, (x, y)) of a w x h image; appends the axis rows it needs to `words` (key -> offset in
    `rows`)."""
    from sais_amd import imgfolder
    g = imgfolder.thumbnail_geometry(w, h, imsize)
    (x, y), (fx, fy) = g if g is not None else ((w, h), (1, 1))

    def axis(src, f, out):
        if g is None:
            return 0, 0
        key = (src, f, out)
        if key not in rows:
            k, buf = imgfolder.lanczos_rows(*key)
            rows[key] = (k, sum(len(b) for b in words))
            if k:
                words.append(buf)
        return rows[key]
    (kx, cx), (ky, cy) = axis(w, fx, x), axis(h, fy, y)
    return [0, h, w, fx, fy, -(-w // fx), -(-h // fy), 0, x, y, kx, ky, cx, cy, 0], (x, y)


def _launch(images, table_rows, sizes, order, words, lut=None):
    """One sais_thumbnail launch: image i writes output slot order[i] (slots packed in slot order).  -> [float32 [3,h,w]]."""
    from sais_amd import _lib as L, imgfolder
    n = len(images)
    elems = [3 * x * y for x, y in sizes]
    slot_off = {}
    off = 0
    for slot in range(n):
        i = order.index(slot)
        slot_off[i] = off
        off += elems[i]
    total = off
    src_off = ws_off = 0
    for i, (img, row) in enumerate(zip(images, table_rows)):
        row[0], row[7], row[14] = src_off, ws_off, slot_off[i]
        src_off += (img.size + 255) // 256 * 256
        if row[3] > 1 or row[4] > 1:
            ws_off += (3 * row[5] * row[6] + 255) // 256 * 256
    table = np.array([tuple(r) for r in table_rows], dtype=imgfolder.THUMB_DTYPE)
    src = np.zeros(src_off, np.uint8)
    for img, row in zip(images, table_rows):
        src[row[0]:row[0] + img.size] = img.reshape(-1)
    coef = np.concatenate(words) if words else np.zeros(1, np.int32)
    need = L.load().sais_thumbnail_workspace_bytes(table.ctypes.data, n)
    assert need >= max(ws_off - 255, 256) and need <= max(ws_off, 256)
    src_d = torch.from_numpy(src).to(DEV)
    table_d = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)
    coef_d = torch.from_numpy(coef).to(DEV)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    lut_d = torch.from_numpy(imgfolder.normalize_table() if lut is None else lut).to(DEV)
    out = torch.full((total + 64,), float("nan"), dtype=torch.float32, device=DEV)          # 64 floats no image owns
    L.call("sais_thumbnail", src_d.data_ptr(), src_d.numel(), table.ctypes.data, table_d.data_ptr(), n, coef.ctypes.data,
           coef_d.data_ptr(), coef.size, ws.data_ptr(), ws.numel(), lut_d.data_ptr(), out.data_ptr(), total,
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[total:]).all(), "wrote past the last slot"
    assert not torch.isnan(out[:total]).any(), "an output element was not written"
    return [out[slot_off[i]:slot_off[i] + elems[i]].view(3, sizes[i][1], sizes[i][0]) for i in range(n)]


def _run_thumbnail(images, imsizes, order=None):
    rows, words, table_rows, sizes = {}, [], [], []
    for img, s in zip(images, imsizes):
        row, size = _thumb_row(img.shape[1], img.shape[0], s, rows, words)
        table_rows.append(row)
        sizes.append(size)
    return _launch(images, table_rows, sizes, list(range(len(images))) if order is None else order, words)


def _want(img, imsize):
    """The dataset's sample of a decoded image: thumbnail(LANCZOS), ToTensor, Normalize."""
    from sais_amd.retrieval import _to_tensor
    p = Image.fromarray(img)
    p.thumbnail((imsize, imsize), Image.LANCZOS)
    return _to_tensor(p)


@functools.lru_cache(maxsize=None)
def _list_case():
    images = [T.make_image(w, h) for w, h, _ in T.GEOMETRIES]
    return images, [s for _, _, s in T.GEOMETRIES], [_want(img, s) for img, (_, _, s) in zip(images, T.GEOMETRIES)]


# ------------------------------------------------------------------------------------------------ kernels
def test_reduce_kernel_matches_image_reduce():
    """The reduce kernel alone: both resample passes skipped (out = the reduced size) and the identity as the table, so the
    floats are the reduced bytes.  Every factor pair in 1..8 x 1..8 on a multiple and a non-multiple size, and (16, 16) on
    130 x 97, in one launch."""
    cases = [(fx, fy, fx * 6, fy * 5) for fx, fy in PAIRS] + [(fx, fy, fx * 6 + fx // 2, fy * 5 + fy - 1) for fx, fy in PAIRS]
    cases.append((16, 16, 130, 97))
    images = [T.make_image(w, h, seed=1) for _, _, w, h in cases]
    table_rows = [[0, h, w, fx, fy, -(-w // fx), -(-h // fy), 0, -(-w // fx), -(-h // fy), 0, 0, 0, 0, 0] for fx, fy, w, h in cases]
    sizes = [(r[8], r[9]) for r in table_rows]
    lut = np.tile(np.arange(256, dtype=np.float32), (3, 1))
    got = _launch(images, table_rows, sizes, list(range(len(cases))), [], lut=lut)
    for (fx, fy, w, h), img, g in zip(cases, images, got):
        want = np.asarray(Image.fromarray(img).reduce((fx, fy)))
        assert np.array_equal(g.numpy().transpose(1, 2, 0), want.astype(np.float32)), (fx, fy, w, h)


def test_thumbnail_list_in_one_launch_with_permuted_slots():
    images, imsizes, want = _list_case()
    n = len(images)
    order = [(7 * i + 3) % n for i in range(n)]
    assert sorted(order) == list(range(n))
    got = _run_thumbnail(images, imsizes, order)
    for whs, g, w in zip(T.GEOMETRIES, got, want):
        assert g.shape == w.shape and torch.equal(g, w), whs


@pytest.mark.parametrize("k", range(len(T.GEOMETRIES)), ids=["%dx%d_%d" % g for g in T.GEOMETRIES])
def test_thumbnail_each_alone(k):
    images, imsizes, want = _list_case()
    got = _run_thumbnail([images[k]], [imsizes[k]])[0]
    assert got.shape == want[k].shape and torch.equal(got, want[k])


def test_thumbnail_widest_output_smallest_band():
    """4030 x 15 -> 1024 x 4: factors 1, ksize 25 on both axes, the widest line the entry takes: one-row bands of 27 lines
    (83 KiB of LDS)."""
    from sais_amd import _lib as L, imgfolder
    assert L.THUMB_MAX_OUT == 1024
    assert imgfolder.thumbnail_geometry(4030, 15, 1024) == ((1024, 4), (1, 1))
    assert imgfolder.lanczos_rows(4030, 1, 1024)[0] == 25 and imgfolder.lanczos_rows(15, 1, 4)[0] == 25
    img = T.make_image(4030, 15, seed=4)
    got = _run_thumbnail([img], [1024])[0]
    assert torch.equal(got, _want(img, 1024))


# ------------------------------------------------------------------------------------------------ loader
# name -> (w, h, save options); the last three are off the GPU decode path.  At imsize 96 every thumbnail keeps a side of
# 16 or more (the tool's backbone needs one whole patch), and land1 / prog / trunc share the shape 96 x 72
FOLDER = [("land0", 200, 150, dict(quality=90)), ("port0", 150, 200, dict(quality=75)),
          ("land1", 200, 150, dict(quality=75, subsampling=0)), ("port1", 150, 200, dict(quality=90, subsampling=2)),
          ("small", 24, 20, dict(quality=90)), ("mid", 80, 60, dict(quality=85, subsampling=1)),
          ("rst", 203, 151, dict(quality=75, restart_marker_blocks=3)), ("odd", 131, 197, dict(quality=60, subsampling=0)),
          ("wide", 260, 48, dict(quality=80)), ("prog", 200, 150, dict(quality=80, progressive=True)),
          ("gray", 90, 130, dict(quality=80)), ("trunc", 200, 150, dict(quality=90))]
OFF_GPU = ("prog", "gray", "trunc")


def _write_roxford(root):
    d = os.path.join(root, "roxford5k", "jpg")
    os.makedirs(d)
    for k, (name, w, h, kw) in enumerate(FOLDER):
        img = T.make_image(w, h, seed=10 + k)
        buf = io.BytesIO()
        Image.fromarray(img[:, :, 0] if name == "gray" else img).save(buf, "JPEG", **kw)
        blob = buf.getvalue()
        with open(os.path.join(d, name + ".jpg"), "wb") as fh:
            fh.write(blob[:len(blob) * 19 // 20] if name == "trunc" else blob)          # cut inside its last tenth
    names = [f[0] for f in FOLDER]
    cfg = {"imlist": names[2:], "qimlist": names[:2],
           "gnd": [{"easy": [0, 4], "hard": [6], "junk": [5]}, {"easy": [1], "hard": [5, 7], "junk": []}]}
    with open(os.path.join(root, "roxford5k", "gnd_roxford5k.pkl"), "wb") as fh:
        pickle.dump(cfg, fh)
    return cfg


@pytest.fixture(scope="module")
def roxford(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("thumb_data"))
    return root, _write_roxford(root)


@pytest.mark.parametrize("imsize", [32, 96])
def test_loader_equals_the_pillow_dataset(roxford, imsize):
    from sais_amd import imgfolder
    from sais_amd.retrieval import OxfordParisDataset
    root, cfg = roxford
    loader = imgfolder.GpuImageLoader(DEV)
    for split, names in (("train", cfg["imlist"]), ("query", cfg["qimlist"])):
        raw = imgfolder.RawOxfordParis(root, "roxford5k", split)
        ref = OxfordParisDataset(root, "roxford5k", split, imsize=imsize)
        assert raw.samples == ref.samples == names
        items, tags = imgfolder.collate_raw([raw[i] for i in range(len(raw))])
        assert [it[1] is None for it in items] == [n in ("prog", "gray") for n in names]
        got = loader.thumbnail(items, imsize)
        plan = loader.last_plan
        assert plan.pillow == [] and sorted(plan.host) == [i for i, n in enumerate(names) if n in ("prog", "gray")]
        for i, g in enumerate(got):
            want, idx = ref[i]
            assert int(tags[i]) == idx == i
            assert tuple(g.shape) == (1,) + tuple(want.shape), names[i]
            assert torch.equal(g[0].cpu(), want), (names[i], imsize)
    # exactly the progressive, the grayscale and the truncated file left the GPU decode path
    assert loader.stats == {"gpu": len(FOLDER) - 3, "unsupported": 2, "failed": 1, "pillow_transform": 0}
    # two landscape / portrait shapes, a restart interval, odd sizes and a strip: eight distinct axes plus the gray file's
    assert len(loader.row_cache) >= 8 and all(k <= 25 for k, _ in loader.row_cache.values())


def test_loader_hands_tall_narrow_files_to_pillow(tmp_path):
    """4 x 600 at imsize 500: Image.resize runs the vertical pass first; the loader's item still equals the dataset's."""
    from sais_amd import imgfolder
    from sais_amd.retrieval import OxfordParisDataset
    d = tmp_path / "roxford5k" / "jpg"
    os.makedirs(d)
    Image.fromarray(T.make_image(4, 600, seed=5)).save(str(d / "tall.jpg"), quality=90)
    Image.fromarray(T.make_image(4, 400, seed=5)).save(str(d / "less.jpg"), quality=90)          # exactly 100 : 1 stays on the GPU
    with open(tmp_path / "roxford5k" / "gnd_roxford5k.pkl", "wb") as fh:
        pickle.dump({"imlist": ["tall", "less"], "qimlist": ["tall"], "gnd": [{"easy": [0], "hard": [], "junk": []}]}, fh)
    raw = imgfolder.RawOxfordParis(str(tmp_path), "roxford5k", "train")
    ref = OxfordParisDataset(str(tmp_path), "roxford5k", "train", imsize=333)
    loader = imgfolder.GpuImageLoader(DEV)
    got = loader.thumbnail([raw[0], raw[1]], 333)
    assert loader.last_plan.pillow == [0] and loader.stats == {"gpu": 1, "unsupported": 0, "failed": 0, "pillow_transform": 1}
    for i in range(2):
        assert torch.equal(got[i][0].cpu(), ref[i][0]), i


def test_folder_has_the_files_it_says(roxford, monkeypatch):
    from sais_amd import jpeg
    root, _ = roxford
    d = os.path.join(root, "roxford5k", "jpg")
    hdr = {n: jpeg.parse_header(open(os.path.join(d, n + ".jpg"), "rb").read()) for n, _, _, _ in FOLDER}
    assert hdr["prog"] is None and hdr["gray"] is None and hdr["trunc"] is not None
    assert hdr["rst"].restart_interval == 3 and hdr["land0"].restart_interval == 0
    from PIL import ImageFile
    monkeypatch.setattr(ImageFile, "LOAD_TRUNCATED_IMAGES", False)      # OxfordParisDataset sets it for the process
    with pytest.raises(OSError):
        Image.open(os.path.join(d, "trunc.jpg")).convert("RGB")        # truncated for Pillow too
    ss = {n: (hdr[n].hsamp, hdr[n].vsamp) for n in ("land0", "land1", "port1", "mid")}
    assert ss == {"land0": (2, 2), "land1": (1, 1), "port1": (2, 2), "mid": (2, 1)}          # 4:2:0 (Pillow's default), 4:4:4, 4:2:0, 4:2:2
    assert Image.open(os.path.join(d, "small.jpg")).size == (24, 20)                      # below both imsizes: untouched


# ------------------------------------------------------------------------------------------------ tool
def _run_tool(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "SAIS", "scripts", "dino-main", "eval_image_retrieval.py"),
                        "--num_workers", "0", *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@functools.lru_cache(maxsize=None)
def backbone():
    from sais_amd.vit import vit_small
    torch.manual_seed(7)
    return vit_small(patch_size=16, num_classes=0).to(DEV).eval()


@pytest.fixture(scope="module")
def tool_runs(roxford, tmp_path_factory):
    """The four legs of the tool at --imsize 96 on the synthetic folder, with the weights of backbone() as the checkpoint:
    the Pillow loader twice (A/A), --gpu_loader, --gpu_loader --group_shapes.  -> {leg: (stdout, trainfeat, queryfeat)}."""
    root, _ = roxford
    work = tmp_path_factory.mktemp("thumb_tool")
    ckpt = str(work / "ckpt.pth")
    torch.save({"teacher": {k: v.cpu() for k, v in backbone().state_dict().items()}}, ckpt)
    legs = {"pillow_a": [], "pillow_b": [], "gpu": ["--gpu_loader", "true", "--gpu_loader_batch", "5"],
            "grouped": ["--gpu_loader", "true", "--gpu_loader_batch", "5", "--group_shapes", "true"]}
    out = {}
    for leg, extra in legs.items():
        dump = str(work / leg)
        text = _run_tool("--data_path", root, "--dataset", "roxford5k", "--imsize", "96", "--pretrained_weights", ckpt,
                         "--dump_features", dump, *extra)
        out[leg] = (text, torch.load(os.path.join(dump, "trainfeat.pth")), torch.load(os.path.join(dump, "queryfeat.pth")))
    return out


def test_tool_gpu_loader_gives_the_pillow_loaders_features(tool_runs):
    """The Pillow leg twice tells whether the backbone is bit-reproducible run to run on identical input.  On the MI355X it
    is (no atomics on the extraction path): A/A is torch.equal, so the --gpu_loader dump must be torch.equal too and the
    `>>` lines identical strings.  Should A/A ever differ, the comparison is to that A/A difference."""
    (ta, tra, qa), (tb, trb, qb), (tg, trg, qg) = tool_runs["pillow_a"], tool_runs["pillow_b"], tool_runs["gpu"]
    assert "loaded with msg" in ta and "train: 10 imgs / query: 2 imgs" in ta and "gpu loader:" not in ta
    lines = lambda t: re.findall(r"^>> .*$", t, flags=re.M)           # noqa: E731
    assert len(lines(ta)) == 2
    aa = max(float((tra - trb).abs().max()), float((qa - qb).abs().max()))
    ag = max(float((tra - trg).abs().max()), float((qa - qg).abs().max()))
    print(f"A/A max difference {aa:.3e}; Pillow vs --gpu_loader {ag:.3e}")
    parity.parity_log("thumbnail_tool_gpu_loader_vs_pillow_abs", ag, aa)
    if aa == 0.0:
        assert torch.equal(tra, trg) and torch.equal(qa, qg)
        assert lines(ta) == lines(tb) == lines(tg)
    else:
        assert ag <= aa
    assert "gpu loader: {'gpu': 9, 'unsupported': 2, 'failed': 1, 'pillow_transform': 0}" in tg


def test_tool_group_shapes(tool_runs):
    """--group_shapes: every row of the grouped dump is nearest, by cosine, to its own row of the per-image dump, and the
    largest grouped-versus-single difference is logged (measured on the MI355X: 0.0, the dumps are bit-identical)."""
    (_, trg, qg), (tgr, trr, qr) = tool_runs["gpu"], tool_runs["grouped"]
    assert "gpu loader: {'gpu': 9, 'unsupported': 2, 'failed': 1, 'pillow_transform': 0}" in tgr
    single, grouped = torch.cat([trg, qg]).double(), torch.cat([trr, qr]).double()
    cos = grouped @ single.T
    assert cos.argmax(1).tolist() == list(range(len(single)))
    diff = float((grouped - single).abs().max())
    print(f"grouped vs per-image dump: max |d| = {diff:.3e}, min own cosine {float(cos.diag().min()):.9f}")
    parity.parity_log("thumbnail_grouped_vs_single_dump_abs", diff, 0.0)      # a logged figure: no bar is asserted


def test_group_shapes_dumps_within_the_feature_bar(tool_runs, roxford):
    """Both dumps of the tool (per image and --group_shapes) against the fp64 reference of tests/retrieval_ref.py on the same
    thumbnails, under the bar rule of tests/test_retrieval_gpu.py::test_retrieval_features: the largest relative error is at
    most 4 x that of the same expression evaluated in numpy f32.  A dump row is the L2-normalised CLS row of the final norm,
    so the reference is unit_rows(gem_from_normed(dense_features)[:, :384]) in fp64 and the f32 yardstick is the same
    normalisation in numpy f32 from the same CLS row.  The measure is well posed at any token count: a quotient x_i / |x| has
    a relative error of a few roundoffs whatever the size of x_i.  (The GeM half of retrieval_features, which
    test_retrieval_features also bounds, is not in the dumps: the tool asks for cls_only.)"""
    from sais_amd import imgfolder
    from sais_amd.retrieval import crop_to_patches
    root, _ = roxford
    model, D = backbone(), 384
    loader = imgfolder.GpuImageLoader(DEV)
    cls, ref = [], []
    for split in ("train", "query"):                                  # the order of the dumps
        raw = imgfolder.RawOxfordParis(root, "roxford5k", split)
        for t in loader.thumbnail([raw[i] for i in range(len(raw))], 96):
            tokens = model.dense_features(crop_to_patches(t), 1)[0].cpu().numpy()          # [1, ntok, 384] f32
            cls.append(tokens[:, 0])
            ref.append(R.gem_from_normed(tokens)[:, :D])
    cls, ref = np.concatenate(cls), R.unit_rows(np.concatenate(ref))
    x = cls
    f32 = x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True, dtype=np.float32)), np.float32(1e-12))
    assert f32.dtype == np.float32
    rel = lambda a: float((np.abs(a.astype(np.float64) - ref) / np.abs(ref)).max())       # noqa: E731
    bar = 4 * rel(f32)
    for leg in ("gpu", "grouped"):
        _, tr, q = tool_runs[leg]
        got = rel(torch.cat([tr, q]).numpy())
        print(f"dump {leg}: max relative error {got:.3e}, numpy f32 {bar / 4:.3e}, bar {bar:.3e}")
        parity.parity_log(f"thumbnail_dump_{leg}_cls_rel", got, bar)
        assert got <= bar, leg
