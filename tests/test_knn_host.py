"""CPU-only: host side of the weighted k-NN evaluation (dataset listing, eval transform, checkpoint handling, the fp64
oracle against the reference's recorded counts, argument checks of the new entry points)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_image_folder_listing(tmp_path):
    from sais_amd.knn import list_image_folder
    for c, files in (("zebra", ["b.JPG", "a.png", "notes.txt"]), ("ant", ["2.jpeg", "10.jpg"]), ("bee", [])):
        (tmp_path / c).mkdir()
        for f in files:
            (tmp_path / c / f).write_bytes(b"x")
    (tmp_path / "ant" / "sub").mkdir()
    (tmp_path / "ant" / "sub" / "0.bmp").write_bytes(b"x")
    (tmp_path / "stray.jpg").write_bytes(b"x")
    classes, samples = list_image_folder(str(tmp_path))
    assert classes == ["ant", "bee", "zebra"]
    rel = [(os.path.relpath(p, tmp_path), l) for p, l in samples]
    assert rel == [("ant/10.jpg", 0), ("ant/2.jpeg", 0), ("ant/sub/0.bmp", 0), ("zebra/a.png", 2), ("zebra/b.JPG", 2)]
    with pytest.raises(FileNotFoundError):
        list_image_folder(str(tmp_path / "bee"))


def test_eval_transform_geometry_and_output():
    from PIL import Image
    from sais_amd.knn import EvalImageFolder, eval_transform_geometry
    assert eval_transform_geometry(1280, 720) == ((455, 256), (116, 16))
    assert eval_transform_geometry(720, 1280) == ((256, 455), (16, 116))
    assert eval_transform_geometry(224, 224) == ((256, 256), (16, 16))
    assert eval_transform_geometry(96, 72) == ((341, 256), (58, 16))
    rng = np.random.default_rng(0)
    img = Image.fromarray(rng.integers(0, 256, (72, 96, 3), dtype=np.uint8))
    out = EvalImageFolder.transform(img)
    assert out.shape == (3, 224, 224) and out.dtype == torch.float32
    want = np.asarray(img.resize((341, 256), Image.BICUBIC).crop((58, 16, 282, 240)), dtype=np.float32) / 255.0
    want = (want - np.float32([0.485, 0.456, 0.406])) / np.float32([0.229, 0.224, 0.225])
    assert np.array_equal(out.numpy(), want.transpose(2, 0, 1))
    gray = EvalImageFolder.transform(Image.fromarray(rng.integers(0, 256, (300, 300), dtype=np.uint8)))      # mode L -> RGB
    assert gray.shape == (3, 224, 224)


def test_checkpoint_key_and_prefixes():
    from sais_amd.knn import backbone_state_dict
    w = {"cls_token": torch.zeros(1), "blocks.0.attn.qkv.weight": torch.ones(2)}
    ckpt = {"student": {"module.backbone." + k: v + 1 for k, v in w.items()} | {"module.head.mlp.0.weight": torch.zeros(1)},
            "teacher": {"backbone." + k: v for k, v in w.items()} | {"head.mlp.0.weight": torch.zeros(1)}, "epoch": 3}
    t = backbone_state_dict(ckpt, "teacher")
    assert set(t) == set(w) | {"head.mlp.0.weight"} and all(torch.equal(t[k], w[k]) for k in w)
    s = backbone_state_dict(ckpt, "student")
    assert set(s) == set(w) | {"head.mlp.0.weight"} and all(torch.equal(s[k], w[k] + 1) for k in w)
    assert backbone_state_dict(w, "teacher") == w                    # a bare backbone state_dict
    assert backbone_state_dict({"module." + k: v for k, v in w.items()}, None).keys() == w.keys()


def test_cli_flags_match_the_reference():
    path = os.path.join(ROOT, "SAIS", "scripts", "dino-main", "eval_knn.py")
    spec = importlib.util.spec_from_file_location("sais_eval_knn", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ns = mod.get_args_parser().parse_args([])
    want = dict(batch_size_per_gpu=128, nb_knn=[10, 20, 100, 200], temperature=0.07, pretrained_weights='', use_cuda=True,
                arch='vit_small', patch_size=16, checkpoint_key='teacher', dump_features=None, load_features=None, num_workers=10,
                dist_url='env://', local_rank=0, data_path='/path/to/imagenet/')
    assert vars(ns) == want
    ns = mod.get_args_parser().parse_args(["--arch", "vit_base"])
    with pytest.raises(NotImplementedError, match="--arch vit_small --patch_size 16"):
        mod.build_model(ns, "cpu")


@pytest.mark.parametrize("name", [c[0] for c in knn_ref.GOLDEN_CASES])
def test_fp64_oracle_reproduces_reference_counts(golden, name):
    """guards the oracle itself: knn_ref.classify against the reference's recorded counts, within the fragile-row bound"""
    g = golden("knn")
    _, nt, nq, C, D, noise, seed = next(c for c in knn_ref.GOLDEN_CASES if c[0] == name)
    train, tl, test, sl = knn_ref.make_case(nt, nq, C, D, noise, seed)
    assert (knn_ref.digest(train, tl, test, sl) == g[f"{name}_sha256"]).all(), "generated inputs differ from the recorded ones"
    s = knn_ref.similarities(test, train)
    for j, k in enumerate(knn_ref.KS):
        nfrag = int(knn_ref.fragile_rows(s, tl, sl, k, C).sum())
        assert nfrag <= knn_ref.FRAGILE_CAP * nq
        top1, top5 = knn_ref.classify(s, tl, sl, k, C)
        ref = g[f"{name}_counts"][j]
        assert abs(top1 - ref[0]) <= nfrag and abs(top5 - ref[1]) <= nfrag, (k, top1, top5, ref, nfrag)


def test_new_entries_reject_bad_arguments():
    from sais_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    ks = (ctypes.c_int * 2)(10, 20)
    assert lib.sais_knn_search(None, None, 0, 4, 100, 384, 10, None, None, None, 0, None) == -1
    big = 1 << 40
    for nq, nt, d, k in ((0, 100, 384, 10), (4, 100, 384, 101), (4, 1000, 384, 257), (4, 100, 100, 10), (4, 100, 1600, 10),
                         (4, 100, 384, 0)):
        assert lib.sais_knn_search(p, p, 1, nq, nt, d, k, p, p, p, big, None) == -1, (nq, nt, d, k)
    assert lib.sais_knn_search(p, p, 1, 4, 100, 384, 10, p, p, p, 8, None) == -1            # workspace too small
    assert lib.sais_knn_vote(None, None, 4, 20, None, 100, 10, 0.07, ks, 2, None, None, None) == -1
    assert lib.sais_knn_vote(p, p, 4, 20, p, 100, 4097, 0.07, ks, 2, p, None, None) == -1  # num_classes
    assert lib.sais_knn_vote(p, p, 4, 20, p, 100, 10, 0.0, ks, 2, p, None, None) == -1     # T
    assert lib.sais_knn_vote(p, p, 4, 10, p, 100, 10, 0.07, ks, 2, p, None, None) == -1    # k_m > kmax
    assert lib.sais_knn_vote(p, p, 4, 20, p, 100, 10, 0.07, (ctypes.c_int * 2)(20, 10), 2, p, None, None) == -1
    assert lib.sais_knn_vote(p, p, 4, 20, p, 100, 10, 0.07, (ctypes.c_int * 9)(*range(1, 10)), 9, p, None, None) == -1
    assert lib.sais_knn_vote(p, p, 4, 20, p, 100, 10, 0.07, None, 2, p, None, None) == -1


def test_workspace_bytes():
    from sais_amd import _lib
    ws = _lib.load().sais_knn_workspace_bytes
    assert ws(0, 100, 10) == 0 and ws(4, 100, 101) == 0 and ws(4, 1000, 257) == 0
    for nt in (1000, 65536, 1281167):
        sizes = [ws(nq, nt, 200) for nq in (1, 2, 100, 128, 129, 1000, 1024, 1025, 8192, 50000, 50001)]
        assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    # the split count is capped: past that, the size does not depend on Nt
    for nq in (1, 229, 8192, 50000):
        assert ws(nq, 65536, 200) == ws(nq, 1281167, 200) == ws(nq, 1 << 30, 200)
        assert ws(nq, 65536, 200) >= nq * 200 * 8
    assert ws(50000, 1281167, 200) <= 50000 * 512 * 8               # O(kmax) entries per row once one split fills the GPU
    assert ws(229, 1281167, 100) < ws(229, 1281167, 200)
