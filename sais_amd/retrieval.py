"""Copy detection (dino-main/eval_copy_detection.py, Copydays) and image retrieval (dino-main/eval_image_retrieval.py, revisited
Oxford / Paris) with a DINO backbone as the descriptor, on the HIP kernels of csrc/retrieval.hip.

Device side: `VisionTransformer.retrieval_features` (CLS | GeM descriptor), `PCAWhitening` (sais_colmean_cov, sais_center_rows,
sais_probe_logits, sais_l2norm_fwd), `copy_detection_topk` (KnnIndex.search: no [Nq, Ndb] matrix), `rank_positions`
(sais_rank_positions: the positions of the listed positives and junk images, instead of an argsort of the whole database),
`multi_scale` (sais_resize_bilinear_f32).  Host side, in fp64 as the reference: the eigendecomposition of the whitening matrix
(np.linalg.eigh), both average-precision formulas, `copydays_map`, `compute_map`.  Host tensors raise: there is no CPU fallback.

Frames whose sides are not multiples of the patch size (16; 8 on a ViT-S/8 backbone) are cropped at the right and bottom to the multiple below (`crop_to_patches`).  That is
exactly what the reference computes: its strided convolution drops the remainder and `interpolate_pos_encoding` uses
`w // patch_size`, so the pixels past the last whole patch never reach a token.
"""
import os
import pickle

import numpy as np
import torch

from . import _lib as L
from . import ops
from .knn import KnnIndex

PATCH = 16
SCALES = (1, 1 / 2 ** (1 / 2), 1 / 2)                    # utils.multi_scale
COPYDAYS_BLOCKS = (["original", "strong"] + ["jpegqual/%d" % i for i in (3, 5, 8, 10, 15, 20, 30, 50, 75)]
                   + ["crops/%d" % i for i in (10, 15, 20, 30, 40, 50, 60, 70, 80)])
IMG_EXTENSIONS = ("jpg", "jpeg", "png", "ppm", "bmp", "pgm", "tif", "tiff", "webp")       # is_image_file
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _device_matrix(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.SaisHipError(f"{name}: expected a device tensor (the retrieval path has no CPU fallback)")
    if t.dim() != 2 or t.shape[0] < 1:
        raise ValueError(f"{name}: expected [N, D], got {tuple(t.shape)}")
    return t.float().contiguous()


def _l2norm(x, out):
    if x.shape[1] % 4 or x.shape[1] > 1024:
        raise ValueError(f"rows of {x.shape[1]} floats: sais_l2norm_fwd takes a multiple of 4, at most 1024")
    ops.l2norm_fwd(x, out, torch.empty(x.shape[0], dtype=torch.float32, device=x.device))
    return out


# ------------------------------------------------------------------------------------------------------------ frames
def cropped_size(h, w, patch=PATCH):
    """(h, w) cut down to multiples of the patch size; a side below one patch raises."""
    if h < patch or w < patch:
        raise ValueError(f"a {h} x {w} frame holds no whole {patch} x {patch} patch")
    return h // patch * patch, w // patch * patch


def crop_to_patches(x, patch=PATCH):
    """x [F, 3, H, W] without the right and bottom remainders of H and W modulo the patch size (see the module docstring)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("expected [F, 3, H, W]")
    h, w = cropped_size(x.shape[2], x.shape[3], patch)
    return x if (h, w) == tuple(x.shape[2:]) else x[:, :, :h, :w].contiguous()


def scaled_size(h, w, s):
    """Output size of F.interpolate(scale_factor=s): floor of the product in double."""
    return int(np.floor(float(h) * s)), int(np.floor(float(w) * s))


def resize_bilinear(x, s):
    """F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False) on a device tensor f32 [F, 3, H, W]."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise L.SaisHipError("resize_bilinear: expected a device tensor (no CPU fallback)")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected [F, 3, H, W], got {tuple(x.shape)}")
    x = x.float().contiguous()
    ho, wo = scaled_size(x.shape[2], x.shape[3], s)
    if ho < 1 or wo < 1:
        raise ValueError(f"scale {s} leaves nothing of a {x.shape[2]} x {x.shape[3]} frame")
    y = torch.empty(x.shape[0], 3, ho, wo, dtype=torch.float32, device=x.device)
    ops.resize_bilinear(x, s, y)
    return y


@torch.no_grad()
def multi_scale(samples, model):
    """utils.multi_scale (utils.py:816-830): the mean of model(.) over the scales 1, 1/sqrt(2), 1/2 of `samples`, divided by the
    norm of the WHOLE result tensor, as the reference does.  Each scale is cropped to multiples of the patch size (model.patch
    where the callable carries it, as those of cls_features / descriptor_features do; else 16) before `model` sees it.
    model: a callable on device frames f32 [F, 3, H, W] (`cls_features(vit)` for the retrieval evaluation).
    samples a LIST of such tensors of different sizes (model must take a list: cls_features on a patch-16 backbone): all three
    scales of all items go through the backbone in ONE call (3 n items); row block i of the result is the mean over the scales
    of item i divided by the norm of that block alone, which is what the reference computes at its batch size of 1 (the
    whole-batch norm of the stacked form does not appear).  The two rescaling launches per item stay per item."""
    if isinstance(samples, (list, tuple)):
        return _multi_scale_list(samples, model)
    if not isinstance(samples, torch.Tensor) or not samples.is_cuda:
        raise L.SaisHipError("multi_scale: expected a device tensor (no CPU fallback)")
    frames = samples.float().contiguous()
    patch = getattr(model, "patch", PATCH)
    feats = [model(crop_to_patches(frames if s == 1 else resize_bilinear(frames, s), patch)) for s in SCALES]
    mean = torch.stack(feats).sum(0) / len(SCALES)
    return mean / mean.norm()


def _multi_scale_list(samples, model):
    if len(samples) == 0:
        raise ValueError("multi_scale: an empty list of frames")
    patch = getattr(model, "patch", PATCH)
    views = []
    for x in samples:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise L.SaisHipError("multi_scale: expected device tensors (no CPU fallback)")
        frames = x.float().contiguous()
        views += [crop_to_patches(frames if s == 1 else resize_bilinear(frames, s), patch) for s in SCALES]
    feats = model(views)                                  # [sum over items of 3 F_i, D], item-major, scale, frame
    out, row = torch.empty(sum(x.shape[0] for x in samples), feats.shape[1], dtype=torch.float32, device=feats.device), 0
    for i, x in enumerate(samples):
        Fr = x.shape[0]
        mean = feats[3 * row:3 * (row + Fr)].view(len(SCALES), Fr, -1).sum(0) / len(SCALES)
        out[row:row + Fr] = mean / mean.norm()
        row += Fr
    return out


def cls_features(vit):
    """model(x) of the reference at any resolution: the CLS token of the final norm, f32 [F, 384] (the first half of
    retrieval_features, bit for bit), of the frames cropped to whole patches.  Only the final LayerNorm of the CLS rows runs
    after the blocks: the GeM pass over the patch rows is not computed.  A list of frames of different sizes goes through the
    backbone in one segmented pass (VisionTransformer.retrieval_features on a list): f32 [sum F, 384] in list order."""
    def fn(x):
        if isinstance(x, (list, tuple)):
            return vit.retrieval_features([crop_to_patches(t, fn.patch) for t in x], cls_only=True)
        return vit.retrieval_features(crop_to_patches(x, fn.patch), cls_only=True)
    fn.patch = vit.patch_embed.patch_size
    return fn


def descriptor_features(vit):
    """The Copydays descriptor f32 [F, 768] of the frames cropped to whole patches."""
    fn = lambda x: vit.retrieval_features(crop_to_patches(x, fn.patch))
    fn.patch = vit.patch_embed.patch_size
    return fn


# ------------------------------------------------------------------------------------------------------------ whitening
class PCAWhitening:
    """utils.PCA(dim, whit) (utils.py:655-706) with the statistics and the projection on the device.
    fit(features): mean and the UNCENTRED second moment X^T X / N (eval_copy_detection.py:278-283) by sais_colmean_cov in exact
    f32, then on the host np.linalg.eigh of that f32 matrix with the reference's eigenvalue floor (1e-5 of the largest), descending
    order, `dim` components and dvt = diag(d^-whit) v^T.
    apply(x): (x - mean) dvt^T with L2-normalised rows: the centring is its own launch (not a GEMM bias: the cancellation would
    pass through the whitening gain), the normalisation is sais_l2norm_fwd (F.normalize).  The projection runs on the exact
    f32-input MFMA (sais_probe_logits with one head and a zero bias, 1024 rows per launch), the arithmetic of the reference's f32
    torch.mm: the bf16x3 product of sais_gemm_nt_f32 drops the lo x lo term, and after the whitening gain that alone costs
    2.7e-6 in the similarities of the well-conditioned golden case, where four times the reference's own f32 error is 2.0e-6."""

    ROWS_PER_LAUNCH = 1024          # SAIS_PROBE_MAX_ROWS

    def __init__(self, dim=256, whit=0.5):
        self.dim, self.whit = int(dim), float(whit)
        self.mean = self.cov = self.dvt = self._dvt_dev = None
        self.energy = None

    def fit(self, features):
        x = _device_matrix(features, "features")
        D = x.shape[1]
        if D % 64 or D > 1536:
            raise ValueError(f"features: D = {D} must be a multiple of 64 and at most 1536")
        if not 1 <= self.dim <= D:
            raise ValueError(f"dim = {self.dim} must be in [1, D = {D}]")
        self.mean = torch.empty(D, dtype=torch.float32, device=x.device)
        self.cov = torch.empty(D, D, dtype=torch.float32, device=x.device)
        ops.colmean_cov(x, self.mean, self.cov)
        self.train_pca(self.cov.cpu().numpy())
        return self

    def train_pca(self, cov):
        """The whitening operator of a host second-moment matrix (f32 from the device: the decomposition then runs in f32, as
        the reference's does on cov.cpu().numpy()).  Eigenvalues below 1e-5 of the largest are raised to that floor, the `dim`
        largest directions are kept in descending order and each is scaled by eigenvalue^-whit: dvt [dim, D]."""
        w, v = np.linalg.eigh(cov)
        w = np.maximum(w, w.max() * 1e-5)
        keep = np.argsort(w)[::-1][:self.dim]
        self.energy = float(100.0 * w[keep].sum() / w.sum())
        print("keeping %.2f %% of the energy" % self.energy)
        self.dvt = (v[:, keep] / w[keep] ** self.whit).T
        self._dvt_dev = None

    def apply(self, x, normalize=True):
        if self.dvt is None:
            raise RuntimeError("PCAWhitening.apply before fit")
        x = _device_matrix(x, "x").clone()
        if x.shape[1] != self.dvt.shape[1]:
            raise ValueError(f"x: expected [N, {self.dvt.shape[1]}]")
        if self._dvt_dev is None or self._dvt_dev.device != x.device:
            self._dvt_dev = torch.from_numpy(np.ascontiguousarray(self.dvt, dtype=np.float32)).to(x.device)
        if self.mean is not None:
            ops.center_rows_(x, self.mean)
        out = torch.empty(x.shape[0], self.dim, dtype=torch.float32, device=x.device)
        zero = torch.zeros(self.dim, dtype=torch.float32, device=x.device)
        for i in range(0, x.shape[0], self.ROWS_PER_LAUNCH):
            rows = min(self.ROWS_PER_LAUNCH, x.shape[0] - i)
            L.call("sais_probe_logits", ops._p(x[i:]), ops._p(self._dvt_dev), ops._p(zero), 1, rows, self.dim, x.shape[1],
                   ops._p(out[i:]), ops._stream())
        return _l2norm(out, out) if normalize else out


def l2_normalize(x):
    """F.normalize(x, dim=1, p=2) by sais_l2norm_fwd."""
    x = _device_matrix(x, "x")
    return _l2norm(x, torch.empty_like(x))


# ------------------------------------------------------------------------------------------------------------ copy detection
@torch.no_grad()
def copy_detection_topk(queries, database, k=20):
    """similarity.topk(k) of eval_copy_detection.py:295-296 without the [Nq, Ndb] matrix: (values f32 [Nq, k'], indices i32
    [Nq, k']) with k' = min(k, Ndb), rows sorted by (value descending, index ascending).  Both inputs L2-normalised."""
    q, db = _device_matrix(queries, "queries"), _device_matrix(database, "database")
    return KnnIndex(db).search(q, min(int(k), db.shape[0]))


def average_precision_from_ranks(ranks, nres):
    """Area under the precision-recall polyline of one query (what both score_ap_from_ranks_1, eval_copy_detection.py:97-125,
    and utils.compute_ap, utils.py:709-741, compute).  ranks: ascending 0-based ranks of the positives that were retrieved,
    nres: number of positives.  Positive number j found at rank r spans recall 1 / nres between precision j / r (1 at r = 0)
    and (j + 1) / (r + 1); the sum of the trapezoids, in fp64."""
    if nres < 1:
        raise ValueError("a query without positives has no average precision")
    r = np.asarray(ranks, dtype=np.float64).reshape(-1)
    j = np.arange(r.size, dtype=np.float64)
    before = np.divide(j, r, out=np.ones_like(r), where=r > 0)
    return float(np.sum((before + (j + 1.0) / (r + 1.0)) * (0.5 / nres)))


compute_ap = average_precision_from_ranks            # utils.compute_ap is the same sum


def copydays_blocks(basedir):
    """[(block name, sorted .jpg names)] of a Copydays tree in the reference's block order; the block sizes come from the
    directory listing (157 per block, 229 for `strong`, on the real data).  Blocks that are absent are left out."""
    out = []
    for name in COPYDAYS_BLOCKS:
        d = os.path.join(basedir, name)
        if os.path.isdir(d):
            out.append((name, [f for f in sorted(os.listdir(d)) if f.endswith(".jpg")]))
    if not out or out[0][0] != "original":
        raise FileNotFoundError(f"no `original` block under {basedir}")
    return out


def copydays_map(indices, blocks):
    """CopydaysDataset.eval_result (eval_copy_detection.py:63-92): [(block name, mAP)] from the retrieved database indices
    [sum of block sizes, k] (host array) of the queries in block order.  The database starts with the `original` block: query i
    of a block matches original i, a `strong` query every original with the same four-character prefix."""
    indices = np.asarray(indices)
    rows = sum(len(files) for _, files in blocks)
    if rows != len(indices):
        raise ValueError(f"{len(indices)} query rows for blocks of {rows} files")
    prefix = np.asarray([name[:4] for name in blocks[0][1]])
    out, first = [], 0
    for name, files in blocks:
        aps = []
        for i, fname in enumerate(files):
            positives = np.flatnonzero(prefix == fname[:4]) if name == "strong" else np.asarray([i])
            found = np.flatnonzero(np.isin(indices[first + i], positives))
            aps.append(average_precision_from_ranks(found, len(positives)))
        out.append((name, float(np.sum(aps)) / len(files)))
        first += len(files)
    return out


# ------------------------------------------------------------------------------------------------------------ retrieval ranks
@torch.no_grad()
def rank_positions(sim, lists):
    """sim: device f32 [Nq, Ndb], finite; lists: per query a sequence of database indices.  Returns per query an int64 array:
    the 0-based position of each listed item in np.argsort(-sim[q], kind="stable") (value descending, index ascending), by
    sais_rank_positions — the whole-database argsort of eval_image_retrieval.py:176 is never formed."""
    if not isinstance(sim, torch.Tensor) or not sim.is_cuda:
        raise L.SaisHipError("sim: expected a device tensor (the retrieval path has no CPU fallback)")
    if sim.dim() != 2 or sim.shape[0] < 1 or sim.shape[1] < 1:
        raise ValueError(f"sim: expected [Nq, Ndb], got {tuple(sim.shape)}")
    if len(lists) != sim.shape[0]:
        raise ValueError(f"{len(lists)} lists for {sim.shape[0]} queries")
    sim = sim.float()
    if sim.stride(1) != 1:
        sim = sim.contiguous()                           # (rows may keep a stride of their own)
    arrays = [np.asarray(l, dtype=np.int64).reshape(-1) for l in lists]
    for q, a in enumerate(arrays):
        if a.size and (a.min() < 0 or a.max() >= sim.shape[1]):
            raise ValueError(f"query {q}: database index outside [0, {sim.shape[1]})")
    offsets = np.zeros(len(arrays) + 1, dtype=np.int64)
    np.cumsum([a.size for a in arrays], out=offsets[1:])
    total = int(offsets[-1])
    if total == 0:
        return [np.zeros(0, dtype=np.int64) for _ in arrays]
    if total >= 2 ** 31:
        raise ValueError("too many listed items")
    items = torch.from_numpy(np.concatenate(arrays).astype(np.int32)).to(sim.device)
    off = torch.from_numpy(offsets.astype(np.int32)).to(sim.device)
    pos = torch.empty(total, dtype=torch.int32, device=sim.device)
    ops.rank_positions(sim, off, items, pos)
    pos = pos.cpu().numpy().astype(np.int64)
    return [pos[offsets[q]:offsets[q + 1]] for q in range(len(arrays))]


def gnd_lists(gnd):
    """The database indices compute_map reads per query: `ok` followed by `junk` (absent: none)."""
    return [np.concatenate([np.asarray(g["ok"], dtype=np.int64).reshape(-1),
                            np.asarray(g.get("junk", []), dtype=np.int64).reshape(-1)]) for g in gnd]


def compute_map(positions, gnd, kappas=()):
    """What utils.compute_map (utils.py:744-813) returns, from positions instead of the [Ndb, Nq] rank matrix: positions[q] holds
    the positions of gnd_lists(gnd)[q] (rank_positions).  Per query with a non-empty `ok`: the distinct positions of the
    positives, each moved up by the number of junk images ranked before it (the ranking with the junk taken out); AP of those
    with nres = len(ok); precision at k = (positives within the first kq) / kq with kq = min(k, 1-based position of the last
    positive).  Queries without positives count nowhere: their rows are NaN and the means run over the others.
    Returns (mAP, APs [nq], mean precision at k [len(kappas)], precision at k [nq, len(kappas)])."""
    kappas = np.asarray(list(kappas), dtype=np.int64)
    aps = np.full(len(gnd), np.nan)
    prs = np.full((len(gnd), kappas.size), np.nan)
    for q, g in enumerate(gnd):
        nok = np.asarray(g["ok"]).size
        if nok == 0:
            continue
        listed = np.asarray(positions[q], dtype=np.int64)
        positives, junk = np.unique(listed[:nok]), np.unique(listed[nok:])
        clean = positives - np.searchsorted(junk, positives)          # junk strictly before each positive is dropped
        aps[q] = average_precision_from_ranks(clean, nok)
        cut = np.minimum(kappas, clean[-1] + 1)
        prs[q] = (clean[None, :] < cut[:, None]).sum(1) / cut
    used = ~np.isnan(aps)
    return float(aps[used].sum() / used.sum()), aps, prs[used].sum(0) / used.sum(), prs


def revisited_protocols(gnd):
    """The Medium and Hard ground truths of eval_image_retrieval.py:184-197 from the `easy` / `hard` / `junk` lists."""
    cat = lambda *a: np.concatenate([np.asarray(v, dtype=np.int64).reshape(-1) for v in a])
    medium = [{"ok": cat(g["easy"], g["hard"]), "junk": cat(g["junk"])} for g in gnd]
    hard = [{"ok": cat(g["hard"]), "junk": cat(g["junk"], g["easy"])} for g in gnd]
    return medium, hard


@torch.no_grad()
def evaluate_revisited(sim, gnd, kappas=(1, 5, 10)):
    """((mapM, mprM), (mapH, mprH)) of eval_image_retrieval.py:173-198 from sim = query x database (device f32 [Nq, Ndb])."""
    out = []
    for g in revisited_protocols(gnd):
        m, _, mpr, _ = compute_map(rank_positions(sim, gnd_lists(g)), g, kappas)
        out.append((m, mpr))
    return tuple(out)


@torch.no_grad()
def similarity(queries, database):
    """queries database^T as device f32 [Nq, Ndb] by sais_gemm_nt_f32; rows of `database` are padded to its 128-row tiles."""
    q, db = _device_matrix(queries, "queries"), _device_matrix(database, "database")
    if q.shape[1] != db.shape[1] or q.shape[1] % 64:
        raise ValueError("queries and database need the same feature width, a multiple of 64")
    n = db.shape[0]
    npad = (n + 127) // 128 * 128
    if npad != n:
        db = torch.cat([db, torch.zeros(npad - n, db.shape[1], dtype=torch.float32, device=db.device)])
    out = torch.empty(q.shape[0], npad, dtype=torch.float32, device=q.device)
    ops.gemm_nt_f32(q, db, L.EPI_BIAS_F32, out)
    return out[:, :n]


# ------------------------------------------------------------------------------------------------------------ datasets (host)
def is_image_file(name):
    """The reference's rule: the text after the last dot is one of IMG_EXTENSIONS (case-sensitive)."""
    return name.rpartition(".")[2] in IMG_EXTENSIONS


def list_images(directory):
    """The image files of a flat directory (distractors, whitening images), sorted so that the order does not depend on the
    file system."""
    return [os.path.join(directory, name) for name in sorted(os.listdir(directory)) if is_image_file(name)]


def _to_tensor(img):
    a = np.asarray(img, dtype=np.float32) / 255.0
    a = (a - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


class ImgListDataset(torch.utils.data.Dataset):
    """eval_copy_detection.py:128-158 on Pillow: RGB, Resize((imsize, imsize), bicubic), ToTensor, ImageNet normalisation."""

    def __init__(self, img_list, imsize):
        self.samples, self.imsize = list(img_list), int(imsize)

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        from PIL import Image
        with open(self.samples[i], "rb") as fh:
            img = Image.open(fh).convert("RGB")
        if img.size != (self.imsize, self.imsize):
            img = img.resize((self.imsize, self.imsize), Image.BICUBIC)
        return _to_tensor(img), i


class OxfordParisDataset(torch.utils.data.Dataset):
    """eval_image_retrieval.py:33-71: the query or database images of roxford5k / rparis6k from gnd_<dataset>.pkl, RGB,
    img.thumbnail((imsize, imsize), LANCZOS) (the aspect ratio stays: frames of different sizes), ToTensor, normalisation."""

    def __init__(self, dir_main, dataset, split, imsize=None):
        if dataset not in ("roxford5k", "rparis6k"):
            raise ValueError("Unknown dataset: {}!".format(dataset))
        self.root = os.path.join(dir_main, dataset)
        self.image_dir = os.path.join(self.root, "jpg")
        with open(os.path.join(self.root, f"gnd_{dataset}.pkl"), "rb") as fh:
            self.cfg = pickle.load(fh)                   # imlist, qimlist, gnd: the file's own keys, nothing added
        self.gnd = self.cfg["gnd"]
        self.samples = list(self.cfg["qimlist" if split == "query" else "imlist"])
        self.imsize = imsize

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        from PIL import Image, ImageFile
        ImageFile.LOAD_TRUNCATED_IMAGES = True
        with open(os.path.join(self.image_dir, self.samples[index] + ".jpg"), "rb") as fh:
            img = Image.open(fh).convert("RGB")
        if self.imsize is not None:
            img.thumbnail((self.imsize, self.imsize), Image.LANCZOS)
        return _to_tensor(img), index


class ThumbnailBatches:
    """OxfordParisDataset's loader with the pixels made on the GPU: wraps a DataLoader over imgfolder.RawOxfordParis
    (collate_raw) and a GpuImageLoader, and yields what extract_features takes.  Per image (the default): (samples
    [1, 3, h, w], index [1]) in dataset order, as the Pillow loader at batch size 1 yields them, bit for bit.  With
    group_shapes the thumbnails of one loader batch that share a shape are stacked: ([F, 3, h, w], index [F]), groups in
    the order of their first image; extract_features scatters the rows by index.  A backbone call on F frames computes
    each row as it computes it alone up to the rounding of its kernels' batch-dependent tiling; under multi_scale the
    result is also divided by the norm of the WHOLE batch tensor, a scalar per call that the row normalisation after
    extract_features (l2_normalize) removes up to rounding.  With mixed every loader batch is ONE item: (the list of its
    thumbnails [1, 3, h_k, w_k], index [F]), for a backbone callable that takes frames of different sizes in one segmented pass
    (cls_features on a patch-16 model, multi_scale over it)."""

    def __init__(self, loader, gpu_loader, imsize, group_shapes=False, mixed=False):
        if group_shapes and mixed:
            raise ValueError("ThumbnailBatches: group_shapes and mixed exclude each other")
        self.loader, self.gpu_loader, self.imsize, self.group_shapes = loader, gpu_loader, int(imsize), bool(group_shapes)
        self.mixed = bool(mixed)
        self.dataset = loader.dataset

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for items, tags in self.loader:
            thumbs = self.gpu_loader.thumbnail(items, self.imsize)
            if self.mixed:
                yield list(thumbs), tags
                continue
            if not self.group_shapes:
                for k, t in enumerate(thumbs):
                    yield t, tags[k:k + 1]
                continue
            groups = {}
            for k, t in enumerate(thumbs):
                groups.setdefault(tuple(t.shape[2:]), []).append(k)
            for ks in groups.values():
                yield torch.cat([thumbs[k] for k in ks]), tags[ks]


@torch.no_grad()
def extract_features(fn, loader, device="cuda:0"):
    """Features [N, D] on the device in dataset order; `loader` yields (images, dataset indices), fn maps device frames to [F, D]
    (cls_features, descriptor_features, or multi_scale over one of them: each crops to whole patches itself, multi_scale after
    rescaling the uncropped frame as the reference does).  An item whose images are a LIST of frames of different sizes
    (ThumbnailBatches(mixed=True)) is handed to fn as a list."""
    feats = None
    for samples, index in loader:
        if isinstance(samples, (list, tuple)):
            samples = [t.to(device, non_blocking=True) for t in samples]
        else:
            samples = samples.to(device, non_blocking=True)
        out = fn(samples).float()
        if feats is None:
            feats = torch.zeros(len(loader.dataset), out.shape[-1], dtype=torch.float32, device=device)
        feats.index_copy_(0, index.to(device), out)
    return feats
