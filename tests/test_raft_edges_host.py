"""The numpy references of tests/raft_ref.py against oracle/raft_oracle.py (fp32 torch: avg_pool2d, grid_sample) at the sizes
of test_raft_gpu.py, and against hand-computed values.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import raft_ref as RR
from oracle import raft_oracle as R

SIZES = [(16, 21), (28, 41), (68, 120)]


@pytest.mark.parametrize("H,W", SIZES)
def test_pool_and_lookup_references_agree_with_the_oracle(H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    rows = H * W
    c0 = torch.randn(rows, 1, H, W, generator=g)
    pyr = [c0]
    for _ in range(3):
        pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
    lv32 = RR.pyramid_f32(c0[:, 0].numpy())
    prev = c0[:, 0].numpy()
    for l in range(3):
        want = pyr[l + 1][:, 0].numpy()
        assert lv32[l].shape == want.shape and lv32[l].dtype == np.float32
        assert (np.abs(lv32[l].astype(np.float64) - RR.pool_f64(prev)) <= RR.pool_bar(prev)).all()
        assert np.abs(lv32[l] - want).max() <= 1e-6 * float(np.abs(prev).max())
        prev = lv32[l]
    coords = torch.stack([torch.rand(H, W, generator=g) * (W + 12) - 6, torch.rand(H, W, generator=g) * (H + 12) - 6]).unsqueeze(0)
    coords[0, :, 0, 0] = torch.tensor([0.0, 0.0])
    coords[0, :, 1, 1] = torch.tensor([W - 1.0, H - 1.0])
    coords[0, :, 2, 2] = torch.tensor([-40.0, 3.0])
    want = R.corr_lookup(pyr, coords).numpy()
    got = RR.lookup_f64([p[:, 0].numpy() for p in pyr], coords.numpy(), 4)
    assert got.shape == want.shape == (1, 324, H, W)
    # the oracle samples through normalised grid coordinates in float32: the bar of test_raft_gpu.py
    assert np.abs(got - want).max() <= 1e-4 * float(c0.abs().max())


def test_lookup_reference_by_hand():
    """value 100 y + x + 1 at (x, y): channel n a + b of level 0 reads (x + a - r, y + b - r), zeros outside."""
    H, W, r = 8, 9, 1
    img = (100.0 * np.arange(H)[:, None] + np.arange(W)[None, :] + 1.0).astype(np.float32)
    lv = [np.repeat(img[None], H * W, 0)]
    for _ in range(3):
        lv.append(RR.pool_f32(lv[-1]))
    coords = np.zeros((1, 2, H, W), np.float32)
    coords[0, 0], coords[0, 1] = 3.25, 2.5
    coords[0, :, 0, 1] = (-0.25, 0.0)
    coords[0, :, 0, 2] = (3e9, -3e9)
    out = RR.lookup_f64(lv, coords, r)
    w0 = out[0, :9, 0, 0].reshape(3, 3)
    for a in range(3):
        for b in range(3):
            assert abs(w0[a, b] - (100 * (2.5 + b - r) + 3.25 + a - r + 1)) < 1e-9
    # floor(-0.25) = -1, fraction 0.75: the tap at x = -1 is zero, so a = 1 reads 0.25 * 0 + 0.75 * img[0, 0]
    e = out[0, :9, 0, 1].reshape(3, 3)
    assert e[0, 1] == 0.0 and e[1, 1] == 0.75 * img[0, 0] and abs(e[2, 1] - 1.75) < 1e-12 and e[1, 0] == 0.0
    assert (out[0, :, 0, 2] == 0.0).all()
    # level 1 at half the coordinates
    assert abs(out[0, 9 + 4, 0, 0] - ((1 - .625) * lv[1][0, 1, 1] + .625 * lv[1][0, 1, 2]) * .75
               - ((1 - .625) * lv[1][0, 2, 1] + .625 * lv[1][0, 2, 2]) * .25) < 1e-9


def test_pool_reference_order_and_odd_sizes():
    x = np.array([[[1e8, 1.0, 7.0], [-1e8, 1.0, 7.0], [5.0, 5.0, 5.0]]], np.float32)
    got = RR.pool_f32(x)
    assert got.shape == (1, 1, 1)
    assert got[0, 0, 0] == np.float32(0.25)                 # ((1e8 + 1) + -1e8) + 1 in float32: the first 1 is absorbed
    assert RR.pool_f64(x)[0, 0, 0] == 0.5
    assert abs(0.25 - 0.5) <= RR.pool_bar(x)[0, 0, 0]
    assert [v.shape[1:] for v in RR.pyramid_f32(np.zeros((2, 9, 11), np.float32))] == [(4, 5), (2, 2), (1, 1)]


@pytest.mark.parametrize("C,H,W,k,s,p", [(3, 9, 11, (7, 7), (2, 2), (3, 3)), (5, 6, 7, (3, 3), (1, 1), (1, 1)),
                                         (4, 5, 6, (1, 5), (1, 1), (0, 2)), (4, 5, 6, (5, 1), (1, 1), (2, 0)),
                                         (2, 2, 3, (3, 3), (1, 1), (1, 1)), (6, 4, 5, (1, 1), (2, 2), (0, 0))])
def test_im2col_reference_is_unfold(C, H, W, k, s, p):
    x = torch.randn(C, H, W, generator=torch.Generator().manual_seed(C * H))
    Ho, Wo = RR.conv_out(H, W, *k, *s, *p)
    K = C * k[0] * k[1]
    cols = RR.im2col(x.numpy(), *k, *s, *p, K + 3, Ho * Wo + 2)
    want = F.unfold(x[None], k, padding=p, stride=s)[0].t().numpy()                 # [Ho Wo, K]
    assert np.array_equal(cols[:Ho * Wo, :K], want)
    assert (cols[:Ho * Wo, K] == 1.0).all() and (cols[:Ho * Wo, K + 1:] == 0).all() and (cols[Ho * Wo:] == 0).all()
