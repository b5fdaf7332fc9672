"""The three non-GEMM kernels of sais_amd/csrc/raft.hip on a real MI355X at their edges, through the raw entries: odd sizes at
every pyramid level, a row stride with a poisoned gap, the pooling's LDS grant above 64 KiB and its refusal, every lookup
radius, two volumes in one launch, coordinates on, outside and far outside the level, im2col's padding rows and columns.

References and bars: tests/raft_ref.py (pooling bit-equal to float32 in the kernel's order and within 4 spacings of fp64;
lookup within 16 * 2^-24 * max|level| of fp64; im2col exact).  Outputs land in NaN-filled buffers with a spare row."""
import numpy as np
import pytest
import torch

import parity
import raft_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
POISON = 1e30


@pytest.fixture(scope="module")
def L():
    from sais_amd import _lib
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def level0(rows, H, W, gap, seed):
    """float32 [rows, H W] at row stride H W + gap, the gap holding 1e30: (device buffer, ld0, host [rows, H, W])"""
    host = torch.randn(rows, H * W, generator=torch.Generator().manual_seed(seed))
    buf = torch.full((rows, H * W + gap), POISON, dtype=torch.float32)
    buf[:, :H * W] = host
    return buf.to(DEV), H * W + gap, host.view(rows, H, W).numpy()


def pool(L, c0, ld0, rows, H, W):
    """levels 1..3 out of NaN buffers with one spare row each, which must stay NaN: (rc, [device [rows, Hl Wl]])"""
    bufs = [nan(rows + 1, max(1, (H >> l) * (W >> l))) for l in (1, 2, 3)]
    rc = L.load().sais_raft_corr_pool(c0.data_ptr(), ld0, rows, H, W, *(b.data_ptr() for b in bufs), stream())
    torch.cuda.synchronize()
    for b in bufs:
        assert bool(torch.isnan(b[rows]).all()), "wrote past the last row"
    return rc, [b[:rows] for b in bufs]


def check_pool(L, rows, H, W, gap, seed):
    c0, ld0, host = level0(rows, H, W, gap, seed)
    rc, got = pool(L, c0, ld0, rows, H, W)
    assert rc == 0
    want = RR.pyramid_f32(host)
    prev = host
    for l in range(3):
        g = got[l].cpu().numpy().reshape(want[l].shape)
        assert not np.isnan(g).any()
        assert np.array_equal(g.view(np.int32), want[l].view(np.int32)), f"level {l + 1} of {H} x {W} is not the float32 reference"
        r = float((np.abs(g.astype(np.float64) - RR.pool_f64(prev)) / RR.pool_bar(prev)).max())
        parity.parity_log(f"raft_edge_pool_l{l + 1}", r, 1.0)
        assert r <= 1.0, (l, r)
        prev = want[l]
    return got


@pytest.mark.parametrize("H,W,gap", [(8, 8, 0), (9, 11, 5), (15, 10, 1), (16, 21, 48)])
def test_pool_odd_sizes_and_row_stride(L, H, W, gap):
    check_pool(L, 3, H, W, gap, seed=H * 100 + W)


def test_pool_lds_grant_grows_once_and_the_refusal_writes_nothing(L):
    """One process, in this order: a small size, one above 64 KiB of LDS (the hipFuncSetAttribute path), a small one again
    (the grant is a high-water mark), then one LDS row past the 160 KiB limit."""
    check_pool(L, 3, 8, 8, 0, seed=1)
    assert (176 * 177 + 88 * 88 + 44 * 44) * 4 == 163328
    check_pool(L, 3, 176, 177, 3, seed=2)
    check_pool(L, 3, 16, 21, 0, seed=3)
    assert (177 * 177 + 88 * 88 + 44 * 44) * 4 == 164036
    c0, ld0, _ = level0(3, 177, 177, 0, seed=4)
    rc, got = pool(L, c0, ld0, 3, 177, 177)
    assert rc == -1
    assert all(bool(torch.isnan(g).all()) for g in got)
    lib = L.load()
    a = nan(64)
    assert lib.sais_raft_corr_pool(a.data_ptr(), 63, 1, 8, 8, a.data_ptr(), a.data_ptr(), a.data_ptr(), stream()) == -1     # ld0 < H W
    assert lib.sais_raft_corr_pool(a.data_ptr(), 64, 1, 7, 8, a.data_ptr(), a.data_ptr(), a.data_ptr(), stream()) == -1
    assert lib.sais_raft_corr_pool(a.data_ptr(), 64, 0, 8, 8, a.data_ptr(), a.data_ptr(), a.data_ptr(), stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(a).all())


# ------------------------------------------------------------------------------------------------ lookup
def special_coords(H, W):
    far = [(1e9, 2.0), (-1e9, 2.0), (2.0, 1e9), (2.0, -1e9), (3e9, 3e9), (-3e9, -3e9), (3e9, 2.0), (2.0, -3e9)]
    near = [(3.0, 2.0), (-1.0, -1.0), (0.0, 0.0), (W - 1.0, H - 1.0), (float(W), float(H)), (-0.25, -0.25), (-0.5, 2.0),
            (W - 0.5, 2.0), (2.0, -0.5), (2.0, H - 0.5), (40.0, 3.0), (-40.0, 3.0), (3.0, 40.0), (3.0, -40.0), (W - 1.0, 0.0),
            (0.0, H - 1.0)]
    return near, far


def make_coords(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.stack([torch.rand(B, H, W, generator=g) * (W + 12) - 6, torch.rand(B, H, W, generator=g) * (H + 12) - 6], 1)
    near, far = special_coords(H, W)
    flat = c.view(B, 2, H * W)
    for b in range(B):
        for i, xy in enumerate(near + far):
            flat[b, :, (i * 3 + b) % (H * W)] = torch.tensor(xy)
    far_pos = [[(i * 3 + b) % (H * W) for i in range(len(near), len(near) + len(far))] for b in range(B)]
    return c.contiguous(), far_pos


def volumes(B, H, W, gap, seed):
    """B volumes back to back: level 0 [B H W, H W] at stride H W + gap (1e30 in the gap), levels 1..3 pooled on the host"""
    c0, ld0, host = level0(B * H * W, H, W, gap, seed)
    lv = [host] + RR.pyramid_f32(host)
    dev = [c0] + [torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in lv[1:]]
    return dev, ld0, lv


def lookup(L, dev, ld0, coords_dev, B, H, W, radius):
    n = 2 * radius + 1
    buf = nan(B * 4 * n * n + 1, H * W)
    rc = L.load().sais_raft_lookup(dev[0].data_ptr(), ld0, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                                   coords_dev.data_ptr(), B, H, W, radius, buf.data_ptr(), stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[-1]).all()), "wrote past the output"
    return rc, buf[:-1].view(B, 4 * n * n, H, W)


@pytest.mark.parametrize("radius", [1, 4, 8])
@pytest.mark.parametrize("H,W", [(8, 9), (9, 11), (16, 21)])
def test_lookup_radii_two_volumes_and_hard_coordinates(L, H, W, radius):
    B, n = 2, 2 * radius + 1
    dev, ld0, lv = volumes(B, H, W, gap=7, seed=H * 10 + W)
    coords, far_pos = make_coords(B, H, W, seed=radius)
    cdev = coords.to(DEV)
    rc, got = lookup(L, dev, ld0, cdev, B, H, W, radius)
    assert rc == 0
    g = got.cpu().numpy()
    assert not np.isnan(g).any(), "part of the output was not written"
    want = RR.lookup_f64(lv, coords.numpy(), radius)
    for l in range(4):
        bar = RR.lookup_bar(lv[l])
        err = float(np.abs(g[:, l * n * n:(l + 1) * n * n].astype(np.float64) - want[:, l * n * n:(l + 1) * n * n]).max())
        print(f"lookup {H} x {W} r {radius} level {l}: {err / bar:.3f} of the bar")
        parity.parity_log(f"raft_edge_lookup_l{l}", err / bar, 1.0)
        assert err <= bar, (l, err, bar)
    flat = g.reshape(B, 4 * n * n, H * W)
    for b in range(B):                                       # every tap outside, at 1e9 and past the int range: exactly zero
        assert (flat[b][:, far_pos[b]] == 0.0).all()
    # the same two volumes, one launch each
    HW = H * W
    for b in range(B):
        one = [dev[0][b * HW:(b + 1) * HW]] + [d[b * HW:(b + 1) * HW] for d in dev[1:]]
        rc, got1 = lookup(L, one, ld0, cdev[b:b + 1].contiguous(), 1, H, W, radius)
        assert rc == 0 and torch.equal(got1[0].view(torch.int32), got[b].view(torch.int32)), b


def test_lookup_refusals(L):
    H, W = 8, 9
    dev, ld0, _ = volumes(1, H, W, 0, seed=0)
    coords, _ = make_coords(1, H, W, 0)
    for radius in (0, 9, -1):
        out = nan(4 * 19 * 19, H * W)
        rc = L.load().sais_raft_lookup(dev[0].data_ptr(), ld0, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                                       coords.to(DEV).data_ptr(), 1, H, W, radius, out.data_ptr(), stream())
        torch.cuda.synchronize()
        assert rc == -1 and bool(torch.isnan(out).all()), radius


# ------------------------------------------------------------------------------------------------ im2col
def up(n, m):
    return (n + m - 1) // m * m


IM2COL = [  # C, H, W, (kh, kw), (sh, sw), (ph, pw)
    (5, 6, 7, (1, 1), (1, 1), (0, 0)),
    (3, 7, 10, (3, 3), (1, 1), (1, 1)),
    (3, 13, 19, (7, 7), (2, 2), (3, 3)),
    (6, 5, 9, (1, 5), (1, 1), (0, 2)),
    (6, 9, 5, (5, 1), (1, 1), (2, 0)),
    (2, 2, 3, (5, 5), (1, 1), (2, 2)),          # the image is smaller than the kernel: every patch is mostly padding
    (70, 5, 7, (3, 3), (2, 2), (1, 1)),         # K = 630: the column loop takes three rounds of 256 threads
]


@pytest.mark.parametrize("C,H,W,k,s,p", IM2COL)
def test_im2col_is_the_exact_gather(L, C, H, W, k, s, p):
    x = torch.randn(C, H, W, generator=torch.Generator().manual_seed(C * 100 + H))
    xd = x.to(DEV)
    Ho, Wo = RR.conv_out(H, W, *k, *s, *p)
    npos, K = Ho * Wo, C * k[0] * k[1]
    assert npos % 16 and (npos + 1) % 16                  # only the padded row count is a multiple of the 16 rows of a workgroup
    lds = sorted({K + 1, up(K + 1, 64), K + 38})           # below 256 (one round of the column loop) wherever K allows
    assert min(lds) < 256 or K >= 255
    for rows in (npos, npos + 1, up(npos + 1, 128)):
        for ld in lds:
            buf = nan(rows + 1, ld)
            rc = L.load().sais_im2col_f32(xd.data_ptr(), C, H, W, *k, *s, *p, buf.data_ptr(), ld, rows, stream())
            torch.cuda.synchronize()
            assert rc == 0
            assert bool(torch.isnan(buf[rows]).all()), "wrote past the last row"
            got = buf[:rows].cpu().numpy()
            want = RR.im2col(x.numpy(), *k, *s, *p, ld, rows)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (rows, ld)
            assert (got[:npos, K] == 1.0).all() and (got[:npos, K + 1:] == 0.0).all() and (got[npos:] == 0.0).all()
    buf = nan(npos + 1, K + 1)
    lib = L.load()
    assert lib.sais_im2col_f32(xd.data_ptr(), C, H, W, *k, *s, *p, buf.data_ptr(), K, npos, stream()) == -1          # ld < K + 1
    assert lib.sais_im2col_f32(xd.data_ptr(), C, H, W, *k, *s, *p, buf.data_ptr(), K + 1, npos - 1, stream()) == -1  # rows < Ho Wo
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
