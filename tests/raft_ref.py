"""numpy references of the three non-GEMM kernels of sais_amd/csrc/raft.hip: the correlation-pyramid pooling, the window
lookup and im2col.  Their arithmetic is fully defined (two of them are gathers), so the references are exact statements of it:

  pool_f32    one 2 x 2 average-pooling level in float32, in the kernel's order ((p0 + p1) + pW) + pW1) * 0.25f: bit-equal
  pool_f64    the same level in fp64, and pool_bar: 4 float32 spacings at the magnitude A = 0.25 (|p0| + |p1| + |pW| + |pW1|)
              (three additions round to at most 3 * 2^-24 * 4 A before the exact scale by 0.25, i.e. under 3 spacings of A)
  lookup_f64  the (2r + 1)^2 bilinear window per position and level in fp64; the integer and fractional parts of
              coords * 2^-l are formed in float32 exactly as the kernel forms them, taps outside the level are zero, window
              index a runs along x; lookup_bar: 16 * 2^-24 * max|level l| (nine float32 roundings on values of at most twice
              the largest tap, with or without fused multiply-add)
  im2col      the exact gather, bias column and zero padding of sais_im2col_f32"""
import numpy as np

LEVELS = 4


# ------------------------------------------------------------------------------------------------ pooling
def _quads(x):
    """the four taps of every 2 x 2 cell of [rows, H, W] (odd last row / column dropped)"""
    H2, W2 = x.shape[1] // 2, x.shape[2] // 2
    x = x[:, :2 * H2, :2 * W2]
    return x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]


def pool_f32(x):
    p0, p1, pw, pw1 = _quads(np.asarray(x, np.float32))
    return (((p0 + p1) + pw) + pw1) * np.float32(0.25)


def pool_f64(x):
    p0, p1, pw, pw1 = _quads(np.asarray(x, np.float64))
    return (p0 + p1 + pw + pw1) * 0.25


def pool_bar(x):
    p0, p1, pw, pw1 = (np.abs(q) for q in _quads(np.asarray(x, np.float64)))
    a = ((p0 + p1 + pw + pw1) * 0.25).astype(np.float32)
    return 4.0 * np.spacing(np.maximum(a, np.finfo(np.float32).tiny)).astype(np.float64)


def pyramid_f32(c0):
    """levels 1..3 of [rows, H, W] float32, each pooled from the float32 level before it, as the kernel does"""
    out, cur = [], np.asarray(c0, np.float32)
    for _ in range(LEVELS - 1):
        cur = pool_f32(cur)
        out.append(cur)
    return out


# ------------------------------------------------------------------------------------------------ lookup
def lookup_f64(levels, coords, radius):
    """levels: 4 arrays [B H W, Hl, Wl]; coords float32 [B, 2, H, W] (x, y) -> fp64 [B, 4 n n, H, W], n = 2 r + 1."""
    coords = np.asarray(coords, np.float32)
    B, _, H, W = coords.shape
    HW, n = H * W, 2 * radius + 1
    out = np.zeros((B, LEVELS * n * n, HW), np.float64)
    cx0 = coords[:, 0].reshape(B * HW)
    cy0 = coords[:, 1].reshape(B * HW)
    rows = np.arange(B * HW)[:, None, None]
    for l, vol in enumerate(levels):
        P, Hl, Wl = vol.shape
        assert P == B * HW
        inv = np.float32(1.0) / np.float32(1 << l)
        cx, cy = (cx0 * inv).astype(np.float32), (cy0 * inv).astype(np.float32)
        fx0, fy0 = np.floor(cx), np.floor(cy)
        fx, fy = (cx - fx0).astype(np.float32).astype(np.float64), (cy - fy0).astype(np.float32).astype(np.float64)
        # past the int range every tap is outside the level whatever the conversion gives: any far-away value will do
        x0 = np.clip(fx0.astype(np.float64), -2.0 ** 40, 2.0 ** 40).astype(np.int64) - radius
        y0 = np.clip(fy0.astype(np.float64), -2.0 ** 40, 2.0 ** 40).astype(np.int64) - radius
        X = x0[:, None] + np.arange(n + 1)[None, :]                     # [P, n + 1]
        Y = y0[:, None] + np.arange(n + 1)[None, :]
        ok = ((Y >= 0) & (Y < Hl))[:, :, None] & ((X >= 0) & (X < Wl))[:, None, :]
        T = vol[rows, np.clip(Y, 0, Hl - 1)[:, :, None], np.clip(X, 0, Wl - 1)[:, None, :]].astype(np.float64)
        T = np.where(ok, T, 0.0)                                        # [P, y, x]
        l0, r0, l1, r1 = T[:, :-1, :-1], T[:, :-1, 1:], T[:, 1:, :-1], T[:, 1:, 1:]
        fxb, fyb = fx[:, None, None], fy[:, None, None]
        top, bot = l0 + fxb * (r0 - l0), l1 + fxb * (r1 - l1)
        win = top + fyb * (bot - top)                                   # [P, bb (y), a (x)]
        win = win.transpose(0, 2, 1).reshape(B, HW, n * n)              # channel a * n + bb
        out[:, l * n * n:(l + 1) * n * n] = win.transpose(0, 2, 1)
    return out.reshape(B, LEVELS * n * n, H, W)


def lookup_bar(level):
    return 16.0 * 2.0 ** -24 * float(np.abs(level).max())


# ------------------------------------------------------------------------------------------------ im2col
def conv_out(H, W, kh, kw, sh, sw, ph, pw):
    return (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1


def im2col(x, kh, kw, sh, sw, ph, pw, ld, rows):
    """x float32 [C, H, W] -> [rows, ld]: row oy * Wo + ox, column (c * kh + ky) * kw + kx; column K = 1.0 on the rows of
    the image; everything else zero."""
    x = np.asarray(x, np.float32)
    C, H, W = x.shape
    Ho, Wo = conv_out(H, W, kh, kw, sh, sw, ph, pw)
    K = C * kh * kw
    assert Ho > 0 and Wo > 0 and ld >= K + 1 and rows >= Ho * Wo
    xp = np.zeros((C, H + 2 * ph, W + 2 * pw), np.float32)
    xp[:, ph:ph + H, pw:pw + W] = x
    cols = np.zeros((rows, ld), np.float32)
    for c in range(C):
        for ky in range(kh):
            for kx in range(kw):
                patch = xp[c, ky:ky + sh * (Ho - 1) + 1:sh, kx:kx + sw * (Wo - 1) + 1:sw]
                cols[:Ho * Wo, (c * kh + ky) * kw + kx] = patch.reshape(-1)
    cols[:Ho * Wo, K] = 1.0
    return cols
