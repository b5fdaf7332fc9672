// Descriptor evaluations of a DINO backbone (dino-main/eval_copy_detection.py, eval_image_retrieval.py) on gfx950:
//   sais_vit_cls_gem_norm     final LayerNorm + [CLS | GeM(p = 4) of the patch tokens] per frame (eval_copy_detection.py:166-175)
//   sais_colmean_cov          column mean and the uncentred second moment X^T X / N of the whitening set (:278-283)
//   sais_center_rows          x[r] -= mean, in place (:279-280)
//   sais_rank_positions       the positions of listed database items under argsort(-sim) (eval_image_retrieval.py:176, utils.compute_map)
//   sais_resize_bilinear_f32  F.interpolate(scale_factor, bilinear, align_corners=False) of utils.multi_scale
// Nothing here is atomic and every sum runs in one fixed order: each entry is bit-reproducible.
// Covariance arithmetic: the exact f32-input MFMA (v_mfma_f32_16x16x4_f32), bit for bit an fmaf chain in ascending row order.  The
// rows are cut into splits (cov_plan, read by the size query and by the launch); workgroup (tile, split) stores its raw 64 x 64
// partial tile, a second launch adds the splits in ascending order, divides by N and writes the tile and its mirror image.  Only
// tiles with ti <= tj are computed: x_ki x_kj and x_kj x_ki are the same product, so the diagonal tiles are bit-symmetric by
// themselves and the others by the mirrored store.
// LDS image of a covariance step: [32 rows k][64 columns] with 80-float rows; MFMA lane (i = lane & 15, k = lane >> 4) reads
// dword 80 k + i: 80 k mod 64 = 0, 16, 32, 48 -> 64 distinct banks (the image of probe.hip's update kernel).
#include "row384.hpp"
#include "../../include/sais_hip.h"

namespace {

// ---- GeM -----------------------------------------------------------------------------------------------------------------
// The CLS half is one sais_layernorm_fwd launch over the strided CLS rows, written straight into y: the same bits by
// construction (a second copy of the row arithmetic in another kernel is contracted differently by the compiler — which of the
// v - mu of the variance become one fma — and then differs in the last bit of rstd on rare rows).  The patch half: one
// workgroup per frame, one row per half-wave (row384.hpp's layout), as cls_avgpool_norm_kernel (norm.hip).  Half-wave w adds the
// fourth powers of its patch rows w, w + 8, ... in ascending order, the eight partial sums are added in half-wave order.
// The patch half runs in fp64 from the f32 inputs to one final rounding: row mean and variance, the normed value, the clamp, two
// squarings, the sum, the mean and two square roots.  The kernel is a few dozen fp64 operations per element beside a pass of
// twelve blocks, and what it buys is an output within an ulp of the exact value: in f32 a last-bit difference of rstd on the one
// row that dominates a column (a token at 50) moves the result by two ulps, ten times numpy f32's error on the same input, and
// an f32 sum loses "a column that clamps in every row gives the clamp" from ~400 rows on.  Here such a column is the clamp bit
// for bit at every token count (the fourth root of the mean of n copies of c^4 is c to 1e-16).
DEVINL double half_sum(double v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void cls_gem_norm_kernel(const float* x, long frame_stride, int ntok, const float* gamma,
                                                           const float* beta, float eps, float pmin, float* y, long ldy) {
    __shared__ double red[8][D];
    const int l32 = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const float* xf = x + (size_t)blockIdx.x * frame_stride;
    float* yf = y + (size_t)blockIdx.x * ldy;
    float gm[12], bt[12];
    double acc[12];
    load_f32(gamma, l32, gm);
    load_f32(beta, l32, bt);
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.0;
    for (int row = hw ? hw : 8; row < ntok; row += 8) {       // row 0 is the CLS token: the entry's sais_layernorm_fwd launch
        float v[12];
        load_f32(xf + (size_t)row * D, l32, v);
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 12; ++i) s += (double)v[i];
        const double mu = half_sum(s) * (1.0 / D);
        double q = 0.0;
#pragma unroll
        for (int i = 0; i < 12; ++i) { const double d = (double)v[i] - mu; q += d * d; }
        const double rs = 1.0 / sqrt(half_sum(q) * (1.0 / D) + (double)eps);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const double c = fmax(((double)v[i] - mu) * rs * (double)gm[i] + (double)bt[i], (double)pmin);
            const double c2 = c * c;
            acc[i] += c2 * c2;
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) red[hw][col_of(l32, i)] = acc[i];
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += 256) {
        double s = red[0][c];
#pragma unroll
        for (int h = 1; h < 8; ++h) s += red[h][c];
        yf[D + c] = (float)sqrt(sqrt(s / (double)(ntok - 1)));
    }
}

// ---- covariance ----------------------------------------------------------------------------------------------------------
constexpr int CT = 64, CK = 32, CLD = 80;       // tile side, rows per step, LDS row stride in floats
constexpr int COV_WG_TARGET = 1024, COV_MAX_SPLITS = 64, COV_MIN_ROWS = 128;

// The one plan of a covariance launch: tiles on or above the diagonal, rows per split (a whole number of steps), splits that hold
// rows, workspace = raw partial tiles [ns][tiles][64 x 64] followed by the column sums [ns][D]
struct CovPlan { int T, tiles, rows, ns; size_t part_floats, bytes; };
inline CovPlan cov_plan(int N, int Dm) {
    CovPlan p{};
    p.T = Dm / CT;
    p.tiles = p.T * (p.T + 1) / 2;
    int want = COV_WG_TARGET / p.tiles;
    want = want < 1 ? 1 : want > COV_MAX_SPLITS ? COV_MAX_SPLITS : want;
    int rows = ((N + want - 1) / want + CK - 1) / CK * CK;
    p.rows = rows < COV_MIN_ROWS ? COV_MIN_ROWS : rows;
    p.ns = (N + p.rows - 1) / p.rows;
    p.part_floats = (size_t)p.ns * p.tiles * CT * CT;
    p.bytes = (p.part_floats + (size_t)p.ns * Dm) * sizeof(float);
    return p;
}

DEVINL void tile_of(int t, int T, int& ti, int& tj) {        // t-th tile of the upper triangle, row by row
    ti = 0;
    while (t >= T - ti) { t -= T - ti; ++ti; }
    tj = ti + t;
}

// grid (tiles, splits); wave (wr, wc) owns a 32 x 32 quadrant as 2 x 2 MFMA tiles.  Rows past the split's end are staged as zeros
// (fma(0, 0, acc) = acc).  The diagonal tiles also add their 64 columns (the mean) in row order, one column per lane of wave 0.
__global__ __launch_bounds__(256) void cov_partial_kernel(const float* X, long ldx, int N, int Dm, int T, int ntiles, int rows,
                                                          float* part, float* colsum) {
    __shared__ __attribute__((aligned(16))) float As[CK * CLD], Bs[CK * CLD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, g = lane >> 4, li = lane & 15;
    const int tile = blockIdx.x, split = blockIdx.y;
    int ti, tj;
    tile_of(tile, T, ti, tj);
    const bool diag = ti == tj;
    const int r0 = split * rows, r1 = min(N, r0 + rows);
    const int sc = tid & 15, sr = tid >> 4;                // staging: 16 x 16-B chunks per 64-float row, 16 rows per pass
    f32x4 ra[2], rb[2];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = k0 + sr + 16 * i;
            const float* row = X + (size_t)r * ldx + 4 * sc;
            ra[i] = r < r1 ? *(const f32x4*)(row + ti * CT) : f32x4{0, 0, 0, 0};
            rb[i] = r < r1 ? *(const f32x4*)(row + tj * CT) : f32x4{0, 0, 0, 0};
        }
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    float cs = 0.f;
    gload(r0);
    for (int k0 = r0; k0 < r1; k0 += CK) {
        __syncthreads();                                   // the previous step's fragments are read
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *(f32x4*)(As + (sr + 16 * i) * CLD + 4 * sc) = ra[i];
            *(f32x4*)(Bs + (sr + 16 * i) * CLD + 4 * sc) = rb[i];
        }
        __syncthreads();
        if (k0 + CK < r1) gload(k0 + CK);
        if (diag && wid == 0) {
#pragma unroll
            for (int k = 0; k < CK; ++k) cs = __fadd_rn(cs, Bs[k * CLD + lane]);
        }
#pragma unroll
        for (int kk = 0; kk < CK; kk += 4) {
            float a[2], b[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                a[u] = As[(kk + g) * CLD + wr * 32 + u * 16 + li];
                b[u] = Bs[(kk + g) * CLD + wc * 32 + u * 16 + li];
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = mfma4(a[mt], b[nt], acc[mt][nt]);
        }
    }
    float* out = part + ((size_t)split * ntiles + tile) * (CT * CT);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                out[(wr * 32 + mt * 16 + 4 * g + r) * CT + wc * 32 + nt * 16 + li] = acc[mt][nt][r];
    if (diag && wid == 0) colsum[(size_t)split * Dm + ti * CT + lane] = cs;
}

// workgroups [0, 16 tiles): 256 elements of a tile each; the rest: 256 columns of the mean each.  Splits are added in ascending order
__global__ __launch_bounds__(256) void cov_reduce_kernel(const float* part, const float* colsum, int ns, int T, int ntiles, int N,
                                                         int Dm, float* cov, float* mean) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float n = (float)N;
    if (b < ntiles * 16) {
        const int tile = b >> 4, e = (b & 15) * 256 + tid, r = e >> 6, c = e & 63;
        int ti, tj;
        tile_of(tile, T, ti, tj);
        const float* p = part + (size_t)tile * (CT * CT) + e;
        float s = p[0];
        for (int sp = 1; sp < ns; ++sp) s = __fadd_rn(s, p[(size_t)sp * ntiles * (CT * CT)]);
        const float v = __fdiv_rn(s, n);
        const size_t i = (size_t)ti * CT + r, j = (size_t)tj * CT + c;
        if (ti != tj || r <= c) {
            cov[i * Dm + j] = v;
            cov[j * Dm + i] = v;
        }
    } else {
        const int col = (b - ntiles * 16) * 256 + tid;
        if (col >= Dm) return;
        float s = colsum[col];
        for (int sp = 1; sp < ns; ++sp) s = __fadd_rn(s, colsum[(size_t)sp * Dm + col]);
        mean[col] = __fdiv_rn(s, n);
    }
}

__global__ __launch_bounds__(256) void center_rows_kernel(float* x, long ldx, long rows, int dim4, const float* mean) {
    const long total = rows * dim4;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / dim4;
        const int c = (int)(i - r * dim4);
        f32x4* p = (f32x4*)(x + (size_t)r * ldx) + c;
        *p = *p - *((const f32x4*)mean + c);
    }
}

// ---- ranks ---------------------------------------------------------------------------------------------------------------
// grid (queries, RANK_GRID_Y).  A workgroup takes chunks of RCH listed items of its query: the chunk's (value, index) thresholds go
// to LDS, the row is streamed once, every thread counts for each threshold the elements that come before it in the order of
// `before` (common.hpp: value descending, index ascending) in RCH registers, and the counts are added over the workgroup.
// An item outside [0, Ndb) gets position -1 and is never dereferenced.
constexpr int RCH = 64, RANK_GRID_Y = 8;

__global__ __launch_bounds__(256) void rank_positions_kernel(const float* sim, long ld, int Ndb, const int* offsets,
                                                             const int* items, int* pos) {
    __shared__ float tv[RCH];
    __shared__ int tj[RCH];
    __shared__ int red[4][RCH];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int o0 = offsets[q], L = offsets[q + 1] - o0;
    const float* s = sim + (size_t)q * ld;
    for (int c = blockIdx.y; c * RCH < L; c += gridDim.y) {
        const int n = min(RCH, L - c * RCH);
        __syncthreads();                                   // the previous chunk's thresholds and counts are read
        if (tid < RCH) {
            const int j = tid < n ? items[o0 + c * RCH + tid] : -1;
            const bool ok = j >= 0 && j < Ndb;
            tj[tid] = ok ? j : -1;
            tv[tid] = ok ? s[j] : INFINITY;                // nothing comes before (+inf, -1)
        }
        __syncthreads();
        int cnt[RCH];
#pragma unroll
        for (int t = 0; t < RCH; ++t) cnt[t] = 0;
        for (int base = 0; base < Ndb; base += 1024) {
            float v[4];
            int id[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                id[u] = base + tid + 256 * u;
                v[u] = id[u] < Ndb ? s[id[u]] : -INFINITY;       // (-inf comes before no finite value)
            }
#pragma unroll
            for (int t = 0; t < RCH; ++t) {
                const float a = tv[t];
                const int bj = tj[t];
#pragma unroll
                for (int u = 0; u < 4; ++u) cnt[t] += before(v[u], id[u], a, bj) ? 1 : 0;
            }
        }
#pragma unroll
        for (int t = 0; t < RCH; ++t) {
            int w = cnt[t];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o);
            if (lane == 0) red[wid][t] = w;
        }
        __syncthreads();
        if (tid < n) pos[o0 + c * RCH + tid] = tj[tid] < 0 ? -1 : red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    }
}

// ---- bilinear resize ------------------------------------------------------------------------------------------------------
// torch's upsample_bilinear2d with align_corners = False: source coordinate rscale (dst + 0.5) - 0.5 as ONE fused multiply-add
// in f32 (what torch's kernels evaluate; two roundings move a weight by up to an ulp of the coordinate), clamped at 0, the second
// neighbour clamped at the border, weights (1 - l, l); columns first, then rows, in f32
DEVINL void src_index(float rscale, int dst, int size, int& i0, int& i1, float& l) {
    const float sf = fmaxf(__builtin_fmaf(rscale, (float)dst + 0.5f, -0.5f), 0.f);
    i0 = min((int)sf, size - 1);
    i1 = i0 + (i0 < size - 1 ? 1 : 0);
    l = sf - (float)i0;
}

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* x, long planes, int H, int W, int Ho, int Wo, float rh,
                                                              float rw, float* y) {
    const long total = planes * Ho * Wo;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % Wo);
        const long t = i / Wo;
        const int oy = (int)(t % Ho);
        const float* p = x + (size_t)(t / Ho) * H * W;
        int y0, y1, x0, x1;
        float ly, lx;
        src_index(rh, oy, H, y0, y1, ly);
        src_index(rw, ox, W, x0, x1, lx);
        const float hy = 1.f - ly, hx = 1.f - lx;
        const float top = __fadd_rn(__fmul_rn(hx, p[(size_t)y0 * W + x0]), __fmul_rn(lx, p[(size_t)y0 * W + x1]));
        const float bot = __fadd_rn(__fmul_rn(hx, p[(size_t)y1 * W + x0]), __fmul_rn(lx, p[(size_t)y1 * W + x1]));
        y[i] = __fadd_rn(__fmul_rn(hy, top), __fmul_rn(ly, bot));
    }
}

int grid_for(long n) {
    const long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
}  // namespace

extern "C" int sais_vit_cls_gem_norm(const float* x, long frame_stride, int frames, int ntok, int dim, const float* gamma,
                                     const float* beta, float eps, float p_clamp_min, float* y, long ldy, void* stream) {
    SAIS_ENTER();
    if (!x || !gamma || !beta || !y || dim != D || frames <= 0 || ntok < 2 || (frame_stride & 3) || (ldy & 3)) return SAIS_ERR_ARG;
    if (frame_stride < (long)ntok * D || ldy < 2 * D || !(p_clamp_min > 0.f)) return SAIS_ERR_ARG;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) & 15) return SAIS_ERR_ARG;
    const int rc = sais_layernorm_fwd(x, frame_stride, frames, dim, gamma, beta, eps, nullptr, 0, y, ldy, nullptr, nullptr, stream);
    if (rc != SAIS_OK) return rc;
    hipLaunchKernelGGL(cls_gem_norm_kernel, dim3(frames), dim3(256), 0, (hipStream_t)stream, x, frame_stride, ntok, gamma, beta,
                       eps, p_clamp_min, y, ldy);
    return sais_check_launch();
}

static bool cov_shape_ok(int N, int Dm) { return N >= 1 && Dm >= CT && Dm % CT == 0 && Dm <= SAIS_COV_MAX_DIM; }

extern "C" size_t sais_colmean_cov_workspace_bytes(int N, int Dm) { return cov_shape_ok(N, Dm) ? cov_plan(N, Dm).bytes : 0; }

extern "C" int sais_colmean_cov(const float* X, long ldx, int N, int Dm, float* mean, float* cov, void* workspace,
                                size_t workspace_bytes, void* stream) {
    SAIS_ENTER();
    if (!X || !mean || !cov || !workspace || !cov_shape_ok(N, Dm) || ldx < Dm || (ldx & 3)) return SAIS_ERR_ARG;
    if (((uintptr_t)X | (uintptr_t)workspace) & 15) return SAIS_ERR_ARG;
    const CovPlan pl = cov_plan(N, Dm);
    if (workspace_bytes < pl.bytes) return SAIS_ERR_ARG;
    float* part = (float*)workspace;
    float* colsum = part + pl.part_floats;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cov_partial_kernel, dim3(pl.tiles, pl.ns), dim3(256), 0, s, X, ldx, N, Dm, pl.T, pl.tiles, pl.rows, part,
                       colsum);
    hipLaunchKernelGGL(cov_reduce_kernel, dim3(pl.tiles * 16 + (Dm + 255) / 256), dim3(256), 0, s, part, colsum, pl.ns, pl.T,
                       pl.tiles, N, Dm, cov, mean);
    return sais_check_launch();
}

extern "C" int sais_center_rows(float* x, long ldx, long rows, int dim, const float* mean, void* stream) {
    SAIS_ENTER();
    if (!x || !mean || rows <= 0 || dim <= 0 || (dim & 3) || ldx < dim || (ldx & 3)) return SAIS_ERR_ARG;
    if (((uintptr_t)x | (uintptr_t)mean) & 15) return SAIS_ERR_ARG;
    hipLaunchKernelGGL(center_rows_kernel, dim3(grid_for(rows * (dim / 4))), dim3(256), 0, (hipStream_t)stream, x, ldx, rows,
                       dim / 4, mean);
    return sais_check_launch();
}

extern "C" int sais_rank_positions(const float* sim, long ld, int Nq, int Ndb, const int* offsets, const int* items, int* pos,
                                   void* stream) {
    SAIS_ENTER();
    if (!sim || !offsets || Nq <= 0 || Ndb <= 0 || Ndb > (1 << 30) || ld < Ndb) return SAIS_ERR_ARG;
    if (!items || !pos) return SAIS_ERR_ARG;
    hipLaunchKernelGGL(rank_positions_kernel, dim3(Nq, RANK_GRID_Y), dim3(256), 0, (hipStream_t)stream, sim, ld, Ndb, offsets,
                       items, pos);
    return sais_check_launch();
}

extern "C" int sais_resize_bilinear_f32(const float* x, int frames, int H, int W, double scale, float* y, int Ho, int Wo,
                                        void* stream) {
    SAIS_ENTER();
    if (!x || !y || frames <= 0 || H <= 0 || W <= 0 || !(scale > 0.0)) return SAIS_ERR_ARG;
    if (Ho != (int)((double)H * scale) || Wo != (int)((double)W * scale) || Ho <= 0 || Wo <= 0) return SAIS_ERR_ARG;
    const float r = (float)(1.0 / scale);                  // the given scale factor, not Ho / H (recompute_scale_factor = None)
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3(grid_for(3L * frames * Ho * Wo)), dim3(256), 0, (hipStream_t)stream, x,
                       3L * frames, H, W, Ho, Wo, r, r, y);
    return sais_check_launch();
}
