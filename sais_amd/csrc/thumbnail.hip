// img.thumbnail((imsize, imsize), Image.LANCZOS) + ToTensor + Normalize on the GPU, bit for bit: the loader of
// eval_image_retrieval.py (retrieval.OxfordParisDataset).  The image was converted to RGB first, so Pillow has no JPEG draft
// mode to use; Image.thumbnail is then (Pillow 12.2):
//   (x, y)   the aspect-preserving size; an image that is not larger is left untouched
//   fx, fy   int(W / x / 2.0) or 1, int(H / y / 2.0) or 1 (reducing_gap = 2.0)
//   reduce   img.reduce((fx, fy)) where a factor exceeds 1: a box average, the last column and row possibly partial
//   resize   resize((x, y), LANCZOS, box = (0, 0, W / fx, H / fy)) with the box ends rounded to C floats
// Image.resize has one more branch: an image that after the reduce is more than 100 times as high as wide, with a lower
// output, gets its VERTICAL pass first.  These kernels run the horizontal pass first, so that geometry is refused
// (SAIS_ERR_ARG, sais_thumbnail_fits answers 0) and the loader hands such a file to Pillow.
// One SaisThumb per image carries that geometry; the sizes, the factors and the output sizes differ per image.
//
// Two kernels.  thumb_reduce_kernel restates Reduce.c: every output pixel is ((sum + n / 2) * multiplier(n)) >> 24 over
// its n source pixels, multiplier(n) = (UINT32)(2^32 / (256 n)) from a FLOAT division (division_UINT32).  Reduce.c's
// special-cased factor pairs shift where n is a power of two, which is the same number.  thumb_resample_kernel is the band
// scheme of resample.hpp with the coefficient rows read from global memory (lanczos_rows.hpp writes them on the host: no
// kernel evaluates sin): one workgroup per (image, band of output rows), the horizontal pass of the input rows the band
// needs into LDS as uint8, rounded and clipped as Pillow stores its intermediate image, then the vertical tap, the
// normalisation table, floats x-fastest.  Pillow skips a pass whose axis keeps its size with a whole box; kx = 0 / ky = 0
// says so and the kernel copies instead.  An untouched image is both passes skipped: a normalised copy.
//
// The arithmetic is restated in numpy in tests/thumb_ref.py, which tests/test_thumbnail_host.py holds against Pillow.
#include <algorithm>

#include "common.hpp"
#include "lanczos_rows.hpp"
#include "resample.hpp"
#include "../../include/sais_hip.h"

namespace {
using resample::PRECISION_BITS;
using resample::clip8;
constexpr int THREADS = 256;
constexpr int MAX_OUT = SAIS_THUMB_MAX_OUT;
constexpr int MAX_SIDE = 65535;
constexpr long long MAX_PIXELS = 1LL << 28;  // src_w * src_h: every pixel index inside int
constexpr int MAX_BLOCK = 65536;             // fx * fy: 256 * n stays exact in a float and every sum inside 32 bits
constexpr int MAX_BAND = 32;
constexpr int LDS_TARGET = 64 * 1024;        // the tallest band that stays below this (two workgroups per CU and more)
constexpr int LDS_LIMIT = 160 * 1024 - 3 * 256 * 4;      // dynamic part: the CU's 160 KiB less the static table
constexpr int REDUCE_MAX_CHUNKS = 1024;      // workgroups per image of the reduce launch (grid-stride beyond)

__host__ __device__ inline bool reduced(const SaisThumb& d) { return d.fx > 1 || d.fy > 1; }

// the geometry alone: sizes, factors, taps.  No buffer is consulted
__host__ __device__ inline bool geometry_ok(const SaisThumb& d) {
    if (d.src_h < 1 || d.src_w < 1 || d.src_h > MAX_SIDE || d.src_w > MAX_SIDE) return false;
    if ((long long)d.src_h * d.src_w > MAX_PIXELS) return false;
    if (d.fx < 1 || d.fy < 1 || d.fx > MAX_SIDE || d.fy > MAX_SIDE || (long long)d.fx * d.fy > MAX_BLOCK) return false;
    if (d.rw != (d.src_w + d.fx - 1) / d.fx || d.rh != (d.src_h + d.fy - 1) / d.fy) return false;
    if (d.out_w < 1 || d.out_h < 1 || d.out_w > MAX_OUT || d.out_h > MAX_OUT) return false;
    if (d.kx < 0 || d.ky < 0 || d.kx > MAX_SIDE || d.ky > MAX_SIDE) return false;
    if ((d.kx == 0 && d.out_w != d.rw) || (d.ky == 0 && d.out_h != d.rh)) return false;     // a skipped pass keeps the size
    if ((long long)d.rh > 100LL * d.rw && d.out_h < d.rh) return false;     // Image.resize runs the vertical pass first there
    return true;
}

__host__ __device__ inline bool thumb_ok(const SaisThumb& d, size_t src_bytes, size_t coef_ints, size_t ws_bytes,
                                         size_t out_elems) {
    if (!geometry_ok(d)) return false;
    if (d.src_offset < 0 || (size_t)d.src_offset + (size_t)d.src_h * d.src_w * 3 > src_bytes) return false;
    if (reduced(d) && (d.ws_offset < 0 || (size_t)d.ws_offset + (size_t)d.rh * d.rw * 3 > ws_bytes)) return false;
    if (d.kx && (d.cx_offset < 0 || (size_t)d.cx_offset + (size_t)d.out_w * (2 + d.kx) > coef_ints)) return false;
    if (d.ky && (d.cy_offset < 0 || (size_t)d.cy_offset + (size_t)d.out_h * (2 + d.ky) > coef_ints)) return false;
    return d.out_offset >= 0 && (size_t)d.out_offset + (size_t)3 * d.out_h * d.out_w <= out_elems;
}

// input rows a band of `band` output rows can touch (resample::band_rows_bound with the box's scale); a skipped pass: its own
__host__ __device__ inline int rows_bound(const SaisThumb& d, int band) {
    if (d.ky == 0) return band;
    const double scale = (double)(float)((double)d.src_h / d.fy) / d.out_h;
    return (int)((band - 1) * scale) + 2 + d.ky;
}

__host__ __device__ inline long long band_lds(const SaisThumb& d, int band) {
    return ((long long)rows_bound(d, band) * d.out_w * 3 + 15) & ~15LL;
}

// the tallest band below twice the output height whose rows stay within LDS_TARGET; one row if none does
__host__ __device__ inline int pick_band(const SaisThumb& d) {
    for (int band = MAX_BAND; band > 1; band >>= 1)
        if (band < 2 * d.out_h && band_lds(d, band) <= LDS_TARGET) return band;
    return 1;
}

// Reduce.c division_UINT32(n, 8).  The division is correctly rounded on the device (hipcc's default for fp32 '/'), as on the host
__host__ __device__ inline unsigned reduce_multiplier(unsigned n) { return (unsigned)(4294967296.0f / (float)(256u * n)); }

__global__ __launch_bounds__(THREADS) void thumb_reduce_kernel(const unsigned char* __restrict__ src, size_t src_bytes,
                                                               const SaisThumb* __restrict__ table, size_t coef_ints,
                                                               unsigned char* __restrict__ ws, size_t ws_bytes,
                                                               size_t out_elems) {
    const SaisThumb d = table[blockIdx.x];
    if (!thumb_ok(d, src_bytes, coef_ints, ws_bytes, out_elems) || !reduced(d)) return;
    const unsigned char* in = src + d.src_offset;
    unsigned char* dst = ws + d.ws_offset;
    const int total = d.rw * d.rh;
    for (int p = blockIdx.y * THREADS + threadIdx.x; p < total; p += gridDim.y * THREADS) {
        const int oy = p / d.rw, ox = p - oy * d.rw;
        const int x0 = ox * d.fx, y0 = oy * d.fy;
        const int bw = min(d.fx, d.src_w - x0), bh = min(d.fy, d.src_h - y0);       // partial at the right and bottom edge
        const unsigned n = (unsigned)(bw * bh);
        unsigned s0 = n / 2, s1 = s0, s2 = s0;
        for (int yy = 0; yy < bh; ++yy) {
            const unsigned char* q = in + ((size_t)(y0 + yy) * d.src_w + x0) * 3;
            for (int xx = 0; xx < bw; ++xx) { s0 += q[3 * xx]; s1 += q[3 * xx + 1]; s2 += q[3 * xx + 2]; }
        }
        const unsigned m = reduce_multiplier(n);
        unsigned char* t = dst + (size_t)p * 3;
        t[0] = (unsigned char)((s0 * m) >> 24); t[1] = (unsigned char)((s1 * m) >> 24); t[2] = (unsigned char)((s2 * m) >> 24);
    }
}

__global__ __launch_bounds__(THREADS) void thumb_resample_kernel(const unsigned char* __restrict__ src, size_t src_bytes,
                                                                 const SaisThumb* __restrict__ table,
                                                                 const int* __restrict__ coef, size_t coef_ints,
                                                                 const unsigned char* __restrict__ ws, size_t ws_bytes,
                                                                 const float* __restrict__ lut_g, float* __restrict__ out,
                                                                 size_t out_elems, int lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rows[];      // [nrows][out_w][3]
    __shared__ float lut[3 * 256];
    const SaisThumb d = table[blockIdx.x];
    if (!thumb_ok(d, src_bytes, coef_ints, ws_bytes, out_elems)) return;      // the host entry checked its copy of the table
    const int tid = threadIdx.x, band = pick_band(d);
    if (band_lds(d, band) > lds_bytes) return;
    const int y0 = blockIdx.y * band;
    if (y0 >= d.out_h) return;
    const int ny = min(band, d.out_h - y0), out_w = d.out_w, line = out_w * 3;
    for (int i = tid; i < 3 * 256; i += THREADS) lut[i] = lut_g[i];           // visible after the barrier below
    const unsigned char* in = reduced(d) ? ws + d.ws_offset : src + d.src_offset;          // uint8 [rh][rw][3]

    // the input rows of this band
    const int* vb = coef + d.cy_offset;                                       // [out_h][2], then [out_h][ky]
    const int* vk = vb + 2 * d.out_h;
    int r0 = y0, nrows = ny;
    if (d.ky) {
        r0 = vb[2 * y0];
        nrows = vb[2 * (y0 + ny - 1)] + vb[2 * (y0 + ny - 1) + 1] - r0;
    }
    if (r0 < 0 || nrows < 1 || nrows > rows_bound(d, band) || r0 + nrows > d.rh) return;

    // horizontal pass (or the rows as they are), rounded and clipped to uint8
    const int* hb = coef + d.cx_offset;                                       // [out_w][2], then [out_w][kx]
    const int* hk = hb + 2 * out_w;
    const unsigned char* first = in + (size_t)r0 * d.rw * 3;
    for (int item = tid; item < nrows * out_w; item += THREADS) {
        const int row = item / out_w, xl = item - row * out_w;
        unsigned char* t = rows + (size_t)item * 3;
        if (d.kx == 0) {
            const unsigned char* p = first + ((size_t)row * d.rw + xl) * 3;
            t[0] = p[0]; t[1] = p[1]; t[2] = p[2];
            continue;
        }
        const int xmin = hb[2 * xl];
        int cnt = hb[2 * xl + 1];
        if (xmin < 0 || cnt < 0 || cnt > d.kx || xmin + cnt > d.rw) cnt = 0;  // the host entry refused such a row
        const int* k = hk + (size_t)xl * d.kx;
        const unsigned char* p = first + ((size_t)row * d.rw + xmin) * 3;
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int x = 0; x < cnt; ++x) {
            const int kv = k[x];
            a0 += p[3 * x] * kv; a1 += p[3 * x + 1] * kv; a2 += p[3 * x + 2] * kv;
        }
        t[0] = (unsigned char)clip8(a0); t[1] = (unsigned char)clip8(a1); t[2] = (unsigned char)clip8(a2);
    }
    __syncthreads();

    // vertical pass (or the row as it is), ToTensor + Normalize through the table: out[c][y][x], x fastest
    float* dst = out + d.out_offset;
    for (int item = tid; item < 3 * ny * out_w; item += THREADS) {
        const int c = item / (ny * out_w), rem = item - c * ny * out_w, yl = rem / out_w, x = rem - yl * out_w;
        int v;
        if (d.ky == 0) {
            v = rows[(size_t)yl * line + x * 3 + c];
        } else {
            const int ymin = vb[2 * (y0 + yl)];
            int cnt = vb[2 * (y0 + yl) + 1];
            if (ymin < r0 || cnt < 0 || cnt > d.ky || ymin + cnt > r0 + nrows) cnt = 0;
            const int* k = vk + (size_t)(y0 + yl) * d.ky;
            const unsigned char* col = rows + (size_t)(ymin - r0) * line + x * 3 + c;
            int acc = 1 << (PRECISION_BITS - 1);
            for (int y = 0; y < cnt; ++y) acc += col[(size_t)y * line] * k[y];
            v = clip8(acc);
        }
        dst[((size_t)c * d.out_h + y0 + yl) * out_w + x] = lut[c * 256 + v];
    }
}

// the rows of one axis as the kernel will read them: every tap inside the input, and (vertical) every band inside its bound
bool axis_rows_ok(const int* b, int out, int k, int in) {
    for (int i = 0; i < out; ++i)
        if (b[2 * i] < 0 || b[2 * i + 1] < 1 || b[2 * i + 1] > k || b[2 * i] + b[2 * i + 1] > in) return false;
    return true;
}

bool bands_ok(const SaisThumb& d, const int* vb, int band) {
    for (int y0 = 0; y0 < d.out_h; y0 += band) {
        const int last = std::min(y0 + band, d.out_h) - 1, r0 = vb[2 * y0], r1 = vb[2 * last] + vb[2 * last + 1];
        if (r1 - r0 < 1 || r1 - r0 > rows_bound(d, band)) return false;
        for (int y = y0; y <= last; ++y)
            if (vb[2 * y] < r0 || vb[2 * y] + vb[2 * y + 1] > r1) return false;
    }
    return true;
}
}  // namespace

extern "C" int sais_lanczos_rows(int src_size, int factor, int out_size, int* bounds, int* coefs, int ksize) {
    if (src_size < 1 || factor < 1 || out_size < 1 || src_size > MAX_SIDE || factor > MAX_SIDE || out_size > MAX_SIDE)
        return SAIS_ERR_ARG;
    const lanczos::BoxAxis a = lanczos::make_axis(src_size, factor, out_size);
    if (!lanczos::needs_pass(a, out_size)) return 0;                        // Pillow skips this pass
    if (!bounds && !coefs) return a.ksize;                                  // the size query
    if (!bounds || !coefs || ksize != a.ksize) return SAIS_ERR_ARG;
    for (int xx = 0; xx < out_size; ++xx) lanczos::row(a, xx, coefs + (size_t)xx * ksize, bounds[2 * xx], bounds[2 * xx + 1]);
    return a.ksize;
}

extern "C" int sais_thumbnail_fits(const SaisThumb* d) {
    return d && geometry_ok(*d) && band_lds(*d, 1) <= LDS_LIMIT ? 1 : 0;
}

extern "C" size_t sais_thumbnail_workspace_bytes(const SaisThumb* table_host, int n) {
    if (!table_host || n < 1 || n > 65535) return 0;
    size_t need = 256;                                                       // never 0 for a valid table
    for (int i = 0; i < n; ++i) {
        const SaisThumb& d = table_host[i];
        if (!geometry_ok(d) || (reduced(d) && d.ws_offset < 0)) return 0;
        if (reduced(d)) need = std::max(need, (size_t)d.ws_offset + (size_t)d.rh * d.rw * 3);
    }
    return need;
}

extern "C" int sais_thumbnail(const unsigned char* src, size_t src_bytes, const SaisThumb* table_host,
                              const SaisThumb* table_dev, int n, const int* coef_host, const int* coef_dev, size_t coef_ints,
                              unsigned char* ws, size_t ws_bytes, const float* lut, float* out, size_t out_elems,
                              void* stream) {
    SAIS_ENTER();
    if (!src || !table_host || !table_dev || !coef_host || !coef_dev || !ws || !lut || !out || n < 1 || n > 65535)
        return SAIS_ERR_ARG;
    long long lds = 0;
    int max_bands = 0, max_chunks = 0;
    for (int i = 0; i < n; ++i) {
        const SaisThumb& d = table_host[i];
        if (!thumb_ok(d, src_bytes, coef_ints, ws_bytes, out_elems)) return SAIS_ERR_ARG;
        if (band_lds(d, 1) > LDS_LIMIT) return SAIS_ERR_ARG;                 // sais_thumbnail_fits says so
        const int band = pick_band(d);
        if (d.kx && !axis_rows_ok(coef_host + d.cx_offset, d.out_w, d.kx, d.rw)) return SAIS_ERR_ARG;
        if (d.ky && (!axis_rows_ok(coef_host + d.cy_offset, d.out_h, d.ky, d.rh) || !bands_ok(d, coef_host + d.cy_offset, band)))
            return SAIS_ERR_ARG;
        lds = std::max(lds, band_lds(d, band));
        max_bands = std::max(max_bands, (d.out_h + band - 1) / band);
        if (reduced(d)) max_chunks = std::max(max_chunks, std::min(REDUCE_MAX_CHUNKS, (d.rw * d.rh + THREADS - 1) / THREADS));
    }
    if (lds > LDS_LIMIT) return SAIS_ERR_ARG;
    if (max_chunks)
        hipLaunchKernelGGL(thumb_reduce_kernel, dim3(n, max_chunks), dim3(THREADS), 0, (hipStream_t)stream, src, src_bytes,
                           table_dev, coef_ints, ws, ws_bytes, out_elems);
    if (hipFuncSetAttribute((const void*)thumb_resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_LIMIT) !=
        hipSuccess)
        return sais_check_launch();
    hipLaunchKernelGGL(thumb_resample_kernel, dim3(n, max_bands), dim3(THREADS), (int)lds, (hipStream_t)stream, src, src_bytes,
                       table_dev, coef_dev, coef_ints, ws, ws_bytes, lut, out, out_elems, (int)lds);
    return sais_check_launch();
}
