// Pillow's 8-bit ImagingResample (Resample.c), the one copy of it in the library: the geometry of one axis, the coefficient
// row of one output index (computed in double, normalised, rounded to 22-bit integers), the rounding of an accumulator, and
// the band body (coefficient rows + horizontal pass into LDS, vertical tap out of it) of the kernels that compute their rows
// on the device.  Used by augment.hip (crop_resize_kernel) and imgfolder.hip (image_transform_kernel), both compiled with
// -ffp-contract=off because the host code being restated has no fused multiply-add, and by preprocess.hip, which builds its
// coefficient tables from make_axis / axis_coefs on the host (x86 host code has no fused multiply-add to contract).
#pragma once
#include <cmath>

namespace resample {
constexpr int PRECISION_BITS = 32 - 8 - 2;
enum { BILINEAR = 0, BICUBIC = 1 };

struct Axis {
    double scale, support, ss;
    int in, ksize, filter;
};

// Resample.c precompute_coeffs, box = the whole axis of `in` samples resampled to `out`
__host__ __device__ inline Axis make_axis(int in, int out, int filter = BICUBIC) {
    Axis a;
    a.in = in;
    a.filter = filter;
    a.scale = (double)in / out;
    const double filterscale = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = (filter == BICUBIC ? 2.0 : 1.0) * filterscale;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    a.ss = 1.0 / filterscale;
    return a;
}

__host__ __device__ inline void axis_bounds(const Axis& a, int xx, int& xmin, int& cnt, double& center) {
    center = (xx + 0.5) * a.scale;
    xmin = (int)(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + a.support + 0.5);
    if (xmax > a.in) xmax = a.in;
    cnt = xmax - xmin;
}

__host__ __device__ inline double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

__host__ __device__ inline double bilinear(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

__host__ __device__ inline double filter_weight(int filter, double x) { return filter == BICUBIC ? bicubic(x) : bilinear(x); }

// coefficient row of output index xx: normalised in double, then normalize_coeffs_8bpc
__host__ __device__ inline void axis_coefs(const Axis& a, int xx, int* k, int& xmin, int& cnt) {
    double center;
    axis_bounds(a, xx, xmin, cnt, center);
    double ww = 0.0;
    for (int x = 0; x < cnt; ++x) ww += filter_weight(a.filter, (x + xmin - center + 0.5) * a.ss);
    for (int x = 0; x < cnt; ++x) {
        double w = filter_weight(a.filter, (x + xmin - center + 0.5) * a.ss);
        if (ww != 0.0) w /= ww;
        k[x] = w < 0 ? (int)(-0.5 + w * (1 << PRECISION_BITS)) : (int)(0.5 + w * (1 << PRECISION_BITS));
    }
}

// input rows a band of `band` output rows can touch: first rows of its first and last output row are at most
// (band - 1) * scale + 1 apart, and no row has more than ksize taps
__host__ __device__ inline int band_rows_bound(const Axis& ay, int band) { return (int)((band - 1) * ay.scale) + 2 + ay.ksize; }

__device__ inline int clip8(int acc) {
    const int v = acc >> PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ---------------------------------------------------------------------------------------------- the band
// One workgroup resamples a band of `band` output rows, out_w columns wide: LDS holds the coefficient rows of the columns,
// those of the band's rows, and the horizontally resampled input rows the band needs.
__host__ __device__ inline int band_lds_bytes(int out_w, const Axis& ax, const Axis& ay, int band) {
    const long long ints = (long long)out_w * ax.ksize + 2 * out_w + (long long)band * ay.ksize + 2 * band;
    const long long bytes = ints * 4 + (((long long)band_rows_bound(ay, band) * out_w * 3 + 15) & ~15LL);
    return bytes > (1 << 30) ? (1 << 30) : (int)bytes;
}

// the tallest band of at most MAX_BAND rows whose LDS stays within LDS_TARGET; SHORT_OUT: and below twice the output height
template <int MAX_BAND, int LDS_TARGET, bool SHORT_OUT>
__host__ __device__ inline int pick_band(int out_h, int out_w, const Axis& ax, const Axis& ay) {
    for (int band = MAX_BAND; band > 1; band >>= 1)
        if ((!SHORT_OUT || band < 2 * out_h) && band_lds_bytes(out_w, ax, ay, band) <= LDS_TARGET) return band;
    return 1;
}

template <int THREADS>
struct Band {
    int* vk;                        // [band][ky]
    int* vb;                        // [band][2]
    unsigned char* rows;            // [nrows][out_w][3]
    int ky, line, r0;

    // Output columns first_x .. first_x + out_w - 1 and rows first_y .. first_y + ny - 1 of the resampled box, whose first
    // pixel is at `box` in an image of `pitch` pixels per row: carves `lds` (band_lds_bytes), fills the coefficient rows and
    // runs the horizontal pass of the input rows this band needs, rounded and clipped to uint8 as Pillow stores its
    // intermediate image.  Every thread of the workgroup calls it; false (for all of them) if the rows exceed band_rows_bound.
    __device__ bool fill(unsigned char* lds, const Axis& ax, const Axis& ay, int out_w, int band, int first_x, int first_y,
                         int ny, const unsigned char* box, int pitch, int tid) {
        const int kx = ax.ksize;
        ky = ay.ksize;
        line = out_w * 3;
        int* hk = (int*)lds;                      // [out_w][kx]
        int* hb = hk + out_w * kx;                // [out_w][2]
        vk = hb + 2 * out_w;
        vb = vk + band * ky;
        rows = (unsigned char*)(vb + 2 * band);
        for (int xl = tid; xl < out_w; xl += THREADS) axis_coefs(ax, first_x + xl, hk + xl * kx, hb[2 * xl], hb[2 * xl + 1]);
        for (int yl = tid; yl < ny; yl += THREADS) axis_coefs(ay, first_y + yl, vk + yl * ky, vb[2 * yl], vb[2 * yl + 1]);
        __syncthreads();
        r0 = vb[0];
        const int nrows = vb[2 * (ny - 1)] + vb[2 * (ny - 1) + 1] - r0;
        if (nrows > band_rows_bound(ay, band)) return false;

        const unsigned char* src = box + (size_t)r0 * pitch * 3;
        for (int item = tid; item < nrows * out_w; item += THREADS) {
            const int row = item / out_w, xl = item - row * out_w;
            const int xmin = hb[2 * xl], cnt = hb[2 * xl + 1];
            const int* k = hk + xl * kx;
            const unsigned char* p = src + ((size_t)row * pitch + xmin) * 3;
            int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
            for (int x = 0; x < cnt; ++x) {
                const int kv = k[x];
                a0 += p[3 * x] * kv; a1 += p[3 * x + 1] * kv; a2 += p[3 * x + 2] * kv;
            }
            unsigned char* t = rows + (size_t)item * 3;
            t[0] = (unsigned char)clip8(a0); t[1] = (unsigned char)clip8(a1); t[2] = (unsigned char)clip8(a2);
        }
        __syncthreads();
        return true;
    }

    // the finished byte of output row yl of the band at byte `idx` (3 * column + channel) of the line
    __device__ int tap(int yl, int idx) const {
        const int cnt = vb[2 * yl + 1];
        const int* k = vk + yl * ky;
        const unsigned char* col = rows + (size_t)(vb[2 * yl] - r0) * line + idx;
        int acc = 1 << (PRECISION_BITS - 1);
        for (int y = 0; y < cnt; ++y) acc += col[(size_t)y * line] * k[y];
        return clip8(acc);
    }
};
}  // namespace resample
