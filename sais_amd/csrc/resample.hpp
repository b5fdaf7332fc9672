// Pillow's 8-bit ImagingResample (Resample.c), the parts every kernel that restates it shares: the geometry of one axis,
// the coefficient row of one output index (computed in double, normalised, rounded to 22-bit integers), the rounding of an
// accumulator.  Used by augment.hip (crop_resize_kernel) and imgfolder.hip (image_transform_kernel); both are compiled with
// -ffp-contract=off, because the host code being restated has no fused multiply-add.
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
__device__ inline void axis_coefs(const Axis& a, int xx, int* k, int& xmin, int& cnt) {
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
}  // namespace resample
