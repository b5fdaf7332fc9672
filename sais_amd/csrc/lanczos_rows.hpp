// Lanczos coefficient rows of Pillow's 8-bit ImagingResample (Resample.c precompute_coeffs + normalize_coeffs_8bpc) for one
// axis with a box [0, in1): host only.  lanczos_filter is sinc(x) * sinc(x / 3) from the C library's sin in double, and one
// differing ulp of a device sin could flip a rounded 22-bit coefficient, so no kernel evaluates it: thumbnail.hip reads the
// rows this header writes from global memory.  The rounding of a coefficient is resample.hpp's (PRECISION_BITS); the
// bilinear / bicubic rows of resample.hpp are not touched by this file.
#pragma once
#include <cmath>

#include "resample.hpp"

namespace lanczos {
struct BoxAxis {
    double in1, scale, support, ss;
    int in, ksize;
};

// the axis of `src` samples after Image.reduce by `factor`: ceil(src / factor) samples, of which the box keeps
// [0, src / factor).  Image.resize hands the box to _imaging.c as C floats ("(ffff)"): the box end is rounded to float.
inline BoxAxis make_axis(int src, int factor, int out) {
    BoxAxis a;
    a.in = (src + factor - 1) / factor;
    a.in1 = (double)(float)((double)src / factor);
    a.scale = a.in1 / out;
    const double filterscale = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 3.0 * filterscale;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    a.ss = 1.0 / filterscale;
    return a;
}

// ImagingResampleInner: a pass runs when the size changes or the box is not the whole axis
inline bool needs_pass(const BoxAxis& a, int out) { return out != a.in || a.in1 != (double)a.in; }

inline double sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

inline double filter(double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0; }

// coefficient row of output index xx: k[0 .. ksize), zero past the taps
inline void row(const BoxAxis& a, int xx, int* k, int& xmin, int& cnt) {
    const double center = 0.0 + (xx + 0.5) * a.scale;
    xmin = (int)(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + a.support + 0.5);
    if (xmax > a.in) xmax = a.in;
    cnt = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < cnt; ++x) ww += filter((x + xmin - center + 0.5) * a.ss);
    for (int x = 0; x < a.ksize; ++x) {
        if (x >= cnt) { k[x] = 0; continue; }
        double w = filter((x + xmin - center + 0.5) * a.ss);
        if (ww != 0.0) w /= ww;
        k[x] = w < 0 ? (int)(-0.5 + w * (1 << resample::PRECISION_BITS)) : (int)(0.5 + w * (1 << resample::PRECISION_BITS));
    }
}
}  // namespace lanczos
