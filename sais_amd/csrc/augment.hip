// DINO multi-crop augmentation on the GPU: decoded uint8 frames -> the normalised float32 views that
// DataAugmentationDINO (sais_amd/dino_data.py; main_dino.py:633-679 of the reference) makes with Pillow, bit for bit.
// The random decisions of a view are drawn on the host (dino_data.draw_view) and arrive as one SaisAugView per view.
//
//   sais_augment_crop_resize   RandomResizedCrop's pixel half: img.crop(box).resize((s, s), BICUBIC) = Pillow's 8-bit
//                              ImagingResample on the CROPPED image (taps clamp at the box).  Every view has its own box,
//                              so its own coefficient rows: they are computed in the kernel in double, as Resample.c
//                              does on the host (this file is compiled with -ffp-contract=off).  One workgroup per
//                              (view, band of output rows); the band itself (coefficient rows, horizontal pass into LDS,
//                              vertical tap out of it) is resample.hpp's, shared with imgfolder.hip: the kernel here
//                              keeps the descriptor check, the source address and the interleaved uint8 store.
//   sais_augment_color         flip, the ColorJitter ops in the drawn order, grayscale, GaussianBlur (three box passes
//                              per axis), solarize, ToTensor + Normalize.  One workgroup per view; the view lives in LDS
//                              from the first op to the last and only floats are written.
//
// The arithmetic is restated in numpy in tests/aug_ref.py (the resampler: tests/resample_ref.py), which
// tests/test_augment_host.py holds against Pillow.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "resample.hpp"
#include "../../include/sais_hip.h"

namespace {
using namespace resample;
constexpr int MAX_SIZE = SAIS_AUG_MAX_SIZE;
constexpr int RESIZE_THREADS = 256;
constexpr int COLOR_THREADS = 1024;
constexpr int LDS_TARGET = 40 * 1024;        // crop_resize picks the tallest band that stays below this
constexpr int LDS_LIMIT = 160 * 1024;
enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3, OP_GRAY = 4 };

struct Border { int left, top, width, height; };

// ---------------------------------------------------------------------------------------------- resampling geometry
// (resample.hpp: Axis, make_axis, band_lds_bytes, pick_band, Band; every view here is bicubic and square)
__host__ __device__ inline int pick_band(int S, const Axis& ax, const Axis& ay) {
    return resample::pick_band<16, LDS_TARGET, false>(S, S, ax, ay);
}

__host__ __device__ inline bool view_geometry_ok(const SaisAugView& v, int nframes, const Border& b, size_t u8_bytes) {
    if (v.size < 1 || v.size > MAX_SIZE) return false;
    if (v.u8_offset < 0 || (size_t)v.u8_offset + (size_t)v.size * v.size * 3 > u8_bytes) return false;
    if (v.frame < 0 || v.frame >= nframes) return false;
    return v.box[0] >= 0 && v.box[1] >= 0 && v.box[2] > v.box[0] && v.box[3] > v.box[1] && v.box[2] <= b.width &&
           v.box[3] <= b.height;
}

__global__ __launch_bounds__(RESIZE_THREADS) void crop_resize_kernel(const unsigned char* __restrict__ frames, int nframes,
                                                                     int H, int W, Border b,
                                                                     const SaisAugView* __restrict__ views,
                                                                     unsigned char* __restrict__ out, size_t out_bytes,
                                                                     int lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const SaisAugView v = views[blockIdx.x];
    if (!view_geometry_ok(v, nframes, b, out_bytes)) return;          // the host entry checked its copy of the table
    const int S = v.size, tid = threadIdx.x;
    const int bw = v.box[2] - v.box[0], bh = v.box[3] - v.box[1];
    const Axis ax = make_axis(bw, S), ay = make_axis(bh, S);
    const int band = pick_band(S, ax, ay);
    if (band_lds_bytes(S, ax, ay, band) > lds_bytes) return;
    const int y0 = blockIdx.y * band;
    if (y0 >= S) return;
    const int ny = min(band, S - y0);
    const unsigned char* box = frames + (((size_t)v.frame * H + b.top + v.box[1]) * W + b.left + v.box[0]) * 3;
    Band<RESIZE_THREADS> bd;
    if (!bd.fill(lds, ax, ay, S, band, 0, y0, ny, box, W, tid)) return;

    // vertical pass: [S][S][3] uint8, x and channel fastest
    const int line = S * 3;
    unsigned char* dst = out + v.u8_offset;
    for (int item = tid; item < ny * line; item += RESIZE_THREADS) {
        const int yl = item / line, rem = item - yl * line;
        dst[(size_t)(y0 + yl) * line + rem] = (unsigned char)bd.tap(yl, rem);
    }
}

// ---------------------------------------------------------------------------------------------- colour chain
// LDS row pitch of a view: bytes of a row rounded to dwords, an odd number of them, so that the threads of the
// horizontal blur passes (one per row) fall on different banks
__host__ __device__ inline int row_pitch(int S) {
    int dw = (S * 3 + 3) / 4;
    if ((dw & 1) == 0) ++dw;
    return dw * 4;
}

__host__ __device__ inline int color_lds_bytes(int S) { return ((S * row_pitch(S) + 15) & ~15) + 3 * 256 * 4 + 64 * 4; }

__device__ inline int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Blend.c: out = in1 + alpha * (in2 - in1) in float; truncated when interpolating, clipped when extrapolating
__device__ inline int blend(int d, int s, float f, bool interp) {
    const float t = (float)d + f * (float)(s - d);
    if (interp) return (int)t & 255;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// Convert.c rgb2hsv + the hue shift + hsv2rgb; float variables, double where the C expression has a double literal
__device__ inline void hue_shift(int& r, int& g, int& b, int shift) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int uv = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        const double hd = (double)h / 6.0 + 1.0;                      // in [5/6, 11/6]: fmod(hd, 1.0) is exact
        h = (float)(hd >= 1.0 ? hd - 1.0 : hd);
        uh = min(max((int)((double)h * 255.0), 0), 255);
        us = min(max((int)((double)s * 255.0), 0), 255);
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        r = g = b = uv;
        return;
    }
    const double hf = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(hf);
    const float f = (float)(hf - (double)(float)i);
    const float fs = (float)((double)(float)us / 255.0);
    const float v = (float)uv;
    const int p = min(max((int)__builtin_round((double)v * (1.0 - (double)fs)), 0), 255);
    const int q = min(max((int)__builtin_round((double)v * (1.0 - (double)fs * (double)f)), 0), 255);
    const int t = min(max((int)__builtin_round((double)v * (1.0 - (double)fs * (1.0 - (double)f))), 0), 255);
    switch (i % 6) {
        case 0: r = uv; g = t; b = p; break;
        case 1: r = q; g = uv; b = p; break;
        case 2: r = p; g = uv; b = t; break;
        case 3: r = p; g = q; b = uv; break;
        case 4: r = t; g = p; b = uv; break;
        default: r = uv; g = p; b = q; break;
    }
}

// BoxBlur.c _gaussian_blur_radius (3 passes) and the constants of ImagingHorizontalBoxBlur
struct Box { int r; unsigned ww, fw; };
__device__ inline Box box_constants(float radius) {
    const float sigma2 = radius * radius / 3;
    const float L = (float)sqrt(12.0 * (double)sigma2 + 1.0);
    const float l = (float)floor(((double)L - 1.0) / 2.0);
    float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    const float fr = l + a;
    Box bx;
    bx.r = (int)fr;
    bx.ww = (unsigned)((float)(1 << 24) / (fr * 2 + 1));
    bx.fw = ((1u << 24) - (unsigned)(bx.r * 2 + 1) * bx.ww) / 2;
    return bx;
}

// one in-place box pass over a line of n bytes `stride` apart; box radius 0 or 1, the line extended by its edge pixels.
// w0..w4 are the source pixels x-2 .. x+2: everything a later output needs is read before its byte is overwritten
__device__ inline void box_line(unsigned char* p, int n, int stride, const Box bx) {
    unsigned w0, w1, w2 = p[0], w3 = p[min(1, n - 1) * stride], w4 = p[min(2, n - 1) * stride];
    w0 = w1 = w2;
    for (int x = 0; x < n; ++x) {
        const unsigned acc = bx.r ? w1 + w2 + w3 : w2;
        const unsigned far = bx.r ? w0 + w4 : w1 + w3;
        const unsigned nxt = p[min(x + 3, n - 1) * stride];
        p[x * stride] = (unsigned char)((acc * bx.ww + far * bx.fw + (1u << 23)) >> 24);
        w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = nxt;
    }
}

__global__ __launch_bounds__(COLOR_THREADS) void color_kernel(const unsigned char* __restrict__ u8, size_t u8_bytes,
                                                              const SaisAugView* __restrict__ views, int size,
                                                              const float* __restrict__ lut_g, float* __restrict__ out,
                                                              size_t out_elems) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const SaisAugView v = views[blockIdx.x];
    if (v.size != size) return;                                        // one launch per distinct view size
    const int S = size, tid = threadIdx.x, pitch = row_pitch(S), npix = S * S;
    if (v.u8_offset < 0 || (size_t)v.u8_offset + (size_t)npix * 3 > u8_bytes || v.out_offset < 0 ||
        (size_t)v.out_offset + (size_t)npix * 3 > out_elems || !(v.blur_radius >= 0.0f && v.blur_radius <= 2.0f))
        return;                                                        // the host entry checked its copy of the table
    unsigned char* px = lds;                                           // [S][pitch], RGB interleaved
    float* lut = (float*)(lds + ((S * pitch + 15) & ~15));             // [3][256]
    unsigned* red = (unsigned*)(lut + 3 * 256);                        // [waves]
    for (int i = tid; i < 3 * 256; i += COLOR_THREADS) lut[i] = lut_g[i];

    // load, mirrored if the view is flipped
    const unsigned char* src = u8 + v.u8_offset;
    for (int i = tid; i < npix * 3; i += COLOR_THREADS) {
        const int y = i / (S * 3), rem = i - y * S * 3, x = rem / 3, c = rem - 3 * x;
        px[y * pitch + x * 3 + c] = src[(y * S + (v.flip ? S - 1 - x : x)) * 3 + c];
    }
    __syncthreads();

    // the pointwise ops in order, 4 bits each; a pass runs up to the next contrast op, which needs the mean of L of
    // the image as it is at that point
    unsigned ops = 0;
    int nops = 0;
    if (v.jitter)
        for (int k = 0; k < 4; ++k) ops |= (unsigned)(v.order[k] & 3) << (4 * nops++);
    if (v.gray) ops |= (unsigned)OP_GRAY << (4 * nops++);
    const float fb = v.brightness, fc = v.contrast, fs = v.saturation;
    const bool ib = fb >= 0.0f && fb <= 1.0f, ic = fc >= 0.0f && fc <= 1.0f, is = fs >= 0.0f && fs <= 1.0f;
    for (int i0 = 0; i0 < nops;) {
        int mean = 0;
        if (((ops >> (4 * i0)) & 15) == OP_CONTRAST) {
            unsigned sum = 0;
            for (int i = tid; i < npix; i += COLOR_THREADS) {
                const unsigned char* p = px + (i / S) * pitch + (i % S) * 3;
                sum += luma(p[0], p[1], p[2]);
            }
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
            if ((tid & 63) == 0) red[tid >> 6] = sum;
            __syncthreads();
            unsigned total = 0;
            for (int w = 0; w < COLOR_THREADS / 64; ++w) total += red[w];
            mean = (int)((double)total / (double)npix + 0.5);          // int(ImageStat.Stat(L).mean[0] + 0.5)
        }
        int i1 = i0 + 1;
        while (i1 < nops && ((ops >> (4 * i1)) & 15) != OP_CONTRAST) ++i1;
        for (int i = tid; i < npix; i += COLOR_THREADS) {
            unsigned char* p = px + (i / S) * pitch + (i % S) * 3;
            int r = p[0], g = p[1], b = p[2];
            for (int k = i0; k < i1; ++k) {
                switch ((ops >> (4 * k)) & 15) {
                    case OP_BRIGHTNESS: r = blend(0, r, fb, ib); g = blend(0, g, fb, ib); b = blend(0, b, fb, ib); break;
                    case OP_CONTRAST: r = blend(mean, r, fc, ic); g = blend(mean, g, fc, ic); b = blend(mean, b, fc, ic); break;
                    case OP_SATURATION: {
                        const int l = luma(r, g, b);
                        r = blend(l, r, fs, is); g = blend(l, g, fs, is); b = blend(l, b, fs, is);
                        break;
                    }
                    case OP_HUE: hue_shift(r, g, b, v.hue_shift); break;
                    default: r = g = b = luma(r, g, b);
                }
            }
            p[0] = (unsigned char)r; p[1] = (unsigned char)g; p[2] = (unsigned char)b;
        }
        __syncthreads();
        i0 = i1;
    }

    // GaussianBlur: three box passes along x, three along y (Pillow transposes, blurs rows and transposes back)
    if (v.blur) {
        const Box bx = box_constants(v.blur_radius);
        for (int pass = 0; pass < 3; ++pass) {
            if (tid < 3 * S) box_line(px + (tid % S) * pitch + tid / S, S, 3, bx);
            __syncthreads();
        }
        for (int pass = 0; pass < 3; ++pass) {
            if (tid < 3 * S) box_line(px + tid, S, pitch, bx);
            __syncthreads();
        }
    }

    // solarize, ToTensor + Normalize through the table: out[c][y][x]
    float* dst = out + v.out_offset;
    for (int i = tid; i < npix * 3; i += COLOR_THREADS) {
        const int c = i / npix, rem = i - c * npix, y = rem / S, x = rem - y * S;
        int val = px[y * pitch + x * 3 + c];
        if (v.solarize && val >= 128) val = 255 - val;
        dst[i] = lut[c * 256 + val];
    }
}

bool order_ok(const int* o) {
    int seen = 0;
    for (int k = 0; k < 4; ++k) {
        if (o[k] < 0 || o[k] > 3) return false;
        seen |= 1 << o[k];
    }
    return seen == 15;
}
}  // namespace

extern "C" size_t sais_augment_workspace_bytes(const SaisAugView* views, int nviews) {
    if (!views || nviews <= 0) return 0;
    size_t need = 0;
    for (int i = 0; i < nviews; ++i) {
        const SaisAugView& v = views[i];
        if (v.size < 1 || v.size > MAX_SIZE || v.u8_offset < 0) return 0;
        const size_t end = (size_t)v.u8_offset + (size_t)v.size * v.size * 3;
        if (end > need) need = end;
    }
    return (need + 255) & ~(size_t)255;
}

extern "C" int sais_augment_crop_resize(const unsigned char* frames, int nframes, int height, int width, const int* border4,
                                        const SaisAugView* views_host, const SaisAugView* views_dev, int nviews,
                                        unsigned char* views_u8, size_t views_u8_bytes, void* stream) {
    SAIS_ENTER();
    if (!frames || !border4 || !views_host || !views_dev || !views_u8 || nframes <= 0 || height <= 0 || width <= 0 ||
        nviews <= 0)
        return SAIS_ERR_ARG;
    const Border b{border4[0], border4[1], border4[2], border4[3]};
    if (b.left < 0 || b.top < 0 || b.width <= 0 || b.height <= 0 || b.left + b.width > width || b.top + b.height > height)
        return SAIS_ERR_ARG;
    int lds = 0, max_bands = 0;
    for (int i = 0; i < nviews; ++i) {
        const SaisAugView& v = views_host[i];
        if (!view_geometry_ok(v, nframes, b, views_u8_bytes)) return SAIS_ERR_ARG;
        const Axis ax = make_axis(v.box[2] - v.box[0], v.size), ay = make_axis(v.box[3] - v.box[1], v.size);
        const int band = pick_band(v.size, ax, ay);
        const int need = band_lds_bytes(v.size, ax, ay, band);
        if (need > LDS_LIMIT) return SAIS_ERR_ARG;                     // a downscale of several hundred to one
        lds = std::max(lds, need);
        max_bands = std::max(max_bands, (v.size + band - 1) / band);
    }
    if (hipFuncSetAttribute((const void*)crop_resize_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_LIMIT) !=
        hipSuccess)
        return sais_check_launch();
    hipLaunchKernelGGL(crop_resize_kernel, dim3(nviews, max_bands), dim3(RESIZE_THREADS), lds, (hipStream_t)stream, frames,
                       nframes, height, width, b, views_dev, views_u8, views_u8_bytes, lds);
    return sais_check_launch();
}

extern "C" int sais_augment_color(const unsigned char* views_u8, size_t views_u8_bytes, const SaisAugView* views_host,
                                  const SaisAugView* views_dev, int nviews, const float* lut, float* out, size_t out_elems,
                                  void* stream) {
    SAIS_ENTER();
    if (!views_u8 || !views_host || !views_dev || !lut || !out || nviews <= 0) return SAIS_ERR_ARG;
    bool sizes[MAX_SIZE + 1] = {};
    for (int i = 0; i < nviews; ++i) {
        const SaisAugView& v = views_host[i];
        if (v.size < 1 || v.size > MAX_SIZE) return SAIS_ERR_ARG;
        const size_t n = (size_t)v.size * v.size * 3;
        if (v.u8_offset < 0 || (size_t)v.u8_offset + n > views_u8_bytes || v.out_offset < 0 ||
            (size_t)v.out_offset + n > out_elems)
            return SAIS_ERR_ARG;
        if (v.jitter && !order_ok(v.order)) return SAIS_ERR_ARG;
        // blend factors as ColorJitter can draw them (the arithmetic was checked on [0, 2]); NaN fails every comparison
        if (v.jitter && !(v.brightness >= 0.0f && v.brightness <= 2.0f && v.contrast >= 0.0f && v.contrast <= 2.0f &&
                          v.saturation >= 0.0f && v.saturation <= 2.0f && v.hue_shift >= -255 && v.hue_shift <= 255))
            return SAIS_ERR_ARG;
        if (!(v.blur_radius >= 0.0f && v.blur_radius <= 2.0f)) return SAIS_ERR_ARG;
        sizes[v.size] = true;
    }
    if (hipFuncSetAttribute((const void*)color_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_LIMIT) != hipSuccess)
        return sais_check_launch();
    for (int s = 1; s <= MAX_SIZE; ++s) {
        if (!sizes[s]) continue;
        hipLaunchKernelGGL(color_kernel, dim3(nviews), dim3(COLOR_THREADS), color_lds_bytes(s), (hipStream_t)stream, views_u8,
                           views_u8_bytes, views_dev, s, lut, out, out_elems);
        const int rc = sais_check_launch();
        if (rc != SAIS_OK) return rc;
    }
    return SAIS_OK;
}
