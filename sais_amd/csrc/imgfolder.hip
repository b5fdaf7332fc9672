// Image-folder transforms on the GPU: decoded uint8 RGB images of any size, packed in one buffer -> the normalised
// float32 [3,out_h,out_w] tensors the Pillow datasets of the evaluation tools yield, bit for bit:
//   knn.EvalImageFolder.transform     Resize(256, bicubic) + CenterCrop(224)
//   linear.TrainImageFolder.apply     crop box, bilinear to 224 x 224, flip
//   retrieval.ImgListDataset          bicubic to imsize x imsize
// each followed by ToTensor + Normalize.  One SaisImgXform per image says: crop `box`, resample it to rw x rh with Pillow's
// 8-bit ImagingResample (resample.hpp), take the out_w x out_h window at (win_left, win_top) of the result, mirror it if
// `flip`.  Only the output indices of the window are evaluated.
//
// One workgroup per (image, band of output rows): the coefficient rows of the window's columns and of the band's rows are
// computed in the kernel in double (this file is compiled with -ffp-contract=off), the horizontal pass of the input rows the
// band needs goes to LDS as uint8 [rows][out_w][3], rounded and clipped as Pillow stores its intermediate image, and the
// vertical pass reads it, applies the flip and the [3][256] normalisation table, and writes floats x-fastest.  There is
// no uint8 intermediate in global memory.  The band height is chosen per image from the LDS budget.  Everything up to the
// vertical tap is resample.hpp's band (Band, band_lds_bytes, pick_band), shared with augment.hip: the kernel here keeps the
// descriptor check, the source address and the channel-major store with flip and table.
//
// The arithmetic is restated in numpy in tests/resample_ref.py (the geometries and the table: tests/imgfolder_ref.py), which
// tests/test_imgfolder_host.py holds against Pillow.
#include <algorithm>

#include "common.hpp"
#include "resample.hpp"
#include "../../include/sais_hip.h"

namespace {
using namespace resample;
constexpr int THREADS = 256;
constexpr int MAX_OUT = SAIS_IMG_MAX_OUT;
constexpr int MAX_RESAMPLED = 1 << 20;       // rw, rh: far beyond any image, keeps every index inside int
constexpr int LDS_TARGET = 64 * 1024;        // the tallest band that stays below this (two workgroups per CU and more)
constexpr int LDS_LIMIT = 160 * 1024 - 3 * 256 * 4;      // dynamic part: the CU's 160 KiB less the static table

// everything but the LDS fit: the box, the window, the offsets
__host__ __device__ inline bool xform_ok(const SaisImgXform& d, int out_h, int out_w, size_t src_bytes, size_t out_elems) {
    if (d.src_h < 1 || d.src_w < 1 || d.src_h > 65535 || d.src_w > 65535) return false;
    if (d.src_offset < 0 || (size_t)d.src_offset + (size_t)d.src_h * d.src_w * 3 > src_bytes) return false;
    if (!(d.box[0] >= 0 && d.box[1] >= 0 && d.box[2] > d.box[0] && d.box[3] > d.box[1] && d.box[2] <= d.src_w &&
          d.box[3] <= d.src_h))
        return false;
    if (d.rw < 1 || d.rh < 1 || d.rw > MAX_RESAMPLED || d.rh > MAX_RESAMPLED) return false;
    if (d.win_left < 0 || d.win_top < 0 || d.win_left > d.rw - out_w || d.win_top > d.rh - out_h) return false;
    if (d.filter != BILINEAR && d.filter != BICUBIC) return false;
    return d.out_offset >= 0 && (size_t)d.out_offset + (size_t)3 * out_h * out_w <= out_elems;
}

struct Plan { Axis ax, ay; int band, lds; };

__host__ __device__ inline Plan plan_of(const SaisImgXform& d, int out_h, int out_w) {
    Plan p;
    p.ax = make_axis(d.box[2] - d.box[0], d.rw, d.filter);
    p.ay = make_axis(d.box[3] - d.box[1], d.rh, d.filter);
    p.band = pick_band<32, LDS_TARGET, true>(out_h, out_w, p.ax, p.ay);      // no band of twice the output height or more
    p.lds = band_lds_bytes(out_w, p.ax, p.ay, p.band);
    return p;
}

__global__ __launch_bounds__(THREADS) void image_transform_kernel(const unsigned char* __restrict__ src, size_t src_bytes,
                                                                  const SaisImgXform* __restrict__ table, int out_h, int out_w,
                                                                  const float* __restrict__ lut_g, float* __restrict__ out,
                                                                  size_t out_elems, int lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ float lut[3 * 256];
    const SaisImgXform d = table[blockIdx.x];
    if (!xform_ok(d, out_h, out_w, src_bytes, out_elems)) return;      // the host entry checked its copy of the table
    const Plan p = plan_of(d, out_h, out_w);
    if (p.lds > lds_bytes) return;
    const int tid = threadIdx.x, band = p.band;
    const int y0 = blockIdx.y * band;
    if (y0 >= out_h) return;
    const int ny = min(band, out_h - y0);
    for (int i = tid; i < 3 * 256; i += THREADS) lut[i] = lut_g[i];      // visible after the barriers of the band
    const unsigned char* box = src + d.src_offset + ((size_t)d.box[1] * d.src_w + d.box[0]) * 3;
    Band<THREADS> bd;
    if (!bd.fill(lds, p.ax, p.ay, out_w, band, d.win_left, d.win_top + y0, ny, box, d.src_w, tid)) return;

    // vertical pass, flip, ToTensor + Normalize through the table: out[c][y][x], x fastest
    float* dst = out + d.out_offset;
    for (int item = tid; item < 3 * ny * out_w; item += THREADS) {
        const int c = item / (ny * out_w), rem = item - c * ny * out_w, yl = rem / out_w, x = rem - yl * out_w;
        const int xs = d.flip ? out_w - 1 - x : x;
        dst[((size_t)c * out_h + y0 + yl) * out_w + x] = lut[c * 256 + bd.tap(yl, xs * 3 + c)];
    }
}
}  // namespace

extern "C" int sais_image_transform_fits(const SaisImgXform* d, int out_h, int out_w) {
    if (!d || out_h < 1 || out_w < 1 || out_h > MAX_OUT || out_w > MAX_OUT) return 0;
    if (d->box[2] <= d->box[0] || d->box[3] <= d->box[1] || d->rw < 1 || d->rh < 1 || d->rw > MAX_RESAMPLED ||
        d->rh > MAX_RESAMPLED || d->box[2] - (long long)d->box[0] > 65535 || d->box[3] - (long long)d->box[1] > 65535 ||
        (d->filter != BILINEAR && d->filter != BICUBIC))
        return 0;
    return plan_of(*d, out_h, out_w).lds <= LDS_LIMIT ? 1 : 0;
}

extern "C" int sais_image_transform(const unsigned char* src, size_t src_bytes, const SaisImgXform* table_host,
                                    const SaisImgXform* table_dev, int n, int out_h, int out_w, const float* lut, float* out,
                                    size_t out_elems, void* stream) {
    SAIS_ENTER();
    if (!src || !table_host || !table_dev || !lut || !out || n <= 0 || out_h < 1 || out_w < 1 || out_h > MAX_OUT ||
        out_w > MAX_OUT)
        return SAIS_ERR_ARG;
    int lds = 0, max_bands = 0;
    for (int i = 0; i < n; ++i) {
        const SaisImgXform& d = table_host[i];
        if (!xform_ok(d, out_h, out_w, src_bytes, out_elems)) return SAIS_ERR_ARG;
        const Plan p = plan_of(d, out_h, out_w);
        if (p.lds > LDS_LIMIT) return SAIS_ERR_ARG;                    // an extreme downscale: sais_image_transform_fits says so
        lds = std::max(lds, p.lds);
        max_bands = std::max(max_bands, (out_h + p.band - 1) / p.band);
    }
    if (hipFuncSetAttribute((const void*)image_transform_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            LDS_LIMIT) != hipSuccess)
        return sais_check_launch();
    hipLaunchKernelGGL(image_transform_kernel, dim3(n, max_bands), dim3(THREADS), lds, (hipStream_t)stream, src, src_bytes,
                       table_dev, out_h, out_w, lut, out, out_elems, lds);
    return sais_check_launch();
}
