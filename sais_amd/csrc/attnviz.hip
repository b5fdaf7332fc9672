// Attention-map rendering for video frames (dino-main/video_generation.py, visualize_attention.py):
//   sais_vit_cls_probs    row 0 of the last block's softmax (Attention.forward, vision_transformer.py:83-90) at any token count
//   sais_attn_mass_mask   "keep xx% of the mass" (video_generation.py:197-205): sort, normalise, cumsum, compare, un-sort
//   sais_attn_render      the masked head mean (:229-238) and matplotlib's Normalize + colormap + nearest upsampling (:207-226, :233)
//
// CLS probabilities.  One workgroup per (frame, head); lane (r = lane >> 3, c = lane & 7) owns the 16-B piece c of the key rows
// 32 i + 8 wave + r, as csrc/attn_cls.hip does: a wave instruction moves 8 whole 128-B head rows of K, a dot product is a
// reduction over the 8 lanes of a row group.  The scaled scores go to LDS (at most 4097 floats), then maximum, exp and sum over
// the row in fp32 and one store per key.  One pass over K, no V.  The work of a row is the same in every launch: its result does
// not depend on the number of frames.
//
// Mass mask.  One workgroup per row: (value, index) keys — the value's bits made order-preserving in the high word, the index in
// the low word, so equal values keep ascending index order (the stable rule) — are sorted in LDS by a bitonic network; the
// inclusive cumulative sum runs in fp64 (16 consecutive elements per thread, then a serial scan of the 256 partials: one fixed
// order), element j is kept iff cum_j / total > 1 - threshold, and the flags are scattered back by index.
//
// Render.  This file is compiled with -ffp-contract=off: the heat map and the colour index restate numpy's f32 arithmetic
// (multiply, divide, add; subtract, divide, scale by 256, truncate) bit for bit.
#include "common.hpp"
#include "../../include/sais_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------- CLS probabilities
constexpr int HD = 64, NH = 6, DM = 384;
constexpr int MAXTOK = SAIS_VIT_ATTN_ANY_MAX_TOKENS;
constexpr float SCALE = 0.125f;                  // 64^-0.5

DEVINL float red_c(float v) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); return v + __shfl_xor(v, 4); }

__global__ __launch_bounds__(256) void cls_probs_kernel(const bf16* q, long ldq, const bf16* k, long ldk, int ntok, float* probs) {
    __shared__ float sc[MAXTOK + 7];
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane >> 3, c = lane & 7;
    const int f = blockIdx.x / NH, h = blockIdx.x - f * NH;
    float qf[8];
    {
        const bf16x8 v = *(const bf16x8*)(q + (size_t)f * ldq + h * HD + 8 * c);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[e] = (float)v[e];
    }
    const bf16* kp = k + (size_t)f * ntok * ldk + h * HD + 8 * c;
    for (int k0 = 8 * wv + r; k0 < ntok; k0 += 128) {         // four independent row groups in flight per wave
        bf16x8 kv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) kv[u] = *(const bf16x8*)(kp + (size_t)min(k0 + 32 * u, ntok - 1) * ldk);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) s = __builtin_fmaf((float)kv[u][e], qf[e], s);
            s = red_c(s) * SCALE;
            if (c == 0 && k0 + 32 * u < ntok) sc[k0 + 32 * u] = s;       // keys past ntok never enter the maximum
        }
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int j = tid; j < ntok; j += 256) mx = fmaxf(mx, sc[j]);
    mx = wave_max(mx);
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int j = tid; j < ntok; j += 256) {                   // (a thread reads back only what it wrote itself)
        const float e = __expf(sc[j] - mx);
        sc[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wv] = sum;
    __syncthreads();
    const float inv = 1.0f / (((red[4] + red[5]) + red[6]) + red[7]);
    float* out = probs + (size_t)blockIdx.x * ntok;
    for (int j = tid; j < ntok; j += 256) out[j] = sc[j] * inv;
}

// ---------------------------------------------------------------------------------------------- mass mask
constexpr int MAXN = SAIS_ATTN_MASK_MAX_N;

// f32 bits -> u32 with the same order (-0 is taken as +0 first: equal values must compare equal)
DEVINL unsigned ord_of(float v) {
    const unsigned b = __float_as_uint(v + 0.0f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
DEVINL float val_of(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

__global__ __launch_bounds__(256) void mass_mask_kernel(const float* p, long ldp, int n, double cut, unsigned char* keep) {
    __shared__ unsigned long long keys[MAXN];
    __shared__ double part[256];
    __shared__ double total;
    const int tid = threadIdx.x;
    const float* row = p + (size_t)blockIdx.x * ldp;
    int P = 256;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += 256)
        keys[i] = i < n ? ((unsigned long long)ord_of(row[i]) << 32) | (unsigned)i : ~0ull;      // padding sorts last
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const unsigned long long a = keys[i], b = keys[i + j];
                if ((a > b) == ((i & kk) == 0)) { keys[i] = b; keys[i + j] = a; }
            }
            __syncthreads();
        }
    const int E = P >> 8, e0 = tid * E;                       // sorted elements e0 .. e0 + E - 1 are this thread's
    double s = 0.0;
    for (int e = 0; e < E; ++e)
        if (e0 + e < n) s += (double)val_of((unsigned)(keys[e0 + e] >> 32));
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double run = 0.0;
        for (int t = 0; t < 256; ++t) { const double v = part[t]; part[t] = run; run += v; }
        total = run;
    }
    __syncthreads();
    const double tot = total;
    double cum = part[tid];
    unsigned char* out = keep + (size_t)blockIdx.x * n;
    for (int e = 0; e < E; ++e) {
        if (e0 + e >= n) break;
        const unsigned long long key = keys[e0 + e];
        cum += (double)val_of((unsigned)(key >> 32));
        out[(unsigned)key] = (tot > 0.0 && cum / tot > cut) ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------- heat map + colour image
constexpr int RNB = SAIS_ATTN_RENDER_WS_FLOATS / 2;         // partial (min, max) pairs per frame: ceil(4096 / 256)

// grid (ceil(n / 256), frames): heat[f, j] = sum over the heads, ascending, of (p * keep) / nheads, starting from the first term
__global__ __launch_bounds__(256) void heat_kernel(const float* p, long ldp, const unsigned char* keep, int nh_total, int head0,
                                                   int nheads, int n, float* heat, float* ws) {
    __shared__ float smn[4], smx[4];
    const int f = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const float nhf = (float)nheads;
    float acc = 0.f;
    if (j < n) {
        for (int hh = 0; hh < nheads; ++hh) {
            const size_t rowi = (size_t)f * nh_total + head0 + hh;
            const float m = keep ? (keep[rowi * n + j] ? 1.0f : 0.0f) : 1.0f;
            const float term = (p[rowi * ldp + j] * m) / nhf;
            acc = hh == 0 ? term : acc + term;
        }
        heat[(size_t)f * n + j] = acc;
    }
    if (!ws) return;
    float mn = j < n ? acc : INFINITY, mx = j < n ? acc : -INFINITY;
    mn = -wave_max(-mn); mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[((size_t)f * RNB + blockIdx.x) * 2] = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
        ws[((size_t)f * RNB + blockIdx.x) * 2 + 1] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
    }
}

// grid (ceil(H W / 256), frames), one thread per output pixel: Normalize (x - vmin, / (vmax - vmin), all zero for a constant
// map), Colormap.__call__ (x 256, the value 256 -> 255, truncation), the byte table, and the patch's colour to its pixels
__global__ __launch_bounds__(256) void colour_kernel(const float* heat, const float* ws, int nparts, int h, int w, int patch,
                                                     const unsigned char* lut, unsigned char* rgb) {
    __shared__ unsigned char slut[768];
    __shared__ float svmin, svmax;
    const int f = blockIdx.y, n = h * w;
    for (int i = threadIdx.x; i < 768; i += 256) slut[i] = lut[i];
    if (threadIdx.x == 0) {
        float mn = INFINITY, mx = -INFINITY;
        for (int b = 0; b < nparts; ++b) {
            mn = fminf(mn, ws[((size_t)f * RNB + b) * 2]);
            mx = fmaxf(mx, ws[((size_t)f * RNB + b) * 2 + 1]);
        }
        svmin = mn; svmax = mx;
    }
    __syncthreads();
    const int H = h * patch, W = w * patch;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    const float v = heat[(size_t)f * n + (y / patch) * w + x / patch];
    const float vmin = svmin, vmax = svmax;
    int idx = 0;
    if (vmin != vmax) {
        float t = (v - vmin) / (vmax - vmin);
        t *= 256.0f;
        idx = t == 256.0f ? 255 : (int)t;
        idx = min(max(idx, 0), 255);
    }
    unsigned char* o = rgb + ((size_t)f * H * W + i) * 3;
    o[0] = slut[3 * idx]; o[1] = slut[3 * idx + 1]; o[2] = slut[3 * idx + 2];
}

}  // namespace

extern "C" int sais_vit_cls_probs(const void* q, long ldq, const void* k, long ldk, int frames, int ntok, float* probs,
                                  void* stream) {
    SAIS_ENTER();
    if (!q || !k || !probs || frames <= 0 || ntok < 2 || ntok > MAXTOK) return SAIS_ERR_ARG;
    if (ldq < DM || ldk < DM || (ldq & 7) || (ldk & 7) || ((uintptr_t)q & 15) || ((uintptr_t)k & 15)) return SAIS_ERR_ARG;
    if ((long)frames * NH > 0x7fffffffL) return SAIS_ERR_ARG;
    hipLaunchKernelGGL(cls_probs_kernel, dim3(frames * NH), dim3(256), 0, (hipStream_t)stream, (const bf16*)q, ldq, (const bf16*)k,
                       ldk, ntok, probs);
    return sais_check_launch();
}

extern "C" int sais_attn_mass_mask(const float* p, long ldp, int rows, int n, double threshold, unsigned char* keep,
                                   void* stream) {
    SAIS_ENTER();
    if (!p || !keep || rows <= 0 || n < 1 || n > MAXN || ldp < n || !(threshold > 0.0 && threshold < 1.0)) return SAIS_ERR_ARG;
    hipLaunchKernelGGL(mass_mask_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, p, ldp, n, 1.0 - threshold, keep);
    return sais_check_launch();
}

extern "C" int sais_attn_render(const float* p, long ldp, const unsigned char* keep, int frames, int nh_total, int head0,
                                int nheads, int h, int w, int n, int patch, const unsigned char* lut, float* heat,
                                unsigned char* rgb, float* workspace, void* stream) {
    SAIS_ENTER();
    if (!p || !heat || (rgb && (!lut || !workspace))) return SAIS_ERR_ARG;
    if (frames <= 0 || frames > 65535 || nh_total <= 0 || head0 < 0 || nheads <= 0 || head0 > nh_total - nheads) return SAIS_ERR_ARG;
    if (h < 1 || w < 1 || n < 1 || n > MAXN || (long)h * w != n || ldp < n || patch < 1 || patch > 64) return SAIS_ERR_ARG;
    const int nparts = (n + 255) / 256;                    // <= RNB
    hipLaunchKernelGGL(heat_kernel, dim3(nparts, frames), dim3(256), 0, (hipStream_t)stream, p, ldp, keep, nh_total, head0, nheads,
                       n, heat, rgb ? workspace : (float*)nullptr);
    if (rgb) {
        const int npix = h * patch * w * patch;            // <= 4096 * 4096
        hipLaunchKernelGGL(colour_kernel, dim3((npix + 255) / 256, frames), dim3(256), 0, (hipStream_t)stream, (const float*)heat,
                           (const float*)workspace, nparts, h, w, patch, lut, rgb);
    }
    return sais_check_launch();
}
