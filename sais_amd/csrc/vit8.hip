// The two kernels the patch-8 DINO ViT (ViT-S/8) adds to the streaming pass of attn_any.hip (gfx950):
//   * the 8 x 8 patch gather (PatchEmbed, dino-main/vision_transformer.py:116-131, Conv2d(3, 384, 8, 8) as a K = 192 GEMM);
//   * the CLS-query attention of the LAST block at ANY token count.  attn_cls.hip keeps the 1 x ntok score row of a (frame, head)
//     in the registers of one wave, which stops at 200 tokens; a patch-8 frame is 785 tokens at 224 x 224 and up to 4097.  Here one
//     workgroup of four waves owns a (frame, head): pass 1 reads K once, leaves the fp32 scores in LDS (4097 x 4 B) and finds the
//     row maximum, pass 2 reads V once and accumulates exp(s - max) v in fp32.  P is never rounded (as in attn_cls.hip), the four
//     waves' partial sums are added in a fixed order: no atomics, bit-reproducible, and a frame's result does not depend on the
//     number of frames in the launch.  Forward only (patch 8 is an inference path).
// Data moves as in attn_cls.hip: lane (r = lane >> 3, c = lane & 7) owns the 16-B piece c of a 128-B head row, a wave instruction
// moves 8 whole rows, the workgroup 32 rows per pass; rows past ntok are reached by clamped loads only.
#include "common.hpp"
#include "../../include/sais_hip.h"

namespace {
constexpr int HD = 64, NH = 6, DM = 384;
constexpr int NW = 4, RPP = 8 * NW;              // waves per workgroup, key rows per pass
constexpr int MAXT = SAIS_VIT_ATTN_ANY_MAX_TOKENS;
constexpr int SC_LEN = (MAXT + RPP - 1) / RPP * RPP;
constexpr float SCALE = 0.125f;                  // 64^-0.5

DEVINL float red_c(float v) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); return v + __shfl_xor(v, 4); }
DEVINL float red_r(float v) { v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); return v + __shfl_xor(v, 32); }

// grid: frames * 6 workgroups, workgroup = (frame, head)
__global__ __launch_bounds__(64 * NW) void attn_cls_any_kernel(const bf16* qkv, long ld, int ntok, bf16* out, long ldo) {
    __shared__ float sc[SC_LEN];                 // scaled scores of the CLS query; [0, ntok) is written
    __shared__ float wmax[NW], wsum[NW];
    __shared__ float wacc[NW][HD];
    const int f = blockIdx.x / NH, h = blockIdx.x - f * NH;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane >> 3, c = lane & 7;
    const bf16* base = qkv + (size_t)f * ntok * ld + h * HD + 8 * c;
    float q[8];
    {
        const bf16x8 qv = *(const bf16x8*)base;  // the CLS row: the only q that is read
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = (float)qv[e];
    }
    const bf16* kp = base + DM;
    const bf16* vp = base + 2 * DM;
    const int npass = (ntok + RPP - 1) / RPP;
    float mx = -INFINITY;
    for (int i = 0; i < npass; ++i) {
        const int k = RPP * i + 8 * w + r;
        const bf16x8 kv = *(const bf16x8*)(kp + (size_t)(k < ntok ? k : ntok - 1) * ld);
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d += (float)kv[e] * q[e];
        const float s = red_c(d) * SCALE;
        if (k < ntok) {
            mx = fmaxf(mx, s);
            if (c == 0) sc[k] = s;
        }
    }
    mx = wave_max(mx);                           // -inf in a wave without a key (ntok < 32): wave 0 always has key 0
    if (lane == 0) wmax[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    float sum = 0.f;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int i = 0; i < npass; ++i) {
        const int k = RPP * i + 8 * w + r;
        const bf16x8 vv = *(const bf16x8*)(vp + (size_t)(k < ntok ? k : ntok - 1) * ld);
        const float p = k < ntok ? __expf(sc[k] - mx) : 0.f;
        sum += p;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += p * (float)vv[e];
    }
    sum = red_r(sum);                            // (the 8 lanes of a row hold the same p)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = red_r(acc[e]);
    if (r == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) wacc[w][8 * c + e] = acc[e];
    }
    if (lane == 0) wsum[w] = sum;
    __syncthreads();
    if (tid < 8) {                               // the waves' partials in a fixed order
        const float inv = 1.0f / (((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int d = 8 * tid + e;
            o[e] = (bf16)((((wacc[0][d] + wacc[1][d]) + wacc[2][d]) + wacc[3][d]) * inv);
        }
        *(bf16x8*)(out + (size_t)f * ldo + h * HD + 8 * tid) = o;
    }
}

// PatchEmbed with 8 x 8 patches on H x W frames: patch rows in row-major order of the (H / 8, W / 8) grid, 192 columns
// (c, py, px).  One thread = one 8-pixel patch row segment: a 32-B load, a 16-B store.
__global__ __launch_bounds__(256) void patchify_rect8_kernel(const float* img, bf16* out, int frames, int H, int W) {
    const int Gh = H >> 3, Gw = W >> 3;
    const long total = (long)frames * 3 * H * Gw;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long t = i;
        const int gx = t % Gw; t /= Gw;
        const int y = t % H; t /= H;
        const int c = t % 3;
        const int f = t / 3;
        const float* src = img + (((size_t)f * 3 + c) * H + y) * W + gx * 8;
        const int gy = y >> 3, py = y & 7;
        bf16* dst = out + ((size_t)f * Gh * Gw + (size_t)gy * Gw + gx) * 192 + c * 64 + py * 8;
        const f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 4);
        bf16x8 d;
        d[0] = (bf16)a[0]; d[1] = (bf16)a[1]; d[2] = (bf16)a[2]; d[3] = (bf16)a[3];
        d[4] = (bf16)b[0]; d[5] = (bf16)b[1]; d[6] = (bf16)b[2]; d[7] = (bf16)b[3];
        *(bf16x8*)dst = d;
    }
}
}  // namespace

extern "C" int sais_vit_attn_cls_fwd_any(const void* qkv, long ldqkv, int frames, int ntok, void* out, long ldo, void* stream) {
    SAIS_ENTER();
    if (!qkv || !out || frames <= 0 || frames > 0x7fffffff / NH || (ldqkv & 7) || (ldo & 7) || ldqkv < 3 * DM || ldo < DM)
        return SAIS_ERR_ARG;
    if (ntok < 2 || ntok > SAIS_VIT_ATTN_ANY_MAX_TOKENS) return SAIS_ERR_ARG;
    hipLaunchKernelGGL(attn_cls_any_kernel, dim3((unsigned)(frames * NH)), dim3(64 * NW), 0, (hipStream_t)stream, (const bf16*)qkv,
                       ldqkv, ntok, (bf16*)out, ldo);
    return sais_check_launch();
}

extern "C" int sais_patchify_rect8(const float* frames_f32, int frames, int H, int W, void* patches_bf16, void* stream) {
    SAIS_ENTER();
    if (!frames_f32 || !patches_bf16 || frames <= 0 || H <= 0 || W <= 0 || (H & 7) || (W & 7)) return SAIS_ERR_ARG;
    const long total = (long)frames * 3 * H * (W >> 3);
    long blocks = (total + 255) / 256;
    blocks = blocks > 65536 ? 65536 : blocks;
    hipLaunchKernelGGL(patchify_rect8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_f32,
                       (bf16*)patches_bf16, frames, H, W);
    return sais_check_launch();
}
