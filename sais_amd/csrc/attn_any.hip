// Streaming self-attention forward of the DINO ViT for ANY token count (dense features at other resolutions than 224 / 96:
// dino-main/eval_video_segmentation.py runs 480 x 832 frames = 1561 tokens), and the rectangular patch gather that feeds it.
//   Attention.forward — dino-main/vision_transformer.py:80-92, inference only (no probabilities, no backward).
// attn_vit.hip keeps the whole K and V of a head in LDS, which stops at a few hundred tokens.  Here K and V arrive in tiles of 64
// keys: the tile body is attn_stream_tile (attn_stream.hpp), shared with the segmented launch of attn_seg.hip.  This kernel is its
// one-token-count case: frame f of the launch is rows f ntok .. (f + 1) ntok - 1.
#include "attn_stream.hpp"
#include "../../include/sais_hip.h"

namespace {
// grid (query tiles of 16 NW, heads, frames); NW waves of 16 queries each
template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_stream_kernel(const bf16* qkv, long ldq, int ntok, bf16* out, long ldo, float* lse,
                                                              float scale) {
    const int h = blockIdx.y, f = blockIdx.z;
    attn_stream_tile<NW>(qkv + (size_t)f * ntok * ldq + h * HD, ldq, ntok, blockIdx.x * (16 * NW), out, (size_t)f * ntok, h, ldo,
                         lse, ((size_t)f * NH + h) * ntok, scale);
}

// PatchEmbed on H x W frames: as patchify_kernel (misc.hip) with a (H / 16, W / 16) grid, patch rows in row-major grid order,
// the same 768 columns (c, py, px).  One thread = one 16-pixel patch row segment.
__global__ __launch_bounds__(256) void patchify_rect_kernel(const float* img, bf16* out, int frames, int H, int W) {
    const int Gh = H >> 4, Gw = W >> 4;
    const long total = (long)frames * 3 * H * Gw;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long t = i;
        const int gx = t % Gw; t /= Gw;
        const int y = t % H; t /= H;
        const int c = t % 3;
        const int f = t / 3;
        const float* src = img + (((size_t)f * 3 + c) * H + y) * W + gx * 16;
        const int gy = y >> 4, py = y & 15;
        bf16* dst = out + ((size_t)f * Gh * Gw + (size_t)gy * Gw + gx) * 768 + c * 256 + py * 16;
        patch_row16(src, dst);
    }
}
}  // namespace

extern "C" int sais_vit_attn_fwd_any(const void* qkv, long ldqkv, int frames, int ntok, void* out, long ldo, float* lse,
                                     void* stream) {
    SAIS_ENTER();
    if (!qkv || !out || frames <= 0 || frames > 65535 || (ldqkv & 7) || (ldo & 3) || ldqkv < 3 * DM || ldo < DM) return SAIS_ERR_ARG;
    if (ntok < 2 || ntok > SAIS_VIT_ATTN_ANY_MAX_TOKENS) return SAIS_ERR_ARG;
    // 64-query workgroups (4 waves) unless they would leave the chip short of two workgroups per CU: then 32-query ones.  One
    // 480 x 832 frame (1561 tokens) is 6 x 25 = 150 workgroups of 64 queries on 256 CUs, 294 of 32.
    const long wg64 = (long)frames * NH * ((ntok + 63) / 64);
    if (wg64 >= 512) {
        hipLaunchKernelGGL(attn_stream_kernel<4>, dim3((ntok + 63) / 64, NH, frames), dim3(256), 0, (hipStream_t)stream,
                           (const bf16*)qkv, ldqkv, ntok, (bf16*)out, ldo, lse, 0.125f);
    } else {
        hipLaunchKernelGGL(attn_stream_kernel<2>, dim3((ntok + 31) / 32, NH, frames), dim3(128), 0, (hipStream_t)stream,
                           (const bf16*)qkv, ldqkv, ntok, (bf16*)out, ldo, lse, 0.125f);
    }
    return sais_check_launch();
}

extern "C" int sais_patchify_rect(const float* frames_f32, int frames, int H, int W, void* patches_bf16, void* stream) {
    SAIS_ENTER();
    if (!frames_f32 || !patches_bf16 || frames <= 0 || H <= 0 || W <= 0 || (H & 15) || (W & 15)) return SAIS_ERR_ARG;
    const long total = (long)frames * 3 * H * (W >> 4);
    long blocks = (total + 255) / 256;
    blocks = blocks > 65536 ? 65536 : blocks;
    hipLaunchKernelGGL(patchify_rect_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_f32,
                       (bf16*)patches_bf16, frames, H, W);
    return sais_check_launch();
}
