// Streaming self-attention forward of the DINO ViT for ANY token count (dense features at other resolutions than 224 / 96:
// dino-main/eval_video_segmentation.py runs 480 x 832 frames = 1561 tokens), and the rectangular patch gather that feeds it.
//   Attention.forward — dino-main/vision_transformer.py:80-92, inference only (no probabilities, no backward).
// attn_vit.hip keeps the whole K and V of a head in LDS, which stops at a few hundred tokens.  Here K and V arrive in tiles of 64
// keys (160-B LDS rows as in attn_vit.hip: conflict-free for the row fragments of K and the transposed fragments of V), double
// buffered: the global loads of tile t + 1 are issued before the products of tile t and written to the other buffer after them,
// one barrier per tile.  A wave owns 16 queries for the whole sweep; scores are computed transposed, S^T = K Q^T (key on the
// accumulator rows, query on the lane), so the running maximum / sum of a query are per-lane scalars (plus two shuffles over the
// four lane groups) and P^T is already the B operand of O^T += V^T P^T.  Online softmax: when a tile raises the maximum the
// accumulators and the running sum are rescaled by exp2((m_old - m_new) c).  No atomics: bit-reproducible, and a query's result
// does not depend on the workgroup size chosen by the launcher.
#include "attn_frag.hpp"
#include "../../include/sais_hip.h"

namespace {
constexpr int KT = 64;                    // keys per tile
constexpr int MAT_BYTES = KT * ROWB;

// grid (query tiles of 16 NW, heads, frames); NW waves of 16 queries each
template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_stream_kernel(const bf16* qkv, long ldq, int ntok, bf16* out, long ldo, float* lse,
                                                              float scale) {
    constexpr int NT = 64 * NW, RPP = NT / 8, NPASS = KT / RPP;      // RPP: tile rows staged per pass (8 threads per row)
    __shared__ __attribute__((aligned(16))) char smem[4 * MAT_BYTES];      // K0 | V0 | K1 | V1
    const int h = blockIdx.y, f = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const bf16* base = qkv + (size_t)f * ntok * ldq + h * HD;
    const int q = blockIdx.x * (16 * NW) + wid * 16 + li;             // tail rows: clamped loads, no stores
    bf16x8 fq[2];
    {
        const bf16* p = base + (size_t)(q < ntok ? q : ntok - 1) * ldq + 8 * g;
        fq[0] = *(const bf16x8*)p;
        fq[1] = *(const bf16x8*)(p + 32);
    }
    const int ntile = (ntok + KT - 1) / KT;
    const int sc = tid & 7, sr = tid >> 3;
    u32x4 vk[NPASS], vv[NPASS];
    auto gload = [&](int t) {                                         // clamped (not branched-on) row addresses
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            const int r = t * KT + sr + RPP * i, rc = r < ntok ? r : ntok - 1;
            vk[i] = *(const u32x4*)(base + DM + (size_t)rc * ldq + sc * 8);
            vv[i] = *(const u32x4*)(base + 2 * DM + (size_t)rc * ldq + sc * 8);
        }
    };
    auto lstore = [&](int t) {                                        // V rows past the end are zero: 0 x P = 0 whatever was there
        char* sK = smem + (t & 1) * 2 * MAT_BYTES;
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            const int rl = sr + RPP * i;
            const u32x4 z = {0, 0, 0, 0};
            *(u32x4*)(sK + rl * ROWB + sc * 16) = vk[i];
            *(u32x4*)(sK + MAT_BYTES + rl * ROWB + sc * 16) = t * KT + rl < ntok ? vv[i] : z;
        }
    };
    const float c = scale * LOG2E;
    float m = -INFINITY, lsum = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0, 0, 0, 0};
    gload(0);
    lstore(0);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < ntile; ++t) {
        const char* sK = smem + (t & 1) * 2 * MAT_BYTES;
        const char* sV = sK + MAT_BYTES;
        if (t + 1 < ntile) gload(t + 1);
        // S^T strip: s[u][r] = score(key 64 t + 16 u + 4 g + r, query li); keys past the end are -inf BEFORE the row maximum
        f32x4 s[4];
        float tmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            f32x4 a = {0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) a = mfma16(row_frag(sK, 16 * u + li, 4 * ks + g), fq[ks], a);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (t * KT + 16 * u + 4 * g + r >= ntok) a[r] = -INFINITY;
                tmax = fmaxf(tmax, a[r]);
            }
            s[u] = a;
        }
        tmax = group_max(tmax);                                       // every tile has at least one real key: finite
        const float mn = fmaxf(m, tmax);
        const float alpha = fast_exp2((m - mn) * c);                  // first tile: exp2(-inf) = 0
        const float mc = -mn * c;
        m = mn;
        float ts = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float e = fast_exp2(__builtin_fmaf(s[u][r], c, mc)); s[u][r] = e; ts += e; }
        lsum = __builtin_fmaf(lsum, alpha, ts);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 pf = pack_p(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] = mfma16(tr_frag(sV, ks, dt, g, li), pf, o[dt]);
        }
        if (t + 1 < ntile) lstore(t + 1);                             // the other buffer: its readers passed the last barrier
        __syncthreads();
    }
    const float sum = group_sum(lsum);
    const float inv = 1.0f / sum;
    if (q < ntok) {                                                   // lane: query q, d = 16 dt + 4 g + r
        bf16* orow = out + ((size_t)f * ntok + q) * ldo + h * HD + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            bf16x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (bf16)(o[dt][r] * inv);
            *(bf16x4*)(orow + 16 * dt) = v;
        }
        if (lse && g == 0) lse[((size_t)f * NH + h) * ntok + q] = m * scale + __logf(sum);
    }
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
        bf16x8 lo, hi;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const f32x4 a = *(const f32x4*)(src + 8 * k), b = *(const f32x4*)(src + 8 * k + 4);
            bf16x8& d = k ? hi : lo;
            d[0] = (bf16)a[0]; d[1] = (bf16)a[1]; d[2] = (bf16)a[2]; d[3] = (bf16)a[3];
            d[4] = (bf16)b[0]; d[5] = (bf16)b[1]; d[6] = (bf16)b[2]; d[7] = (bf16)b[3];
        }
        *(bf16x8*)dst = lo;
        *(bf16x8*)(dst + 8) = hi;
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
