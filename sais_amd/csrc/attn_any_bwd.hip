// Streaming self-attention backward of the DINO ViT for ANY token count: the backward of attn_any.hip's forward, so the patch-16
// backbone can be trained at frame sizes other than 224 x 224 / 96 x 96.
//   Attention.forward — dino-main/vision_transformer.py:80-92; the arithmetic is that of attn_vit.hip's resident backward:
//   P = exp2(s c - lse log2e) in f32 from the saved log-sum-exp, delta = rowsum(dO * the saved bf16 out) in f32,
//   dS = P (dP - delta) in f32 rounded once to bf16 for the dQ and the dK product, P rounded once to bf16 for dV,
//   dQ = dS K scale, dK = dS^T Q scale, dV = P^T dO accumulated in f32 on the bf16 MFMA and rounded once on store.
// Two launches, each the only writer of what it stores (the shape of tattn_long.hip): no float atomics, no cross-workgroup sums,
// bit-reproducible, and a row's result does not depend on the workgroup size the launcher picks.
//   launch 1, per (frame, head, tile of 16 NW queries): a wave owns 16 queries (query on the lane: Q / dO row fragments, lse and
//     delta are per-lane values), computes delta for them, stores it to the workspace (f32 [frames, 6, ntok]) and sweeps the keys:
//     K and V arrive in tiles of 64 rows, double buffered in LDS exactly as in attn_stream_kernel (160-B rows, the global loads of
//     tile t + 1 issued before the products of tile t, one barrier per tile).  S^T = K Q^T and dP^T = V dO^T put dS^T in
//     registers as the B operand of dQ^T += K^T dS^T.  Keys past ntok: score -inf before the exponential (P = 0), V rows zero.
//   launch 2, per (frame, head, tile of 16 NW keys): a wave owns 16 keys (key on the lane: its K / V row fragments stay in
//     registers) and sweeps the queries: Q, dO, lse log2e and delta arrive in tiles of 64 rows, double buffered the same way.
//     S = Q K^T and dP = dO V^T put P and dS in registers as the B operands of dV^T += dO^T P and dK^T += Q^T dS.  Query rows
//     past ntok: lse = +inf (P = 0), delta = 0, Q and dO rows zero — they contribute nothing and are not stored.
// S, dP and the exponential are computed TWICE, once per launch: 7 tile products per (query, key) pair instead of the 5 of the
// single-pass resident kernel.  That is the price of owning every output; the resident kernel pays a workgroup barrier per 32
// queries and a dS image in LDS instead, which needs the whole head in LDS.  Rows outside the tensor are reached by clamped loads
// only and never stored.
#include "attn_stream_bwd.hpp"
#include "../../include/sais_hip.h"

namespace {
// The two tile bodies (attn_stream_dq_tile, attn_stream_dkv_tile) live in attn_stream_bwd.hpp, shared with the segmented
// backward of attn_seg.hip; the kernels here place a workgroup at its (frame, head, tile).
// launch 1: grid (query tiles of 16 NW, heads, frames); NW waves of 16 queries each
template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_stream_dq_kernel(const bf16* qkv, long ldq, const bf16* dout, long ldo,
                                                                 const bf16* out, long ldout, const float* lse, int ntok,
                                                                 float* delta, bf16* dqkv, long lddq, float scale) {
    const int h = blockIdx.y, f = blockIdx.z;
    const size_t row0 = (size_t)f * ntok, stat = ((size_t)f * NH + h) * ntok;
    attn_stream_dq_tile<NW>(qkv + row0 * ldq + h * HD, ldq, dout + row0 * ldo + h * HD, ldo, out + row0 * ldout + h * HD, ldout,
                            lse + stat, ntok, blockIdx.x * (16 * NW), delta + stat, dqkv + row0 * lddq + h * HD, lddq, scale);
}

// launch 2: grid (key tiles of 16 NW, heads, frames); NW waves of 16 keys each
template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_stream_dkv_kernel(const bf16* qkv, long ldq, const bf16* dout, long ldo,
                                                                  const float* lse, const float* delta, int ntok, bf16* dqkv,
                                                                  long lddq, float scale) {
    const int h = blockIdx.y, f = blockIdx.z;
    const size_t row0 = (size_t)f * ntok, stat = ((size_t)f * NH + h) * ntok;
    attn_stream_dkv_tile<NW>(qkv + row0 * ldq + h * HD, ldq, dout + row0 * ldo + h * HD, ldo, lse + stat, delta + stat, ntok,
                             blockIdx.x * (16 * NW), dqkv + row0 * lddq + h * HD, lddq, scale);
}

template <int NW>
void launch_pair(const void* qkv, long ldqkv, const void* dout, long lddo, const void* out, long ldout, const float* lse, int frames,
                 int ntok, void* dqkv, long lddqkv, float* delta, hipStream_t stream) {
    const dim3 grid((ntok + 16 * NW - 1) / (16 * NW), NH, frames), block(64 * NW);
    hipLaunchKernelGGL(attn_stream_dq_kernel<NW>, grid, block, 0, stream, (const bf16*)qkv, ldqkv, (const bf16*)dout, lddo,
                       (const bf16*)out, ldout, lse, ntok, delta, (bf16*)dqkv, lddqkv, 0.125f);
    hipLaunchKernelGGL(attn_stream_dkv_kernel<NW>, grid, block, 0, stream, (const bf16*)qkv, ldqkv, (const bf16*)dout, lddo, lse,
                       (const float*)delta, ntok, (bf16*)dqkv, lddqkv, 0.125f);
}
}  // namespace

extern "C" size_t sais_vit_attn_bwd_any_workspace_bytes(int frames, int ntok) {
    if (frames <= 0 || ntok <= 0) return 0;
    return (size_t)frames * NH * (size_t)ntok * sizeof(float);        // delta f32 [frames, 6, ntok]
}

extern "C" int sais_vit_attn_bwd_any(const void* qkv, long ldqkv, const void* dout, long lddo, const void* out, long ldout,
                                     const float* lse, int frames, int ntok, void* dqkv, long lddqkv, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    SAIS_ENTER();
    if (!qkv || !dout || !out || !lse || !dqkv || !workspace || frames <= 0 || frames > 65535) return SAIS_ERR_ARG;
    if (ntok < 2 || ntok > SAIS_VIT_ATTN_ANY_MAX_TOKENS) return SAIS_ERR_ARG;
    if ((ldqkv & 7) || (lddo & 7) || (ldout & 7) || (lddqkv & 7) || ldqkv < 3 * DM || lddo < DM || ldout < DM || lddqkv < 3 * DM)
        return SAIS_ERR_ARG;
    if (workspace_bytes < sais_vit_attn_bwd_any_workspace_bytes(frames, ntok)) return SAIS_ERR_ARG;
    // The forward's rule (attn_any.hip): 64-row workgroups (4 waves) unless they would leave the chip short of two workgroups
    // per CU, then 32-row ones.  Both launches take the same form; a row's result is the same in either.
    const long wg64 = (long)frames * NH * ((ntok + 63) / 64);
    if (wg64 >= 512)
        launch_pair<4>(qkv, ldqkv, dout, lddo, out, ldout, lse, frames, ntok, dqkv, lddqkv, (float*)workspace, (hipStream_t)stream);
    else
        launch_pair<2>(qkv, ldqkv, dout, lddo, out, ldout, lse, frames, ntok, dqkv, lddqkv, (float*)workspace, (hipStream_t)stream);
    return sais_check_launch();
}
