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
#include "attn_frag.hpp"
#include "../../include/sais_hip.h"

namespace {
constexpr int KT = 64;                    // rows per streamed tile (keys in launch 1, queries in launch 2)
constexpr int MAT_BYTES = KT * ROWB;

DEVINL void load_row_frags(const bf16* base, long ld, int row, int ntok, int g, bf16x8 (&f)[2]) {
    const bf16* p = base + (size_t)(row < ntok ? row : ntok - 1) * ld + 8 * g;
    f[0] = *(const bf16x8*)p;
    f[1] = *(const bf16x8*)(p + 32);
}

// ------------------------------------------------------------------------------------------ launch 1: delta and dQ
// grid (query tiles of 16 NW, heads, frames); NW waves of 16 queries each
template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_stream_dq_kernel(const bf16* qkv, long ldq, const bf16* dout, long ldo,
                                                                 const bf16* out, long ldout, const float* lse, int ntok,
                                                                 float* delta, bf16* dqkv, long lddq, float scale) {
    constexpr int NT = 64 * NW, RPP = NT / 8, NPASS = KT / RPP;      // RPP: tile rows staged per pass (8 threads per row)
    __shared__ __attribute__((aligned(16))) char smem[4 * MAT_BYTES];      // K0 | V0 | K1 | V1
    const int h = blockIdx.y, f = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const bf16* base = qkv + (size_t)f * ntok * ldq + h * HD;
    const int q = blockIdx.x * (16 * NW) + wid * 16 + li;             // tail rows: clamped loads, no stores
    const int qc = q < ntok ? q : ntok - 1;
    const size_t stat = ((size_t)f * NH + h) * ntok;
    bf16x8 fq[2], fdo[2];
    float dlt = 0.f;
    {
        bf16x8 fo[2];
        load_row_frags(base, ldq, q, ntok, g, fq);
        load_row_frags(dout + (size_t)f * ntok * ldo + h * HD, ldo, q, ntok, g, fdo);
        load_row_frags(out + (size_t)f * ntok * ldout + h * HD, ldout, q, ntok, g, fo);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) dlt = __builtin_fmaf((float)fdo[ks][e], (float)fo[ks][e], dlt);
        dlt = group_sum(dlt);
    }
    const float lq = lse[stat + qc] * LOG2E;
    if (q < ntok && g == 0) delta[stat + q] = dlt;
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
    auto lstore = [&](int t) {                                        // V rows past the end are zero; K rows are copies of the last
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
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0, 0, 0, 0};
    gload(0);
    lstore(0);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < ntile; ++t) {
        const char* sK = smem + (t & 1) * 2 * MAT_BYTES;
        const char* sV = sK + MAT_BYTES;
        if (t + 1 < ntile) gload(t + 1);
        // dS^T strip: ds[u][r] for key 64 t + 16 u + 4 g + r, query li; keys past the end are -inf BEFORE the exponential
        f32x4 ds[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            f32x4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                a = mfma16(row_frag(sK, 16 * u + li, 4 * ks + g), fq[ks], a);       // S^T[key][q]
                b = mfma16(row_frag(sV, 16 * u + li, 4 * ks + g), fdo[ks], b);      // dP^T[key][q]
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (t * KT + 16 * u + 4 * g + r >= ntok) a[r] = -INFINITY;
                const float pv = fast_exp2(__builtin_fmaf(a[r], c, -lq));
                ds[u][r] = pv * (b[r] - dlt);                                       // x scale at the store
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 dsf = pack_p(ds[2 * ks], ds[2 * ks + 1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) dq[dt] = mfma16(tr_frag(sK, ks, dt, g, li), dsf, dq[dt]);   // dQ^T[d][q]
        }
        if (t + 1 < ntile) lstore(t + 1);                             // the other buffer: its readers passed the last barrier
        __syncthreads();
    }
    if (q < ntok) {                                                   // lane: query q, d = 16 dt + 4 g + r
        bf16* qrow = dqkv + ((size_t)f * ntok + q) * lddq + h * HD + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            bf16x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (bf16)(dq[dt][r] * scale);
            *(bf16x4*)(qrow + 16 * dt) = v;
        }
    }
}

// ------------------------------------------------------------------------------------------ launch 2: dK and dV
// grid (key tiles of 16 NW, heads, frames); NW waves of 16 keys each
constexpr int QBUF_BYTES = 2 * MAT_BYTES + 2 * KT * 4;               // Q | dO | lse log2e [64] | delta [64]
template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_stream_dkv_kernel(const bf16* qkv, long ldq, const bf16* dout, long ldo,
                                                                  const float* lse, const float* delta, int ntok, bf16* dqkv,
                                                                  long lddq, float scale) {
    constexpr int NT = 64 * NW, RPP = NT / 8, NPASS = KT / RPP;
    __shared__ __attribute__((aligned(16))) char smem[2 * QBUF_BYTES];
    const int h = blockIdx.y, f = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const bf16* base = qkv + (size_t)f * ntok * ldq + h * HD;
    const bf16* dob = dout + (size_t)f * ntok * ldo + h * HD;
    const size_t stat = ((size_t)f * NH + h) * ntok;
    const int key = blockIdx.x * (16 * NW) + wid * 16 + li;           // tail rows: clamped loads, no stores
    bf16x8 fk[2], fv[2];
    load_row_frags(base + DM, ldq, key, ntok, g, fk);
    load_row_frags(base + 2 * DM, ldq, key, ntok, g, fv);
    const int ntile = (ntok + KT - 1) / KT;
    const int sc = tid & 7, sr = tid >> 3;
    u32x4 vq[NPASS], vd[NPASS];
    float vl, vdl;                                                    // statistics of tile row (tid & 63); threads < 64 store them
    auto gload = [&](int t) {
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            const int r = t * KT + sr + RPP * i, rc = r < ntok ? r : ntok - 1;
            vq[i] = *(const u32x4*)(base + (size_t)rc * ldq + sc * 8);
            vd[i] = *(const u32x4*)(dob + (size_t)rc * ldo + sc * 8);
        }
        const int r = t * KT + lane, rc = r < ntok ? r : ntok - 1;
        vl = lse[stat + rc];
        vdl = delta[stat + rc];
    };
    auto lstore = [&](int t) {                                        // query rows past the end: zero rows, lse = +inf, delta = 0
        char* sQ = smem + (t & 1) * QBUF_BYTES;
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            const int rl = sr + RPP * i;
            const bool ok = t * KT + rl < ntok;
            const u32x4 z = {0, 0, 0, 0};
            *(u32x4*)(sQ + rl * ROWB + sc * 16) = ok ? vq[i] : z;
            *(u32x4*)(sQ + MAT_BYTES + rl * ROWB + sc * 16) = ok ? vd[i] : z;
        }
        if (tid < KT) {
            const bool ok = t * KT + tid < ntok;
            float* sL = (float*)(sQ + 2 * MAT_BYTES);
            sL[tid] = ok ? vl * LOG2E : INFINITY;                     // exp2(-inf) = 0: pad queries
            sL[KT + tid] = ok ? vdl : 0.f;
        }
    };
    const float c = scale * LOG2E;
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dk[dt] = f32x4{0, 0, 0, 0}; dv[dt] = f32x4{0, 0, 0, 0}; }
    gload(0);
    lstore(0);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < ntile; ++t) {
        const char* sQ = smem + (t & 1) * QBUF_BYTES;
        const char* sO = sQ + MAT_BYTES;
        const float* sL = (const float*)(sQ + 2 * MAT_BYTES);
        const float* sD = sL + KT;
        if (t + 1 < ntile) gload(t + 1);
        f32x4 p[4], ds[4];                                            // lane holds query 64 t + 16 u + 4 g + r, key li
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            f32x4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                a = mfma16(row_frag(sQ, 16 * u + li, 4 * ks + g), fk[ks], a);       // S[q][key]
                b = mfma16(row_frag(sO, 16 * u + li, 4 * ks + g), fv[ks], b);       // dP[q][key]
            }
            const f32x4 l4 = *(const f32x4*)(sL + 16 * u + 4 * g);
            const f32x4 d4 = *(const f32x4*)(sD + 16 * u + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = fast_exp2(__builtin_fmaf(a[r], c, -l4[r]));
                p[u][r] = pv;
                ds[u][r] = pv * (b[r] - d4[r]);                                     // x scale at the dK store
            }
        }
#pragma unroll
        for (int qs = 0; qs < 2; ++qs) {
            const bf16x8 pf = pack_p(p[2 * qs], p[2 * qs + 1]), dsf = pack_p(ds[2 * qs], ds[2 * qs + 1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                dv[dt] = mfma16(tr_frag(sO, qs, dt, g, li), pf, dv[dt]);            // dV^T[d][key]
                dk[dt] = mfma16(tr_frag(sQ, qs, dt, g, li), dsf, dk[dt]);           // dK^T[d][key]
            }
        }
        if (t + 1 < ntile) lstore(t + 1);
        __syncthreads();
    }
    if (key < ntok) {                                                 // lane: key, d = 16 dt + 4 g + r
        bf16* krow = dqkv + ((size_t)f * ntok + key) * lddq + DM + h * HD + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            bf16x4 a, b;
#pragma unroll
            for (int r = 0; r < 4; ++r) { a[r] = (bf16)(dk[dt][r] * scale); b[r] = (bf16)dv[dt][r]; }
            *(bf16x4*)(krow + 16 * dt) = a;
            *(bf16x4*)(krow + DM + 16 * dt) = b;
        }
    }
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
