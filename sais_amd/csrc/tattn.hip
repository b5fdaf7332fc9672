// Masked multi-head self-attention of the temporal TransformerEncoder (4 heads x 96, S = T + 1 <= 96 tokens per sequence):
// the nn.MultiheadAttention core inside the torch-1.8 post-norm TransformerEncoderLayer, with key_padding_mask, train-mode
// dropout on the attention weights and the README.md:43-48 head-averaged attention-map return
// (prepare_model.py:74-81,197-221).  Forward and backward, exact fp32 on the matrix cores.
//
// Round 2 computed every dot product with VALU FMAs out of LDS (two LDS reads per FMA: 16x below the VALU rate, 15 / 28 us
// per layer for 33 x 33 x 96 problems).  Here every product runs on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate:
// bit-for-bit an fmaf chain, at the fp32 VALU peak rate but with one LDS dword per 32 flop).  One 256-thread workgroup per
// (sequence, head); q, k, v (and dctx) of the head sit in LDS with 100-float rows.
//
// Operand trick: the 16x16x4 MFMA sums over 4 "k slots" (lane >> 4).  The summation order is free, so slot g of step s is
// mapped to feature d = 24 g + s: a lane then needs 24 CONTIGUOUS floats of its row (six ds_read_b128, conflict-free with the
// 100-float stride) for the whole 96-deep dot product instead of 24 scattered dwords.
// Orientation: scores are computed transposed, S^T[key][query] = K Q^T, so a lane owns one QUERY (column) and 4 keys per
// 16-key tile: softmax is an in-lane loop plus two shuffles, and P^T is already the B operand of ctx^T = V^T P^T (slot g of
// step r <-> key 4 g + r) with no lane movement.  The backward needs P and dS with the KEY on the lane as well (dV, dK sum
// over queries): the waves re-own key tiles after a barrier and rebuild both from the per-query statistics left in LDS.
// The arithmetic this file has in common with tattn_long.hip (score scale, dropout rule, masked score tile, 4-key accumulate,
// dK / dV step) is written once, in tattn_frag.hpp; here are the staging and the softmax of the resident form.
#include "tattn_frag.hpp"
#include "../../include/sais_hip.h"

namespace {
// head slices q, k, v of qkv [B*S, 1152] -> sQ / sK / sV [S_pad][TLD], rows >= S zero.  Addresses are clamped instead of
// branched on and a lane issues the loads of SU consecutive passes (3 SU float4) before the first LDS write: the
// `if (s < S) load` loop this replaces compiled to one dependent round trip per pass and matrix (~15 per launch for S = 33,
// each ~0.5 us of a 16-us kernel).
constexpr int SU = 3;
DEVINL void stage_qkv(const float* qkv, int b, int h, int S, int Spad, float* sQ, float* sK, float* sV, int tid) {
    const int total = Spad * (THD / 4);
    for (int i0 = tid; i0 < total; i0 += 256 * SU) {
        f32x4 v[SU][3];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const int i = min(i0 + 256 * u, total - 1), s = i / (THD / 4), c4 = i % (THD / 4);
            const float* src = qkv + ((size_t)b * S + min(s, S - 1)) * (3 * D) + h * THD + 4 * c4;
#pragma unroll
            for (int w = 0; w < 3; ++w) v[u][w] = *(const f32x4*)(src + w * D);
        }
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const int i = i0 + 256 * u;
            if (i < total) {
                const int s = i / (THD / 4), c4 = i % (THD / 4);
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                *(f32x4*)(sQ + s * TLD + 4 * c4) = s < S ? v[u][0] : z;
                *(f32x4*)(sK + s * TLD + 4 * c4) = s < S ? v[u][1] : z;
                *(f32x4*)(sV + s * TLD + 4 * c4) = s < S ? v[u][2] : z;
            }
        }
    }
}
// key flags of sequence b into LDS: 1 = masked (key_padding_mask) or past the sequence; read back per (key tile, lane)
// without the serialised global byte loads the `key >= S || pad[key]` form compiled to
DEVINL void stage_pad(const unsigned char* pad, int S, int Spad, unsigned char* sP, int tid) {
    if (tid < Spad) sP[tid] = tid >= S ? (unsigned char)1 : pad[tid];
}

constexpr int MAXT = 6;                                  // 16-token tiles: S <= 96

// Train mode (p > 0): the dropped weights go into P v and into the returned map (Drop, tattn_frag.hpp).
__global__ __launch_bounds__(256) void tattn_fwd_kernel(const float* qkv, const unsigned char* key_pad, int S, float* ctx,
                                                       float* attn_avg, float p_drop, const unsigned long long* rng,
                                                       unsigned sid) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nt = (S + 15) >> 4, Spad = nt * 16;
    float* sQ = (float*)smem;
    float* sK = sQ + Spad * TLD;
    float* sV = sK + Spad * TLD;
    unsigned char* sP = (unsigned char*)(sV + Spad * TLD);
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    stage_pad(key_pad + (size_t)b * S, S, Spad, sP, tid);
    stage_qkv(qkv, b, h, S, Spad, sQ, sK, sV, tid);
    __syncthreads();
    const Drop drop(p_drop, rng, sid, b, h, S);
    for (int qt = wid; qt < nt; qt += 4) {
        const int q = 16 * qt + li;                      // this lane's query (column of S^T)
        float qf[24];
        load24(sQ + q * TLD, g, qf, QSCALE);
        f32x4 p[MAXT];
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < MAXT; kt += 2) {           // two key tiles per pass: two independent accumulator chains
            if (kt >= nt) break;
            float kf[24], kg[24];
            load24(sK + (16 * kt + li) * TLD, g, kf);
            if (kt + 1 < nt) {
                load24(sK + (16 * (kt + 1) + li) * TLD, g, kg);
                dot_tile2(kf, qf, kg, qf, p[kt], p[kt + 1]);          // register r: key 16 kt + 4 g + r, query q
            } else {
                p[kt] = dot_tile(kf, qf);
            }
        }
#pragma unroll
        for (int kt = 0; kt < MAXT; ++kt) {
            if (kt >= nt) break;
            mask_tile(sP, 16 * kt, g, p[kt], m);
        }
        m = group_max(m);
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < MAXT; ++kt) {
            if (kt >= nt) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float e = __expf(p[kt][r] - m); p[kt][r] = e; sum += e; }
        }
        const float inv = 1.0f / group_sum(sum);
#pragma unroll
        for (int kt = 0; kt < MAXT; ++kt) {
            if (kt >= nt) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * kt + 4 * g + r;
                float v = p[kt][r] * inv;
                if (drop.on && q < S && key < S) v *= drop.keep(q, key);
                p[kt][r] = v;
                if (attn_avg && q < S && key < S) atomicAdd(attn_avg + ((size_t)b * S + q) * S + key, v * (1.0f / TH));
            }
        }
        // ctx^T[d][query] = sum_key v[key][d] P^T[key][query]: six independent accumulator chains (one per 16 features)
        Acc6 acc;
        zero6(acc);
#pragma unroll
        for (int kt = 0; kt < MAXT; ++kt) {
            if (kt >= nt) break;
            accumulate4(sV, 16 * kt, p[kt], g, li, acc);
        }
        if (q < S) store6(ctx + ((size_t)b * S + q) * D + h * THD, g, acc);
    }
}

// With dropout: ctx = P' v, P' = P m / (1 - p).  dV = P'^T dctx; dP = (dctx v^T) m / (1 - p); dS = P (dP - rowsum(P dP)) scale;
// dq = dS k; dk = dS^T q.  dctx = sum of nslab raw split-K slabs (slab_stride floats apart) of the out_proj dX GEMM.
__global__ __launch_bounds__(256) void tattn_bwd_kernel(const float* qkv, const unsigned char* key_pad, int S,
                                                       const float* dctx, int nslab, long slab_stride, float* dqkv,
                                                       float p_drop, const unsigned long long* rng, unsigned sid) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nt = (S + 15) >> 4, Spad = nt * 16;
    float* sQ = (float*)smem;
    float* sK = sQ + Spad * TLD;
    float* sV = sK + Spad * TLD;
    float* sG = sV + Spad * TLD;                          // dctx
    float* sM = sG + Spad * TLD;                          // per query: row max, 1 / row sum, rowsum(P dP)
    float* sI = sM + Spad;
    float* sDot = sI + Spad;
    unsigned char* sP = (unsigned char*)(sDot + Spad);
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    stage_pad(key_pad + (size_t)b * S, S, Spad, sP, tid);
    {   // dctx = sum of the out_proj dX slabs: the loads of SU passes x one slab in flight together
        const int total = Spad * (THD / 4);
        for (int i0 = tid; i0 < total; i0 += 256 * SU) {
            f32x4 v[SU];
            const float* src[SU];
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int i = min(i0 + 256 * u, total - 1), sr = i / (THD / 4), c4 = i % (THD / 4);
                src[u] = dctx + ((size_t)b * S + min(sr, S - 1)) * D + h * THD + 4 * c4;
                v[u] = *(const f32x4*)src[u];
            }
            for (int z = 1; z < nslab; ++z) {
#pragma unroll
                for (int u = 0; u < SU; ++u) v[u] += *(const f32x4*)(src[u] + (size_t)z * slab_stride);
            }
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int i = i0 + 256 * u;
                if (i < total) {
                    const int sr = i / (THD / 4), c4 = i % (THD / 4);
                    *(f32x4*)(sG + sr * TLD + 4 * c4) = sr < S ? v[u] : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
    }
    stage_qkv(qkv, b, h, S, Spad, sQ, sK, sV, tid);
    __syncthreads();
    const Drop drop(p_drop, rng, sid, b, h, S);

    // ---- phase 1: a wave owns 16 queries (on the lane), all keys: statistics, dS^T, dq
    for (int qt = wid; qt < nt; qt += 4) {
        const int q = 16 * qt + li;
        float qf[24], gf[24];
        load24(sQ + q * TLD, g, qf, QSCALE);
        load24(sG + q * TLD, g, gf);
        f32x4 p[MAXT], dp[MAXT];
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < MAXT; ++kt) {
            if (kt >= nt) break;
            score_dp_tile(sK, sV, sP, 16 * kt, qf, gf, g, li, p[kt], dp[kt], m);
        }
        m = group_max(m);
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < MAXT; ++kt) {
            if (kt >= nt) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float e = __expf(p[kt][r] - m); p[kt][r] = e; sum += e; }
        }
        const float inv = 1.0f / group_sum(sum);
        float dot = 0.f;
#pragma unroll
        for (int kt = 0; kt < MAXT; ++kt) {
            if (kt >= nt) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * kt + 4 * g + r;
                const float pv = p[kt][r] * inv;
                const float kp = (q < S && key < S) ? drop.keep(q, key) : 0.f;
                p[kt][r] = pv;
                dp[kt][r] *= kp;                         // dP = dP' m / (1 - p)
                dot += pv * dp[kt][r];
            }
        }
        dot = group_sum(dot);
        if (g == 0) { sM[q] = m; sI[q] = inv; sDot[q] = dot; }
#pragma unroll
        for (int kt = 0; kt < MAXT; ++kt) {
            if (kt >= nt) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) p[kt][r] = p[kt][r] * (dp[kt][r] - dot) * QSCALE;     // dS^T[key][query]
        }
        // dq^T[d][query] = sum_key k[key][d] dS^T[key][query]
        Acc6 acc;
        zero6(acc);
#pragma unroll
        for (int kt = 0; kt < MAXT; ++kt) {
            if (kt >= nt) break;
            accumulate4(sK, 16 * kt, p[kt], g, li, acc);
        }
        if (q < S) store6(dqkv + ((size_t)b * S + q) * (3 * D) + h * THD, g, acc);
    }
    __syncthreads();

    // ---- phase 2: a wave owns 16 keys (on the lane), all queries: P' and dS with the key on the lane -> dV, dK
    for (int kt = wid; kt < nt; kt += 4) {
        const int key = 16 * kt + li;
        const bool key_ok = !sP[key];
        float kf[24], vf[24];
        load24(sK + key * TLD, g, kf);
        load24(sV + key * TLD, g, vf);
        Acc6 adv, adk;
        zero6(adv);
        zero6(adk);
        for (int qt = 0; qt < nt; ++qt)
            dkv_step(sQ, sG, sM, sI, sDot, 16 * qt, 16 * qt, S, key, key_ok, kf, vf, drop, g, li, adv, adk);
        if (key < S) {
            float* o = dqkv + ((size_t)b * S + key) * (3 * D) + D + h * THD;
            store6(o, g, adk);
            store6(o + D, g, adv);
        }
    }
}

// zero-fill as a KERNEL node: the head-averaged map is accumulated with atomics over the four heads.  (Round 6: as a
// hipMemsetAsync node inside a captured graph the fill was right on the first replay and left garbage in the map on later ones —
// tools/scratch/win_dbg3.py, the opt-in hipGraph form of run_windows; a kernel node replays like every other launch.)
__global__ __launch_bounds__(256) void zero_f32_kernel(float* p, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) p[i] = 0.f;
}
}  // namespace

extern "C" int sais_temporal_attn_fwd(const float* qkv, const unsigned char* key_pad, int B, int S, float* ctx,
                                      float* attn_avg, float p_drop, const unsigned long long* rng_state,
                                      unsigned site, void* stream) {
    SAIS_ENTER();
    if (!qkv || !key_pad || !ctx || B <= 0 || S <= 0 || S > SAIS_TEMPORAL_MAX_S_FWD) return SAIS_ERR_ARG;
    if (p_drop < 0.f || p_drop >= 1.f || (p_drop > 0.f && !rng_state)) return SAIS_ERR_ARG;
    const int Spad = (S + 15) / 16 * 16;
    const int lds = 3 * Spad * TLD * 4 + Spad;
    if (sais_grow_dyn_lds<tattn_fwd_kernel>(lds)) return SAIS_ERR_LAUNCH;
    hipStream_t s = (hipStream_t)stream;
    if (attn_avg) {
        const long n = (long)B * S * S;
        hipLaunchKernelGGL(zero_f32_kernel, dim3((unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024)), dim3(256), 0, s, attn_avg, n);
    }
    hipLaunchKernelGGL(tattn_fwd_kernel, dim3(TH, B), dim3(256), lds, s, qkv, key_pad, S, ctx, attn_avg, p_drop, rng_state,
                       site);
    return sais_check_launch();
}

extern "C" int sais_temporal_attn_bwd(const float* qkv, const unsigned char* key_pad, int B, int S,
                                      const float* dctx, int nslab, long slab_stride, float* dqkv, float p_drop,
                                      const unsigned long long* rng_state, unsigned site, void* stream) {
    SAIS_ENTER();
    if (!qkv || !key_pad || !dctx || !dqkv || B <= 0 || S <= 0 || S > SAIS_TEMPORAL_MAX_S_BWD || nslab <= 0 || (slab_stride & 3))
        return SAIS_ERR_ARG;
    if (p_drop < 0.f || p_drop >= 1.f || (p_drop > 0.f && !rng_state)) return SAIS_ERR_ARG;
    const int Spad = (S + 15) / 16 * 16;
    const int lds = (4 * Spad * TLD + 3 * Spad) * 4 + Spad;
    if (sais_grow_dyn_lds<tattn_bwd_kernel>(lds)) return SAIS_ERR_LAUNCH;
    hipLaunchKernelGGL(tattn_bwd_kernel, dim3(TH, B), dim3(256), lds, (hipStream_t)stream, qkv, key_pad, S, dctx, nslab,
                       slab_stride, dqkv, p_drop, rng_state, site);
    return sais_check_launch();
}
