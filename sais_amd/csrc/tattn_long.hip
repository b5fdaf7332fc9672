// Masked multi-head self-attention of the temporal TransformerEncoder for sequences past the 96 tokens tattn.hip keeps resident:
// 1 <= S <= SAIS_TEMPORAL_LONG_MAX_S = 2001 (the 2000-row position table + CLS), forward and backward, the contract of tattn.hip.
//
// What the shape buys: keys and values STREAM through LDS in 64-row tiles (2 x 25.6 KB at the 100-float row of tattn.hip), a
// workgroup owns 64 queries (16 per wave, the query on the lane), so LDS use is 51 KB at any S where the resident form needs
// 3 (4) x S x 400 B and stops at 96.  The forward makes ONE pass with online rescaling when no map is wanted (layers 0-2) and two
// (row statistics, then normalised probabilities) when it is (last layer; there a workgroup owns 16 queries, loops over the
// four heads and its waves split the keys of a tile: see tattn_long_fwd_map_kernel).  The backward has one launch per output that owns
// it and no float atomics: per (b, h, query tile) the row statistics and dQ over all key tiles, per (b, h, key tile) dK and dV
// over all query tiles, P recomputed from the statistics of the first launch.  ctx, dqkv AND the map are bit-reproducible:
// the map's head sum has a fixed order (one workgroup loops over the four heads of its query tile and owns its map rows).
//
// Arithmetic: exact fp32 on v_mfma_f32_16x16x4_f32, scores transposed (key on the accumulator rows, query on the lane) as in
// tattn.hip; what the two files compute alike (score scale, dropout rule, masked score tile, 4-key accumulate, dK / dV step)
// is written once, in tattn_frag.hpp.  Online form, per 64-key tile: m' = max(m, tile max), alpha = exp(m - m'), l = l alpha +
// sum exp(s - m'), acc = acc alpha + (exp(s - m') keep) v; ctx = acc / ((1 - p) l).  Each lane keeps the partial l of its own
// 4 keys per 16; the four lane groups are added at the end (group_sum).  Map form: every wave runs that recurrence over its quarter
// of each key tile, then m = max_w m_w, l = sum_w l_w exp(m_w - m) in wave order; P = exp(s - m) (1 / l), P' = P keep /
// (1 - p), avg = ((P'_0 / 4 + P'_1 / 4) + P'_2 / 4) + P'_3 / 4, ctx = P' v.  Dropout mask element ((b 4 + h) S + i) S + j in
// 64 bits, the Philox state of tattn.hip: sais_dropout_mask regenerates what is applied here.
//
// Backward workspace (sais_temporal_attn_long_bwd_workspace_bytes): dctx summed over its slabs f32 [B S, 384], then per
// (b, h, query) the row max, 1 / row sum and rowsum(P dP) = three f32 [B, 4, S].  The entry point has no ctx argument, so
// rowsum(P dP) = sum_j P_j keep_j / (1 - p) (dctx . v_j) is accumulated online in the statistics pass next to l.
#include "tattn_frag.hpp"
#include "../../include/sais_hip.h"

namespace {
constexpr int LT = 64;                                   // rows of a staging tile = queries (keys) a workgroup owns

// rows row0 .. row0 + 63 of the 96-float slice at `src` (row stride ld floats, S rows) -> dst [64][TLD]; rows >= S zero.
// Addresses are clamped, the six loads of a lane are in flight before the first LDS write (stage_qkv of tattn.hip).
DEVINL void stage_tile(const float* src, int ld, int row0, int S, float* dst, int tid) {
    f32x4 v[6];
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        const int i = tid + 256 * u, r = i / (THD / 4), c4 = i % (THD / 4);
        v[u] = *(const f32x4*)(src + (size_t)min(row0 + r, S - 1) * ld + 4 * c4);
    }
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        const int i = tid + 256 * u, r = i / (THD / 4), c4 = i % (THD / 4);
        *(f32x4*)(dst + r * TLD + 4 * c4) = row0 + r < S ? v[u] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
// key flags of the tile: 1 = masked (key_padding_mask) or past the sequence
DEVINL void stage_flags(const unsigned char* pad, int row0, int S, unsigned char* sP, int tid) {
    if (tid < LT) sP[tid] = row0 + tid >= S ? (unsigned char)1 : pad[row0 + tid];
}

// scaled scores of the staged 64-key tile against the lane's query (s[j][r]: key 16 j + 4 g + r), -inf on flagged keys; returns
// the tile's max over the query's 64 keys
DEVINL float tile_scores(const float* sK, const unsigned char* sP, const float (&qf)[24], int g, int li, f32x4 (&s)[4]) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; j += 2) {
        float kf[24], kg[24];
        load24(sK + (16 * j + li) * TLD, g, kf);
        load24(sK + (16 * (j + 1) + li) * TLD, g, kg);
        dot_tile2(kf, qf, kg, qf, s[j], s[j + 1]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) mask_tile(sP, 16 * j, g, s[j], m);
    return group_max(m);
}
// the same with dP'[query][key] = dctx_q . v_key next to it
DEVINL float tile_scores_dp(const float* sK, const float* sV, const unsigned char* sP, const float (&qf)[24], const float (&gf)[24],
                            int g, int li, f32x4 (&s)[4], f32x4 (&dp)[4]) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) score_dp_tile(sK, sV, sP, 16 * j, qf, gf, g, li, s[j], dp[j], m);
    return group_max(m);
}
// acc^T[d][query] += sum_key x[key][d] w^T[key][query] over the staged tile (x = sV: ctx; x = sK: dq)
DEVINL void tile_accumulate(const float* sX, const f32x4 (&w)[4], int g, int li, Acc6& acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) accumulate4(sX, 16 * j, w[j], g, li, acc);
}

// grid (query tiles, 4 heads, B): one pass with online rescaling, no map
__global__ __launch_bounds__(256) void tattn_long_fwd_kernel(const float* qkv, const unsigned char* key_pad, int S, float* ctx,
                                                            float p_drop, const unsigned long long* rng, unsigned sid) {
    __shared__ __attribute__((aligned(16))) float sK[LT * TLD];
    __shared__ __attribute__((aligned(16))) float sV[LT * TLD];
    __shared__ unsigned char sP[LT];
    const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const int q = LT * blockIdx.x + 16 * wid + li, nkt = (S + LT - 1) / LT;
    const float* seq = qkv + (size_t)b * S * (3 * D);
    const unsigned char* pad = key_pad + (size_t)b * S;
    const Drop drop(p_drop, rng, sid, b, h, S);
    float qf[24];
    load24(seq + (size_t)min(q, S - 1) * (3 * D) + h * THD, g, qf, QSCALE);
    float m = -INFINITY, l = 0.f;
    Acc6 acc;
    zero6(acc);
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        stage_tile(seq + D + h * THD, 3 * D, LT * kt, S, sK, tid);
        stage_tile(seq + 2 * D + h * THD, 3 * D, LT * kt, S, sV, tid);
        stage_flags(pad, LT * kt, S, sP, tid);
        __syncthreads();
        f32x4 s[4];
        const float mn = fmaxf(m, tile_scores(sK, sP, qf, g, li, s));      // move the running max, rescale what is accumulated
        const float alpha = __expf(m - mn);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < THD / 16; ++dt) acc[dt] *= alpha;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = LT * kt + 16 * j + 4 * g + r;
                float v = __expf(s[j][r] - m);
                l += v;
                if (drop.on && q < S && key < S && drop.keep(q, key) == 0.f) v = 0.f;
                s[j][r] = v;
            }
        tile_accumulate(sV, s, g, li, acc);
    }
    const float fin = drop.inv_keep / group_sum(l);
#pragma unroll
    for (int dt = 0; dt < THD / 16; ++dt) acc[dt] *= fin;
    if (q < S) store6(ctx + ((size_t)b * S + q) * D + h * THD, g, acc);
}

// The map form.  grid (16-query tiles, 1, B): the workgroup owns 16 queries and their rows of attn_avg and loops over the four
// heads (fixed-order head sum); its four waves split the KEYS of every staged tile (wave w: keys 16 w .. 16 w + 15), so a
// tile costs each wave one 16 x 16 score tile and the grid is four times as wide as with 64 queries per workgroup.  Pass 1:
// each wave runs the online recurrence over its key quarters; the four (max, sum) pairs meet in LDS and are combined in wave
// order: M = max m_w, L = sum_w l_w exp(m_w - M).  Pass 2: P = exp(s - M) / L, the map, and each wave's partial P' v, summed in
// wave order through the (by then free) K tile.  A wave whose keys so far are all masked has m = -inf: its factors are
// taken as exp(0) / exp(-inf) explicitly, never -inf - -inf.
__global__ __launch_bounds__(256) void tattn_long_fwd_map_kernel(const float* qkv, const unsigned char* key_pad, int S,
                                                                float* ctx, float* attn_avg, float p_drop,
                                                                const unsigned long long* rng, unsigned sid) {
    __shared__ __attribute__((aligned(16))) float sK[LT * TLD];
    __shared__ __attribute__((aligned(16))) float sV[LT * TLD];
    __shared__ float sM[4][16], sL[4][16];
    __shared__ unsigned char sP[LT];
    static_assert(LT * TLD >= 4 * 16 * THD, "the K tile holds the four partial ctx tiles");
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const int q0 = 16 * blockIdx.x, q = q0 + li, nkt = (S + LT - 1) / LT;
    const float* seq = qkv + (size_t)b * S * (3 * D);
    const unsigned char* pad = key_pad + (size_t)b * S;
    for (int h = 0; h < TH; ++h) {
        const Drop drop(p_drop, rng, sid, b, h, S);
        float qf[24];
        load24(seq + (size_t)min(q, S - 1) * (3 * D) + h * THD, g, qf, QSCALE);
        // ---- pass 1
        float m = -INFINITY, l = 0.f;
        for (int kt = 0; kt < nkt; ++kt) {
            __syncthreads();
            stage_tile(seq + D + h * THD, 3 * D, LT * kt, S, sK, tid);
            stage_flags(pad, LT * kt, S, sP, tid);
            __syncthreads();
            float kf[24];
            load24(sK + (16 * wid + li) * TLD, g, kf);
            f32x4 s = dot_tile(kf, qf);                   // register r: key 16 wid + 4 g + r of the tile, query q
            float mt = -INFINITY;                         // own copy of mask_tile (tattn_frag.hpp): keep the two in step
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (sP[16 * wid + 4 * g + r]) s[r] = -INFINITY;
                mt = fmaxf(mt, s[r]);
            }
            const float mn = fmaxf(m, group_max(mt));
            if (mn != -INFINITY) {
                l *= __expf(m - mn);                      // m = -inf: l is 0 and the factor exp(-inf) = 0
                m = mn;
#pragma unroll
                for (int r = 0; r < 4; ++r) l += __expf(s[r] - m);
            }
        }
        l = group_sum(l);
        if (g == 0) { sM[wid][li] = m; sL[wid][li] = l; }
        __syncthreads();
        float M = fmaxf(fmaxf(sM[0][li], sM[1][li]), fmaxf(sM[2][li], sM[3][li])), L = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) L += sL[w][li] * __expf(sM[w][li] - M);          // a wave without a key: 0 exp(-inf) = 0
        const float inv = 1.0f / L;
        // ---- pass 2
        Acc6 acc;
        zero6(acc);
        for (int kt = 0; kt < nkt; ++kt) {
            __syncthreads();
            stage_tile(seq + D + h * THD, 3 * D, LT * kt, S, sK, tid);
            stage_tile(seq + 2 * D + h * THD, 3 * D, LT * kt, S, sV, tid);
            stage_flags(pad, LT * kt, S, sP, tid);
            __syncthreads();
            float kf[24];
            load24(sK + (16 * wid + li) * TLD, g, kf);
            f32x4 s = dot_tile(kf, qf);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = LT * kt + 16 * wid + 4 * g + r;
                float v = sP[16 * wid + 4 * g + r] ? 0.f : __expf(s[r] - M) * inv;
                if (drop.on && q < S && key < S) v *= drop.keep(q, key);
                s[r] = v;
                if (q < S && key < S) {
                    float* a = attn_avg + ((size_t)b * S + q) * S + key;
                    *a = h == 0 ? v * (1.0f / TH) : *a + v * (1.0f / TH);
                }
                const float* row = sV + (16 * wid + 4 * g + r) * TLD + li;         // own copy of a step of accumulate4
#pragma unroll
                for (int dt = 0; dt < THD / 16; ++dt) acc[dt] = mfma4(row[16 * dt], v, acc[dt]);
            }
        }
        __syncthreads();                                  // every wave is done with the K tile: it takes the partial ctx tiles
#pragma unroll
        for (int dt = 0; dt < THD / 16; ++dt) *(f32x4*)(sK + (wid * 16 + li) * THD + 16 * dt + 4 * g) = acc[dt];
        __syncthreads();
        for (int i = tid; i < 16 * THD; i += 256) {       // ((w0 + w1) + w2) + w3, whole rows of ctx
            const int qq = i / THD, d = i % THD;
            const float v = ((sK[i] + sK[16 * THD + i]) + sK[2 * 16 * THD + i]) + sK[3 * 16 * THD + i];
            if (q0 + qq < S) ctx[((size_t)b * S + q0 + qq) * D + h * THD + d] = v;
        }
    }
}

// grid (query tiles, 4 heads, B): the slab sum of dctx and the row statistics into the workspace, then dq.
// dS = P (dP - rowsum(P dP)) scale with dP = (dctx v^T) keep / (1 - p);  dq = dS k.
__global__ __launch_bounds__(256) void tattn_long_bwd_dq_kernel(const float* qkv, const unsigned char* key_pad, int S,
                                                               const float* dctx, int nslab, long slab_stride, float* dqkv,
                                                               float p_drop, const unsigned long long* rng, unsigned sid,
                                                               float* wsG, float* wsM, float* wsI, float* wsDot) {
    __shared__ __attribute__((aligned(16))) float sK[LT * TLD];
    __shared__ __attribute__((aligned(16))) float sV[LT * TLD];
    __shared__ unsigned char sP[LT];
    const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const int q = LT * blockIdx.x + 16 * wid + li, qc = min(q, S - 1), nkt = (S + LT - 1) / LT;
    const float* seq = qkv + (size_t)b * S * (3 * D);
    const unsigned char* pad = key_pad + (size_t)b * S;
    const Drop drop(p_drop, rng, sid, b, h, S);
    float qf[24], gf[24];
    load24(seq + (size_t)qc * (3 * D) + h * THD, g, qf, QSCALE);
    const float* grow = dctx + ((size_t)b * S + qc) * D + h * THD;
    load24(grow, g, gf);
    for (int z = 1; z < nslab; ++z) {                     // dctx = slab 0 + slab 1 + ... in turn, as tattn.hip sums them
        float t[24];
        load24(grow + (size_t)z * slab_stride, g, t);
#pragma unroll
        for (int i = 0; i < 24; ++i) gf[i] += t[i];
    }
    if (q < S) {
#pragma unroll
        for (int i = 0; i < 6; ++i)
            *(f32x4*)(wsG + ((size_t)b * S + q) * D + h * THD + 24 * g + 4 * i) = f32x4{gf[4 * i], gf[4 * i + 1], gf[4 * i + 2], gf[4 * i + 3]};
    }
    // ---- pass 1: row max, row sum and sum_j exp(s_j - m) dP_j, online
    float m = -INFINITY, l = 0.f, dsum = 0.f;
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        stage_tile(seq + D + h * THD, 3 * D, LT * kt, S, sK, tid);
        stage_tile(seq + 2 * D + h * THD, 3 * D, LT * kt, S, sV, tid);
        stage_flags(pad, LT * kt, S, sP, tid);
        __syncthreads();
        f32x4 s[4], dp[4];
        const float mn = fmaxf(m, tile_scores_dp(sK, sV, sP, qf, gf, g, li, s, dp));
        const float alpha = __expf(m - mn);
        m = mn;
        l *= alpha;
        dsum *= alpha;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = LT * kt + 16 * j + 4 * g + r;
                const float e = __expf(s[j][r] - m);
                l += e;
                if (q < S && key < S) dsum += e * (dp[j][r] * drop.keep(q, key));
            }
    }
    const float inv = 1.0f / group_sum(l);
    const float dot = group_sum(dsum) * inv;
    if (g == 0 && q < S) {
        const size_t o = ((size_t)b * TH + h) * S + q;
        wsM[o] = m; wsI[o] = inv; wsDot[o] = dot;
    }
    // ---- pass 2: dS^T on the registers, dq^T[d][query] = sum_key k[key][d] dS^T[key][query]
    Acc6 acc;
    zero6(acc);
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        stage_tile(seq + D + h * THD, 3 * D, LT * kt, S, sK, tid);
        stage_tile(seq + 2 * D + h * THD, 3 * D, LT * kt, S, sV, tid);
        stage_flags(pad, LT * kt, S, sP, tid);
        __syncthreads();
        f32x4 s[4], dp[4];
        tile_scores_dp(sK, sV, sP, qf, gf, g, li, s, dp);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = LT * kt + 16 * j + 4 * g + r;
                const float pv = __expf(s[j][r] - m) * inv;
                const float kp = (q < S && key < S) ? drop.keep(q, key) : 0.f;
                s[j][r] = pv * (dp[j][r] * kp - dot) * QSCALE;
            }
        tile_accumulate(sK, s, g, li, acc);
    }
    if (q < S) store6(dqkv + ((size_t)b * S + q) * (3 * D) + h * THD, g, acc);
}

// grid (key tiles, 4 heads, B): a wave owns 16 keys (on the lane) and loops over the query tiles; P' and dS rebuilt from the
// statistics of the launch above.  dV = P'^T dctx;  dK = dS^T q.
__global__ __launch_bounds__(256) void tattn_long_bwd_dkv_kernel(const float* qkv, const unsigned char* key_pad, int S,
                                                                float* dqkv, float p_drop, const unsigned long long* rng,
                                                                unsigned sid, const float* wsG, const float* wsM,
                                                                const float* wsI, const float* wsDot) {
    __shared__ __attribute__((aligned(16))) float sQ[LT * TLD];
    __shared__ __attribute__((aligned(16))) float sG[LT * TLD];
    __shared__ __attribute__((aligned(16))) float sM[LT];
    __shared__ __attribute__((aligned(16))) float sI[LT];
    __shared__ __attribute__((aligned(16))) float sDot[LT];
    const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const int key = LT * blockIdx.x + 16 * wid + li, kc = min(key, S - 1), nqt = (S + LT - 1) / LT;
    const float* seq = qkv + (size_t)b * S * (3 * D);
    const Drop drop(p_drop, rng, sid, b, h, S);
    const bool key_ok = key < S && !key_pad[(size_t)b * S + kc];
    float kf[24], vf[24];
    load24(seq + (size_t)kc * (3 * D) + D + h * THD, g, kf);
    load24(seq + (size_t)kc * (3 * D) + 2 * D + h * THD, g, vf);
    Acc6 adv, adk;
    zero6(adv);
    zero6(adk);
    for (int qt = 0; qt < nqt; ++qt) {
        __syncthreads();
        stage_tile(seq + h * THD, 3 * D, LT * qt, S, sQ, tid);
        stage_tile(wsG + (size_t)b * S * D + h * THD, D, LT * qt, S, sG, tid);
        if (tid < LT) {
            const size_t o = ((size_t)b * TH + h) * S + min(LT * qt + tid, S - 1);
            sM[tid] = wsM[o]; sI[tid] = wsI[o]; sDot[tid] = wsDot[o];
        }
        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < 4; ++j)
            dkv_step(sQ, sG, sM, sI, sDot, 16 * j, LT * qt + 16 * j, S, key, key_ok, kf, vf, drop, g, li, adv, adk);
    }
    if (key < S) {
        float* o = dqkv + ((size_t)b * S + key) * (3 * D) + D + h * THD;
        store6(o, g, adk);
        store6(o + D, g, adv);
    }
}

bool bad_common(int B, int S, float p_drop, const unsigned long long* rng_state) {
    if (B <= 0 || B > 65535 || S <= 0 || S > SAIS_TEMPORAL_LONG_MAX_S) return true;
    return !(p_drop >= 0.f && p_drop < 1.f) || (p_drop > 0.f && !rng_state);
}
}  // namespace

extern "C" size_t sais_temporal_attn_long_bwd_workspace_bytes(int B, int S) {
    if (B <= 0 || S <= 0 || S > SAIS_TEMPORAL_LONG_MAX_S) return 0;
    return ((size_t)B * S * D + 3 * (size_t)B * TH * S) * sizeof(float);
}

extern "C" int sais_temporal_attn_fwd_long(const float* qkv, const unsigned char* key_pad, int B, int S, float* ctx,
                                           float* attn_avg, float p_drop, const unsigned long long* rng_state, unsigned site,
                                           void* stream) {
    SAIS_ENTER();
    if (!qkv || !key_pad || !ctx || bad_common(B, S, p_drop, rng_state)) return SAIS_ERR_ARG;
    const unsigned nqt = (unsigned)((S + LT - 1) / LT);
    hipStream_t s = (hipStream_t)stream;
    if (attn_avg)
        hipLaunchKernelGGL(tattn_long_fwd_map_kernel, dim3((unsigned)((S + 15) / 16), 1, B), dim3(256), 0, s, qkv, key_pad, S, ctx,
                           attn_avg, p_drop, rng_state, site);
    else
        hipLaunchKernelGGL(tattn_long_fwd_kernel, dim3(nqt, TH, B), dim3(256), 0, s, qkv, key_pad, S, ctx, p_drop, rng_state, site);
    return sais_check_launch();
}

extern "C" int sais_temporal_attn_bwd_long(const float* qkv, const unsigned char* key_pad, int B, int S, const float* dctx,
                                           int nslab, long slab_stride, float* dqkv, float p_drop,
                                           const unsigned long long* rng_state, unsigned site, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    SAIS_ENTER();
    if (!qkv || !key_pad || !dctx || !dqkv || bad_common(B, S, p_drop, rng_state) || nslab <= 0 || (slab_stride & 3))
        return SAIS_ERR_ARG;
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < sais_temporal_attn_long_bwd_workspace_bytes(B, S))
        return SAIS_ERR_ARG;
    float* wsG = (float*)workspace;
    float* wsM = wsG + (size_t)B * S * D;
    float* wsI = wsM + (size_t)B * TH * S;
    float* wsDot = wsI + (size_t)B * TH * S;
    const dim3 grid((unsigned)((S + LT - 1) / LT), TH, B);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tattn_long_bwd_dq_kernel, grid, dim3(256), 0, s, qkv, key_pad, S, dctx, nslab, slab_stride, dqkv, p_drop,
                       rng_state, site, wsG, wsM, wsI, wsDot);
    hipLaunchKernelGGL(tattn_long_bwd_dkv_kernel, grid, dim3(256), 0, s, qkv, key_pad, S, dqkv, p_drop, rng_state, site, wsG, wsM,
                       wsI, wsDot);
    return sais_check_launch();
}
