// The tile body of the streaming self-attention forward, one copy for attn_any.hip (one token count for every frame of the
// launch) and attn_seg.hip (segments of different token counts in one launch).  K and V of ONE (frame, head) arrive in tiles of
// 64 keys (160-B LDS rows as in attn_vit.hip: conflict-free for the row fragments of K and the transposed fragments of V), double
// buffered: the global loads of tile t + 1 are issued before the products of tile t and written to the other buffer after them,
// one barrier per tile.  A wave owns 16 queries for the whole sweep; scores are computed transposed, S^T = K Q^T (key on the
// accumulator rows, query on the lane), so the running maximum / sum of a query are per-lane scalars (plus two shuffles over the
// four lane groups) and P^T is already the B operand of O^T += V^T P^T.  Online softmax: when a tile raises the maximum the
// accumulators and the running sum are rescaled by exp2((m_old - m_new) c).  No atomics: bit-reproducible, and a query's result
// depends on its frame's rows alone: not on the workgroup size, the position of the workgroup in the grid or what else the launch
// holds.
#pragma once
#include "attn_frag.hpp"

namespace {
constexpr int KT = 64;                    // keys per tile
constexpr int MAT_BYTES = KT * ROWB;

// One workgroup of NW waves = the 16 NW queries from q0 on of one (frame, head).  base: the frame's first qkv row at the head's q
// columns (row stride ldq; k at + 384, v at + 768); the frame's output rows start at row r0 of out (row stride ldo), head h at
// columns 64 h; the ntok log-sum-exps of this (frame, head) start at lse[l0] (lse may be null).
template <int NW>
DEVINL void attn_stream_tile(const bf16* base, long ldq, int ntok, int q0, bf16* out, size_t r0, int h, long ldo, float* lse,
                             size_t l0, float scale) {
    constexpr int NT = 64 * NW, RPP = NT / 8, NPASS = KT / RPP;      // RPP: tile rows staged per pass (8 threads per row)
    __shared__ __attribute__((aligned(16))) char smem[4 * MAT_BYTES];      // K0 | V0 | K1 | V1
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const int q = q0 + wid * 16 + li;                                 // tail rows: clamped loads, no stores
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
        bf16* orow = out + (r0 + q) * ldo + h * HD + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            bf16x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (bf16)(o[dt][r] * inv);
            *(bf16x4*)(orow + 16 * dt) = v;
        }
        if (lse && g == 0) lse[l0 + q] = m * scale + __logf(sum);
    }
}

// 16 pixels of one patch row, f32 -> bf16 (round to nearest even): the unit of the 16 x 16 patch gathers
DEVINL void patch_row16(const float* src, bf16* dst) {
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
}  // namespace
