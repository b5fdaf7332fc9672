// The two tile bodies of the streaming self-attention backward, one copy for attn_any_bwd.hip (one token count for every frame of
// the launch) and attn_seg.hip (segments of different token counts in one launch).  The arithmetic and the two-launch shape are
// described at the top of attn_any_bwd.hip: each body is the only writer of what it stores, a row's result depends on the rows of
// its own frame alone: not on the workgroup size, the position of the workgroup in the grid or what else the launch holds.
// Every pointer a body takes is already at ITS (frame, head): qkv / dout / out / dqkv at the frame's first row and the head's q
// columns (k at + 384, v at + 768), lse / delta at the ntok statistics of this (frame, head).
#pragma once
#include "attn_stream.hpp"

namespace {
DEVINL void load_row_frags(const bf16* base, long ld, int row, int ntok, int g, bf16x8 (&f)[2]) {
    const bf16* p = base + (size_t)(row < ntok ? row : ntok - 1) * ld + 8 * g;
    f[0] = *(const bf16x8*)p;
    f[1] = *(const bf16x8*)(p + 32);
}

// ------------------------------------------------------------------------------------------ launch 1: delta and dQ
// One workgroup of NW waves = the 16 NW queries from q0 on; a wave owns 16 of them.
template <int NW>
DEVINL void attn_stream_dq_tile(const bf16* base, long ldq, const bf16* dob, long ldo, const bf16* ob, long ldout, const float* lse,
                                int ntok, int q0, float* delta, bf16* dqb, long lddq, float scale) {
    constexpr int NT = 64 * NW, RPP = NT / 8, NPASS = KT / RPP;      // RPP: tile rows staged per pass (8 threads per row)
    __shared__ __attribute__((aligned(16))) char smem[4 * MAT_BYTES];      // K0 | V0 | K1 | V1
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const int q = q0 + wid * 16 + li;                                 // tail rows: clamped loads, no stores
    const int qc = q < ntok ? q : ntok - 1;
    bf16x8 fq[2], fdo[2];
    float dlt = 0.f;
    {
        bf16x8 fo[2];
        load_row_frags(base, ldq, q, ntok, g, fq);
        load_row_frags(dob, ldo, q, ntok, g, fdo);
        load_row_frags(ob, ldout, q, ntok, g, fo);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) dlt = __builtin_fmaf((float)fdo[ks][e], (float)fo[ks][e], dlt);
        dlt = group_sum(dlt);
    }
    const float lq = lse[qc] * LOG2E;
    if (q < ntok && g == 0) delta[q] = dlt;
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
        bf16* qrow = dqb + (size_t)q * lddq + 4 * g;
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
// One workgroup of NW waves = the 16 NW keys from k0 on; a wave owns 16 of them.
constexpr int QBUF_BYTES = 2 * MAT_BYTES + 2 * KT * 4;               // Q | dO | lse log2e [64] | delta [64]
template <int NW>
DEVINL void attn_stream_dkv_tile(const bf16* base, long ldq, const bf16* dob, long ldo, const float* lse, const float* delta,
                                 int ntok, int k0, bf16* dqb, long lddq, float scale) {
    constexpr int NT = 64 * NW, RPP = NT / 8, NPASS = KT / RPP;
    __shared__ __attribute__((aligned(16))) char smem[2 * QBUF_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
    const int key = k0 + wid * 16 + li;                               // tail rows: clamped loads, no stores
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
        vl = lse[rc];
        vdl = delta[rc];
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
        bf16* krow = dqb + (size_t)key * lddq + DM + 4 * g;
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
}  // namespace
