// Shared by the 128 x 128 NT GEMMs of gemm.hip, gemm_nt_exp.hip and gemm_nt_f32.hip.  Device: tile constants and the 16-columns-per-
// lane epilogue of the four-wave (2 x 2 waves of 64 x 64) tile.  Host (end of file): what sais_gemm_nt and sais_gemm_nt_exp_ share.
// The bf16x3 stage of gemm_nt_f32.hip (LDS image, K step) is in f32x3_tile.hpp, shared with knn.hip.
#pragma once
#include "gemm_nt_epi.hpp"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;      // 16 KiB per operand per stage

// Epilogue in two phases.  vmcnt is in-order and counts stores on CDNA4, so a load issued after a store cannot be
// consumed before that store has been acknowledged: phase A issues EVERY load a lane needs (bias once, the
// residual / pre-activation rows of all four 16-row sub-tiles), phase B only does arithmetic and stores.
struct EpiAux {
    f32x4 r[4][4];        // f32 aux (residual / position rows): 16 columns x 4 sub-tiles
    bf16x8 u[4][2];       // bf16 aux (pre-activation)
    u32x4 q[4];           // one-byte GELU' codes
};

template <int EPI>
DEVINL void epilogue_loads(const NtParams& p, int mbase, int li, int n, float (&b)[16], EpiAux& a) {
    if (p.bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 t = *(const f32x4*)(p.bias + n + 4 * i);
            b[4 * i] = t[0]; b[4 * i + 1] = t[1]; b[4 * i + 2] = t[2]; b[4 * i + 3] = t[3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) b[i] = 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        int m = mbase + mt * 16 + li;
        m = m < p.M ? m : p.M - 1;
        if constexpr (EPI == SAIS_EPI_BIAS_RESID_F32 || EPI == SAIS_EPI_PATCH_F32) {
            size_t row = m;
            if constexpr (EPI == SAIS_EPI_PATCH_F32) row = (m % p.grp_in) + p.grp_off;
            const float* r = (const float*)p.aux + row * p.ldaux + n;
#pragma unroll
            for (int i = 0; i < 4; ++i) a.r[mt][i] = *(const f32x4*)(r + 4 * i);
        } else if constexpr (EPI == SAIS_EPI_DGELU_BF16 || EPI == SAIS_EPI_DRELU_BF16 || EPI == SAIS_EPI_MUL_BF16) {
            const bf16* u = (const bf16*)p.aux + (size_t)m * p.ldaux + n;
            a.u[mt][0] = *(const bf16x8*)u;
            a.u[mt][1] = *(const bf16x8*)(u + 8);
        } else if constexpr (EPI == SAIS_EPI_MULQ_BF16) {
            a.q[mt] = *(const u32x4*)((const unsigned char*)p.aux + (size_t)m * p.ldaux + n);
        }
    }
}

template <int EPI>
DEVINL void epilogue(const NtParams& p, int m, int n, const float (&v)[16], const float (&b)[16], const EpiAux& a, int mt) {
    // one output row m, 16 contiguous columns n..n+15 (n multiple of 16)
    float y[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) y[i] = v[i] + b[i];

    auto store_bf16 = [&](void* base, int ld, const float (&z)[16]) {
        bf16x8 lo, hi;
#pragma unroll
        for (int i = 0; i < 8; ++i) { lo[i] = (bf16)z[i]; hi[i] = (bf16)z[8 + i]; }
        bf16* o = (bf16*)base + (size_t)m * ld + n;
        *(bf16x8*)o = lo;
        *(bf16x8*)(o + 8) = hi;
    };
    auto store_f32 = [&](void* base, int ld, size_t row, const float (&z)[16]) {
        float* o = (float*)base + row * ld + n;
#pragma unroll
        for (int i = 0; i < 4; ++i) *(f32x4*)(o + 4 * i) = f32x4{z[4 * i], z[4 * i + 1], z[4 * i + 2], z[4 * i + 3]};
    };

    if constexpr (EPI == SAIS_EPI_BIAS_BF16) {
        store_bf16(p.out, p.ldo, y);
    } else if constexpr (EPI == SAIS_EPI_BIAS_RELU_BF16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) y[i] = fmaxf(y[i], 0.f);
        store_bf16(p.out, p.ldo, y);
    } else if constexpr (EPI == SAIS_EPI_BIAS_F32) {
        store_f32(p.out, p.ldo, m, y);
    } else if constexpr (EPI == SAIS_EPI_BIAS_RESID_F32 || EPI == SAIS_EPI_PATCH_F32) {
        if constexpr (EPI == SAIS_EPI_BIAS_RESID_F32) {
            if (p.rowscale) {                                   // DropPath: residual + s_m (acc + bias)
                const float sc = p.rowscale[m];
#pragma unroll
                for (int i = 0; i < 16; ++i) y[i] *= sc;
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) y[i] += a.r[mt][i >> 2][i & 3];
        size_t orow = m;
        if constexpr (EPI == SAIS_EPI_PATCH_F32) orow = (size_t)(m / p.grp_in) * p.grp_out + (m % p.grp_in) + p.grp_off;
        store_f32(p.out, p.ldo, orow, y);
        if constexpr (EPI == SAIS_EPI_BIAS_RESID_F32)
            if (p.out2) store_bf16(p.out2, p.ldo2, y);
    } else if constexpr (EPI == SAIS_EPI_BIAS_GELU_BF16) {
        if (p.out2) store_bf16(p.out2, p.ldo2, y);          // pre-activation u (training)
        gelu_erf_n(y);
        store_bf16(p.out, p.ldo, y);
    } else if constexpr (EPI == SAIS_EPI_BIAS_GELU_GRAD_BF16) {
        float d[16];
        gelu_and_grad_n(y, d);
        store_bf16(p.out2, p.ldo2, d);
        store_bf16(p.out, p.ldo, y);
    } else if constexpr (EPI == SAIS_EPI_BIAS_GELU_GRADQ_BF16) {
        float d[16];
        gelu_and_grad_n(y, d);
        *(u32x4*)((unsigned char*)p.out2 + (size_t)m * p.ldo2 + n) =
            u32x4{gq8_pack4(d[0], d[1], d[2], d[3]), gq8_pack4(d[4], d[5], d[6], d[7]), gq8_pack4(d[8], d[9], d[10], d[11]),
                  gq8_pack4(d[12], d[13], d[14], d[15])};
        store_bf16(p.out, p.ldo, y);
    } else if constexpr (EPI == SAIS_EPI_MUL_BF16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) y[i] *= (float)a.u[mt][i >> 3][i & 7];
        store_bf16(p.out, p.ldo, y);
    } else if constexpr (EPI == SAIS_EPI_MULQ_BF16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) y[i] *= gq8_decode(a.q[mt][i >> 2], i & 3);
        store_bf16(p.out, p.ldo, y);
    } else if constexpr (EPI == SAIS_EPI_DGELU_BF16) {
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
            f32x2 g;
            dgelu_erf2(f32x2{(float)a.u[mt][i >> 3][i & 7], (float)a.u[mt][i >> 3][(i & 7) + 1]}, g);
            y[i] *= g.x, y[i + 1] *= g.y;
        }
        store_bf16(p.out, p.ldo, y);
    } else if constexpr (EPI == SAIS_EPI_DRELU_BF16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) y[i] = (float)a.u[mt][i >> 3][i & 7] > 0.f ? y[i] : 0.f;
        store_bf16(p.out, p.ldo, y);
    }
}

// the epilogues sais_gemm_nt takes, one kernel instantiation each: X(E) for every one
#define NT_EPILOGUES(X)                                                                                                          \
    X(SAIS_EPI_BIAS_BF16) X(SAIS_EPI_BIAS_RELU_BF16) X(SAIS_EPI_BIAS_F32) X(SAIS_EPI_BIAS_RESID_F32) X(SAIS_EPI_BIAS_GELU_BF16) \
    X(SAIS_EPI_DGELU_BF16) X(SAIS_EPI_DRELU_BF16) X(SAIS_EPI_PATCH_F32) X(SAIS_EPI_BIAS_GELU_GRAD_BF16) X(SAIS_EPI_MUL_BF16)     \
    X(SAIS_EPI_BIAS_GELU_GRADQ_BF16) X(SAIS_EPI_MULQ_BF16)

// host side: kernel parameters and the 128 x 128 tile count of a bf16 NT GEMM
inline NtParams nt_params(const SaisGemm* g) {
    return NtParams{(const bf16*)g->A, (const bf16*)g->B, g->lda, g->ldb, g->M, g->N, g->K, g->bias,
                    g->out, g->ldo, g->out2, g->ldo2, g->aux, g->ldaux, g->grp_in, g->grp_out, g->grp_off, g->rowscale};
}
inline dim3 nt_tiles(const SaisGemm* g) { return dim3((g->N / BN) * ((g->M + BM - 1) / BM)); }

}  // namespace
