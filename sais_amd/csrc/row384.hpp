// Row blocks of the D = 384 column kernels of norm.hip (ViT LayerNorm) and tgemm.hip (the temporal encoder's row kernels):
// one row per half-wave, lane l32 owns columns 128 i + 4 l32 .. + 3 (i = 0..2) as 12 registers (three 16-B accesses), all
// statistics in fp32.  Also the LayerNorm row statistics, the LayerNorm autograd row and the dgamma / dbeta column flush.
// ln_fwd_kernel and ln_bwd_kernel (norm.hip) keep their own copies of the statistics and of the autograd row: through the
// functions here their register counts moved (profiles/kernel_blocks_isa.json); those copies must stay in step with these.
#pragma once
#include "common.hpp"

namespace {
constexpr int D = 384;

DEVINL int col_of(int l32, int i) { return 128 * (i >> 2) + 4 * l32 + (i & 3); }      // column of register i of lane l32
DEVINL void load_f32(const float* p, int l32, float (&v)[12]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        f32x4 t = *(const f32x4*)(p + 128 * i + 4 * l32);
        v[4 * i] = t[0]; v[4 * i + 1] = t[1]; v[4 * i + 2] = t[2]; v[4 * i + 3] = t[3];
    }
}
DEVINL void load_bf16(const bf16* p, int l32, float (&v)[12]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        bf16x4 t = *(const bf16x4*)(p + 128 * i + 4 * l32);
        v[4 * i] = (float)t[0]; v[4 * i + 1] = (float)t[1]; v[4 * i + 2] = (float)t[2]; v[4 * i + 3] = (float)t[3];
    }
}
DEVINL void store_f32(float* p, int l32, const float (&v)[12]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) *(f32x4*)(p + 128 * i + 4 * l32) = f32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
}
DEVINL void store_bf16(bf16* p, int l32, const float (&v)[12]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        bf16x4 t;
        t[0] = (bf16)v[4 * i]; t[1] = (bf16)v[4 * i + 1]; t[2] = (bf16)v[4 * i + 2]; t[3] = (bf16)v[4 * i + 3];
        *(bf16x4*)(p + 128 * i + 4 * l32) = t;
    }
}

// the LayerNorm statistics of the half-wave's row: mean and 1 / sqrt(var + eps), two-pass
DEVINL void ln_row_stats(const float (&v)[12], float eps, float& mu, float& rs) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) s += v[i];
    mu = half_sum(s) * (1.0f / D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) { const float d = v[i] - mu; q += d * d; }
    rs = rsqrtf(half_sum(q) * (1.0f / D) + eps);
}

// autograd of y = (x - mu) rs g + b for the row: xv = x -> xhat, dy -> dx = rs (dy g - mean(dy g) - xhat mean(dy g xhat)); ag += dy xhat, ab += dy
DEVINL void ln_row_bwd(float (&dy)[12], float (&xv)[12], const float (&gm)[12], float mu, float rs, float (&ag)[12],
                       float (&ab)[12]) {
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        xv[i] = (xv[i] - mu) * rs;
        ag[i] += dy[i] * xv[i];
        ab[i] += dy[i];
        dy[i] *= gm[i];
        c1 += dy[i];
        c2 += dy[i] * xv[i];
    }
    c1 = half_sum(c1) * (1.0f / D);
    c2 = half_sum(c2) * (1.0f / D);
#pragma unroll
    for (int i = 0; i < 12; ++i) dy[i] = rs * (dy[i] - c1 - xv[i] * c2);
}

// dgamma += column sums of ag, dbeta += of ab over the 8 half-waves of a 256-thread workgroup: through LDS, then one
// fp32 atomic per column and workgroup.  Every thread of the workgroup calls it
DEVINL void ln_flush_dgamma_dbeta(float (&red)[2][8][D], int hw, int l32, const float (&ag)[12], const float (&ab)[12],
                                  float* dgamma, float* dbeta) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            red[0][hw][128 * i + 4 * l32 + j] = ag[4 * i + j];
            red[1][hw][128 * i + 4 * l32 + j] = ab[4 * i + j];
        }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * D; c += 256) {
        const int which = c / D, col = c - which * D;
        float s = 0.f;
#pragma unroll
        for (int h = 0; h < 8; ++h) s += red[which][h][col];
        atomicAdd((which ? dbeta : dgamma) + col, s);
    }
}
}  // namespace
