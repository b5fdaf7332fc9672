// One 128 x 128 x 64 stage of the "bf16x3" product (fp32 operands at ~fp32 accuracy on the bf16 matrix cores): the LDS image
// A_hi | A_lo | B_hi | B_lo and the K step over it.  Shared by gemm_nt_f32x3_kernel (gemm_nt_f32.hip) and knn_search_kernel
// (knn.hip), which promises the arithmetic of the former: the split, the term order and the K order are stated here only.
// Four waves as 2 x 2 of 64 x 64 (wr, wc); swizzle, operand swap and weight-row permutation as in the bf16 NT kernel.
#pragma once
#include "common.hpp"

namespace {
constexpr int F32X3_IMG_BYTES = 128 * 64 * 2;            // one operand half: 128 rows x 64 bf16
constexpr int F32X3_LDS_BYTES = 4 * F32X3_IMG_BYTES;

DEVINL void f32x3_store_row(char* smem, int r, int sc, const f32x4& a0, const f32x4& a1, const u32x4& bhi, const u32x4& blo) {
    u32x4 hi, lo;
    split8(a0, a1, hi, lo);
    *(u32x4*)(smem + swz(r, sc)) = hi;
    *(u32x4*)(smem + F32X3_IMG_BYTES + swz(r, sc)) = lo;
    *(u32x4*)(smem + 2 * F32X3_IMG_BYTES + swz(perm_row(r), sc)) = bhi;
    *(u32x4*)(smem + 3 * F32X3_IMG_BYTES + swz(perm_row(r), sc)) = blo;
}

// acc += a_hi b_lo + a_lo b_hi + a_hi b_hi over the 64 k of the stage (2 x 48 MFMAs), smallest term first
DEVINL void f32x3_kstep(const char* smem, int wr, int wc, int g, int li, f32x4 (&acc)[4][4]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        bf16x8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int oa = swz(wr * 64 + t * 16 + li, ks * 4 + g), ob = swz(wc * 64 + t * 16 + li, ks * 4 + g);
            ah[t] = *(const bf16x8*)(smem + oa);
            al[t] = *(const bf16x8*)(smem + F32X3_IMG_BYTES + oa);
            bh[t] = *(const bf16x8*)(smem + 2 * F32X3_IMG_BYTES + ob);
            bl[t] = *(const bf16x8*)(smem + 3 * F32X3_IMG_BYTES + ob);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                f32x4 c = acc[mt][nt];
                c = mfma16(bl[nt], ah[mt], c);
                c = mfma16(bh[nt], al[mt], c);
                c = mfma16(bh[nt], ah[mt], c);
                acc[mt][nt] = c;
            }
    }
}
}  // namespace
