// Shared by the temporal attention kernels of tattn.hip (q, k, v of a head resident in LDS, S <= 96) and tattn_long.hip (keys and
// values streamed in tiles, any S): the head geometry of the temporal encoder, the 100-float LDS row and the exact-fp32 16 x 16 tile
// product on v_mfma_f32_16x16x4_f32 (slot g of step s <-> feature 24 g + s; see the operand trick in tattn.hip).
#pragma once
#include "attn_frag.hpp"

namespace {
constexpr int D = 384, TH = 4, THD = 96, TLD = 100;       // TLD: floats per LDS row

// row[24 g .. 24 g + 23] -> registers (times `mul`)
DEVINL void load24(const float* row, int g, float (&f)[24], float mul = 1.0f) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const f32x4 t = *(const f32x4*)(row + 24 * g + 4 * i);
        f[4 * i] = t[0] * mul; f[4 * i + 1] = t[1] * mul; f[4 * i + 2] = t[2] * mul; f[4 * i + 3] = t[3] * mul;
    }
}
// T[i][j] = sum_d X[i][d] Y[j][d] for the 16 x 16 tile whose rows i / columns j are the rows `x` / `y` were loaded from:
// lane (li, g) register r holds T[4 g + r][li]
DEVINL f32x4 dot_tile(const float (&x)[24], const float (&y)[24]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 24; ++s) acc = mfma4(x[s], y[s], acc);
    return acc;
}
// two tiles at once: the two accumulator chains are independent, so the MFMAs issue back to back (a single chain waits
// out the 40-cycle dependent latency of the 32-cycle instruction)
DEVINL void dot_tile2(const float (&x0)[24], const float (&y0)[24], const float (&x1)[24], const float (&y1)[24], f32x4& a0,
                      f32x4& a1) {
    a0 = f32x4{0.f, 0.f, 0.f, 0.f};
    a1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 24; ++s) {
        a0 = mfma4(x0[s], y0[s], a0);
        a1 = mfma4(x1[s], y1[s], a1);
    }
}
}  // namespace
