// Shared by the temporal attention kernels of tattn.hip (q, k, v of a head resident in LDS, S <= 96) and tattn_long.hip (keys and
// values streamed in tiles, any S): the head geometry of the temporal encoder, the 100-float LDS row, the exact-fp32 16 x 16 tile
// product on v_mfma_f32_16x16x4_f32 (slot g of step s <-> feature 24 g + s; see the operand trick in tattn.hip), and every piece
// of arithmetic that makes the two forms one operator: the score scale, the dropout rule, the masked score tile, the 4-key
// accumulate and the dK / dV step.  The files keep what their designs differ in: staging, the softmax recurrence, the slab sum.
#pragma once
#include "attn_frag.hpp"
#include "philox.hpp"

namespace {
constexpr int D = 384, TH = 4, THD = 96, TLD = 100;       // TLD: floats per LDS row
constexpr float QSCALE = 0.10206207261596577f;            // 96^-0.5, on q as it is loaded and on dS

// Train mode (p > 0): the attention weights are dropped AFTER the softmax and BEFORE P v, and the returned map is the dropped
// one (torch-1.8 F.multi_head_attention_forward).  Mask element index: ((b * 4 + h) * S + i) * S + j, in 64 bits.
struct Drop {
    const unsigned long long* rng; unsigned sid, thr; unsigned long long base; int S; bool on; float inv_keep;
    DEVINL Drop(float p, const unsigned long long* r, unsigned s, int b, int h, int S_)
        : rng(r), sid(s), thr(drop_threshold(p)), base(((unsigned long long)b * TH + h) * S_ * S_), S(S_), on(p > 0.f),
          inv_keep(p > 0.f ? 1.0f / (1.0f - p) : 1.0f) {}
    // 1 / (1 - p) where (query, key) is kept, 0 where dropped
    DEVINL float keep(int q, int key) const {
        return (!on || philox_keep(rng, sid, base + (unsigned long long)q * S + key, thr)) ? inv_keep : 0.f;
    }
};

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

// The tiles below are 16 rows of an LDS image, named by the image and the tile's first row `row0`.
// -inf on the flagged keys of a score tile (register r: key row0 + 4 g + r), m = max(m, the rest)
DEVINL void mask_tile(const unsigned char* flags, int row0, int g, f32x4& s, float& m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (flags[row0 + 4 * g + r]) s[r] = -INFINITY;
        m = fmaxf(m, s[r]);
    }
}
// the 16 keys of a tile (the key on the lane) against the lane's query qf and its dctx row gf: masked scores^T with their max,
// and dP'[query][key] = dctx_q . v_key
DEVINL void score_dp_tile(const float* sK, const float* sV, const unsigned char* flags, int row0, const float (&qf)[24],
                          const float (&gf)[24], int g, int li, f32x4& s, f32x4& dp, float& m) {
    float kf[24], vf[24];
    load24(sK + (row0 + li) * TLD, g, kf);
    load24(sV + (row0 + li) * TLD, g, vf);
    dot_tile2(kf, qf, vf, gf, s, dp);
    mask_tile(flags, row0, g, s, m);
}

using Acc6 = f32x4[THD / 16];                             // one accumulator chain per 16 features
DEVINL void zero6(Acc6& acc) {
#pragma unroll
    for (int dt = 0; dt < THD / 16; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// the lane's part of the transposed accumulators into its row `o` of a [.., 96] slice: features 16 dt + 4 g .. + 3
DEVINL void store6(float* o, int g, const Acc6& acc) {
#pragma unroll
    for (int dt = 0; dt < THD / 16; ++dt) *(f32x4*)(o + 16 * dt + 4 * g) = acc[dt];
}
// acc^T[d][query] += sum_row x[row][d] w^T[row][query] over a tile: slot g of step r <-> row row0 + 4 g + r
DEVINL void accumulate4(const float* x, int row0, const f32x4& w, int g, int li, Acc6& acc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float* row = x + (row0 + 4 * g + r) * TLD + li;
#pragma unroll
        for (int dt = 0; dt < THD / 16; ++dt) acc[dt] = mfma4(row[16 * dt], w[r], acc[dt]);
    }
}

// One 16-query step of dK / dV with the key on the lane.  The tile's queries sit at rows row0 .. of sQ / sG / sM / sI / sDot (q,
// dctx, row max, 1 / row sum, rowsum(P dP)) and are queries q0 .. of the sequence.  Scores and dP' are rebuilt, then
// P' = P keep and dS = P (dP' keep - rowsum) scale;  dV^T[d][key] += sum_q dctx[q][d] P'[q][key],  dK^T[d][key] += sum_q
// q[q][d] dS[q][key]  (register r and slot g of step r <-> query 4 g + r).
DEVINL void dkv_step(const float* sQ, const float* sG, const float* sM, const float* sI, const float* sDot, int row0, int q0, int S,
                     int key, bool key_ok, const float (&kf)[24], const float (&vf)[24], const Drop& drop, int g, int li, Acc6& adv,
                     Acc6& adk) {
    float xf[24], yf[24];
    load24(sQ + (row0 + li) * TLD, g, xf, QSCALE);
    load24(sG + (row0 + li) * TLD, g, yf);
    f32x4 s, dpp;
    dot_tile2(xf, kf, yf, vf, s, dpp);
    const f32x4 m4 = *(const f32x4*)(sM + row0 + 4 * g);
    const f32x4 i4 = *(const f32x4*)(sI + row0 + 4 * g);
    const f32x4 d4 = *(const f32x4*)(sDot + row0 + 4 * g);
    f32x4 pp, ds;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * g + r;
        const bool ok = key_ok && q < S;
        const float pv = ok ? __expf(s[r] - m4[r]) * i4[r] : 0.f;
        const float kp = ok ? drop.keep(q, key) : 0.f;
        pp[r] = pv * kp;
        ds[r] = ok ? pv * (dpp[r] * kp - d4[r]) * QSCALE : 0.f;
    }
#pragma unroll
    for (int dt = 0; dt < THD / 16; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (row0 + 4 * g + r) * TLD + 16 * dt + li;
            adv[dt] = mfma4(sG[row], pp[r], adv[dt]);
            adk[dt] = mfma4(sQ[row], ds[r], adk[dt]);
        }
}
}  // namespace
