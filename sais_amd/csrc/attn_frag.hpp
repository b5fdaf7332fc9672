// Shared by the attention kernels of attn_vit.hip (K and V of a head resident in LDS) and attn_any.hip (K and V streamed in
// tiles): the head geometry of the DINO ViT, the 160-B-row LDS image and its MFMA fragments, and the softmax pieces of the
// S^T = K Q^T orientation (key on the accumulator rows, query on the lane).  tattn.hip uses group_max / group_sum.
#pragma once
#include "common.hpp"

namespace {
constexpr int HD = 64, NH = 6, DM = 384;
constexpr int ROWB = 160;                 // LDS row stride in bytes
constexpr float LOG2E = 1.4426950408889634f;

DEVINL bf16x8 row_frag(const char* lds, int row, int chunk) { return *(const bf16x8*)(lds + row * ROWB + chunk * 16); }

// transposed fragment for k-step s (32 tokens) and 16-wide column tile ct:
// element e of lane group g  <->  token 32 s + 16 (e >> 2) + 4 g + (e & 3)
DEVINL bf16x8 tr_frag(const char* lds, int s, int ct, int g, int li) {
    const char* p = lds + (32 * s + 4 * g + (li >> 2)) * ROWB + (16 * ct + 4 * (li & 3)) * 2;
    return cat4(lds_read_tr16(p), lds_read_tr16(p + 16 * ROWB));
}

// raw v_exp_f32 (exp2f() adds a denormal-range fix-up of 4 VALU per element; arguments here are <= ~0 and a
// flush to zero of results below 2^-126 is exactly what softmax wants)
DEVINL float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// over the four lane groups g = lane >> 4 that share a query (lanes li, li + 16, li + 32, li + 48)
DEVINL float group_max(float v) { v = fmaxf(v, __shfl_xor(v, 16)); return fmaxf(v, __shfl_xor(v, 32)); }
DEVINL float group_sum(float v) { v += __shfl_xor(v, 16); return v + __shfl_xor(v, 32); }

DEVINL bf16x8 pack_p(const f32x4& a, const f32x4& b) {
    bf16x8 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[i] = (bf16)a[i]; r[4 + i] = (bf16)b[i]; }
    return r;
}
}  // namespace
