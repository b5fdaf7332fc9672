// Frames of DIFFERENT sizes in one backbone pass (eval_image_retrieval.py keeps the aspect ratio of every thumbnail; utils.
// multi_scale adds two rescaled copies of each): every frame is a SEGMENT of the stacked token rows, described by one record of a
// device table (sais_vit_seg, include/sais_hip.h), and each kernel here is one launch over all segments, so the launch list of a
// pass does not depend on how many frames or shapes it holds.  Inference only, patch 16.
//   attn_seg_kernel      the streaming attention forward: attn_stream_tile (attn_stream.hpp, the body of attn_any.hip's kernel)
//                        on the (segment, first query) pair a host-made tile table names for the workgroup
//   patchify_seg_kernel  the 16 x 16 patch gather from a packed pixel buffer
//   embed_seg_kernel     token rows = CLS + pos[0] | patch GEMM output + the positional table interpolated to the segment's grid
//                        (interpolate_pos_encoding, vision_transformer.py:174-194, separable: one tap matrix per axis)
//   cls_gather_seg_kernel  the CLS row of every segment, for the final LayerNorm launch
#include "attn_stream.hpp"
#include "../../include/sais_hip.h"

namespace {
constexpr int POS_SIDE = 14;              // the 14 x 14 positional grid of the patch-16 model

// grid (tiles, heads): tiles[b] = (segment, first query)
template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_seg_kernel(const bf16* qkv, long ldq, const sais_vit_seg* segs, const int2* tiles,
                                                           bf16* out, long ldo, float* lse, float scale) {
    const int2 tq = tiles[blockIdx.x];
    const int h = blockIdx.y, row0 = segs[tq.x].row0, ntok = segs[tq.x].ntok;
    attn_stream_tile<NW>(qkv + (size_t)row0 * ldq + h * HD, ldq, ntok, tq.y, out, (size_t)row0, h, ldo, lse,
                         (size_t)row0 * NH + (size_t)h * ntok, scale);
}

// the last segment s with key(s) <= v, key(s) = row0 - s * minus (minus = 0: token rows; 1: patch rows, one CLS row per segment)
DEVINL int seg_of(const sais_vit_seg* segs, int nseg, int v, int minus) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].row0 - mid * minus <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one thread = one 16-pixel patch row segment: item i = (patch row, channel, row of the patch)
__global__ __launch_bounds__(256) void patchify_seg_kernel(const float* pix, const sais_vit_seg* segs, int nseg, bf16* out,
                                                           long total) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int p = (int)(i / 48), rem = (int)(i % 48), c = rem >> 4, py = rem & 15;
        const int s = seg_of(segs, nseg, p, 1);
        const sais_vit_seg sg = segs[s];
        const int pl = p - (sg.row0 - s), gy = pl / sg.gw, gx = pl % sg.gw, W = 16 * sg.gw;
        const float* src = pix + sg.pix + ((size_t)c * 16 * sg.gh + 16 * gy + py) * W + gx * 16;
        patch_row16(src, out + (size_t)p * 768 + c * 256 + py * 16);
    }
}

// one thread = four columns of one token row.  The positional row of patch (y, x): sum_a Ty[y][a] (sum_b Tx[x][b] pos[1 + 14 a + b])
// over the non-zero taps (at most four per axis: sixteen terms, each sum sequential in ascending index)
__global__ __launch_bounds__(256) void embed_seg_kernel(const float* pe, const float* cls, const float* pos, const float* taps,
                                                        const sais_vit_seg* segs, int nseg, float* x, long total) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int r = (int)(i / 96), c = 4 * (int)(i % 96);
        const int s = seg_of(segs, nseg, r, 0);
        const sais_vit_seg sg = segs[s];
        const int t = r - sg.row0;
        f32x4 v;
        if (t == 0) {
            v = *(const f32x4*)(cls + c) + *(const f32x4*)(pos + c);
        } else {
            const int pl = t - 1;
            f32x4 pv;
            if (sg.tap_y < 0) {                                       // 224 x 224: the table itself (:177-178)
                pv = *(const f32x4*)(pos + (size_t)(1 + pl) * DM + c);
            } else {
                const float* ty = taps + sg.tap_y + (pl / sg.gw) * POS_SIDE;
                const float* tx = taps + sg.tap_x + (pl % sg.gw) * POS_SIDE;
                pv = f32x4{0, 0, 0, 0};
                for (int a = 0; a < POS_SIDE; ++a) {
                    const float wy = ty[a];
                    if (wy == 0.f) continue;
                    f32x4 in = {0, 0, 0, 0};
                    for (int b = 0; b < POS_SIDE; ++b) {
                        const float wx = tx[b];
                        if (wx != 0.f) in += wx * *(const f32x4*)(pos + (size_t)(1 + POS_SIDE * a + b) * DM + c);
                    }
                    pv += wy * in;
                }
            }
            v = *(const f32x4*)(pe + (size_t)(r - s - 1) * DM + c) + pv;
        }
        *(f32x4*)(x + (size_t)r * DM + c) = v;
    }
}

__global__ __launch_bounds__(256) void cls_gather_seg_kernel(const float* x, long ldx, const sais_vit_seg* segs, float* out,
                                                             int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < total) *(f32x4*)(out + 4 * (size_t)i) = *(const f32x4*)(x + (size_t)segs[i / 96].row0 * ldx + 4 * (i % 96));
}

// The host copy of the table: every record in range, segments in ascending row order without overlap inside `rows` rows;
// dense: stacked without gaps from row 0 (what the kernels that find a row's segment by search need)
bool segs_ok(const sais_vit_seg* h, int nseg, long rows, bool dense) {
    if (!h || nseg < 1 || nseg > 65535 || rows < 2 || rows > 0x7fffffffL) return false;
    long next = 0;
    for (int s = 0; s < nseg; ++s) {
        const sais_vit_seg& g = h[s];
        if (g.ntok < 2 || g.ntok > SAIS_VIT_ATTN_ANY_MAX_TOKENS || g.gh < 1 || g.gw < 1 || (long)g.gh * g.gw != g.ntok - 1)
            return false;
        if (g.row0 < next || (dense && g.row0 != next)) return false;
        next = (long)g.row0 + g.ntok;
        if (next > rows) return false;
    }
    return true;
}

unsigned blocks_of(long total) {
    const long b = (total + 255) / 256;
    return (unsigned)(b > 65536 ? 65536 : b);
}
}  // namespace

extern "C" int sais_vit_seg_qtile(const sais_vit_seg* segs_host, int nseg) {
    if (!segs_host || nseg < 1 || nseg > 65535) return SAIS_ERR_ARG;
    long wg64 = 0;
    for (int s = 0; s < nseg; ++s) {
        if (segs_host[s].ntok < 2 || segs_host[s].ntok > SAIS_VIT_ATTN_ANY_MAX_TOKENS) return SAIS_ERR_ARG;
        wg64 += (segs_host[s].ntok + 63) / 64;
    }
    return NH * wg64 >= 512 ? 64 : 32;                               // the rule of sais_vit_attn_fwd_any on the pass's total
}

extern "C" int sais_vit_attn_fwd_seg(const void* qkv, long ldqkv, long rows, const sais_vit_seg* segs_host,
                                     const sais_vit_seg* segs_dev, int nseg, const int* tiles_host, const int* tiles_dev,
                                     int ntiles, void* out, long ldo, float* lse, void* stream) {
    SAIS_ENTER();
    if (!qkv || !out || !segs_host || !segs_dev || !tiles_host || !tiles_dev) return SAIS_ERR_ARG;
    if ((ldqkv & 7) || (ldo & 3) || ldqkv < 3 * DM || ldo < DM) return SAIS_ERR_ARG;
    if (((uintptr_t)segs_dev & 15) || ((uintptr_t)tiles_dev & 7)) return SAIS_ERR_ARG;
    if (!segs_ok(segs_host, nseg, rows, false)) return SAIS_ERR_ARG;
    const int qt = sais_vit_seg_qtile(segs_host, nseg);
    long want = 0;
    for (int s = 0; s < nseg; ++s) want += (segs_host[s].ntok + qt - 1) / qt;
    if (ntiles != want) return SAIS_ERR_ARG;
    for (int t = 0; t < ntiles; ++t) {                               // a tile outside its segment would read and write other rows
        const int s = tiles_host[2 * t], q0 = tiles_host[2 * t + 1];
        if (s < 0 || s >= nseg || q0 < 0 || q0 % qt || q0 >= segs_host[s].ntok) return SAIS_ERR_ARG;
    }
    if (qt == 64) {
        hipLaunchKernelGGL(attn_seg_kernel<4>, dim3(ntiles, NH), dim3(256), 0, (hipStream_t)stream, (const bf16*)qkv, ldqkv,
                           segs_dev, (const int2*)tiles_dev, (bf16*)out, ldo, lse, 0.125f);
    } else {
        hipLaunchKernelGGL(attn_seg_kernel<2>, dim3(ntiles, NH), dim3(128), 0, (hipStream_t)stream, (const bf16*)qkv, ldqkv,
                           segs_dev, (const int2*)tiles_dev, (bf16*)out, ldo, lse, 0.125f);
    }
    return sais_check_launch();
}

extern "C" int sais_patchify_seg(const float* pixels_f32, long npix, const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev,
                                 int nseg, void* patches_bf16, void* stream) {
    SAIS_ENTER();
    if (!pixels_f32 || !patches_bf16 || !segs_dev || ((uintptr_t)pixels_f32 & 15) || ((uintptr_t)segs_dev & 15)) return SAIS_ERR_ARG;
    if (!segs_ok(segs_host, nseg, 0x7fffffffL, true)) return SAIS_ERR_ARG;
    long np = 0;
    for (int s = 0; s < nseg; ++s) {
        const sais_vit_seg& g = segs_host[s];
        const long n = 768L * g.gh * g.gw;
        if (g.pix < 0 || (g.pix & 3) || g.pix + n > npix) return SAIS_ERR_ARG;
        np += (long)g.gh * g.gw;
    }
    const long total = 48 * np;
    hipLaunchKernelGGL(patchify_seg_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, pixels_f32, segs_dev, nseg,
                       (bf16*)patches_bf16, total);
    return sais_check_launch();
}

extern "C" int sais_vit_embed_seg(const float* patch_out, const float* cls, const float* pos, const float* taps_dev, long ntaps,
                                  const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev, int nseg, float* x, long rows,
                                  void* stream) {
    SAIS_ENTER();
    if (!patch_out || !cls || !pos || !segs_dev || !x) return SAIS_ERR_ARG;
    if (((uintptr_t)patch_out | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)x | (uintptr_t)segs_dev) & 15) return SAIS_ERR_ARG;
    if (!segs_ok(segs_host, nseg, rows, true)) return SAIS_ERR_ARG;
    for (int s = 0; s < nseg; ++s) {
        const sais_vit_seg& g = segs_host[s];
        if (g.tap_y < 0 || g.tap_x < 0) {                            // the table itself: only at its own grid
            if (g.tap_y != -1 || g.tap_x != -1 || g.gh != POS_SIDE || g.gw != POS_SIDE) return SAIS_ERR_ARG;
        } else if (!taps_dev || (long)g.tap_y + (long)POS_SIDE * g.gh > ntaps || (long)g.tap_x + (long)POS_SIDE * g.gw > ntaps) {
            return SAIS_ERR_ARG;
        }
    }
    const long m = (long)segs_host[nseg - 1].row0 + segs_host[nseg - 1].ntok, total = 96 * m;
    hipLaunchKernelGGL(embed_seg_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, patch_out, cls, pos, taps_dev,
                       segs_dev, nseg, x, total);
    return sais_check_launch();
}

extern "C" int sais_vit_cls_gather_seg(const float* x, long ldx, long rows, const sais_vit_seg* segs_host,
                                       const sais_vit_seg* segs_dev, int nseg, float* out, void* stream) {
    SAIS_ENTER();
    if (!x || !out || !segs_dev || (ldx & 3) || ldx < DM || (((uintptr_t)x | (uintptr_t)out | (uintptr_t)segs_dev) & 15))
        return SAIS_ERR_ARG;
    if (!segs_ok(segs_host, nseg, rows, false)) return SAIS_ERR_ARG;
    const int total = 96 * nseg;
    hipLaunchKernelGGL(cls_gather_seg_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, ldx, segs_dev, out,
                       total);
    return sais_check_launch();
}
