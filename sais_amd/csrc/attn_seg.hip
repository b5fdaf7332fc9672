// Frames of DIFFERENT sizes in one backbone pass (eval_image_retrieval.py keeps the aspect ratio of every thumbnail; utils.
// multi_scale adds two rescaled copies of each): every frame is a SEGMENT of the stacked token rows, described by one record of a
// device table (sais_vit_seg, include/sais_hip.h), and each kernel here is one launch over all segments, so the launch list of a
// pass does not depend on how many frames or shapes it holds.  Patch 16; inference and (the *_bwd_* / scatter / expand kernels)
// training.
//   attn_seg_kernel      the streaming attention forward: attn_stream_tile (attn_stream.hpp, the body of attn_any.hip's kernel)
//                        on the (segment, first query) pair a host-made tile table names for the workgroup
//   patchify_seg_kernel  the 16 x 16 patch gather from a packed pixel buffer
//   embed_seg_kernel     token rows = CLS + pos[0] | patch GEMM output + the positional table interpolated to the segment's grid
//                        (interpolate_pos_encoding, vision_transformer.py:174-194, separable: one tap matrix per axis)
//   cls_gather_seg_kernel  the CLS row of every segment, for the final LayerNorm launch
// The backward of the pass:
//   attn_seg_dq_kernel / attn_seg_dkv_kernel  the streaming attention backward: the two tile bodies of attn_stream_bwd.hpp (those
//                        of attn_any_bwd.hip) on the forward's tile table, read once as query tiles and once as key tiles
//   embed_bwd_cast_seg_kernel / embed_bwd_pos_seg_kernel  the backward of embed_seg_kernel: the bf16 patch-row gradient, and the
//                        gradient of the class token and the positional table through the transposed tap matrices
//   cls_scatter_seg_kernel  the inverse of the gather; rows_expand_seg_kernel  per-segment values (DropPath scales) to rows
#include "attn_stream_bwd.hpp"
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

// grid (tiles, heads): the forward's tile table read as QUERY tiles (delta and dQ) ...
template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_seg_dq_kernel(const bf16* qkv, long ldq, const bf16* dout, long ldo, const bf16* out,
                                                              long ldout, const float* lse, const sais_vit_seg* segs,
                                                              const int2* tiles, float* delta, bf16* dqkv, long lddq, float scale) {
    const int2 tq = tiles[blockIdx.x];
    const int h = blockIdx.y, ntok = segs[tq.x].ntok;
    const size_t row0 = (size_t)segs[tq.x].row0, stat = row0 * NH + (size_t)h * ntok;
    attn_stream_dq_tile<NW>(qkv + row0 * ldq + h * HD, ldq, dout + row0 * ldo + h * HD, ldo, out + row0 * ldout + h * HD, ldout,
                            lse + stat, ntok, tq.y, delta + stat, dqkv + row0 * lddq + h * HD, lddq, scale);
}

// ... and as KEY tiles (dK and dV)
template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_seg_dkv_kernel(const bf16* qkv, long ldq, const bf16* dout, long ldo,
                                                               const float* lse, const float* delta, const sais_vit_seg* segs,
                                                               const int2* tiles, bf16* dqkv, long lddq, float scale) {
    const int2 tq = tiles[blockIdx.x];
    const int h = blockIdx.y, ntok = segs[tq.x].ntok;
    const size_t row0 = (size_t)segs[tq.x].row0, stat = row0 * NH + (size_t)h * ntok;
    attn_stream_dkv_tile<NW>(qkv + row0 * ldq + h * HD, ldq, dout + row0 * ldo + h * HD, ldo, lse + stat, delta + stat, ntok, tq.y,
                             dqkv + row0 * lddq + h * HD, lddq, scale);
}

// one thread = four columns of one patch row: dpatch = bf16(dx) of the patch rows in segment order (round to nearest even)
__global__ __launch_bounds__(256) void embed_bwd_cast_seg_kernel(const float* dx, const sais_vit_seg* segs, int nseg, bf16* dpatch,
                                                                 long total) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int p = (int)(i / 96), c = 4 * (int)(i % 96);
        const int s = seg_of(segs, nseg, p, 1);
        const f32x4 v = *(const f32x4*)(dx + (size_t)(p + s + 1) * DM + c);
        bf16x4 o;
        o[0] = (bf16)v[0]; o[1] = (bf16)v[1]; o[2] = (bf16)v[2]; o[3] = (bf16)v[3];
        *(bf16x4*)(dpatch + (size_t)p * DM + c) = o;
    }
}

// The gradient of the positional table and the class token.  Workgroup j < 196 owns dpos[1 + j] (j = 14 a + b), workgroup 196 owns
// dpos[0] and dcls: one writer per output element, no atomics.  The workgroup is EMB_PARTS parts of 128 threads (96 of them own
// four columns each); part k sums the segments [k per, (k + 1) per), per = ceil(nseg / EMB_PARTS), in ascending order, inside a
// segment y ascending, then x ascending, over the non-zero taps: acc = fma(Ty[y][a] * Tx[x][b], dx, acc) in f32 from 0 (a
// 14 x 14 segment: acc += its row 1 + j).  The parts are then added in ascending k from 0 and the total is added to the
// gradient buffer once.  The order depends on the table alone: two calls are bit-equal.
constexpr int EMB_PARTS = 8;
__global__ __launch_bounds__(128 * EMB_PARTS) void embed_bwd_pos_seg_kernel(const float* dx, const float* taps,
                                                                            const sais_vit_seg* segs, int nseg, float* dcls,
                                                                            float* dpos) {
    __shared__ __attribute__((aligned(16))) float part[EMB_PARTS][DM];
    const int j = blockIdx.x, k = threadIdx.x >> 7, c = 4 * (threadIdx.x & 127);
    const int per = (nseg + EMB_PARTS - 1) / EMB_PARTS, s0 = k * per, s1 = min(nseg, s0 + per);
    if (c < DM) {
        f32x4 acc = {0, 0, 0, 0};
        if (j == POS_SIDE * POS_SIDE) {
            for (int s = s0; s < s1; ++s) acc += *(const f32x4*)(dx + (size_t)segs[s].row0 * DM + c);
        } else {
            const int a = j / POS_SIDE, b = j % POS_SIDE;
            for (int s = s0; s < s1; ++s) {
                const sais_vit_seg sg = segs[s];
                const float* rows = dx + ((size_t)sg.row0 + 1) * DM + c;
                if (sg.tap_y < 0) {                                   // 14 x 14: the table itself, weight one
                    acc += *(const f32x4*)(rows + (size_t)j * DM);
                    continue;
                }
                const float* ty = taps + sg.tap_y + a;
                const float* tx = taps + sg.tap_x + b;
                for (int y = 0; y < sg.gh; ++y) {
                    const float wy = ty[y * POS_SIDE];
                    if (wy == 0.f) continue;
                    for (int x = 0; x < sg.gw; ++x) {
                        const float wx = tx[x * POS_SIDE];
                        if (wx == 0.f) continue;
                        const float w = wy * wx;
                        const f32x4 v = *(const f32x4*)(rows + ((size_t)y * sg.gw + x) * DM);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(w, v[e], acc[e]);
                    }
                }
            }
        }
        *(f32x4*)(&part[k][c]) = acc;
    }
    __syncthreads();
    if (k == 0 && c < DM) {
        f32x4 t = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < EMB_PARTS; ++i) t += *(const f32x4*)(&part[i][c]);
        if (j == POS_SIDE * POS_SIDE) {
            *(f32x4*)(dcls + c) += t;
            *(f32x4*)(dpos + c) += t;
        } else {
            *(f32x4*)(dpos + (size_t)(1 + j) * DM + c) += t;
        }
    }
}

// dst[row0 of segment s] = src[s]: the inverse of cls_gather_seg_kernel (the other rows of dst are the caller's: zeroed)
__global__ __launch_bounds__(256) void cls_scatter_seg_kernel(const float* src, const sais_vit_seg* segs, float* dst, long ldd,
                                                              int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < total) *(f32x4*)(dst + (size_t)segs[i / 96].row0 * ldd + 4 * (i % 96)) = *(const f32x4*)(src + 4 * (size_t)i);
}

// out[b][r] = in[b][segment of row r], b < nb, r < rows (dense)
__global__ __launch_bounds__(256) void rows_expand_seg_kernel(const float* in, const sais_vit_seg* segs, int nseg, int nb, long rows,
                                                              float* out) {
    for (long r = blockIdx.x * 256L + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
        const int s = seg_of(segs, nseg, (int)r, 0);
        for (int b = 0; b < nb; ++b) out[(size_t)b * rows + r] = in[(size_t)b * nseg + s];
    }
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

// the tap matrices every segment names lie inside the tap buffer (a 14 x 14 segment names none: both offsets -1)
bool taps_ok(const sais_vit_seg* h, int nseg, const float* taps_dev, long ntaps) {
    for (int s = 0; s < nseg; ++s) {
        const sais_vit_seg& g = h[s];
        if (g.tap_y < 0 || g.tap_x < 0) {                            // the table itself: only at its own grid
            if (g.tap_y != -1 || g.tap_x != -1 || g.gh != POS_SIDE || g.gw != POS_SIDE) return false;
        } else if (!taps_dev || (long)g.tap_y + (long)POS_SIDE * g.gh > ntaps || (long)g.tap_x + (long)POS_SIDE * g.gw > ntaps) {
            return false;
        }
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

namespace {
// The host copy of the tile table against a checked segment table: the rows per workgroup (64 or 32) when the table covers every
// segment in steps of it with ntiles = sum ceil(ntok / qtile) pairs that each lie inside their segment, else SAIS_ERR_ARG
int tiles_qtile(const sais_vit_seg* segs_host, int nseg, const int* tiles_host, int ntiles) {
    const int qt = sais_vit_seg_qtile(segs_host, nseg);
    if (qt < 0) return SAIS_ERR_ARG;
    long want = 0;
    for (int s = 0; s < nseg; ++s) want += (segs_host[s].ntok + qt - 1) / qt;
    if (ntiles != want) return SAIS_ERR_ARG;
    for (int t = 0; t < ntiles; ++t) {                               // a tile outside its segment would read and write other rows
        const int s = tiles_host[2 * t], q0 = tiles_host[2 * t + 1];
        if (s < 0 || s >= nseg || q0 < 0 || q0 % qt || q0 >= segs_host[s].ntok) return SAIS_ERR_ARG;
    }
    return qt;
}
}  // namespace

extern "C" int sais_vit_attn_fwd_seg(const void* qkv, long ldqkv, long rows, const sais_vit_seg* segs_host,
                                     const sais_vit_seg* segs_dev, int nseg, const int* tiles_host, const int* tiles_dev,
                                     int ntiles, void* out, long ldo, float* lse, void* stream) {
    SAIS_ENTER();
    if (!qkv || !out || !segs_host || !segs_dev || !tiles_host || !tiles_dev) return SAIS_ERR_ARG;
    if ((ldqkv & 7) || (ldo & 3) || ldqkv < 3 * DM || ldo < DM) return SAIS_ERR_ARG;
    if (((uintptr_t)segs_dev & 15) || ((uintptr_t)tiles_dev & 7)) return SAIS_ERR_ARG;
    if (!segs_ok(segs_host, nseg, rows, false)) return SAIS_ERR_ARG;
    const int qt = tiles_qtile(segs_host, nseg, tiles_host, ntiles);
    if (qt < 0) return SAIS_ERR_ARG;
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
    if (!taps_ok(segs_host, nseg, taps_dev, ntaps)) return SAIS_ERR_ARG;
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

extern "C" size_t sais_vit_attn_bwd_seg_workspace_bytes(long rows) {
    if (rows <= 0) return 0;
    return (size_t)rows * NH * sizeof(float);                         // delta f32 [6 * rows], laid out as lse
}

extern "C" int sais_vit_attn_bwd_seg(const void* qkv, long ldqkv, const void* dout, long lddo, const void* out, long ldout,
                                     const float* lse, long rows, const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev,
                                     int nseg, const int* tiles_host, const int* tiles_dev, int ntiles, void* dqkv, long lddqkv,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    SAIS_ENTER();
    if (!qkv || !dout || !out || !lse || !dqkv || !workspace || !segs_host || !segs_dev || !tiles_host || !tiles_dev)
        return SAIS_ERR_ARG;
    if ((ldqkv & 7) || (lddo & 7) || (ldout & 7) || (lddqkv & 7) || ldqkv < 3 * DM || lddo < DM || ldout < DM || lddqkv < 3 * DM)
        return SAIS_ERR_ARG;
    if (((uintptr_t)segs_dev & 15) || ((uintptr_t)tiles_dev & 7)) return SAIS_ERR_ARG;
    if (!segs_ok(segs_host, nseg, rows, false)) return SAIS_ERR_ARG;
    if (workspace_bytes < sais_vit_attn_bwd_seg_workspace_bytes(rows)) return SAIS_ERR_ARG;
    const int qt = tiles_qtile(segs_host, nseg, tiles_host, ntiles);
    if (qt < 0) return SAIS_ERR_ARG;
    const dim3 grid(ntiles, NH);
    hipStream_t s = (hipStream_t)stream;
    float* delta = (float*)workspace;
    if (qt == 64) {
        hipLaunchKernelGGL(attn_seg_dq_kernel<4>, grid, dim3(256), 0, s, (const bf16*)qkv, ldqkv, (const bf16*)dout, lddo,
                           (const bf16*)out, ldout, lse, segs_dev, (const int2*)tiles_dev, delta, (bf16*)dqkv, lddqkv, 0.125f);
        hipLaunchKernelGGL(attn_seg_dkv_kernel<4>, grid, dim3(256), 0, s, (const bf16*)qkv, ldqkv, (const bf16*)dout, lddo, lse,
                           (const float*)delta, segs_dev, (const int2*)tiles_dev, (bf16*)dqkv, lddqkv, 0.125f);
    } else {
        hipLaunchKernelGGL(attn_seg_dq_kernel<2>, grid, dim3(128), 0, s, (const bf16*)qkv, ldqkv, (const bf16*)dout, lddo,
                           (const bf16*)out, ldout, lse, segs_dev, (const int2*)tiles_dev, delta, (bf16*)dqkv, lddqkv, 0.125f);
        hipLaunchKernelGGL(attn_seg_dkv_kernel<2>, grid, dim3(128), 0, s, (const bf16*)qkv, ldqkv, (const bf16*)dout, lddo, lse,
                           (const float*)delta, segs_dev, (const int2*)tiles_dev, (bf16*)dqkv, lddqkv, 0.125f);
    }
    return sais_check_launch();
}

extern "C" int sais_vit_embed_bwd_seg(const float* dx, long rows, const float* taps_dev, long ntaps, const sais_vit_seg* segs_host,
                                      const sais_vit_seg* segs_dev, int nseg, float* dcls, float* dpos, void* dpatch_bf16,
                                      void* stream) {
    SAIS_ENTER();
    if (!dx || !dcls || !dpos || !dpatch_bf16 || !segs_dev) return SAIS_ERR_ARG;
    if (((uintptr_t)dx | (uintptr_t)dcls | (uintptr_t)dpos | (uintptr_t)segs_dev) & 15) return SAIS_ERR_ARG;
    if ((uintptr_t)dpatch_bf16 & 7) return SAIS_ERR_ARG;
    if (!segs_ok(segs_host, nseg, rows, true) || !taps_ok(segs_host, nseg, taps_dev, ntaps)) return SAIS_ERR_ARG;
    const long m = (long)segs_host[nseg - 1].row0 + segs_host[nseg - 1].ntok, total = 96 * (m - nseg);
    hipLaunchKernelGGL(embed_bwd_cast_seg_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, dx, segs_dev, nseg,
                       (bf16*)dpatch_bf16, total);
    hipLaunchKernelGGL(embed_bwd_pos_seg_kernel, dim3(POS_SIDE * POS_SIDE + 1), dim3(128 * EMB_PARTS), 0, (hipStream_t)stream, dx,
                       taps_dev, segs_dev, nseg, dcls, dpos);
    return sais_check_launch();
}

extern "C" int sais_vit_cls_scatter_seg(const float* src, const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev, int nseg,
                                        float* dst, long ldd, long rows, void* stream) {
    SAIS_ENTER();
    if (!src || !dst || !segs_dev || (ldd & 3) || ldd < DM || (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)segs_dev) & 15))
        return SAIS_ERR_ARG;
    if (!segs_ok(segs_host, nseg, rows, false)) return SAIS_ERR_ARG;
    const int total = 96 * nseg;
    hipLaunchKernelGGL(cls_scatter_seg_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, segs_dev, dst, ldd,
                       total);
    return sais_check_launch();
}

extern "C" int sais_vit_rows_expand_seg(const float* per_seg, int nb, const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev,
                                        int nseg, float* out, long rows, void* stream) {
    SAIS_ENTER();
    if (!per_seg || !out || !segs_dev || nb < 1 || ((uintptr_t)segs_dev & 15)) return SAIS_ERR_ARG;
    if (!segs_ok(segs_host, nseg, rows, true)) return SAIS_ERR_ARG;
    if ((long)segs_host[nseg - 1].row0 + segs_host[nseg - 1].ntok != rows) return SAIS_ERR_ARG;      // every row has a segment
    hipLaunchKernelGGL(rows_expand_seg_kernel, dim3(blocks_of(rows)), dim3(256), 0, (hipStream_t)stream, per_seg, segs_dev, nseg, nb,
                       rows, out);
    return sais_check_launch();
}
