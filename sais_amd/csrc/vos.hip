// Video object segmentation by label propagation over frozen patch features (dino-main/eval_video_segmentation.py):
//   sais_vos_propagate         label_propagation (:113-150) without the [nctx n, n] affinity matrix
//   sais_vos_upsample_argmax   the tail of eval_video_tracking_davis (:74-76): bilinear upsampling, norm_mask (:102-110), argmax
//
// Propagation.  A workgroup owns 16 consecutive queries (target patches, row-major over the h x w grid) and sweeps, per context
// frame, the 16-key tiles of the grid rows its windows can reach; a tile whose columns lie outside every window of the
// workgroup is skipped.  The 16 x 16 cosine tile is 96 exact-f32 MFMA steps (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain,
// the same order for every (query, key) pair and every context slot, so identical rows give bit-identical cosines) straight from
// global memory: the query fragments stay in registers, the features are L2-normalised by the caller.  exp(10 cos) is monotone
// in cos, so selection is done on the cosines, in two sweeps:
//   sweep 0  every lane keeps the `topk` largest in-window cosines it has seen (a small unsorted list in LDS, its minimum in a
//            register: after the first tiles an insertion is rare); one thread per query then extracts the topk-th largest of the
//            16 lists of its query = the threshold t (-inf when the window holds fewer than topk keys: everything is kept);
//   sweep 1  recomputes the same cosines (bit-identically) and every in-window entry with cos >= t — ties at the threshold
//            included, however many — adds exp(10 cos) and exp(10 cos) * segs[c, :, key] to the lane's own accumulators in LDS.
// The 16 accumulators of a query are summed in a fixed order and divided by the weight sum.  No atomics: bit-reproducible.
#include "common.hpp"
#include "../../include/sais_hip.h"

namespace {

constexpr int FD = SAIS_VOS_DIM;

struct VosParams {
    const float* tar;      // [n, 384]
    const float* ctx;      // [nctx, n, 384]
    const float* segs;     // [nctx, C, n]
    float* out;            // [C, n]
    int n, h, w, nctx, C, r, topk;
    int slot[SAIS_VOS_MAX_CONTEXT];      // context c lives in slot[c] of ctx / segs
};

inline size_t vos_lds_bytes(int C, int topk) { return (size_t)(256 * topk + 256 * (C + 1) + 16) * sizeof(float); }

__global__ __launch_bounds__(256) void vos_propagate_kernel(VosParams p) {
    extern __shared__ __attribute__((aligned(16))) float vsm[];
    float* const lists = vsm;                              // [256][topk]
    float* const acc = vsm + 256 * p.topk;                 // [256][C + 1]: channels, then the weight sum
    float* const thr = acc + 256 * (p.C + 1);              // [16]
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = p.n, w = p.w, R = p.r, C = p.C, topk = p.topk;
    const int q0 = blockIdx.x * 16, q = q0 + li, qc = q < n ? q : n - 1;
    const int yq = qc / w, xq = qc - yq * w;
    // the workgroup's queries: grid rows ya .. yb, columns bx0 .. bx1 (the whole width when they span two rows)
    const int qb = min(q0 + 15, n - 1), ya = q0 / w, yb = qb / w;
    const int bx0 = ya == yb ? q0 - ya * w : 0, bx1 = ya == yb ? qb - yb * w : w - 1;
    int klo = 0, khi = n;
    if (R > 0) { klo = max(0, ya - R) * w; khi = (min(p.h - 1, yb + R) + 1) * w; }
    const int kt0 = klo >> 4, nkt = ((khi + 15) >> 4) - kt0;

    // MFMA step (kk, e): lane (li, g) supplies element 16 kk + 4 g + e of its row, for the key and the query operand alike
    f32x4 qf[24];
    {
        const float* qrow = p.tar + (size_t)qc * FD + 4 * g;
#pragma unroll
        for (int kk = 0; kk < 24; ++kk) qf[kk] = *(const f32x4*)(qrow + 16 * kk);
    }
    float* const mylist = lists + tid * topk;
    float* const myacc = acc + tid * (C + 1);
    for (int j = 0; j < topk; ++j) mylist[j] = -INFINITY;
    for (int j = 0; j <= C; ++j) myacc[j] = 0.f;
    float lmin = -INFINITY, t = -INFINITY;
    int lpos = 0;

    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll 1
        for (int item = wid; item < p.nctx * nkt; item += 4) {
            const int c = item / nkt, k0 = (kt0 + item - c * nkt) * 16, sl = p.slot[c];
            if (R > 0) {                                   // wave-uniform: a tile inside one grid row, left or right of every window
                const int kb = min(k0 + 15, n - 1), yka = k0 / w, ykb = kb / w;
                if (yka == ykb && (kb - ykb * w < bx0 - R || k0 - yka * w > bx1 + R)) continue;
            }
            const float* krow = p.ctx + ((size_t)sl * n + min(k0 + li, n - 1)) * FD + 4 * g;
            f32x4 kf[24];
#pragma unroll
            for (int kk = 0; kk < 24; ++kk) kf[kk] = *(const f32x4*)(krow + 16 * kk);
            f32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};   // two chains (even / odd kk): back-to-back issue
#pragma unroll
            for (int kk = 0; kk < 24; kk += 2)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a0 = mfma4(kf[kk][e], qf[kk][e], a0);
                    a1 = mfma4(kf[kk + 1][e], qf[kk + 1][e], a1);
                }
            const f32x4 cosv = a0 + a1;                    // cosv[r]: key k0 + 4 g + r, query q0 + li
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int key = k0 + 4 * g + r4;
                bool ok = key < n && q < n;
                if (R > 0) {
                    const int yk = key / w, xk = key - yk * w;
                    ok = ok && abs(yk - yq) <= R && abs(xk - xq) <= R;
                }
                const float v = cosv[r4];
                if (!ok) continue;
                if (pass == 0) {
                    if (v > lmin) {                        // replace the list's minimum, find the new one
                        mylist[lpos] = v;
                        lmin = INFINITY;
                        for (int j = 0; j < topk; ++j) {
                            const float u = mylist[j];
                            if (u < lmin) { lmin = u; lpos = j; }
                        }
                    }
                } else if (v >= t) {
                    const float wgt = expf(10.0f * v);
                    myacc[C] += wgt;
                    const float* sp = p.segs + (size_t)sl * C * n + key;
                    for (int ch = 0; ch < C; ++ch) myacc[ch] = __builtin_fmaf(wgt, sp[(size_t)ch * n], myacc[ch]);
                }
            }
        }
        if (pass == 0) {
            __syncthreads();
            if (tid < 16) {                                // query tid: the lists of threads 16 s + tid, s = 4 wave + g
                float last = -INFINITY;
                for (int round = 0; round < topk; ++round) {
                    float best = -INFINITY;
                    int bi = -1;
                    for (int s = 0; s < 16; ++s)
                        for (int j = 0; j < topk; ++j) {
                            const int idx = (16 * s + tid) * topk + j;
                            const float u = lists[idx];
                            if (u > best) { best = u; bi = idx; }
                        }
                    last = best;
                    if (bi < 0) break;                     // fewer than topk in-window keys: keep them all
                    lists[bi] = -INFINITY;
                }
                thr[tid] = last;
            }
            __syncthreads();
            t = thr[li];
        }
    }
    __syncthreads();
    for (int ch = tid >> 4; ch < C; ch += 16) {            // thread: query q0 + (tid & 15), channels ch, ch + 16, ..
        const int l2 = tid & 15;
        float sum = 0.f, ws = 0.f;
        for (int s = 0; s < 16; ++s) {
            const float* a = acc + (16 * s + l2) * (C + 1);
            sum += a[ch];
            ws += a[C];
        }
        if (q0 + l2 < n) p.out[(size_t)ch * n + q0 + l2] = sum / ws;
    }
}

// ---------------------------------------------------------------------------------------------- upsample + norm_mask + argmax
constexpr int UNB = SAIS_VOS_UPSAMPLE_WS_FLOATS / 2;       // partial (min, max) pairs per channel

// F.interpolate(mode='bilinear', align_corners=False, scale_factor=patch) at output pixel (y, x) of one channel
DEVINL float bilerp(const float* ch, int h, int w, int y, int x, float inv) {
    const float sy = fmaxf((y + 0.5f) * inv - 0.5f, 0.f), sx = fmaxf((x + 0.5f) * inv - 0.5f, 0.f);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = sy - y0, lx = sx - x0, hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * ch[y0 * w + x0] + lx * ch[y0 * w + x1]) + ly * (hx * ch[y1 * w + x0] + lx * ch[y1 * w + x1]);
}

// grid (UNB, C): partial minimum / maximum of the upsampled channel
__global__ __launch_bounds__(256) void vos_minmax_kernel(const float* seg, int h, int w, int patch, float* ws) {
    __shared__ float smn[4], smx[4];
    const int c = blockIdx.y, H = h * patch, W = w * patch;
    const float* ch = seg + (size_t)c * h * w;
    const float inv = 1.0f / patch;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < H * W; i += UNB * 256) {
        const int y = i / W, x = i - y * W;
        const float v = bilerp(ch, h, w, y, x, inv);
        mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
    mn = -wave_max(-mn); mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[((size_t)c * UNB + blockIdx.x) * 2] = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
        ws[((size_t)c * UNB + blockIdx.x) * 2 + 1] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
    }
}

// one thread per output pixel: norm_mask per channel, then torch.max(dim=0): the first of the largest, a NaN (a constant
// positive channel is 0 / 0 after norm_mask) counting as the largest
__global__ __launch_bounds__(256) void vos_argmax_kernel(const float* seg, int C, int h, int w, int patch, const float* ws,
                                                         unsigned char* labels) {
    __shared__ float smn[SAIS_VOS_MAX_CLASSES], smx[SAIS_VOS_MAX_CLASSES];
    if ((int)threadIdx.x < C) {
        float mn = INFINITY, mx = -INFINITY;
        for (int b = 0; b < UNB; ++b) {
            mn = fminf(mn, ws[((size_t)threadIdx.x * UNB + b) * 2]);
            mx = fmaxf(mx, ws[((size_t)threadIdx.x * UNB + b) * 2 + 1]);
        }
        smn[threadIdx.x] = mn; smx[threadIdx.x] = mx;
    }
    __syncthreads();
    const int H = h * patch, W = w * patch;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    const float inv = 1.0f / patch;
    float best = 0.f;
    int bc = 0;
    for (int c = 0; c < C; ++c) {
        float v = bilerp(seg + (size_t)c * h * w, h, w, y, x, inv);
        if (smx[c] > 0.f) v = (v - smn[c]) / (smx[c] - smn[c]);
        if (c == 0 || v > best || (v != v && best == best)) { best = v; bc = c; }
    }
    labels[i] = (unsigned char)bc;
}

}  // namespace

extern "C" int sais_vos_propagate(const float* tar, const float* ctx, const float* segs, int nctx, int C, int h, int w, int dim,
                                  int radius, int topk, const int* ctx_order, float* out, void* stream) {
    SAIS_ENTER();
    if (!tar || !ctx || !segs || !out) return SAIS_ERR_ARG;
    if (nctx < 1 || nctx > SAIS_VOS_MAX_CONTEXT || C < 1 || C > SAIS_VOS_MAX_CLASSES || topk < 1 || topk > SAIS_VOS_MAX_TOPK)
        return SAIS_ERR_ARG;
    if (h < 1 || w < 1 || (long)h * w > SAIS_VOS_MAX_PATCHES || dim != SAIS_VOS_DIM || radius < 0) return SAIS_ERR_ARG;
    const int n = h * w;
    VosParams p{tar, ctx, segs, out, n, h, w, nctx, C, radius, topk, {0}};
    for (int c = 0; c < nctx; ++c) {
        p.slot[c] = ctx_order ? ctx_order[c] : c;
        if (p.slot[c] < 0 || p.slot[c] >= SAIS_VOS_MAX_CONTEXT) return SAIS_ERR_ARG;
    }
    if (!sais_dyn_lds_once<vos_propagate_kernel>((int)vos_lds_bytes(SAIS_VOS_MAX_CLASSES, SAIS_VOS_MAX_TOPK))) return SAIS_ERR_LAUNCH;
    hipLaunchKernelGGL(vos_propagate_kernel, dim3((n + 15) / 16), dim3(256), vos_lds_bytes(C, topk), (hipStream_t)stream, p);
    return sais_check_launch();
}

extern "C" int sais_vos_upsample_argmax(const float* seg, int C, int h, int w, int patch, unsigned char* labels,
                                        float* workspace, void* stream) {
    SAIS_ENTER();
    if (!seg || !labels || !workspace) return SAIS_ERR_ARG;
    if (C < 1 || C > SAIS_VOS_MAX_CLASSES || h < 1 || w < 1 || (long)h * w > SAIS_VOS_MAX_PATCHES || patch < 1 || patch > 64)
        return SAIS_ERR_ARG;
    const int npix = h * patch * w * patch;                // <= 4096 * 4096
    hipLaunchKernelGGL(vos_minmax_kernel, dim3(UNB, C), dim3(256), 0, (hipStream_t)stream, seg, h, w, patch, workspace);
    hipLaunchKernelGGL(vos_argmax_kernel, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, seg, C, h, w, patch,
                       (const float*)workspace, labels);
    return sais_check_launch();
}
