// bf16 MFMA TN GEMMs for the SAIS hot path (gfx950): every weight / bias gradient.
//
//  sais_gemm_tn : dW[N1,N2] += P[M,N1]^T . Q[M,N2],  db[N1] += colsum(P); grouped forms for the dW of a whole block in one launch.
//
// TN: dW[N1,N2] += sum_m P[m,N1] Q[m,N2].  Reduction index m is the SLOW dimension of both
// operands, so MFMA fragments (8 consecutive k per lane) are column reads of the row-major LDS
// tiles: ds_read_b64_tr_b16 (two per fragment).  LDS rows are padded 256 -> 288 B so the 8 rows a
// half-wave touches per read fall on distinct banks.  Split over M (gridDim.z) with fp32
// atomicAdd of the partial tiles; db via one extra MFMA column of ones in the n2-tile-0 blocks.
#include "common.hpp"
#include "tn_plan.hpp"

namespace {

constexpr int TROW = 288;              // padded LDS row bytes (128 bf16 + 16 pad)
constexpr int TTILE = TK * TROW;       // 18 KiB

struct TnParams {
    const void* P; const void* Q; int ldp, ldq, M, N1, N2;
    float* dW; int ldw; float* db; int rows_per_split;
};

// 8 consecutive elements -> packed bf16x8 (f32 inputs are rounded to bf16 while staging)
DEVINL u32x4 load8_bf16(const bf16* p) { return *(const u32x4*)p; }
DEVINL u32x4 load8_bf16(const float* p) {
    f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
    bf16x8 v;
    v[0] = (bf16)a[0]; v[1] = (bf16)a[1]; v[2] = (bf16)a[2]; v[3] = (bf16)a[3];
    v[4] = (bf16)b[0]; v[5] = (bf16)b[1]; v[6] = (bf16)b[2]; v[7] = (bf16)b[3];
    return __builtin_bit_cast(u32x4, v);
}

// one 128x128 output tile over rows [mbeg, mend) of P / Q
// OWNED: the workgroup is the only writer of its output tile in this launch (one M-split), so the accumulation into dW / db
// is a plain read-add-write instead of 16 k atomics per tile (the few-row temporal dW GEMMs were atomics-bound: 37 -> 23 us)
// NP = P columns (= dW rows) per tile: 128, or 64 for the few-row temporal dW launches (twice the workgroups, half the
// read-add-write epilogue per workgroup)
template <typename T, bool OWNED = false, int NP = 128>
DEVINL void tn_tile(const TnParams& p, int n1_0, int n2_0, int mbeg, int mend, char* smem) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, g = lane >> 4, li = lane & 15;

    // staging: tile = 64 rows x 128 cols bf16 = 64 x 16 chunks; thread -> chunk tid&15, rows tid>>4 + 16 i
    const int sc = tid & 15, sr = tid >> 4;
    u32x4 rp[4], rq[4];
    auto gload = [&](int mb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int m = mb + sr + 16 * i;
            bool ok = m < mend;
            rp[i] = (ok && sc < NP / 8) ? load8_bf16((const T*)p.P + (size_t)m * p.ldp + n1_0 + sc * 8) : u32x4{0, 0, 0, 0};
            rq[i] = ok ? load8_bf16((const T*)p.Q + (size_t)m * p.ldq + n2_0 + sc * 8) : u32x4{0, 0, 0, 0};
        }
    };
    auto lstore = [&](int stage) {
        char* s = smem + stage * 2 * TTILE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int off = (sr + 16 * i) * TROW + sc * 16;
            *(u32x4*)(s + off) = rp[i];
            *(u32x4*)(s + TTILE + off) = rq[i];
        }
    };

    constexpr int PT = NP / 32;                    // 16-column P tiles per wave (the wave owns NP / 2 dW rows)
    f32x4 acc[PT][4];
    f32x4 accb[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        accb[i] = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    }
    const bool do_bias = p.db != nullptr && n2_0 == 0 && wc == 0;
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (bf16)1.0f;

    // tr16 read address: lane-in-group = 4q + p supplies row q, cols c0 + 4p..4p+3 of the 4x16 block
    const int q4 = li >> 2, p4 = li & 3;
    const int nsteps = (mend - mbeg + TK - 1) / TK;
    gload(mbeg);
    lstore(0);
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        if (st + 1 < nsteps) gload(mbeg + (st + 1) * TK);
        const char* sp = smem + cur * 2 * TTILE;
        const char* sq = sp + TTILE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fp[PT], fq[4];
            // k-slot (g, e) <-> m = 32 ks + 16 (e>>2) + 4 g + (e&3): a half-wave touches 8 CONSECUTIVE rows
            // per read (conflict-free with the 288-B row stride); P and Q use the same slot map.
            const int rbase = (ks * 32 + 4 * g + q4) * TROW + p4 * 8;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                int cq = (wc * 64 + t * 16) * 2;
                fq[t] = cat4(lds_read_tr16(sq + rbase + cq), lds_read_tr16(sq + rbase + 16 * TROW + cq));
            }
#pragma unroll
            for (int t = 0; t < PT; ++t) {
                int cp = (wr * (NP / 2) + t * 16) * 2;
                fp[t] = cat4(lds_read_tr16(sp + rbase + cp), lds_read_tr16(sp + rbase + 16 * TROW + cp));
            }
#pragma unroll
            for (int it = 0; it < PT; ++it)
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) acc[it][jt] = mfma16(fp[it], fq[jt], acc[it][jt]);
            if (do_bias) {
#pragma unroll
                for (int it = 0; it < PT; ++it) accb[it] = mfma16(fp[it], ones, accb[it]);
            }
        }
        if (st + 1 < nsteps) lstore(cur ^ 1);
        __syncthreads();
    }
    // D[i = n1][j = n2]: lane holds n2 = tile + li, n1 = tile + 4g + r
#pragma unroll
    for (int it = 0; it < PT; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int n1 = n1_0 + wr * (NP / 2) + it * 16 + 4 * g + r;
            float* row = p.dW + (size_t)n1 * p.ldw + n2_0 + wc * 64 + li;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                if constexpr (OWNED) row[jt * 16] += acc[it][jt][r];
                else atomicAdd(row + jt * 16, acc[it][jt][r]);
            }
            if (do_bias && li == 0) {
                if constexpr (OWNED) p.db[n1] += accb[it][r];
                else atomicAdd(p.db + n1, accb[it][r]);
            }
        }
}

// LDS-DMA variant of tn_tile for bf16 operands when every M-split is a whole number of 64-row steps:
// unpadded 256-B rows, 32-B units XOR-swizzled by (row & 7) on the SOURCE address (a half-wave's transposed read
// touches 8 consecutive rows x 32 B -> 8 distinct units = all 64 banks), two 32-KiB stages.
DEVINL const char* tr_addr(const char* tile, int row, int col) {       // col multiple of 4
    return tile + row * 256 + ((((col >> 4) ^ (row & 7)) << 5) | ((col & 15) << 1));
}

DEVINL void tn_tile_dma(const TnParams& p, int n1_0, int n2_0, int mbeg, int mend, char* smem) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1, g = lane >> 4, li = lane & 15;
    constexpr int T16 = 64 * 256;                                       // 16 KiB per operand per stage
    // pieces 4w..4w+3 of each operand: piece = 4 rows; lane -> row 4*piece + (lane>>4), position lane&15
    const bf16* psrc[4]; const bf16* qsrc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 4 * (4 * wid + j) + (lane >> 4);
        const int c = lane & 15, u = (c >> 1) ^ (r & 7);
        psrc[j] = (const bf16*)p.P + (size_t)(mbeg + r) * p.ldp + n1_0 + u * 16 + (c & 1) * 8;
        qsrc[j] = (const bf16*)p.Q + (size_t)(mbeg + r) * p.ldq + n2_0 + u * 16 + (c & 1) * 8;
    }
    auto issue = [&](int stage, int step) {
        char* s = smem + stage * 2 * T16 + (4 * wid) * 1024;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            glds16(psrc[j] + (size_t)step * 64 * p.ldp, s + j * 1024);
            glds16(qsrc[j] + (size_t)step * 64 * p.ldq, s + T16 + j * 1024);
        }
    };
    f32x4 acc[4][4];
    f32x4 accb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        accb[i] = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    }
    const bool do_bias = p.db != nullptr && n2_0 == 0 && wc == 0;
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (bf16)1.0f;
    const int q4 = li >> 2, p4 = li & 3;
    const int nsteps = (mend - mbeg) / TK;
    issue(0, 0);
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        if (st + 1 < nsteps) issue(cur ^ 1, st + 1);
        const char* sp = smem + cur * 2 * T16;
        const char* sq = sp + T16;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fp[4], fq[4];
            const int row = ks * 32 + 4 * g + q4;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int cp = wr * 64 + t * 16 + 4 * p4, cq = wc * 64 + t * 16 + 4 * p4;
                fp[t] = cat4(lds_read_tr16(tr_addr(sp, row, cp)), lds_read_tr16(tr_addr(sp, row + 16, cp)));
                fq[t] = cat4(lds_read_tr16(tr_addr(sq, row, cq)), lds_read_tr16(tr_addr(sq, row + 16, cq)));
            }
#pragma unroll
            for (int it = 0; it < 4; ++it)
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) acc[it][jt] = mfma16(fp[it], fq[jt], acc[it][jt]);
            if (do_bias) {
#pragma unroll
                for (int it = 0; it < 4; ++it) accb[it] = mfma16(fp[it], ones, accb[it]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int n1 = n1_0 + wr * 64 + it * 16 + 4 * g + r;
            float* row = p.dW + (size_t)n1 * p.ldw + n2_0 + wc * 64 + li;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) atomicAdd(row + jt * 16, acc[it][jt][r]);
            if (do_bias && li == 0) atomicAdd(p.db + n1, accb[it][r]);
        }
}

template <typename T>
__global__ __launch_bounds__(256) void gemm_tn_kernel(TnParams p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TTILE];   // 72 KiB
    // 1-D grid, XCD-aware order with the M-split as the slow index: the (N1/128)*(N2/128) tiles of one split
    // run on ONE XCD back to back and share that split's P and Q row slabs through its L2 (the slabs are then
    // fetched from HBM once instead of once per tile).
    const int nt2 = p.N2 / 128, ntile = (p.N1 / 128) * nt2;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int split = wg / ntile, t12 = wg - split * ntile;
    const int mbeg = split * p.rows_per_split;
    const int mend = min(p.M, mbeg + p.rows_per_split);
    if (mbeg >= mend) return;
    tn_tile<T>(p, (t12 / nt2) * 128, (t12 % nt2) * 128, mbeg, mend, smem);
}

// Several weight-gradient GEMMs over the SAME M rows in one launch (the four nn.Linear of a ViT block): 108 tiles
// instead of 9-36, so 4 M-splits fill the chip where the per-GEMM launches needed 12-48, and the fp32 atomic
// traffic (64 KiB per workgroup) drops by the same factor.
struct TnGroup {
    TnParams item[SAIS_TN_MAX_ITEMS];
    int tile_end[SAIS_TN_MAX_ITEMS];          // prefix sums of tiles per item
    int nitems, ntiles;
};

__global__ __launch_bounds__(256) void gemm_tn_grouped_kernel(TnGroup gp) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TTILE];
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int split = wg / gp.ntiles;
    int t = wg - split * gp.ntiles, it = 0;
    while (it + 1 < gp.nitems && t >= gp.tile_end[it]) ++it;
    if (it > 0) t -= gp.tile_end[it - 1];
    const TnParams& p = gp.item[it];
    const int nt2 = p.N2 / 128;
    const int mbeg = split * p.rows_per_split;
    const int mend = min(p.M, mbeg + p.rows_per_split);
    if (mbeg >= mend) return;
    if ((mend - mbeg) % TK == 0) tn_tile_dma(p, (t / nt2) * 128, (t % nt2) * 128, mbeg, mend, smem);
    else tn_tile<bf16>(p, (t / nt2) * 128, (t % nt2) * 128, mbeg, mend, smem);
}

// the same grouping for fp32 operands (rounded to bf16 while staging): the four dW of a temporal-encoder layer, M = a few
// hundred rows, where the launch count rather than the arithmetic is what costs
template <bool OWNED, int NP = 128>
__global__ __launch_bounds__(256) void gemm_tn_grouped_f32_kernel(TnGroup gp) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TTILE];
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int split = wg / gp.ntiles;
    int t = wg - split * gp.ntiles, it = 0;
    while (it + 1 < gp.nitems && t >= gp.tile_end[it]) ++it;
    if (it > 0) t -= gp.tile_end[it - 1];
    const TnParams& p = gp.item[it];
    const int nt2 = p.N2 / 128;
    const int mbeg = split * p.rows_per_split;
    const int mend = min(p.M, mbeg + p.rows_per_split);
    if (mbeg >= mend) return;
    tn_tile<float, OWNED, NP>(p, (t / nt2) * NP, (t % nt2) * 128, mbeg, mend, smem);
}

// Wide variant of the grouped dW kernel: 128 (P columns) x 384 (Q columns) output tile per 512-thread workgroup
// (8 waves as 2 x 4, 64 x 96 per wave), used when every item has N2 % 384 == 0 (all four dW of a ViT block do).
// The 128x128 kernel above is paced by its global->LDS fill stream (ablation in LABNOTES.md 4.1: 2.8 GB of fills per
// launch, DMA-only 223 us vs 166 us of MFMA work); this tile needs a third fewer fill bytes per flop: 64 KiB per
// 64-row step (P 16 KiB + three 128-column blocks of Q) for 2 x 128 x 384 x 64 flop.  Two 64-KiB stages = 128 KiB of
// LDS, one workgroup per CU; 36 tiles x 7 M-splits = 252 workgroups fill the 256 CUs in one round.
constexpr int WBLK = 64 * 256;                 // one 64-row x 128-column block, 16 KiB
constexpr int WSTAGE = 4 * WBLK;               // P block + 3 Q blocks

struct TnWideGroup : TnGroup {};                 // the same items and prefix sums, in 128 x 384 tiles

// The wide dW kernel: 128 x 384 tile, 8 waves (2 x 4 of 64 x 96), global -> VGPR -> LDS staging (a plain vector load does
// not hold the wave the way an LDS-DMA issue does) with two tiles in flight in registers (a first-touch row slab comes
// from HBM, and one step is not enough to cover that latency), transposed fragment reads.
// Ping-pong schedule.  Round 1's version had all eight waves read fragments together, run their 48 MFMAs
// together and meet at one barrier per step, so the MFMA pipe of a SIMD idled while both of its waves were in the LDS
// phase (PMC: MFMA busy 39 %).  Here a step is four barrier intervals per wave,
//     R0: fragments of k-half 0 + first half of the next tile's LDS writes / global loads
//     M0: 24 MFMAs          R1: fragments of k-half 1 + second half of the writes / loads          M1: 24 MFMAs
// and the waves 4-7 (the SIMD partners of 0-3) run ONE INTERVAL BEHIND (one extra barrier before the loop, the other
// group takes it after): in every interval one wave of each SIMD owns the MFMA pipe while its partner is in the LDS.
// Hazards (intervals numbered globally; group A's step s is 4s..4s+3, group B's 4s+1..4s+4): tile s+1 is written into
// buffer (s+1)&1 during 4s..4s+3 and first read in 4s+4; the old contents (tile s-1) were last read in 4s-2 (A) and
// 4s-1 (B), and every R interval ends with lgkmcnt(0) BEFORE its barrier, so those reads have returned.
// (212 -> 197 us per block inside the step.  Measured and dropped on this kernel: one bias MFMA per wave instead of four
// on the wc = 0 waves, hand-counted vmcnt(12) instead of the compiler's vmcnt(7..4): no change either way — the kernel
// is paced by the global fill stream, LABNOTES.md 4.2.)
// SLAB (round 5): instead of 96 fp32 atomicAdd instructions per wave at the very end (7 M-splits x 7.1 MB = 49.8 MB of
// atomics that all 252 workgroups issue at the same moment; the chip retires ~1.3 TB/s of them), every workgroup stores its
// raw 128 x 384 partial tile ONCE, in register order (16 B per lane, 1 KiB per wave-instruction), into the slab of its split;
// tn_slab_finish_kernel sums the splits in a fixed order and adds the result to dW / db: deterministic gradients.
// NI (round 5, opt-in SAIS_TN_NI=2): barrier intervals per 64-row step.  4 = the schedule above.  2 = one LDS interval (the
// fragments of BOTH k-halves, the whole next tile's LDS writes, the loads of the tile after it) and one interval of 48 MFMAs per
// step: half the barriers — the bare MFMA + barrier skeleton of the 4-interval form already takes 130 of the kernel's 198 us —
// paid for with 80 instead of 40 fragment registers, which leaves room for ONE staging register set (a tile is requested one
// step before its LDS write instead of two).
template <bool SLAB, int NI = 4>
__global__ __launch_bounds__(512) void gemm_tn_pp_kernel(TnWideGroup gp, float* slabs) {
    extern __shared__ __attribute__((aligned(16))) char wsmem[];          // 2 x WSTAGE
    CLK_STAMP(3);
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int split = wg / gp.ntiles;
    int t = wg - split * gp.ntiles, it0 = 0;
    while (it0 + 1 < gp.nitems && t >= gp.tile_end[it0]) ++it0;
    if (it0 > 0) t -= gp.tile_end[it0 - 1];
    const TnParams& p = gp.item[it0];
    const int nt2 = p.N2 / WQ;
    const int n1_0 = (t / nt2) * 128, n2_0 = (t % nt2) * WQ;
    const int mbeg = split * p.rows_per_split;
    const int mend = min(p.M, mbeg + p.rows_per_split);
    if (mbeg >= mend) return;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 2, wc = wid & 3, g = lane >> 4, li = lane & 15;
    const int blk = wid >> 1;
    const bf16* src0 = blk == 0 ? (const bf16*)p.P + n1_0 : (const bf16*)p.Q + n2_0 + (blk - 1) * 128;
    const int ld = blk == 0 ? p.ldp : p.ldq;
    const bf16* pbase = src0 + (size_t)(mbeg + 32 * (wid & 1) + (lane >> 4)) * ld + (lane & 15) * 8;
    const int nsteps = (mend - mbeg) / TK;
    u32x4 stg[2][8];
    auto gload4 = [&](int step, u32x4 (&dst)[8], int h) {
        step = step < nsteps ? step : nsteps - 1;
#pragma unroll
        for (int j = 4 * h; j < 4 * h + 4; ++j) dst[j] = *(const u32x4*)(pbase + (size_t)(step * TK + 4 * j) * ld);
    };
    auto lwrite4 = [&](int stage, const u32x4 (&src)[8], int h) {
        char* s = wsmem + stage * WSTAGE + blk * WBLK;
#pragma unroll
        for (int j = 4 * h; j < 4 * h + 4; ++j) {
            const int r = 4 * (8 * (wid & 1) + j) + (lane >> 4), c = lane & 15;
            *(u32x4*)(s + r * 256 + ((((c >> 1) ^ (r & 7)) << 5) | ((c & 1) << 4))) = src[j];
        }
    };
    f32x4 acc[4][6];
    f32x4 accb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        accb[i] = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    }
    const bool do_bias = p.db != nullptr && n2_0 == 0 && wc == 0;
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (bf16)1.0f;
    const int q4 = li >> 2, p4 = li & 3;
    bf16x8 fp[4], fq[6];
    auto frags = [&](int cur, int ks) {
        const char* sp = wsmem + cur * WSTAGE;
        const char* sq = sp + WBLK;
        const int row = ks * 32 + 4 * g + q4;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int cp = wr * 64 + tt * 16 + 4 * p4;
            fp[tt] = cat4(lds_read_tr16(tr_addr(sp, row, cp)), lds_read_tr16(tr_addr(sp, row + 16, cp)));
        }
#pragma unroll
        for (int tt = 0; tt < 6; ++tt) {
            const int c = wc * 96 + tt * 16;
            const char* qb = sq + (c >> 7) * WBLK;
            const int cq = (c & 127) + 4 * p4;
            fq[tt] = cat4(lds_read_tr16(tr_addr(qb, row, cq)), lds_read_tr16(tr_addr(qb, row + 16, cq)));
        }
    };
    auto fence = [&] {                                            // end of an LDS interval
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    auto mma = [&] {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) acc[i][j] = mfma16(fp[i], fq[j], acc[i][j]);
        if (do_bias) {
#pragma unroll
            for (int i = 0; i < 4; ++i) accb[i] = mfma16(fp[i], ones, accb[i]);
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    // one step on buffer `cur`: stg[s] holds tile st+1 (goes to the other buffer), tile st+3 is loaded into it afterwards
    auto step = [&](int cur, int st, u32x4 (&sreg)[8]) {
        frags(cur, 0);
        lwrite4(cur ^ 1, sreg, 0);
        gload4(st + 3, sreg, 0);
        fence();
        mma();
        frags(cur, 1);
        lwrite4(cur ^ 1, sreg, 1);
        gload4(st + 3, sreg, 1);
        fence();
        mma();
    };
    if constexpr (NI == 2) {
        bf16x8 fp2[2][4], fq2[2][6];
        auto frags2 = [&](int cur) {
            const char* sp = wsmem + cur * WSTAGE;
            const char* sq = sp + WBLK;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int row = ks * 32 + 4 * g + q4;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int cp = wr * 64 + tt * 16 + 4 * p4;
                    fp2[ks][tt] = cat4(lds_read_tr16(tr_addr(sp, row, cp)), lds_read_tr16(tr_addr(sp, row + 16, cp)));
                }
#pragma unroll
                for (int tt = 0; tt < 6; ++tt) {
                    const int c = wc * 96 + tt * 16;
                    const char* qb = sq + (c >> 7) * WBLK;
                    const int cq = (c & 127) + 4 * p4;
                    fq2[ks][tt] = cat4(lds_read_tr16(tr_addr(qb, row, cq)), lds_read_tr16(tr_addr(qb, row + 16, cq)));
                }
            }
        };
        auto mma2 = [&] {
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 6; ++j) acc[i][j] = mfma16(fp2[ks][i], fq2[ks][j], acc[i][j]);
                if (do_bias) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) accb[i] = mfma16(fp2[ks][i], ones, accb[i]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        };
        gload4(0, stg[0], 0); gload4(0, stg[0], 1);
        lwrite4(0, stg[0], 0); lwrite4(0, stg[0], 1);
        gload4(1, stg[0], 0); gload4(1, stg[0], 1);
        __syncthreads();
        if (wr == 1) __builtin_amdgcn_s_barrier();                // waves 4-7 run one interval behind
        for (int st = 0; st < nsteps; ++st) {
            const int cur = st & 1;
            frags2(cur);
            lwrite4(cur ^ 1, stg[0], 0); lwrite4(cur ^ 1, stg[0], 1);     // tile st + 1 (a repeat of the last tile at the end)
            gload4(st + 2, stg[0], 0); gload4(st + 2, stg[0], 1);
            fence();
            mma2();
        }
        if (wr == 0) __builtin_amdgcn_s_barrier();
    } else {
    gload4(0, stg[0], 0); gload4(0, stg[0], 1);
    gload4(1, stg[1], 0); gload4(1, stg[1], 1);
    lwrite4(0, stg[0], 0); lwrite4(0, stg[0], 1);
    gload4(2, stg[0], 0); gload4(2, stg[0], 1);
    __syncthreads();
    if (wr == 1) __builtin_amdgcn_s_barrier();                    // waves 4-7 run one interval behind
    for (int st = 0; st < nsteps; st += 2) {
        step(0, st, stg[1]);
        if (st + 1 < nsteps) step(1, st + 1, stg[0]);
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();
    }
    if constexpr (SLAB) {
        const int tg = (wg - split * gp.ntiles), zt = split * gp.ntiles + tg;
        f32x4* o = (f32x4*)slabs + ((size_t)zt * 8 + wid) * (24 * 64) + lane;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) o[(i * 6 + j) * 64] = acc[i][j];
        if (do_bias && li == 0) {
            float* ob = slabs + (size_t)gridDim.x * (8 * 24 * 64 * 4) + (size_t)zt * 128 + wr * 64 + 4 * g;
#pragma unroll
            for (int i = 0; i < 4; ++i) *(f32x4*)(ob + i * 16) = accb[i];
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n1 = n1_0 + wr * 64 + i * 16 + 4 * g + r;
            float* row = p.dW + (size_t)n1 * p.ldw + n2_0 + wc * 96 + li;
#pragma unroll
            for (int j = 0; j < 6; ++j) atomicAdd(row + j * 16, acc[i][j][r]);
            if (do_bias && li == 0) atomicAdd(p.db + n1, accb[i][r]);
        }
}

// One thread per (tile, wave, accumulator tile, lane): the nsplit partial f32x4 of its position are loaded together (up to 16
// loads in flight per thread; round 5's form walked them one dependent load at a time from 288 workgroups and cost more than the
// atomics it replaced), summed in a fixed order and added to dW; the bias parts by the last blocks of the grid.
__global__ __launch_bounds__(256) void tn_slab_finish_kernel(TnWideGroup gp, const float* slabs, int nsplit) {
    constexpr int PER_TILE = 8 * 24 * 64;                                     // f32x4 elements of one workgroup's slab
    const int nbody = gp.ntiles * PER_TILE / 256;
    const size_t zstride = (size_t)gp.ntiles * PER_TILE;                      // f32x4 per split
    if ((int)blockIdx.x < nbody) {
        const int e = blockIdx.x * 256 + threadIdx.x;
        int t = e / PER_TILE;
        const int w8 = e - t * PER_TILE, lane = w8 & 63, ij = (w8 >> 6) % 24, w = (w8 >> 6) / 24;
        const f32x4* src = (const f32x4*)slabs + (size_t)t * PER_TILE + w8;
        f32x4 v[16];
        f32x4 sum = {0.f, 0.f, 0.f, 0.f};
        for (int z0 = 0; z0 < nsplit; z0 += 16) {              // unconditional loads (clamped index), values selected afterwards
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = src[(size_t)min(z0 + u, nsplit - 1) * zstride];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const float keep = z0 + u < nsplit ? 1.f : 0.f;
                sum += v[u] * keep;
            }
        }
        int it0 = 0;
        while (it0 + 1 < gp.nitems && t >= gp.tile_end[it0]) ++it0;
        if (it0 > 0) t -= gp.tile_end[it0 - 1];
        const TnParams& p = gp.item[it0];
        const int nt2 = p.N2 / WQ;
        const int n1_0 = (t / nt2) * 128, n2_0 = (t % nt2) * WQ;
        const int wr = w >> 2, wc = w & 3, i = ij / 6, j = ij - 6 * i, g = lane >> 4, li = lane & 15;
        float* row = p.dW + (size_t)(n1_0 + wr * 64 + i * 16 + 4 * g) * p.ldw + n2_0 + wc * 96 + j * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) row[(size_t)r * p.ldw] += sum[r];
        return;
    }
    const int e = (blockIdx.x - nbody) * 256 + threadIdx.x;
    if (e >= gp.ntiles * 128) return;
    int t = e >> 7;
    const int tg = t, c = e & 127;
    int it0 = 0;
    while (it0 + 1 < gp.nitems && t >= gp.tile_end[it0]) ++it0;
    if (it0 > 0) t -= gp.tile_end[it0 - 1];
    const TnParams& p = gp.item[it0];
    const int nt2 = p.N2 / WQ;
    if (p.db == nullptr || t % nt2 != 0) return;
    const float* bb = slabs + (size_t)nsplit * zstride * 4 + (size_t)tg * 128 + c;
    float sum = 0.f;
    for (int z = 0; z < nsplit; ++z) sum += bb[(size_t)z * gp.ntiles * 128];
    p.db[(t / nt2) * 128 + c] += sum;
}

}  // namespace

// SAIS_TN_XL = 4 | 8 waves (default 4; 8 in experimental builds only), 0 = the 128 x 384 kernel; SAIS_TN_XL_SLABS = 0: fp32 atomics
// instead of slabs + finish; SAIS_TN_SLABS = 1: the round-5 slab form of the 128 x 384 kernel (implies SAIS_TN_XL = 0).  Once per process.
static const TnSwitches& tn_switches() {
    static const bool old_slabs = sais_env_int("SAIS_TN_SLABS", 0) != 0;
    static const int xl = old_slabs ? 0 : sais_env_int("SAIS_TN_XL", 4);
    static const TnSwitches v = {SAIS_EXPERIMENTAL || !xl ? xl : 4, sais_env_int("SAIS_TN_XL_SLABS", 1) != 0, old_slabs};
    return v;
}
CLK_EXPORT(gemm_tn)

// argument check of the grouped launches; align = leading-dimension multiple of the operands (8 for bf16, 4 for fp32; 0: shapes only)
static bool tn_items_ok(const SaisTnItem* items, int nitems, int M, int nsplit, int align) {
    if (!items || nitems <= 0 || nitems > SAIS_TN_MAX_ITEMS || M <= 0 || nsplit <= 0) return false;
    for (int i = 0; i < nitems; ++i) {
        const SaisTnItem& t = items[i];
        if (t.N1 % 128 || t.N2 % 128 || (align && (!t.P || !t.Q || !t.dW || t.ldp % align || t.ldq % align))) return false;
    }
    return true;
}

// items -> the tp x tq tiles of one grouped launch
template <class Group>
static Group tn_group(const SaisTnItem* items, int nitems, int M, int rows, int tp, int tq) {
    Group gp; gp.nitems = nitems; gp.ntiles = 0;
    for (int i = 0; i < nitems; ++i) {
        const SaisTnItem& t = items[i];
        gp.item[i] = TnParams{t.P, t.Q, t.ldp, t.ldq, M, t.N1, t.N2, t.dW, t.ldw, t.db, rows};
        gp.tile_end[i] = gp.ntiles += (t.N1 / tp) * (t.N2 / tq);
    }
    return gp;
}

static int launch_tn(const void* P, int ldp, const void* Q, int ldq, int M, int N1, int N2, float* dW, int ldw,
                     float* db, int nsplit, void* stream, bool f32) {
    if (!P || !Q || !dW || M <= 0 || N1 % 128 || N2 % 128 || ldp % 8 || ldq % 8 || nsplit <= 0) return SAIS_ERR_ARG;
    const TnSplit sp = tn_split(M, nsplit);
    TnParams p{P, Q, ldp, ldq, M, N1, N2, dW, ldw, db, sp.rows};
    dim3 grid((N2 / 128) * (N1 / 128) * sp.ns);
    if (f32) hipLaunchKernelGGL(gemm_tn_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(gemm_tn_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, p);
    return sais_check_launch();
}

extern "C" size_t sais_gemm_tn_grouped_slab_bytes(const SaisTnItem* items, int nitems, int M) {
    if (!items || nitems <= 0 || nitems > SAIS_TN_MAX_ITEMS || M <= 0) return 0;
    return tn_plan(items, nitems, M, 1, TN_ANY_SLABS, tn_switches()).slab_bytes;
}

// The plan of a launch without making it (no GPU; not in the ABI): of sais_gemm_tn_grouped_f32 (f32 != 0), else of _ws for an offer of bytes
// (< 0: no slabs).  out = TnForm, tiles, M-splits, rows per split, workgroups, slab bytes used.  SAIS_ERR_ARG: refused shapes, offer too small
extern "C" int sais_gemm_tn_plan_(const SaisTnItem* items, int nitems, int M, int nsplit, int64_t slab_bytes_offered, int f32,
                                  int64_t out[6]) {
    if (!tn_items_ok(items, nitems, M, nsplit, 0) || !out) return SAIS_ERR_ARG;
    const TnPlan pl = f32 ? tn_plan_f32(items, nitems, M, nsplit)
                          : tn_plan(items, nitems, M, nsplit, slab_bytes_offered < 0 ? TN_NO_SLABS : slab_bytes_offered, tn_switches());
    const int64_t v[6] = {pl.form, pl.tiles, pl.nsplit, pl.rows, pl.workgroups, (int64_t)pl.slab_bytes};
    for (int i = 0; i < 6; ++i) out[i] = v[i];
    return pl.short_offer ? SAIS_ERR_ARG : SAIS_OK;
}

extern "C" int sais_gemm_tn_grouped(const SaisTnItem* items, int nitems, int M, int nsplit, void* stream) {
    return sais_gemm_tn_grouped_ws(items, nitems, M, nsplit, nullptr, 0, stream);
}

extern "C" int sais_gemm_tn_grouped_ws(const SaisTnItem* items, int nitems, int M, int nsplit, void* slabs, size_t slab_bytes,
                                       void* stream) {
    SAIS_ENTER();
    if (!tn_items_ok(items, nitems, M, nsplit, 8)) return SAIS_ERR_ARG;
    const int64_t offer = !slabs ? TN_NO_SLABS : slab_bytes > (size_t)INT64_MAX ? INT64_MAX : (int64_t)slab_bytes;
    const TnPlan pl = tn_plan(items, nitems, M, nsplit, offer, tn_switches());
    if (pl.short_offer || (pl.slab_bytes && ((uintptr_t)slabs & 15))) return SAIS_ERR_ARG;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(pl.workgroups);
    switch (pl.form) {
        case TN_XL_SLAB: case TN_XL_ATOMIC:
            return sais_tn_xl_launch(pl, items, nitems, M, tn_switches().xl_waves, pl.form == TN_XL_SLAB ? (float*)slabs : nullptr, stream);
        case TN_WIDE_SLAB: case TN_WIDE_ATOMIC: {
            const TnWideGroup wg = tn_group<TnWideGroup>(items, nitems, M, pl.rows, 128, WQ);
            if (!sais_dyn_lds_once<gemm_tn_pp_kernel<false>>(2 * WSTAGE) || !sais_dyn_lds_once<gemm_tn_pp_kernel<true>>(2 * WSTAGE))
                return SAIS_ERR_LAUNCH;
#if SAIS_EXPERIMENTAL
            static const int tn_ni = sais_env_int("SAIS_TN_NI", 4);
            if (tn_ni == 2 && pl.form == TN_WIDE_ATOMIC) {
                if (!sais_dyn_lds_once<gemm_tn_pp_kernel<false, 2>>(2 * WSTAGE)) return SAIS_ERR_LAUNCH;
                hipLaunchKernelGGL((gemm_tn_pp_kernel<false, 2>), grid, dim3(512), 2 * WSTAGE, st, wg, (float*)nullptr);
                break;
            }
#endif
            // the slab form is opt-in (SAIS_TN_SLABS=1): bit-reproducible weight gradients.  Measured SLOWER than the atomics (LABNOTES
            // R5.1: 254 vs 240 us stand-alone, 12.86 vs 12.76 ms per step) — the atomic tail this was built to remove is not there.
            if (pl.form == TN_WIDE_SLAB) {
                hipLaunchKernelGGL(gemm_tn_pp_kernel<true>, grid, dim3(512), 2 * WSTAGE, st, wg, (float*)slabs);
                hipLaunchKernelGGL(tn_slab_finish_kernel, dim3(pl.tiles * (8 * 24 * 64) / 256 + (pl.tiles * 128 + 255) / 256), dim3(256), 0, st, wg, (const float*)slabs, pl.nsplit);
            } else hipLaunchKernelGGL(gemm_tn_pp_kernel<false>, grid, dim3(512), 2 * WSTAGE, st, wg, (float*)nullptr);
            break;
        }
        default: {
            const TnGroup gp = tn_group<TnGroup>(items, nitems, M, pl.rows, 128, 128);
            hipLaunchKernelGGL(gemm_tn_grouped_kernel, grid, dim3(256), 0, st, gp);
        }
    }
    return sais_check_launch();
}

extern "C" int sais_gemm_tn_grouped_f32(const SaisTnItem* items, int nitems, int M, int nsplit, void* stream) {
    SAIS_ENTER();
    if (!tn_items_ok(items, nitems, M, nsplit, 4)) return SAIS_ERR_ARG;
    const TnPlan pl = tn_plan_f32(items, nitems, M, nsplit);
    const dim3 grid(pl.workgroups); const hipStream_t st = (hipStream_t)stream;
    const TnGroup gp = tn_group<TnGroup>(items, nitems, M, pl.rows, pl.form == TN_F32_OWNER64 ? 64 : 128, 128);
    if (pl.form == TN_F32_OWNER64) hipLaunchKernelGGL((gemm_tn_grouped_f32_kernel<true, 64>), grid, dim3(256), 0, st, gp);
    else if (pl.form == TN_F32_OWNER128) hipLaunchKernelGGL(gemm_tn_grouped_f32_kernel<true>, grid, dim3(256), 0, st, gp);
    else hipLaunchKernelGGL(gemm_tn_grouped_f32_kernel<false>, grid, dim3(256), 0, st, gp);
    return sais_check_launch();
}

extern "C" int sais_gemm_tn_f32(const void* P, int ldp, const void* Q, int ldq, int M, int N1, int N2,
                                float* dW, int ldw, float* db, int nsplit, void* stream) {
    SAIS_ENTER();
    return launch_tn(P, ldp, Q, ldq, M, N1, N2, dW, ldw, db, nsplit, stream, true);
}

extern "C" int sais_gemm_tn(const void* P, int ldp, const void* Q, int ldq, int M, int N1, int N2,
                            float* dW, int ldw, float* db, int nsplit, void* stream) {
    SAIS_ENTER();
    return launch_tn(P, ldp, Q, ldq, M, N1, N2, dW, ldw, db, nsplit, stream, false);
}
