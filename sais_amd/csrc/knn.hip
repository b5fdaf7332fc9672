// Weighted k-NN evaluation of frozen features (dino-main/eval_knn.py:143-182) without the [Nq, Nt] similarity matrix:
//   sais_knn_search  the kmax nearest train rows of every test row by dot product, in the bf16x3 arithmetic of
//                    sais_gemm_nt_f32 (hi.lo + lo.hi + hi.hi per 32-deep MFMA step, fp32 accumulate, same K order for every
//                    (test row, train row) pair wherever it falls: duplicate train rows get bit-equal values)
//   sais_knn_vote    votes[c] = sum over the first k neighbours with label c of expf(val / T) for up to 8 values of k in one
//                    pass over the neighbour list, and the five best classes of each
// Search: a workgroup owns 128 test rows and one contiguous range of 128-row train tiles (a "split").  Per train tile the
// 128 x 128 similarity tile is accumulated as in gemm_nt_f32.hip, parked in the LDS the operand tiles used, and every wave
// scans 32 of its rows: columns above the row's running threshold (its kmax-th best so far) are appended in column order
// to the row's candidate buffer in the workspace; a buffer that could overflow at the next tile is sorted and cut to kmax,
// which also raises the threshold.  Order everywhere is (value descending, train index ascending); tiles stream in index
// order, so a later column that only EQUALS the threshold loses the tie and the strict compare is exact.  A second launch
// merges the splits.  No atomics: results are bit-reproducible.
#include "f32x3_tile.hpp"
#include "../../include/sais_hip.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;           // the stage of f32x3_tile.hpp
constexpr int PAD_IDX = 0x40000000;            // candidate-buffer padding: value -inf, index PAD_IDX + position
constexpr int TARGET_WGS = 256;                // splits are added until rows x splits reaches one workgroup per CU
constexpr int MIN_TILES_PER_SPLIT = 4, MAX_SPLITS = 64;

struct KnnPlan { int row_tiles, ntiles, tiles_per_split, nsplit, cap; };

inline int knn_cap(int kmax) { return kmax + BN <= 256 ? 256 : 512; }      // room for kmax kept + one full tile

inline KnnPlan knn_plan(int Nq, int Nt, int kmax) {
    KnnPlan p;
    p.row_tiles = (Nq + BM - 1) / BM;
    p.ntiles = (Nt + BN - 1) / BN;
    int want = TARGET_WGS / p.row_tiles, lim = p.ntiles / MIN_TILES_PER_SPLIT;
    want = want < lim ? want : lim;
    want = want > MAX_SPLITS ? MAX_SPLITS : (want < 1 ? 1 : want);
    p.tiles_per_split = (p.ntiles + want - 1) / want;
    p.nsplit = (p.ntiles + p.tiles_per_split - 1) / p.tiles_per_split;
    p.cap = knn_cap(kmax);
    return p;
}

// candidate (row, split) buffers: bounded independently of the launch's actual split count, monotone in Nq
inline size_t knn_ws_entries(int Nq, int Nt) {
    const int ntiles = (Nt + BN - 1) / BN;
    int lim = ntiles / MIN_TILES_PER_SPLIT;
    lim = lim > MAX_SPLITS ? MAX_SPLITS : (lim < 1 ? 1 : lim);
    size_t a = (size_t)Nq * lim, b = (size_t)BM * TARGET_WGS;
    a = a < b ? a : b;
    return a > (size_t)Nq ? a : (size_t)Nq;
}

struct Cand { float v; int i; };

// bitonic sort of 64 R entries held as entry e = 64 r + lane, best first
template <int R>
DEVINL void wave_sort(float (&v)[R], int (&x)[R], int lane) {
#pragma unroll
    for (int k = 2; k <= 64 * R; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j < 64) {
                const bool lower = (lane & j) == 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float ov = __shfl_xor(v[r], j);
                    const int ox = __shfl_xor(x[r], j);
                    const bool up = ((64 * r + lane) & k) == 0;
                    const bool ob = before(ov, ox, v[r], x[r]);
                    if ((lower == up) ? ob : !ob) { v[r] = ov; x[r] = ox; }
                }
            } else {
                const int jr = j >> 6;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (r & jr) continue;
                    const int r2 = r | jr;
                    const bool up = ((64 * r) & k) == 0;
                    if (before(v[r2], x[r2], v[r], x[r]) == up) {
                        const float tv = v[r]; v[r] = v[r2]; v[r2] = tv;
                        const int tx = x[r]; x[r] = x[r2]; x[r2] = tx;
                    }
                }
            }
        }
    }
}

template <int R>
DEVINL float entry_value(const float (&v)[R], int e) {          // value of entry e, in every lane
    float t = v[0];
#pragma unroll
    for (int r = 1; r < R; ++r) t = (e >> 6) == r ? v[r] : t;
    return __shfl(t, e & 63);
}

// sort the first cnt entries of buf, keep the best kmax in place; returns the kmax-th value (-inf if cnt < kmax)
template <int R>
DEVINL float prune(Cand* buf, int cnt, int kmax, int lane) {
    float v[R];
    int x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = 64 * r + lane;
        const Cand c = e < cnt ? buf[e] : Cand{-INFINITY, PAD_IDX + e};
        v[r] = c.v; x[r] = c.i;
    }
    wave_sort<R>(v, x, lane);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = 64 * r + lane;
        if (e < kmax) buf[e] = Cand{v[r], x[r]};
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // other lanes of this wave read these entries back later
    return entry_value<R>(v, kmax - 1);
}

struct KnnSearchParams {
    const float* test;            // f32 [Nq, D]
    const float* train;           // f32 [Nt, D]                       (SPLIT == false)
    const bf16* train3;           // bf16 [Nt, 3 D] = [hi | lo | hi]   (SPLIT == true: sais_split_bf16x3, b_side)
    int Nq, Nt, D, kmax, tiles_per_split, cap;
    Cand* cand;                   // [nsplit][Nq][cap]
};

// physical byte offset of S[row][col] in the parked similarity tile: 512-B rows, 16-B chunk index XOR (row & 31)
DEVINL int s_off(int row, int col) { return row * 512 + ((((col >> 2) ^ (row & 31))) << 4) + ((col & 3) << 2); }

template <bool SPLIT, int R>
__global__ __launch_bounds__(256) void knn_search_kernel(KnnSearchParams p) {
    __shared__ __attribute__((aligned(16))) char smem[F32X3_LDS_BYTES];      // A_hi | A_lo | B_hi | B_lo, then the f32 tile
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, g = lane >> 4, li = lane & 15;
    const int m0 = blockIdx.x * BM, split = blockIdx.y;
    const int tile0 = split * p.tiles_per_split;
    const int ntiles_all = (p.Nt + BN - 1) / BN;
    const int ntile = min(p.tiles_per_split, ntiles_all - tile0);
    const int nk = p.D / BK;
    const int sc = tid & 7, sr = tid >> 3;
    // lane l < 32 of wave w keeps the state of row 32 w + l
    float thr_l = -INFINITY;
    int cnt_l = 0;

    f32x4 ra[4][2], rb[4][2];
    u32x4 qh[4], ql[4];
    auto gload = [&](int step) {
        const int t = step / nk, k0 = (step - t * nk) * BK;
        const int n0 = (tile0 + t) * BN;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = sr + 32 * i, m = m0 + r;
            const bool ok = m < p.Nq;
            const float* pa = p.test + (size_t)(ok ? m : 0) * p.D + k0 + sc * 8;
            ra[i][0] = ok ? *(const f32x4*)pa : f32x4{0, 0, 0, 0};
            ra[i][1] = ok ? *(const f32x4*)(pa + 4) : f32x4{0, 0, 0, 0};
            const int n = min(n0 + r, p.Nt - 1);                 // rows past the end repeat the last one; the scan drops them
            if constexpr (SPLIT) {
                const bf16* pb = p.train3 + (size_t)n * 3 * p.D + k0 + sc * 8;
                qh[i] = *(const u32x4*)pb;
                ql[i] = *(const u32x4*)(pb + p.D);
            } else {
                const float* pb = p.train + (size_t)n * p.D + k0 + sc * 8;
                rb[i][0] = *(const f32x4*)pb;
                rb[i][1] = *(const f32x4*)(pb + 4);
            }
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            u32x4 hi, lo;
            if constexpr (SPLIT) { hi = qh[i]; lo = ql[i]; } else split8(rb[i][0], rb[i][1], hi, lo);
            f32x3_store_row(smem, sr + 32 * i, sc, ra[i][0], ra[i][1], hi, lo);
        }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

    const int nstep = ntile * nk;
    gload(0);
    for (int step = 0, kt = 0, t = 0; step < nstep; ++step) {
        __syncthreads();                       // previous operand tile / parked similarity tile fully consumed
        lstore();
        __syncthreads();
        if (step + 1 < nstep) gload(step + 1);
        // own copy of f32x3_kstep (f32x3_tile.hpp): same fragments, same MFMA order
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int oa = swz(wr * 64 + u * 16 + li, ks * 4 + g), ob = swz(wc * 64 + u * 16 + li, ks * 4 + g);
                ah[u] = *(const bf16x8*)(smem + oa);
                al[u] = *(const bf16x8*)(smem + F32X3_IMG_BYTES + oa);
                bh[u] = *(const bf16x8*)(smem + 2 * F32X3_IMG_BYTES + ob);
                bl[u] = *(const bf16x8*)(smem + 3 * F32X3_IMG_BYTES + ob);
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
        if (++kt < nk) continue;
        kt = 0;
        // ---- the similarity tile of train tile t is complete: park it, then scan it row by row
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                *(f32x4*)(smem + s_off(wr * 64 + mt * 16 + li, wc * 64 + 16 * g + 4 * nt)) = acc[mt][nt];
                acc[mt][nt] = f32x4{0, 0, 0, 0};
            }
        __syncthreads();
        const int n0 = (tile0 + t) * BN;
        const bool last = t + 1 == ntile;
        const unsigned long long below = (1ull << lane) - 1;
        for (int rr = 0; rr < 32; ++rr) {
            const int row = wid * 32 + rr, m = m0 + row;
            if (m >= p.Nq) break;                              // wave-uniform
            Cand* buf = p.cand + ((size_t)split * p.Nq + m) * p.cap;
            float thr = __shfl(thr_l, rr);
            int cnt = __shfl(cnt_l, rr);
            const float v0 = *(const float*)(smem + s_off(row, lane)), v1 = *(const float*)(smem + s_off(row, 64 + lane));
            const bool p0 = n0 + lane < p.Nt && v0 > thr, p1 = n0 + 64 + lane < p.Nt && v1 > thr;
            const unsigned long long b0 = __ballot(p0), b1 = __ballot(p1);
            if (b0 | b1) {
                const int c0 = __popcll(b0);
                if (p0) buf[cnt + __popcll(b0 & below)] = Cand{v0, n0 + lane};
                if (p1) buf[cnt + c0 + __popcll(b1 & below)] = Cand{v1, n0 + 64 + lane};
                cnt += c0 + __popcll(b1);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            }
            // keep room for a whole tile; get a threshold as soon as kmax candidates exist; leave the buffer sorted at the end
            if (cnt > p.cap - BN || (cnt >= p.kmax && thr == -INFINITY) || last) {
                thr = prune<R>(buf, cnt, p.kmax, lane);
                cnt = min(cnt, p.kmax);
            }
            if (lane == rr) { thr_l = thr; cnt_l = cnt; }
        }
        ++t;
    }
    // entries past the split's own candidates, for the merge: padding
    for (int rr = 0; rr < 32; ++rr) {
        const int m = m0 + wid * 32 + rr;
        if (m >= p.Nq) break;
        const int cnt = __shfl(cnt_l, rr);
        Cand* buf = p.cand + ((size_t)split * p.Nq + m) * p.cap;
        for (int e = cnt + lane; e < p.kmax; e += 64) buf[e] = Cand{-INFINITY, PAD_IDX + e};
    }
}

// one wave per test row: fold the splits' sorted kmax-lists into one (512-entry sorts: kept list | next split's list)
__global__ __launch_bounds__(64) void knn_merge_kernel(const Cand* cand, int Nq, int nsplit, int cap, int kmax, float* val, int* idx) {
    const int m = blockIdx.x, lane = threadIdx.x;
    float v[8];
    int x[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int e = 64 * r + lane;
        const Cand c = e < kmax ? cand[(size_t)m * cap + e] : Cand{-INFINITY, PAD_IDX + e};
        v[r] = c.v; x[r] = c.i;
    }
    for (int s = 1; s < nsplit; ++s) {
        const Cand* src = cand + ((size_t)s * Nq + m) * cap;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int e = 64 * r + lane;
            if (r < 4) {
                if (e >= kmax) { v[r] = -INFINITY; x[r] = PAD_IDX + e; }
            } else {
                const Cand c = e - 256 < kmax ? src[e - 256] : Cand{-INFINITY, 0};
                v[r] = c.v; x[r] = c.i;
            }
            if (x[r] >= PAD_IDX || x[r] < 0 || v[r] == -INFINITY) { v[r] = -INFINITY; x[r] = PAD_IDX + e; }     // distinct padding keys
        }
        wave_sort<8>(v, x, lane);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = 64 * r + lane;
        if (e < kmax) {
            val[(size_t)m * kmax + e] = v[r];
            idx[(size_t)m * kmax + e] = x[r] >= PAD_IDX ? -1 : x[r];
        }
    }
}

struct KnnVoteParams {
    const float* val; const int* idx; const int* labels;
    int Nq, Nt, kmax, num_classes, m;
    int ks[8];
    float T;
    int* pred; float* votes;
};

// one wave per test row.  The neighbour loop is serial (fp32 accumulation in neighbour order); lane l owns the classes = l mod 64
__global__ __launch_bounds__(64) void knn_vote_kernel(KnnVoteParams p) {
    __shared__ float votes[4096];
    __shared__ float sw[256];
    __shared__ int sl[256];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int C = p.num_classes, klast = p.ks[p.m - 1];
    for (int c = lane; c < C; c += 64) votes[c] = 0.f;
    for (int j = lane; j < klast; j += 64) {
        const int i = p.idx[(size_t)row * p.kmax + j];
        const bool ok = i >= 0 && i < p.Nt;
        const int l = ok ? p.labels[i] : -1;
        sl[j] = l >= 0 && l < C ? l : -1;
        sw[j] = expf(p.val[(size_t)row * p.kmax + j] / p.T);
    }
    __syncthreads();
    int j = 0;
    for (int t = 0; t < p.m; ++t) {
        for (; j < p.ks[t]; ++j) {
            const int l = sl[j];
            if (l >= 0 && (l & 63) == lane) votes[l] += sw[j];
        }
        __syncthreads();
        if (p.votes) {
            float* o = p.votes + ((size_t)t * p.Nq + row) * C;
            for (int c = lane; c < C; c += 64) o[c] = votes[c];
        }
        wave_best5(votes, C, lane, p.pred + ((size_t)t * p.Nq + row) * 5);      // by (vote descending, class ascending)
        __syncthreads();
    }
}

}  // namespace

extern "C" size_t sais_knn_workspace_bytes(int Nq, int Nt, int kmax) {
    if (Nq <= 0 || Nt <= 0 || kmax < 1 || kmax > SAIS_KNN_MAX_K || kmax > Nt) return 0;
    return knn_ws_entries(Nq, Nt) * knn_cap(kmax) * sizeof(Cand);
}

extern "C" int sais_knn_search(const float* test, const void* train, int train_is_split, int Nq, int Nt, int D, int kmax,
                               float* val, int* idx, void* workspace, size_t workspace_bytes, void* stream) {
    SAIS_ENTER();
    if (!test || !train || !val || !idx || !workspace) return SAIS_ERR_ARG;
    if (Nq <= 0 || Nt <= 0 || kmax < 1 || kmax > SAIS_KNN_MAX_K || kmax > Nt) return SAIS_ERR_ARG;
    if (D <= 0 || D % BK || D > SAIS_KNN_MAX_DIM || Nt >= PAD_IDX) return SAIS_ERR_ARG;
    if (workspace_bytes < sais_knn_workspace_bytes(Nq, Nt, kmax)) return SAIS_ERR_ARG;
    const KnnPlan pl = knn_plan(Nq, Nt, kmax);
    if ((size_t)pl.nsplit * Nq > knn_ws_entries(Nq, Nt)) return SAIS_ERR_ARG;
    KnnSearchParams p{test, train_is_split ? nullptr : (const float*)train, train_is_split ? (const bf16*)train : nullptr,
                      Nq, Nt, D, kmax, pl.tiles_per_split, pl.cap, (Cand*)workspace};
    const dim3 grid(pl.row_tiles, pl.nsplit);
    hipStream_t s = (hipStream_t)stream;
    if (pl.cap == 256) {
        if (train_is_split) hipLaunchKernelGGL((knn_search_kernel<true, 4>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((knn_search_kernel<false, 4>), grid, dim3(256), 0, s, p);
    } else {
        if (train_is_split) hipLaunchKernelGGL((knn_search_kernel<true, 8>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((knn_search_kernel<false, 8>), grid, dim3(256), 0, s, p);
    }
    hipLaunchKernelGGL(knn_merge_kernel, dim3(Nq), dim3(64), 0, s, (const Cand*)workspace, Nq, pl.nsplit, pl.cap, kmax, val, idx);
    return sais_check_launch();
}

extern "C" int sais_knn_vote(const float* val, const int* idx, int Nq, int kmax, const int* train_labels, int Nt, int num_classes,
                             float T, const int* ks, int m, int* pred, float* votes, void* stream) {
    SAIS_ENTER();
    if (!val || !idx || !train_labels || !ks || !pred) return SAIS_ERR_ARG;
    if (Nq <= 0 || Nt <= 0 || kmax < 1 || kmax > SAIS_KNN_MAX_K || num_classes < 1 || num_classes > SAIS_KNN_MAX_CLASSES) return SAIS_ERR_ARG;
    if (m < 1 || m > SAIS_KNN_MAX_KS || !(T > 0.f)) return SAIS_ERR_ARG;
    KnnVoteParams p{val, idx, train_labels, Nq, Nt, kmax, num_classes, m, {0, 0, 0, 0, 0, 0, 0, 0}, T, pred, votes};
    for (int t = 0; t < m; ++t) {
        if (ks[t] < 1 || ks[t] > kmax || (t && ks[t] <= ks[t - 1])) return SAIS_ERR_ARG;
        p.ks[t] = ks[t];
    }
    hipLaunchKernelGGL(knn_vote_kernel, dim3(Nq), dim3(64), 0, (hipStream_t)stream, p);
    return sais_check_launch();
}
