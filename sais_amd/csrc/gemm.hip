// bf16 MFMA NT GEMM for the SAIS hot path (gfx950).
//
//  sais_gemm_nt : C[M,N] = A[M,K] . B[N,K]^T  (+ fused epilogue)  — every nn.Linear forward
//                 (vision_transformer.py:59-65,80-92; prepare_model.py:74-81,416) and, fed with the
//                 pre-transposed weight, every dX = dY . W.
//  (fp32 operands: gemm_nt_f32.hip; weight / bias gradients: gemm_tn.hip; rejected forms of the kernels here: gemm_nt_exp.hip)
//
// Tiling: 128x128 output tile per 256-thread workgroup (4 waves as 2x2, 64x64 per wave = 4x4 MFMA
// 16x16x32 tiles, 64 fp32 accumulator VGPRs), BK = 64, two LDS stages (64 KiB), one barrier per K-step,
// global->register->LDS staging issued before the MFMAs of the current step.
// LDS image: 128-B rows, 16-B chunk index XOR (row & 7)  -> conflict-free ds_read_b128 fragment reads.
// Operands are swapped in the MFMA (weights as "A", activations as "B") and weight rows are permuted
// while staging so that every lane ends up with 16 CONTIGUOUS output columns of one output row:
// epilogue stores are 32-B (bf16) / 64-B (fp32) per lane, a full 128-B line per row per wave.
#include "gemm_nt_tile.hpp"

namespace {

// Staging is LDS-DMA (global_load_lds_dwordx4: no VGPR round trip, no ds_write): one wave-instruction fills
// 1 KiB = 8 LDS rows of 128 B linearly, so the XOR swizzle (and the weight-row permutation) is applied to the
// per-lane SOURCE address: LDS slot (row r, position c') receives global chunk c' ^ (r & 7).
template <int EPI>
__global__ __launch_bounds__(256) void gemm_nt_kernel(NtParams p) {
    __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1, g = lane >> 4, li = lane & 15;
    const int ntn = p.N / BN;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int n0 = (tile % ntn) * BN, m0 = (tile / ntn) * BM;

    // wave w issues pieces 4w..4w+3 of each operand tile; piece q = LDS rows 8q..8q+7
    const int sub = lane >> 3, spos = lane & 7, schunk = spos ^ sub;
    const bf16* asrc[4]; const bf16* bsrc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 8 * (4 * wid + j) + sub;
        int m = m0 + r;
        m = m < p.M ? m : p.M - 1;                                   // clamp: rows >= M are never stored
        asrc[j] = p.A + (size_t)m * p.lda + schunk * 8;
        bsrc[j] = p.B + (size_t)(n0 + perm_row(r)) * p.ldb + schunk * 8;
    }
    auto issue = [&](int stage, int k0) {
        char* s = smem + stage * 2 * TILE_BYTES + (4 * wid) * 1024;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            glds16(asrc[j] + k0, s + j * 1024);
            glds16(bsrc[j] + k0, s + TILE_BYTES + j * 1024);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

    int nk = p.K / BK, kbase = 0;
    if constexpr (EPI == SAIS_EPI_RAW_SLABS_F32) {                   // split-K: slice blockIdx.y of the K range
        const int per = (nk + (int)gridDim.y - 1) / (int)gridDim.y;
        kbase = blockIdx.y * per;
        nk = min(per, nk - kbase);
        if (nk <= 0) nk = 0;
    }
    if (nk > 0) issue(0, kbase * BK);
    __syncthreads();
    // the epilogue's own loads (bias, residual / pre-activation rows: first-touch HBM data) are issued before the MFMAs
    // of the LAST K-step, so their latency runs under that step instead of in front of the stores
    float bias[16];
    EpiAux aux;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) issue(cur ^ 1, (kbase + kt + 1) * BK);
        const char* sa = smem + cur * 2 * TILE_BYTES;
        const char* sb = sa + TILE_BYTES;
        if constexpr (EPI != SAIS_EPI_RAW_SLABS_F32)
            if (kt == nk - 1) epilogue_loads<EPI>(p, m0 + wr * 64, li, n0 + wc * 64 + 16 * g, bias, aux);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fa[4], fb[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                fa[t] = *(const bf16x8*)(sa + swz(wr * 64 + t * 16 + li, ks * 4 + g));
                fb[t] = *(const bf16x8*)(sb + swz(wc * 64 + t * 16 + li, ks * 4 + g));
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = mfma16(fb[nt], fa[mt], acc[mt][nt]);
        }
        __syncthreads();                      // drains this wave's LDS-DMA (vmcnt(0)) and fences the buffer swap
    }

    // lane holds, for row m = m0 + wr*64 + mt*16 + li, columns n0 + wc*64 + 16 g + (4 nt + r)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        int m = m0 + wr * 64 + mt * 16 + li;
        if (m >= p.M) continue;
        float v[16];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[4 * nt + r] = acc[mt][nt][r];
        if constexpr (EPI == SAIS_EPI_RAW_SLABS_F32) {
            float* o = (float*)p.out + ((size_t)blockIdx.y * p.M + m) * p.ldo + n0 + wc * 64 + 16 * g;
#pragma unroll
            for (int i = 0; i < 4; ++i) *(f32x4*)(o + 4 * i) = f32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
        } else {
            epilogue<EPI>(p, m, n0 + wc * 64 + 16 * g, v, bias, aux, mt);
        }
    }
}

// y = sum_z slabs[z] + bias; y *= rowscale[m]; y += aux; -> f32 and / or bf16 (fixed summation order: deterministic)
__global__ __launch_bounds__(256) void splitk_finish_kernel(const float* ws, int ks, int M, int N, int lds, const float* bias,
                                                            const float* rowscale, const float* aux, int ldaux, float* out32,
                                                            int ldo32, bf16* out16, int ldo16) {
    const int n4 = N >> 2;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < (long)M * n4; i += (long)gridDim.x * 256) {
        const int m = (int)(i / n4), n = (int)(i - (long)m * n4) * 4;
        f32x4 y = *(const f32x4*)(ws + (size_t)m * lds + n);
        for (int z = 1; z < ks; ++z) y += *(const f32x4*)(ws + ((size_t)z * M + m) * lds + n);
        if (bias) y += *(const f32x4*)(bias + n);
        if (rowscale) y *= rowscale[m];
        if (aux) y += *(const f32x4*)(aux + (size_t)m * ldaux + n);
        if (out32) *(f32x4*)(out32 + (size_t)m * ldo32 + n) = y;
        if (out16) {
            bf16x4 o;
            o[0] = (bf16)y[0]; o[1] = (bf16)y[1]; o[2] = (bf16)y[2]; o[3] = (bf16)y[3];
            *(bf16x4*)(out16 + (size_t)m * ldo16 + n) = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Persistent form of the eight-wave kernel: a workgroup walks tiles b, b + G, ... and issues the first LDS-DMA loads of
// its NEXT tile (A'(0), W'(0), A'(1)) before the epilogue of the current one, so the per-tile prologue (the first
// K-tile's round trip, ~19 % of a K = 384 tile) runs under the epilogue's arithmetic and stores.  vmcnt is in-order
// and counts stores: the wait that follows the epilogue allows exactly the stores it issued (+ the two A'(1) pieces)
// to stay outstanding, which is only known for full tiles, so a ragged tile waits for everything.
// SAIS_NT_STAMP (debug builds only, tools/nt_stamp.py): lane 0 of every wave of workgroup 0 records the shader clock at the
// phase boundaries of its THIRD tile; sais_debug_nt_stamps() copies the table out.
#ifdef SAIS_NT_STAMP
__device__ unsigned long long g_nt_stamps[8][16];
#define NTSTAMP(i) do { if (blockIdx.x == 0 && titer == 2 && lane == 0) g_nt_stamps[wid][i] = __builtin_readcyclecounter(); } while (0)
#else
#define NTSTAMP(i) do { } while (0)
#endif
// SAIS_NT_ABL (timing ablations, results are WRONG when set; LABNOTES R4.4): 1 no K loop (no operand loads, no MFMAs),
// 2 no epilogue (no epilogue loads, arithmetic, stores), 4 / 8 role split — even / odd workgroups (4) or the lower / upper
// 256 workgroups (8) run ONLY the K loops resp. ONLY the epilogues of their tiles: do the two phases overlap on a CU at all?
#ifndef SAIS_NT_ABL
#define SAIS_NT_ABL 0
#endif
template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_nt_w8p_kernel(NtParams p, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // A ring: 3 x 16 KiB, then W: 2 x 16 KiB
    CLK_STAMP(EPI == SAIS_EPI_BIAS_GELU_GRAD_BF16 ? 1 : EPI == SAIS_EPI_MUL_BF16 ? 2 : 0);
    [[maybe_unused]] const int abl_role = (SAIS_NT_ABL & 4) ? (blockIdx.x & 1) : (SAIS_NT_ABL & 8) ? ((blockIdx.x >> 8) & 1) : -1;
    const bool do_k = !(SAIS_NT_ABL & 1) && abl_role != 1, do_e = !(SAIS_NT_ABL & 2) && abl_role != 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 2, wc = wid & 3, g = lane >> 4, li = lane & 15;
    const int ntn = p.N / BN;
    const int sub = lane >> 3, spos = lane & 7, schunk = spos ^ sub;
    const bf16* asrc[2]; const bf16* bsrc[2];
    auto set_tile = [&](int v, int& m0, int& n0) {
        const int tile = xcd_remap(v, ntiles);
        n0 = (tile % ntn) * BN; m0 = (tile / ntn) * BM;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = 8 * (2 * wid + j) + sub;
            int m = m0 + r;
            m = m < p.M ? m : p.M - 1;                               // clamp: rows >= M are never stored
            asrc[j] = p.A + (size_t)m * p.lda + schunk * 8;
            bsrc[j] = p.B + (size_t)(n0 + perm_row32(r)) * p.ldb + schunk * 8;
        }
    };
    char* const sW = smem + 3 * TILE_BYTES;
    auto issue_a = [&](int kt) {
        char* s = smem + (kt % 3) * TILE_BYTES + (2 * wid) * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(asrc[j] + kt * BK, s + j * 1024);
    };
    auto issue_w = [&](int kt) {
        char* s = sW + (kt & 1) * TILE_BYTES + (2 * wid) * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(bsrc[j] + kt * BK, s + j * 1024);
    };
    const int nk = p.K / BK;
    // store instructions one wave issues in a full tile's epilogue
    constexpr int SROW = (EPI == SAIS_EPI_BIAS_F32) ? 2 : (EPI == SAIS_EPI_BIAS_RESID_F32) ? 2 : (EPI == SAIS_EPI_PATCH_F32) ? 2
                       : (EPI == SAIS_EPI_BIAS_GELU_GRAD_BF16 || EPI == SAIS_EPI_BIAS_GELU_GRADQ_BF16) ? 2 : 1;
    const int nstores = 4 * (SROW + ((EPI == SAIS_EPI_BIAS_RESID_F32 || EPI == SAIS_EPI_BIAS_GELU_BF16) && p.out2 ? 1 : 0));

    // A-operand prefetch into L2 (K = 384, N >= 1024).  The ntn column tiles of a row tile run side by side on one XCD and
    // all of them wait for the same first-touch fetch of the A rows; once the epilogues of the other CUs keep HBM busy
    // with writes that fetch takes several microseconds, far more than the two K-steps of lead the LDS ring gives
    // (measured: the GELU + GELU' GEMM takes 145 us, 123 us with an L2-resident A).  So while a workgroup is in the
    // epilogue of tile i, wave 0 touches its 1/ntn share of the cache lines of tile i+1's A rows that the in-loop loads
    // would only ask for later (k >= 128: lines 2-5 of every 768-B row; lines 0-1 are being fetched by A'(0), A'(1)):
    // one global_load_dword, 44-60 active lanes, result never used.  It is the youngest load at the tile switch (one
    // more allowed in that wait) and is retired by the counted wait of K-step 0.  fc1 + GELU' 129 -> 124 us, qkv 68.5 ->
    // 66.5 us inside the step.  (Prefetching two tiles ahead is no better; the same trick on the bf16 aux tile of the
    // MUL epilogue is WORSE, 128 vs 118 us: that operand is bandwidth, not latency.)
    const bool do_pf = nk == 6 && ntn >= 8 && ntn <= 16 && wid == 0;
    unsigned pf_keep = 0;
    auto prefetch_a = [&](int pm0, int tcol) {
        const int per = (BM + ntn - 1) / ntn;                      // rows per sharing workgroup
        const int row = tcol * per + (lane >> 2);
        if ((lane >> 2) < per && row < BM) {
            int m = pm0 + row;
            m = m < p.M ? m : p.M - 1;
            const bf16* q = p.A + (size_t)m * p.lda + (2 + (lane & 3)) * 64;
            asm volatile("global_load_dword %0, %1, off" : "=v"(pf_keep) : "v"(q) : "memory");
        }
    };
    int v = blockIdx.x, m0, n0;
    if (v >= ntiles) return;
    set_tile(v, m0, n0);
    if (do_k) {
        issue_a(0);
        issue_w(0);
        if (nk > 1) issue_a(1);
    }
    if (nk > 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    [[maybe_unused]] int titer = -1;
    for (;;) {
        ++titer;
        NTSTAMP(0);
        f32x4 acc[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
        float bias[8];
        EpiAux8 aux;
        // The barrier-paced K loop outranks the epilogue of the OTHER workgroup on this CU (round 3): the two share the SIMDs'
        // issue ports, and at equal priority the epilogue's VALU stream (GELU: ~19 slots per element) delays the waves the
        // whole workgroup waits for at the next barrier.  fc1 + GELU' 124 -> 117-120 us, dX fc2 114 -> 108-112, qkv 67 -> 63-65
        // on two boxes; priorities 1, 2 and 3 measure the same.
        __builtin_amdgcn_s_setprio(2);
        for (int kt = 0; kt < (do_k ? nk : 0); ++kt) {
            if (kt + 1 < nk) issue_w(kt + 1);
            if (kt + 2 < nk) issue_a(kt + 2);
            const char* sa = smem + (kt % 3) * TILE_BYTES;
            const char* sb = sW + (kt & 1) * TILE_BYTES;
            if (kt == nk - 1 && do_e) epilogue_loads8<EPI>(p, m0 + wr * 64, li, n0 + wc * 32 + 8 * g, bias, aux);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 fa[4], fb[2];
#pragma unroll
                for (int t = 0; t < 4; ++t) fa[t] = *(const bf16x8*)(sa + swz(wr * 64 + t * 16 + li, ks * 4 + g));
#pragma unroll
                for (int t = 0; t < 2; ++t) fb[t] = *(const bf16x8*)(sb + swz(wc * 32 + t * 16 + li, ks * 4 + g));
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = mfma16(fb[nt], fa[mt], acc[mt][nt]);
            }
            if (kt + 2 < nk) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
            else if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // last step: only the epilogue's loads are out
            NTSTAMP(1 + 2 * kt);                                         // MFMAs issued, operands of the next step awaited
            __builtin_amdgcn_s_barrier();
            NTSTAMP(2 + 2 * kt);
        }
        __builtin_amdgcn_s_setprio(0);
        // the next tile's first loads go out before this tile's epilogue
        const int cm0 = m0, cn0 = n0;
        const int nv = v + gridDim.x;
        const bool more = nv < ntiles;
        asm volatile("" ::"v"(pf_keep));                               // the previous prefetch has been retired by now
        if (more) {
            set_tile(nv, m0, n0);
            if (do_k) {
                issue_a(0);
                issue_w(0);
                if (nk > 1) issue_a(1);
                if (do_pf) prefetch_a(m0, xcd_remap(nv, ntiles) % ntn);
            }
        }
        if (SAIS_NT_ABL) {
            if (!do_k) epilogue_loads8<EPI>(p, cm0 + wr * 64, li, cn0 + wc * 32 + 8 * g, bias, aux);
            if (!do_e) {                                               // keep the MFMAs alive
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) asm volatile("" ::"v"(acc[mt][nt]));
            }
        }
#pragma unroll
        for (int mt = 0; mt < (do_e ? 4 : 0); ++mt) {
            const int m = cm0 + wr * 64 + mt * 16 + li;
            if (m >= p.M) continue;
            float vv[8];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) vv[4 * nt + r] = acc[mt][nt][r];
            epilogue8<EPI>(p, m, cn0 + wc * 32 + 8 * g, vv, bias, aux, mt);
        }
        NTSTAMP(13);                                                     // epilogue arithmetic done, stores issued
        if (!more) break;
        v = nv;
        // A'(0) and W'(0) must have landed; the two A'(1) pieces and this epilogue's stores may stay in flight
        const int allow = (cm0 + BM <= p.M && nk > 1) ? nstores + 2 + (do_pf ? 1 : 0) : 0;
        if (allow == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else if (allow == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
        else if (allow == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else if (allow == 11) asm volatile("s_waitcnt vmcnt(11)" ::: "memory");
        else if (allow == 14) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
        else if (allow == 15) asm volatile("s_waitcnt vmcnt(15)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        NTSTAMP(14);                                                     // the next tile's first operands have landed
        __builtin_amdgcn_s_barrier();
        NTSTAMP(15);
    }
}

#ifdef SAIS_NT_STAMP
extern "C" int sais_debug_nt_stamps(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_nt_stamps), sizeof(unsigned long long) * 8 * 16) == hipSuccess ? 0 : -2;
}
#endif

}  // namespace

extern "C" int sais_gemm_nt_row_(const SaisGemm* g, void* stream);      // gemm_row.hip: row-owning tiles, N = 384
extern "C" int sais_gemm_nt_exp_(const SaisGemm* g, int nt_grid, void* stream);   // gemm_nt_exp.hip: 0 = not taken, > 0 = launched
CLK_EXPORT(gemm)

// one epilogue's launch: the persistent eight-wave kernel on nt_grid workgroups (big) or the four-wave kernel, a tile per workgroup
template <int E>
static int launch_nt(const NtParams& p, dim3 grid, bool big, int nt_grid, hipStream_t stream) {
    if (big) {
        if (!sais_dyn_lds_once<gemm_nt_w8p_kernel<E>>(5 * TILE_BYTES)) return SAIS_ERR_LAUNCH;
        const int nt = (int)grid.x;
        hipLaunchKernelGGL(gemm_nt_w8p_kernel<E>, dim3(nt < nt_grid ? nt : nt_grid), dim3(512), 5 * TILE_BYTES, stream, p, nt);
    } else {
        hipLaunchKernelGGL(gemm_nt_kernel<E>, grid, dim3(256), 0, stream, p);
    }
    return sais_check_launch();
}
#define NT_CASE(E) case E: return launch_nt<E>(p, grid, big, nt_grid, (hipStream_t)stream);

extern "C" int sais_gemm_nt(const SaisGemm* g, void* stream) {
    SAIS_ENTER();
    if (!g || !g->A || !g->B || !g->out) return SAIS_ERR_ARG;
    if (g->M <= 0 || g->N % BN || g->K % BK || g->lda % 8 || g->ldb % 8 || g->ldo % 8) return SAIS_ERR_ARG;
    if ((g->epilogue == SAIS_EPI_BIAS_GELU_GRAD_BF16 || g->epilogue == SAIS_EPI_BIAS_GELU_GRADQ_BF16) && !g->out2) return SAIS_ERR_ARG;
    if (g->epilogue == SAIS_EPI_BIAS_GELU_GRADQ_BF16 && (g->ldo2 % 16 || ((uintptr_t)g->out2 & 15))) return SAIS_ERR_ARG;
    if (g->epilogue == SAIS_EPI_MULQ_BF16 && (!g->aux || g->ldaux % 16 || ((uintptr_t)g->aux & 15))) return SAIS_ERR_ARG;
    if ((g->epilogue == SAIS_EPI_MUL_BF16 || g->epilogue == SAIS_EPI_DGELU_BF16 || g->epilogue == SAIS_EPI_DRELU_BF16 ||
         g->epilogue == SAIS_EPI_BIAS_RESID_F32) && !g->aux)
        return SAIS_ERR_ARG;
    const NtParams p = nt_params(g);
    if (g->rowscale && g->epilogue != SAIS_EPI_BIAS_RESID_F32) return SAIS_ERR_ARG;
    const dim3 grid = nt_tiles(g);
    // Two kernels, chosen by M alone: the four-wave 128x128 kernel for small M (inference batches, tests, the
    // patch-embed epilogue) and the persistent eight-wave A-ring kernel for the ViT GEMMs of a training step
    // (M >= 8192).  Round 1's other variants (wave-specialised, register-stationary, non-persistent eight-wave,
    // four-wave A-ring) were measured slower inside the step and are gone from the library (LABNOTES.md 4.1).
    const bool big = g->M >= 8192;
    // persistent workgroups of the eight-wave kernel (2 per CU); SAIS_NT_GRID=256 = one per CU (diagnostic: LABNOTES R5.2)
    static const int nt_grid_env = sais_env_int("SAIS_NT_GRID", 0);
    const int nt_grid = nt_grid_env > 0 ? nt_grid_env : 512;
    if (g->epilogue == SAIS_EPI_RAW_SLABS_F32) {                // split-K over grp_in slices: small M only, raw fp32 slabs
        if (big || g->grp_in < 1 || g->grp_in > g->K / BK || g->ldo % 4) return SAIS_ERR_ARG;
        hipLaunchKernelGGL(gemm_nt_kernel<SAIS_EPI_RAW_SLABS_F32>, dim3(grid.x, g->grp_in), dim3(256), 0, (hipStream_t)stream, p);
        return sais_check_launch();
    }
    // the plain N = 384 GEMMs of a training step (dX of proj, the last block's fc2): balanced row tiles of gemm_row.hip
    if (big && g->N == 384 && (g->epilogue == SAIS_EPI_BIAS_BF16 || (g->epilogue == SAIS_EPI_BIAS_RESID_F32 && !g->out2)))
        return sais_gemm_nt_row_(g, stream);
    if (big && g->rowscale) return SAIS_ERR_ARG;               // the eight-wave kernel has no row-scale epilogue
#if SAIS_EXPERIMENTAL
    if (big)
        if (const int r = sais_gemm_nt_exp_(g, nt_grid, stream)) return r > 0 ? SAIS_OK : r;
#endif
    switch (g->epilogue) {
        NT_EPILOGUES(NT_CASE)
        default: return SAIS_ERR_ARG;
    }
#undef NT_CASE
}

extern "C" int sais_splitk_finish(const float* slabs, int nslabs, int M, int N, int lds, const float* bias,
                                  const float* rowscale, const float* aux, int ldaux, float* out32, int ldo32, void* out16,
                                  int ldo16, void* stream) {
    SAIS_ENTER();
    if (!slabs || nslabs < 1 || M <= 0 || N <= 0 || N % 4 || lds % 4 || (!out32 && !out16)) return SAIS_ERR_ARG;
    if ((aux && ldaux % 4) || (out32 && ldo32 % 4) || (out16 && ldo16 % 4)) return SAIS_ERR_ARG;
    const long n = (long)M * (N / 4);
    const int grid = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(splitk_finish_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, slabs, nslabs, M, N, lds, bias,
                       rowscale, aux, ldaux, out32, ldo32, (bf16*)out16, ldo16);
    return sais_check_launch();
}
