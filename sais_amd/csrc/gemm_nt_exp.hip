// EXPERIMENT RECORDS (built only with -DSAIS_EXPERIMENTAL=1: tools/build_variant.sh exp -DSAIS_EXPERIMENTAL=1).
// Three other organisations of the persistent K = 384 GEMM of gemm.hip, each correct, each measured slower than gemm_nt_w8p_kernel
// (LABNOTES R5.1, R5.2, R5.6).  The default library does not contain them; the switches SAIS_NT_W8R / _W16 / _W4 are then ignored.
#include "gemm_nt_tile.hpp"
#if SAIS_EXPERIMENTAL

namespace {

// ---------------------------------------------------------------------------------------------
// W in registers (round 5, LABNOTES R5.6; K = 384 only, the K loop fully unrolled).  The stamps of R5.2 show a K-step of
// gemm.hip's w8p kernel taking 1 200-1 700 cycles of a wave's time for 256 cycles of its MFMAs: W(kt + 1) is requested at the top of step
// kt and awaited at its end (two-slot W ring: one exposed L2 round trip of LDS-DMA per step), and a third W slot does not fit two
// workgroups per CU.  Here W does not pass through LDS at all: a wave loads the MFMA fragments of ITS 32 weight columns
// straight from global memory (L2-resident: 16-B per lane, four loads per step) TWO steps ahead into a rotating triple of register
// sets (+ 32 VGPRs), and the 80 KiB of LDS become a five-slot A ring with four steps of lead.  Per step and wave: 2 LDS-DMA issues
// instead of 4, 8 fragment reads instead of 12, no W to publish at the barrier.  vmcnt is one in-order counter, so the issue
// order inside a step is W first, then A, and the counted wait at the end of step kt leaves exactly A(kt + 3), W(kt + 2), A(kt + 4)
// in flight.
template <int EPI>
__global__ __launch_bounds__(512, 4) void gemm_nt_w8r_kernel(NtParams p, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // A ring: 5 x 16 KiB
    constexpr int NK = 6, NA = 5;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 2, wc = wid & 3, g = lane >> 4, li = lane & 15;
    const int ntn = p.N / BN;
    const int sub = lane >> 3, spos = lane & 7, schunk = spos ^ sub;
    const bf16* asrc[2]; const bf16* wsrc[2];
    auto set_tile = [&](int v, int& m0, int& n0) {
        const int tile = xcd_remap(v, ntiles);
        n0 = (tile % ntn) * BN; m0 = (tile / ntn) * BM;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = 8 * (2 * wid + j) + sub;
            int m = m0 + r;
            m = m < p.M ? m : p.M - 1;
            asrc[j] = p.A + (size_t)m * p.lda + schunk * 8;
            // fragment tile j of this wave's 32 columns: MFMA row li <-> weight row 8 (li >> 2) + 4 j + (li & 3) (perm_row32: a
            // lane then owns 8 contiguous output columns), k = 8 g .. 8 g + 7 of a 32-deep half-step
            wsrc[j] = p.B + (size_t)(n0 + wc * 32 + 8 * (li >> 2) + 4 * j + (li & 3)) * p.ldb + 8 * g;
        }
    };
    auto issue_a = [&](int kt) {
        char* s = smem + (kt % NA) * TILE_BYTES + (2 * wid) * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(asrc[j] + kt * BK, s + j * 1024);
    };
    bf16x8 wf[3][2][2];                                               // [set][k-half][column tile]
    // The W loads are inline asm: the compiler's own s_waitcnt insertion does not see the counted waits below and put vmcnt(0)
    // in front of the MFMAs of steps 0 and 3 (first version: 201 instead of 141 us).  Invisible to it, they are ordered by hand:
    // every counted wait names the register set it makes valid as an in / out operand, so no MFMA that reads the set can be
    // scheduled above the wait.
    auto load_w = [&](int kt, bf16x8 (&dst)[2][2]) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst[ks][nt]) : "v"(wsrc[nt] + kt * BK + ks * 32) : "memory");
    };
#define W8R_WAIT(N, SET) asm volatile("s_waitcnt vmcnt(" #N ") lgkmcnt(0)"                                                 \
                                      : "+v"(wf[SET][0][0]), "+v"(wf[SET][0][1]), "+v"(wf[SET][1][0]), "+v"(wf[SET][1][1]) :: "memory")
    constexpr int SROW = (EPI == SAIS_EPI_BIAS_F32) ? 2 : (EPI == SAIS_EPI_BIAS_RESID_F32) ? 2 : (EPI == SAIS_EPI_PATCH_F32) ? 2
                       : (EPI == SAIS_EPI_BIAS_GELU_GRAD_BF16 || EPI == SAIS_EPI_BIAS_GELU_GRADQ_BF16) ? 2 : 1;
    const int nstores = 4 * (SROW + ((EPI == SAIS_EPI_BIAS_RESID_F32 || EPI == SAIS_EPI_BIAS_GELU_BF16) && p.out2 ? 1 : 0));
    auto prologue = [&] {                                             // W(0), A(0), W(1), A(1), A(2), A(3): the order the waits count on
        load_w(0, wf[0]);
        issue_a(0);
        load_w(1, wf[1]);
        issue_a(1);
        issue_a(2);
        issue_a(3);
        __builtin_amdgcn_sched_barrier(0);
    };
    int v = blockIdx.x, m0, n0;
    if (v >= ntiles) return;
    set_tile(v, m0, n0);
    prologue();
    W8R_WAIT(10, 0);                                                  // W(0) and A(0) are in; W(1), A(1..3) may be in flight
    __builtin_amdgcn_s_barrier();
    int carry = 0;                           // stores of the previous tile's epilogue that may still be in flight at step 0
    for (;;) {
        f32x4 acc[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
        float bias[8];
        EpiAux8 aux;
        __builtin_amdgcn_s_setprio(2);
#pragma unroll
        for (int kt = 0; kt < NK; ++kt) {
            if (kt + 2 < NK) load_w(kt + 2, wf[(kt + 2) % 3]);
            if (kt + 4 < NK) issue_a(kt + 4);
            __builtin_amdgcn_sched_barrier(0);
            const char* sa = smem + (kt % NA) * TILE_BYTES;
            if (kt == NK - 1) epilogue_loads8<EPI>(p, m0 + wr * 64, li, n0 + wc * 32 + 8 * g, bias, aux);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 fa[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) fa[t] = *(const bf16x8*)(sa + swz(wr * 64 + t * 16 + li, ks * 4 + g));
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = mfma16(wf[kt % 3][ks][nt], fa[mt], acc[mt][nt]);
            }
            // in flight after this point (oldest first): [kt = 0: A(2), A(3), the previous tile's stores] W(kt+2), A(kt+4) and,
            // before them, A(kt+3) — everything older, i.e. W(kt+1) and A(kt+1), has to be in
            if (kt == 0) {                                            // makes W(1) = set 1 valid
                const int allow = 10 + carry;
                if (allow == 10) W8R_WAIT(10, 1);
                else if (allow == 14) W8R_WAIT(14, 1);
                else if (allow == 18) W8R_WAIT(18, 1);
                else W8R_WAIT(4, 1);
            } else if (kt == 1) W8R_WAIT(8, 2);
            else if (kt == 2) W8R_WAIT(6, 0);
            else if (kt == 3) W8R_WAIT(4, 1);
            else if (kt == 4) W8R_WAIT(0, 2);
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // last step: only the epilogue's loads are out
            __builtin_amdgcn_s_barrier();
        }
        __builtin_amdgcn_s_setprio(0);
        const int cm0 = m0, cn0 = n0;
        const int nv = v + gridDim.x;
        const bool more = nv < ntiles;
        if (more) {
            set_tile(nv, m0, n0);
            prologue();
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int m = cm0 + wr * 64 + mt * 16 + li;
            if (m >= p.M) continue;
            float vv[8];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) vv[4 * nt + r] = acc[mt][nt][r];
            epilogue8<EPI>(p, m, cn0 + wc * 32 + 8 * g, vv, bias, aux, mt);
        }
        if (!more) break;
        v = nv;
        // W'(0) and A'(0) must be in; W'(1), A'(1..3) and this epilogue's stores may stay in flight (a ragged tile issues fewer
        // stores than counted: wait for everything)
        const int allow = (cm0 + BM <= p.M) ? nstores + 10 : 0;
        carry = allow ? nstores : 0;
        if (allow == 14) W8R_WAIT(14, 0);                             // makes W'(0) = set 0 valid
        else if (allow == 18) W8R_WAIT(18, 0);
        else { W8R_WAIT(0, 0); carry = 0; }
        __builtin_amdgcn_s_barrier();
    }
#undef W8R_WAIT
}

// ---------------------------------------------------------------------------------------------
// Two eight-wave groups of ONE 1024-thread workgroup in ENFORCED anti-phase (round 5, LABNOTES R5.2).  Measured on gemm_nt_w8p_kernel
// of gemm.hip (SAIS_NT_GRID, SAIS_NT_ABL builds): K loops alone 62.5 us with two workgroups per CU and 81 us with one, epilogues alone
// 58 us (HBM-bound) either way, the whole kernel 141 us = MORE than their sum — the two workgroups of a CU run the same program
// from the same start, so both are in their K loops together (each slowed by the other) and in their epilogues together (the
// store path and HBM saturated, the matrix pipe idle), and a tile's first-touch A rows are fetched while every CU writes.
// Here the two tile pipelines of a CU are two wave groups of one workgroup that share every s_barrier: group 0 runs the nk
// K-steps of its tile while group 1 runs the epilogue of ITS previous tile in nk slices (one 16-row sub-tile per interval,
// then idle intervals), and vice versa.  At any moment eight waves feed the matrix pipe and eight drain to HBM, the next
// tile's first operands are requested a whole half-period ahead, and HBM sees a steady write stream.
// Same tile, LDS image (2 x 80 KiB), epilogues and registers as the eight-wave kernel.  Needs nk >= 5.
#ifdef SAIS_NT_STAMP
__device__ unsigned long long g_nt16_stamps[16][36];
#endif
template <int EPI>
__global__ __launch_bounds__(1024) void gemm_nt_w16_kernel(NtParams p, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem_all[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w16 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = w16 >> 3, wid = w16 & 7;
    char* const smem = smem_all + grp * (5 * TILE_BYTES);            // this group's A ring (3 x 16 KiB) + W ring (2 x 16 KiB)
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
            m = m < p.M ? m : p.M - 1;
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
    constexpr int SROW = (EPI == SAIS_EPI_BIAS_F32) ? 2 : (EPI == SAIS_EPI_BIAS_RESID_F32) ? 2 : (EPI == SAIS_EPI_PATCH_F32) ? 2
                       : (EPI == SAIS_EPI_BIAS_GELU_GRAD_BF16 || EPI == SAIS_EPI_BIAS_GELU_GRADQ_BF16) ? 2 : 1;
    const int nstores = 4 * (SROW + ((EPI == SAIS_EPI_BIAS_RESID_F32 || EPI == SAIS_EPI_BIAS_GELU_BF16) && p.out2 ? 1 : 0));
    // virtual workgroup ids: group 0 = blockIdx.x, group 1 = blockIdx.x + gridDim.x (same XCD); both walk with stride 2 G
    const int G2 = 2 * (int)gridDim.x;
    auto count = [&](int v0) { return v0 < ntiles ? (ntiles - v0 + G2 - 1) / G2 : 0; };
    const int nA = count(blockIdx.x), nB = count(blockIdx.x + gridDim.x);
    const int mine = grp ? nB : nA;
    const int totA = 2 * nk * nA, totB = nB ? nk + 2 * nk * nB : 0;
    const int total = totA > totB ? totA : totB;                     // barriers every wave of the workgroup takes
    int done = 0;
#ifdef SAIS_NT_STAMP
    // lane 0 of every wave of workgroup 0 stamps the shader clock BEFORE and AFTER each of 18 consecutive barriers (from the
    // 24th on: both groups are in steady state): arrival and release times of every interval (tools/nt16_stamp.py)
    auto bar = [&] {
        const int k = done - 24;
        if (blockIdx.x == 0 && lane == 0 && k >= 0 && k < 18) g_nt16_stamps[w16][2 * k] = __builtin_readcyclecounter();
        __builtin_amdgcn_s_barrier();
        if (blockIdx.x == 0 && lane == 0 && k >= 0 && k < 18) g_nt16_stamps[w16][2 * k + 1] = __builtin_readcyclecounter();
        ++done;
    };
#else
    auto bar = [&] { __builtin_amdgcn_s_barrier(); ++done; };
#endif
    int v = blockIdx.x + grp * gridDim.x, m0 = 0, n0 = 0;
    if (mine > 0) {
        set_tile(v, m0, n0);
        issue_a(0);
        issue_w(0);
        issue_a(1);
    }
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (grp == 1 && mine > 0)
        for (int i = 0; i < nk; ++i) bar();                          // group 1 runs half a period behind
    for (int t = 0; t < mine; ++t) {
        f32x4 acc[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
        float bias[8];
        EpiAux8 aux;
        __builtin_amdgcn_s_setprio(2);
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 1 < nk) issue_w(kt + 1);
            if (kt + 2 < nk) issue_a(kt + 2);
            const char* sa = smem + (kt % 3) * TILE_BYTES;
            const char* sb = sW + (kt & 1) * TILE_BYTES;
            if (kt == nk - 1) epilogue_loads8<EPI>(p, m0 + wr * 64, li, n0 + wc * 32 + 8 * g, bias, aux);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 fa[4], fb[2];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) fa[tt] = *(const bf16x8*)(sa + swz(wr * 64 + tt * 16 + li, ks * 4 + g));
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) fb[tt] = *(const bf16x8*)(sb + swz(wc * 32 + tt * 16 + li, ks * 4 + g));
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = mfma16(fb[nt], fa[mt], acc[mt][nt]);
            }
            if (kt + 2 < nk) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
            else if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // last step: only the epilogue's loads are out
            bar();
        }
        __builtin_amdgcn_s_setprio(0);
        // epilogue phase = nk intervals beside the OTHER group's K loop.  The next tile's first operands go out first: they
        // have the whole phase to arrive.
        const int cm0 = m0, cn0 = n0;
        const bool more = t + 1 < mine;
        if (more) {
            v += G2;
            set_tile(v, m0, n0);
            issue_a(0);
            issue_w(0);
            issue_a(1);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int m = cm0 + wr * 64 + mt * 16 + li;
            if (m < p.M) {
                float vv[8];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) vv[4 * nt + r] = acc[mt][nt][r];
                epilogue8<EPI>(p, m, cn0 + wc * 32 + 8 * g, vv, bias, aux, mt);
            }
            bar();
        }
        for (int i = 4; i < nk - 1; ++i) bar();
        // A'(0) and W'(0) must have landed before the phase's last barrier; the two A'(1) pieces and this epilogue's stores may
        // stay in flight (vmcnt is in-order: they are younger)
        const int allow = (more && cm0 + BM <= p.M) ? nstores + 2 : 0;
        if (allow == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else if (allow == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else if (allow == 14) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bar();
    }
    while (done < total) bar();
}

// ---------------------------------------------------------------------------------------------
// Four workgroups per CU (round 5).  LABNOTES R4.4: a workgroup of gemm.hip's eight-wave kernel is a latency CHAIN (K loop ->
// epilogue -> K loop; neither phase is slowed by what the CU's other workgroup does), so the launch takes tiles-per-workgroup x
// chain length and what shortens it is more chains per CU.  Same 128 x 128 tile, same fill bytes per flop, but FOUR waves of
// 64 x 64 (16 MFMAs per wave between barriers, as before; 8 instead of 12 fragment reads for them) and K in steps of 32:
// 8-KiB stages, A ring of three + W ring of two = 40 KiB per workgroup, <= 128 VGPRs -> four workgroups = four chains per CU,
// and no two waves of a workgroup share a SIMD (the barrier skew of the eight-wave form was the SIMD sibling).
// LDS image: 64-B rows; the 16-B chunk c of row r sits at position c ^ qmap(r), which makes the ds_read_b128 fragment reads
// conflict-free for the hardware's lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... (MI355X_MICROARCH.md, LDS).
constexpr int QK = 32;
constexpr int QTILE = 128 * QK * 2;              // 8 KiB per operand per stage
DEVINL int qmap(int r) { const int q = (r >> 2) & 3; return (((q ^ (q >> 1)) & 1) << 1) | (q >> 1); }
DEVINL int swz64(int row, int chunk) { return row * 64 + ((chunk ^ qmap(row)) << 4); }

template <int EPI>
__global__ __launch_bounds__(256, 4) void gemm_nt_w4q_kernel(NtParams p, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // A ring: 3 x 8 KiB, then W: 2 x 8 KiB
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1, g = lane >> 4, li = lane & 15;
    const int ntn = p.N / BN;
    const int srow = lane >> 2, spos = lane & 3;
    const bf16* asrc[2]; const bf16* bsrc[2];
    auto set_tile = [&](int v, int& m0, int& n0) {
        const int tile = xcd_remap(v, ntiles);
        n0 = (tile % ntn) * BN; m0 = (tile / ntn) * BM;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = 16 * (2 * wid + j) + srow;
            const int c = spos ^ qmap(r);
            int m = m0 + r;
            m = m < p.M ? m : p.M - 1;
            asrc[j] = p.A + (size_t)m * p.lda + c * 8;
            bsrc[j] = p.B + (size_t)(n0 + perm_row(r)) * p.ldb + c * 8;
        }
    };
    char* const sW = smem + 3 * QTILE;
    auto issue_a = [&](int kt) {
        char* s = smem + (kt % 3) * QTILE + (2 * wid) * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(asrc[j] + kt * QK, s + j * 1024);
    };
    auto issue_w = [&](int kt) {
        char* s = sW + (kt & 1) * QTILE + (2 * wid) * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(bsrc[j] + kt * QK, s + j * 1024);
    };
    const int nk = p.K / QK;
    constexpr bool LATE = EPI == SAIS_EPI_MUL_BF16 || EPI == SAIS_EPI_DGELU_BF16 || EPI == SAIS_EPI_DRELU_BF16;
    [[maybe_unused]] const int tk = nk >= 4 ? nk - 4 : 0;
    [[maybe_unused]] unsigned pf_keep = 0;
    constexpr int SROW = (EPI == SAIS_EPI_BIAS_F32 || EPI == SAIS_EPI_BIAS_RESID_F32 || EPI == SAIS_EPI_PATCH_F32) ? 4
                       : (EPI == SAIS_EPI_BIAS_GELU_GRAD_BF16) ? 4 : 2;
    const int nstores = 4 * (SROW + ((EPI == SAIS_EPI_BIAS_RESID_F32 || EPI == SAIS_EPI_BIAS_GELU_BF16) && p.out2 ? 2 : 0));
    int v = blockIdx.x, m0, n0;
    if (v >= ntiles) return;
    set_tile(v, m0, n0);
    issue_a(0);
    issue_w(0);
    issue_a(1);
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (;;) {
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
        float bias[16];
        EpiAux aux;
        __builtin_amdgcn_s_setprio(2);
        for (int kt = 0; kt < nk; ++kt) {
            if constexpr (LATE) {
                // the bf16 aux tile of this wave (64 rows x 128 B) is first-touch HBM data and there are no registers to hold
                // it during the K loop (64 accumulators + 32 fragment registers): one discarded dword per row pulls the 64
                // lines into L2 three steps early (retired by this step's counted wait), the real loads follow the loop
                if (kt == tk) {
                    int m = m0 + wr * 64 + lane;
                    m = m < p.M ? m : p.M - 1;
                    const bf16* q = (const bf16*)p.aux + (size_t)m * p.ldaux + n0 + wc * 64;
                    asm volatile("global_load_dword %0, %1, off" : "=v"(pf_keep) : "v"(q) : "memory");
                }
            }
            if (kt + 1 < nk) issue_w(kt + 1);
            if (kt + 2 < nk) issue_a(kt + 2);
            const char* sa = smem + (kt % 3) * QTILE;
            const char* sb = sW + (kt & 1) * QTILE;
            if constexpr (!LATE) {
                if (kt == nk - 1) epilogue_loads<EPI>(p, m0 + wr * 64, li, n0 + wc * 64 + 16 * g, bias, aux);
            }
            bf16x8 fa[4], fb[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                fa[t] = *(const bf16x8*)(sa + swz64(wr * 64 + t * 16 + li, g));
                fb[t] = *(const bf16x8*)(sb + swz64(wc * 64 + t * 16 + li, g));
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = mfma16(fb[nt], fa[mt], acc[mt][nt]);
            if (kt + 2 < nk) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
            else if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // last step: only the epilogue's loads are out
            __builtin_amdgcn_s_barrier();
        }
        __builtin_amdgcn_s_setprio(0);
        const int cm0 = m0, cn0 = n0;
        const int nv = v + gridDim.x;
        const bool more = nv < ntiles;
        if constexpr (LATE) {
            asm volatile("" ::"v"(pf_keep));
            epilogue_loads<EPI>(p, cm0 + wr * 64, li, cn0 + wc * 64 + 16 * g, bias, aux);
        }
        if (more) {
            set_tile(nv, m0, n0);
            issue_a(0);
            issue_w(0);
            issue_a(1);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int m = cm0 + wr * 64 + mt * 16 + li;
            if (m >= p.M) continue;
            float vv[16];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) vv[4 * nt + r] = acc[mt][nt][r];
            epilogue<EPI>(p, m, cn0 + wc * 64 + 16 * g, vv, bias, aux, mt);
        }
        if (!more) break;
        v = nv;
        // A'(0) and W'(0) must have landed; the two A'(1) pieces and this epilogue's stores may stay in flight
        const int allow = (cm0 + BM <= p.M) ? nstores + 2 : 0;
        if (allow == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else if (allow == 18) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
        else if (allow == 26) asm volatile("s_waitcnt vmcnt(26)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
}

#ifdef SAIS_NT_STAMP
extern "C" int sais_debug_nt16_stamps(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_nt16_stamps), sizeof(unsigned long long) * 16 * 36) == hipSuccess ? 0 : -2;
}
#endif

}  // namespace

// epilogues the four-workgroups-per-CU kernel is built for (the fp32-aux ones need 64 more registers than it has)
static constexpr bool w4_epi(int e) {
    return e == SAIS_EPI_BIAS_BF16 || e == SAIS_EPI_BIAS_GELU_GRAD_BF16 || e == SAIS_EPI_MUL_BF16 || e == SAIS_EPI_BIAS_GELU_BF16 ||
           e == SAIS_EPI_BIAS_RELU_BF16;
}

enum { NT_W8R = 1, NT_W16, NT_W4Q };

template <int E>
static int launch_nt_exp(int form, const NtParams& p, int nt, int nt_grid, hipStream_t stream) {
    if (form == NT_W8R) {
        if (!sais_dyn_lds_once<gemm_nt_w8r_kernel<E>>(5 * TILE_BYTES)) return SAIS_ERR_LAUNCH;
        hipLaunchKernelGGL(gemm_nt_w8r_kernel<E>, dim3(nt < nt_grid ? nt : nt_grid), dim3(512), 5 * TILE_BYTES, stream, p, nt);
    } else if (form == NT_W16) {
        if (!sais_dyn_lds_once<gemm_nt_w16_kernel<E>>(10 * TILE_BYTES)) return SAIS_ERR_LAUNCH;
        const int half = (nt + 1) / 2;
        hipLaunchKernelGGL(gemm_nt_w16_kernel<E>, dim3(half < 256 ? half : 256), dim3(1024), 10 * TILE_BYTES, stream, p, nt);
    } else {
        hipLaunchKernelGGL(gemm_nt_w4q_kernel<E>, dim3(nt < 1024 ? nt : 1024), dim3(256), 5 * QTILE, stream, p, nt);
    }
    return sais_check_launch() == SAIS_OK ? 1 : SAIS_ERR_LAUNCH;
}
#define NT_EXP_CASE(E) case E: return launch_nt_exp<E>(form, p, (int)nt_tiles(g).x, nt_grid, (hipStream_t)stream);

// Called by sais_gemm_nt (gemm.hip) for M >= 8192 after its argument checks: 0 = no switch asks for one of the forms here or the
// form does not cover this GEMM (the caller goes on to the shipped kernel), 1 = launched, < 0 = error.
extern "C" int sais_gemm_nt_exp_(const SaisGemm* g, int nt_grid, void* stream) {
    static const bool nt_w8r = sais_env_int("SAIS_NT_W8R", 0) != 0, nt_w16 = sais_env_int("SAIS_NT_W16", 0) != 0,
                      nt_w4 = sais_env_int("SAIS_NT_W4", 0) != 0;
    const bool w4e = w4_epi(g->epilogue);
    const int form = nt_w8r && w4e && g->K == 6 * BK ? NT_W8R
                   : nt_w16 && g->K / BK >= 5 ? NT_W16
                   : nt_w4 && w4e && g->K >= 2 * QK ? NT_W4Q : 0;
    if (!form) return 0;
    const NtParams p = nt_params(g);
    switch (g->epilogue) {
        NT_EPILOGUES(NT_EXP_CASE)
        default: return 0;
    }
#undef NT_EXP_CASE
}

#endif  // SAIS_EXPERIMENTAL
