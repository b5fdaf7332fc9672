// Linear probe on frozen features (dino-main/eval_linear.py:103-109,163-183,237-251): up to 8 classifier heads that differ only
// in learning rate, trained from ONE feature batch in three launches for any number of heads.
//   sais_probe_logits  Z[h] = X W[h]^T + b[h]                                   (nn.Linear, :246-251)
//   sais_probe_ce      per (head, row): lse, loss_row = lse - z[target], the five best classes, and in train mode, in place,
//                      dZ = (softmax - onehot) / B                              (nn.CrossEntropyLoss, mean reduction, :176)
//   sais_probe_update  G = dZ[h]^T X per 64 x 64 tile of W[h], then torch's momentum SGD on that tile: m = mu m + G,
//                      W -= lr[h] m (:103-108; dampening 0, weight decay 0).  dW is never written to memory.
// Arithmetic: the exact f32-input MFMA (v_mfma_f32_16x16x4_f32), which is bit for bit an fmaf chain in ascending k.  Every
// output element has ONE accumulator that runs over the whole K in ascending order, tails are zero-staged: a row's logits do
// not depend on the batch size, on the row's position or on the number of heads.  Reductions over rows (bias gradient, mean
// loss) run in row order in one thread; nothing is atomic, so every result is bit-reproducible.
// LDS images: operand element [i][k] of a 16 x 4 MFMA step is read by lane (i = lane & 15, k = lane >> 4) as one dword.
//   logits: [64 rows][32 k] with 36-float rows: bank = 36 i + k, 36 i mod 64 are 16 distinct multiples of 4 -> no conflicts
//   update: [32 k][64 i] with 80-float rows:   bank = 80 k + i, 80 k mod 64 = 0, 16, 32, 48              -> no conflicts
#include "common.hpp"
#include "../../include/sais_hip.h"

namespace {

constexpr int BT = 64;                       // tile side of both GEMMs (rows x classes, classes x features)
constexpr int LK = 32, LLD = 36;             // logits: K step, LDS row stride in floats
constexpr int UK = 32, ULD = 80;             // update: K (= batch row) step, LDS row stride in floats

struct LogitsParams {
    const float* X;      // [B, Dm]
    const float* W;      // [H, C, Dm]
    const float* b;      // [H, C]
    float* Z;            // [H, B, C]
    int B, C, Dm;
};

// grid (class tiles, row tiles, heads); wave (wr, wc) owns the 32 x 32 quadrant as 2 x 2 MFMA tiles
__global__ __launch_bounds__(256) void probe_logits_kernel(LogitsParams p) {
    __shared__ __attribute__((aligned(16))) float As[BT * LLD], Bs[BT * LLD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, g = lane >> 4, li = lane & 15;
    const int n0 = blockIdx.x * BT, m0 = blockIdx.y * BT, h = blockIdx.z;
    const float* W = p.W + (size_t)h * p.C * p.Dm;
    const int sc = tid & 7, sr = tid >> 3;                 // staging: 8 x 16-B chunks per 32-float row, 32 rows per pass
    f32x4 ra[2], rb[2];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = sr + 32 * i;
            ra[i] = m0 + r < p.B ? *(const f32x4*)(p.X + (size_t)(m0 + r) * p.Dm + k0 + 4 * sc) : f32x4{0, 0, 0, 0};
            rb[i] = n0 + r < p.C ? *(const f32x4*)(W + (size_t)(n0 + r) * p.Dm + k0 + 4 * sc) : f32x4{0, 0, 0, 0};
        }
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    gload(0);
    for (int k0 = 0; k0 < p.Dm; k0 += LK) {
        __syncthreads();                                   // the previous step's fragments are read
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *(f32x4*)(As + (sr + 32 * i) * LLD + 4 * sc) = ra[i];
            *(f32x4*)(Bs + (sr + 32 * i) * LLD + 4 * sc) = rb[i];
        }
        __syncthreads();
        if (k0 + LK < p.Dm) gload(k0 + LK);
#pragma unroll
        for (int kk = 0; kk < LK; kk += 4) {
            float a[2], b[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                a[u] = As[(wr * 32 + u * 16 + li) * LLD + kk + g];
                b[u] = Bs[(wc * 32 + u * 16 + li) * LLD + kk + g];
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = mfma4(a[mt], b[nt], acc[mt][nt]);
        }
    }
    float* Z = p.Z + (size_t)h * p.B * p.C;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int c = n0 + wc * 32 + nt * 16 + li;
        if (c >= p.C) continue;
        const float bias = p.b[(size_t)h * p.C + c];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wr * 32 + mt * 16 + 4 * g + r;
                if (m < p.B) Z[(size_t)m * p.C + c] = acc[mt][nt][r] + bias;
            }
    }
}

// one wave per (head, row); the row's logits sit in LDS
__global__ __launch_bounds__(64) void probe_ce_kernel(float* Z, const int* targets, int B, int C, int train, float* loss_rows,
                                                      int* top5) {
    __shared__ float z[SAIS_PROBE_MAX_CLASSES];
    const int row = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    float* zr = Z + ((size_t)h * B + row) * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) {
        const float v = zr[c];
        z[c] = v;
        mx = fmaxf(mx, v);
    }
    mx = wave_max(mx);
    __syncthreads();
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(z[c] - mx);
    s = wave_sum(s);
    const float lse = mx + logf(s);
    const int t = targets[row];
    if (lane == 0) loss_rows[(size_t)h * B + row] = lse - (t >= 0 && t < C ? z[t] : 0.f);      // (the host checks the range)
    if (top5) wave_best5(z, C, lane, top5 + ((size_t)h * B + row) * 5);      // by (logit descending, class ascending)
    if (train) {
        const float inv = 1.0f / (float)B;
        for (int c = lane; c < C; c += 64) zr[c] = (expf(z[c] - lse) - (c == t ? 1.0f : 0.0f)) * inv;
    }
}

// mean of a head's row losses in row order: the rows are staged in LDS by the whole wave, one thread adds them
DEVINL void loss_mean(const float* loss_rows, int B, float* stage /* [SAIS_PROBE_MAX_ROWS] */, int lane, float* out) {
    for (int r = lane; r < B; r += 64) stage[r] = loss_rows[r];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (lane == 0) {
        float s = 0.f;
        for (int r = 0; r < B; ++r) s += stage[r];
        *out = s / (float)B;
    }
}

__global__ __launch_bounds__(64) void probe_loss_kernel(const float* loss_rows, int B, float* loss) {
    __shared__ float stage[SAIS_PROBE_MAX_ROWS];
    loss_mean(loss_rows + (size_t)blockIdx.x * B, B, stage, threadIdx.x, loss + blockIdx.x);
}

// grid (feature tiles, class tiles, heads); wave (wr, wc) owns the 32 x 32 quadrant (classes x features) of the tile
__global__ __launch_bounds__(256) void probe_update_kernel(SaisProbeUpdate p) {
    __shared__ __attribute__((aligned(16))) float Gs[UK * ULD], Xs[UK * ULD];      // dZ [row][class], X [row][feature]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, g = lane >> 4, li = lane & 15;
    const int d0 = blockIdx.x * BT, c0 = blockIdx.y * BT, h = blockIdx.z;
    const int B = p.B, C = p.C, Dm = p.Dm;
    const float* dZ = p.dZ + (size_t)h * B * C;
    const int gc = tid & 63, gr = tid >> 6;                // dZ staging: one class column, rows gr + 4 i (C need not be even)
    const int xc = tid & 15, xr = tid >> 4;                // X staging: 16 x 16-B chunks per 64-float row, rows xr + 16 i
    float rg[8];
    f32x4 rx[2];
    auto gload = [&](int r0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = r0 + gr + 4 * i;
            rg[i] = r < B && c0 + gc < C ? dZ[(size_t)r * C + c0 + gc] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = r0 + xr + 16 * i;
            rx[i] = r < B ? *(const f32x4*)(p.X + (size_t)r * Dm + d0 + 4 * xc) : f32x4{0, 0, 0, 0};
        }
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    gload(0);
    for (int r0 = 0; r0 < B; r0 += UK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) Gs[(gr + 4 * i) * ULD + gc] = rg[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *(f32x4*)(Xs + (xr + 16 * i) * ULD + 4 * xc) = rx[i];
        __syncthreads();
        if (r0 + UK < B) gload(r0 + UK);
#pragma unroll
        for (int kk = 0; kk < UK; kk += 4) {
            float a[2], b[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                a[u] = Gs[(kk + g) * ULD + wr * 32 + u * 16 + li];
                b[u] = Xs[(kk + g) * ULD + wc * 32 + u * 16 + li];
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = mfma4(a[mt], b[nt], acc[mt][nt]);
        }
    }
    const float mu = p.momentum, lr = p.lr[h];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = c0 + wr * 32 + mt * 16 + 4 * g + r;
            if (c >= C) continue;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const size_t at = ((size_t)h * C + c) * Dm + d0 + wc * 32 + nt * 16 + li;      // d < Dm: Dm % 64 == 0
                const float m = mu * p.mW[at] + acc[mt][nt][r];
                p.mW[at] = m;
                p.W[at] -= lr * m;
            }
        }
    if (blockIdx.x != 0) return;
    // the owners of feature tile 0: the bias of their 64 classes, db[c] = sum over the rows of dZ[r][c] in row order
    if (tid < BT && c0 + tid < C) {
        const int c = c0 + tid;
        float s = 0.f;
        for (int r = 0; r < B; ++r) s += dZ[(size_t)r * C + c];
        const size_t at = (size_t)h * C + c;
        const float m = mu * p.mb[at] + s;
        p.mb[at] = m;
        p.b[at] -= lr * m;
    }
    // ... and the owner of class tile 0 the head's mean loss (wave 1: wave 0 is busy with the bias), staged in the dZ image
    if (blockIdx.y == 0 && p.loss) {                       // (workgroup-uniform)
        __syncthreads();                                   // every wave has read its last fragments
        if (wid == 1) loss_mean(p.loss_rows + (size_t)h * B, B, Gs, lane, p.loss + h);
    }
}

bool shape_ok(int H, int B, int C, int Dm) {
    return H >= 1 && H <= SAIS_PROBE_MAX_HEADS && B >= 1 && B <= SAIS_PROBE_MAX_ROWS && C >= 1 && C <= SAIS_PROBE_MAX_CLASSES &&
           Dm >= BT && Dm % BT == 0 && Dm <= SAIS_PROBE_MAX_DIM;
}

}  // namespace

static_assert(UK * ULD >= SAIS_PROBE_MAX_ROWS, "the loss rows are staged in the dZ image");

extern "C" int sais_probe_logits(const float* X, const float* W, const float* b, int H, int B, int C, int Dm, float* Z,
                                 void* stream) {
    SAIS_ENTER();
    if (!X || !W || !b || !Z || !shape_ok(H, B, C, Dm)) return SAIS_ERR_ARG;
    LogitsParams p{X, W, b, Z, B, C, Dm};
    hipLaunchKernelGGL(probe_logits_kernel, dim3((C + BT - 1) / BT, (B + BT - 1) / BT, H), dim3(256), 0, (hipStream_t)stream, p);
    return sais_check_launch();
}

extern "C" int sais_probe_ce(float* Z, const int* targets, int H, int B, int C, int train, float* loss_rows, int* top5,
                             float* loss, void* stream) {
    SAIS_ENTER();
    if (!Z || !targets || !loss_rows || !shape_ok(H, B, C, BT)) return SAIS_ERR_ARG;
    if (!train && (!loss || !top5)) return SAIS_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(probe_ce_kernel, dim3(B, H), dim3(64), 0, s, Z, targets, B, C, train ? 1 : 0, loss_rows, top5);
    if (loss) hipLaunchKernelGGL(probe_loss_kernel, dim3(H), dim3(64), 0, s, (const float*)loss_rows, B, loss);
    return sais_check_launch();
}

extern "C" int sais_probe_update(const SaisProbeUpdate* u, void* stream) {
    SAIS_ENTER();
    if (!u || !u->X || !u->dZ || !u->W || !u->b || !u->mW || !u->mb || !shape_ok(u->H, u->B, u->C, u->Dm)) return SAIS_ERR_ARG;
    if ((u->loss == nullptr) != (u->loss_rows == nullptr)) return SAIS_ERR_ARG;
    if (!(u->momentum >= 0.f && u->momentum < 1.f)) return SAIS_ERR_ARG;
    for (int h = 0; h < u->H; ++h)
        if (!(u->lr[h] >= 0.f && u->lr[h] < INFINITY)) return SAIS_ERR_ARG;
    hipLaunchKernelGGL(probe_update_kernel, dim3(u->Dm / BT, (u->C + BT - 1) / BT, u->H), dim3(256), 0, (hipStream_t)stream, *u);
    return sais_check_launch();
}
