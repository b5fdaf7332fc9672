/* libsais_hip.so — C ABI of the MI355X (gfx950) kernels behind the SAIS ViT-over-video hot path.
 *
 * The reference (danikiyasseh/SAIS) has no FFI / plugin interface: every op on this path is a stock
 * torch.nn module executed by ATen on the CPU.  The entry points below are therefore the operator
 * set a maintainer would bind in place of those modules; each one cites the reference code it
 * replaces (paths relative to SAIS/scripts/).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions (all entry points):
 *   - raw DEVICE pointers owned by the caller; no allocation, no host sync, no global state;
 *   - asynchronous on the passed hipStream_t (`stream`, passed as void*); re-entrant across streams;
 *   - returns 0 (SAIS_OK) or a negative error code, never throws;
 *   - "bf16" = bfloat16 storage, "f32" = IEEE float; all accumulation / statistics in f32;
 *   - row-major tensors, `ld*` = leading dimension in ELEMENTS.
 */
#ifndef SAIS_HIP_H
#define SAIS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAIS_ABI_VERSION 13
int sais_abi_version(void);
/* text of the HIP error behind the calling thread's last SAIS_ERR_LAUNCH (-2) return */
const char* sais_last_error(void);

/* ---------------------------------------------------------------- GEMM  C = A . B^T (+epilogue)
 * Replaces nn.Linear.forward everywhere on the path:
 *   dino-main/vision_transformer.py:59-65 (Mlp fc1/fc2), :80-92 (Attention qkv/proj), :128-131
 *   (PatchEmbed conv == GEMM on patches); prepare_model.py:74-81 (TransformerEncoderLayer in_proj /
 *   out_proj / linear1 / linear2).  With the transposed weight it is also dX = dY . W.          */
enum {
    SAIS_EPI_BIAS_BF16 = 0,       /* out bf16 = acc + bias                                           */
    SAIS_EPI_BIAS_RELU_BF16 = 1,  /* out bf16 = relu(acc + bias)                                     */
    SAIS_EPI_BIAS_F32 = 2,        /* out f32  = acc + bias                                           */
    SAIS_EPI_BIAS_RESID_F32 = 3,  /* out f32  = aux(f32) + acc + bias ; out2 (optional) same in bf16 */
    SAIS_EPI_BIAS_GELU_BF16 = 4,  /* out bf16 = gelu_erf(acc + bias) ; out2 (optional) = acc + bias  */
    SAIS_EPI_DGELU_BF16 = 5,      /* out bf16 = acc * gelu'(aux bf16)                                */
    SAIS_EPI_DRELU_BF16 = 6,      /* out bf16 = acc * (aux bf16 > 0)                                 */
    SAIS_EPI_BIAS_RELU_F32 = 8,   /* (f32 GEMM only) out f32 = relu(acc + bias)                      */
    SAIS_EPI_DRELU_F32 = 9,       /* (f32 GEMM only) out f32 = acc * (aux f32 > 0)                   */
    SAIS_EPI_BIAS_GELU_GRAD_BF16 = 10, /* out bf16 = gelu_erf(acc + bias) ; out2 bf16 = gelu'(acc + bias): the training
                                     forward stores the derivative instead of the pre-activation, so that ...     */
    SAIS_EPI_MUL_BF16 = 11,       /* ... the backward is out bf16 = acc * aux(bf16), with no erf/exp in its epilogue */
    SAIS_EPI_PATCH_F32 = 7,       /* patch-embed: row f*grp_in+q -> token row f*grp_out+q+grp_off,
                                     out f32 = acc + bias + aux(f32 pos)[q+grp_off]                  */
    SAIS_EPI_BIAS_GELU_GRADQ_BF16 = 13, /* (ABI 12) as 10, but out2 holds gelu'(acc + bias) as ONE BYTE per element: code q =
                                     clamp(rint(26 + 203 d), 0, 255), i.e. d = (q - 26) / 203 — 0 and 1 are exact, the range
                                     [-0.128, 1.128] covers gelu' (min -0.129, max 1.129), step 0.0049 (rms error 0.0014; a bf16
                                     near 0.5 has 0.0011): half the bytes of the tensor the backward reads again; ldo2 in bytes */
    SAIS_EPI_MULQ_BF16 = 14,      /* (ABI 12) out bf16 = acc * (aux(u8) - 26) / 203: the backward of 13; ldaux in bytes        */
    SAIS_EPI_RAW_SLABS_F32 = 12   /* (ABI 8, M < 8192 only) split-K: K is cut into grp_in slices, slice z writes its raw partial
                                     sums to out f32 [grp_in][M][ldo]; sais_splitk_finish sums them in a fixed order      */
};

typedef struct SaisGemm {
    const void* A; int lda;        /* bf16 [M,K]                         */
    const void* B; int ldb;        /* bf16 [N,K]  (nn.Linear weight)     */
    int M, N, K;                   /* N % 128 == 0, K % 64 == 0          */
    int epilogue;                  /* SAIS_EPI_*                         */
    const float* bias;             /* f32 [N] or NULL                    */
    void* out; int ldo;
    void* out2; int ldo2;
    const void* aux; int ldaux;
    int grp_in, grp_out, grp_off;  /* SAIS_EPI_PATCH_F32 only            */
    const float* rowscale;         /* SAIS_EPI_BIAS_RESID_F32 only, optional: DropPath (vision_transformer.py:27-46,111,113)
                                      out = aux + rowscale[m] * (acc + bias), rowscale[m] = keep / (1 - p) of row m's sample */
    /* sais_gemm_nt_f32 only: train-mode dropout of the temporal encoder layer fused into the epilogue (p_drop = 0: none);
     * mask element = m * N + n of site `site` (see sais_dropout_f32):  _BIAS_RESID_F32: out = aux + drop(acc + bias)
     * (dropout1 / dropout2);  _BIAS_RELU_F32: out = drop(relu(acc + bias)) (the FFN dropout);  _DRELU_F32: out =
     * drop(acc) where aux > 0 (its backward, same site).                                                          */
    float p_drop; const unsigned long long* rng_state; unsigned site;
} SaisGemm;

int sais_gemm_nt(const SaisGemm* g, void* stream);
/* Second half of a SAIS_EPI_RAW_SLABS_F32 product (the [frames, 384] GEMMs of the CLS-only last ViT block: a K = 1536 loop
 * over 6 output tiles is 24 serial steps; cut 12 ways it is 72 workgroups of 2):
 *   y = sum_z slabs[z][m][n] + bias[n];  y *= rowscale[m] (optional);  y += aux[m][n] (optional, f32);
 *   out32 (optional) = y, out16 (optional) = bf16(y).  Deterministic (fixed summation order, no atomics).            */
int sais_splitk_finish(const float* slabs, int nslabs, int M, int N, int lds, const float* bias, const float* rowscale,
                       const float* aux, int ldaux, float* out32, int ldo32, void* out16, int ldo16, void* stream);

/* Same contract with FP32 operands (A f32 [M,K], B f32 [N,K], out f32) at ~fp32 accuracy: each operand is
 * split hi/lo into two bf16 and three MFMA products are accumulated ("bf16x3").  Epilogues:
 * SAIS_EPI_BIAS_F32, _BIAS_RESID_F32 (aux f32), _BIAS_RELU_F32, _DRELU_F32 (aux f32).  This is what the
 * temporal TransformerEncoder's nn.Linear layers run on (prepare_model.py:74-81, called at :213): its
 * activations feed the <=1e-3 logit parity bar directly and are tiny.
 * Optional split-K for these few-row problems: out2 = caller workspace f32 [ldo2][M][N], ldo2 = number of K
 * splits (must divide K/64); partial sums land there and a second tiny kernel reduces + applies the epilogue. */
int sais_gemm_nt_f32(const SaisGemm* g, void* stream);

/* ---------------------------------------------------------------- the temporal encoder's linear layers (round 3)
 * The same "bf16x3" arithmetic as sais_gemm_nt_f32, tiled for M = clips x (T + 1) = a few hundred rows: 64 x 64 output
 * tiles, two K-steps of loads in flight, optional split-K into RAW partial slabs out[z][M][N] (z < nsplit, nsplit divides
 * K / 64) that the row kernels below consume — there is no separate reduce launch.  N % 64 == 0, K % 64 == 0.
 *   SAIS_TG_RAW        out[z] = partial A . W^T                      (out_proj / linear2 forward; every N = 384 dX)
 *   SAIS_TG_BIAS       out = A . W^T + bias (bias may be NULL)       (in_proj, prepare_model.py:213 -> MultiheadAttention)
 *   SAIS_TG_BIAS_RELU  out = drop(relu(A . W^T + bias))              (linear1 + activation + dropout)
 *   SAIS_TG_DRELU      out = drop(A . W^T) where aux > 0, else 0     (its backward; aux = the saved, dropped relu output)
 * drop(): train-mode dropout, mask element m * N + n of `site`, p_drop = 0 for none.                                  */
#define SAIS_TG_RAW 0
#define SAIS_TG_BIAS 1
#define SAIS_TG_BIAS_RELU 2
#define SAIS_TG_DRELU 3
typedef struct SaisTGemm {
    const float* A; long lda;      /* f32 [M,K]                          */
    const float* W; long ldw;      /* f32 [N,K]  (nn.Linear weight, or its transpose for dX) */
    int M, N, K;
    int epilogue;                  /* SAIS_TG_*                          */
    int nsplit;                    /* SAIS_TG_RAW: number of K splits = slabs written; otherwise 1 */
    const float* bias;             /* f32 [N] or NULL                    */
    const float* aux; long ldaux;  /* SAIS_TG_DRELU                      */
    float* out; long ldo;          /* f32 [M,N] (RAW: [nsplit][M][N], ldo = N) */
    float p_drop; const unsigned long long* rng_state; unsigned site;
} SaisTGemm;
int sais_tgemm(const SaisTGemm* g, void* stream);
/* the K split this library recommends for a SAIS_TG_RAW launch of that shape (>= 1; the slab workspace the caller passes
 * as `out` is nsplit * M * N floats): the sizing rule lives here, not in the host language                               */
int sais_tgemm_nsplit(int M, int N, int K);
/* Row kernels over D = 384 that CONSUME the slabs (split-K reduce + epilogue + LayerNorm in one pass):
 *   sais_temporal_ln_fwd:  y = resid + drop(sum_z slabs[z] + bias) ;  z = LayerNorm(y; gamma, beta, eps) ; mean / rstd saved
 *       = `src = src + dropout1(out_proj(..))` / `src = src + dropout2(linear2(..))` followed by norm1 / norm2 of the
 *         torch-1.8 post-norm TransformerEncoderLayer (prepare_model.py:74-81).  y may be NULL (inference).
 *   sais_temporal_ln_bwd:  dy = sum_z slabs[z] + add (either may be NULL) ;  dx = autograd of that LayerNorm at (x, mean,
 *       rstd) ;  dx_drop = drop(dx) (optional second output: the gradient entering the residual BRANCH) ;
 *       dgamma += sum_m dy xhat ; dbeta += sum_m dy.                                                                  */
int sais_temporal_ln_fwd(const float* slabs, int nslab, long slab_stride, const float* bias, const float* resid, int rows,
                         float p_drop, const unsigned long long* rng_state, unsigned site, float* y, const float* gamma,
                         const float* beta, float eps, float* z, float* mean, float* rstd, void* stream);
int sais_temporal_ln_bwd(const float* slabs, int nslab, long slab_stride, const float* add, const float* x,
                         const float* mean, const float* rstd, const float* gamma, int rows, float* dx, float* dx_drop,
                         float p_drop, const unsigned long long* rng_state, unsigned site, float* dgamma, float* dbeta,
                         void* stream);

/* dW[N1,N2] += P[M,N1]^T . Q[M,N2]  and (db != NULL)  db[N1] += column sums of P.
 * Weight / bias gradients of every nn.Linear above (autograd of F.linear).  Accumulates with f32
 * atomics into dW/db (caller zeroes them: optimizer.zero_grad(), perform_training.py:155).
 * Alignment, for this entry and the four sais_gemm_tn_* entries below: P and Q must be 16-B aligned (they are read in 16-B pieces),
 * ldp and ldq multiples of 8 elements (4 for sais_gemm_tn_grouped_f32), dW and db 4-B aligned; N1 and N2 multiples of 128.  */
int sais_gemm_tn(const void* P, int ldp, const void* Q, int ldq, int M, int N1, int N2,
                 float* dW, int ldw, float* db, int nsplit, void* stream);
/* Several weight-gradient GEMMs over the same M rows in ONE launch (all bf16): the four nn.Linear of a ViT
 * block give 108 output tiles, so a few M-splits fill the chip and the atomic traffic shrinks accordingly. */
#define SAIS_TN_MAX_ITEMS 48
typedef struct SaisTnItem {
    const void* P; int ldp;        /* bf16 [M,N1]  (dY)  */
    const void* Q; int ldq;        /* bf16 [M,N2]  (X)   */
    int N1, N2;
    float* dW; int ldw;            /* f32 [N1,N2], accumulated */
    float* db;                     /* f32 [N1] or NULL         */
} SaisTnItem;
int sais_gemm_tn_grouped(const SaisTnItem* items, int nitems, int M, int nsplit, void* stream);
/* ABI 10: the same launch with a caller-provided slab workspace.  In the large-tile regime (round 6, csrc/gemm_tn_xl.hip: every
 * N1 % 192 == 0 and N2 % 384 == 0, M % 32 == 0, M >= 8192, >= 48 32-row steps per M-split — the four nn.Linear of a ViT block at
 * training size) the M-splits store their raw 192 x 384 partial tiles into `slabs` (plain 16-B stores) and a second launch sums
 * them in a FIXED order into dW / db: no fp32 atomics (10 splits x 7.1 MB of them per ViT block otherwise, ~50 us of the launch),
 * bit-reproducible weight gradients.  sais_gemm_tn_grouped_slab_bytes returns the bytes that launch uses (0: no slab form applies
 * and `slabs` is ignored); slabs 16-B aligned; NULL = fp32 atomics; fewer bytes than that = SAIS_ERR_ARG.  The query and the launch
 * read ONE plan (csrc/tn_plan.hpp: form, tiles, M-splits, slab bytes), so they cannot disagree.  Environment, read once per process: SAIS_TN_XL = 0 selects
 * the 128 x 384 kernel of rounds 2-5 (whose own slab form stays opt-in: SAIS_TN_SLABS = 1), SAIS_TN_XL = 8 the eight-wave form
 * of the large tile, SAIS_TN_XL_SLABS = 0 its atomics (LABNOTES R6.1).                                                      */
size_t sais_gemm_tn_grouped_slab_bytes(const SaisTnItem* items, int nitems, int M);
int sais_gemm_tn_grouped_ws(const SaisTnItem* items, int nitems, int M, int nsplit, void* slabs, size_t slab_bytes, void* stream);
/* the same with FP32 P and Q (rounded to bf16 while staging, like sais_gemm_tn_f32): one launch for the four weight
 * gradients of a temporal-encoder layer                                                                        */
int sais_gemm_tn_grouped_f32(const SaisTnItem* items, int nitems, int M, int nsplit, void* stream);
/* same as sais_gemm_tn with f32 P and Q (rounded to bf16 while staging; f32 accumulation) */
int sais_gemm_tn_f32(const void* P, int ldp, const void* Q, int ldq, int M, int N1, int N2,
                     float* dW, int ldw, float* db, int nsplit, void* stream);

/* ---------------------------------------------------------------- GEMM with LayerNorm in the epilogue (N = 384)
 * The ViT block's residual stream is D = 384 wide, so a workgroup that owns a 128-row x 384-column output tile owns
 * whole rows and can normalise them before they leave the registers (SURVEY §7 steps 4-5, §8b `proj_residual`,
 * `fc2_residual`, `ln_qkv`, `ln_fc1_gelu`):
 *   sais_gemm_ln_fwd:  x_out = A . W^T + bias + resid ;  out16 = LayerNorm(x_out; gamma, beta, eps) ; mean/rstd saved.
 *       = `x = x + attn.proj(...)` / `x = x + mlp.fc2(...)` followed by the NEXT `norm2` / `norm1`
 *         (Block.forward, dino-main/vision_transformer.py:107-113; nn.LayerNorm(eps=1e-6) via vit_small :243-247).
 *   sais_gemm_ln_bwd:  dy = A . W^T (the dX of fc1 / qkv: autograd of F.linear, :59-65 / :80-92) followed by autograd
 *       of that LayerNorm:  dx = dres + rstd (dy g - mean(dy g) - xhat mean(dy g xhat)),  dgamma += sum_m dy xhat,
 *       dbeta += sum_m dy.  `resid` is the LayerNorm INPUT x saved by the forward, `mean`/`rstd` its statistics.
 * W is bf16 [384,K] (K % 64 == 0), A bf16 [M,K]; out32 / dres may alias (in-place residual-gradient update).       */
typedef struct SaisGemmLn {
    const void* A; int lda;        /* bf16 [M,K]                                              */
    const void* W; int ldw;        /* bf16 [384,K]                                            */
    int M, K;
    const float* bias;             /* fwd: f32 [384] or NULL; bwd: unused                     */
    const float* resid; int ldr;   /* fwd: residual f32 [M,384]; bwd: LayerNorm input x f32   */
    float* out32; int ldo32;       /* fwd: x_out; bwd: dx (f32, optional)                     */
    void* out16; int ldo16;        /* fwd: LayerNorm(x_out) bf16; bwd: dx bf16 (optional)     */
    const float* gamma; const float* beta; float eps;
    float* mean; float* rstd;      /* fwd: outputs [M] (optional); bwd: inputs                */
    const float* dres; int lddres; /* bwd: residual-stream gradient added to dx (optional)    */
    float* dgamma; float* dbeta;   /* bwd: f32 [384], accumulated (both or neither)           */
    const float* rowscale;         /* fwd, optional (DropPath): x_out = resid + rowscale[m] * (A.W^T + bias)            */
    const float* rowscale16;       /* bwd, optional (DropPath): out16 = bf16(rowscale16[m] * dx): the gradient that enters
                                      the NEXT branch's backward GEMMs; out32 (the residual-stream gradient) is not scaled */
    int dres_period;               /* bwd (ABI 8): 0 = dres is [M,384].  > 0: dres is COMPACT [ceil(M / period), 384]: row m of the
                                      residual-stream gradient is dres[m / period] when m % period == 0 and ZERO otherwise — the
                                      gradient entering the last ViT block exists on the CLS rows only (period = tokens per frame;
                                      VisionTransformer.forward returns x[:, 0], vision_transformer.py:212-214)            */
    const void* xn16; int ldxn16;  /* bwd, optional (ABI 11): the bf16 LayerNorm OUTPUT y = xhat * gamma + beta the forward saved for the
                                      next GEMM and for dW.  With it (and `beta`) the epilogue rebuilds xhat = (y - beta) / gamma from
                                      768 B per row instead of reading the 1536-B fp32 `resid` row (-38.7 MB per launch at config 2);
                                      `resid` must still be valid: a workgroup falls back to it when some |gamma_c| < 1e-3 or
                                      |beta_c| > 64 |gamma_c| (the division would amplify y's bf16 rounding).  xhat enters dx only
                                      through xhat * mean(dy g xhat), a term ~1/sqrt(384) of dy: measured effect on the ViT parameter
                                      gradients <= 1e-3 relative (tests).  SAIS_LN_BWD_X16=0 in the environment ignores the field. */
} SaisGemmLn;
int sais_gemm_ln_fwd(const SaisGemmLn* g, void* stream);
int sais_gemm_ln_bwd(const SaisGemmLn* g, void* stream);

/* ---------------------------------------------------------------- the MLP branch of a ViT block as ONE launch (ABI 8)
 * Block-level entry points (ln_fc1_gelu + fc2_residual of Block.forward in one call).
 *   sais_mlp_fwd:  Mlp.forward (dino-main/vision_transformer.py:49-65: fc1 -> nn.GELU() exact erf -> fc2, dropout p = 0)
 *       + the residual add of Block.forward (:111-112: x = x + drop_path(mlp(norm2(x)))) + the NEXT LayerNorm of the
 *       residual stream (the next block's norm1, :107-108; eps 1e-6 via vit_small :243-247):
 *         u = X . W1^T + bias1;  h = GELU(u);  g = GELU'(u);
 *         out32 = resid + rowscale[m] * (h . W2^T + tail.bias);  out16 = LayerNorm(out32);  mean / rstd saved.
 *       X = LayerNorm2(x_mid) bf16 [M,384]; W1 = fc1.weight bf16 [H,384]; W2 = fc2.weight bf16 [384,H]; H % 128 == 0.
 *       h / g: bf16 [M,H] outputs the backward pass needs (dW2 = d^T h, du = (d W2) g).  g == NULL (inference): GELU'
 *       is not evaluated, and with h == NULL too the hidden activation is never written to HBM at all.
 *       tail.gamma == NULL: no following LayerNorm (the last block): only out32 is written.
 *   sais_mlp_bwd:  autograd of the same branch up to the block's norm2 (backward of :59-65 and of nn.LayerNorm):
 *         du = (X . W1^T) * g  (X = bf16 gradient entering the branch [M,384], W1 = fc2.weight^T bf16 [H,384], g = GELU'(u)
 *         saved by the forward) -> written to h (dW1 = du^T xn2 needs it);  dxn = du . W2^T (W2 = fc1.weight^T bf16 [384,H]);
 *         then exactly sais_gemm_ln_bwd's epilogue on dxn with tail.{resid = x_mid, mean, rstd, gamma, dres, dgamma, dbeta,
 *         out32, out16, rowscale16}.
 * `tail` is read like the argument of sais_gemm_ln_fwd / _bwd; its A / lda / W / ldw / M / K fields are ignored.        */
typedef struct SaisMlp {
    const void* X; int ldx;
    const void* W1; int ldw1;
    const float* bias1;            /* fwd: f32 [H] or NULL; bwd: unused */
    const void* W2; int ldw2;
    int M, H;
    void* h; int ldh;
    void* g; int ldg;
    SaisGemmLn tail;
} SaisMlp;
int sais_mlp_fwd(const SaisMlp* a, void* stream);
int sais_mlp_bwd(const SaisMlp* a, void* stream);

/* ================================================================ block-level entry points (ABI 8)
 * One call = one Block of the ViT (dino-main/vision_transformer.py:95-113: x = x + drop_path(attn(norm1(x)));
 * x = x + drop_path(mlp(norm2(x)))) in either direction: C-side sequencing of the GEMM-level entries above, so that a host
 * in any language drives the encoder with 12 + 12 calls per step instead of re-implementing the ~25-launch plan of
 * sais_amd/vit.py.  Conventions as everywhere: raw device pointers owned by the caller, no allocation, no host sync,
 * asynchronous on `stream`, 0 / negative return.  Scratch comes from the caller: `workspace` of at least
 * sais_workspace_bytes(op, frames, ntok) bytes, 256-B aligned.  The LayerNorms sit where the kernels fuse them: a forward call
 * CONSUMES norm1(x_in) (xn1, written by the previous block's call, or by sais_layernorm_fwd for block 0) and PRODUCES the next
 * block's norm1(x_out) (xn_next; next_norm_g == NULL for the last block).                                               */
enum SaisOp { SAIS_OP_VIT_BLOCK_FWD = 0, SAIS_OP_VIT_BLOCK_BWD = 1, SAIS_OP_TEMPORAL_LAYER_FWD = 2, SAIS_OP_TEMPORAL_LAYER_BWD = 3 };
size_t sais_workspace_bytes(int op, int frames, int ntok);   /* temporal ops: (op, sequences B, tokens S) */
/* (ABI 12) bytes per element of the GELU' tensor sais_vit_block_fwd writes and sais_vit_block_bwd reads: 1 = one-byte codes
 * (default; epilogues 13 / 14), 2 = bf16 (environment SAIS_GELU_GRAD_Q8=0, read once per process; epilogues 10 / 11). */
int sais_gelu_grad_bytes(void);

typedef struct SaisVitBlockParams {
    /* bf16 weight shadows [out,in] + f32 biases (nn.Linear of Attention :68-92 and Mlp :49-65), f32 LayerNorm parameters */
    const void* qkv_w;  const float* qkv_b;       /* [1152,384] */
    const void* proj_w; const float* proj_b;      /* [384,384]  */
    const void* fc1_w;  const float* fc1_b;       /* [1536,384] */
    const void* fc2_w;  const float* fc2_b;       /* [384,1536] */
    const float* norm1_g; const float* norm1_b;   /* backward only (norm1_b: ABI 11, may be NULL = fp32 LayerNorm input path) */
    const float* norm2_g; const float* norm2_b;
    const float* next_norm_g; const float* next_norm_b;   /* forward: norm1 of the NEXT block, or NULL */
    /* backward only: transposed bf16 shadows [in,out] (dX = dY . W runs on the same NT kernels) and f32 gradient accumulators */
    const void* qkv_wt; const void* proj_wt; const void* fc1_wt; const void* fc2_wt;
    float* d_qkv_w; float* d_qkv_b; float* d_proj_w; float* d_proj_b; float* d_fc1_w; float* d_fc1_b; float* d_fc2_w; float* d_fc2_b;
    float* d_norm1_g; float* d_norm1_b; float* d_norm2_g; float* d_norm2_b;
} SaisVitBlockParams;

typedef struct SaisVitBlockFwd {
    int frames, ntok;                /* M = frames * ntok token rows; ntok = 197 or 37 */
    const void* xn1;                 /* in : bf16 [M,384] norm1(x_in)                                             */
    const float* x_in;               /* in : f32 [M,384] residual stream                                          */
    void* qkv;                       /* out: bf16 [M,1152]   (saved for backward)                                 */
    void* attn_out;                  /* out: bf16 [M,384]    (saved)                                              */
    float* lse;                      /* out: f32 [frames,6,ntok] (saved; NULL in inference)                        */
    float* x_mid;                    /* out: f32 [M,384] x after the attention branch (may alias x_in in inference) */
    void* xn2;                       /* out: bf16 [M,384] norm2(x_mid) (saved)                                     */
    float* mean2; float* rstd2;      /* out: f32 [M] (saved; NULL in inference)                                    */
    void* h;                         /* out: bf16 [M,1536] GELU(u) (saved; NULL in inference: workspace is used)    */
    void* gelu_grad;                 /* out: [M,1536] GELU'(u), sais_gelu_grad_bytes() bytes per element: one-byte codes (ABI 12,
                                        SAIS_EPI_BIAS_GELU_GRADQ_BF16) or bf16 (saved; NULL in inference: not evaluated)       */
    float* x_out;                    /* out: f32 [M,384] (may alias x_mid in inference)                            */
    void* xn_next;                   /* out: bf16 [M,384] next block's norm1(x_out) (with next_norm_g)             */
    float* mean_next; float* rstd_next;   /* out: f32 [M] (optional)                                              */
    const float* rowscale_attn; const float* rowscale_mlp;   /* DropPath row scales f32 [M] of the two branches, or NULL */
} SaisVitBlockFwd;
int sais_vit_block_fwd(const SaisVitBlockParams* w, const SaisVitBlockFwd* a, void* workspace, size_t ws_bytes, void* stream);

typedef struct SaisVitBlockBwd {
    int frames, ntok;
    /* what the forward call saved */
    const float* x_in; const float* mean1; const float* rstd1; const void* xn1; const void* qkv; const void* attn_out;
    const float* lse; const float* x_mid; const float* mean2; const float* rstd2; const void* xn2; const void* h;
    const void* gelu_grad;
    float* dx;                       /* in/out: f32 [M,384] gradient of the residual stream (x_out's on entry, x_in's on return) */
    const void* dx16_in;             /* in : bf16 [M,384] = bf16(rowscale_mlp * dx): what enters the MLP branch           */
    void* dx16_out;                  /* out: bf16 [M,384] = bf16(rowscale_prev * dx on return): the next call's dx16_in    */
    const float* rowscale_attn;      /* DropPath scale of THIS block's attention branch, or NULL                           */
    const float* rowscale_prev;      /* DropPath scale of the PREVIOUS block's MLP branch (applied to dx16_out), or NULL   */
    int defer_dw;                    /* (ABI 13) != 0: the weight / bias gradients of this block are NOT launched by this call;
                                        sais_vit_blocks_dw launches them for several blocks at once.  Until then the caller keeps
                                        this struct's tensors, the workspace of this call and dx16_in untouched (dx16_out must
                                        then be a different buffer than dx16_in)                                             */
} SaisVitBlockBwd;
int sais_vit_block_bwd(const SaisVitBlockParams* w, const SaisVitBlockBwd* a, void* workspace, size_t ws_bytes, void* stream);
/* (ABI 13) The weight / bias gradients of `nblocks` blocks whose sais_vit_block_bwd calls ran with defer_dw, as ONE grouped launch of
 * 4 nblocks GEMMs (dW += P^T Q over the M = frames x ntok rows; LABNOTES R6.8).  One launch per block cuts M into ten splits so
 * that its 24 tiles fill the chip, and every split writes a partial tile that a second launch sums; two blocks per launch need five
 * splits, ten blocks none: 187 -> 160 -> 149 us per block at M = 50 432.  w[i], a[i], workspaces[i] = what call i was given
 * (each workspace >= sais_workspace_bytes(SAIS_OP_VIT_BLOCK_BWD, ...) bytes = ws_bytes). */
int sais_vit_blocks_dw(const SaisVitBlockParams* const* w, const SaisVitBlockBwd* const* a, void* const* workspaces, size_t ws_bytes,
                       int nblocks, const SaisTnItem* extra, int nextra, void* stream);
/* extra / nextra: further GEMMs over the same M rows to ride in the launch (the k / v weight gradient of the CLS-only last block:
 * 4 more tiles); 4 nblocks + nextra <= SAIS_TN_MAX_ITEMS. */

/* One layer of the temporal encoder per call: the torch-1.8 POST-norm nn.TransformerEncoderLayer(d 384, 4 heads, FF 2048,
 * ReLU, dropout 0.1, LayerNorm eps 1e-5) of prepare_model.py:74-81 as patched by README.md:43-48 (returns the attention map):
 *   src = norm1(src + dropout1(out_proj(MHA(src))));  src = norm2(src + dropout2(linear2(dropout(relu(linear1(src)))))).
 * 7 launches forward, 8 backward, sequenced by the library; fp32 tensors, linears on the bf16x3 path (sais_tgemm).
 * Dropout: p_drop = 0 for eval(); sites site0 .. site0 + 3 = attention weights, dropout1, FFN dropout, dropout2.        */
typedef struct SaisTemporalLayerParams {
    const float* in_proj_w;  const float* in_proj_b;    /* [1152,384], [1152] */
    const float* out_proj_w; const float* out_proj_b;   /* [384,384]          */
    const float* linear1_w;  const float* linear1_b;    /* [2048,384]         */
    const float* linear2_w;  const float* linear2_b;    /* [384,2048]         */
    const float* norm1_g; const float* norm1_b; const float* norm2_g; const float* norm2_b;
    /* backward only: fp32 transposed copies [in,out] and gradient accumulators */
    const float* in_proj_wt; const float* out_proj_wt; const float* linear1_wt; const float* linear2_wt;
    float* d_in_proj_w; float* d_in_proj_b; float* d_out_proj_w; float* d_out_proj_b; float* d_linear1_w; float* d_linear1_b;
    float* d_linear2_w; float* d_linear2_b; float* d_norm1_g; float* d_norm1_b; float* d_norm2_g; float* d_norm2_b;
} SaisTemporalLayerParams;

typedef struct SaisTemporalLayerFwd {
    int B, S;                            /* B sequences of S tokens: M = B * S rows; S <= 96                                */
    const float* z;                      /* in : f32 [M,384]                                                               */
    const unsigned char* key_pad;        /* in : u8 [B,S], 1 = masked key                                                  */
    float* qkv; float* ctx;              /* out: f32 [M,1152], [M,384] (saved for backward)                                */
    float* attn_avg;                     /* out, optional: f32 [B,S,S] head-averaged attention weights (the returned map)  */
    float* y1;                           /* out, optional (saved): f32 [M,384] input of norm1                               */
    float* z1; float* mean1; float* rstd1;   /* out: norm1 output (saved) and its statistics (optional)                     */
    float* h;                            /* out: f32 [M,2048] drop(relu(linear1(z1))) (saved)                               */
    float* y2;                           /* out, optional (saved): input of norm2                                           */
    float* z_out; float* mean2; float* rstd2;
    float p_drop; const unsigned long long* rng_state; unsigned site0;
} SaisTemporalLayerFwd;
int sais_temporal_layer_fwd(const SaisTemporalLayerParams* w, const SaisTemporalLayerFwd* a, void* workspace, size_t ws_bytes,
                            void* stream);

typedef struct SaisTemporalLayerBwd {
    int B, S;
    const float* z; const float* qkv; const float* ctx; const float* y1; const float* mean1; const float* rstd1;
    const float* z1; const float* h; const float* y2; const float* mean2; const float* rstd2; const unsigned char* key_pad;
    /* gradient wrt the layer OUTPUT = sum of nslab raw split-K slabs (slab_stride floats apart; the next layer's dx_slabs) +
     * dz_add; either part may be NULL / 0                                                                                  */
    const float* dz_slabs; int nslab; long slab_stride; const float* dz_add;
    /* gradient wrt the layer INPUT, in the same two-part form: dx_slabs f32 [sais_tgemm_nsplit(M,384,1152)][M][384] (raw dX of
     * in_proj) and dx_add f32 [M,384] (the residual path)                                                                  */
    float* dx_slabs; float* dx_add;
    float p_drop; const unsigned long long* rng_state; unsigned site0;
    /* optional (ABI 9): SaisTnItem[4] on the HOST.  When set, the layer's four weight / bias gradient GEMMs are NOT launched:
     * their items (operands inside `workspace` and the saved tensors) are written here, and the caller launches them later
     * with sais_gemm_tn_grouped_f32(items, n, B * S, 1, stream) — e.g. all layers of an encoder in ONE launch — and must keep
     * this call's `workspace` untouched until then (one workspace per layer).                                              */
    SaisTnItem* dw_items_out;
} SaisTemporalLayerBwd;
int sais_temporal_layer_bwd(const SaisTemporalLayerParams* w, const SaisTemporalLayerBwd* a, void* workspace, size_t ws_bytes,
                            void* stream);

/* ---------------------------------------------------------------- LayerNorm over dim = 384
 * nn.LayerNorm in Block / final norm (vision_transformer.py:99,103,107-113,212; eps 1e-6 from
 * vit_small :243-247) and norm1/norm2 of the post-norm TransformerEncoderLayer (prepare_model.py:74-81;
 * eps 1e-5).  Row r of x starts at x + r*ldx (so the CLS-only final norm is ldx = 197*384).
 * Outputs are optional (NULL): y_bf16 feeds the next MFMA GEMM, y_f32 is the post-norm residual,
 * mean/rstd are saved for backward.                                                              */
int sais_layernorm_fwd(const float* x, long ldx, int rows, int dim, const float* gamma, const float* beta,
                       float eps, void* y_bf16, long ldy16, float* y_f32, long ldy32, float* mean, float* rstd,
                       void* stream);
/* dy = dy_bf16 (optional) + dy_f32 (optional);  dx = dres (optional) + dLN(dy);  dgamma/dbeta += (atomics). */
int sais_layernorm_bwd(const void* dy_bf16, long lddy16, const float* dy_f32, long lddy32, const float* x, long ldx,
                       const float* mean, const float* rstd, const float* gamma, const float* dres, long lddres,
                       int rows, int dim, float* dx_f32, long lddx32, void* dx_bf16, long lddx16, float* dgamma,
                       float* dbeta, const float* rowscale16 /*optional: dx_bf16 = bf16(rowscale16[row] * dx), DropPath*/,
                       float* dx_f32_drop /*optional, ld = lddx32: dropout(dx) with mask element row * 384 + col of `site`:
                       the gradient that enters a dropped branch of the temporal encoder layer*/,
                       float p_drop, const unsigned long long* rng_state, unsigned site, void* stream);

/* ---------------------------------------------------------------- ViT spatial attention (197 tokens, 6 heads x 64)
 * Attention.forward core, vision_transformer.py:83-90: softmax(q k^T / 8) v per (frame, head).
 * qkv bf16 [frames*ntok, 3*384] laid out as the qkv Linear writes it (q | k | v, head-major inside).
 * out bf16 [frames*ntok, 384]; lse f32 [frames,6,ntok] (saved for backward, optional);
 * probs f32 [frames,6,ntok,ntok] (optional: get_last_selfattention, :216-223).
 * ntok = 197 (224 x 224 frames) or 37 (the 96 x 96 local crops of DINO pre-training, main_dino.py:658-663;
 * prepare_tokens at that size, vision_transformer.py:196-207); anything else is SAIS_ERR_ARG.     */
int sais_vit_attn_fwd(const void* qkv, long ldqkv, int frames, int ntok, void* out, long ldo, float* lse, float* probs,
                      void* stream);
/* dqkv bf16 [frames*ntok, 1152] from dout bf16 [frames*ntok, 384] and the saved forward output `out` (same shape:
 * delta_q = sum_d dout[q,d] out[q,d] is the softmax-backward row term, computed in the kernel).  One single-pass
 * kernel: P is rebuilt once per (query, key) from lse.  delta_ws is unused since ABI 2 (may be NULL).              */
int sais_vit_attn_bwd(const void* qkv, long ldqkv, const void* dout, long lddo, const void* out, long ldout,
                      const float* lse, float* delta_ws, int frames, int ntok, void* dqkv, long lddqkv, void* stream);
/* The LAST block's attention (ABI 8).  VisionTransformer.forward returns norm(x)[:, 0] (vision_transformer.py:209-214): of the
 * last block only the CLS row of every frame is read, so of its Attention.forward (:80-92) only the CLS QUERY is needed (keys
 * and values of all tokens still are).  out bf16 [frames, 384] (compact: one row per frame).  The backward takes the compact
 * dout bf16 [frames, 384], recomputes P and writes the WHOLE dqkv bf16 [frames*ntok, 1152]: dk, dv for every token, dq on the
 * CLS rows and zeros on the others.  Results equal sais_vit_attn_fwd / _bwd restricted to those rows (fp32 softmax here). */
int sais_vit_attn_cls_fwd(const void* qkv, long ldqkv, int frames, int ntok, void* out, long ldo, void* stream);
int sais_vit_attn_cls_bwd(const void* qkv, long ldqkv, const void* dout, long lddo, int frames, int ntok, void* dqkv,
                          long lddqkv, void* stream);

/* ---------------------------------------------------------------- optical-flow stage: RAFT correlation volume (ABI 8)
 * The reference renders its flow maps with ptlflow's `raft` ('things' checkpoint): SAIS/scripts/extract_representations.py
 * :33,62-67,221-252,267 and main.sh:18.  ptlflow 0.2.5 is a third-party dependency that is ABSENT from the reference tree
 * and this image: PARITY UNPINNED — these entries follow the published model (Teed & Deng, ECCV 2020) and are tested against
 * oracle/raft_oracle.py.  The all-pairs correlation itself is sais_gemm_nt_f32 on the [H W, 256] feature matrices.
 *   sais_raft_corr_pool: levels 1-3 of the correlation pyramid (2 x 2 average pooling over the last two dims of
 *       [rows, 1, H, W]; corr0 row r starts at corr0 + r * ld0) in one pass.  l1 / l2 / l3: f32 [rows, (H>>l) * (W>>l)].
 *   sais_raft_lookup: out f32 [B, 4 (2r+1)^2, H, W]; channel l (2r+1)^2 + a (2r+1) + b = level l sampled (bilinear, zeros
 *       outside, pixel coordinates) at (x / 2^l + a - r, y / 2^l + b - r) for (x, y) = coords[b', :, y', x'].          */
int sais_raft_corr_pool(const float* corr0, long ld0, int rows, int H, int W, float* l1, float* l2, float* l3, void* stream);
int sais_raft_lookup(const float* l0, long ld0, const float* l1, const float* l2, const float* l3, const float* coords,
                     int B, int H, int W, int radius, float* out, void* stream);
/* Convolution as a matrix-core GEMM (ABI 10; the RAFT encoders / update block, extract_representations.py:221-252 via ptlflow's
 * `raft`): cols f32 [rows, ld] <- im2col of ONE image x f32 [C, H, W]; row = output position oy * Wo + ox, column
 * (c * kh + ky) * kw + kx = the order of weight.view(Cout, C * kh * kw); column C*kh*kw holds 1.0 (append the bias to the weight
 * matrix as that column), the remaining columns and the rows >= Ho * Wo are zero (pad ld to a multiple of 64 and rows to a
 * multiple of 128 for sais_gemm_nt_f32).  y[Cout, Ho * Wo] = sais_gemm_nt_f32(A = weights [Cout, ld], B = cols) is NCHW.    */
int sais_im2col_f32(const float* x, int C, int H, int W, int kh, int kw, int sh, int sw, int ph, int pw,
                    float* cols, int ld, int rows, void* stream);

/* ---------------------------------------------------------------- ViT embedding glue
 * PatchEmbed + prepare_tokens, vision_transformer.py:116-131,196-207.                            */
int sais_patchify(const float* frames_f32 /*[F,3,side,side]*/, int frames, int side /* % 16 == 0 */,
                  void* patches_bf16 /*[F*(side/16)^2,768]*/, void* stream);
int sais_vit_cls_rows(const float* cls, const float* pos0, float* tokens, long frame_stride, int frames, int dim,
                      void* stream);
/* The classifier input of the linear probe with --avgpool_patchtokens (dino-main/eval_linear.py:166-170, n_last_blocks = 1):
 * x f32 [frames][ntok, dim] (frame_stride floats apart) is the residual stream after the last block; LayerNorm (gamma, beta, eps:
 * the final self.norm, vision_transformer.py:212) of all ntok rows, then y[f][2 j] = norm(x)[f][0][j] (the CLS token) and
 * y[f][2 j + 1] = mean over the ntok - 1 patch rows of norm(x)[f][1..][j]: the reference's cat(..., dim=-1).reshape
 * interleaves.  y f32, ldy >= 2 dim floats between frames.  One workgroup per frame, the patch mean summed in a fixed order. */
int sais_vit_cls_avgpool_norm(const float* x, long frame_stride, int frames, int ntok, int dim, const float* gamma,
                              const float* beta, float eps, float* y, long ldy, void* stream);
/* dcls/dpos += reductions of dtokens f32 [F,ntok,dim]; dpatch_bf16 [F*(ntok-1), dim] = rows 1.. (dY of patch GEMM) */
int sais_vit_embed_bwd(const float* dtokens, int frames, int ntok, int dim, float* dcls, float* dpos,
                       void* dpatch_bf16, void* stream);

/* Prefetch hint (ABI 8): reads [p, p + bytes) once with discarded loads so that the range is cache-resident (L2 /
 * Infinity Cache) for the kernels that follow — the temporal encoder's ~70 small launches otherwise each pay a first-touch
 * HBM round trip for weights the ViT's traffic evicted.  No effect on results.  p 16-B aligned.                       */
int sais_touch(const void* p, long bytes, void* stream);

/* ---------------------------------------------------------------- optimizer + weight shadows
 * optim.SGD(params, lr) — prepare_model.py:566-567, perform_training.py:155-158 (no momentum / wd).
 * param -= lr * grad_scale * grad; shadow_bf16 (optional) refreshed in the same pass.
 * param, grad 16-B aligned, shadow_bf16 8-B aligned: SAIS_ERR_ARG otherwise.                     */
int sais_sgd_step(float* param, const float* grad, void* shadow_bf16, long n, float lr, float grad_scale, void* stream);
int sais_cast_bf16(const float* src, void* dst_bf16, long n, void* stream);
int sais_transpose_cast_bf16(const float* src, int rows, int cols, void* dst_bf16 /*[cols,rows]*/, void* stream);
int sais_transpose_f32(const float* src, int rows, int cols, float* dst /*[cols,rows]*/, void* stream);
/* All transposed weight shadows of a model in ONE launch (the per-weight launches above are ~5 us each and a ViT-S
 * has 48 of them per optimizer step).  `items` is a DEVICE array, built once per model: the addresses are fixed.  */
typedef struct SaisTransposeItem {
    const float* src;        /* [rows, cols] f32                                              */
    void*        dst;        /* [cols, rows] bf16 (dst_is_f32 == 0) or f32                     */
    int rows, cols;
    int tile_begin;          /* prefix sum of ceil(rows/32)*ceil(cols/32) over preceding items */
    int reserved;
} SaisTransposeItem;
int sais_transpose_batch(const SaisTransposeItem* items_dev, int nitems, int total_tiles, int dst_is_f32, void* stream);
int sais_scale_f32(float* p, long n, float s, void* stream);

/* ---------------------------------------------------------------- frame preprocessing (uint8 frames -> ViT input)
 * SurgDataset.__getitem__, dino-main/main_dino.py:295-316 + the transform of extract_representations.py:158-162:
 * CenterCrop((height_frac*H, width_frac*W)) -> Resize((224,224)) -> ToTensor -> Normalize(mean, std), bit-identical to
 * torchvision 0.9.0 + Pillow's 8-bit bilinear resampler.  A plan holds the per-geometry coefficient tables on the
 * device (built once: allocation + upload); sais_preprocess_run only launches, so it can be graph-captured.
 * frames: device uint8 [F, H, W, 3] (RGB, as decoded); out: device float32 [F, 3, 224, 224].  `frames` must be 4-byte
 * aligned (the kernel reads it as dwords aligned from that pointer): sais_preprocess_run returns SAIS_ERR_ARG otherwise.
 * A slice of a batch whose frames have H*W*3 % 4 != 0 need not be; copy it first.
 * sais_preprocess_plan_describe is the geometry half of plan_create on the host alone (no device call, same refusals
 * and codes): info = left, top, cw, ch (the crop box), kx, ky (Pillow's ksize per axis), band (output rows per
 * workgroup: 8, 4, 2 or 1), nbands, max_rows (input rows of the tallest band), lds_bytes.  The horizontal pass runs
 * (kx + 3) >> 2 groups of four taps up to kx = 32 and a byte-wise loop past it.  Additive: the ABI version stays.    */
#define SAIS_PREPROCESS_INFO_INTS 10
/* 1 where Pillow resamples a cw x ch crop box vertical pass first (more than 100 rows per column, height reduced): the
 * plan then runs a second, plain kernel in that order (the passes round to uint8 in between, so the order shows).     */
int  sais_preprocess_vertical_first(int cw, int ch);
typedef struct SaisPreprocessPlan SaisPreprocessPlan;
int  sais_preprocess_plan_describe(int H, int W, double height_frac, double width_frac, int* info /* [10] */);
int  sais_preprocess_plan_create(int H, int W, double height_frac, double width_frac, const float* mean3,
                                 const float* std3, SaisPreprocessPlan** plan);
int  sais_preprocess_plan_box(const SaisPreprocessPlan* plan, int* box4 /* left, top, right, bottom */);
int  sais_preprocess_run(const SaisPreprocessPlan* plan, const unsigned char* frames, int nframes, float* out, void* stream);
void sais_preprocess_plan_destroy(SaisPreprocessPlan* plan);

/* ---------------------------------------------------------------- JPEG decode (compressed frames -> uint8 RGB)
 * Image.open(path) + np.asarray of SurgDataset.__getitem__, dino-main/main_dino.py:295-316, as used by the feature
 * extraction of extract_representations.py:158-162: baseline / extended-sequential Huffman JPEG, 8 bit, 3 components
 * as YCbCr, luma 1x1 / 2x1 / 2x2 over chroma 1x1, one interleaved scan, any restart interval.  Output is bit-identical
 * to libjpeg-turbo at Pillow's defaults (JDCT_ISLOW, fancy upsampling, jdcolor.c ycc_rgb_convert).  Anything else is
 * SAIS_JPEG_UNSUPPORTED at parse time and stays with the caller's host decoder.
 *
 * sais_jpeg_parse is a host function (no GPU): it walks the markers with every length checked against n.
 * sais_jpeg_decode only launches: the caller packs the files' bytes and one SaisJpegHeader per image (scan_offset
 * rebased to the packed buffer) into device memory and passes a workspace of sais_jpeg_workspace_bytes.  status[i] is
 * 0 for a decoded image, else a SAIS_JPEG_E* bit set: that image's output slot is undefined and the caller decodes
 * the file on the host.  Corrupt entropy data never reads outside its own file's bytes.                          */
#define SAIS_JPEG_UNSUPPORTED (-3)
#define SAIS_JPEG_E_CODE 1           /* invalid Huffman code, or a coefficient size beyond 8-bit baseline   */
#define SAIS_JPEG_E_RUN 2            /* AC run past k = 63                                                  */
#define SAIS_JPEG_E_MARKER 4         /* RST out of sequence, unexpected marker, or no marker ends the scan  */
#define SAIS_JPEG_E_SHORT 8          /* entropy data ends before the last MCU of a restart interval, or none */
#define SAIS_JPEG_E_SYNC 16          /* speculative Huffman decode did not synchronise within the pass bound */
#define SAIS_JPEG_E_RANGE 32         /* a dequantised coefficient or IDCT value out of range (no encoder's)   */
typedef struct SaisJpegHuff {        /* one DHT table in decode form                                         */
    uint16_t lookup[512];            /* next 9 bits -> (code length << 8) | symbol; 0 = a code longer than 9 */
    int32_t maxcode[18];             /* largest code of length l (l = 1..16), -1 if none                     */
    int32_t valoffset[18];           /* symbol of code c of length l = huffval[c + valoffset[l]]              */
    uint8_t huffval[256];
} SaisJpegHuff;
typedef struct SaisJpegHeader {
    int height, width;
    int hsamp, vsamp;                /* luma sampling factors (chroma is 1x1)                                */
    int restart_interval;            /* MCUs per restart interval, 0 = none                                  */
    int mcu_count, segments;         /* MCUs of the image; restart segments = ceil(mcu_count / interval)     */
    int qsel[3], dcsel[3], acsel[3]; /* table of each component                                              */
    int64_t scan_offset;             /* first byte of the entropy-coded data                                 */
    int64_t scan_bytes;              /* bytes from there to the end of the file (the scan ends at its marker) */
    uint16_t quant[4][64];           /* natural order                                                        */
    SaisJpegHuff dc[2], ac[2];
} SaisJpegHeader;
typedef struct SaisJpegBatch {
    int n, height, width;            /* images of one geometry                                                */
    int total_segments;              /* sum of the images' `segments`                                         */
    int64_t total_scan_bytes;        /* sum of the images' scan_bytes                                         */
    int64_t data_bytes;              /* size of the packed `data` buffer: every scan range must lie inside it */
} SaisJpegBatch;
int    sais_jpeg_parse(const unsigned char* data, size_t n, SaisJpegHeader* out);
size_t sais_jpeg_workspace_bytes(int n, int height, int width, int64_t total_scan_bytes, int total_segments);
int    sais_jpeg_decode(const SaisJpegBatch* batch, const unsigned char* data, const SaisJpegHeader* headers,
                        void* workspace, size_t workspace_bytes, unsigned char* out /* [n,H,W,3] */, int* status,
                        void* stream);
/* The same decode for a batch of mixed sizes: the same files, arithmetic and status bits, every image with the height and
 * width of its own header.  Image i is a contiguous uint8 [h_i, w_i, 3] at out + out_offset[i] (bytes; the layout is the
 * caller's, e.g. the running sum of h * w * 3).  Headers and offsets are passed twice, as the augment entries take their
 * table: the host copies size the workspace and the launch grids and are checked by the entry (SAIS_ERR_ARG and no launch
 * for an offset outside `out`, a workspace below sais_jpeg_mixed_workspace_bytes, scan bytes beyond data_bytes, n outside
 * 1..65535), the device copies are what the kernels read.  An image whose device header does not fit the regions and grids
 * the host copy sized, or whose device offset leaves `out`, gets SAIS_JPEG_E_MARKER and writes nothing.  The workspace grows
 * with the sum of the images' own sizes (coefficients and planes are laid out by prefix sums), not with n x the largest.   */
size_t sais_jpeg_mixed_workspace_bytes(const SaisJpegHeader* headers_host, int n);
int    sais_jpeg_decode_mixed(int n, const unsigned char* data, int64_t data_bytes, const SaisJpegHeader* headers_host,
                              const SaisJpegHeader* headers_dev, const int64_t* out_offset_host, const int64_t* out_offset_dev,
                              void* workspace, size_t workspace_bytes, unsigned char* out, size_t out_bytes, int* status,
                              void* stream);

/* ---------------------------------------------------------------- JPEG encode (uint8 RGB on the device -> scan bytes)
 * The counterpart of the decoder for images made on the device (attention heat maps, colour-coded flow): baseline sequential,
 * 8 bit, one interleaved scan without restart markers, the four Annex K Huffman tables, YCbCr 4:2:0 (subsampling 2) or 4:4:4
 * (subsampling 0), byte-identical to libjpeg-turbo at Pillow's defaults (rgb_ycc_convert, h2v2_downsample, jfdctint.c).
 * sais_jpeg_encode writes, for image i, the bytes from the first entropy-coded byte through the EOI marker to
 * out[i * out_stride ...] and their count to nbytes[i]; an image whose bytes do not fit out_stride gets nbytes[i] = -1 and
 * nothing is written to its slot.  The headers are the caller's (sais_amd/jpeg_enc.py: header).  sais_jpeg_encode_bound (a
 * host function) is the worst case of one image: blocks x the longest block code, doubled for byte stuffing, + padding + EOI.
 * SAIS_ERR_ARG: n outside 1..65535, a side outside 1..65535, another subsampling, a q entry of 0 or above 255, a workspace
 * smaller than sais_jpeg_encode_workspace_bytes, out_stride < 2. */
typedef struct SaisJpegEncParams {
    unsigned short q[2][64];         /* luma and chroma quantisation tables, natural order                   */
    int subsampling;                 /* 0 = 4:4:4, 2 = 4:2:0                                                  */
} SaisJpegEncParams;
size_t sais_jpeg_encode_bound(int height, int width, int subsampling);
size_t sais_jpeg_encode_workspace_bytes(int n, int height, int width, int subsampling);
int    sais_jpeg_encode(const unsigned char* rgb, int n, int height, int width, const SaisJpegEncParams* p, void* workspace,
                        size_t workspace_bytes, unsigned char* out, size_t out_stride, int* nbytes, void* stream);

/* ---------------------------------------------------------------- DINO multi-crop augmentation (uint8 frames -> views)
 * DataAugmentationDINO, dino-main/main_dino.py:633-679, on the frames SurgDataset.__getitem__ border-crops (:295-316):
 * per view RandomResizedCrop (BICUBIC) -> flip -> ColorJitter -> grayscale -> GaussianBlur -> solarize -> ToTensor ->
 * Normalize, bit-identical to the Pillow pipeline of sais_amd/dino_data.py for the same drawn parameters (one
 * SaisAugView per view, drawn on the host by dino_data.draw_view).
 *
 * The view table is passed twice: `views_host` is checked by the entry (SAIS_ERR_ARG and no launch for a size above
 * SAIS_AUG_MAX_SIZE, an empty box or one outside the border-cropped frame, a blur radius outside [0, 2], blend factors
 * outside [0, 2], an order that is no permutation, offsets outside the buffers), `views_dev` is the same table in device
 * memory, read by the kernels (which skip a view their copy shows to be out of range).  Both entries only launch.
 *   sais_augment_crop_resize  frames uint8 [nframes,height,width,3]; border4 = left, top, width, height of the border
 *                             crop; view i -> uint8 [size,size,3] at views_u8 + u8_offset
 *   sais_augment_color        uint8 views -> float32 [3,size,size] at out + out_offset (elements); lut = device float
 *                             [3][256], the normalised value of every byte per channel
 *   sais_augment_workspace_bytes  size of the uint8 view buffer the table addresses (0 = bad table)                 */
#define SAIS_AUG_MAX_SIZE 224
typedef struct SaisAugView {
    int frame;                       /* index into frames                                                     */
    int box[4];                      /* left, top, right, bottom in the border-cropped frame                  */
    int size;                        /* the view is size x size                                               */
    int flip, jitter;
    int order[4];                    /* jitter ops in application order: 0 brightness 1 contrast 2 saturation 3 hue */
    float brightness, contrast, saturation;
    int hue_shift;                   /* added to the H channel mod 256                                        */
    int gray, blur;
    float blur_radius;               /* GaussianBlur radius, used when blur != 0                              */
    int solarize, reserved;
    int64_t u8_offset;               /* bytes, into views_u8                                                  */
    int64_t out_offset;              /* float elements, into out                                              */
} SaisAugView;
size_t sais_augment_workspace_bytes(const SaisAugView* views_host, int nviews);
int    sais_augment_crop_resize(const unsigned char* frames, int nframes, int height, int width, const int* border4,
                                const SaisAugView* views_host, const SaisAugView* views_dev, int nviews,
                                unsigned char* views_u8, size_t views_u8_bytes, void* stream);
int    sais_augment_color(const unsigned char* views_u8, size_t views_u8_bytes, const SaisAugView* views_host,
                          const SaisAugView* views_dev, int nviews, const float* lut, float* out, size_t out_elems,
                          void* stream);

/* ---------------------------------------------------------------- image-folder transforms (uint8 images -> float32 batches)
 * The Pillow transforms of the evaluation tools' datasets (knn.EvalImageFolder: Resize(256, bicubic) + CenterCrop(224);
 * linear.TrainImageFolder: crop box, bilinear to 224 x 224, flip; retrieval.ImgListDataset: bicubic to imsize x imsize), each
 * followed by ToTensor + Normalize, on decoded images of any size packed in one uint8 buffer.  Image i -> float32
 * [3,out_h,out_w] at out + out_offset (elements), bit-identical to
 *   img.crop(box).resize((rw, rh), filter).crop((win_left, win_top, win_left + out_w, win_top + out_h)) [.transpose(FLIP_LEFT_RIGHT)]
 * through `lut` (device float [3][256], the normalised value of every byte per channel).  Only the window is evaluated.
 * The table is passed twice, as the augment entries take theirs: SAIS_ERR_ARG and nothing launched for out_h / out_w outside
 * 1..SAIS_IMG_MAX_OUT, an empty box or one outside the image, a window that leaves the resampled image, a filter that is
 * neither, an offset outside the buffers, or a descriptor whose one-row band does not fit in LDS (a downscale of several
 * hundred to one: sais_image_transform_fits, a host function, answers 0 for it, so a caller can route it elsewhere first). */
#define SAIS_IMG_MAX_OUT 512
#define SAIS_IMG_BILINEAR 0
#define SAIS_IMG_BICUBIC 1
typedef struct SaisImgXform {
    int64_t src_offset;              /* bytes, into src: the image is uint8 [src_h, src_w, 3]                  */
    int src_h, src_w;
    int box[4];                      /* left, top, right, bottom: cropped first                               */
    int rw, rh;                      /* the box is resampled to rw x rh                                        */
    int win_left, win_top;           /* origin of the out_w x out_h window inside the resampled image         */
    int filter;                      /* SAIS_IMG_BILINEAR (support 1) or SAIS_IMG_BICUBIC (support 2, a = -0.5) */
    int flip;
    int64_t out_offset;              /* float elements, into out                                              */
} SaisImgXform;
int    sais_image_transform_fits(const SaisImgXform* d, int out_h, int out_w);
int    sais_image_transform(const unsigned char* src, size_t src_bytes, const SaisImgXform* table_host,
                            const SaisImgXform* table_dev, int n, int out_h, int out_w, const float* lut, float* out,
                            size_t out_elems, void* stream);

/* ---------------------------------------------------------------- thumbnail(LANCZOS) of the retrieval loader (csrc/thumbnail.hip)
 * retrieval.OxfordParisDataset: Image.open(fh).convert("RGB"), img.thumbnail((imsize, imsize), Image.LANCZOS), ToTensor +
 * Normalize, on decoded images of any size packed in one uint8 buffer.  Additive entries: the ABI version does not change.
 * After convert() the image is a plain Image, so Image.thumbnail (Pillow 12.2) uses no JPEG draft mode; it is
 *   (x, y) = the aspect-preserving size (Image.thumbnail, round_aspect); not larger than the image: left untouched
 *   fx = int(W / x / 2.0) or 1, fy = int(H / y / 2.0) or 1          (Image.resize, reducing_gap = 2.0)
 *   img.reduce((fx, fy)) where a factor exceeds 1                    (Image.reduce / Reduce.c: box average, rw x rh =
 *                                                                     ceil(W / fx) x ceil(H / fy), last column / row partial)
 *   resize((x, y), LANCZOS, box = (0, 0, W / fx, H / fy))            (Resample.c: precompute_coeffs with lanczos_filter,
 *                                                                     normalize_coeffs_8bpc, ImagingResampleInner; the box
 *                                                                     ends are C floats: _imaging.c parses "(ffff)")
 * Image.resize ends with a branch for tall, narrow images: where the reduced image has rh > 100 * rw and out_h < rh, the vertical
 * pass runs first, as a resize of its own.  These entries run the horizontal pass first, so they REFUSE that geometry
 * (SAIS_ERR_ARG; sais_thumbnail_fits answers 0) and a caller routes such an image to Pillow.
 * Image i -> float32 [3, out_h, out_w] at out + out_offset (elements) through `lut` (device float [3][256]), bit-identical.
 * lanczos_filter is sinc(x) * sinc(x / 3) from the C library's sin in double; no kernel evaluates it.  sais_lanczos_rows, a
 * host function, writes the rows of one axis: bounds int [out][2] (first input index, taps) and coefs int [out][ksize] for
 * `src_size` samples reduced by `factor` and resampled to `out_size`.  It returns ksize; 0 where Pillow skips the pass (same
 * size, whole box: nothing is written); with bounds = coefs = NULL it only answers ksize.  In the coefficient buffer of
 * sais_thumbnail the rows of an axis lie at c?_offset (ints) as [out][2] bounds followed by [out][k?] coefficients; k? = 0
 * says the pass is skipped (the side must then equal the reduced side; both 0 with factors 1: a normalised copy).
 * The table and the coefficient buffer are passed twice, as the augment entries take their table: the host copies are checked
 * (every tap inside the reduced image, every band within its LDS rows), the device copies are read.  SAIS_ERR_ARG and nothing
 * launched for n outside 1..65535, output sides outside 1..SAIS_THUMB_MAX_OUT, source sides above 65535 or more than 2^28
 * pixels, a factor below 1 or fx * fy above 65536, rw / rh that are not the reduced size, the vertical-first geometry above, an offset outside a buffer, or a
 * one-row band that does not fit in LDS (sais_thumbnail_fits, a host function, answers 0 for a geometry that is refused, so a
 * caller can route it elsewhere first).  SAIS_THUMB_MAX_OUT is 1024: the coefficient rows stay in global memory, LDS holds
 * only the horizontally resampled rows of a band ((2 + ky) * out_w * 3 bytes for a one-row band, 83 KiB at 1024 and ky = 25).
 * The workspace holds the reduced images at ws_offset (bytes, chosen by the caller; unused with factors 1);
 * sais_thumbnail_workspace_bytes answers the bytes a table needs (0: a refused table). */
#define SAIS_THUMB_MAX_OUT 1024
typedef struct SaisThumb {
    int64_t src_offset;              /* bytes, into src: the image is uint8 [src_h, src_w, 3]                  */
    int src_h, src_w;
    int fx, fy;                      /* Image.reduce factors, >= 1                                             */
    int rw, rh;                      /* ceil(src_w / fx), ceil(src_h / fy)                                     */
    int64_t ws_offset;               /* bytes, into ws: the reduced image uint8 [rh, rw, 3]                    */
    int out_w, out_h;
    int kx, ky;                      /* taps per coefficient row; 0 = the pass is skipped                      */
    int64_t cx_offset, cy_offset;    /* ints, into coef                                                        */
    int64_t out_offset;              /* float elements, into out                                               */
} SaisThumb;
int    sais_lanczos_rows(int src_size, int factor, int out_size, int* bounds, int* coefs, int ksize);
int    sais_thumbnail_fits(const SaisThumb* d);
size_t sais_thumbnail_workspace_bytes(const SaisThumb* table_host, int n);
int    sais_thumbnail(const unsigned char* src, size_t src_bytes, const SaisThumb* table_host, const SaisThumb* table_dev, int n,
                      const int* coef_host, const int* coef_dev, size_t coef_ints, unsigned char* ws, size_t ws_bytes,
                      const float* lut, float* out, size_t out_elems, void* stream);

/* ---------------------------------------------------------------- temporal encoder glue (dim 384, 4 heads x 96)
 * prepareInputForTransformer, prepare_model.py:179-195: z[b,0] = frame_cls, z[b,1+t] = x[b,t] + pos[t]
 * (out of place: the reference's in-place += on the caller's tensor is NOT reproduced).          */
int sais_temporal_prepare_fwd(const float* x, long x_clip_stride, long x_frame_stride, const float* pos /*[T,384]*/,
                              const float* cls, int B, int T, float* z_f32, void* z_bf16 /*optional*/, void* stream);
/* backward: dz = dz_f32 + sum_z slabs[z] (either may be NULL; slabs = the raw split-K output of the in_proj dX GEMM) */
int sais_temporal_prepare_bwd(const float* dz_f32, const float* slabs, int nslab, long slab_stride, int B, int T, float* dx,
                              long dx_clip_stride, long dx_frame_stride, int accumulate, float* dpos, float* dcls,
                              void* stream);
/* nn.MultiheadAttention core of the torch-1.8 post-norm TransformerEncoderLayer (prepare_model.py:74-81,
 * called at :213): q scaled by 96^-0.5, key_pad[b][j] != 0 -> -inf, softmax, (dropout,) P v — exact fp32 on the matrix
 * cores (v_mfma_f32_16x16x4_f32), one workgroup per (sequence, head).
 * attn_avg f32 [B,S,S] (optional) = P averaged over the 4 heads = the README.md:43-48 attention map. */
#define SAIS_TEMPORAL_MAX_S_FWD 96
#define SAIS_TEMPORAL_MAX_S_BWD 96
int sais_temporal_attn_fwd(const float* qkv /*[B*S,1152]*/, const unsigned char* key_pad /*[B,S]*/, int B, int S,
                           float* ctx /*[B*S,384]*/, float* attn_avg, float p_drop, const unsigned long long* rng_state,
                           unsigned site, void* stream);
/* dctx = sum over nslab raw split-K slabs (slab_stride floats apart) of the out_proj dX GEMM; nslab = 1: a plain tensor */
int sais_temporal_attn_bwd(const float* qkv, const unsigned char* key_pad, int B, int S, const float* dctx, int nslab,
                           long slab_stride, float* dqkv /*[B*S,1152]*/, float p_drop, const unsigned long long* rng_state,
                           unsigned site, void* stream);
/* The same attention for 1 <= S <= SAIS_TEMPORAL_LONG_MAX_S (the 2000-row position table + CLS; csrc/tattn_long.hip): keys and
 * values stream through LDS in 64-row tiles, a workgroup owns 64 queries.  Same arguments, same mask element index (in 64 bits),
 * same Philox state.  attn_avg needs NO pre-zeroing and is bit-reproducible (fixed-order head sum), as are ctx and dqkv.  The
 * backward takes a workspace of sais_temporal_attn_long_bwd_workspace_bytes(B, S) bytes, 16-B aligned (the slab sum of dctx and
 * the row statistics its first launch leaves for the second); no float atomics.  SAIS_ERR_ARG and nothing launched for S out
 * of range, B > 65535, p_drop outside [0, 1), p_drop > 0 without rng_state, slab_stride & 3, or a workspace too small.
 * sais_temporal_layer_fwd / _bwd use these for S > SAIS_TEMPORAL_MAX_S_FWD and the resident kernels up to it. */
#define SAIS_TEMPORAL_LONG_MAX_S 2001
size_t sais_temporal_attn_long_bwd_workspace_bytes(int B, int S);
int sais_temporal_attn_fwd_long(const float* qkv, const unsigned char* key_pad, int B, int S, float* ctx,
                                float* attn_avg /*optional [B,S,S]*/, float p_drop, const unsigned long long* rng_state,
                                unsigned site, void* stream);
int sais_temporal_attn_bwd_long(const float* qkv, const unsigned char* key_pad, int B, int S, const float* dctx, int nslab,
                                long slab_stride, float* dqkv, float p_drop, const unsigned long long* rng_state, unsigned site,
                                void* workspace, size_t workspace_bytes, void* stream);
/* Train mode (model.train(), train.py:59): nn.TransformerEncoderLayer's default dropout = 0.1 (prepare_model.py:75) acts at
 * four sites per layer: on the attention weights (p_drop above: after the softmax, before P v; the returned map is the
 * dropped one, as in torch 1.8), after out_proj (dropout1), after the ReLU (dropout) and after linear2 (dropout2).
 * Masks come from Philox4x32-10 keyed by rng_state = {seed, offset} in DEVICE memory (graph replays draw fresh masks:
 * sais_rng_advance is a graph node), the site id and the element index; forward and backward regenerate them, nothing is
 * stored.  sais_dropout_f32: out = (resid ? resid : 0) + x * keep / (1 - p) (out may alias x); applied to a gradient with
 * the same (state, site) it is the backward of itself.  sais_dropout_mask exports the keep mask (tests feed it to the oracle).
 * The stream of numbers is this library's, not torch's: a torch run with the same seed draws different masks.
 * The rule, for every site: the draw of element idx is word idx % 4 of Philox4x32-10 at counter {idx / 4 low word, idx / 4
 * high word, site, offset low word} and key {seed low word, seed high word ^ offset high word}; the element is kept  <=>
 * draw >= (unsigned)min(p * 2^32, 4294967040) with the product in fp32; kept values are scaled by the fp32 1 / (1 - p).   */
int sais_rng_advance(unsigned long long* state /*{seed, offset}*/, void* stream);
int sais_dropout_f32(const float* x, const float* resid /*optional*/, float* out, long n, float p,
                     const unsigned long long* rng_state, unsigned site, void* stream);
int sais_dropout_mask(unsigned char* mask, long n, float p, const unsigned long long* rng_state, unsigned site, void* stream);
/* DropPath / stochastic depth of the ViT blocks in train mode (vision_transformer.py:27-46,105-113; rates
 * linspace(0, drop_path_rate, depth), :150): x = x + keep_f / (1 - p) * branch(x), one Bernoulli(1 - p) draw per sample f.
 * sais_droppath_scales fills the per-ROW scale arrays of `nbranch` branches in one launch (out f32 [nbranch][samples *
 * rows_per_sample]; keep from the same Philox state as the dropout, site = site0 + branch, element = sample); they are
 * the `rowscale` of SaisGemm (SAIS_EPI_BIAS_RESID_F32) / SaisGemmLn forward and the `rowscale16` of the LayerNorm backward
 * entry points.  sais_cast_bf16_rows: dst = bf16(rowscale[row] * src) (the first branch gradient of the backward pass). */
int sais_droppath_scales(float* out, const float* rates_dev /*[nbranch]*/, int nbranch, int samples, int rows_per_sample,
                         const unsigned long long* rng_state, unsigned site0, void* stream);
int sais_cast_bf16_rows(const float* src, const float* rowscale, void* dst_bf16, long rows, int dim, void* stream);

/* ---------------------------------------------------------------- head + SupCon / prototype loss
 * fullModel.forward Prototypes branch, prepare_model.py:215,220,381-416:
 *   rep = mean_s relu(z_rgb[b,s,0]) (+ mean_s relu(z_flow[b,s,0]));  emb = linear(relu(rep))   (256 outputs);
 *   s runs over the `nsnippets` snippets of clip b (:381-382; sequences b*nsnippets + s of the encoder output).
 * The two streams may have different padded lengths (sequence strides): at inference the flow stream
 * has 1-2 frames per 15-frame window (prepare_dataset.py:2660-2666).                              */
int sais_head_fwd(const float* z_rgb, const float* z_flow, long clip_stride, long clip_stride_flow, int B,
                  int nsnippets, const float* W /*[256,384]*/, const float* bias,
                  const unsigned char* use_b /*[B] or NULL*/, const float* WB, const float* biasB,
                  float* rep /*[B,384] saved*/, float* emb /*[B,256]*/, void* stream);
/* use_b: multi-domain models ('+' in the domain name, two-stream, prepare_model.py:405-414): clips flagged 1 (domain !=
 * 'NH_02') go through linearB = (WB, biasB) instead of linear = (W, bias); the backward routes dz through the same head
 * and accumulates each clip's weight / bias gradient into the head it used (dW / dbias or dWB / dbiasB).              */
int sais_head_bwd(const float* demb, const float* W, const float* rep, const float* z_rgb, const float* z_flow,
                  long clip_stride, long clip_stride_flow, int B, int nsnippets, const unsigned char* use_b,
                  const float* WB, float* dW, float* dbias, float* dWB, float* dbiasB, float* dz_rgb, float* dz_flow,
                  void* stream);
/* MIL pathway, inference direction (fullModel.forward task 'MIL', prepare_model.py:356-361; its training raises inside the
 * reference).  sais_mil_forward: tokens[b, s] = relu(z_rgb[(b * ns + s), CLS row]) + clip_pos[s] = the input of
 * getClipReps' clip-level encoder (:452-460; z_rgb = frame-encoder output, seq_stride floats between sequences).  The
 * encoder itself is the same kernel chain as the frame encoder on transEncoderClip's weights (no mask, no CLS).
 * sais_mil_head: reps = relu(enc) (:465), then MIL_Head (:470-488): gated attention over the snippets per class
 * (calcAttention :131-138), video representation and score (:140-148).  attention is [nclasses][B][nsnippets].        */
int sais_mil_forward(const float* z_rgb, long seq_stride, const float* clip_pos /*[ns,384]*/, int B, int nsnippets,
                     float* tokens /*[B*ns,384]*/, void* stream);
int sais_mil_head(const float* enc /*[B*ns,384]*/, int B, int nsnippets, int nclasses, const float* WA, const float* bA,
                  const float* WB, const float* bB, const float* w_att /*[3,256]*/, const float* b_att /*[3]*/,
                  const float* w_fin /*[3,384]*/, const float* b_fin /*[3]*/, float* reps, float* logits /*[B,C]*/,
                  float* attention, void* stream);
/* Optional importance head (-il): importance_function = Linear(384 -> 1) on the ReLU'd encoder output sequence,
 * prepare_model.py:55-56,419-421.  out[m] = w . relu(z[m,:]) + b.  bwd ACCUMULATES into dz / dw / db.        */
int sais_importance_fwd(const float* z /*[M,384] pre-ReLU*/, const float* w, const float* b, int M, float* out, void* stream);
int sais_importance_bwd(const float* dlogit /*[M]*/, const float* z, const float* w, int M, float* dz, float* dw,
                        float* db, void* stream);
/* calcImportanceLoss, prepare_miscellaneous.py:48-60 (quirks kept: scalar mean BCE broadcast against the inverted
 * mask with its last entry dropped; mean over label-0 samples, NaN if none).  logits [B,T+1] (slot 0 = CLS),
 * target [B,T], ipad [B,T+1] (1 = masked).  dlogits (optional) [B,T+1] = scale * d loss / d logits; with no
 * label-0 sample the loss is NaN and dlogits is exactly 0, as autograd of the mean over an empty selection gives. */
int sais_importance_loss(const float* logits, const float* target, const unsigned char* ipad, const int* labels,
                         int B, int T, float* loss, float* dlogits, float scale, void* stream);

/* calcNCELoss / getProbs, prepare_miscellaneous.py:14-46,111-126: sim = s_hat p_hat^T (the class logits),
 * probs = softmax(sim), loss = -mean log probs[i, label_col[i]].  With demb != NULL also the gradients:
 * demb (written) and dprotos (accumulated), both scaled by loss_scale.                            */
int sais_nce(const float* emb /*[B,256]*/, const float* protos /*[C,256]*/, const int* label_col, int B, int C,
             float* sim, float* probs, float* loss, float* demb, float* dprotos, float loss_scale, void* stream);

/* ================================================================ DINO pre-training objective
 * SAIS/scripts/dino-main/main_dino.py trains the ViT-S/16 encoder by self-distillation: train_one_epoch (:517-576) runs
 * teacher(images[:2]) and student(images) through utils.MultiCropWrapper (utils.py:595-630; 2 global 224 x 224 crops + N
 * local 96 x 96 crops), DINOHead (vision_transformer.py:257-291), DINOLoss (:579-630), utils.clip_gradients
 * (utils.py:132-141), utils.cancel_gradients_last_layer (:144-149), AdamW on utils.get_params_groups (:633-645) and the
 * EMA teacher update (:563-566).  The ViT and the head's nn.Linear layers run on the GEMM / attention entry points
 * above (sais_vit_attn_* with ntok 197 / 37, sais_gemm_nt_f32, sais_gemm_tn_f32); the entries below are the rest.  */

/* lse[r] = log sum_k exp((x[r][k] - center[k]) * scale), center may be NULL.  Teacher rows: scale = 1 / temp with the
 * centre (F.softmax((teacher_output - self.center) / temp), :605); student rows: scale = 1 / student_temp, no centre
 * (F.log_softmax(student_out[v]), :600,614).  n % 4 == 0.                                                            */
int sais_dino_row_lse(const float* x, long ld, int rows, int n, float scale, const float* center, float* lse, void* stream);
/* DINOLoss.forward (:596-619) and its gradient.  student f32 [ncrops*B, n] (row v*B + b = view v of sample b, the
 * chunk(ncrops) layout), teacher f32 [2*B, n], s_lse / t_lse from sais_dino_row_lse.  Writes
 *   loss[0]  = 1/n_terms sum_{iq < 2} sum_{v != iq} mean_b sum_k -q_iq[b,k] log_softmax(s_v[b] / student_temp)[k]
 *   dlogits  = d loss / d student   (f32 [ncrops*B, n])
 * partials: workspace of sais_dino_loss_partials(B, n) floats (fixed-order reduction, no atomics).                  */
int sais_dino_loss_partials(int B, int n);
int sais_dino_loss(const float* student, long lds, const float* teacher, long ldt, const float* center, const float* s_lse,
                   const float* t_lse, int B, int ncrops, int n, float student_temp, float teacher_temp, float* dlogits,
                   long ldd, float* partials, float* loss, void* stream);
/* DINOLoss.update_center (:621-630) in two steps so that the data-parallel all-reduce of the [1, n] column sums
 * (dist.all_reduce(batch_center), :627) sits between them:  out[k] = sum_r x[r][k];  then
 * center = center * momentum + colsum * inv_count * (1 - momentum),  inv_count = 1 / (rows * world_size).           */
int sais_dino_colsum(const float* x, long ld, int rows, int n, float* out, void* stream);
int sais_dino_center_ema(float* center, const float* colsum, int n, float momentum, float inv_count, void* stream);

/* DINOHead.forward pieces (vision_transformer.py:287-291): nn.GELU() between the MLP's Linear layers (f32 in / out; the
 * backward is du = dh * gelu'(u)), F.normalize(x, dim=-1, p=2) (eps 1e-12) and nn.utils.weight_norm of the last layer
 * (:277-281: w = g v / ||v||_row; _bwd ACCUMULATES dv and, when dg != NULL, dg).  One wave per row, dim <= 1024.      */
int sais_gelu_fwd_f32(const float* u, float* h, long n, void* stream);
/* bf16x3 operand image of an f32 matrix [rows, cols] for sais_gemm_nt: dst bf16 [rows, 3 * cols] = [hi | hi | lo] (A side,
 * b_side = 0) or [hi | lo | hi] (B side), hi = bf16(x), lo = bf16(x - hi): one bf16 GEMM over K' = 3 K then sums the
 * three products of the "bf16x3" arithmetic in fp32.  Used for the head's 256 -> 65536 last layer (the logits).        */
int sais_split_bf16x3(const float* src, long ld, int rows, int cols, void* dst_bf16, int b_side, void* stream);
int sais_gelu_bwd_f32(const float* dh, const float* u, float* du, long n, void* stream);
int sais_l2norm_fwd(const float* z, int rows, int dim, float eps, float* out, float* inv, void* stream);
int sais_l2norm_bwd(const float* dout, const float* out, const float* inv, int rows, int dim, float eps, float* dz, void* stream);
int sais_weight_norm_fwd(const float* v, const float* g, int rows, int dim, float* w, float* inv, void* stream);
int sais_weight_norm_bwd(const float* dw, const float* v, const float* g, const float* inv, int rows, int dim, float* dv,
                         float* dg, void* stream);

/* VisionTransformer.interpolate_pos_encoding (vision_transformer.py:174-194) for crops that are not 224 x 224: the
 * bicubic resampling of the 14 x 14 positional grid is a fixed linear map Wm f32 [nout, nin] (built once per
 * resolution by the host, sais_amd/vit.py); out [1 + nout, dim]: row 0 = pos row 0 (the CLS position, :179),
 * rows 1.. = Wm . pos[1..].  _bwd ACCUMULATES the transpose into dpos [1 + nin, dim].                              */
int sais_pos_interp_fwd(const float* Wm, int nout, int nin, const float* pos, int dim, float* out, void* stream);
int sais_pos_interp_bwd(const float* Wm, int nout, int nin, const float* dout, int dim, float* dpos, void* stream);

/* The optimizer tail of train_one_epoch over one flat parameter buffer (sais_amd/flat.py), cut by the host into chunks
 * of <= sais_opt_chunk_elems() elements that never straddle a tensor ("segment").
 * sais_grad_norms: norms[seg] = scale * ||grad of tensor seg||_2 — what utils.clip_gradients computes per parameter
 *   (:135-136); seg_first_chunk int [nseg + 1]; partial_ws f32 [nchunks].  scale / SaisAdamW.grad_scale = 1 / world_size
 *   when `grad` holds the all-reduced SUM over the data-parallel ranks (DDP averages, main_dino.py:413), else 1.
 * sais_adamw_ema_step, per element of every chunk, in this order:
 *   scale  g *= grad_scale
 *   clip   g *= min(1, clip / (norm + 1e-6))                       utils.py:137-140  (clip = 0: off, main_dino.py:547)
 *   AdamW  p *= 1 - lr * wd (segments flagged SAIS_OPT_DECAY: the `regularized` group, utils.py:633-645; the others
 *          decay 0);  m = lerp(m, g, 1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 *          p -= lr / bc1 * m / (sqrt(v) / sqrt_bc2 + eps)          torch.optim.AdamW, main_dino.py:446,556
 *          bc1 = 1 - beta1^t, sqrt_bc2 = sqrt(1 - beta2^t) per step-count class: class 1 (SAIS_OPT_CLASS1) = the last
 *          layer, whose step count lags while frozen1 != 0 (utils.cancel_gradients_last_layer, utils.py:144-149:
 *          p.grad = None -> the optimizer skips the tensor entirely); SAIS_OPT_NO_GRAD: requires_grad False (weight_g)
 *   EMA    teacher = teacher * ema_m + (1 - ema_m) * p              main_dino.py:563-566 (teacher may be NULL)
 *   and the bf16 MFMA shadows of both (param16 / teacher16, may be NULL) are refreshed in the same pass.            */
#define SAIS_OPT_DECAY 1
#define SAIS_OPT_CLASS1 2
#define SAIS_OPT_NO_GRAD 4
typedef struct SaisOptChunk { long off; int len; int seg; } SaisOptChunk;
typedef struct SaisAdamW {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;     /* flat f32 buffers, same layout   */
    float* teacher; void* param16; void* teacher16;                         /* optional                        */
    const SaisOptChunk* chunks; int nchunks;                                /* device table                    */
    const int* seg_flags; const float* norms;                               /* device, per segment             */
    float clip, lr, weight_decay, beta1, beta2, eps;
    float bc1[2], sqrt_bc2[2]; int frozen1;
    float ema_m;
    float grad_scale;
} SaisAdamW;
int sais_opt_chunk_elems(void);
int sais_grad_norms(const float* grad, const SaisOptChunk* chunks, int nchunks, const int* seg_first_chunk, int nseg,
                    float scale, float* partial_ws, float* norms, void* stream);
int sais_adamw_ema_step(const SaisAdamW* a, void* stream);

/* ================================================================ weighted k-NN evaluation (dino-main/eval_knn.py:143-182)
 * The frozen-feature classifier without the [Nq, Nt] similarity matrix (sais_amd/csrc/knn.hip, host: sais_amd/knn.py).
 * sais_knn_search: test f32 [Nq, D] and train [Nt, D], rows L2-normalised; train is f32, or with train_is_split != 0 the
 *   bf16 [Nt, 3 D] B-side image of sais_split_bf16x3 (an index is split once and reused; both forms give the same bits).
 *   Writes the kmax largest dot products of every test row, val f32 [Nq, kmax] and idx i32 [Nq, kmax], sorted by
 *   (value descending, train index ascending); the same order decides which of several equal values are kept at the cut.
 *   Arithmetic: bf16x3 on the matrix cores, one K order for every pair, no atomics: duplicate train rows get bit-equal
 *   values and a call is bit-reproducible.  1 <= kmax <= SAIS_KNN_MAX_K, kmax <= Nt, D % 64 == 0, D <= SAIS_KNN_MAX_DIM;
 *   any Nq >= 1 and Nt.  workspace: sais_knn_workspace_bytes(Nq, Nt, kmax) bytes (candidate lists per test row and train
 *   split; it does not grow with Nt once the split count has reached its cap).
 * sais_knn_vote: for each of ks[0] < ... < ks[m-1] <= kmax (host array, m <= SAIS_KNN_MAX_KS)
 *   votes_j[c] = sum over the first ks[j] neighbours n with train_labels[idx[n]] == c of expf(val[n] / T), added in fp32
 *   in neighbour order; pred i32 [m, Nq, 5] = the five best classes by (vote descending, class ascending), which is
 *   torch.sort(descending=True) on the CPU; votes f32 [m, Nq, num_classes] is written when not NULL.
 *   num_classes <= SAIS_KNN_MAX_CLASSES.                                                                              */
#define SAIS_KNN_MAX_K 256
#define SAIS_KNN_MAX_DIM 1536
#define SAIS_KNN_MAX_CLASSES 4096
#define SAIS_KNN_MAX_KS 8
size_t sais_knn_workspace_bytes(int Nq, int Nt, int kmax);
int sais_knn_search(const float* test, const void* train, int train_is_split, int Nq, int Nt, int D, int kmax, float* val,
                    int* idx, void* workspace, size_t workspace_bytes, void* stream);
int sais_knn_vote(const float* val, const int* idx, int Nq, int kmax, const int* train_labels, int Nt, int num_classes,
                  float T, const int* ks, int m, int* pred, float* votes, void* stream);

/* ================================================================ linear probe on frozen features (dino-main/eval_linear.py)
 * H classifier heads (1 <= H <= SAIS_PROBE_MAX_HEADS) that differ only in learning rate are trained from one feature batch
 * (sais_amd/csrc/probe.hip, host: sais_amd/linear.py).  All tensors f32: X [B, Dm], W [H, C, Dm], b [H, C], Z [H, B, C];
 * 1 <= B <= SAIS_PROBE_MAX_ROWS, 1 <= C <= SAIS_PROBE_MAX_CLASSES, Dm % 64 == 0, Dm <= SAIS_PROBE_MAX_DIM.  Arithmetic: the
 * exact f32-input MFMA, one accumulator chain per output element in ascending k; no atomics: bit-reproducible.
 * sais_probe_logits: Z[h] = X W[h]^T + b[h] (LinearClassifier.forward, eval_linear.py:246-251).  A row's logits do not
 *   depend on B, on the row's position or on H.
 * sais_probe_ce: nn.CrossEntropyLoss with mean reduction (eval_linear.py:176, :216) per (head, row): loss_rows f32 [H, B] =
 *   lse - z[target]; top5 i32 [H, B, 5] (NULL allowed with train) = the five best classes by (logit descending, class
 *   ascending), slots >= C hold -1 (utils.accuracy, eval_linear.py:218-221); with train != 0, Z is replaced in place by
 *   dZ = (softmax - onehot) / B.  loss f32 [H] (NULL allowed with train) = mean of loss_rows over the rows, added in row
 *   order by a second small launch.  targets i32 [B] in [0, C).
 * sais_probe_update: per 64 x 64 tile of W[h], G = dZ[h]^T X over the B rows in ascending order, then torch.optim.SGD with
 *   momentum (eval_linear.py:103-108; dampening 0, weight decay 0): m = momentum m + G, W -= lr[h] m; a zero-initialised
 *   buffer gives torch's first step (buf = grad).  The owners of feature tile 0 do the same for b with db[c] = sum over rows
 *   of dZ[r][c] in row order.  dW is never stored.  With loss / loss_rows set, loss[h] = mean of loss_rows[h] in row order
 *   rides in this launch (a training step is then three launches: logits, ce, update).  0 <= momentum < 1, lr[h] >= 0.  */
#define SAIS_PROBE_MAX_HEADS 8
#define SAIS_PROBE_MAX_ROWS 1024
#define SAIS_PROBE_MAX_CLASSES 4096
#define SAIS_PROBE_MAX_DIM 1920
typedef struct {
    const float* X;            /* [B, Dm] */
    const float* dZ;           /* [H, B, C], from sais_probe_ce in train mode */
    float* W;                  /* [H, C, Dm] */
    float* b;                  /* [H, C] */
    float* mW;                 /* momentum buffers, as W and b */
    float* mb;
    const float* loss_rows;    /* [H, B] or NULL */
    float* loss;               /* [H] or NULL (both or neither) */
    int H, B, C, Dm;
    float momentum;
    float lr[SAIS_PROBE_MAX_HEADS];
} SaisProbeUpdate;
int sais_probe_logits(const float* X, const float* W, const float* b, int H, int B, int C, int Dm, float* Z, void* stream);
int sais_probe_ce(float* Z, const int* targets, int H, int B, int C, int train, float* loss_rows, int* top5, float* loss,
                  void* stream);
int sais_probe_update(const SaisProbeUpdate* u, void* stream);

/* ================================================================ dense ViT features at any resolution
 * (dino-main/eval_video_segmentation.py runs get_intermediate_layers on 480 x 832 frames: 30 x 52 patches + CLS = 1561 tokens;
 * sais_amd/csrc/attn_any.hip, host: VisionTransformer.dense_features).  Additive entries: the ABI version does not change.
 * sais_vit_attn_fwd_any: the layouts and arithmetic contract of sais_vit_attn_fwd (qkv bf16 [frames*ntok, 1152] = q | k | v
 *   head-major, out bf16 [frames*ntok, 384], fp32 softmax statistics, lse f32 [frames, 6, ntok] optional) for any
 *   2 <= ntok <= SAIS_VIT_ATTN_ANY_MAX_TOKENS: keys and values stream through LDS in tiles of 64 with an online softmax; keys
 *   past the end are masked before the row maximum, rows past frames * ntok of `out` are not written.  Forward only, no
 *   probabilities.  No atomics: bit-reproducible, and a row's result does not depend on the workgroup size the launcher picks.
 * sais_patchify_rect: frames f32 [F, 3, H, W], H and W multiples of 16 -> patches bf16 [F * (H/16) * (W/16), 768], patch rows
 *   in row-major order of the (H/16, W/16) grid, the 768 columns in sais_patchify's order (c, py, px).                   */
#define SAIS_VIT_ATTN_ANY_MAX_TOKENS 4097
int sais_vit_attn_fwd_any(const void* qkv, long ldqkv, int frames, int ntok, void* out, long ldo, float* lse /*optional*/,
                          void* stream);
int sais_patchify_rect(const float* frames_f32 /*[F,3,H,W]*/, int frames, int H, int W, void* patches_bf16, void* stream);

/* ================================================================ ViT-S/16 training at any frame size
 * (sais_amd/csrc/attn_any_bwd.hip, host: VisionTransformer.forward under grad).  Additive entries: the ABI version does not change.
 * sais_vit_attn_bwd_any: the backward of sais_vit_attn_fwd_any with the layouts and the arithmetic of sais_vit_attn_bwd, for any
 *   2 <= ntok <= SAIS_VIT_ATTN_ANY_MAX_TOKENS and frames <= 65535.  qkv bf16 [frames*ntok, 1152] = q | k | v head-major, dout and
 *   out (the saved forward output) bf16 [frames*ntok, 384], lse f32 [frames, 6, ntok] as the forward wrote it, dqkv bf16
 *   [frames*ntok, 1152]: every element written exactly once.  P = exp2(s c - lse log2e) in f32, delta = rowsum(dout * out) in f32,
 *   dS = P (dP - delta) rounded once to bf16 for dQ and dK, P rounded once to bf16 for dV; f32 accumulation, one rounding on
 *   store.  Two launches, each the only writer of its outputs: (frame, head, query tile) computes delta (to the workspace, f32
 *   [frames, 6, ntok]) and dQ with K / V streamed through LDS in 64-row tiles; (frame, head, key tile) computes dK and dV with Q /
 *   dO / lse / delta streamed the same way.  S and dP are computed in both (7 tile products per pair instead of 5).  No atomics:
 *   bit-reproducible, and a row's result does not depend on the workgroup size the launcher picks (64-row workgroups iff
 *   frames * 6 * ceil(ntok / 64) >= 512, else 32-row ones).  Keys past ntok are masked before the exponential, query rows past
 *   ntok contribute nothing; rows outside the tensor are reached by clamped loads only and never stored.
 *   SAIS_ERR_ARG and nothing launched for: a null pointer, frames or ntok out of range, a row stride that is not a multiple of 8
 *   or below the row width (1152 for qkv / dqkv, 384 for dout / out), workspace_bytes below
 *   sais_vit_attn_bwd_any_workspace_bytes(frames, ntok) (0 for non-positive arguments).  The workspace is 16-B aligned.        */
size_t sais_vit_attn_bwd_any_workspace_bytes(int frames, int ntok);
int sais_vit_attn_bwd_any(const void* qkv, long ldqkv, const void* dout, long lddo, const void* out, long ldout,
                          const float* lse, int frames, int ntok, void* dqkv, long lddqkv, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ================================================================ ViT-S/8: the patch-8 backbone (inference)
 * (sais_amd/csrc/vit8.hip, host: VisionTransformer with patch_size = 8).  Additive entries: the ABI version does not change.
 * sais_patchify_rect8: frames f32 [F, 3, H, W], H and W positive multiples of 8 -> patches bf16 [F * (H/8) * (W/8), 192], patch
 *   rows in row-major order of the (H/8, W/8) grid, the 192 columns in (c, py, px) order (the Conv2d weight of PatchEmbed
 *   flattened); each value is the round-to-nearest-even bf16 of the f32 pixel.  Anything else is SAIS_ERR_ARG.
 * sais_vit_attn_cls_fwd_any: the contract of sais_vit_attn_cls_fwd for any 2 <= ntok <= SAIS_VIT_ATTN_ANY_MAX_TOKENS.  qkv bf16
 *   [frames * ntok, 1152] (row stride ldqkv >= 1152, a multiple of 8), out bf16 [frames, 384] (row stride ldo >= 384, a multiple
 *   of 8): the attention output of the CLS query of every (frame, head).  q is read from the CLS row ONLY (the q columns of the
 *   other rows may be unwritten), K and V of all tokens once; scores, row maximum and sum in fp32, P is not rounded; rows past
 *   ntok are reached by clamped loads only.  One workgroup per (frame, head), no atomics: bit-reproducible, and a frame's result
 *   does not depend on the number of frames in the launch.  Forward only.                                                      */
int sais_patchify_rect8(const float* frames_f32 /*[F,3,H,W]*/, int frames, int H, int W, void* patches_bf16, void* stream);
int sais_vit_attn_cls_fwd_any(const void* qkv, long ldqkv, int frames, int ntok, void* out, long ldo, void* stream);

/* ================================================================ video object segmentation: label propagation
 * (dino-main/eval_video_segmentation.py; sais_amd/csrc/vos.hip, host: sais_amd/vos.py).
 * sais_vos_propagate: label_propagation (:113-150) for one target frame.  n = h * w <= SAIS_VOS_MAX_PATCHES patches, row-major.
 *   tar f32 [n, dim] and ctx f32 [nctx, n, dim]: patch features with L2-NORMALISED rows (normalise a frame once, when it enters
 *   the context: sais_l2norm_fwd); segs f32 [nctx, C, n]: the context frames' soft masks; out f32 [C, n].
 *   a[c, key, q] = exp(10 cos(q, key_c)) where |y_q - y_key| <= radius and |x_q - x_key| <= radius (everywhere when radius ==
 *   0), else 0.  Per query q, t = the topk-th largest of the nctx * n values a[., ., q]; every entry with a >= t is kept — ties at
 *   the threshold ALL stay, and with fewer than topk in-window entries t = 0 keeps every in-window entry.  out[:, q] = the
 *   average of segs[c, :, key] over the kept entries weighted by a.  Selection is done on the cosines (exp is monotone), which
 *   are exact-f32 MFMA dot products in one fixed order: identical rows give bit-identical cosines in every context slot.
 *   1 <= nctx <= SAIS_VOS_MAX_CONTEXT, 1 <= C <= SAIS_VOS_MAX_CLASSES, 1 <= topk <= SAIS_VOS_MAX_TOPK, dim == SAIS_VOS_DIM.
 *   ctx_order (host array of nctx values in [0, SAIS_VOS_MAX_CONTEXT), or NULL for 0 .. nctx - 1): context c is slot
 *   ctx_order[c] of ctx and segs, so a ring buffer of frames is read in the reference's order (first frame, then oldest to
 *   newest) without moving it.  One launch, no workspace, no atomics: bit-reproducible.
 * sais_vos_upsample_argmax: seg f32 [C, h, w] -> labels u8 [h * patch, w * patch] (:74-76): bilinear upsampling by `patch`
 *   (align_corners = False: source coordinate (i + 0.5) / patch - 0.5 clamped at 0, neighbours clamped at the border), then per
 *   channel norm_mask (:102-110) on the UPSAMPLED map (maximum <= 0: left as it is; else minus its minimum, divided by the
 *   maximum of the shifted map), then the channel argmax per pixel, ties to the lowest channel, a NaN (a constant positive
 *   channel: 0 / 0) counting as the largest, as torch.max does.  1 <= patch <= 64.  workspace: SAIS_VOS_UPSAMPLE_WS_FLOATS
 *   floats per channel.  Two launches (partial min / max, then normalise + argmax).                                       */
#define SAIS_VOS_DIM 384
#define SAIS_VOS_MAX_CONTEXT 16
#define SAIS_VOS_MAX_CLASSES 64
#define SAIS_VOS_MAX_TOPK 16
#define SAIS_VOS_MAX_PATCHES 4096
#define SAIS_VOS_UPSAMPLE_WS_FLOATS 128
int sais_vos_propagate(const float* tar, const float* ctx, const float* segs, int nctx, int C, int h, int w, int dim, int radius,
                       int topk, const int* ctx_order /*host, optional*/, float* out, void* stream);
int sais_vos_upsample_argmax(const float* seg, int C, int h, int w, int patch, unsigned char* labels, float* workspace,
                             void* stream);

/* ================================================================ attention-map rendering
 * (dino-main/video_generation.py and visualize_attention.py; sais_amd/csrc/attnviz.hip, host: VisionTransformer.cls_attention and
 * sais_amd/attnviz.py).  Additive entries: the ABI version does not change.  No atomics: every entry is bit-reproducible.
 * sais_vit_cls_probs: row 0 of the last block's softmax (Attention.forward, vision_transformer.py:83-90) at any token count.
 *   q bf16 [frames, 384] (the CLS queries, row stride ldq), k bf16 [frames * ntok, 384] head-major (row stride ldk: the K third
 *   of a qkv buffer is passed in place), 2 <= ntok <= SAIS_VIT_ATTN_ANY_MAX_TOKENS.  probs f32 [frames, 6, ntok] =
 *   softmax_j(q_h . k_{j,h} / 8) over ALL ntok keys, the CLS key included; scores, row maximum and sum in fp32, keys past ntok
 *   never enter the maximum, nothing is written past frames * 6 * ntok.  ldq, ldk multiples of 8, q and k 16-B aligned.  One
 *   workgroup per (frame, head): a row's result does not depend on the number of frames.
 * sais_attn_mass_mask: "keep xx% of the mass" (video_generation.py:197-205) per row.  p f32 [rows, n] (row stride ldp),
 *   1 <= n <= SAIS_ATTN_MASK_MAX_N, 0 < threshold < 1, keep u8 [rows, n].  The row is ordered ascending by value, equal values
 *   in ascending index order (stable); element j is kept iff its inclusive cumulative sum divided by the row sum is
 *   > 1 - threshold.  The sums run in fp64 in one fixed order.  A row whose sum is 0 keeps nothing.
 * sais_attn_render: p f32 [frames, nh_total, n] (row stride ldp, row = frame * nh_total + head), keep u8 [frames, nh_total, n]
 *   or NULL (no masking), heads head0 .. head0 + nheads - 1, grid h x w with h * w == n <= SAIS_ATTN_MASK_MAX_N, 1 <= patch <= 64.
 *   heat f32 [frames, h, w]: the sum over the heads, ascending and starting from the first term, of (p * keep) / nheads — an f32
 *   product by 0 or 1, an f32 division, f32 additions, as numpy evaluates video_generation.py:235-238.
 *   rgb u8 [frames, h * patch, w * patch, 3] (NULL: heat only): per frame vmin / vmax of heat, then matplotlib's Normalize and
 *   Colormap.__call__ on f32: ((x - vmin) / (vmax - vmin)) * 256 truncated, the value 256 -> 255, index 0 everywhere for a
 *   constant map; lut u8 [256, 3] on the device; every pixel of a patch gets the patch's colour (nearest upsampling).
 *   workspace: SAIS_ATTN_RENDER_WS_FLOATS floats per frame, needed with rgb.  Two launches with rgb, one without.        */
#define SAIS_ATTN_MASK_MAX_N 4096
#define SAIS_ATTN_RENDER_WS_FLOATS 32
int sais_vit_cls_probs(const void* q, long ldq, const void* k, long ldk, int frames, int ntok, float* probs, void* stream);
int sais_attn_mass_mask(const float* p, long ldp, int rows, int n, double threshold, unsigned char* keep, void* stream);
int sais_attn_render(const float* p, long ldp, const unsigned char* keep /*optional*/, int frames, int nh_total, int head0,
                     int nheads, int h, int w, int n, int patch, const unsigned char* lut, float* heat,
                     unsigned char* rgb /*optional*/, float* workspace, void* stream);

/* ================================================================ copy detection and image retrieval
 * (dino-main/eval_copy_detection.py and eval_image_retrieval.py; sais_amd/csrc/retrieval.hip, host: VisionTransformer.
 * retrieval_features and sais_amd/retrieval.py).  Additive entries: the ABI version does not change.  No atomics, every sum in one
 * fixed order: every entry is bit-reproducible.
 * sais_vit_cls_gem_norm: the Copydays descriptor (eval_copy_detection.py:166-175), the sibling of sais_vit_cls_avgpool_norm.
 *   x f32 [frames][ntok, dim] (frame_stride floats apart) is the residual stream after the last block; LayerNorm (gamma, beta,
 *   eps) of all ntok rows, then y[f][0 : dim] = norm(x)[f][0] (the CLS token: a sais_layernorm_fwd launch, so its bits) and
 *   y[f][dim + j] = (mean over the ntok - 1 patch rows of max(norm(x)[f][1..][j], p_clamp_min)^4)^(1/4): GeM with exponent 4 as
 *   two squarings and two square roots, the patch half in fp64 from the f32 inputs to one final rounding and summed in a fixed order, the halves CONCATENATED as the reference's torch.cat(dim=1) does.  y f32, ldy >= 2 dim
 *   floats between frames.  Any ntok >= 2, dim == 384, p_clamp_min > 0.  The normed [frames, ntok, dim] tensor is not written.
 * sais_colmean_cov: X f32 [N, D] (row stride ldx) -> mean f32 [D] = column means and cov f32 [D, D] = X^T X / N, UNCENTRED as
 *   eval_copy_detection.py:283 computes it.  D % 64 == 0, D <= SAIS_COV_MAX_DIM, any N >= 1.  The exact f32-input MFMA: per element
 *   an fmaf chain over the rows of a split in ascending order; the splits store raw partial tiles, a second launch adds them in
 *   ascending order and divides by N.  Only the tiles on or above the diagonal are computed, the others are their mirror image:
 *   cov is bit-symmetric.  workspace: sais_colmean_cov_workspace_bytes(N, D) bytes (0 for a shape the entry rejects); the query
 *   and the launch read one plan.
 * sais_center_rows: x[r][0 : dim] -= mean in place (database -= mean_feature, :279-280), x f32 [rows, dim] with row stride ldx,
 *   dim % 4 == 0, 16-B aligned.
 * sais_rank_positions: sim f32 [Nq, Ndb] (row stride ld), finite; offsets i32 [Nq + 1] and items i32 [offsets[Nq]] on the
 *   device: per query a list of database indices (CSR).  pos[t] = the 0-based position of items[t] in its query's row under the
 *   order (value descending, index ascending) = #{i : s[i] > s[j] or (s[i] == s[j] and i < j)}, which is
 *   np.argsort(-s, kind="stable") — the positions utils.compute_map looks up with np.in1d (eval_image_retrieval.py:176).  The row
 *   is streamed once per chunk of 64 listed items; a query with an empty list does no work; an item outside [0, Ndb) gets -1.
 *   Integer and exact.  Ndb <= 2^30.  offsets must be non-decreasing with offsets[0] >= 0 and offsets[Nq] <= the length of items and
 *   pos: they are device data and are NOT checked (a decreasing pair is read as an empty list; an offset past the arrays is read
 *   out of bounds).  sais_amd.retrieval.rank_positions builds them from host lists and checks the items; a direct caller owns that.
 * sais_resize_bilinear_f32: F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False) of utils.multi_scale on
 *   x f32 [frames, 3, H, W] -> y f32 [frames, 3, Ho, Wo] with Ho = floor(H scale), Wo = floor(W scale) (checked).  The source
 *   coordinate is (float)(1 / scale) (dst + 0.5) - 0.5 clamped at 0: the given scale factor, as torch uses it with
 *   recompute_scale_factor = None.                                                                                       */
#define SAIS_COV_MAX_DIM 1536
int sais_vit_cls_gem_norm(const float* x, long frame_stride, int frames, int ntok, int dim, const float* gamma, const float* beta,
                          float eps, float p_clamp_min, float* y, long ldy, void* stream);
size_t sais_colmean_cov_workspace_bytes(int N, int D);
int sais_colmean_cov(const float* X, long ldx, int N, int D, float* mean, float* cov, void* workspace, size_t workspace_bytes,
                     void* stream);
int sais_center_rows(float* x, long ldx, long rows, int dim, const float* mean, void* stream);
int sais_rank_positions(const float* sim, long ld, int Nq, int Ndb, const int* offsets, const int* items, int* pos, void* stream);
int sais_resize_bilinear_f32(const float* x, int frames, int H, int W, double scale, float* y, int Ho, int Wo, void* stream);

/* ================================================================ frames of different sizes in one backbone pass
 * (sais_amd/csrc/attn_seg.hip, host: sais_amd/vit_seg.py and VisionTransformer.retrieval_features / dense_features on a list).
 * Additive entries: the ABI version does not change.  Patch 16 only.  No atomics: every entry is bit-reproducible.
 * A pass is described by one table with one sais_vit_seg record per FRAME (a segment of the stacked [M, .] token rows):
 *   row0: its first token row; ntok = 1 + gh * gw tokens (2 .. SAIS_VIT_ATTN_ANY_MAX_TOKENS), gh x gw its patch grid; pix: the
 *   offset in floats of its pixels [3, 16 gh, 16 gw] (contiguous) in a packed f32 buffer, a multiple of 4; tap_y / tap_x: the
 *   offsets in floats of its two per-axis interpolation matrices f32 [gh, 14] and [gw, 14] in a tap buffer (the rows of
 *   interpolate_pos_encoding's bicubic map along one axis, vision_transformer.py:174-194; a matrix depends on the grid side
 *   alone and is shared by every segment with that side), or both -1 for a 14 x 14 grid, which takes the positional table itself.
 * Every entry takes the table twice: the host copy is what the argument checks read, the device copy (16-B aligned) what the kernel
 * reads; they must hold the same records.  Segments are in ascending row order and do not overlap; `rows` is the number of rows
 * the stacked tensors have (rows past the last segment are never touched).  The entries marked "dense" need row0 of segment s
 * = the sum of ntok of the segments before it (stacked from row 0 without gaps).
 * SAIS_ERR_ARG and nothing launched for: a null table, nseg outside 1 .. 65535, a record out of these ranges, a misaligned or
 * too small row stride, and what each entry adds below.
 * sais_vit_seg_qtile: the queries per workgroup sais_vit_attn_fwd_seg uses for these segments, 64 or 32: the rule of
 *   sais_vit_attn_fwd_any applied to the pass (64 iff 6 * sum ceil(ntok / 64) >= 512).  Host only, reads ntok.
 * sais_vit_attn_fwd_seg: the streaming attention forward over all segments in ONE launch.  qkv bf16 [rows, 1152] (row stride ldqkv
 *   >= 1152, a multiple of 8), out bf16 [rows, 384] (ldo >= 384, a multiple of 4), lse f32 [6 * rows] or NULL: segment s owns
 *   lse[6 row0 .. 6 (row0 + ntok)) as [6, ntok].  tiles: ntiles (segment, first query) pairs of int32, one per workgroup, in any
 *   order, covering the queries of every segment in steps of qtile = sais_vit_seg_qtile(...) exactly once — ntiles must equal
 *   sum ceil(ntok / qtile) and every pair must lie inside its segment (checked on the host copy; 8-B aligned on the device).
 *   Contract: the bytes written for segment s equal what sais_vit_attn_fwd_any(frames = 1, ntok) writes for
 *   (qkv + row0 ldqkv, out + row0 ldo, lse + 6 row0), in either workgroup form: both kernels run one tile body
 *   (csrc/attn_stream.hpp), in which a query's result depends on the rows of its own frame alone.
 * sais_patchify_seg (dense): pixels f32 [npix] packed -> patches bf16 [sum gh gw, 768] in segment order; per segment bit-equal
 *   to sais_patchify_rect on that frame.  A segment whose pixels do not lie inside [0, npix) is SAIS_ERR_ARG.
 * sais_vit_embed_seg (dense): x f32 [rows, 384] token rows of every segment: row0 = cls + pos[0]; row0 + 1 + p = patch_out[row0 -
 *   s + p] + the positional row of patch p, where patch_out f32 [sum gh gw, 384] is the patch GEMM's output with its bias, pos f32
 *   [197, 384] the positional table and the positional row of patch (y, x) is sum_a Ty[y][a] (sum_b Tx[x][b] pos[1 + 14 a + b])
 *   over the non-zero taps in ascending order (f32, at most sixteen terms).  taps f32 [ntaps]; a matrix outside it is SAIS_ERR_ARG.
 * sais_vit_cls_gather_seg: out f32 [nseg, 384] = x[row0 of every segment] (x f32, row stride ldx >= 384, a multiple of 4): the
 *   input of the sais_layernorm_fwd launch that makes the features.                                                            */
typedef struct sais_vit_seg {
    int row0, ntok, gh, gw;
    long long pix;
    int tap_y, tap_x;
} sais_vit_seg;
int sais_vit_seg_qtile(const sais_vit_seg* segs_host, int nseg);
int sais_vit_attn_fwd_seg(const void* qkv, long ldqkv, long rows, const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev,
                          int nseg, const int* tiles_host, const int* tiles_dev, int ntiles, void* out, long ldo, float* lse,
                          void* stream);
int sais_patchify_seg(const float* pixels_f32, long npix, const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev, int nseg,
                      void* patches_bf16, void* stream);
int sais_vit_embed_seg(const float* patch_out, const float* cls, const float* pos, const float* taps_dev, long ntaps,
                       const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev, int nseg, float* x, long rows, void* stream);
int sais_vit_cls_gather_seg(const float* x, long ldx, long rows, const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev,
                            int nseg, float* out, void* stream);

/* ---------------------------------------------------------------- the backward of the segmented pass (training on mixed sizes)
 * Additive entries in the same file; the table rules above hold, no entry uses atomics, two calls are bit-equal.
 * sais_vit_attn_bwd_seg: the backward of sais_vit_attn_fwd_seg over all segments in TWO launches, as sais_vit_attn_bwd_any: the
 *   forward's tile table read as (segment, first query) for delta and dQ, then as (segment, first key) for dK and dV; the rows per
 *   workgroup are sais_vit_seg_qtile(...) in both.  qkv / dqkv bf16 [rows, 1152], dout / out bf16 [rows, 384] (row strides
 *   multiples of 8, >= 1152 / 384), lse f32 [6 * rows] as the segmented forward wrote it ([6, ntok] at 6 row0), workspace: the f32
 *   delta in the same layout, sais_vit_attn_bwd_seg_workspace_bytes(rows) = 24 rows bytes (0 for rows <= 0).  Every element of dqkv
 *   inside a segment has exactly one writer; rows (and pad columns) outside every segment are never touched.
 *   Contract: the bytes of dqkv written for segment s equal what sais_vit_attn_bwd_any(frames = 1, ntok) writes for
 *   (qkv + row0 ldqkv, dout + row0 lddo, out + row0 ldout, lse + 6 row0, dqkv + row0 lddqkv), in either workgroup form and with
 *   padded row strides: both files run the two tile bodies of csrc/attn_stream_bwd.hpp.
 *   SAIS_ERR_ARG and nothing launched: what sais_vit_attn_fwd_seg refuses, a null lse / dout / dqkv / workspace, a short workspace.
 * sais_vit_embed_bwd_seg (dense): the backward of sais_vit_embed_seg from dx f32 [rows, 384] (contiguous), accumulated INTO the
 *   gradient buffers as sais_vit_embed_bwd does:
 *     dpatch bf16 [sum gh gw, 384] = bf16(dx) of the patch rows in segment order (the dY operand of sais_gemm_tn);
 *     dcls[384] += sum_s dx[row0_s];  dpos[0] += the same sum;
 *     dpos[1 + 14 a + b] += sum_s sum_y sum_x Ty_s[y][a] Tx_s[x][b] dx[row0_s + 1 + y gw + x]   (a 14 x 14 segment: its rows).
 *   f32, fixed order: one workgroup owns one row of dpos; it cuts the segments into 8 runs of ceil(nseg / 8) consecutive ones,
 *   sums each run from 0 in ascending (segment, y, x) over the non-zero taps as acc = fma(Ty Tx, dx, acc) (the product rounded to
 *   f32 first; weight one for a 14 x 14 segment), adds the 8 partial sums in ascending order from 0 and adds the total to the
 *   buffer.  Per element the error is at most (terms + 2) 2^-24 sum |Ty Tx dx| (+ 2^-24 |the value it is added to|).
 * sais_vit_cls_scatter_seg: dst[row0 of segment s] = src[s] (src f32 [nseg, 384] contiguous; dst f32, row stride ldd >= 384, a
 *   multiple of 4; the other rows are not touched): the inverse of sais_vit_cls_gather_seg.
 * sais_vit_rows_expand_seg (dense, rows = the rows of the pass): out f32 [nb, rows], out[b][r] = per_seg[b][segment of r]
 *   (per_seg f32 [nb, nseg]): per-segment DropPath scales (sais_droppath_scales with samples = nseg, rows_per_sample = 1) as the
 *   per-row scales the GEMM epilogues read.                                                                                    */
size_t sais_vit_attn_bwd_seg_workspace_bytes(long rows);
int sais_vit_attn_bwd_seg(const void* qkv, long ldqkv, const void* dout, long lddo, const void* out, long ldout, const float* lse,
                          long rows, const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev, int nseg, const int* tiles_host,
                          const int* tiles_dev, int ntiles, void* dqkv, long lddqkv, void* workspace, size_t workspace_bytes,
                          void* stream);
int sais_vit_embed_bwd_seg(const float* dx, long rows, const float* taps_dev, long ntaps, const sais_vit_seg* segs_host,
                           const sais_vit_seg* segs_dev, int nseg, float* dcls, float* dpos, void* dpatch_bf16, void* stream);
int sais_vit_cls_scatter_seg(const float* src, const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev, int nseg, float* dst,
                             long ldd, long rows, void* stream);
int sais_vit_rows_expand_seg(const float* per_seg, int nb, const sais_vit_seg* segs_host, const sais_vit_seg* segs_dev, int nseg,
                             float* out, long rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif
