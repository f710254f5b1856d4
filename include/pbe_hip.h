/*
 * libpbe_hip.so — C-ABI of the MI355X (gfx950) native kernels behind Paint-by-Example's
 * PLMS denoising hot path.
 *
 * The reference (zhanwenchen/pbe) is 100 % Python on PyTorch and has NO native layer or FFI
 * (SURVEY.md "Quick facts"); every entry point below therefore replaces an ATen dispatch made
 * from a reference Python function, cited per entry as file:line under /root/reference.
 * The host side (this repo's `ldm/` package, same import paths / class names / state_dict keys
 * as the reference) binds these symbols with ctypes (pbe_amd/lib.py); INTEGRATION.md shows the
 * stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative PBE_E* code; pbe_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - the CALLER allocates every buffer (device memory); the library never allocates, frees or
 *     retains a pointer.  Kernels are enqueued on `stream` (a hipStream_t) and never synchronise,
 *     so every call is capturable in a hipGraph.
 *   - activations are fp16, NHWC ("tokens x channels") unless an entry says otherwise; GEMM and
 *     attention accumulate in fp32 on the matrix cores; norms / softmax reduce in fp32.
 *   - descriptors are plain C structs of pointers and sizes (no torch types).
 */
#ifndef PBE_HIP_H
#define PBE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBE_ABI_VERSION 8

#define PBE_OK 0
#define PBE_EINVAL (-1)  /* bad shape / alignment / null pointer          */
#define PBE_ELAUNCH (-2) /* hipLaunch failed                              */
#define PBE_ENOTSUP (-3) /* shape outside what the kernels are built for  */

/* epilogue activations */
#define PBE_ACT_NONE 0
#define PBE_ACT_SILU 1
#define PBE_ACT_GELU_ERF 2
#define PBE_ACT_QUICK_GELU 3
#define PBE_ACT_GEGLU 4 /* GEMM only: W rows interleaved (x_j, gate_j); C[m, j] = x_j * gelu_erf(gate_j), width N/2 (attention.py:43-45) */

#define PBE_DTYPE_F16 0
#define PBE_DTYPE_F8E4M3 1 /* OCP e4m3fn (gfx950's fp8; not the fnuz form of gfx942) */

typedef void* pbe_stream_t; /* hipStream_t */

int pbe_abi_version(void);
const char* pbe_last_error(void);
/* sha256 (first 16 hex digits) over the sources and flags the library was built from (pbe_amd/build.py); the ctypes loader
 * recomputes it from the tree and refuses a stale binary instead of silently running old kernels. */
const char* pbe_source_hash(void);
/* sizeof() of the descriptor structs as THIS binary was compiled: a binding checks its own struct layout against them
 * at load time (pbe_amd/lib.py does; the ctypes stub of INTEGRATION.md section 2 does), so a binding written for an older
 * ABI hands over a short struct and gets an error instead of an out-of-bounds read. */
size_t pbe_sizeof_gemm_desc(void);
size_t pbe_sizeof_conv3x3_desc(void);
size_t pbe_sizeof_attn_desc(void);
size_t pbe_sizeof_attn_mx8_desc(void);
size_t pbe_sizeof_mx8_out_desc(void);
size_t pbe_sizeof_ctx_attn_desc(void);
size_t pbe_sizeof_gnfold_desc(void);
/* The implicit-GEMM kernels' parameter block (internal to the library; for layout tests): its size, and the size of its HEAD - the leading
 * bytes that hold everything a workgroup reads before its first fetch; epilogue, statistics and diagnostic fields lie behind it. */
size_t pbe_sizeof_igemm_params(void);
size_t pbe_sizeof_igemm_head(void);

/* ---------------------------------------------------------------------------------------------
 * pbe_gemm_f16 — C[m,n] = act(alpha * sum_k A[m,k] * W[n,k] + bias + rowvec[m / group_rows, n]) + R[m,n]
 * Replaces torch.nn.Linear / 1x1 Conv2d / einsum dispatches:
 *   ldm/modules/attention.py:198-205,41,61,270-285 (to_q/k/v, to_out, GEGLU proj, FF out, proj_in/out),
 *   ldm/modules/diffusionmodules/openaimodel.py:218-224,234-241,623-628 (emb_layers, skip 1x1, time_embed),
 *   ldm/modules/diffusionmodules/model.py:152-204 (VAE q/k/v/proj_out and both bmm's),
 *   ldm/modules/encoders/xf.py:30-57, transformers CLIP q/k/v/out_proj/fc1/fc2, latent_diffusion.py:112.
 * A may be split along K into two sources (A | A2 at K1) so torch.cat((h, skip), 1)
 * (openaimodel.py:883) is never materialised.
 * ------------------------------------------------------------------------------------------ */
typedef struct pbe_gemm_desc {
    const void* A;      /* fp16 [M, K1] row-major, leading dim lda                    */
    const void* A2;     /* fp16 [M, K-K1] or NULL                                     */
    const void* W;      /* fp16 [N, K] row-major (torch Linear layout), leading dim ldw */
    void* C;            /* fp16 [M, N], leading dim ldc                               */
    const float* bias;  /* fp32 [N] (or [M] when bias_per_row) or NULL                */
    const void* rowvec; /* fp16 [ceil(M/group_rows), ldv] broadcast over row groups, or NULL */
    const void* resid;  /* fp16 [M, N] leading dim ldr, added AFTER act, or NULL      */
    int32_t M, N, K, K1;
    int64_t lda, lda2, ldw, ldc, ldr;
    int32_t ldv, group_rows;
    int64_t strideA, strideW, strideC, strideR; /* batch strides (elements)           */
    int32_t batch;
    float alpha;
    int32_t act;
    int32_t bias_per_row;
    void* workspace;        /* optional device scratch for split-K partial sums (fp32), or NULL     */
    size_t workspace_bytes; /* any size: the split is clamped to what fits (64 MiB covers the path) */
    int32_t tile_cfg;       /* -1 = built-in heuristic; else (block-tile config 0..21, the tile table of igemm_kernel.h; 10..14 are the halo-resident conv tiles and apply to stride-1 3x3 convs only, on maps where the tile's pixels are whole rows of one image or a whole number of images (any other request plans as -1), 15..18 deep-ring forms of 3 / 4 / 6 / 9, 19 / 20 A-stationary LayerNorm-fold tiles, 21 dense only; fp8 operands run 3, 4, 6, 8 or 9 and map any other pick to one of them) | (split-K factor << 8), factor 0 = library's choice */
    /* fp8 operands (BASELINE configs[4]): operand_dtype = PBE_DTYPE_F8E4M3 -> A [M, K] and W [N, K] hold OCP e4m3 bytes, lda / ldw /
     * strideA / strideW count BYTES (multiples of 16, K % 16 == 0, no A2), and C = act(alpha * a_scale[m] * w_scale[n] * sum_k A W + ...):
     * a_scale fp32 [M] per row of A (e.g. per token, from pbe_layernorm_f8), w_scale fp32 [N] per row of W (per output channel, from the
     * pack); *_scale_stride = elements between the batches' scale vectors (0: shared).  C, bias, rowvec, resid stay as in the fp16 form. */
    const float* a_scale;
    const float* w_scale;
    int64_t a_scale_stride, w_scale_stride;
    int32_t operand_dtype;  /* PBE_DTYPE_F16 (0) or PBE_DTYPE_F8E4M3 (1) */
    /* Extended epilogue (ABI 7; fp16 operands, batch 1, never split-K) - the transformer block's GEMM chain, attention.py:198-252:
     *  alpha_cols > 0: alpha multiplies columns n < alpha_cols only (q of a fused q | k | v projection, pre-scaled for pbe_attention_f16);
     *  LayerNorm FOLDED into this GEMM (attention.py:248-252 norm1 / norm3 -> to_q/k/v, ff.net[0].proj): A holds the raw rows x, W must be
     *    W * gamma, bias must be W beta (+ the layer's bias), ln_colsum[n] = sum_k (W gamma)[n, k] of the fp16 values, and the epilogue forms
     *    rstd[m] * (acc - mean[m] * ln_colsum[n]) from the row statistics: (sum, sum of squares) of row m = sum over p < ln_parts of the
     *    float2 ln_stats[(p * ln_stats_ld + m)] (written by the PRODUCER of x through row_stats_out, or by pbe_row_stats_f16);
     *  row_stats_out: float2 [column tiles][row_stats_ld] partial (sum, sumsq) of THIS launch's stored fp16 output rows, one partial per column tile
     *    (pbe_gemm_plan's out6[5] tells how many), for the LayerNorm that reads the output;
     *  VT: columns n >= vt_col0 go to VT[b * vt_bs + (n - vt_col0) * vt_rs + tok] instead of C (row m = b * vt_tokens + tok): V^T for
     *    pbe_attention_f16 out of the same launch as q | k.  The V^T columns start on a column tile: vt_col0 must be a multiple of the
     *    width of at least one extended-epilogue tile (64, 128, 160 or 320 columns), and the plan picks among the tiles whose width divides
     *    it (a requested tile_cfg whose width does not is replaced by one).  Any other vt_col0 is refused with PBE_EINVAL, by pbe_gemm_plan
     *    and pbe_gemm_f16 alike, before anything is launched. */
    int32_t alpha_cols;
    const float* ln_stats;
    int32_t ln_parts;
    int64_t ln_stats_ld;
    const float* ln_colsum;
    float ln_eps;
    float* row_stats_out;
    int64_t row_stats_ld;   /* rows between two column tiles' partials in row_stats_out (>= M; 0 = M) */
    void* VT;
    int32_t vt_col0, vt_tokens;
    int64_t vt_bs, vt_rs;
} pbe_gemm_desc;
int pbe_gemm_f16(const pbe_gemm_desc* d, pbe_stream_t stream);
/* Plan / workspace query for the SAME descriptor (nothing is launched): out6 = {tile config index, split-K factor,
 * tile rows BM, tile columns BN, workgroups, column tiles}; *workspace_needed = bytes of split-K scratch the plan uses (0 when the
 * plan does not split).  A descriptor with a smaller workspace gets a smaller factor, never an error. */
int pbe_gemm_plan(const pbe_gemm_desc* d, int32_t* out6, size_t* workspace_needed);

/* ---------------------------------------------------------------------------------------------
 * pbe_conv3x3_f16 — NHWC 3x3 convolution as an implicit GEMM on the matrix cores.
 *   Y[b,oy,ox,co] = act(sum_{dy,dx,ci} X[b, iy, ix, ci] * Wp[co, k(dy*3+dx, ci)] + bias[co]
 *                       + rowvec[b, co]) + R[b,oy,ox,co]        (k(tap, ci): see kblock below)
 *   iy = oy*stride + dy - pad (zero outside), optional nearest-2x upsample of X fused in the gather,
 *   X optionally the channel concat of two tensors (X | X2).
 * Replaces Conv2d(k=3) dispatches in openaimodel.py:216,229-231 (ResBlock), :109-119 (Upsample:
 * F.interpolate + conv), :150-160 (Downsample s2 p1), :658-662,824-828 (conv in/out);
 * model.py:44-81,92-121 (VAE convs; Downsample pad (0,1,0,1) + s2 p0 == pad=0 here).
 * Requires C1 % 64 == 0 and C2 % 64 == 0; small-Cin convs go through pbe_im2col3x3_f16 + GEMM.
 * Wp is the OIHW weight re-packed by the host to [Cout, 9*Cin] in (channel block, tap, channel) order — see kblock.
 * ------------------------------------------------------------------------------------------ */
typedef struct pbe_conv3x3_desc {
    const void* X;
    const void* X2;
    const void* Wp;
    void* Y;
    const float* bias;
    const void* rowvec; /* fp16 [B, ldv]: per-(sample, channel) add (ResBlock emb, openaimodel.py:273) */
    const void* resid;  /* fp16 [B,Ho,Wo,Cout] */
    int32_t B, H, W, C1, C2, Cout;
    int32_t stride, pad, upsample; /* upsample: 0; 1 = nearest-2x fused in the gather (Wp as usual, 9 taps); 2 = the same operation in PHASE form: Wp holds
                                      four weight sets [4][Cout][4*Cin] (phase (py, px) = output pixel parity; per phase the 3x3 taps that fall on one
                                      source pixel are summed: pbe_amd.ops.pack_conv3x3_up_phases), four 2x2 convs on the source grid, 4/9 of the MACs;
                                      pad 1, stride 1, no X2 / rowvec / resid */
    int32_t ldv;
    int32_t act;
    void* workspace;        /* optional split-K scratch, as in pbe_gemm_desc */
    size_t workspace_bytes;
    int32_t tile_cfg;       /* -1 = heuristic, else tile config | (split-K factor << 8), as in pbe_gemm_desc */
    int32_t kblock;         /* channel block cb of Wp's K order: k = ((ci/cb)*T + tap)*cb + ci%cb, ci counted over the concat X | X2; multiple
                               of 64 that divides C1 and C2 (0 = 64; anything else is PBE_EINVAL).  T = taps of the form:
                                 upsample 0 and 1: T = 9, tap = dy*3 + dx.  A pixel's 9 taps are then re-read within 9*cb/64 k-tiles (L2 hits)
                                 upsample 2:       T = 4, tap = ty*2 + tx, in each of the four weight sets [Cout][4*Cin] alike
                                                   (pbe_amd.ops.pack_conv3x3_up_phases packs cb = 64)
                               The halo-resident tiles take cb = 64 only: at another kblock a request for one runs a gather tile instead.
                               The result is the same conv at every kblock; its fp32 summation order (k-tiles of 64 in K order) is not */
    /* Y feeds a GroupNorm (ResBlock: conv -> GroupNorm32 -> SiLU, openaimodel.py:213-227; the block's output -> the next normalisation):
     * group_stats_out != NULL asks the conv's copy-out for the per-(sample, row block, group) partial (sum, sumsq) of the STORED fp16
     * values, in pbe_groupnorm_f16's partial layout [B][blocks][group_stats_groups][2] (fp32; size it for blocks <= Ho*Wo / 64).
     * *group_stats_blocks (host int, written before the call returns) = blocks per sample actually produced, or 0 when the planned tile
     * cannot (split-K, a tile that is not whole groups of one sample, multi-pass epilogue): the caller then runs pbe_groupnorm_f16,
     * else pbe_groupnorm_apply_f16 with these partials.  Fixed summation order: bit-reproducible run to run. */
    float* group_stats_out;
    int32_t group_stats_groups;
    int32_t* group_stats_blocks;
} pbe_conv3x3_desc;
int pbe_conv3x3_f16(const pbe_conv3x3_desc* d, pbe_stream_t stream);
int pbe_conv3x3_plan(const pbe_conv3x3_desc* d, int32_t* out6, size_t* workspace_needed); /* as pbe_gemm_plan */
/* Host only, nothing is launched: the launch-invariant values the planned tile's kernel receives for its prologue (tile order, split-K
 * slice, halo geometry and the reciprocals it divides with).  out32 = {tile, split-K, BM, BN, mode (1 gather, 2 halo-resident), m_fast,
 * tdiv, mg_tdiv, split_per, sv_ns, sv_gdiv, mg_sv_gdiv, hw, mg_hw, mg_wo, per_blk, mg_per_blk, mg_kb, th, hw2, hps, nsub, halo rows, tiles
 * per image, mg_tpi, mh_hps, mh_hw2, log2 W, log2 pixels per (sub-)image, halo image rows of the tile,
 * offset of the parameter block's first tail field (= head size), offset of its last tail field}; mg_x = floor(2^32 / x) and
 * mh_x = ceil(2^20 / x) as 32-bit patterns (pbe_amd/csrc/igemm_params.h: udiv_mg, udiv_h). */
int pbe_conv3x3_prologue(const pbe_conv3x3_desc* d, int32_t* out32);
/* Host only: row cfg of the tile table the planners choose from.  out8 = {BM, BN, waves along m, waves along n, ring depth S in k-tiles
 * of 64 (S - 1 in flight), forms bit mask (1 dense, 2 gather conv, 4 halo-resident conv, 8 extended epilogue, 16 fp8 operands,
 * 32 A-stationary, 64 forced only), halo image rows (0: not a halo tile), workgroups of the tile a CU holds}; PBE_EINVAL past the last
 * row (the rows are numbered from 0 without gaps). */
int pbe_tile_info(int32_t cfg, int32_t* out8);

/* im2col for the three small-Cin convs (9->320 U-Net in, 3->128 VAE in, 4->512 VAE decoder in):
 * X fp16 NHWC [B,H,W,Cp] -> out fp16 [B*Ho*Wo, 9*Cp]. */
int pbe_im2col3x3_f16(const void* X, void* out, int32_t B, int32_t H, int32_t W, int32_t Cp,
                      int32_t stride, int32_t pad, pbe_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * pbe_groupnorm_f16 — GroupNorm(groups) [+ SiLU] over NHWC fp16, fp32 statistics.
 * Replaces GroupNorm32 (util.py:214-216, eps 1e-5) + SiLU in openaimodel.py:213-215,225-227,824-826;
 * Normalize (attention.py:77-78 / model.py:40-41, eps 1e-6) + swish (model.py:35-37).
 * Input may be the channel concat X | X2 (C2 = 0 for a single source).  Output [B, HW, C1+C2].
 * workspace: pbe_groupnorm_workspace_bytes(B, HW) bytes of device scratch.
 * ------------------------------------------------------------------------------------------ */
size_t pbe_groupnorm_workspace_bytes(int32_t B, int32_t HW);
int pbe_groupnorm_f16(const void* X, const void* X2, const float* gamma, const float* beta, void* Y,
                      int32_t B, int32_t HW, int32_t C1, int32_t C2, int32_t groups, float eps,
                      int32_t silu, void* workspace, size_t workspace_bytes, pbe_stream_t stream);
/* The normalisation pass alone, statistics given as partials [B][blocks][groups][2] (sum, sumsq) - from pbe_conv3x3_f16's
 * group_stats_out.  Single source (no concat), any map size. */
int pbe_groupnorm_apply_f16(const void* X, const float* partials, int32_t blocks, const float* gamma, const float* beta, void* Y,
                            int32_t B, int32_t HW, int32_t C, int32_t groups, float eps, int32_t silu, pbe_stream_t stream);

/* pbe_layernorm_f16 — LayerNorm over the last dim C (C % 8 == 0, C <= 2048) of fp16 rows.
 * Replaces attention.py:240-242 (norm1/3), xf.py:22-28, HF CLIP layer norms. */
int pbe_layernorm_f16(const void* X, const float* gamma, const float* beta, void* Y, int64_t rows,
                      int32_t C, int64_t ldx, int64_t ldy, float eps, pbe_stream_t stream);

/* pbe_row_stats_f16 — out[r] = float2(sum, sum of squares) of the fp16 row X[r, :C]: the one-partial form of the row statistics a
 * LayerNorm-folding GEMM reads (pbe_gemm_desc.ln_stats, ln_parts = 1) when the producer of X did not emit them (row_stats_out). */
int pbe_row_stats_f16(const void* X, float* out, int64_t rows, int32_t C, int64_t ldx, pbe_stream_t stream);

/* pbe_layernorm_f8 — the same LayerNorm emitting OCP e4m3 bytes and one fp32 scale per row (BASELINE configs[4]):
 * Y[r, :] = e4m3(LN(X[r, :]) / row_scale[r]), row_scale[r] = max|LN(X[r, :])| / 448, floored at 2^-100 (1 for an all-zero row): always
 * finite, normal and positive; round to nearest even, saturating; ldy in bytes (multiple of 16).  Feeds the fp8 operand form of
 * pbe_gemm_f16 (A = Y, a_scale = row_scale). */
int pbe_layernorm_f8(const void* X, const float* gamma, const float* beta, void* Y, float* row_scale, int64_t rows,
                     int32_t C, int64_t ldx, int64_t ldy, float eps, pbe_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * pbe_attention_f16 — fused softmax(Q K^T * scale) V (flash-style, no [N,N] tensor in HBM).
 * Replaces attention.py:214-229 (einsum, softmax, einsum) and HF CLIP eager attention.
 *   Q: fp16, element (b, n, h, d) at Q[b*q_bs + n*q_rs + h*D + d]   (same for K with k_*),
 *   VT: V transposed, element (b, h, d, n) at VT[b*vt_bs + (h*D+d)*vt_rs + n]  (vt_rs % 8 == 0,
 *       the row must be readable up to the next multiple of 8 past Nk),
 *   O: fp16, element (b, n, h, d) at O[b*o_bs + n*o_rs + h*D + d].
 * D % 8 == 0, D <= 160.  The softmax reference maximum is deferred (raised when a tile exceeds it by 2^8); the d = 40 form keeps it
 * as an fp16 number / 64, i.e. |scale * log2(e) * q.k| must stay below 4e6.
 * ------------------------------------------------------------------------------------------ */
typedef struct pbe_attn_desc {
    const void* Q;
    const void* K;
    const void* VT;
    void* O;
    int32_t B, H, Nq, Nk, D;
    int64_t q_bs, q_rs, k_bs, k_rs, vt_bs, vt_rs, o_bs, o_rs;
    float scale;
    int32_t q_prescaled; /* 1: Q already holds scale * log2(e) * q (the projection GEMM applied it in its fp32 epilogue, pbe_gemm_desc.alpha_cols);
                            `scale` is then ignored */
} pbe_attn_desc;
int pbe_attention_f16(const pbe_attn_desc* d, pbe_stream_t stream);

/* pbe_attention_kbias_f16 — the product of pbe_attention_f16 with a per-(sample, key) logit bias: cross-attention
 * (attention.py:207-230) over a context whose tokens carry non-negative weights w[b, key], softmax weight proportional to
 * w[b, key] * exp(scale * q.k).  key_bias: fp32, element (b, key) at key_bias[b*kb_bs + key], = log2 w[b, key]: the LOG2 domain the
 * kernel's exp2 works in (added after scale * log2(e), or directly to a q_prescaled product), shared by the H heads of sample b;
 * -inf removes the key (weight 0: a padded ragged batch), +inf and NaN are not allowed, and every sample needs at least one finite
 * entry (otherwise its rows are 0 / 0).  Nothing past key Nk - 1 is read.  Same operands, D range, strides and alignment as
 * pbe_attention_f16 (the descriptor is unchanged); Nk <= 8192 (the sample's bias row is kept in LDS).  A bias of all zeros gives
 * pbe_attention_f16's result within its rounding, not its bits at D = 40: this form never keeps the softmax reference in the head-dim
 * padding, because a reference taken from a tile whose keys are all absent would be -inf. */
int pbe_attention_kbias_f16(const pbe_attn_desc* d, const float* key_bias, int64_t kb_bs, pbe_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MX-fp8 attention core (opt-in, pbe_amd.precision.set_attention_precision): OCP e4m3 operands with one E8M0 (power-of-two) scale
 * per 32 consecutive contraction elements, both products on v_mfma_scale_f32_32x32x64_f8f6f4.
 *
 * pbe_quant_mx8_f16 — quantise fp16 rows whose contraction dim is contiguous.  Each 32-element block of one head gets the smallest
 * power of two s with max|alpha x| / s <= 448 (an all-zero block: 1.0) and the bytes e4m3(alpha x / s), round to nearest even,
 * saturating at +-448, never NaN.
 *   PBE_MX8_TOKENS (q, k): X element (b, n, h, d) at X[(b*N + n)*rs + h*D + d];
 *       Y bytes [B*N][H*DP], DP = D rounded up to 64 (zero padding); S [B][H][DP/32][NP], NP = N rounded up to 64.
 *   PBE_MX8_VT (V^T):      X element (b, h, d, n) at X[((b*H + h)*D + d)*rs + n];
 *       Y bytes [B*H*D][NP] (zero past N);                          S [B][H][NP/32][DV], DV = 32 * (D/32 + 1).
 * Scale pads (tokens past N, rows past D) hold 1.0 (127).  D % 8 == 0, rs % 8 == 0, X and Y 16-byte aligned.
 *
 * pbe_attention_mx8 — O = softmax(scale_log2e / log2(e) * Q K^T) V from those layouts (Q and K: PBE_MX8_TOKENS at Nq / Nk,
 * VT: PBE_MX8_VT at Nk).  O: fp16, element (b, n, h, d) at O[b*o_bs + n*o_rs + h*D + d].  D in {40, 80, 160}; anything else is
 * PBE_EINVAL.  P = exp2(s - m) <= 2^8 is rounded to e4m3 once and feeds both the numerator and the denominator (a ones row of V^T).
 * ------------------------------------------------------------------------------------------ */
#define PBE_MX8_TOKENS 0
#define PBE_MX8_VT 1
int pbe_quant_mx8_f16(const void* X, void* Y, void* S, int32_t mode, int32_t B, int32_t H, int32_t N, int32_t D, int64_t rs, float alpha,
                      pbe_stream_t stream);

typedef struct pbe_attn_mx8_desc {
    const void* Q;
    const void* Q_scale;
    const void* K;
    const void* K_scale;
    const void* VT;
    const void* VT_scale;
    void* O;
    int32_t B, H, Nq, Nk, D;
    int64_t o_bs, o_rs;
    float scale_log2e; /* multiplies the scores (log2 domain): scale * log2(e), or 1 when the quantiser's alpha applied it to Q */
} pbe_attn_mx8_desc;
int pbe_attention_mx8(const pbe_attn_mx8_desc* d, pbe_stream_t stream);

/* pbe_gemm_mx8out_f16 — the GEMM of pbe_gemm_f16 whose output columns leave as MX-fp8 operands of pbe_attention_mx8 instead of fp16:
 * every 32-element block of a range is quantised in the epilogue from the fp16 value pbe_gemm_f16 would store, multiplied by the range's
 * alpha in fp32, so the bytes and scales are exactly those of pbe_gemm_f16 followed by pbe_quant_mx8_f16 (padding included).
 * d->C and d->VT are not written and may be null.  Two forms:
 *   channel_rows = 0: the LayerNorm-folded q | k | v projection (fp16 operands, ln_stats, vt_col0 / vt_tokens as in pbe_gemm_f16) or an
 *       fp8-operand q | k projection: GEMM rows are the B*N tokens; a TOKENS range covers H*D columns from col0, a VT range the H*D
 *       columns from col0 = d->vt_col0 (fp16 form only).  The fp16 form takes exactly three ranges: q (TOKENS, col0 0), k (TOKENS,
 *       col0 H*D) and V^T (VT, col0 2*H*D) of an N = 3*H*D output;
 *   channel_rows = 1: the swapped V^T projection (fp8 operands, batch = B, M = H*D rows = channels, N columns = tokens): one VT range.
 * Refused (PBE_EINVAL): N % 64 != 0, D not in {40, 80, 160}, ranges with different B / H / N / D, targets not 16-byte aligned, split-K,
 * a residual, GEGLU, row statistics, an fp16 problem without the LayerNorm fold or without all three ranges, and a requested tile
 * with an MX block across a tile boundary (a planned tile never has one).
 * pbe_gemm_mx8out_plan: the tile that launches (out6 as pbe_gemm_plan), host only; PBE_EINVAL where pbe_gemm_mx8out_f16 refuses. */
typedef struct pbe_mx8_out_range {
    void* data;            /* e4m3 bytes in the layout of pbe_quant_mx8_f16 */
    void* scale;           /* E8M0 scales, same (data and scale 16-byte aligned) */
    int32_t layout;        /* PBE_MX8_TOKENS or PBE_MX8_VT */
    int32_t col0;          /* first GEMM output column of the range */
    float alpha;           /* multiplies the fp16 value before rounding (pbe_quant_mx8_f16's alpha) */
    int32_t B, H, N, D;
} pbe_mx8_out_range;
typedef struct pbe_mx8_out_desc {
    int32_t nranges;       /* 1 .. 3 */
    int32_t channel_rows;  /* see above */
    pbe_mx8_out_range r[3];
} pbe_mx8_out_desc;
int pbe_gemm_mx8out_f16(const pbe_gemm_desc* d, const pbe_mx8_out_desc* mx, pbe_stream_t stream);
int pbe_gemm_mx8out_plan(const pbe_gemm_desc* d, const pbe_mx8_out_desc* mx, int32_t* out6);

/* pbe_gemm_gnfold_f16 - pbe_gemm_f16 on GroupNorm(A) without the normalised tensor: A holds the RAW rows x [M, K] of `tokens` rows per
 * sample, and the kernel replaces every A element by fp16(x * sc[b, k] + sh[b, k]) (one fp32 multiply-add, one rounding) behind its LDS
 * read - the value and the bits pbe_groupnorm_apply_f16(silu = 0) would have stored, so C and row_stats_out equal those of the two
 * launches.  table: fp32 [samples][K / 8][16] from pbe_groupnorm_table_f32 (sc | sh of 8 consecutive channels), ld = 2 K floats per
 * sample, ceil(M / tokens) samples.  Accepted: a 2-D fp16 problem (batch 1, no A2, ln_stats, VT, alpha_cols, GEGLU; bias, rowvec, resid,
 * act and row_stats_out as in pbe_gemm_f16), K % 64 == 0, K <= 1280, and a tile whose row count divides `tokens` (a tile's rows then
 * belong to one sample; a requested tile that does not is replaced by the heuristic's pick among those that do).  PBE_EINVAL
 * otherwise: the caller then runs pbe_groupnorm_apply_f16 and pbe_gemm_f16.  Never split-K.
 * pbe_gemm_gnfold_plan: the tile that launches (out6 as pbe_gemm_plan), host only; PBE_EINVAL where pbe_gemm_gnfold_f16 refuses.
 * pbe_groupnorm_table_f32: sc[b, c] = rstd[b, g] gamma[c], sh[b, c] = beta[c] - mean[b, g] sc[b, c] from the partial statistics
 * [B][blocks][groups][2] (group_stats_out of pbe_conv3x3_f16), with the finalise and the fp32 expressions of pbe_groupnorm_apply_f16. */
typedef struct pbe_gnfold_desc {
    const float* table; /* fp32 [samples][K / 8][16], 16-byte aligned */
    int64_t ld;         /* floats per sample: 2 K */
    int32_t tokens;     /* rows of A per sample */
} pbe_gnfold_desc;
int pbe_groupnorm_table_f32(const float* partials, int32_t blocks, const float* gamma, const float* beta, float* table, int32_t B, int32_t HW,
                            int32_t C, int32_t groups, float eps, pbe_stream_t stream);
int pbe_gemm_gnfold_f16(const pbe_gemm_desc* d, const pbe_gnfold_desc* g, pbe_stream_t stream);
int pbe_gemm_gnfold_plan(const pbe_gemm_desc* d, const pbe_gnfold_desc* g, int32_t* out6);

/* ---------------------------------------------------------------------------------------------
 * pbe_ctx_attention_f16 — x + attn2(LayerNorm(x), context) of a transformer block (attention.py:207-230, 268-272) for a SHORT context
 * of Nk = 1..16 tokens, as one launch over the residual stream.  Everything that depends on the context alone is folded by the caller
 * (once per context, pbe_gemm_f16 launches): with k = to_k(context), v = to_v(context), per sample b, head h, context token j
 *   Kq[b, h*Nk + j, c] = scale * log2(e) * gamma[c] * sum_d k[b,j,h,d] * Wq[h*D + d, c]      fp16 [B, HJ, C], HJ = H * Nk
 *   colsum[b, hj]      = sum_c of the fp16 values Kq[b, hj, c];  kbias[b, hj] = scale * log2(e) * sum_d k[b,j,h,d] * (Wq beta)[h*D + d]
 *   Vo[b, c, h*Nk + j] = sum_d Wo[c, h*D + d] * v[b,j,h,d]                                    fp16 [B, C, HJ]
 * and the kernel computes, for row m of sample b = m / tokens,
 *   Y[m,:] = X[m,:] + bias + sum_{h, j<Nk} softmax_j( rstd[m] * (X[m,:] . Kq[b,hj,:] - mean[m] * colsum[b,hj]) + kbias[b,hj] ) * Vo[b,:,hj]
 * The head dimension D is folded away.  Both products run on the matrix cores with fp32 accumulation; the softmax (exp2: the scores
 * are in the log2 domain) runs in fp32 over each head's Nk columns with the group maximum subtracted, its weights are rounded to fp16
 * once.  mean / rstd come from the row statistics of X under the contract of pbe_gemm_desc.ln_stats (float2 (sum, sumsq) partials:
 * the producer's row_stats_out, or pbe_row_stats_f16).  row_stats_out (or NULL): float2 [M] (sum, sumsq) of the stored fp16 rows of
 * Y, ONE partial (the layout of pbe_row_stats_f16), for the LayerNorm-folded GEMM that reads Y.  Row tiles never straddle two
 * samples; Kq rows and Vo columns past HJ are never read as values (operands may be padded or not).  Bit-reproducible run to run.
 * Accepted: C % 64 == 0, 64 <= C <= 1280, 1 <= Nk <= 16, H * Nk <= 128, M a multiple of tokens >= 1; leading dimensions and batch
 * strides multiples of 8 elements, vo_rs >= HJ rounded up to 8, X / Y / Kq / Vo 16-byte aligned.  Anything else: PBE_EINVAL.
 * ------------------------------------------------------------------------------------------ */
typedef struct pbe_ctx_attn_desc {
    const void* X;          /* fp16 [M, C], leading dim ldx: the residual stream (raw, not normalised)  */
    void* Y;                /* fp16 [M, C], leading dim ldy                                              */
    const void* Kq;         /* fp16: element (b, hj, c) at Kq[b*kq_bs + hj*kq_rs + c]                    */
    const float* colsum;    /* fp32: element (b, hj) at colsum[b*cs_bs + hj]                             */
    const float* kbias;     /* fp32: element (b, hj) at kbias[b*cs_bs + hj]                              */
    const void* Vo;         /* fp16: element (b, c, hj) at Vo[b*vo_bs + c*vo_rs + hj]                    */
    const float* bias;      /* fp32 [C]: to_out's bias                                                   */
    const float* ln_stats;  /* float2 [ln_parts][ln_stats_ld] partial (sum, sumsq) of X's rows           */
    float* row_stats_out;   /* float2 [M] (sum, sumsq) of Y's stored rows, or NULL                       */
    int32_t M, C, tokens, H, Nk;
    int64_t ldx, ldy, kq_bs, kq_rs, vo_bs, vo_rs, cs_bs;
    int32_t ln_parts;
    int64_t ln_stats_ld;
    float ln_eps;
} pbe_ctx_attn_desc;
int pbe_ctx_attention_f16(const pbe_ctx_attn_desc* d, pbe_stream_t stream);

/* pbe_ctx_attention_w_f16 — pbe_ctx_attention_f16 with exemplar weights (attention.py:207-230 with context token j of sample b
 * counted w[b, j] >= 0 times): log2w fp32, element (b, j) at log2w[b*w_bs + j], = log2 w[b, j] (-inf for weight 0), is added to
 * kbias[b, h*Nk + j] in fp32 when the kernel stages it, for every head h.  The folded operands (Kq, colsum, kbias, Vo) do not depend
 * on the weights: they can change without re-folding.  Every sample needs one token of positive weight.  log2w of all zeros gives the
 * bits of pbe_ctx_attention_f16. */
int pbe_ctx_attention_w_f16(const pbe_ctx_attn_desc* d, const float* log2w, int64_t w_bs, pbe_stream_t stream);

/* pbe_ctx_attention_rw_f16 — pbe_ctx_attention_f16 with a weight per (sample, query row, context token): regional exemplars, token j
 * counts e[b, t, j] >= 0 times at row t of sample b.  log2rw fp32, element (b, t, j) at log2rw[b*rw_bs + t*rw_rs + j] for t < tokens,
 * j < Nk, = log2 e[b, t, j] (-inf for 0; the caller has multiplied the exemplar weights in), is added to kbias[b, h*Nk + j] in fp32
 * BEFORE the LayerNorm fold's multiply-adds, for every head h.  Every row needs one token of positive weight; a +inf or NaN entry
 * corrupts its own row only.  Rows past a sample's last token clamp their table row as they clamp X: nothing past row tokens - 1 of a
 * sample's table, or past column Nk - 1 of a row, is read.  A table of zeros gives the bits of pbe_ctx_attention_f16, a table equal
 * to log2 w[b, j] on every row those of pbe_ctx_attention_w_f16 (Y and row_stats_out).  The folded operands do not depend on it.
 * Required: log2rw non-null and 4-byte aligned, rw_rs >= Nk, rw_bs >= 0; additive to the ABI (same descriptor). */
int pbe_ctx_attention_rw_f16(const pbe_ctx_attn_desc* d, const float* log2rw, int64_t rw_bs, int64_t rw_rs, pbe_stream_t stream);

/* pbe_ctx_attention_map_f16 — any of the three launches above with the ATTRIBUTION MAP as a side output: the softmax weights of
 * attention.py:207-230 (`attn = sim.softmax(dim=-1)`), which the reference discards after `einsum('b i j, b j d -> b i d', attn, v)`,
 * averaged over the heads.  amap fp32, element (b, t, j) at amap[b*am_bs + t*am_rs + j] for t < tokens, j < Nk, takes
 *   (1 / H) * sum_{h = 0 .. H-1} p[b, t, h, j]
 * where p are the fp16 weights the second product really multiplies, summed in that fixed order in fp32 and multiplied by the fp32
 * value 1.0f / H: the share of cross-attention context token j received at row t.  accumulate == 0 stores it; accumulate != 0 adds it
 * to what is there with one fp32 add (a plain read-modify-write by the one thread that owns the element - no atomics: launches on one
 * stream accumulate deterministically).  log2w / w_bs as pbe_ctx_attention_w_f16 or NULL, log2rw / rw_bs / rw_rs as
 * pbe_ctx_attention_rw_f16 or NULL, not both non-NULL; both NULL is pbe_ctx_attention_f16.  Y and row_stats_out carry the bits of the
 * corresponding entry without the map.  Rows past a sample's last token are not written; nothing outside t < tokens, j < Nk of a
 * sample's map is touched (rows may be padded: am_rs >= Nk).
 * Required: amap non-null and 4-byte aligned, am_rs >= Nk, am_bs >= 0; additive to the ABI (same descriptor). */
int pbe_ctx_attention_map_f16(const pbe_ctx_attn_desc* d, const float* log2w, int64_t w_bs, const float* log2rw, int64_t rw_bs,
                              int64_t rw_rs, float* amap, int64_t am_bs, int64_t am_rs, int32_t accumulate, pbe_stream_t stream);

/* pbe_ctx_map_gather_f32 — a level's attribution accumulator acc fp32 [B, h*w, K] (rows in NHWC order t = y*w + x, as
 * pbe_ctx_attention_map_f16 fills it) onto a picture grid: out fp32 [B, K, fy*h, fx*w],
 *   out[b, j, y, x] (+)= s * (acc[b, (y / fy) * w + (x / fx), j] / div)
 * i.e. a nearest upsample by the integer factors (fy, fx) and the transposition to the [B, K, H, W] layout region maps use.  div > 0
 * is the number of launches that accumulated into acc (an IEEE division: n launches that each added exactly 1 give exactly 1; 1 for
 * none), s the weight of the level in the average.  accumulate == 0 stores, != 0 adds; every step is rounded on its own. */
int pbe_ctx_map_gather_f32(const float* acc, float* out, int32_t B, int32_t K, int32_t h, int32_t w, int32_t fy, int32_t fx, float s,
                           float div, int32_t accumulate, pbe_stream_t stream);

/* pbe_softmax_rows_f16 — Y[r,:] = softmax(scale * X[r,:]) over rows of `cols` fp16 (VAE mid attention,
 * model.py:193-195: one head, d = 512, N = 4096, scores kept in HBM once per image). */
int pbe_softmax_rows_f16(const void* X, void* Y, int64_t rows, int32_t cols, int64_t ldx, int64_t ldy,
                         float scale, pbe_stream_t stream);

/* pbe_geglu_f16 — Y[m, f] = H[m, f] * gelu_erf(H[m, F + f])  (attention.py:43-45). */
int pbe_geglu_f16(const void* H, void* Y, int64_t M, int32_t F, pbe_stream_t stream);

/* pbe_timestep_embedding_f16 — util.py:151-171: out[b, :] = cat(cos(t f_k), sin(t f_k)), fp16 [B, dim]. */
int pbe_timestep_embedding_f16(const int64_t* t, void* out, int32_t B, int32_t dim, float max_period,
                               pbe_stream_t stream);

/* Layout conversion at the API boundary (the reference API is NCHW fp32/fp16):
 * src fp32 NCHW [B,C,HW] -> dst fp16 NHWC [B,HW,Cp] (channels C..Cp-1 zero) and back. */
int pbe_nchw_f32_to_nhwc_f16(const float* src, void* dst, int32_t B, int32_t C, int32_t HW, int32_t Cp,
                             pbe_stream_t stream);
int pbe_nhwc_f16_to_nchw_f32(const void* src, float* dst, int32_t B, int32_t C, int32_t HW, int32_t ld,
                             pbe_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PLMS sampler element-wise steps (plms.py:177-248), state kept fp32 NCHW [B,4,HW].
 * pbe_plms_pack_input: x9 = cat(x, z_inpaint, mask) (plms.py:225) duplicated `dup` times along the
 *   batch for classifier-free guidance (plms.py:185), as fp16 NHWC [dup*B, HW, 16] (9 real channels).
 * pbe_plms_update: eps_out fp16 NHWC [dup*B, HW, ld] from the U-Net ->
 *   e_t = e_u + scale (e_c - e_u)                       (plms.py:188-189; dup == 1: e_t = eps_out)
 *   e'  = c0 e_t + c1 h1 + c2 h2 + c3 h3                (plms.py:230-244; Adams-Bashforth weights)
 *   pred_x0 = (x - sqrt(1-a_t) e') / sqrt(a_t);  x_prev = sqrt(a_prev) pred_x0 + sqrt(1-a_prev) e'
 *   coef = {c0,c1,c2,c3, sqrt_one_minus_at, 1/sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev)} (host floats).
 * ------------------------------------------------------------------------------------------ */
int pbe_plms_pack_input(const float* x, const float* z_inpaint, const float* mask, void* x9,
                        int32_t B, int32_t HW, int32_t dup, pbe_stream_t stream);
int pbe_plms_update(const void* eps_out, int32_t ld, int32_t dup, float cfg_scale, const float* x,
                    const float* h1, const float* h2, const float* h3, const float* coef8,
                    float* e_t, float* x_prev, float* pred_x0, int32_t B, int32_t HW,
                    pbe_stream_t stream);

/* pbe_dpmpp_update — one step of the DPM-Solver++(2M) sampler (ldm/models/diffusion/dpm_solver.py), one launch:
 *   e      = e_u + scale (e_c - e_u)                        (dup == 2; dup == 1: e = eps_out - the expression of the PLMS update)
 *   x0     = (x - sigma_t e) * (1 / alpha_t)                (the data prediction: pred_x0, and the next step's history)
 *   x_next = kx x + k0 x0 [+ k1 x0_prev]                    (first order: k1 = 0; second order: x0_prev = the previous step's x0)
 * eps_out fp16 NHWC [dup*B, HW, ld], ld >= 4 (channels 4.. are padding, never read; with ld % 4 == 0 and an 8-byte aligned base the
 * 4 values of a token are one read); x, x0_prev, x0_out, x_next fp32 NCHW [B,4,HW]; coef5 = {sigma_t, 1/alpha_t, kx, k0, k1} (host
 * floats).  x0_prev may be NULL (then k1 must be 0: anything else is refused), x0_out may be NULL (the last step needs no history).
 * fp32 throughout, every multiply-add fused: 4 roundings in x0, 7 in x_next. */
int pbe_dpmpp_update(const void* eps_out, int32_t ld, int32_t dup, float cfg_scale, const float* x, const float* x0_prev,
                     const float* coef5, float* x0_out, float* x_next, int32_t B, int32_t HW, pbe_stream_t stream);

/* Stochastic sampler options reachable from the reference CLI (scripts/inference.py:164,342 --ddim_eta; plms.py:150-153 / ddim.py:178-181):
 * pbe_axpy_f32          y += a * x : the sigma_t * noise * temperature term of a DDIM step with eta > 0 (ddim.py:236-238);
 * pbe_qsample_blend_f32 out = (sqrt_ac x0 + sqrt_1m_ac noise) * mask + (1 - mask) * img : img_orig = q_sample(x0, ts) blended under `mask`
 *                       (fp32 NCHW [B,C,HW]; mask [B,1,HW] or [B,C,HW]).  The noise tensors are the caller's (the reference draws them
 *                       from the device RNG: not reproducible across devices, so parity uses injected noise). */
int pbe_axpy_f32(float* y, float a, const float* x, int64_t n, pbe_stream_t stream);
int pbe_qsample_blend_f32(const float* x0, const float* noise, const float* mask, const float* img, float sqrt_ac, float sqrt_1m_ac,
                          float* out, int32_t B, int32_t C, int32_t HW, int32_t mask_channels, pbe_stream_t stream);

/* pbe_posterior_sample — distributions.py:25-37 + latent_diffusion.py:262:
 * moments fp16 NHWC [B,HW,ld] (mean 0..3 | logvar 4..7), eps fp32 NCHW [B,4,HW] ->
 * z fp32 NCHW = scale * (mean + exp(0.5 clamp(logvar,-30,20)) * eps). */
int pbe_posterior_sample(const void* moments, int32_t ld, const float* eps, float* z, int32_t B,
                         int32_t HW, float scale, pbe_stream_t stream);

/* pbe_scale_latent_f16 — decode_first_stage prologue (latent_diffusion.py:454,506): fp32 NCHW
 * [B,C>=4,HW] -> fp16 NHWC [B,HW,8] of (1/scale_factor) * z[:, :4]. */
int pbe_scale_latent_f16(const float* z, void* out, int32_t B, int32_t C, int32_t HW, float inv_scale,
                         pbe_stream_t stream);

/* pbe_clip_patchify_f16 — HF CLIPVisionEmbeddings patch conv (14x14 s14, no bias) as im2col:
 * pixels fp32 NCHW [B,3,S,S] -> fp16 [B*(S/P)^2, Kp], k = c*P*P + ky*P + kx, zero padded to Kp. */
int pbe_clip_patchify_f16(const float* pixels, void* out, int32_t B, int32_t S, int32_t P, int32_t Kp,
                          pbe_stream_t stream);

/* pbe_add_rows_f16 — Y[b, r, :] = X[r, :] + V[:]  for r in [0, rows): class-token row of the CLIP
 * embedding (class_embedding + position_embedding[0]) written to tokens[b, 0, :]. */
int pbe_bcast_row_f16(const void* a, const void* b, void* Y, int32_t B, int32_t C, int64_t y_bs,
                      pbe_stream_t stream);

/* pbe_image_post_f32 — scripts/inference.py:347: clamp((x+1)/2, 0, 1) of fp16 NHWC [B,HW,ld] -> fp32 NCHW [B,3,HW]. */
int pbe_image_post_f32(const void* src, float* dst, int32_t B, int32_t HW, int32_t ld, pbe_stream_t stream);

/* pbe_resize_bilinear_f32 — scripts/inference.py:332 `Resize([h, w])(mask)` on fp32 planes [planes, Hin, Win] -> [planes, Hout, Wout]:
 * bilinear, align_corners = False; antialias = 1 is the triangle filter of torchvision >= 0.17 (F.interpolate(antialias=True)),
 * antialias = 0 the 2-tap form of the reference's pinned torchvision 0.12. */
int pbe_resize_bilinear_f32(const float* src, float* dst, int32_t planes, int32_t Hin, int32_t Win, int32_t Hout,
                            int32_t Wout, int32_t antialias, pbe_stream_t stream);

/* Image I/O on the device (scripts/inference.py:305-322 pre-processing, :346-399 outputs; test_bench_dataset.py:74-99):
 * pbe_u8_to_planes_f32     u8 HWC [B, H*W, C] -> fp32 CHW planes: (v/255 - mean[c]) / std[c]  (ToTensor + Normalize), or the mask
 *                          forms binarize = 1: (1 - v/255) thresholded at 0.5 (inference.py:311-315), 2: 1 - v/255 (test bench);
 * pbe_mul_planes_f32       out[b,c] = x[b,c] * m[b,0]                                  (inpaint_image = image * mask, :319);
 * pbe_planes_to_u8_canvas  one CHW image -> a rectangle of a u8 HWC canvas: trunc(255 * clamp(x * a[c] + b[c], 0, 1)); the result /
 *                          GT / inpaint / ref / mask files and the 4-tile grid (make_grid, pad 2) are such rectangles. */
int pbe_u8_to_planes_f32(const void* src, float* dst, int32_t B, int32_t C, int32_t HW, const float* mean3, const float* std3,
                         int32_t binarize, pbe_stream_t stream);
int pbe_mul_planes_f32(const float* x, const float* m, float* out, int32_t B, int32_t C, int32_t HW, pbe_stream_t stream);
int pbe_planes_to_u8_canvas(const float* src, void* canvas, int32_t H, int32_t W, int32_t Hc, int32_t Wc, int32_t y0, int32_t x0,
                            const float* a3, const float* b3, int32_t bcast, pbe_stream_t stream);

/* Windowed pre/post-processing (pbe_amd/csrc/window.hip; not in the reference): inpaint a region of a picture of any size and paste it
 * back.  picture: u8 [Hs, Ws, 3] contiguous; mask: u8 [Hs, Ws], a byte >= 128 is the hole; window (y0, x0, wh, ww) inside the picture;
 * working size (H, W).  Edges up to 16384.  One picture per call.
 * AA(src, (h, w) -> (h', w')) below is the antialiased triangle filter of pbe_resize_bilinear_f32 (ATen upsample_bilinear2d_aa), per axis
 * n -> n': scale s = n / n', support sup = max(s, 1), centre c = s (o + 0.5), taps lo = max((int)(c - sup + 0.5), 0) ..
 * min((int)(c + sup + 0.5), n) - 1, weight_j = max(1 - |j + 0.5 - c| / sup, 0) / (their sum) - evaluated in integers: with den = 2 max(n, n'),
 * wnum_j = max(den - |(2j + 1) n' - (2o + 1) n|, 0) and weight_j = (float)wnum_j / (float)(sum_j wnum_j), so neither the tap range nor a
 * weight carries a coordinate rounding and at n = n' the filter is exactly the identity.  out = sum_k wy_k * (sum_j src[k, j] * wx_j): row
 * sums first, one fmaf per tap in tap order (r = fmaf(v, wx, r), then acc = fmaf(r, wy, acc)), weights recomputed per tap (no tap cap,
 * no scratch).
 * pbe_window_image_u8_f32    dst[c, Y, X] = (AA(window bytes / 255, (wh, ww) -> (H, W))[c] - mean[c]) / std[c], fp32 [3, H, W]; taps outside
 *                            the window are clipped as at an image edge; v / 255, the subtraction and the division are IEEE fp32 in the order
 *                            of pbe_u8_to_planes_f32, so a window of the working size gives that kernel's bits.
 * pbe_window_mask_u8_f32     dst[0, Y, X] = 0 if any mask byte >= 128 lies in window rows (Y*wh)/H .. ceil((Y+1)*wh/H) - 1 and the columns
 *                            likewise (integer arithmetic), else 1; fp32 [1, H, W].  Exact; at wh = H, ww = W it is binarize = 1 above.
 * pbe_feather_alpha_f32      alpha[y, x] = (float)box_r(dilate_r(hole))(y0 + y, x0 + x) / (float)(2r+1)^2, fp32 [wh, ww]: dilate_r = maximum and
 *                            box_r = integer count over the (2r+1)^2 square, both on picture coordinates clamped to the picture (replicate
 *                            padding; they read the mask beyond the window); one IEEE division.  0 <= r <= 2047.  Four separable passes
 *                            through `workspace`, at least pbe_feather_alpha_workspace_bytes(wh, ww, r) bytes of device scratch.
 * pbe_paste_window_u8        for every window pixel with alpha > 0 and each channel: res = AA(result, (H, W) -> (wh, ww)), o = byte / 255,
 *                            v = fmaf(alpha, res, (1 - alpha) * o), byte = rint(255 * clamp(v, 0, 1)) (half to even); result fp32 [3, H, W].
 *                            Pixels with alpha == 0 and everything outside the window are not written.
 * pbe_paste_window_tone_u8   pbe_paste_window_u8 with res = fmaf(gain3[c], res, offset3[c]) per channel between the filter and the blend
 *                            (gain3 / offset3: three floats each on the HOST, passed by value into the launch): the tone map of
 *                            pbe_tone_stats_i64 below.  Gain 1 and offset 0 give pbe_paste_window_u8's bytes.
 * pbe_paste_window_field_u8  pbe_paste_window_u8 with res[c] += f_c between the filter and the blend, f_c the bilinear sample of `field`
 *                            (fp32 [3, Hc, Wc] on the device, pbe_tone_field_f32's, Hc = ceil(H / cell), Wc = ceil(W / cell)) at the window
 *                            pixel's centre: ty = fmaf(oy + 0.5f, sy, -0.5f) with sy = (float)((double)H / ((double)wh cell)) computed on
 *                            the host, iy = floorf(ty), rows clamp(iy) and clamp(iy + 1) to 0 .. Hc - 1, fraction ty - iy, fmaf(t, b - a, a)
 *                            along y and then along x (x alike).  A zero field gives pbe_paste_window_u8's bytes, a constant field b those
 *                            of pbe_paste_window_tone_u8 at gain 1 and offset b. */
int pbe_window_image_u8_f32(const void* picture, float* dst, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t wh, int32_t ww,
                            int32_t H, int32_t W, const float* mean3, const float* std3, pbe_stream_t stream);
int pbe_window_mask_u8_f32(const void* mask, float* dst, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t wh, int32_t ww,
                           int32_t H, int32_t W, pbe_stream_t stream);
size_t pbe_feather_alpha_workspace_bytes(int32_t wh, int32_t ww, int32_t r);
int pbe_feather_alpha_f32(const void* mask, float* alpha, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t wh, int32_t ww, int32_t r,
                          void* workspace, size_t workspace_bytes, pbe_stream_t stream);
int pbe_paste_window_u8(const float* result, const float* alpha, void* picture, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t wh,
                        int32_t ww, int32_t H, int32_t W, pbe_stream_t stream);
int pbe_paste_window_tone_u8(const float* result, const float* alpha, void* picture, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0,
                             int32_t wh, int32_t ww, int32_t H, int32_t W, const float* gain3, const float* offset3, pbe_stream_t stream);

/* Tone of a pasted window (pbe_amd/csrc/tone.hip; not in the reference): the sums from which pbe_amd.window.fit_tone fits one affine map
 * per window and channel that brings the result's known pixels back onto the original's.
 * pbe_tone_stats_i64         image fp32 [B, 3, H, W] model-normalised in [-1, 1] (pbe_window_image_u8_f32 at mean = std = 0.5), result fp32
 *                            [B, 3, H, W] in [0, 1] (pbe_image_post_f32), sel fp32 [B, 1, H, W] -> stats int64 [B, 3, 6].  Per pixel and
 *                            channel o = (int)rintf(255 c01(0.5 x + 0.5)) and q = (int)rintf(255 c01(r)), c01(v) = fminf(fmaxf(v, 0), 1)
 *                            (a NaN counts as 0; half to even); a pixel counts iff sel >= 0.5f (a NaN selects nothing).  Row [b, c] is
 *                            n, sum o, sum q, sum o^2, sum q^2, sum o q over the counted pixels of sample b; n is the same in a sample's
 *                            three rows.  EVERY element is written (no counted pixel: six zeros): neither stats nor the workspace need
 *                            clearing.  Integer sums only, no atomics: per-thread 32-bit accumulators, a wave and a block reduction,
 *                            64-bit block partials in `workspace` (at least pbe_tone_stats_workspace_bytes(B, H, W) bytes of device
 *                            scratch, 8-byte aligned) and a finalise kernel - the table does not depend on the order the blocks ran in.
 *                            H, W <= 16384, B <= 65535. */
int pbe_paste_window_field_u8(const float* result, const float* alpha, void* picture, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0,
                              int32_t wh, int32_t ww, int32_t H, int32_t W, const float* field, int32_t Hc, int32_t Wc, int32_t cell,
                              pbe_stream_t stream);
size_t pbe_tone_stats_workspace_bytes(int32_t B, int32_t H, int32_t W);
int pbe_tone_stats_i64(const float* image, const float* result, const float* sel, int64_t* stats, int32_t B, int32_t H, int32_t W,
                       void* workspace, size_t workspace_bytes, pbe_stream_t stream);

/* A tone that varies across the window (pbe_amd/csrc/tone_field.hip; not in the reference): a low-frequency field of the difference o - q
 * of the two bytes of pbe_tone_stats_i64, which pbe_paste_window_field_u8 adds to the pasted window.
 * pbe_tone_cells_i32         image, result, sel as for pbe_tone_stats_i64; cell in {4, 8, 16, 32, 64} working pixels -> cells int32
 *                            [B, 4, Hc, Wc], Hc = ceil(H / cell), Wc = ceil(W / cell): plane 0 the number n of pixels of the cell with
 *                            sel >= 0.5f, planes 1 .. 3 sum (o - q) over them per channel; the cells of the last row and column may be
 *                            ragged.  Integer sums (|sum| <= 255 cell^2 < 2^21), no atomics; every element is written exactly once, so
 *                            `cells` needs no clearing.  4- / 2-wide loads where W is a multiple of 4 / 2 and the three tensors start on
 *                            16 / 8 bytes, else scalar ones.  H, W <= 16384, B <= 65535.
 * pbe_tone_field_f32         cells -> field fp32 [B, 3, Hc, Wc] in [0, 1] units by a pull-push fill.  PULL: level 0 is the table, level
 *                            l + 1 has ceil(Hl / 2) x ceil(Wl / 2) cells, each the int64 sum of its up to four children, up to 1 x 1.
 *                            MEAN at every level: m = clamp((float)((double)S / (255.0 (double)n)), -limit, +limit) where n > 0, else 0.
 *                            PUSH: v_top = m_top; below it u = the parent field at the child's centre, separably: along y rows a = i >> 1
 *                            and b = clamp(a + (i odd ? 1 : -1), 0, H(l+1) - 1), r = fmaf(0.25f, b - a, a), then the same along x;
 *                            w = (float)min(n, cell^2) / (float)cell^2 and v = fmaf(w, m - u, u).  A sample whose whole-window n is 0 or
 *                            below min_pixels gets a field of zeros.  One launch, one workgroup per sample; the pyramid lives in
 *                            `workspace` (at least pbe_tone_field_workspace_bytes(B, Hc, Wc) bytes of device scratch, 8-byte aligned),
 *                            which needs no clearing; every element of `field` is written.  limit finite and > 0, min_pixels >= 0,
 *                            Hc Wc <= 2^20, B <= 65535. */
int pbe_tone_cells_i32(const float* image, const float* result, const float* sel, int32_t* cells, int32_t B, int32_t H, int32_t W, int32_t cell,
                       pbe_stream_t stream);
size_t pbe_tone_field_workspace_bytes(int32_t B, int32_t Hc, int32_t Wc);
int pbe_tone_field_f32(const int32_t* cells, float* field, int32_t B, int32_t Hc, int32_t Wc, int32_t cell, float limit, int32_t min_pixels,
                       void* workspace, size_t workspace_bytes, pbe_stream_t stream);

/* Holes of a mask (pbe_amd/csrc/holes.hip; not in the reference): connected components of the hole, for one window per hole
 * (pbe_amd.window.plan_holes, pipeline.inpaint_holes).  mask: u8 [Hs, Ws] contiguous, a byte >= 128 is a hole pixel; labels: i32 [Hs, Ws]
 * contiguous.  Edges up to 16384, so a linear index y * Ws + x fits an int32.  Integers only: every output is unique and compared by
 * equality.  Caller-owned buffers, an explicit stream, no synchronisation and no host read-back; no workgroup waits for another.
 * pbe_mask_components_u8_i32 labels[y, x] = -1 on a non-hole pixel, else the SMALLEST linear index of any pixel of its connected component;
 *                            connectivity 8 (diagonal neighbours join) or 4, anything else is an error.  Every element of labels is written,
 *                            no byte outside mask is read.  Union-find on the label plane itself: 64 x 16 tiles in LDS, atomicMin links
 *                            across the tile borders in global memory, a flattening pass (three launches).  `workspace`: at least
 *                            pbe_mask_components_workspace_bytes(Hs, Ws) bytes of device scratch.
 * pbe_component_boxes_i32    labels as written above -> *count = the number of components (device int32; the true number even above
 *                            `capacity`) and, if count <= capacity, rows 0 .. count - 1 of table (i32 [capacity, 6]) = (label, ya, yb, xa,
 *                            xb, area) of the distinct components, bounds inclusive, area in pixels, in unspecified order; rows from count
 *                            on are not written.  If count > capacity the table's content is unspecified (nothing outside it is written).
 *                            1 <= capacity <= 2^20.  A wave sums the pixels that share a label over 16 rows of 64 columns before its atomics.  `workspace`: at
 *                            least pbe_component_boxes_workspace_bytes(Hs, Ws, capacity) bytes.
 * pbe_select_components_u8   out_mask[y, x] = 255 if labels[y, x] is in `wanted` (device i32 [n_wanted], ASCENDING, 0 <= n_wanted <= 4096),
 *                            else 0; u8 [Hs, Ws], every byte written. */
size_t pbe_mask_components_workspace_bytes(int32_t Hs, int32_t Ws);
int pbe_mask_components_u8_i32(const void* mask, int32_t* labels, int32_t Hs, int32_t Ws, int32_t connectivity, void* workspace,
                               size_t workspace_bytes, pbe_stream_t stream);
size_t pbe_component_boxes_workspace_bytes(int32_t Hs, int32_t Ws, int32_t capacity);
int pbe_component_boxes_i32(const int32_t* labels, int32_t* table, int32_t* count, int32_t Hs, int32_t Ws, int32_t capacity, void* workspace,
                            size_t workspace_bytes, pbe_stream_t stream);
int pbe_select_components_u8(const int32_t* labels, const int32_t* wanted, int32_t n_wanted, void* out_mask, int32_t Hs, int32_t Ws,
                             pbe_stream_t stream);

/* The shape of a mask (pbe_amd/csrc/maskshape.hip; not in the reference): the exact squared Euclidean distance map of a mask and what
 * grows, shrinks, closes, opens and boxes a hole with it (pbe_amd.ops.mask_grow ..., pbe_amd.window.shape_mask).  mask: u8 [Hs, Ws]
 * contiguous, a byte >= 128 is a hole pixel; edges up to 16384.  Integers only, no atomics: every output is unique and compared by
 * equality.  Caller-owned buffers, an explicit stream.
 * pbe_mask_dist2_u8_i32      d2[y, x] = min(min over (y', x') in S of (y - y')^2 + (x - x')^2, rmax^2 + 1), i32 [Hs, Ws]; S = the hole pixels
 *                            (to_hole = 1) or the non-hole pixels (to_hole = 0) INSIDE the picture - the outside is neither, so a hole that
 *                            touches the border is not eroded from that side; an empty S gives rmax^2 + 1 everywhere.  0 <= rmax <= 2047.
 *                            The true Euclidean minimum at any size, no chamfer: a column pass (rows since the last pixel of S, down and up,
 *                            saturated at rmax + 1, 16 bits per pixel in `workspace`) and a row pass (per pixel the taps dx = 0, +-1, ...
 *                            of dx^2 + g^2 from LDS until dx^2 >= the best so far).  `workspace`: 2-byte aligned, at least
 *                            pbe_mask_dist2_workspace_bytes(Hs, Ws) bytes (0 for edges out of range).  No synchronisation.
 * pbe_mask_from_dist2_u8     out_mask[y, x] = 255 where d2 <= t2 (above = 0) or where d2 > t2 (above = 1), else 0; t2 >= 0; every byte written.
 *                            Growing a hole by a disc of radius r is d2(to_hole = 1) <= floor(r^2), shrinking it d2(to_hole = 0) > floor(r^2).
 * pbe_fill_boxes_u8          boxes: device i32 [n, 4], rows (ya, yb, xa, xb) inclusive, 0 <= n <= 4096 -> out_mask = 255 inside any box, else
 *                            0; every byte written, n = 0 gives zeros.  A row that is not a box inside the picture (ya > yb, xa > xb, a
 *                            bound outside) is refused before anything is launched: for that the rows are read back on `stream` (at most
 *                            64 KiB), so THIS entry point waits for the stream and cannot be captured into a graph. */
size_t pbe_mask_dist2_workspace_bytes(int32_t Hs, int32_t Ws);
int pbe_mask_dist2_u8_i32(const void* mask, int32_t* d2, int32_t Hs, int32_t Ws, int32_t to_hole, int32_t rmax, void* workspace,
                          size_t workspace_bytes, pbe_stream_t stream);
int pbe_mask_from_dist2_u8(const int32_t* d2, void* out_mask, int32_t Hs, int32_t Ws, int32_t t2, int32_t above, pbe_stream_t stream);
int pbe_fill_boxes_u8(const int32_t* boxes, int32_t n, void* out_mask, int32_t Hs, int32_t Ws, pbe_stream_t stream);

/* The exemplar cut from a uint8 picture on the device (pbe_amd/csrc/exemplar.hip; not in the reference, which resizes the exemplar with
 * PIL on the host, scripts/inference.py:309): Pillow's 8-bit resize in its own integers, byte-equal to Image.resize.  Additive to ABI 8.
 * The tables of one axis come from the host (pbe_amd.exemplar.resample_tables: Pillow's precompute_coeffs + normalize_coeffs_8bpc in
 * float64): bounds i32 [out, 2], rows (xmin, n), and coeffs i32 [out, ksize], the n weights of an output index rounded to 22 fractional
 * bits, zero past n; both on the device, 4-byte aligned, 1 <= ksize <= 98305.  A pass gives, per byte,
 *   clip((2^21 + sum_{x < n} src[xmin + x] * coeffs[i, x]) >> 22, 0, 255)       int32 accumulator, arithmetic shift, no float.
 * The kernels clamp xmin, n and every tap to the operands, so a wrong table cannot make them read outside; it gives wrong bytes.
 * pbe_resample_h_u8          picture u8 [Hs, Ws, 3], its rows first .. last - 1 -> out u8 [last - first, ow, 3]: the horizontal pass.  mask
 *                            (may be NULL) u8 [Hs, Ws]: a source pixel whose mask byte is < 128 reads as the three bytes fill3 (HOST
 *                            pointer, required with a mask).  The source segment of 64 output columns is staged through LDS in rounds
 *                            of 4096 pixels (whole aligned dwords, each byte once per workgroup); ksize is a loop, not a register array.
 * pbe_resample_v_u8          src u8 [rows, ow, 3] -> out u8 [oh, ow, 3]: the vertical pass (bounds count rows of src).  mask (may be NULL)
 *                            u8 [rows, ow] / fill3 as above, for launches on the picture itself.  planes (may be NULL) fp32 [3, oh, ow]
 *                            takes (byte / 255 - mean3[c]) / std3[c] with the expression of pbe_u8_to_planes_f32 (csrc/u8_norm.h): its bits.
 *                            With bounds (y, 1) and coefficient 2^22 the pass is a copy (what Pillow does when it skips both passes).
 * pbe_resample_workspace_bytes  bytes of the intermediate of `rows` rows of `ow` pixels (0 for edges outside 1 .. 16384).
 * pbe_mask_box_i32           mask u8 [Hs, Ws] -> table i32 [bands, 4], bands = pbe_mask_box_bands(Hs) = ceil(Hs / 32): row b holds
 *                            (ya, yb, xa, xb), inclusive, of the bytes >= 128 in mask rows 32 b .. 32 b + 31, or four -1 where there is
 *                            none.  No atomics: one workgroup per band, every element written once; the caller reduces the rows.
 * All edges 1 .. 16384.  No synchronisation; the entry points return PBE_EINVAL for null / misaligned / out-of-range arguments. */
size_t pbe_resample_workspace_bytes(int32_t rows, int32_t ow);
int pbe_resample_h_u8(const void* picture, const void* mask, const uint8_t* fill3, void* out, int32_t Hs, int32_t Ws, int32_t first, int32_t last,
                      int32_t ow, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, pbe_stream_t stream);
int pbe_resample_v_u8(const void* src, const void* mask, const uint8_t* fill3, void* out, float* planes, int32_t rows, int32_t ow, int32_t oh,
                      const int32_t* bounds, const int32_t* coeffs, int32_t ksize, const float* mean3, const float* std3, pbe_stream_t stream);
int32_t pbe_mask_box_bands(int32_t Hs);
int pbe_mask_box_i32(const void* mask, int32_t* table, int32_t Hs, int32_t Ws, int32_t bands, pbe_stream_t stream);

/* Noise as a function of per-sample seeds (csrc/noise.hip; ABI 8 additive): Philox4x32-10 as published (Salmon et al., SC'11; multipliers
 * 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, 10 rounds).  For sample b and element e of its flat array:
 *   key = (seed lo32, seed hi32), seeds[b] read as unsigned 64 bits;  counter = (e / 4, sub[b], stream_id lo32, stream_id hi32).
 * pbe_philox_u32        out u32 [B, n_words]: word w of a sample is x[w % 4] of counter w / 4.
 * pbe_randn_philox_f32  out fp32 [B, n] = a * out + b * z.  From the words of counter q = e / 4: u = ((x0 >> 8) + 1) 2^-24 in (0, 1],
 *                       v = (x1 >> 8) 2^-24 in [0, 1), r = sqrtf(-2 logf(u)), (s, c) = sincospif(2 v); elements 4q, 4q + 1 are r c, r s and
 *                       4q + 2, 4q + 3 the same from (x2, x3).  With a == 0 out is never read (NaN in it does not come through) and the
 *                       result is b * z; otherwise it is fmaf(b, z, a * out): with a == 1 the bits of pbe_axpy_f32 on a plain draw.
 * seeds i64 [B] and sub i32 [B] (NULL: 0) are device arrays.  A value depends on (seed, sub, stream_id, e) alone: not on B, the sample's
 * place in the batch, n, or the alignment of out (4 bytes is enough).  No state, no atomics, no synchronisation (capturable); every
 * element is written exactly once.  B <= 65535, n <= 2^32 - 4. */
int pbe_philox_u32(uint32_t* out, const int64_t* seeds, const int32_t* sub, int32_t B, int64_t n_words, uint64_t stream_id, pbe_stream_t stream);
int pbe_randn_philox_f32(float* out, const int64_t* seeds, const int32_t* sub, int32_t B, int64_t n, uint64_t stream_id, float a, float b,
                         pbe_stream_t stream);

/* pbe_tune— developer knobs for A/B runs in one process (never needed for correctness):
 * key 1: force an implicit-GEMM tile config index (-1 = heuristic); key 2: allow split-K (0/1);
 * key 3: attention queries-per-wave factor (0 = heuristic, 1, 2); key 4: ping-pong main loop of the halo-resident conv tiles (0/1);
 * key 5: per-launch choice of the XCD tile order (m fastest where that fetches fewer bytes into the 8 L2s; 0 = always n fastest);
 * key 6: attention at d = 40 keeps the softmax reference maximum in the head-dim padding (0 = the multiply-add form);
 * key 7: rows per thread of the two-pass GroupNorm kernels (default 16); key 8: extra dynamic LDS bytes per attention workgroup
 *        (fewer resident workgroups per CU: occupancy experiments).
 */
int pbe_tune(int32_t key, int32_t value);

/* ---- per-kernel-class timing with HIP events on the launch stream (bench.py roofline leg) ---- */
int pbe_prof_enable(int32_t on);
int pbe_prof_reset(void);
/* out[5*k + {0..4}] = {launches, total ms, total work (FLOP for the matrix-core classes, bytes otherwise), total algorithmic bytes,
 * roofline ms = sum over launches of max(FLOP / 2.5e15, bytes / 8e12) - the bound that binds each launch} for class k; returns
 * #classes.  Synchronises the recorded events (call outside any timed region). */
int pbe_prof_collect(double* out, int32_t max_classes);
const char* pbe_prof_class_name(int32_t klass);

#ifdef __cplusplus
}
#endif
#endif /* PBE_HIP_H */
