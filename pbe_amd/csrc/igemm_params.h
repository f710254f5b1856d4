// Kernarg struct, diagnostics macros and small helpers shared by the implicit-GEMM kernel (igemm_kernel.h, igemm_astat.hip) and its host side (igemm_plan.h).
#pragma once
#include <cstddef>
#include <type_traits>
#include <utility>
#include "common.h"
#include "../../include/pbe_hip.h"

struct IGemmP {
    // ---- HEAD: everything a workgroup reads between kernel entry and its first LDS-DMA, contiguous so the scalar loads of the prologue
    //      come from the first cache lines of the kernarg segment (offsets pinned by the static_asserts below).  A REORDER ONLY: the
    //      compiler still fetches the head as the code reaches it, and a mode skips the fields of the others
    //      (hw / mg_hw .. mg_kb: MODE 1; h_*: MODE 2).  astat_regs_kernel reads mg_tdiv (divisor tiles_m) and mg_per_blk (its run) ----
    const h16* A; const h16* A2; const h16* W;
    long lda, lda2, ldw;
    long sA, sW;
    int M, N, K, K1;
    int splits;
    int m_fast;     // an XCD's run of tiles walks m fastest (one weight panel, many activation rows) instead of n fastest (launch_cfg)
    // launch-invariant prologue values (igemm_prologue, host): the kernel holds no run-time division before its first fetch.
    // mg_* = floor(2^32 / divisor) for udiv_mg (exact for every 32-bit numerator), mh_* = ceil(2^20 / divisor) for the halo rows' udiv_h
    int tdiv; unsigned mg_tdiv;                          // tile id -> (tm_i, tn_i): divisor tiles_m (m fastest) or tiles_n
    int split_per;                                       // split-K: k-tiles (MODE 0 / 1) or channel blocks (MODE 2) per slice
    int sv_ns;                                           // samples per tile of the staged epilogue vectors
    int sv_gdiv; unsigned mg_sv_gdiv;                    // row tiles per sample (group_rows / BM, >= 1): first sample of a tile = tm_i / sv_gdiv
    // conv gather
    int H, Wd, C1, C2, Ho, Wo, cstride, pad, ups, cb;   // cb = channel block of the K order (multiple of 64)
    int phase;                                           // MODE 1: nearest-2x upsample + 3x3 conv as FOUR 2x2 convs on the source grid (see the tap table); blockIdx.y = output phase
    int th;                                              // MODE 2: image rows per tile (tile = th full rows, or whole images)
    int hw; unsigned mg_hw, mg_wo;                       // MODE 1 tap table: output pixels per sample, m -> (b, oy, ox)
    int per_blk; unsigned mg_per_blk, mg_kb;             // MODE 1 split-K resume: k-tiles per channel block (taps x cb / 64), per tap
    // MODE 2 halo geometry: row stride W + 1, halo rows per (sub-)image, whole images per tile, valid halo rows, row tiles per image,
    // log2 of the image width and of the pixels per (sub-)image (both powers of two: halo_rows)
    int h_hw2, h_hps, h_nsub, h_rows, h_tpi; unsigned mg_h_tpi, mh_hps, mh_hw2; int h_lgw, h_lgimg;
    // ---- TAIL: epilogue, statistics and diagnostic fields ----
    h16* C;
    const float* bias; const h16* rowvec; const h16* resid;
    long ldc, ldr;
    int ldv, group_rows;
    long sC, sR;
    float alpha; int act; int bias_row; int vec;
    // fp8 (OCP e4m3) operands: rows are bytes (the loader sees them as K/2 halfs); C = acc * sa[m] * sw[n] (* alpha) + ...
    const float* sa; const float* sw; long ssa, ssw;
    // split-K: gridDim.z slices of the k-tile range, fp32 partial slabs [splits][M][N]
    float* ws;
    // extended epilogue of the dense tiles (EX instantiations, the transformer block's GEMM chain; ldm/modules/attention.py:198-252):
    int alpha_cols;                  // > 0: alpha multiplies columns n < alpha_cols only (q of a fused q | k | v launch, pre-scaled for the attention kernel)
    const float* ln_stat;            // LayerNorm folded into THIS GEMM: A holds the raw rows x, W = W * gamma, bias = W beta (+ bias), and
    int ln_parts; long ln_ld;        //   the epilogue forms rstd[m] * (acc - mean[m] * colsum[n]); (sum, sumsq) of row m = sum over ln_parts float2 partials
    const float* ln_c1; float ln_eps; double ln_inv_k;
    long rstat_ld;
    float* rstat;                    // this launch's OUTPUT rows feed a LayerNorm: per (column tile, row) partial (sum, sumsq) of the stored fp16 values
    h16* vt; int vt_col0, vt_tok;    // columns n >= vt_col0 are stored TRANSPOSED: vt[b * vt_bs + (n - vt_col0) * vt_rs + tok], m = b * vt_tok + tok
    long vt_bs, vt_rs;               //   (V^T for the attention kernel from the same launch as q | k)
    // conv output feeds a GroupNorm: per (sample, row block of the tile grid, group) partial (sum, sumsq) of the STORED fp16 values (after the
    // residual add), in pbe_groupnorm_f16's partial layout [B][blocks][groups][2] - the norm's statistics pass is then not launched
    float* gstat; int gs_cg, gs_groups, gs_hw;      // channels per group, groups of the whole tensor, output pixels per sample
    int* gs_report;                                 // HOST pointer (launch_cfg): row blocks per sample the launch writes partials for, 0 = this tile cannot
    // MX-fp8 output (EX_MX instantiations, pbe_gemm_mx8out_f16): column ranges [mx_c0, mx_c0 + width) of the output leave as OCP e4m3 bytes
    // + E8M0 scales in pbe_quant_mx8_f16's layouts (include/pbe_hip.h) instead of fp16; C is not written.  Shared B, H, N, D (N % 64 == 0);
    // mx_crow: rows are the H*D channels of V^T, columns its N tokens, blockIdx.y = sample (the swapped V^T GEMM); else rows are tokens
    unsigned char* mx_data[3]; unsigned char* mx_scale[3];
    int mx_c0[3], mx_layout[3]; float mx_alpha[3]; int mx_nr, mx_crow;
    int mx_H, mx_N, mx_D, mx_DP, mx_DV;
    // GroupNorm folded into A (EX_GN instantiations, pbe_gemm_gnfold_f16): A holds the raw rows x, the tile's rows belong to ONE sample and every A
    // fragment becomes (h16)(x * sc[k] + sh[k]) behind its LDS read - the value and the rounding of gn_apply_kernel (norm.hip).  gn_tab: fp32
    // [samples][K / 8][16], sc | sh of 8 consecutive channels (pbe_groupnorm_table_f32); gn_tdiv = row tiles per sample
    const float* gn_tab; int gn_tdiv; unsigned mg_gn_tdiv;
    int sv_ok;      // bias + row vector of a tile come from LDS (set per tile shape in launch_cfg)
#ifdef PBE_STAMPS
    unsigned long long* stamps;     // diagnostic build only (tools/phase_stamps.py): 16 words per workgroup
#endif
};
// the head is what the host fills for the prologue and what a workgroup fetches first: four 64-byte lines of the kernarg segment
constexpr size_t kIGemmHeadBytes = offsetof(IGemmP, C);
static_assert(offsetof(IGemmP, A) == 0 && offsetof(IGemmP, lda) == 24 && offsetof(IGemmP, M) == 64 && offsetof(IGemmP, tdiv) == 88 &&
              offsetof(IGemmP, H) == 112 && offsetof(IGemmP, hw) == 160 && offsetof(IGemmP, h_hw2) == 184 && kIGemmHeadBytes == 224,
              "IGemmP: the prologue head moved");
static_assert(offsetof(IGemmP, bias) == 232 && offsetof(IGemmP, ldc) == 256 && offsetof(IGemmP, alpha) == 296 && offsetof(IGemmP, ws) == 344 &&
              offsetof(IGemmP, ln_stat) == 360, "IGemmP: the epilogue tail moved");

// Diagnostic build (-DPBE_STAMPS, never the shipped library): wave 0 of every workgroup records s_memtime at its phase
// boundaries into a buffer of its own; no output value depends on a stamp (cdna_hip_programming.md section 7, in-kernel stamps).
#ifdef PBE_STAMPS
#define PBE_STAMP(i)                                                                                                   \
    do {                                                                                                               \
        if (p.stamps && threadIdx.x == 0) {                                                                            \
            const long wg_ = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;                     \
            p.stamps[wg_ * 16 + (i)] = ((i) == 7 || (i) == 8) ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime();    \
        }                                                                                                              \
    } while (0)
// main-loop accounting of wave 0: cycles inside the counted vmcnt waits (words 9), the barrier after the fragment reads (10) and
// the barrier that ends a k-tile (11), DMA issue + fragment reads up to lgkmcnt(0) (12), the MFMA block (13)
#define PBE_ACC_DECL unsigned long long acc_w_ = 0, acc_b1_ = 0, acc_b2_ = 0, acc_r_ = 0, acc_m_ = 0, acc_t_ = 0
#define PBE_ACC_T0() acc_t_ = __builtin_amdgcn_s_memtime()
#define PBE_ACC(v) v += __builtin_amdgcn_s_memtime() - acc_t_
#define PBE_ACC_STORE()                                                                                                \
    do {                                                                                                               \
        if (p.stamps && threadIdx.x == 0) {                                                                            \
            const long wg_ = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;                     \
            p.stamps[wg_ * 16 + 9] = acc_w_; p.stamps[wg_ * 16 + 10] = acc_b1_; p.stamps[wg_ * 16 + 11] = acc_b2_;    \
            p.stamps[wg_ * 16 + 12] = acc_r_; p.stamps[wg_ * 16 + 13] = acc_m_;                                       \
        }                                                                                                              \
    } while (0)
#else
#define PBE_STAMP(i) do { } while (0)
#define PBE_ACC_DECL do { } while (0)
#define PBE_ACC_T0() do { } while (0)
#define PBE_ACC(v) do { } while (0)
#define PBE_ACC_STORE() do { } while (0)
#endif

// Priority of the MFMA block.  PBE_PRIO_MODE: 0 = s_setprio 1 around every MFMA block, 1 = none (shipped: same-device A/B over the
// whole pipeline, conv class 193.2 -> 191.9 ms, GEMM class unchanged), 2 = static: waves 4-7 of an 8-wave tile at priority 1 for
// the whole main loop (MI355X_MICROARCH.md, Two waves per SIMD, item 4: 192.1 ms)
#ifndef PBE_PRIO_MODE
#define PBE_PRIO_MODE 1
#endif
#if PBE_PRIO_MODE == 0
#define PBE_SETPRIO(x) __builtin_amdgcn_s_setprio(x)
#else
#define PBE_SETPRIO(x) do { } while (0)
#endif

// Diagnostic build (-DPBE_RACE_MUTANT=1 | 2 | 3, never the shipped library): the positive control of the race screens (tests/racescreen.py,
// DESIGN.md "Race screens").  Each value relaxes the counted vmcnt wait in front of ONE structure's LDS fragment reads by one tile's
// pieces, i.e. the waves read a ring slot whose DMA may still be in flight: 1 = the ring loop (MODE 0 / 1), 2 = the halo loops (MODE 2,
// both forms), 3 = the A-stationary loop (igemm_astat.hip: every wait but the run's last; its screens compare with tile 9's bits, not with
// integers).  1 and 2 never before the slice's tenth k-tile (PBE_RACE_MUTANT_KT): the slot's previous occupant is then a k-tile of the
// same slice, which the screens' diagnosis can name.  A loop that keeps ONE tile in flight beyond the one it
// waits for is relaxed at that k-tile only (every relaxed wait shows: the tile was issued one period ago); a ring that keeps two or more
// hides a single early wait (the tile was issued two periods ago and the earlier waits kept the queue short), so there every wait from
// that k-tile on is relaxed and the waves run ahead of the DMA.  Only the immediate of an s_waitcnt changes: no global address, store or
// barrier depends on it, so the worst outcome is a wrong number.  The mutant is a constant term of each wait (ring_wait's BUMP): 0 compiles the shipped code.
#ifndef PBE_RACE_MUTANT
#define PBE_RACE_MUTANT 0
#endif
#define PBE_RACE_MUTANT_KT 9

#define EX_LN 1
#define EX_ST 2
#define EX_VT 4
#define EX_MX 8        // MX-fp8 copy-out (IGemmP.mx_*): a compile-time form of copy_out, never a run-time branch of the fp16 kernels
#define EX_GN 16       // GroupNorm applied to the A fragments (IGemmP.gn_*): a compile-time form of the main loop, its table behind the LDS image
#define PBE_GN_MAX_K 1280
#define PBE_GLDS16(gsrc, ldst)                                                                     \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc),         \
                                     (__attribute__((address_space(3))) void*)(ldst), 16, 0, 0)

// Divisions of the prologue by launch-invariant divisors: the host passes a reciprocal (igemm_prologue), the kernel multiplies.
// n / d for ANY 32-bit n and 1 <= d < 2^31, mg = floor(2^32 / d) (2^32 - 1 for d = 1): n mg / 2^32 lies in (n / d - 1, n / d], so the
// estimate is the quotient or one less and one fix-up makes it exact (5 scalar instructions against ~40 of the generic division)
__host__ __device__ __forceinline__ unsigned udiv_mg(unsigned n, unsigned d, unsigned mg) {
    unsigned q = (unsigned)(((unsigned long long)n * mg) >> 32);
    q += (n - q * d >= d) ? 1u : 0u;
    return q;
}
static inline unsigned mg_of(unsigned d) { return d <= 1 ? 0xffffffffu : (unsigned)((1ull << 32) / d); }
// a / d for 0 <= a < 1024 and 1 <= d <= 512 (halo rows and their divisors: HPA <= 512), mh = ceil(2^20 / d).  With e = mh d - 2^20, 0 <= e < d:
// a mh / 2^20 = a / d + a e / (d 2^20), and the excess a e / (d 2^20) < a / 2^20 < 2^-10 < 1 / d.  a / d lies at least 1 / d below the next
// integer, so the floor is the quotient - exact without a fix-up, one 24-bit multiply and a shift
// (the float-reciprocal form this replaces took 9 instructions, ~50 times per lane of a halo tile)
__host__ __device__ __forceinline__ int udiv_h(int a, unsigned mh) {
#ifdef __HIP_DEVICE_COMPILE__
    return (int)(__umul24((unsigned)a, mh) >> 20);
#else
    return (int)(((unsigned)a * mh) >> 20);
#endif
}
static inline unsigned mh_of(unsigned d) { return (unsigned)(((1u << 20) + d - 1) / d); }

template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// The counted wait of a ring that keeps up to D - 1 later tiles in flight: `rem` of them (UNIT vmcnt entries each) and EXTRA younger entries
// may stay behind the tile the waves read next.  BUMP = 1 is the race mutant's wait (PBE_RACE_MUTANT above): one more tile, the awaited one itself.
template <int UNIT, int EXTRA, int D, int BUMP = 0> __device__ __forceinline__ void ring_wait(int rem) {
    if constexpr (D >= 3) { if (rem >= 2) { wait_vmcnt<(2 + BUMP) * UNIT + EXTRA>(); return; } }
    if constexpr (D >= 2) { if (rem >= 1) { wait_vmcnt<(1 + BUMP) * UNIT + EXTRA>(); return; } }
    wait_vmcnt<BUMP * UNIT + EXTRA>();
}
