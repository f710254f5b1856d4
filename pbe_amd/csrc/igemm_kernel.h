// Implicit-GEMM on the gfx950 matrix cores: one kernel body, three activation loaders.
//
//   MODE 0 (dense)   C[m,n] = sum_k A[m,k] W[n,k]          Linear / 1x1 conv / bmm
//   MODE 1 (conv3x3) m = (b,oy,ox), k = (ci/cb, tap, ci%cb) NHWC 3x3 conv gather, zero padding, cb % 64 == 0,
//                                                          optional fused nearest-2x upsample and
//                                                          two-source channel concat
//   MODE 2 (conv3x3) the same K order with the activation HALO resident in LDS (stride 1, pad 1, image width 8 .. 128):
//                    only the weight tile streams per k-tile; the two large tiles run a ping-pong main loop (see there)
//
// Structure (CDNA4, wave64):
//   * workgroup = NWM x NWN waves, block tile BM x BN x 64, each wave owns (BM/NWM) x (BN/NWN) as
//     16x16 tiles of v_mfma_f32_16x16x32_f16 (two k-steps per k-tile).  The weights are the MFMA "A" operand and the
//     activations the "B" operand, so an accumulator register quad holds 4 consecutive n for one m.
//   * tiles stream global -> LDS with global_load_lds_dwordx4 (LDS-DMA, no staging registers) into an S-slot ring
//     (S = 2 .. 4 by tile: S - 1 k-tiles in flight across ONE raw s_barrier per k-tile, retired with counted s_waitcnt vmcnt).
//     A k-tile row is 64 halfs = 128 B = one whole cache line: a DMA instruction fetches 8 complete lines.  (Round 1 staged
//     32 halfs per row; the half-line pieces capped the per-CU fill at 37 GB/s and the MFMA pipe sat idle for 55 % of the
//     main loop - tools/phase_stamps.py, profiles/r02_phase_stamps_bk32.txt.)
//   * LDS image: rows of 128 B = 8 chunks of 16 B.  An LDS-DMA instruction writes 64 lanes x 16 B linearly, so the bank
//     swizzle is applied to the per-lane SOURCE chunk (position p of row r holds global chunk p ^ (r & 7)) and again on
//     the fragment read: every ds_read_b128 of a 16x16x32 fragment is bank-conflict free in both k-steps.
//   * a DMA piece is LEAN (see the loader state): rows beyond M / N are clamped to the last row, the source is a pointer register
//     plus a scalar k offset, the LDS address an SGPR; padding pixels of the convs, a ragged last k-tile and a k-tile that
//     straddles the two concatenated sources read a 16-byte zero block through a per-lane select (LDS-DMA cannot mask a lane).
//   * workgroup ids are remapped so each XCD owns a contiguous run of tiles; the run walks n fastest or m fastest, whichever
//     fetches fewer bytes into the eight L2s for the launch's operand sizes (launch_cfg).
//   * small-M / deep-K problems are split along K over gridDim.z with a deterministic fp32 slab reduction.
//   * epilogue: alpha, bias, row-broadcast vector, activation in fp32 registers -> fp16 C tile in
//     LDS (one wave-row group at a time) -> whole 16-byte row segments to HBM, residual fused.
//   * what bounds the big conv tiles on real data is the power limit: cycles removed from the schedule come back
//     as a lower clock.
#pragma once
#include "igemm_params.h"
#include "igemm_mx8_out.h"
static __device__ __attribute__((aligned(16))) unsigned int g_pbe_zero16[4] = {0u, 0u, 0u, 0u};   // (one copy per translation unit)

typedef long i64;
// one 16-byte fragment = two 8-byte fp8 operands: both MFMAs take the SAME byte positions from the two matrices, so together
// they contract the 64 k-values of a (4 lane-quads x 16 bytes) k-step whatever order the hardware assigns inside an operand
__device__ __forceinline__ f32x4 mfma_pair_f8(const h16x8& w, const h16x8& a, f32x4 acc) {
    typedef i64 i64x2 __attribute__((ext_vector_type(2)));
    const i64x2 wv = __builtin_bit_cast(i64x2, w), av = __builtin_bit_cast(i64x2, a);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wv[0], av[0], acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wv[1], av[1], acc, 0, 0, 0);
}

// The dynamic LDS of one igemm_kernel instantiation, stated ONCE: the kernel takes its byte offsets from here, launch_cfg (igemm_plan.h) the
// byte count, the svec row count and GS_OK.  [ring: S stages of A | W k-tiles (MODE 2: two halo images, then the weight ring); the epilogue's
// fp16 C tile reuses it] [tab: 9 taps x BM pixel indices, MODE 1] [svec: bias + row vector, SVEC_ROWS samples x BN floats] [sca | scw | lnc -
// F8: scales of A's rows, of W's rows; EX: rstd and -mean rstd per row, colsum per column]
template <int BM, int BN, int NWM, int NWN, int MODE, int S, int HPA, bool F8, int EX> struct TileGeom {
    static constexpr int NT = NWM * NWN * 64, WM = BM / NWM, CLD = BN + 8, KIB160 = 160 * 1024;
    static constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128, STAGE = A_BYTES + W_BYTES;
    static constexpr int HALO_BYTES = HPA * 128, WRING_OFF = 2 * HALO_BYTES;             // MODE 2: one halo image; the weight ring behind two
    static constexpr int RING = MODE == 2 ? WRING_OFF + S * W_BYTES : S * STAGE;
    static constexpr int C_PASS = WM * CLD * 2, MAIN = RING > C_PASS ? RING : C_PASS;    // the C tile of one wave-row group
    static constexpr int TAB_OFF = RING, TAB_BYTES = MODE == 1 ? 9 * BM * 4 : 0, SVEC_OFF = MAIN + TAB_BYTES;
    static constexpr int SVEC_ROWS = MAIN + 4 * BN * 4 <= KIB160 ? 4 : 3;                // samples per tile the staged vectors can serve (sv_ok)
    static constexpr bool SCALES = F8 || (EX & 7) != 0;
    static constexpr int SCA_OFF = SVEC_OFF + 4 * BN * 4, SCW_OFF = SCA_OFF + BM * 4, LNC_OFF = SCW_OFF + BM * 4;
    static constexpr int SCALE_BYTES = F8 ? (BM + BN) * 4 : (EX & 7) != 0 ? (2 * BM + BN) * 4 : 0;
    static constexpr int LDS_BYTES = MAIN + TAB_BYTES + (SCALES ? 4 : SVEC_ROWS) * BN * 4 + SCALE_BYTES;
    // whole C tile at once when it fits the ring's LDS, else one wave-row group per pass; GroupNorm statistics from the copy-out: scratch behind the C tile
    static constexpr bool ONE_PASS = (size_t)BM * CLD * 2 <= (size_t)S * STAGE;
    static constexpr int GS_OFF = (BM * CLD * 2 + 15) & ~15;
    static constexpr bool GS_OK = MODE != 0 && ONE_PASS && !F8 && (NT / (BN / 8)) >= 1 && (size_t)GS_OFF + ((size_t)(NT / (BN / 8)) * BN + BN) * 8 <= (size_t)RING;
    static_assert((!SCALES || SVEC_ROWS == 4) && (ONE_PASS ? BM * CLD * 2 : C_PASS) <= MAIN, "sca sits four svec rows behind svec; the C tile of a pass ends before svec");
    static_assert((F8 ? SCW_OFF + BN * 4 : (EX & 7) != 0 ? LNC_OFF + BN * 4 : SVEC_OFF + SVEC_ROWS * BN * 4) == LDS_BYTES, "the last region ends at LDS_BYTES");
    // EX_GN: the sample's sc | sh table, 8 K bytes for THIS launch's K, lies behind everything else (launch_cfg adds it to the dynamic LDS)
    static constexpr int GN_OFF = LDS_BYTES, GN_MAX_BYTES = (EX & EX_GN) ? 8 * PBE_GN_MAX_K : 0;
    static_assert(LDS_BYTES + GN_MAX_BYTES <= KIB160, "tile does not fit the 160 KiB LDS");
};

// ---- the tile table: every (BM, BN, NWM, NWN, S, HPA) the kernel is instantiated for; the planner and the dispatch (igemm_plan.h) walk it ----
// Forms a tile is instantiated for (TileCfg.forms): the dispatch of each form launches exactly these rows, the planner picks among them.
enum : unsigned {
    F_DENSE = 1u << 0,      // MODE 0 (igemm_dense.hip)
    F_CONV = 1u << 1,       // MODE 1 gather (igemm_conv.hip)
    F_HALO = 1u << 2,       // MODE 2 halo-resident conv (igemm_halo.hip); hpa = rows of its halo image
    F_EX = 1u << 3,         // extended epilogue (igemm_ex_{ln,st,qkv,all}.hip)
    F_F8 = 1u << 4,         // fp8 operands (igemm_f8.hip)
    F_ASTAT = 1u << 5,      // A-stationary (igemm_astat.hip), where pbe_astat_ok() holds
    F_FORCED = 1u << 6,     // only through desc.tile_cfg / the tuned table, never by the heuristic
};
// s = ring depth in k-tiles of 64 (the weight ring of the halo / A-stationary tiles): the deepest that fits the LDS share of the tile's
// workgroups per CU.  eff = relative per-FLOP efficiency of the tile when the chip is full (ordered by staged bytes per FLOP); eff_shallow
// the same for shallow-K problems (< 10 k-tiles), dominated by the prologue / epilogue.  Both efficiency columns are fitted to the 472
// measured shapes of profiles/r01_autotune_report.txt (the heuristic then costs 4 % over the best tile per shape, 12 % before the fit);
// pbe_amd/tuned_mi355x.json overrides them per shape (desc.tile_cfg), so they only decide shapes outside the table.
// f8 = the tile an fp8-operand problem runs when the planner picks this one (the fp8 form instantiates a subset of the dense tiles).
struct TileCfg { int bm, bn, nwm, nwn, s, slots_per_cu; double eff, eff_shallow; int hpa; unsigned forms; int f8; };
static constexpr TileCfg kTiles[] = {
    {256, 256, 2, 4, 2, 1, 1.00, 0.82, 0, F_DENSE | F_CONV, 3},                     // 0: 128 KiB
    {256, 128, 4, 2, 3, 1, 0.82, 0.72, 0, F_DENSE | F_CONV, 3},                     // 1: 144 KiB
    {128, 256, 2, 4, 3, 1, 0.75, 0.66, 0, F_DENSE | F_CONV, 3},                     // 2: 144 KiB
    {128, 128, 2, 2, 2, 2, 0.88, 1.00, 0, F_DENSE | F_CONV | F_EX | F_F8, 3},       // 3:  64 KiB, 4 waves: two workgroups per CU
    {128, 64, 2, 2, 2, 3, 0.65, 0.84, 0, F_DENSE | F_CONV | F_EX | F_F8, 4},        // 4:  48 KiB
    {64, 128, 2, 2, 2, 3, 0.65, 0.85, 0, F_DENSE | F_CONV | F_EX, 6},               // 5:  48 KiB
    {64, 64, 2, 2, 2, 4, 0.60, 0.80, 0, F_DENSE | F_CONV | F_EX | F_F8, 6},         // 6:  32 KiB
    {256, 320, 2, 4, 2, 1, 1.05, 0.80, 0, F_DENSE | F_CONV, 8},                     // 7: 144 KiB: N = 320 / 640 / 960 / 1280 without column padding (142 FLOP per staged byte)
    {128, 320, 2, 4, 2, 1, 0.96, 0.95, 0, F_DENSE | F_CONV | F_EX | F_F8, 8},       // 8: 112 KiB: same, half the rows: fills the chip when M / 256 < 256 tiles
    {128, 160, 2, 2, 2, 2, 0.90, 0.97, 0, F_DENSE | F_CONV | F_EX | F_F8, 9},       // 9:  72 KiB, 4 waves: two workgroups per CU overlap each other's prologue / epilogue
    // halo-resident 3x3 conv tiles (stride 1, pad 1, image width 8 .. 128 = tile width, and the tile's bm pixels are whole rows of one
    // image or a whole number of images - halo_rows(); any other map runs the gather tiles): only the weights stream per k-tile
    {256, 160, 4, 2, 3, 1, 1.40, 1.40, 392, F_HALO, 9},                   // 10: 160 KiB: 256 pixels (4 rows at 64x64) x 160 channels, 8 waves, ping-pong
    {128, 160, 4, 2, 3, 1, 1.20, 1.20, 264, F_HALO, 9},                   // 11: 128 KiB: 128 pixels x 160 channels
    {128, 320, 2, 4, 2, 1, 1.25, 1.25, 264, F_HALO, 9},                   // 12: 149 KiB: 128 pixels x 320 channels
    {256, 128, 4, 2, 3, 1, 1.30, 1.30, 392, F_HALO, 9},                   // 13: 148 KiB: channel counts that are multiples of 128 only, ping-pong
    {128, 128, 4, 2, 3, 1, 1.10, 1.10, 392, F_HALO, 9},                   // 14: 148 KiB: one 128-pixel row of a 128-wide image (VAE)
    // deep-ring forms of the small dense tiles, ONE workgroup per CU: for grids of <= 256 workgroups (M <= 2 048 rows) the second
    // workgroup of a CU never arrives, and S = 2 then leaves one k-tile in flight per CU - a k-tile per DMA round trip
    {128, 128, 2, 2, 4, 1, 0.50, 0.50, 0, F_DENSE | F_CONV | F_EX, 3},              // 15: 128 KiB
    {128, 64, 2, 2, 4, 1, 0.40, 0.40, 0, F_DENSE | F_CONV | F_EX, 4},               // 16:  96 KiB
    {64, 64, 2, 2, 4, 2, 0.38, 0.38, 0, F_DENSE | F_CONV | F_EX, 6},                // 17:  64 KiB
    {128, 160, 2, 2, 4, 1, 0.52, 0.52, 0, F_DENSE | F_CONV | F_EX, 9},              // 18: 144 KiB
    // A-stationary persistent tiles (igemm_astat.hip): K = 320 GEGLU projection with the LayerNorm fold, A block in registers, 4 waves,
    // two workgroups per CU; only through desc.tile_cfg / the tuned table where pbe_astat_ok() holds
    {128, 128, 4, 1, 3, 2, 0.0, 0.0, 0, F_ASTAT | F_FORCED, 9},           // 19: weight ring 48 KiB
    {128, 160, 4, 1, 3, 2, 0.0, 0.0, 0, F_ASTAT | F_FORCED, 9},           // 20: weight ring 60 KiB (256 registers, 14 spilled)
    // dense 8-wave tile with 160 columns: 6.5 LDS-DMA pieces per wave and k-tile against 40 MFMAs (the 4-wave 128x160 tile: 9)
    {256, 160, 4, 2, 3, 1, 0.0, 0.0, 0, F_DENSE | F_FORCED, 9}};          // 21: 156 KiB
static constexpr int kNCfg = sizeof(kTiles) / sizeof(kTiles[0]);
static constexpr bool f8_column_ok() {      // every row maps to a tile the fp8 form instantiates
    for (const TileCfg& t : kTiles)
        if (!(kTiles[t.f8].forms & F_F8)) return false;
    return true;
}
static_assert(f8_column_ok(), "kTiles: an f8 column names a tile without F_F8");

// (the 4-wave tiles live two workgroups per CU - two waves per SIMD, 256 registers each.  The V^T form of the 128x160 tile would take 268
//  and halve the occupancy: its bound is declared; the LayerNorm-only (252) and statistics-only (228) forms fit unconstrained and
//  keep their natural allocation - capped to 192 registers the GEGLU projection ran 11 % slower)
template <int BM, int BN, int NWM, int NWN, int MODE, int S, int HPA = 0, bool PP = false, bool F8 = false, int EX = 0>
#ifndef PBE_EX_MINWAVES
#define PBE_EX_MINWAVES 2
#endif
__global__ void __launch_bounds__(NWM* NWN * 64, ((EX & 4) != 0 && NWM * NWN == 4 && S == 2) ? PBE_EX_MINWAVES : 1) igemm_kernel(const IGemmP p) {
    // EX (MODE 0, fp16 operands, one-pass epilogue tiles): the extended epilogue, a bit mask of what THIS instantiation carries -
    // EX_LN LayerNorm folded in, EX_ST row statistics out, EX_VT column-range alpha + transposed V^T tiles (see IGemmP).  Separate
    // instantiations per combination in use (GEGLU: EX_LN; proj_in / to_out: EX_ST; q|k|v^T: EX_LN | EX_VT): a kernel's registers are
    // the maximum over its paths, and the all-in-one form ran the GEGLU projection 11 % slower than the plain tile (tools/gemm_ex_ab.py).
    constexpr bool EXL = (EX & 1) != 0, EXS = (EX & 2) != 0, EXV = (EX & 4) != 0, EXM = (EX & EX_MX) != 0;
    constexpr int EXF = EX & 7;                       // the fp16 extended-epilogue features (EX_MX only changes the copy-out)
    constexpr bool EXG = (EX & EX_GN) != 0;           // GroupNorm folded into the A fragments (MODE 0, K % 64 == 0, one sample per tile: the host checks)
    // F8 (MODE 0 only): A and W hold OCP e4m3 bytes, a k-tile row of 128 B is 128 k-values; v_mfma_f32_16x16x32_fp8_fp8 runs at
    // the fp16 MFMA's rate, the gain is half the bytes through the fill path that bounds these GEMMs.  The epilogue multiplies
    // by the per-row scale of A and the per-row scale of W (per output column) before bias / activation / residual.
    // MODE 2 = 3x3 conv (stride 1, pad 1) with the activation HALO resident in LDS: a tile is BM pixels = whole image rows (or whole
    // images); for every 64-channel block its (rows + 2) x (width + 2) halo (HPA rows of 128 B, zero outside the image) is staged
    // ONCE and all 9 taps read their shifted windows from it, so only the weight tile streams per k-tile.  MODE 1 re-stages the
    // activation tile for every tap: with two 128x160 workgroups per CU that is 74 KB of LDS-DMA per 1 280 MFMA pipe cycles -
    // more than a CU's fill path delivers (phase stamps: 3 190 cycles per k-tile inside the sampler).  Here a 256x160 tile moves
    // 20.5 KB + 5.7 KB for the same MFMA work.  S = weight ring depth.
    // S = LDS ring depth (S - 1 k-tiles of 64 in flight).  Sized per tile so the ring fills the LDS one workgroup (8-wave tiles)
    // or two to three workgroups (4-wave tiles) can own on a CU.
    // (A "ping-pong" form of the main loop for the 8-wave tiles - wave groups 0-3 / 4-7 offset by one barrier, [fragment reads +
    //  DMA issue | MFMAs] with two barriers per k-tile - was built and measured on every conv / GEMM shape of the path: bit-identical
    //  output, 7 % slower on the conv class (780.9 -> 724.0 TFLOP/s), 2 % slower on the GEMM class.  profiles/r02_ab_pingpong_rejected.txt.)
    using G = TileGeom<BM, BN, NWM, NWN, MODE, S, HPA, F8, EX>;      // the LDS layout
    constexpr int NW = NWM * NWN, NT = NW * 64;
    constexpr int D = S - 1;
    constexpr int WM = BM / NWM, WN = BN / NWN, TM = WM / 16, TN = WN / 16;
    constexpr int A_BYTES = G::A_BYTES, W_BYTES = G::W_BYTES, STAGE = G::STAGE, CLD = G::CLD;
    constexpr int PA = BM / 8, PW = BN / 8;           // 8-row x 128-byte DMA pieces (1 KiB = one wave instruction)
    constexpr int LA = PA / NW, LW = (PW + NW - 1) / NW, LPT = LA + LW;
    static_assert(S >= 2 && S <= 4 && PA % NW == 0 && BM % 16 == 0 && BN % 16 == 0, "A pieces must divide over the waves (weight pieces may be padded)");
    static_assert(MODE != 2 || (HPA % 8 == 0 && HPA >= BM), "halo image must hold the tile");
    static_assert(EXF == 0 || (MODE == 0 && !F8), "extended epilogue: dense fp16 tiles only");
    static_assert(!EXM || (MODE == 0 && !EXS && (F8 || EXF == (EX_LN | EX_VT))), "MX-fp8 copy-out: the fp8 tiles and the q|k|v^T form");
    static_assert(!EXG || (MODE == 0 && !F8 && !EXL), "GroupNorm fold: dense fp16 tiles whose A is not LayerNorm-folded too");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: every LDS-DMA destination below is an SGPR expression
    const int wm = wave % NWM, wn = wave / NWM;
    PBE_ACC_DECL;
#if PBE_PRIO_MODE == 2
    if (NW == 8 && __builtin_amdgcn_readfirstlane(wave) >= 4) __builtin_amdgcn_s_setprio(1);
#endif
    PBE_STAMP(0);                                    // workgroup start
    PBE_STAMP(7);                                    // wall clock (100 MHz) of the start
    int tile;
    {   // XCD-aware tile order (bijective for any grid size)
        const int nwg = gridDim.x, id = blockIdx.x, q = nwg >> 3, r = nwg & 7, xcd = id & 7;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
    }
    // Each XCD's L2 fetches what ITS tiles touch.  n fastest: an XCD's run covers few row blocks of A and every column block of
    // W - right where A is the big operand (64x64 maps).  m fastest: few column blocks of W and every row block of A - right where
    // W is (16x16 / 8x8 maps: 29 MB of weights against 5 MB of activations; n fastest made all 8 L2s fetch all 29).
    // (tile / tiles_m | tile / tiles_n: one divisor per launch, its reciprocal from the host)
    const int tq = (int)udiv_mg((unsigned)tile, (unsigned)p.tdiv, p.mg_tdiv), tr = tile - tq * p.tdiv;
    const int tn_i = p.m_fast ? tq : tr, tm_i = p.m_fast ? tr : tq;
    const int m0 = tm_i * BM, n0 = tn_i * BN;
    const long bz = blockIdx.y;
#ifdef PBE_STAMPS
    if (m0 >= 0) PBE_STAMP(14);                      // first kernarg-dependent value (tile origin) ready
#endif

    // ---- loader state: this lane's row inside an 8-row DMA piece and its source chunk ----
    // LDS rows are 128 B (64 halfs = 8 chunks of 16 B) = one whole cache line per row: a wave's DMA instruction fetches 8
    // complete lines (64-byte row pieces - the BK = 32 layout of round 1 - filled at 37 GB/s per CU in the real kernel,
    // tools/phase_stamps.py: 1 440 cycles per k-tile of a 128x320 tile against 640 cycles of MFMA work).
    // LDS-DMA writes lane l at base + 16 l, so the bank swizzle goes on the SOURCE chunk: position p of row r holds global
    // chunk p ^ (r & 7); the fragment read applies the same XOR (conflict-free ds_read_b128 for both k-steps, checked by
    // enumeration over the hardware's 16-lane service groups).
    const int lrow = lane >> 3;
    const int gch = (lane & 7) ^ lrow;
    const h16* zsrc = reinterpret_cast<const h16*>(g_pbe_zero16);

    // A DMA piece must stay LEAN: tools/ubench_loop.hip (this loop's instruction mix, operands from L2) runs a k-tile of the
    // 256x160 tile in 1 550-1 630 cycles with "pointer + scalar k offset" pieces and in 1 850-2 500 with the form this kernel used to
    // compile to (per-lane zero-block select, LDS address through a VGPR, a branch per piece): next to MFMAs every VALU instruction
    // of a piece waits for an issue slot.  So: rows beyond M / N are CLAMPED to the last row (their products land in accumulators
    // that are never stored), the source pointer of a piece is one 64-bit add, its LDS address an SGPR; only a k-tile that needs
    // per-lane zeros (K % 64 != 0: the last one) or straddles the two concatenated sources takes the select form.
    const h16* a_cur[LA];                             // source row of each piece at k = 0, + this lane's chunk (current concat source)
    const h16* a_alt[LA];                             // the same for the second source, pre-offset by -K1
#pragma unroll
    for (int i = 0; i < LA; ++i) {
        const int m = min(m0 + (wave * LA + i) * 8 + lrow, p.M - 1);
        a_cur[i] = p.A + bz * p.sA + (long)m * p.lda + gch * 8;
        a_alt[i] = p.A2 ? p.A2 + (long)m * p.lda2 + gch * 8 - p.K1 : a_cur[i];
    }
    // conv: K is ordered (channel block cb, tap, channel) so the 9 taps of a pixel's cb channels are consecutive k-tiles -
    // the shifted re-reads hit L2 instead of going back to the Infinity Cache / HBM (measured: tap-major order re-fetched the
    // input 9x beyond L2).  The tap -> input-pixel map of this tile's BM rows is built once into LDS:
    // tab[tap][row] = pixel index, or -1 outside the (virtual) image.
    int* tab = reinterpret_cast<int*>(smem + G::TAB_OFF);
    // Epilogue vectors of this tile, staged ONCE (their global latency hides under the first DMA tile):
    // svec[s][c] = bias[n0 + c] + rowvec[first sample of the tile + s][n0 + c], up to 4 samples per tile.
    float* svec = reinterpret_cast<float*>(smem + G::SVEC_OFF);
    const int sv_ns = p.sv_ns;                       // samples per tile (tile is sample-aligned when sv_ok)
    if (MODE == 1) {
        const int hw = p.hw, Hv = p.H << p.ups, Wv = p.Wd << p.ups;
        // Phase form (p.phase): a 3x3 conv over a nearest-2x upsampled image reads, for the output pixel (2y + py, 2x + px), only a 2x2
        // block of SOURCE pixels - rows {y - 1 + py, y + py}, columns {x - 1 + px, x + px} - because the 9 taps fall on 4 distinct
        // sources (py = 0: taps ky = 0 | 1, 2 -> rows y - 1 | y; py = 1: ky = 0, 1 | 2 -> y | y + 1).  The host sums the weights that
        // share a source (4 weight sets of 4 taps): 4 / 9 of the MACs, rows = source pixels, blockIdx.y = phase, and the epilogue
        // scatters row m = (b, y, x) to output pixel (2y + py, 2x + px).  Zero padding agrees: source row -1 <=> upsampled row -1 / -2.
        const int py = p.phase ? (int)(blockIdx.y >> 1) : 0, px = p.phase ? (int)(blockIdx.y & 1) : 0;
        for (int row = tid; row < BM; row += NT) {            // one thread per tile row: one (b, oy, ox) decode, 9 (or 4) taps
            const int m = m0 + row;
            const bool rok = m < p.M;
            const int b = (int)udiv_mg((unsigned)m, (unsigned)hw, p.mg_hw), rem = m - b * hw;
            const int oy = (int)udiv_mg((unsigned)rem, (unsigned)p.Wo, p.mg_wo), ox = rem - oy * p.Wo;
            const int iy0 = oy * p.cstride - p.pad, ix0 = ox * p.cstride - p.pad;
            if (p.phase) {
#pragma unroll
                for (int tp = 0; tp < 4; ++tp) {
                    const int iy = oy - 1 + py + (tp >> 1), ix = ox - 1 + px + (tp & 1);
                    const bool ok = rok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.Wd;
                    tab[tp * BM + row] = ok ? (b * p.H + iy) * p.Wd + ix : -1;
                }
                continue;
            }
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) {
                const int iy = iy0 + tp / 3, ix = ix0 + tp % 3;
                const bool ok = rok && (unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv;
                tab[tp * BM + row] = ok ? (b * p.H + (iy >> p.ups)) * p.Wd + (ix >> p.ups) : -1;
            }
        }
        __syncthreads();
    }
    const h16* w_row[LW];
#pragma unroll
    for (int i = 0; i < LW; ++i) {
        // (a padding piece - PW not a multiple of NW, halo tiles only - repeats the last real piece: same source, same LDS bytes)
        const int n = min(n0 + min(wave + NW * i, PW - 1) * 8 + lrow, p.N - 1);
        w_row[i] = p.W + bz * p.sW + (long)n * p.ldw + gch * 8;
    }
    const int nk_all = (p.K + 63) >> 6;
    int kt0 = 0, nk = nk_all;                        // this workgroup's k-tile range [kt0, nk)
    if (p.splits > 1) {
        kt0 = blockIdx.z * p.split_per;
        nk = min(nk_all, kt0 + p.split_per);
    }
    // conv K order: (channel block of cb, tap, channel): state of the NEXT k-tile to issue
    const int KB = MODE == 1 ? p.cb >> 6 : 1;        // k-tiles per (block, tap) visit
    const int ntap = (MODE == 1 && p.phase) ? 4 : 9;
    int tap = 0, c0 = 0, kj = 0;
    if (MODE == 1 && kt0 > 0) {
        const int cblk = (int)udiv_mg((unsigned)kt0, (unsigned)p.per_blk, p.mg_per_blk), r = kt0 - cblk * p.per_blk;
        tap = (int)udiv_mg((unsigned)r, (unsigned)KB, p.mg_kb); kj = r - tap * KB; c0 = cblk * p.cb + kj * 64;
    }
    // MODE 1: per piece the running source pointer and its advance per k-tile (a padding pixel keeps reading the zero block: advance 0)
    const h16* a_src[LA];
    int a_inc[LA];
    bool fresh = true;
#pragma unroll
    for (int i = 0; i < LA; ++i) { a_src[i] = zsrc; a_inc[i] = 0; }
    // MODE 0: the k-tile where the second concat source takes over, and the two rare k-tiles that need per-lane selects
    const bool ktail = (p.K & 63) != 0, straddle = p.A2 && (p.K1 & 63);
    const int kt_sw = p.A2 ? p.K1 >> 6 : 0x7fffffff;
    if (MODE == 0 && kt0 > kt_sw) {
#pragma unroll
        for (int i = 0; i < LA; ++i) a_cur[i] = a_alt[i];
    }

    auto issue = [&](int kt, int slot) {              // k-tiles are issued in order: kt0, kt0 + 1, ...
        unsigned char* sa = smem + slot * STAGE;
        unsigned char* sw = sa + A_BYTES;
        const long k = (long)kt * 64;                 // scalar
        const bool slow = (ktail && kt == nk_all - 1) || (straddle && kt == kt_sw);      // uniform
        const int kl = kt * 64 + gch * 8;             // this lane's k (slow form only)
        if (MODE == 0) {
            if (kt == kt_sw && !straddle) {
#pragma unroll
                for (int i = 0; i < LA; ++i) a_cur[i] = a_alt[i];
            }
            if (!slow) {
#pragma unroll
                for (int i = 0; i < LA; ++i) PBE_GLDS16(a_cur[i] + k, sa + (wave * LA + i) * 1024);
            } else {
#pragma unroll
                for (int i = 0; i < LA; ++i) {
                    const h16* src = (kl < p.K1 ? a_cur[i] : a_alt[i]) + k;
                    PBE_GLDS16(kl < p.K ? src : zsrc, sa + (wave * LA + i) * 1024);
                }
                if (straddle && kt == kt_sw) {
#pragma unroll
                    for (int i = 0; i < LA; ++i) a_cur[i] = a_alt[i];
                }
            }
        } else {
            if (kj == 0 || fresh) {                   // new (block, tap): look the pixels up; otherwise +64 channels
                fresh = false;
                const bool first = c0 < p.C1;         // which concat source this channel block lives in (uniform)
                const h16* base = first ? p.A + c0 + gch * 8 : p.A2 + (c0 - p.C1) + gch * 8;
                const long cs = first ? p.C1 : p.C2;
#pragma unroll
                for (int i = 0; i < LA; ++i) {
                    const int pix = tab[tap * BM + (wave * LA + i) * 8 + lrow];
                    a_src[i] = pix >= 0 ? base + (long)pix * cs : zsrc;
                    a_inc[i] = pix >= 0 ? 64 : 0;
                }
            }
#pragma unroll
            for (int i = 0; i < LA; ++i) {
                PBE_GLDS16(a_src[i], sa + (wave * LA + i) * 1024);
                a_src[i] += a_inc[i];
            }
            c0 += 64;
            if (++kj == KB) {
                kj = 0;
                if (++tap == ntap) tap = 0; else c0 -= p.cb;   // next tap of the same block, or first tap of the next block
            }
        }
        if (!slow) {
#pragma unroll
            for (int i = 0; i < LW; ++i) PBE_GLDS16(w_row[i] + k, sw + min(wave + NW * i, PW - 1) * 1024);      // (a padding piece repeats the last real one)
        } else {
#pragma unroll
            for (int i = 0; i < LW; ++i) PBE_GLDS16(kl < p.K ? w_row[i] + k : zsrc, sw + min(wave + NW * i, PW - 1) * 1024);
        }
    };

    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    const int rsw = (fq ^ (fr & 7)) << 4;             // byte offset of k-step 0's chunk; k-step 1 is rsw ^ 64
    const int a_rd = (wm * WM + fr) * 128, w_rd = (wn * WN + fr) * 128;

    float* sca = reinterpret_cast<float*>(smem + G::SCA_OFF);      // F8: per-row scale of A for this tile's rows, then per-column scale (W's rows)
    float* scw = reinterpret_cast<float*>(smem + G::SCW_OFF);      // EX + LayerNorm fold: sca[row] = rstd, scw[row] = -mean * rstd, lnc[col] = colsum of W * gamma
    float* lnc = reinterpret_cast<float*>(smem + G::LNC_OFF);
    auto stage_svec = [&]() {
        if constexpr (F8) {
            for (int idx = tid; idx < BM + BN; idx += NT) {
                float v = 1.f;
                if (idx < BM) { if (p.sa && m0 + idx < p.M) v = p.sa[bz * p.ssa + m0 + idx]; sca[idx] = v; }
                else { const int c = idx - BM; if (p.sw && n0 + c < p.N) v = p.sw[bz * p.ssw + n0 + c]; scw[c] = v; }
            }
        }
        if constexpr (EXL) {
            if (p.ln_stat) {
                for (int idx = tid; idx < BM + BN; idx += NT) {
                    if (idx < BM) {
                        const int m = min(m0 + idx, p.M - 1);
                        float a = 0.f, q = 0.f;
                        for (int z = 0; z < p.ln_parts; ++z) {           // fixed order: deterministic
                            const float2 t = *reinterpret_cast<const float2*>(p.ln_stat + 2 * ((long)z * p.ln_ld + m));
                            a += t.x; q += t.y;
                        }
                        // (only the cancelling subtraction runs in fp64 - three full-rate operations; an fp64 divide + square root per row cost
                        //  the workgroup ~1 500 cycles of a 8 000-cycle K = 320 tile)
                        const double mean = (double)a * p.ln_inv_k;
                        const float var = (float)((double)q * p.ln_inv_k - mean * mean);
                        const float rstd = __builtin_amdgcn_rsqf(fmaxf(var, 0.f) + p.ln_eps);
                        sca[idx] = rstd; scw[idx] = -(float)mean * rstd;
                    } else {
                        const int c = idx - BM;
                        lnc[c] = n0 + c < p.N ? p.ln_c1[n0 + c] : 0.f;
                    }
                }
            }
        }
        if (p.sv_ok && p.splits <= 1) {                  // staged AFTER the first DMAs are in flight: both latencies overlap
            // first sample of the tile: sv_ns whole samples per tile, or sv_gdiv row tiles per sample (tile and sample are aligned: sv_ok)
            const int s0 = !p.rowvec ? 0 : sv_ns > 1 ? tm_i * sv_ns : (int)udiv_mg((unsigned)tm_i, (unsigned)p.sv_gdiv, p.mg_sv_gdiv);
            for (int idx = tid; idx < sv_ns * BN; idx += NT) {
                const int si = idx / BN, c = idx - si * BN, n = n0 + c;
                float v = 0.f;
                if (n < p.N) {
                    if (p.bias && !p.bias_row) v = p.bias[n];
                    if (p.rowvec && (long)(s0 + si) * p.group_rows < p.M) v += (float)p.rowvec[(long)(s0 + si) * p.ldv + n];
                }
                svec[si * BN + c] = v;
            }
        }
    };
    // Tiles with few accumulators fetch BOTH k-steps' fragments before the first MFMA (the second set's LDS latency hides
    // under the first set's MFMAs); the 256-row tiles have no registers for that and read k-step 1 after issuing k-step 0.
    constexpr bool BOTH = TM * TN * 4 + 2 * (TM + TN) * 4 <= 176;

    if constexpr (MODE == 2) {
        constexpr int PAH = HPA / 8, LAH = (PAH + NW - 1) / NW;
        unsigned char* abuf = smem;
        unsigned char* wring = smem + G::WRING_OFF;
        // Halo image of one (sub-)image of the tile: TH + 2 rows of TW + 1 pixels + 1.  A tile spans the image's whole width, so
        // x = -1 and x = TW are always padding: the zero row right of image row y IS the zero row left of image row y + 1
        // (row stride TW + 1 instead of TW + 2; 4 rows of 64 pixels: 391 halo rows instead of 396 - what lets a third weight slot
        // fit beside two halo images of a 256-pixel tile).
        // The geometry is the launch's (igemm_prologue): HW2 = TW + 1, HPS = (TH + 2) HW2 + 1 halo rows per (sub-)image, nsub whole images
        // per tile (nsub > 1) or tiles_per_img row tiles per image; only the base pixel (b0, y0) and the border test belong to the workgroup.
        static_assert(HPA <= 512, "udiv_h: halo rows below 1024, divisors up to 512");
        const int TW = p.Wd, TH = p.th, HW2 = p.h_hw2, HPS = p.h_hps, nsub = p.h_nsub;
        const int b0 = nsub > 1 ? tm_i * nsub : (int)udiv_mg((unsigned)tm_i, (unsigned)p.h_tpi, p.mg_h_tpi);
        const int y0 = nsub > 1 ? 0 : (tm_i - b0 * p.h_tpi) * TH;
        auto halo_pix = [&](int hp) {                 // source pixel of halo row hp of this tile (-1: zero row)
            int pix = -1;
            if (hp < p.h_rows) {
                const int sub = udiv_h(hp, p.mh_hps), r = hp - sub * HPS, hy = udiv_h(r, p.mh_hw2), hx = r - hy * HW2;
                const int y = y0 + hy - 1, x = hx - 1;
                if ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)TW) pix = ((b0 + sub) * p.H + y) * TW + x;
            }
            return pix;
        };
        int hpix[LAH];                                // source pixel of this lane's row in each of its halo pieces (-1: zero)
#pragma unroll
        for (int i = 0; i < LAH; ++i) hpix[i] = halo_pix(min(wave + NW * i, PAH - 1) * 8 + lrow);      // (padding pieces repeat the last real one)
        int hc[TM];                                   // halo row of this lane's pixel in each of its 16-pixel groups (tap (1,1))
#pragma unroll
        for (int j = 0; j < TM; ++j) {                // (image width and pixels per (sub-)image are powers of two: shifts and masks)
            const int ml = wm * WM + j * 16 + fr, sub = ml >> p.h_lgimg, rr = ml - (sub << p.h_lgimg), ty = rr >> p.h_lgw, tx = rr - (ty << p.h_lgw);
            hc[j] = sub * HPS + (ty + 1) * HW2 + tx + 1;
        }
        // running source pointer of each halo piece (channel block by channel block, +64 channels; a padding row keeps reading the
        // zero block) - rebuilt only where the channel blocks cross from the first concat source into the second
        const h16* hptr[LAH];
        auto halo_base = [&](int blk) {
            const int c0b = blk * 64;
            const bool first = c0b < p.C1;
            const h16* base = (first ? p.A + c0b : p.A2 + (c0b - p.C1)) + gch * 8;
            const int cs = first ? p.C1 : p.C2;         // (int x int -> 64 bits: one multiply-add per piece)
#pragma unroll
            for (int i = 0; i < LAH; ++i) {
                hptr[i] = hpix[i] >= 0 ? base + (long)hpix[i] * cs : zsrc;
            }
        };
        auto issue_a1 = [&](int buf_off, int i) {         // piece i (compile-time) of the next block in line, into the halo buffer at buf_off
            PBE_GLDS16(hptr[i], abuf + buf_off + min(wave + NW * i, PAH - 1) * 1024);
            hptr[i] += hpix[i] >= 0 ? 64 : 0;
        };
        auto issue_a = [&](int blk, int buf) {
            if (p.C2 && blk * 64 == p.C1) halo_base(blk);
#pragma unroll
            for (int i = 0; i < LAH; ++i) issue_a1(buf * G::HALO_BYTES, i);
        };
        auto issue_w1 = [&](int kt, int slot, int i) {
            PBE_GLDS16(w_row[i] + (long)kt * 64, wring + slot * W_BYTES + min(wave + NW * i, PW - 1) * 1024);
        };
        auto issue_w = [&](int kt, int slot) {
#pragma unroll
            for (int i = 0; i < LW; ++i) issue_w1(kt, slot, i);
        };
        const int nblk_all = (p.C1 + p.C2) >> 6;
        int blk0 = 0, blk1 = nblk_all;                // this workgroup's channel blocks (split-K at block granularity)
        if (p.splits > 1) {
            blk0 = blockIdx.z * p.split_per;
            blk1 = min(nblk_all, blk0 + p.split_per);
        }
        const int nk2 = blk1 * 9;
        PBE_STAMP(1);
        if (blk0 < blk1) {
            halo_base(blk0);
            issue_a(blk0, 0);
#pragma unroll
            for (int t = 0; t < (PP ? 2 : D); ++t) issue_w(blk0 * 9 + t, t);
        }
        PBE_STAMP(2);
        stage_svec();
        if constexpr (PP) {
            // Ping-pong form (8 waves, two per SIMD; weight ring of 3).  Waves 0-3 and 4-7 alternate: in every half period one group
            // reads its 18 fragments of a k-tile while the other group's MFMAs own the matrix pipe.
            //   period P (tile P), barriers b(2P-1) | b(2P) | b(2P+1):
            //     first half:   group 0 reads tile P's fragments        | group 1 runs the MFMAs of tile P-1
            //     second half:  group 0 runs the MFMAs of tile P        | group 1 reads tile P's fragments
            //   The DMA pieces of period P - W(P + 2) and a share of the next block's halo - go out right behind the fragment reads of
            //   a wave's read half.  The first form of this loop (weight ring of 2, all 7 halo pieces at tap 0, pieces with per-lane
            //   selects at the HEAD of the read half) spent 1 150 cycles in the read half against 680 of MFMAs
            //   (tools/phase_stamps.py); spreading the pieces between the MFMAs was worse still (tools/ubench_loop.hip).
            //   RAW: tile P+1 (issued in period P-1, retired by its issuers at the end of period P) and a halo retired in the second
            //   half of period 9b+8 have landed at b(2P+1), before their first read.  WAR: W(P+2) lands in tile P-1's slot and block
            //   b+1's halo in block b-1's buffer; their last reads (group 1, second half of period P-1 / 9b-1) precede b(2P-1).
            static_assert(NW == 8 && BOTH && S == 3 && LAH <= 8, "ping-pong: two waves per SIMD, both k-steps' fragments in registers, weight ring of 3");
            const int grp = __builtin_amdgcn_readfirstlane(wave >> 2);
            h16x8 fa[2][TM], fw[2][TN];
            // The read half is the long pole (its partner group is computing: every VALU instruction here waits for an issue slot
            // next to the partner's MFMAs - 930 cycles with the fragment addresses computed in place against 680 of MFMAs), so it
            // holds NOTHING but the 18 ds_read_b128 and the DMA pieces: the LDS byte addresses of the next tile's fragments (tap
            // shift, swizzle, halo buffer, ring slot) and the bumped weight pointers are computed inside the wave's OWN MFMA block,
            // a few VALU instructions after every other MFMA, where the matrix pipe covers them.
            int aaddr[2][TM], waddr[2];
            auto tile_shift = [&](int tap) {
                const int trow = tap >= 6 ? 2 : (tap >= 3 ? 1 : 0);
                return (trow - 1) * HW2 + (tap - 3 * trow - 1);
            };
            auto frag_addrs = [&](int blk_n, int tap_n, int slot_n) {      // in one go (prologue only)
                const int shift = tile_shift(tap_n), abase = ((blk_n - blk0) & 1) * G::HALO_BYTES, wb = G::WRING_OFF + slot_n * W_BYTES;
#pragma unroll
                for (int j = 0; j < TM; ++j) {
                    const int ar = hc[j] + shift;
                    aaddr[0][j] = abase + ar * 128 + ((fq ^ (ar & 7)) << 4);
                    aaddr[1][j] = aaddr[0][j] ^ 64;
                }
                waddr[0] = wb + w_rd + rsw;
                waddr[1] = wb + w_rd + (rsw ^ 64);
            };
            auto read_frags = [&]() {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                    for (int j = 0; j < TM; ++j) fa[ks][j] = *reinterpret_cast<const h16x8*>(smem + aaddr[ks][j]);
#pragma unroll
                    for (int i = 0; i < TN; ++i) fw[ks][i] = *reinterpret_cast<const h16x8*>(smem + waddr[ks] + i * 16 * 128);
                }
            };
            const int kt_first = blk0 * 9;
            // The two streams go out through DIFFERENT waves: vmcnt retires in order, so a halo piece (activations no other workgroup
            // shares: full HBM / Infinity Cache latency, ~2 500 cycles under load) ahead of a weight piece (L2, ~600) in ONE wave's
            // queue makes the weight tile as late as the halo - with both in every wave the end-of-period wait stalled for ~500
            // cycles per period.  Group 0 (waves 0-3) issues the weight tiles and retires them every period; group 1 (waves 4-7)
            // issues the next block's halo, two pieces per period from tap 0 on, and retires it once, at tap 8.
            constexpr int PWG = PW / 4, LAHG = (PAH + 3) / 4;
            static_assert(PW % 4 == 0 && LAHG <= 14, "weight pieces split over 4 waves; at most two halo pieces per period over taps 0 .. 6");
            const int gw = wave & 3;
            const h16* wp[PWG];                            // group 0: weight pointers of the NEXT tile to issue
            int hq[LAHG];                                  // group 1: source pixel of this lane's row in halo pieces gw, gw + 4, ...
#pragma unroll
            for (int i = 0; i < PWG; ++i)
                wp[i] = p.W + bz * p.sW + (long)min(n0 + (gw * PWG + i) * 8 + lrow, p.N - 1) * p.ldw + gch * 8 + (long)(kt_first + 2) * 64;
#pragma unroll
            for (int i = 0; i < LAHG; ++i) hq[i] = halo_pix(min(gw + 4 * i, PAH - 1) * 8 + lrow);
            // One MFMA block = the wave's 2 TM TN MFMAs + (a few VALU instructions after every other one) the LDS byte addresses of
            // the fragments of the tile this wave reads NEXT and the bumped weight pointers.
            auto mfmas = [&](int shift_n, int abase_n, int wb_n) {
                static_assert(TM * TN >= 2 * TM + 1 + PWG, "not enough MFMAs to spread the address steps over");
                PBE_SETPRIO(1);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int i = 0; i < TN; ++i)
#pragma unroll
                        for (int j = 0; j < TM; ++j) {
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[ks][i], fa[ks][j], acc[i][j], 0, 0, 0);
                            const int q = (ks * TN + i) * TM + j;             // compile-time after unrolling
                            if (q & 1) {
                                const int st = q >> 1;
                                __builtin_amdgcn_sched_barrier(0);       // (each step pinned between its MFMAs: left free, the unrolled taps' steps
                                if (st < 2 * TM) {                       //  are hoisted together and the block spills)
                                    const int jj = st >> 1;
                                    if ((st & 1) == 0) {
                                        const int ar = hc[jj] + shift_n;
                                        aaddr[0][jj] = abase_n + ar * 128 + ((fq ^ (ar & 7)) << 4);
                                    } else aaddr[1][jj] = aaddr[0][jj] ^ 64;
                                } else if (st == 2 * TM) { waddr[0] = wb_n + w_rd + rsw; waddr[1] = wb_n + w_rd + (rsw ^ 64); }
                                else if (st < 2 * TM + 1 + PWG) wp[st - 2 * TM - 1] += 64;
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                PBE_SETPRIO(0);
            };
            // One channel block = 9 periods, UNROLLED: the tap, the ring slot (9 % 3 == 0: a block starts at slot 0), which DMA pieces
            // a period issues and how many may stay in flight at its end are compile-time constants - the run-time form of this
            // loop spent ~25 scalar branches per period on them (and copied the halo pointer arrays around a switch).
            //   period (blk, tap), right behind the fragment reads: group 0 issues W(kt + 2) into tile kt - 1's slot (unless the block
            //   is the workgroup's last and tap >= 7) and retires W(kt + 1) at the period's end; group 1 issues halo pieces 2 tap and
            //   2 tap + 1 of block blk + 1 and retires the whole halo in its read half of tap 8, before the barrier that opens the
            //   next block.
            auto block = [&](auto LASTC, int blk) {
                constexpr bool LAST = decltype(LASTC)::value;
                const int abase = ((blk - blk0) & 1) * G::HALO_BYTES, abase_o = G::HALO_BYTES - abase;
                const h16* hbase = zsrc;                   // source of halo row 0's chunk for block blk + 1
                long hcs = 0;
                if (!LAST) {
                    const int c0b = (blk + 1) * 64;
                    const bool first = c0b < p.C1;
                    hbase = (first ? p.A + c0b : p.A2 + (c0b - p.C1)) + gch * 8;
                    hcs = first ? p.C1 : p.C2;
                }
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
#ifdef PBE_STAMPS
                    if (tap == 1 && blk == blk0) PBE_STAMP(3);
#endif
                    constexpr int kPWG = PWG;
                    const bool w = !LAST || tap < 7;
                    PBE_ACC_T0();
                    __builtin_amdgcn_sched_barrier(0);
                    read_frags();
                    __builtin_amdgcn_sched_barrier(0);
                    if (grp == 0) {
                        if (w) {
#pragma unroll
                            for (int i = 0; i < PWG; ++i) PBE_GLDS16(wp[i], wring + ((tap + 2) % 3) * W_BYTES + (gw * PWG + i) * 1024);
                        }
                    } else if (!LAST) {
#pragma unroll
                        for (int i = 2 * tap; i < 2 * tap + 2; ++i)
                            if (i < LAHG) PBE_GLDS16(hq[i] >= 0 ? hbase + (long)hq[i] * hcs : zsrc, abuf + abase_o + min(gw + 4 * i, PAH - 1) * 1024);
                        if (tap == 8) wait_vmcnt<0>();     // the next block's halo has landed (this group has nothing else in flight)
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    PBE_ACC(acc_r_);
                    PBE_ACC_T0();
                    __builtin_amdgcn_s_barrier();
                    PBE_ACC(acc_b1_);
                    __builtin_amdgcn_sched_barrier(0);
                    PBE_ACC_T0();
                    {   // this wave reads tile kt + 1 next: tap + 1 of this block, or tap 0 of the next (other halo buffer)
                        const int tn = tap == 8 ? 0 : tap + 1, trow = tn / 3;
                        // (the row stride re-materialised opaquely per tap: as a loop invariant, all 9 taps' fragment addresses are
                        //  hoisted out of the block loop into 70 more registers and the kernel spills)
                        int hw2 = HW2;
                        asm volatile("" : "+s"(hw2));
                        mfmas((trow - 1) * hw2 + (tn - 3 * trow - 1), tap == 8 ? abase_o : abase, G::WRING_OFF + ((tap + 1) % 3) * W_BYTES);
                    }
                    PBE_ACC(acc_m_);
                    PBE_ACC_T0();
                    // W(kt + 1) landed; this period's tile may fly (mutant 2: as if W(kt + 1) may fly too, once per slice)
                    if (grp == 0) { if (PBE_RACE_MUTANT == 2 && tap == 8 && blk == blk0 && w) wait_vmcnt<2 * kPWG>(); else if (w) wait_vmcnt<kPWG>(); else wait_vmcnt<0>(); }
                    PBE_ACC(acc_w_);
                    __builtin_amdgcn_sched_barrier(0);
                    PBE_ACC_T0();
                    __builtin_amdgcn_s_barrier();
                    PBE_ACC(acc_b2_);
                }
            };
            if (blk0 < blk1) {
                frag_addrs(blk0, 0, 0);
                wait_vmcnt<0>();                            // halo of block blk0, W(kt_first) and W(kt_first + 1) landed: every queue starts empty
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (grp == 1) __builtin_amdgcn_s_barrier();  // the stagger: group 1 runs one barrier late
#pragma unroll 1
                for (int blk = blk0; blk + 1 < blk1; ++blk) block(std::false_type{}, blk);
                block(std::true_type{}, blk1 - 1);
                if (grp == 0) __builtin_amdgcn_s_barrier();  // group 1's last M phase
            }
        } else {
            int slot_rd = 0, slot_wr = D % S;
            for (int blk = blk0; blk < blk1; ++blk) {
                const unsigned char* ab = abuf + ((blk - blk0) & 1) * G::HALO_BYTES;
                const bool next_a = blk + 1 < blk1;
#pragma unroll 1
                for (int tap = 0; tap < 9; ++tap) {          // (not unrolled: 9 copies of the body cost registers and 30 000 lines of ISA)
                    const int kt = blk * 9 + tap;
#ifdef PBE_STAMPS
                    if (kt == blk0 * 9 + 1) PBE_STAMP(3);
#endif
                    // W(kt) must have landed.  Younger DMAs that may stay in flight: the later W tiles (D - 1, fewer at the end) and,
                    // at taps 1 .. D, the halo pieces of block blk + 1 (issued at tap 0 right after W(kt0 + D)).  The halo of THIS
                    // block is older than W(kt) (in-order vmcnt), so it has landed too.
                    const int wleft = min(nk2 - 1 - kt, D - 1);
                    const bool a_young = next_a && tap >= 1 && tap <= D;
                    PBE_ACC_T0();
                    const bool shipped = PBE_RACE_MUTANT != 2 || (D == 1 ? kt != blk0 * 9 + PBE_RACE_MUTANT_KT : kt < blk0 * 9 + PBE_RACE_MUTANT_KT);
                    if (shipped) { if (a_young) ring_wait<LW, LAH, D>(wleft); else ring_wait<LW, 0, D>(wleft); }
                    else if (a_young) ring_wait<LW, LAH, D, 1>(wleft);      // as if wleft + 1 weight tiles may stay in flight: W(kt) itself
                    else ring_wait<LW, 0, D, 1>(wleft);
                    PBE_ACC(acc_w_);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    PBE_ACC_T0();
                    __builtin_amdgcn_s_barrier();
                    PBE_ACC(acc_b2_);
                    const unsigned char* sw = wring + slot_rd * W_BYTES;
                    const int trow = tap >= 6 ? 2 : (tap >= 3 ? 1 : 0);
                    const int shift = (trow - 1) * HW2 + (tap - 3 * trow - 1);
                    h16x8 fa[BOTH ? 2 : 1][TM], fw[BOTH ? 2 : 1][TN];
                    int arow[TM];
#pragma unroll
                    for (int j = 0; j < TM; ++j) arow[j] = hc[j] + shift;
#pragma unroll
                    for (int ks = 0; ks < (BOTH ? 2 : 1); ++ks) {
#pragma unroll
                        for (int j = 0; j < TM; ++j)
                            fa[ks][j] = *reinterpret_cast<const h16x8*>(ab + arow[j] * 128 + (((ks * 4 + fq) ^ (arow[j] & 7)) << 4));
#pragma unroll
                        for (int i = 0; i < TN; ++i) fw[ks][i] = *reinterpret_cast<const h16x8*>(sw + w_rd + (rsw ^ (ks * 64)) + i * 16 * 128);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (kt + D < nk2) issue_w(kt + D, slot_wr);
                    if (tap == 0 && next_a) issue_a(blk + 1, (blk + 1 - blk0) & 1);
                    __builtin_amdgcn_sched_barrier(0);
                    PBE_SETPRIO(1);
#pragma unroll
                    for (int i = 0; i < TN; ++i)
#pragma unroll
                        for (int j = 0; j < TM; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[0][i], fa[0][j], acc[i][j], 0, 0, 0);
                    if constexpr (!BOTH) {
#pragma unroll
                        for (int j = 0; j < TM; ++j)
                            fa[0][j] = *reinterpret_cast<const h16x8*>(ab + arow[j] * 128 + (((4 + fq) ^ (arow[j] & 7)) << 4));
#pragma unroll
                        for (int i = 0; i < TN; ++i) fw[0][i] = *reinterpret_cast<const h16x8*>(sw + w_rd + (rsw ^ 64) + i * 16 * 128);
                    }
#pragma unroll
                    for (int i = 0; i < TN; ++i)
#pragma unroll
                        for (int j = 0; j < TM; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[BOTH ? 1 : 0][i], fa[BOTH ? 1 : 0][j], acc[i][j], 0, 0, 0);
                    PBE_SETPRIO(0);
                    slot_rd = slot_rd + 1 == S ? 0 : slot_rd + 1;
                    slot_wr = slot_wr + 1 == S ? 0 : slot_wr + 1;
                }
            }
        }
    } else {
    PBE_STAMP(1);                                    // loader state (+ tap table) ready
#pragma unroll
    for (int t = 0; t < D; ++t)
        if (kt0 + t < nk) issue(kt0 + t, t);
    PBE_STAMP(2);                                    // ring primed (issue only)
    stage_svec();
    // EX_GN: this tile's sample's table -> LDS, a straight 16-byte copy behind the first DMAs; the first k-tile's barrier publishes it
    const float* gnt = reinterpret_cast<const float*>(smem + G::GN_OFF);
    if constexpr (EXG) {
        const int smp = (int)udiv_mg((unsigned)tm_i, (unsigned)p.gn_tdiv, p.mg_gn_tdiv);
        const f32x4* src = reinterpret_cast<const f32x4*>(p.gn_tab + (long)smp * 2 * p.K);
        f32x4* dst = reinterpret_cast<f32x4*>(smem + G::GN_OFF);
        for (int idx = tid; idx < p.K >> 1; idx += NT) dst[idx] = src[idx];
    }
    // one A fragment (8 consecutive channels from k) normalised in place: the fp32 multiply-add and the single rounding of gn_apply_kernel
    auto gn_fold = [&](h16x8& a, int k) {
        const f32x4* t = reinterpret_cast<const f32x4*>(gnt + 2 * k);
        const f32x4 s0 = t[0], s1 = t[1], h0 = t[2], h1 = t[3];
        // (the fp32 result is made opaque before it is rounded: left alone, multiply-add and conversion fuse into v_fma_mixlo / mixhi_f16,
        //  which rounds the exact sum to fp16 ONCE - the pass rounds to fp32 first, and one element in some 8 000 then differs by an ulp)
        float f[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f[e] = (float)a[e] * s0[e] + h0[e];
            f[4 + e] = (float)a[4 + e] * s1[e] + h1[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            asm("" : "+v"(f[e]));
            a[e] = (h16)f[e];
        }
    };
    int slot_rd = 0, slot_wr = D % S;
    for (int kt = kt0; kt < nk; ++kt) {
#ifdef PBE_STAMPS
        if (kt == kt0 + 1) PBE_STAMP(3);             // first k-tile consumed: prologue latency ends
#endif
        const int rem = min(nk - 1 - kt, D - 1);     // later tiles that may stay in flight
        PBE_ACC_T0();
        const bool relaxed = PBE_RACE_MUTANT == 1 && (D == 1 ? kt == kt0 + PBE_RACE_MUTANT_KT : kt >= kt0 + PBE_RACE_MUTANT_KT);
        if (relaxed) ring_wait<LPT, 0, D, 1>(rem);      // as if one more tile may stay in flight: tile kt itself
        else ring_wait<LPT, 0, D>(rem);
        PBE_ACC(acc_w_);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        PBE_ACC_T0();
        __builtin_amdgcn_s_barrier();                // tile kt landed for every wave; slot_wr (tile kt-1's) is free
        PBE_ACC(acc_b2_);
        PBE_ACC_T0();
        const unsigned char* sa = smem + slot_rd * STAGE;
        const unsigned char* sw = sa + A_BYTES;
        h16x8 fa[BOTH ? 2 : 1][TM], fw[BOTH ? 2 : 1][TN];
#pragma unroll
        for (int ks = 0; ks < (BOTH ? 2 : 1); ++ks) {
#pragma unroll
            for (int j = 0; j < TM; ++j) fa[ks][j] = *reinterpret_cast<const h16x8*>(sa + a_rd + (rsw ^ (ks * 64)) + j * 16 * 128);
#pragma unroll
            for (int i = 0; i < TN; ++i) fw[ks][i] = *reinterpret_cast<const h16x8*>(sw + w_rd + (rsw ^ (ks * 64)) + i * 16 * 128);
        }
        __builtin_amdgcn_sched_barrier(0);           // fragment reads go out first, the DMA pieces behind them (tools/ubench_loop.hip:
        if (kt + D < nk) issue(kt + D, slot_wr);     //  cheaper there than before the reads, between the MFMAs or after them)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (EXG) {
#pragma unroll
            for (int ks = 0; ks < (BOTH ? 2 : 1); ++ks)
#pragma unroll
                for (int j = 0; j < TM; ++j) gn_fold(fa[ks][j], kt * 64 + ks * 32 + fq * 8);
        }
        PBE_ACC(acc_r_);
        PBE_ACC_T0();
        PBE_SETPRIO(1);
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j)
                acc[i][j] = F8 ? mfma_pair_f8(fw[0][i], fa[0][j], acc[i][j]) : __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[0][i], fa[0][j], acc[i][j], 0, 0, 0);
        if constexpr (!BOTH) {
#pragma unroll
            for (int j = 0; j < TM; ++j) fa[0][j] = *reinterpret_cast<const h16x8*>(sa + a_rd + (rsw ^ 64) + j * 16 * 128);
#pragma unroll
            for (int i = 0; i < TN; ++i) fw[0][i] = *reinterpret_cast<const h16x8*>(sw + w_rd + (rsw ^ 64) + i * 16 * 128);
            if constexpr (EXG) {
#pragma unroll
                for (int j = 0; j < TM; ++j) gn_fold(fa[0][j], kt * 64 + 32 + fq * 8);
            }
        }
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j)
                acc[i][j] = F8 ? mfma_pair_f8(fw[BOTH ? 1 : 0][i], fa[BOTH ? 1 : 0][j], acc[i][j])
                               : __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[BOTH ? 1 : 0][i], fa[BOTH ? 1 : 0][j], acc[i][j], 0, 0, 0);
        PBE_SETPRIO(0);
        PBE_ACC(acc_m_);
        slot_rd = slot_rd + 1 == S ? 0 : slot_rd + 1;
        slot_wr = slot_wr + 1 == S ? 0 : slot_wr + 1;
    }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    PBE_STAMP(4);                                    // main loop issued
    PBE_ACC_STORE();

    if (p.splits > 1) {
        // raw fp32 partial sums -> slab blockIdx.z; splitk_reduce_kernel applies the epilogue
        float* slab = p.ws + (long)blockIdx.z * p.M * p.N;
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int n = n0 + wn * WN + i * 16 + fq * 4;
#pragma unroll
            for (int j = 0; j < TM; ++j) {
                const int m = m0 + wm * WM + j * 16 + fr;
                if (m < p.M && n < p.N) *reinterpret_cast<f32x4*>(slab + (long)m * p.N + n) = acc[i][j];
            }
        }
        PBE_STAMP(6);
        PBE_STAMP(8);
        return;
    }

    // ---- epilogue: one wave-row group (WM rows of the tile) at a time through LDS ----
    h16* sC = reinterpret_cast<h16*>(smem);
    h16* Cb = p.C + bz * p.sC;
    // phase form: row m = (b, y, x) of phase (py, px) lands on output pixel (2y + py, 2x + px) of the [B, 2H, 2W, N] tensor
    const int ph_off = (MODE == 1 && p.phase) ? (int)(blockIdx.y >> 1) * 2 * p.Wd + (int)(blockIdx.y & 1) : 0;
    auto out_row = [&](int m) -> long {
        if (MODE == 1 && p.phase) { const int q = m / p.Wd; return 4L * p.Wd * q + 2 * (m - q * p.Wd) + ph_off; }
        return m;
    };
    const h16* Rb = p.resid ? p.resid + bz * p.sR : nullptr;
    constexpr int CPR = BN / 8;
    constexpr bool ONE_PASS = G::ONE_PASS, GS_OK = G::GS_OK;      // whole C tile per pass; GroupNorm statistics from the copy-out (TileGeom)
    constexpr int NG = ONE_PASS ? 1 : NWM;            // passes
    constexpr int GR = ONE_PASS ? BM : WM;            // rows per pass
    // The register -> LDS half has a compile-time FAST path (bias / row vector staged in svec, one sample per tile, no
    // per-row bias): the generic form (per-element bounds checks, global bias loads and row-vector gathers with an
    // integer division per quad, all in one unrolled body) ran ~7 000 instructions per thread and cost 35 % of a
    // K = 320 GEMM.
    // Tiles with <= 96 accumulator registers also specialise the activation at compile time (5 copies of the unrolled body);
    // for the 256-row tiles (128-160 accumulator registers) that many copies push the allocator into scratch, so there the
    // activation stays a uniform run-time branch per quad.
    constexpr bool ARMS = TM * TN * 4 <= 96;
    constexpr int CLDT = GR + 8;                      // EX: row stride of the transposed C tile (V^T tiles)
    static_assert(EXF == 0 || (ONE_PASS && (size_t)BN * CLDT * 2 <= (size_t)S * STAGE), "extended epilogue: whole C tile (either orientation) in the ring's LDS");
    static_assert(!EXM || ONE_PASS, "MX-fp8 copy-out: whole C tile in LDS");
    const bool vtile = EXV && p.vt && n0 >= p.vt_col0;     // uniform: this tile's columns belong to the transposed output
    auto stage = [&](int g, auto FAST, auto ACT, auto VTT) {
        constexpr bool F = decltype(FAST)::value, VT = decltype(VTT)::value;
        const int A = decltype(ACT)::value >= 0 ? decltype(ACT)::value : p.act;
        // alpha is re-materialised opaquely per pass: as a plain loop invariant, acc * alpha is hoisted out of the pass loop
        // into a second full set of accumulator registers and the 256-row tiles spill (measured: 30 us of epilogue per tile).
        float al = p.alpha;
        asm volatile("" : "+s"(al));
        float ln_rs[EXL ? TM : 1], ln_nm[EXL ? TM : 1];    // LayerNorm fold: this lane's rows' rstd and -mean rstd (LDS, read once)
        if constexpr (EXL) {
            if (EXF != 7 || p.ln_stat) {
#pragma unroll
                for (int j = 0; j < TM; ++j) {
                    const int ml = (ONE_PASS ? wm * WM : 0) + j * 16 + fr;
                    ln_rs[j] = sca[g * GR + ml]; ln_nm[j] = scw[g * GR + ml];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int nl = wn * WN + i * 16 + fq * 4;
            const int n = n0 + nl;
            float ali = al, c1a[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (EXV) ali = (p.alpha_cols > 0 && n >= p.alpha_cols) ? 1.f : al;
            if constexpr (EXL) {
                if (EXF != 7 || p.ln_stat) {
                    const f32x4 c1 = *reinterpret_cast<const f32x4*>(lnc + nl);
#pragma unroll
                    for (int r = 0; r < 4; ++r) c1a[r] = ali * c1[r];
                }
            }
            float bn[4] = {0.f, 0.f, 0.f, 0.f};
            if (F) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(svec + nl);
#pragma unroll
                for (int r = 0; r < 4; ++r) bn[r] = t[r];
            } else if (!p.sv_ok && p.bias && !p.bias_row) {
#pragma unroll
                for (int r = 0; r < 4; ++r) bn[r] = (n + r < p.N) ? p.bias[n + r] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < TM; ++j) {
                const int ml = (ONE_PASS ? wm * WM : 0) + j * 16 + fr;
                float v[4];
                // every path forms  acc * alpha + (bias + row vector)  with the SAME association (the vector sum first, one fused
                // multiply-add): which path a tile takes depends on the tile shape, and the tile shape must not change the bits
                float add[4] = {bn[0], bn[1], bn[2], bn[3]};
                if (!F) {
                    const int m = m0 + g * GR + ml;
                    if (p.sv_ok) {                           // several samples per tile (8x8 level), or a per-row bias
                        const f32x4 t = *reinterpret_cast<const f32x4*>(svec + (sv_ns > 1 ? (g * GR + ml) / p.group_rows : 0) * BN + nl);
#pragma unroll
                        for (int r = 0; r < 4; ++r) add[r] = t[r];
                    } else if (p.rowvec && m < p.M) {
                        const h16* rv = p.rowvec + (long)(m / p.group_rows) * p.ldv + n;
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (n + r < p.N) add[r] = bn[r] + (float)rv[r];
                    }
                }
                if constexpr (F8) {
                    const float sm = sca[g * GR + ml] * al;
                    const f32x4 sn = *reinterpret_cast<const f32x4*>(scw + nl);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaf(acc[i][j][r], sm * sn[r], add[r]);
                } else if constexpr (EXF != 0) {
                    // NO run-time branch inside the unrolled body: a uniform branch per quad splits it into 40 basic blocks and the
                    // GELU chains (rcp -> 4 fma -> exp) of different quads can no longer be interleaved (the GEGLU projection ran 12 % slower).
                    // The LayerNorm-only / q|k|v forms therefore ALWAYS fold (their dispatch guarantees ln_stat), the V^T orientation is a
                    // compile-time argument of stage(); only the catch-all form (EX = 7) decides at run time.
                    if constexpr (EXL && EXF != 7) {          // LN(x) W^T = rstd (x W'^T - mean colsum(W')) with W' = W gamma (bias holds W beta + b)
                        const float ars = ali * ln_rs[j];    //   alpha (rstd acc - mean rstd colsum) + bias  =  acc (alpha rstd) + ((-mean rstd) (alpha colsum) + bias)
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaf(acc[i][j][r], ars, __builtin_fmaf(ln_nm[j], c1a[r], add[r]));
                    } else {
                        const float ars = (EXL && p.ln_stat) ? ali * ln_rs[j] : ali, nmj = (EXL && p.ln_stat) ? ln_nm[j] : 0.f;      // (c1a = 0 without ln_stat)
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaf(acc[i][j][r], ars, __builtin_fmaf(nmj, c1a[r], add[r]));
                    }
                    if constexpr (VT) {                      // V^T tile: the C tile goes to LDS transposed, [column][row]
#pragma unroll
                        for (int r = 0; r < 4; ++r) sC[(nl + r) * CLDT + ml] = (h16)v[r];
                        continue;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaf(acc[i][j][r], al, add[r]);
                }
                if (!F) {
                    const int m = m0 + g * GR + ml;
                    if (p.bias && p.bias_row) {
                        const float bm = (m < p.M) ? p.bias[m] : 0.f;
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] += bm;
                    }
                }
                if (A == PBE_ACT_GEGLU) {                    // columns interleaved (x_j, gate_j): out_j = x_j * gelu(gate_j)
                    h16x2 o2 = {(h16)(v[0] * gelu_erf_f(v[1])), (h16)(v[2] * gelu_erf_f(v[3]))};
                    *reinterpret_cast<h16x2*>(sC + ml * CLD + (nl >> 1)) = o2;
                } else {
                    apply_act4(v, A);
                    h16x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = (h16)v[r];
                    *reinterpret_cast<h16x4*>(sC + ml * CLD + nl) = o;
                }
            }
        }
    };
    // LDS -> global half: whole 16-byte row segments, residual added on the way out.  A thread's chunks are handled in batches
    // of UB: all residual loads of a batch are issued first, then the LDS reads, then the adds and stores - one exposed memory
    // round trip per batch instead of one per chunk (tools/phase_stamps.py: the chunk-at-a-time form spent 11 400 of a
    // K = 320 GEMM workgroup's 33 800 cycles here when a residual is fused, 4 000 without).
    auto copy_out = [&](int g, auto GG) {
        constexpr bool gg = decltype(GG)::value;             // GEGLU halves the output width
        constexpr int cpr = gg ? CPR / 2 : CPR;
        constexpr int TOT = GR * cpr, IT = (TOT + NT - 1) / NT;
        // (tiles whose accumulators stay live across the passes - NG > 1 - have no registers for a deep batch)
        constexpr int UB = !ONE_PASS ? (IT % 2 == 0 ? 2 : 1) : (IT % 5 == 0 ? 5 : (IT % 4 == 0 ? 4 : (IT % 3 == 0 ? 3 : (IT % 2 == 0 ? 2 : 1))));
        const int Nout = gg ? p.N >> 1 : p.N, nb = gg ? n0 >> 1 : n0;
        if constexpr (EXM && !gg) {
            // MX-fp8 copy-out: one thread per 32-element block of the staged fp16 tile (mx8_*_blocks).  The planner guarantees that no block
            // crosses a tile boundary and that every tile lies inside one range (mx_tile_ok).
            if (p.mx_crow) {                                 // rows = channels, columns = tokens (one VT range, sample bz)
                constexpr int BPR = BN / 32;
                for (int idx = tid; idx < GR * BPR; idx += NT) {
                    const int row = idx / BPR, cb = idx - row * BPR;
                    const int m = m0 + g * GR + row, n = n0 + cb * 32;
                    if (m >= p.M || n >= p.N) continue;
                    mx8_vt_block(p, 0, sC + row * CLD + cb * 32, (int)bz, m, n);
                }
                return;
            }
            const int r = mx8_range(p, n0);
            if (r < 0) return;
            if (p.mx_layout[r] == PBE_MX8_VT) {              // transposed tile (EX_VT): LDS row = channel, GR tokens per row
                if constexpr (EXV) {
                    constexpr int BPR = GR / 32;
                    for (int idx = tid; idx < BN * BPR; idx += NT) {
                        const int crow = idx / BPR, tb = idx - crow * BPR;
                        const int m = m0 + tb * 32;
                        if (m >= p.M || n0 + crow >= p.N) continue;
                        const int b = m / p.mx_N;
                        mx8_vt_block(p, r, sC + crow * CLDT + tb * 32, b, n0 - p.mx_c0[r] + crow, m - b * p.mx_N);
                    }
                }
                return;
            }
            mx8_token_blocks(p, r, sC, CLD, GR, n0, BN, m0 + g * GR, tid, NT);
            return;
        }
        if constexpr (EXV && !gg) {
            if (vtile) {
                // transposed tile: LDS row = output channel, 16-byte chunks of 8 consecutive tokens -> vt[b][channel][token] rows
                constexpr int tpr = GR / 8;
                for (int idx = tid; idx < BN * tpr; idx += NT) {
                    const int crow = idx / tpr, tch = idx - crow * tpr;
                    const int m = m0 + tch * 8, c = n0 - p.vt_col0 + crow;
                    if (m >= p.M || n0 + crow >= p.N) continue;
                    const int b = m / p.vt_tok, tok = m - b * p.vt_tok;
                    *reinterpret_cast<h16x8*>(p.vt + (long)b * p.vt_bs + (long)c * p.vt_rs + tok) = *reinterpret_cast<const h16x8*>(sC + crow * CLDT + tch * 8);
                }
                return;
            }
        }
        if constexpr (EXS && !gg) {
            if (p.rstat) {
                // Row statistics for the LayerNorm that reads this output: 8 lanes per row (full 128-byte lines per row and
                // instruction), each lane sums the STORED fp16 values of its chunks, three xor-shuffles finish the row -
                // fixed order, no atomics.  Partial (sum, sumsq) of (column tile tn_i, row m) -> rstat[tn_i * M + m].
                constexpr int RPP = NT / 8, CPL = (CPR + 7) / 8, NIT = (GR + RPP - 1) / RPP;
                const int l8 = tid & 7, rr = tid >> 3;
                h16x8 r[NIT][CPL];
                if (Rb) {                                    // every residual load of the thread first: one exposed round trip, not NIT
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        const int row = it * RPP + rr, m = m0 + g * GR + row;
#pragma unroll
                        for (int c = 0; c < CPL; ++c) {
                            const int ch = l8 + 8 * c, n = n0 + ch * 8;
                            if (row < GR && m < p.M && ch < CPR && n < p.N) r[it][c] = *reinterpret_cast<const h16x8*>(Rb + (long)m * p.ldr + n);
                        }
                    }
                }
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int row = it * RPP + rr, m = m0 + g * GR + row;
                    const bool rok = row < GR && m < p.M;
                    float s1 = 0.f, s2 = 0.f;
#pragma unroll
                    for (int c = 0; c < CPL; ++c) {
                        const int ch = l8 + 8 * c, n = n0 + ch * 8;
                        if (!(rok && ch < CPR && n < p.N)) continue;
                        h16x8 v = *reinterpret_cast<const h16x8*>(sC + row * CLD + ch * 8);
                        if (Rb) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] = (h16)((float)v[e] + (float)r[it][c][e]);
                        }
#pragma unroll
                        for (int e = 0; e < 8; ++e) { const float f = (float)v[e]; s1 += f; s2 = __builtin_fmaf(f, f, s2); }
                        *reinterpret_cast<h16x8*>(Cb + (long)m * p.ldc + n) = v;
                    }
#pragma unroll
                    for (int o = 1; o < 8; o <<= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
                    if (rok && l8 == 0) *reinterpret_cast<float2*>(p.rstat + 2 * ((long)tn_i * p.rstat_ld + m)) = make_float2(s1, s2);
                }
                return;
            }
        }
        if constexpr (GS_OK && !gg) {
            if (p.gstat) {
                // GroupNorm statistics of this tile's stored values.  A thread keeps ONE 16-byte column chunk and walks rows (slot, slot + RSL,
                // ...): 8 column sums + 8 sums of squares in registers, then a fixed-order fold over the row slots and over a group's columns
                // through LDS (no atomics: bit-reproducible).  Row batches of 4: the residual loads of a batch are issued together.
                constexpr int RSL = NT / CPR, GB = 4;
                float* red = reinterpret_cast<float*>(smem + G::GS_OFF);
                const int slot = tid / CPR, ch = tid - slot * CPR, n = n0 + ch * 8;
                float ca[8], cq[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) { ca[e] = 0.f; cq[e] = 0.f; }
                if (slot < RSL && n < p.N) {
                    for (int r0 = slot; r0 < GR; r0 += RSL * GB) {
                        h16x8 v[GB], r[GB];
                        bool ok[GB];
#pragma unroll
                        for (int u = 0; u < GB; ++u) {
                            const int row = r0 + u * RSL, m = m0 + row;
                            ok[u] = row < GR && m < p.M;
                            if (ok[u] && Rb) r[u] = *reinterpret_cast<const h16x8*>(Rb + (long)m * p.ldr + n);
                        }
#pragma unroll
                        for (int u = 0; u < GB; ++u)
                            if (ok[u]) v[u] = *reinterpret_cast<const h16x8*>(sC + (r0 + u * RSL) * CLD + ch * 8);
#pragma unroll
                        for (int u = 0; u < GB; ++u) {
                            if (!ok[u]) continue;
                            if (Rb) {
#pragma unroll
                                for (int e = 0; e < 8; ++e) v[u][e] = (h16)((float)v[u][e] + (float)r[u][e]);
                            }
#pragma unroll
                            for (int e = 0; e < 8; ++e) { const float f = (float)v[u][e]; ca[e] += f; cq[e] = __builtin_fmaf(f, f, cq[e]); }
                            *reinterpret_cast<h16x8*>(Cb + out_row(m0 + r0 + u * RSL) * p.ldc + n) = v[u];
                        }
                    }
                }
                if (slot < RSL) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) *reinterpret_cast<float2*>(red + ((slot * BN) + ch * 8 + e) * 2) = make_float2(ca[e], cq[e]);
                }
                __syncthreads();
                float* col = red + RSL * BN * 2;               // [BN][2] column totals
                if (tid < BN) {
                    float a = 0.f, q = 0.f;
                    for (int sl = 0; sl < RSL; ++sl) { const float2 t = *reinterpret_cast<const float2*>(red + (sl * BN + tid) * 2); a += t.x; q += t.y; }
                    *reinterpret_cast<float2*>(col + tid * 2) = make_float2(a, q);
                }
                __syncthreads();
                const int cg = p.gs_cg, gl = tid;               // group gl of this tile's BN / cg
                if (gl * cg < BN && n0 + gl * cg < p.N) {
                    float a = 0.f, q = 0.f;
                    for (int c = gl * cg; c < (gl + 1) * cg; ++c) { const float2 t = *reinterpret_cast<const float2*>(col + c * 2); a += t.x; q += t.y; }
                    const int b = m0 / p.gs_hw, blk = (m0 - b * p.gs_hw) / BM, nblk = p.gs_hw / BM;
                    *reinterpret_cast<float2*>(p.gstat + (((long)b * nblk + blk) * p.gs_groups + n0 / cg + gl) * 2) = make_float2(a, q);
                }
                return;
            }
        }
        if (p.vec) {
            for (int it0 = 0; it0 < IT; it0 += UB) {
                h16x8 v[UB], r[UB];
                long go[UB];
                int lo[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const int idx = tid + (it0 + u) * NT;
                    const int row = idx / cpr, ch = idx - row * cpr;
                    const int m = m0 + g * GR + row, n = nb + ch * 8;
                    const bool ok = idx < TOT && m < p.M && n < Nout;
                    go[u] = ok ? out_row(m) * p.ldc + n : -1;
                    lo[u] = row * CLD + ch * 8;
                    if (ok && Rb) r[u] = *reinterpret_cast<const h16x8*>(Rb + (long)m * p.ldr + n);
                }
#pragma unroll
                for (int u = 0; u < UB; ++u)
                    if (go[u] >= 0) v[u] = *reinterpret_cast<const h16x8*>(sC + lo[u]);
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    if (go[u] < 0) continue;
                    if (Rb) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[u][e] = (h16)((float)v[u][e] + (float)r[u][e]);
                    }
                    *reinterpret_cast<h16x8*>(Cb + go[u]) = v[u];
                }
            }
            return;
        }
        for (int idx = tid; idx < TOT; idx += NT) {
            const int row = idx / cpr, ch = idx - row * cpr;
            const int m = m0 + g * GR + row, n = nb + ch * 8;
            if (m >= p.M || n >= Nout) continue;
            const h16x8 v = *reinterpret_cast<const h16x8*>(sC + row * CLD + ch * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (n + e < Nout) {
                    float f = (float)v[e];
                    if (Rb) f += (float)Rb[(long)m * p.ldr + n + e];
                    Cb[out_row(m) * p.ldc + n + e] = (h16)f;
                }
            }
        }
    };
    const bool fast = p.sv_ok && sv_ns == 1 && !(p.bias && p.bias_row);
#pragma unroll 1
    for (int g = 0; g < NG; ++g) {
        __syncthreads();                              // ring reads (g == 0) / previous group's copy-out done
        if (ONE_PASS || wm == g) {
            auto run = [&](auto FAST) {
                if constexpr (EXV) {
                    if (vtile) { stage(g, FAST, std::integral_constant<int, 0>{}, std::true_type{}); return; }      // V^T tiles: no activation
                }
                if constexpr (ARMS) {
                    switch (p.act) {
                        case 1: stage(g, FAST, std::integral_constant<int, 1>{}, std::false_type{}); break;
                        case 2: stage(g, FAST, std::integral_constant<int, 2>{}, std::false_type{}); break;
                        case 3: stage(g, FAST, std::integral_constant<int, 3>{}, std::false_type{}); break;
                        case PBE_ACT_GEGLU: stage(g, FAST, std::integral_constant<int, PBE_ACT_GEGLU>{}, std::false_type{}); break;
                        default: stage(g, FAST, std::integral_constant<int, 0>{}, std::false_type{}); break;
                    }
                } else {
                    stage(g, FAST, std::integral_constant<int, -1>{}, std::false_type{});
                }
            };
            if (fast) run(std::true_type{});
            else run(std::false_type{});
        }
        __syncthreads();
#ifdef PBE_STAMPS
        if (g == NG - 1) PBE_STAMP(5);               // last register -> LDS pass done (includes waiting for the MFMAs to drain)
#endif
        if (p.act == PBE_ACT_GEGLU) copy_out(g, std::true_type{});
        else copy_out(g, std::false_type{});
    }
    PBE_STAMP(6);                                    // stores issued
    PBE_STAMP(8);                                    // wall clock (100 MHz) of the end
}

// Sum the split-K slabs in a fixed order (deterministic) and apply the epilogue: 4 columns per thread.
static __global__ void __launch_bounds__(256) splitk_reduce_kernel(const IGemmP p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int n4 = p.N >> 2;
    if (i >= (long)p.M * n4) return;
    const int m = (int)(i / n4), n = (int)(i - (long)m * n4) * 4;
    // every global load of this thread is issued up front (epilogue operands, then the slabs four at a time): with one
    // load per loop trip the kernel is a chain of `splits` memory round trips.  The ADD order stays slab 0, 1, 2, ... (deterministic).
    float ev[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) {
#pragma unroll
        for (int r = 0; r < 4; ++r) ev[r] = p.bias_row ? p.bias[m] : p.bias[n + r];
    }
    if (p.rowvec) {
        const h16* rv = p.rowvec + (long)(m / p.group_rows) * p.ldv + n;
#pragma unroll
        for (int r = 0; r < 4; ++r) ev[r] += (float)rv[r];
    }
    if (p.resid && p.act != PBE_ACT_GEGLU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) rs[r] = (float)p.resid[(long)m * p.ldr + n + r];
    }
    const float* sl = p.ws + (long)m * p.N + n;
    const long zs = (long)p.M * p.N;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    int z = 0;
    for (; z + 4 <= p.splits; z += 4) {
        const f32x4 t0 = *reinterpret_cast<const f32x4*>(sl + (z + 0) * zs), t1 = *reinterpret_cast<const f32x4*>(sl + (z + 1) * zs);
        const f32x4 t2 = *reinterpret_cast<const f32x4*>(sl + (z + 2) * zs), t3 = *reinterpret_cast<const f32x4*>(sl + (z + 3) * zs);
        a += t0; a += t1; a += t2; a += t3;
    }
    for (; z < p.splits; ++z) a += *reinterpret_cast<const f32x4*>(sl + z * zs);
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = a[r] * p.alpha + ev[r];
    if (p.act == PBE_ACT_GEGLU) {
        h16x2 o2 = {(h16)(v[0] * gelu_erf_f(v[1])), (h16)(v[2] * gelu_erf_f(v[3]))};
        *reinterpret_cast<h16x2*>(p.C + (long)m * p.ldc + (n >> 1)) = o2;
        return;
    }
    h16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float f = (float)(h16)apply_act(v[r], p.act) + rs[r];          // same rounding point as the fused epilogue
        o[r] = (h16)f;
    }
    *reinterpret_cast<h16x4*>(p.C + (long)m * p.ldc + n) = o;
}
