// Host side of the implicit-GEMM kernel (igemm_kernel.h, which also holds the tile table kTiles): the planner, the launch-invariant prologue values and the launcher.
#pragma once
#include "igemm_kernel.h"

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
struct Plan { int cfg; int splits; };
#ifdef PBE_STAMPS
extern unsigned long long* g_pbe_stamps;
#endif
extern int g_pbe_force_cfg;     // (defined in igemm.hip) pbe_tune(1, cfg index [| splits << 8]) forces a tile config (and split-K factor); -1 = heuristic
extern int g_pbe_allow_splitk;  // pbe_tune(2, 0/1)

// k-tiles of 64 per split-K granule: a halo tile splits at channel-block boundaries (9 taps)
static inline int no_empty_slices(int nk, int granule, int s) {
    const int units = (nk + granule - 1) / granule;
    if (s > units) s = units;
    if (s < 2) return 1;
    const int per = (units + s - 1) / s;
    return (units + per - 1) / per;
}

// Split-K at all: batch 1, a workspace, and the 4-column rows of C (and the residual) the reduce kernel writes (reads)
static inline bool splitk_ok(const IGemmP& p, int batch) {
    return g_pbe_allow_splitk && batch == 1 && p.ws && !(p.N & 3) && !(p.ldc & 3) && !(p.resid && (p.ldr & 3));
}

// Clamp a split-K factor to what the problem allows: >= 4 k-tiles of 64 per slice, slabs fit the workspace, no empty slice
static int clamp_splits(const IGemmP& p, const TileCfg& c, size_t ws_bytes, int s) {
    const int nk = (p.K + 63) >> 6;
    if (s > nk / 4) s = nk / 4;
    while (s > 1 && (size_t)s * p.M * p.N * sizeof(float) > ws_bytes) --s;
    return no_empty_slices(nk, c.hpa ? 9 : 1, s);
}

static int splits_for(const IGemmP& p, const TileCfg& c, int batch, size_t ws_bytes, long tiles) {
    if (!splitk_ok(p, batch)) return 1;
    const int nk = (p.K + 63) >> 6;                          // k-tiles of 64
    const long slots = 256L * c.slots_per_cu;
    if (tiles * 4 > slots * 3 || nk < 8) return 1;           // grid already fills >= 75 % of the chip
    const int s = (int)((slots * 5 / 4 + tiles - 1) / tiles);
    return clamp_splits(p, c, ws_bytes, s > 32 ? 32 : s);
}

// Can this conv run as a halo-resident tile of bm pixels with a halo image of hpa rows?  Returns the image rows per tile (0: no).
static int halo_rows(const IGemmP& p, int mode, int bm, int hpa) {
    if (mode != 1 || p.cstride != 1 || p.pad != 1 || p.ups || p.phase || p.cb != 64) return 0;
    const int W = p.Wd, H = p.H;
    if (W < 8 || W > 128 || (W & (W - 1)) || bm % W || (p.M % bm)) return 0;
    const int th = bm / W < H ? bm / W : H;
    if (H % th || bm % (th * W)) return 0;                        // a tile is whole rows of one image or a whole number of images:
    const int nsub = bm / (th * W);                               // whole images per tile when the image is smaller than the tile
    if (nsub > 1 && th != H) return 0;                            // the kernel derives image and row of a pixel from nsub * th * W == bm
    if (nsub * ((th + 2) * (W + 1) + 1) > hpa) return 0;       // halo rows: row stride W + 1 (shared zero column) + 1
    return th;
}

bool pbe_astat_ok(const IGemmP& p, int batch, int cfg);      // igemm_astat.hip: can tile 19 / 20 run this problem?

// MX-fp8 copy-out (IGemmP.mx_*): can tile t write its blocks without any 32-element MX block crossing a tile boundary?  Every range starts
// on a column tile, TOKENS ranges end on one too, every column-tile boundary inside a TOKENS range is a block boundary (h D + 32 j) - at
// half-tile granularity for the A-stationary tile, whose q|k rows leave BN / 2 columns at a time - and V^T blocks of 32 tokens start on
// 32-token boundaries (rows: every tile height is a multiple of 32; columns of the channel-row form: every tile width is).
static inline bool mx_tile_ok(const IGemmP& p, const TileCfg& t) {
    if (t.bm % 32 || t.bn % 32) return false;
    if (p.mx_crow) return true;
    const int D = p.mx_D, w = (t.forms & F_ASTAT) ? t.bn / 2 : t.bn;
    for (int r = 0; r < p.mx_nr; ++r) {
        if (p.mx_c0[r] % t.bn) return false;
        if (p.mx_layout[r] != PBE_MX8_TOKENS) continue;
        const int width = p.mx_H * D;
        if ((p.mx_c0[r] + width) % t.bn && p.mx_c0[r] + width != p.N) return false;
        for (int x = w; x < width; x += w)
            if ((x % D) % 32) return false;
    }
    return true;
}
static inline bool ex_needed(const IGemmP& p) { return p.alpha_cols > 0 || p.ln_stat || p.rstat || p.vt || p.gn_tab; }
// GroupNorm fold (IGemmP.gn_*; gn_tdiv holds the tokens per sample until launch_cfg divides it by the tile's rows): a tile's rows belong to one sample
static inline bool gn_tile_ok(const IGemmP& p, const TileCfg& t) { return (t.forms & F_EX) && !(t.forms & F_ASTAT) && p.gn_tdiv % t.bm == 0; }

// V^T columns start on a column tile (igemm_kernel's vtile): a tile with n0 < vt_col0 stores ALL its columns to C.  The widths the
// extended-epilogue heuristic can choose among: is one of them a divisor of vt_col0?  (A requested tile that cannot run the problem
// falls back to the heuristic, and the forced-only A-stationary tiles are as wide as streaming ones, so this decides every tile_cfg.)
static inline bool vt_tile_exists(int vt_col0) {
    for (const TileCfg& t : kTiles)
        if ((t.forms & F_EX) && !(t.forms & F_FORCED) && vt_col0 % t.bn == 0) return true;
    return false;
}
static inline const char* ex_tile_widths(char* buf, size_t n) {      // "64, 128, 160, 320": the distinct widths above, ascending, for error texts
    size_t len = 0;
    buf[0] = 0;
    for (int last = 0;;) {
        int next = 0;
        for (const TileCfg& t : kTiles)
            if ((t.forms & F_EX) && !(t.forms & F_FORCED) && t.bn > last && (!next || t.bn < next)) next = t.bn;
        if (!next || len + 8 > n) return buf;
        len += snprintf(buf + len, n - len, "%s%d", len ? ", " : "", next);
        last = next;
    }
}

// want_cfg: -1 = heuristic; else (tile config index) | (split-K factor << 8), factor 0 = heuristic factor for that tile.
// A requested factor is clamped to what the problem allows (batch 1, >= 4 k-tiles of 64 per slice, slabs fit the workspace).
// (the developer knobs g_pbe_force_cfg / g_pbe_allow_splitk are READ here and never written outside pbe_tune: a caller that must
//  not split passes ws_bytes = 0, the fallback below passes use_force = false)
static Plan plan_igemm(const IGemmP& p, int batch, size_t ws_bytes, int want_cfg, int mode, bool use_force = true) {
    Plan best{3, 1};
    double best_score = -1.0;
    const int want = (use_force && g_pbe_force_cfg >= 0) ? g_pbe_force_cfg : want_cfg;
    const int forced = (want >= 0 && (want & 255) < kNCfg) ? (want & 255) : -1;
    const int want_splits = want >= 0 ? (want >> 8) & 255 : 0;
    const bool shallow = ((p.K + 63) >> 6) < 10;
    // candidates: the tiles of the problem's form (fp8 operands score the dense tiles and run the f8 column of the pick, below)
    const unsigned forms = mode == 1 ? F_CONV | F_HALO : ex_needed(p) ? F_EX | F_ASTAT : F_DENSE;
    for (int c = 0; c < kNCfg; ++c) {
        if (forced >= 0 && c != forced) continue;
        const TileCfg& t = kTiles[c];
        if (!(t.forms & forms) || ((t.forms & F_FORCED) && forced != c)) continue;
        if ((t.forms & F_ASTAT) && !pbe_astat_ok(p, batch, c)) continue;
        if (p.gn_tab && !gn_tile_ok(p, t)) continue;                         // GroupNorm fold: a streaming tile whose rows lie inside one sample
        if (p.vt && p.vt_col0 % t.bn) continue;                              // extended epilogue: V^T columns start on a tile
        if (p.mx_nr && !mx_tile_ok(p, kTiles[p.sa ? t.f8 : c])) continue;    // MX-fp8 copy-out: the tile that launches keeps every block whole
        if (t.hpa && !halo_rows(p, mode, t.bm, t.hpa)) continue;              // a forced halo tile that does not apply falls back below
        if (t.hpa && p.N % 8) continue;
        const long tm = (p.M + t.bm - 1) / t.bm, tn = (p.N + t.bn - 1) / t.bn;
        const long tiles = tm * tn * batch;
        const int sp = forced >= 0 && want_splits > 0 ? (splitk_ok(p, batch) ? clamp_splits(p, t, ws_bytes, want_splits) : 1)
                                                      : splits_for(p, t, batch, ws_bytes, tiles);
        const double useful = (double)p.M * p.N * batch / ((double)tiles * t.bm * t.bn);
        const double blocks = (double)tiles * sp, slots = 256.0 * t.slots_per_cu;
        const double rounds = (double)((long)((blocks + slots - 1) / slots));
        const double quant = blocks / (rounds * slots);
        const double split_cost = sp > 1 ? 0.93 : 1.0;        // slab write + reduce launch
        const double score = (shallow ? t.eff_shallow : t.eff) * useful * (0.30 + 0.70 * quant) * split_cost;
        if (score > best_score) { best_score = score; best = Plan{c, sp}; }
    }
    if (best_score < 0.0 && forced >= 0)              // the requested tile cannot run this problem: let the heuristic choose
        return plan_igemm(p, batch, ws_bytes, -1, mode, false);
    if (p.sa) best.cfg = kTiles[best.cfg].f8;         // fp8 operands (fill_gemm sets the scales): the tile that launches
    return best;
}

extern int g_pbe_pingpong;      // pbe_tune(4, 0/1): ping-pong main loop of the halo-resident conv tiles
extern int g_pbe_mfast;         // pbe_tune(5, 0/1): let a launch walk its tiles m fastest per XCD when that fetches fewer bytes

// What a launch of tile bm x bn knows before any workgroup starts (p.splits set by the dispatch): the tile order, the halo tile's rows and
// every launch-invariant value of the kernel's prologue (IGemmP head), so that no workgroup divides before its first fetch.
// mode: 0 dense, 1 conv gather, 2 halo-resident conv.
static void igemm_prologue(IGemmP& p, int batch, int bm, int bn, int mode) {
    const int tiles_m = cdiv(p.M, bm), tiles_n = cdiv(p.N, bn);
    {   // bytes the 8 L2s fetch under either tile order (an XCD owns a contiguous run of tiles_m * tiles_n / 8 tiles)
        const double a_bytes = mode != 0 ? 2.0 * (double)(p.M / (p.Ho * p.Wo)) * p.H * p.Wd * (p.C1 + p.C2) : 2.0 * p.M * (double)p.K;
        const double w_bytes = 2.0 * p.N * (double)p.K;
        const double run = tiles_m * (double)tiles_n / 8.0;
        auto frac = [](double blocks_touched, int blocks) { const double f = blocks_touched / blocks; return f < 1.0 ? f : 1.0; };
        const double n_fast = a_bytes * frac(run / tiles_n + 1.0, tiles_m) + w_bytes * frac(run, tiles_n);
        const double m_fast = w_bytes * frac(run / tiles_m + 1.0, tiles_n) + a_bytes * frac(run, tiles_m);
        p.m_fast = (g_pbe_mfast && batch == 1 && m_fast < 0.9 * n_fast) ? 1 : 0;
    }
    p.tdiv = p.m_fast ? tiles_m : tiles_n; p.mg_tdiv = mg_of((unsigned)p.tdiv);
    const int units = mode == 2 ? (p.C1 + p.C2) >> 6 : (p.K + 63) >> 6;            // what split-K slices: channel blocks of a halo tile, else k-tiles
    p.split_per = p.splits > 1 ? (units + p.splits - 1) / p.splits : units;
    p.sv_ns = (p.rowvec && p.group_rows < bm) ? bm / p.group_rows : 1;
    p.sv_gdiv = p.group_rows > bm ? p.group_rows / bm : 1; p.mg_sv_gdiv = mg_of((unsigned)p.sv_gdiv);
    if (mode != 0) {
        const int kb = p.cb >> 6;
        p.hw = p.Ho * p.Wo; p.mg_hw = mg_of((unsigned)p.hw); p.mg_wo = mg_of((unsigned)p.Wo);
        p.per_blk = (p.phase ? 4 : 9) * kb; p.mg_per_blk = mg_of((unsigned)p.per_blk); p.mg_kb = mg_of((unsigned)kb);
    }
    if (mode == 2) {                                                             // halo geometry (igemm_kernel MODE 2; halo_rows admitted the map)
        const int W = p.Wd, th = bm / W < p.H ? bm / W : p.H, img_px = th * W;
        p.th = th;
        p.h_hw2 = W + 1; p.h_hps = (th + 2) * (W + 1) + 1;
        p.h_nsub = bm / img_px; p.h_rows = p.h_nsub * p.h_hps;
        p.h_tpi = p.H / th; p.mg_h_tpi = mg_of((unsigned)p.h_tpi);
        p.mh_hps = mh_of((unsigned)p.h_hps); p.mh_hw2 = mh_of((unsigned)p.h_hw2);
        p.h_lgw = __builtin_ctz((unsigned)W); p.h_lgimg = __builtin_ctz((unsigned)img_px);
    }
}

template <int BM, int BN, int NWM, int NWN, int S, int MODE, int HPA = 0, bool PP = false, bool F8 = false, int EX = 0>
static void launch_cfg(IGemmP p, int batch, hipStream_t s) {
    // (ping-pong only where a wave's MFMA phase - (BM/NWM/16) x (BN/NWN/16) x 2 MFMAs - is as long as its read phase: measured
    //  25 % SLOWER on the 128x160 halo tile, whose 20 MFMAs cannot cover 14 fragment reads + 3 DMA issues)
    if constexpr (MODE == 2 && !PP && S == 3 && (BM / NWM / 16) * (BN / NWN / 16) >= 16) {
        if (g_pbe_pingpong) { launch_cfg<BM, BN, NWM, NWN, S, MODE, HPA, true>(p, batch, s); return; }
    }
    using G = TileGeom<BM, BN, NWM, NWN, MODE, S, HPA, F8, EX>;      // the kernel's LDS layout
    p.sv_ok = !p.rowvec || p.group_rows % BM == 0 || (BM % p.group_rows == 0 && BM / p.group_rows <= G::SVEC_ROWS);
    static std::atomic<uint64_t> attr_done{0};
    pbe_raise_dynamic_lds(attr_done, reinterpret_cast<const void*>(&igemm_kernel<BM, BN, NWM, NWN, MODE, S, HPA, PP, F8, EX>), G::LDS_BYTES + G::GN_MAX_BYTES);
    const int lds_bytes = G::LDS_BYTES + ((EX & EX_GN) ? 8 * p.K : 0);       // EX_GN: + this launch's sc | sh table (K <= PBE_GN_MAX_K)
    if constexpr ((EX & EX_GN) != 0) { p.gn_tdiv /= BM; p.mg_gn_tdiv = mg_of((unsigned)p.gn_tdiv); }      // tokens per sample -> row tiles per sample
    const int tiles_m = cdiv(p.M, BM), tiles_n = cdiv(p.N, BN);
    dim3 grid((unsigned)(tiles_m * tiles_n), batch, p.splits > 1 ? p.splits : 1);
    igemm_prologue(p, batch, BM, BN, MODE);
    {   // GroupNorm statistics from the copy-out: only where the kernel's GS_OK holds and a tile is a whole number of groups inside one sample
        if (p.gstat && !(G::GS_OK && p.splits <= 1 && batch == 1 && p.gs_cg > 0 && p.gs_hw % BM == 0 && BN % p.gs_cg == 0 && !p.phase && p.vec && p.act != PBE_ACT_GEGLU))
            p.gstat = nullptr;
        if (p.gs_report) *p.gs_report = p.gstat ? p.gs_hw / BM : 0;
    }
    // profiling brackets exactly ONE kernel each, so the event averages agree with rocprofv3's per-kernel averages
    pbe_prof_begin(MODE != 0 ? PBE_K_CONV3 : PBE_K_GEMM, s);
    hipLaunchKernelGGL((igemm_kernel<BM, BN, NWM, NWN, MODE, S, HPA, PP, F8, EX>), grid, dim3(NWM * NWN * 64), lds_bytes, s, p);
    {   // algorithmic bytes: every operand once (fp16): activations, weights, output, fused residual
        const double nout = p.act == PBE_ACT_GEGLU ? p.N * 0.5 : (double)p.N;
        const double a_el = MODE != 0 ? (double)(p.M / (p.Ho * p.Wo)) * p.H * p.Wd * (p.C1 + p.C2) : (double)p.M * p.K * batch;
        const double w_el = (double)p.N * p.K * ((MODE == 0 && p.sW) ? batch : 1);
        const double c_el = (double)p.M * nout * batch * (p.resid ? 2.0 : 1.0);
        pbe_prof_end(MODE != 0 ? PBE_K_CONV3 : PBE_K_GEMM, s, 2.0 * p.M * (double)p.N * p.K * batch * (F8 ? 2.0 : 1.0), 2.0 * (a_el + w_el + c_el));
    }
    if (p.splits > 1) {
        const long work = (long)p.M * (p.N >> 2);
        pbe_prof_begin(PBE_K_SPLITK, s);
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, p);
        pbe_prof_end(PBE_K_SPLITK, s, (double)p.M * p.N * (4.0 * p.splits + 2.0));       // bytes: fp32 slabs in, fp16 out
    }
}

// ---- dispatch: launch tile `cfg` of kTiles in one form.  The rows are walked at compile time and launch_cfg is instantiated for the
// rows that carry the form bit only; a tile without it is an error (the planner never picks one) ----
template <unsigned FORM, int MODE, bool F8, int EX, size_t I>
static bool launch_row(IGemmP p, int batch, hipStream_t s) {
    constexpr TileCfg t = kTiles[I];
    if constexpr ((t.forms & FORM) != 0) {
        launch_cfg<t.bm, t.bn, t.nwm, t.nwn, t.s, MODE, t.hpa, false, F8, EX>(p, batch, s);
        return true;
    }
    return false;
}

template <unsigned FORM, int MODE, bool F8, int EX, size_t... I>
static bool launch_rows(int cfg, IGemmP p, int batch, hipStream_t s, std::index_sequence<I...>) {
    return ((cfg == (int)I && launch_row<FORM, MODE, F8, EX, I>(p, batch, s)) || ...);
}

template <unsigned FORM, int MODE, bool F8 = false, int EX = 0>
static int launch_tile(int cfg, IGemmP p, int batch, hipStream_t s) {
    if (launch_rows<FORM, MODE, F8, EX>(cfg, p, batch, s, std::make_index_sequence<kNCfg>{})) return PBE_OK;
    return pbe_set_error(PBE_ENOTSUP, "igemm: tile config %d is not instantiated in form 0x%x", cfg, FORM);
}

// ---- the instantiations live in eleven translation units (igemm_dense / _conv / _halo / _f8 / _ex / _ex_ln / _ex_st / _ex_qkv / _ex_all / _ex_gn / _astat
//      .hip), compiled in parallel ----
int pbe_dispatch_dense(IGemmP p, int batch, hipStream_t s, size_t ws_bytes, int want_cfg);      // MODE 0
int pbe_dispatch_conv(IGemmP p, int batch, hipStream_t s, size_t ws_bytes, int want_cfg);       // MODE 1 gather tiles; forwards F_HALO tiles to
int pbe_launch_halo(int cfg, IGemmP p, int batch, hipStream_t s);                               // MODE 2 halo-resident tiles
int pbe_dispatch_f8(IGemmP p, int batch, hipStream_t s, int want_cfg);
int pbe_dispatch_ex(IGemmP p, int batch, hipStream_t s, int want_cfg);           // picks the feature combination: igemm_ex_{ln,st,qkv,all}.hip
int pbe_launch_ex_ln(int cfg, IGemmP p, int batch, hipStream_t s);
int pbe_launch_ex_st(int cfg, IGemmP p, int batch, hipStream_t s);
int pbe_launch_ex_qkv(int cfg, IGemmP p, int batch, hipStream_t s);
int pbe_launch_ex_all(int cfg, IGemmP p, int batch, hipStream_t s);
int pbe_launch_ex_gn(int cfg, IGemmP p, int batch, hipStream_t s);                                // GroupNorm fold + row statistics (igemm_ex_gn.hip)
void pbe_launch_astat(int cfg, IGemmP p, hipStream_t s);                                                  // tiles 19 / 20 (igemm_astat.hip)
// MX-fp8 copy-out forms (pbe_gemm_mx8out_f16): the q|k|v^T tiles (igemm_ex_qkv.hip, A-stationary tile 20 in igemm_astat.hip) and the fp8 tiles
int pbe_launch_ex_qkv_mx8(int cfg, IGemmP p, int batch, hipStream_t s);
int pbe_launch_f8_mx8(int cfg, IGemmP p, int batch, hipStream_t s);
