// Cross-attention over a SHORT context (2..16 exemplar tokens) folded into one pass over the residual stream, for gfx950
// (wave64, MFMA 32x32x16 f16).  ldm/modules/attention.py:207-230, 268-272 of the reference with everything that depends on the
// context alone precomputed by the host:
//
//   Y[m,:] = X[m,:] + bias + sum_{h, j < Nk} softmax_j( rstd[m] (X[m,:] . Kq[b,(h,j),:] - mean[m] colsum[b,(h,j)]) + kbias[b,(h,j)] ) Vo[b,:,(h,j)]
//
// Kq [B, HJ, C] carries to_q, to_k(context), norm2's gain and scale log2(e); Vo [B, C, HJ] carries to_out and to_v(context); HJ = H Nk
// <= 128.  The head dimension does not appear.  One workgroup = 4 waves = 64 rows of ONE sample (row tiles never straddle samples):
//
//   phase 1  S[64, HJ] = X Kq^T, streamed over C in k-tiles of 64 through LDS (global -> registers -> LDS, the next tile's loads in
//            flight under this tile's MFMAs).  Waves are (row half rw, column half cw): wave (rw, cw) owns rows 32 rw.. and the
//            32-column blocks cw, cw + 2 of S.
//   softmax  S goes to LDS as fp32 (over the staging tiles, which are dead by then); one thread per (row, head) applies the LayerNorm
//            fold, subtracts the group maximum, runs exp2 and writes the weights ONCE as fp16 (padding columns: 0).
//   phase 2  per 32-column tile of C (tiles cw, cw + 2, ..): Y^T = Vo P^T, so the row sits on the lane and 4 consecutive channels in
//            4 accumulator registers: bias + X (re-read, L2-resident) are added, the fp16 result leaves as 8-byte stores and its
//            (sum, sumsq) accumulate per lane for the LayerNorm that reads Y.  P fragments stay in registers for all column tiles.
//
// Rows past the sample's last token are CLAMPED on every read and masked on every write; rows of Kq past HJ are clamped and their
// columns get weight 0; chunks of a Vo row past HJ are zeroed in registers, never trusted (0 * NaN).  Fixed summation order everywhere.
//
// Row-weight form (template RW, pbe_ctx_attention_rw_f16): the weight of context token j depends on the query row too (regional
// exemplars), so log2rw[b, t, j] joins kbias per (row, column) in the softmax stage instead of once per workgroup.  The tile's 64 x Nk
// table entries are fetched into <= 4 registers per thread before phase 1 (their latency hides under it) and parked in an LDS
// array that only this form has (4352 B; the occupancy of 2 is set by the registers, 57344 B fit twice), so the softmax stage stays
// one pass.  The RW = false instantiation is the kernel as it was.
//
// Map form (template AM, pbe_ctx_attention_map_f16): the softmax weights are also a RESULT - the share of cross-attention each context
// token received at each row, averaged over the heads (the attribution map of DESIGN.md section 4.11).  After the barrier that
// completes P the weights are only read, so one thread per (row, token) of the tile, q = row Nk + j < 64 Nk <= 1024 (<= 4 per thread),
// sums the fp16 weights phase 2 multiplies over h = 0 .. H-1 in that order in fp32, multiplies by 1.0f / H and stores the result to
// amap[b am_bs + t am_rs + j], or adds it to what is there: a plain read-modify-write by the one thread that owns the element, no
// atomics, so launches on one stream accumulate deterministically.  No new barrier, no new LDS; rows past the sample's last token
// are not written.  Y and the row statistics keep the bits of the AM = false instantiations, which are the kernel as it was.
#include "common.h"
#include "../../include/pbe_hip.h"

struct CtxP {
    const h16* X; h16* Y; const h16* Kq; const float* colsum; const float* kbias; const h16* Vo; const float* bias;
    const float* ln_stat; float* rstat;
    int C, tokens, H, Nk, HJ, NJ, tps;      // NJ = 32-column blocks of S; tps = row tiles per sample
    long ldx, ldy, kq_bs, kq_rs, vo_bs, vo_rs, cs_bs, ln_ld;
    int ln_parts; float ln_eps; double inv_c;
    const float* log2w; long w_bs;          // pbe_ctx_attention_w_f16: per-(sample, token) log2 weight added to kbias, or null
    const float* log2rw; long rw_bs, rw_rs; // RW form: per-(sample, row, token) log2 weight, element (b, t, j) at b rw_bs + t rw_rs + j
    float* amap; long am_bs, am_rs; int am_acc; // AM form: head-mean softmax weight of (b, t, j) at b am_bs + t am_rs + j, stored or added
};

#define CTX_TM 64          // rows per workgroup
#define CTX_KT 64          // k-tile of phase 1
#define CTX_TS 72          // halfs per staged row (9 16-byte slots, odd: conflict-free ds_read_b128)
#define CTX_SS 129         // floats per row of S (odd: the (row, head) threads of a wave hit 64 different banks)
#define CTX_PS 136         // halfs per row of P (17 slots)
#define CTX_RS 17          // RW form: floats per parked table row (odd: the 64 rows of a wave hit 64 different banks)

template <bool RW, bool AM>
__global__ void __launch_bounds__(256) ctx_attn_kernel(const CtxP p) {
    // [0, 33024): phase 1 staging (X tile 64 x 72, Kq tile 128 x 72 halfs = 27648 B), then S fp32 [64][129]
    __shared__ __attribute__((aligned(16))) unsigned char smem[CTX_TM * CTX_SS * 4 + CTX_TM * CTX_PS * 2];
    __shared__ float s_rstd[CTX_TM], s_nmr[CTX_TM], s_cs[128], s_kb[128];
    __shared__ float2 s_red[2][CTX_TM];
    h16* xs = reinterpret_cast<h16*>(smem);
    h16* ks = xs + CTX_TM * CTX_TS;
    float* S = reinterpret_cast<float*>(smem);
    h16* P = reinterpret_cast<h16*>(smem + CTX_TM * CTX_SS * 4);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h5 = lane >> 5, rw = wave >> 1, cw = wave & 1;
    const int b = blockIdx.x / p.tps, row0 = (blockIdx.x - b * p.tps) * CTX_TM;
    const long mbase = (long)b * p.tokens;
    const int HJ = p.HJ, NJ = p.NJ;
    const h16* Kqb = p.Kq + (long)b * p.kq_bs;
    const h16* Vob = p.Vo + (long)b * p.vo_bs;

    // ---- per-row LayerNorm terms, per-column fold terms ----
    if (tid < CTX_TM) {
        const long m = mbase + min(row0 + tid, p.tokens - 1);
        float a = 0.f, q = 0.f;
        for (int z = 0; z < p.ln_parts; ++z) {               // fixed order: deterministic
            const float2 t = *reinterpret_cast<const float2*>(p.ln_stat + 2 * ((long)z * p.ln_ld + m));
            a += t.x; q += t.y;
        }
        const double mean = (double)a * p.inv_c;             // (only the cancelling subtraction in fp64, as the GEMM's LayerNorm fold)
        const float var = (float)((double)q * p.inv_c - mean * mean);
        const float rstd = __builtin_amdgcn_rsqf(fmaxf(var, 0.f) + p.ln_eps);
        s_rstd[tid] = rstd; s_nmr[tid] = -(float)mean * rstd;
    } else if (tid < CTX_TM + 128) {
        const int c = tid - CTX_TM;
        s_cs[c] = c < HJ ? p.colsum[(long)b * p.cs_bs + c] : 0.f;
        float kb = c < HJ ? p.kbias[(long)b * p.cs_bs + c] : 0.f;
        // exemplar weights: softmax weight ~ w exp(s), i.e. + log2 w in this log2 domain (-inf: token absent), added in fp32 AFTER kbias's
        // own fp16 rounding; column c = (head, token c % Nk).  Done once per workgroup, outside the per-score path.
        if (p.log2w && c < HJ) kb += p.log2w[(long)b * p.w_bs + c % p.Nk];
        s_kb[c] = kb;
    }

    // ---- phase 1: S = X Kq^T ----
    const h16* xsrc[2];
    const h16* ksrc[4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int q = tid + 256 * u, r = q >> 3, c8 = q & 7;
        xsrc[u] = p.X + (mbase + min(row0 + r, p.tokens - 1)) * p.ldx + c8 * 8;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int q = tid + 256 * u, r = q >> 3, c8 = q & 7;
        ksrc[u] = Kqb + (long)min(r, HJ - 1) * p.kq_rs + c8 * 8;
    }
    // RW form: this tile's table entries (row, token) = (q / Nk, q % Nk), q = tid + 256 u < 64 Nk <= 1024; the row is clamped as X's is
    float rwv[4];
    if constexpr (RW) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = tid + 256 * u, r = q / p.Nk, j = q - r * p.Nk;
            rwv[u] = q < CTX_TM * p.Nk ? p.log2rw[(long)b * p.rw_bs + (long)min(row0 + r, p.tokens - 1) * p.rw_rs + j] : 0.f;
        }
    }
    h16x8 xr[2], kr[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) xr[u] = *reinterpret_cast<const h16x8*>(xsrc[u] + k0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u < NJ) kr[u] = *reinterpret_cast<const h16x8*>(ksrc[u] + k0);
    };
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    const int nkt = p.C / CTX_KT;
    fetch(0);
    for (int kt = 0; kt < nkt; ++kt) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int q = tid + 256 * u;
            *reinterpret_cast<h16x8*>(xs + (q >> 3) * CTX_TS + (q & 7) * 8) = xr[u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u < NJ) {
                const int q = tid + 256 * u;
                *reinterpret_cast<h16x8*>(ks + (q >> 3) * CTX_TS + (q & 7) * 8) = kr[u];
            }
        __syncthreads();
        if (kt + 1 < nkt) fetch((kt + 1) * CTX_KT);
#pragma unroll
        for (int s = 0; s < CTX_KT / 16; ++s) {
            const h16x8 a = *reinterpret_cast<const h16x8*>(xs + (rw * 32 + l31) * CTX_TS + s * 16 + 8 * h5);
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (cw + 2 * i < NJ) {
                    const h16x8 w = *reinterpret_cast<const h16x8*>(ks + ((cw + 2 * i) * 32 + l31) * CTX_TS + s * 16 + 8 * h5);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, w, acc[i], 0, 0, 0);
                }
        }
        __syncthreads();                                     // every wave done with the tile before it is overwritten (or S lands on it)
    }
    // accumulator register r of half-wave h5: row (r & 3) + 8 (r >> 2) + 4 h5, column = lane & 31
#pragma unroll
    for (int i = 0; i < 2; ++i)
        if (cw + 2 * i < NJ) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                S[(rw * 32 + (r & 3) + 8 * (r >> 2) + 4 * h5) * CTX_SS + (cw + 2 * i) * 32 + l31] = acc[i][r];
        }
    float* T = nullptr;
    if constexpr (RW) {                                      // park the table in LDS of its own (the discarded branch allocates nothing)
        __shared__ float s_rw[CTX_TM * CTX_RS];
        T = s_rw;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = tid + 256 * u, r = q / p.Nk, j = q - r * p.Nk;
            if (q < CTX_TM * p.Nk) T[r * CTX_RS + j] = rwv[u];
        }
    }
    __syncthreads();

    // ---- LayerNorm fold + grouped softmax (fp32, group maximum subtracted), weights rounded to fp16 once ----
    // RW form: the row's table entry is added to kbias FIRST (fp32), then the same fma chain: a table of zeros gives the plain form's
    // bits, a row-constant table the weighted form's.
    for (int q = tid; q < CTX_TM * p.H; q += 256) {
        const int row = q & (CTX_TM - 1), h = q >> 6;
        float* srow = S + row * CTX_SS + h * p.Nk;
        const float rstd = s_rstd[row], nmr = s_nmr[row];
        float mx = -INFINITY;
        for (int j = 0; j < p.Nk; ++j) {
            float kb = s_kb[h * p.Nk + j];
            if constexpr (RW) kb += T[row * CTX_RS + j];
            const float v = fmaf(rstd, srow[j], fmaf(nmr, s_cs[h * p.Nk + j], kb));
            srow[j] = v;
            mx = fmaxf(mx, v);
        }
        float sum = 0.f;
        for (int j = 0; j < p.Nk; ++j) {
            const float e = fast_exp2(srow[j] - mx);
            srow[j] = e;
            sum += e;
        }
        const float inv = 1.0f / sum;
        h16* prow = P + row * CTX_PS + h * p.Nk;
        for (int j = 0; j < p.Nk; ++j) prow[j] = (h16)(srow[j] * inv);
    }
    {
        const int npad = NJ * 32 - HJ;                       // padding columns: weight 0
        for (int q = tid; q < CTX_TM * npad; q += 256) P[(q & (CTX_TM - 1)) * CTX_PS + HJ + (q >> 6)] = (h16)0.f;
    }
    __syncthreads();

    // ---- phase 2: Y^T = Vo P^T (+ bias + X), row statistics of the stored values ----
    h16x8 pf[8];
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if (s < 2 * NJ) pf[s] = *reinterpret_cast<const h16x8*>(P + (rw * 32 + l31) * CTX_PS + s * 16 + 8 * h5);
    const h16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const int HJ8 = (HJ + 7) & ~7;
    auto load_vo = [&](h16x8 (&vf)[8], int c0) {             // A fragment: lane = channel c0 + (lane & 31), k = 16 s + 8 h5 + 0..7
        const h16* src = Vob + (long)(c0 + l31) * p.vo_rs + 8 * h5;
#pragma unroll
        for (int s = 0; s < 8; ++s)
            if (s < 2 * NJ) {
                const int k0 = s * 16 + 8 * h5;
                h16x8 v = zero8;
                if (k0 < HJ8) {
                    v = *reinterpret_cast<const h16x8*>(src + s * 16);
                    if (k0 + 8 > HJ) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = (k0 + e < HJ) ? v[e] : (h16)0.f;
                    }
                }
                vf[s] = v;
            }
    };
    const int lrow = rw * 32 + l31;                          // this lane's row of the tile
    const bool row_ok = row0 + lrow < p.tokens;
    const long m = mbase + min(row0 + lrow, p.tokens - 1);
    const h16* xrow = p.X + m * p.ldx;
    h16* yrow = p.Y + m * p.ldy;
    float rsum = 0.f, rsq = 0.f;
    const int nct = p.C / 32;
    h16x8 vf[8];
    if (cw < nct) load_vo(vf, cw * 32);
    if constexpr (AM) {                                      // P is complete and only read from here on: the map rides beside phase 2
#pragma clang fp contract(off)                               // (the product is rounded before the add: accumulate = base + stored, bit for bit)
        const float inv_h = 1.0f / (float)p.H;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = tid + 256 * u, r = q / p.Nk, j = q - r * p.Nk;
            if (q < CTX_TM * p.Nk && row0 + r < p.tokens) {
                const h16* pr = P + r * CTX_PS + j;
                float a = 0.f;
                for (int h = 0; h < p.H; ++h) a += (float)pr[h * p.Nk];   // fixed order: the fp16 weights phase 2 multiplies
                a *= inv_h;
                float* dst = p.amap + (long)b * p.am_bs + (long)(row0 + r) * p.am_rs + j;
                *dst = p.am_acc ? *dst + a : a;
            }
        }
    }
    for (int ct = cw; ct < nct; ct += 2) {
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 8; ++s)
            if (s < 2 * NJ) o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[s], pf[s], o, 0, 0, 0);
        if (ct + 2 < nct) load_vo(vf, (ct + 2) * 32);        // next tile's fragments in flight under this tile's epilogue
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = ct * 32 + 8 * g + 4 * h5;          // registers 4 g .. 4 g + 3: channels c .. c + 3
            const h16x4 xv = *reinterpret_cast<const h16x4*>(xrow + c);
            h16x4 yv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const h16 y = (h16)(o[4 * g + r] + p.bias[c + r] + (float)xv[r]);
                const float f = (float)y;
                rsum += f; rsq = fmaf(f, f, rsq);
                yv[r] = y;
            }
            if (row_ok) *reinterpret_cast<h16x4*>(yrow + c) = yv;
        }
    }
    if (p.rstat) {                                           // (sum, sumsq) of the stored fp16 row: half-waves, then the two column waves
        rsum += __shfl_xor(rsum, 32, 64);
        rsq += __shfl_xor(rsq, 32, 64);
        if (h5 == 0) s_red[cw][lrow] = make_float2(rsum, rsq);
        __syncthreads();
        if (tid < CTX_TM && row0 + tid < p.tokens) {
            const float2 a = s_red[0][tid], c = s_red[1][tid];
            *reinterpret_cast<float2*>(p.rstat + 2 * (mbase + row0 + tid)) = make_float2(a.x + c.x, a.y + c.y);
        }
    }
}

extern "C" size_t pbe_sizeof_ctx_attn_desc(void) { return sizeof(pbe_ctx_attn_desc); }

static int ctx_attention_launch(const pbe_ctx_attn_desc* d, const float* log2w, int64_t w_bs, const float* log2rw, int64_t rw_bs, int64_t rw_rs,
                                pbe_stream_t stream, float* amap = nullptr, int64_t am_bs = 0, int64_t am_rs = 0, int accumulate = 0) {
    PBE_REQUIRE(d && d->X && d->Y && d->Kq && d->colsum && d->kbias && d->Vo && d->bias && d->ln_stats, "pbe_ctx_attention_f16: null operand");
    PBE_REQUIRE(d->C % 64 == 0 && d->C >= 64 && d->C <= 1280, "pbe_ctx_attention_f16: C = %d unsupported (multiple of 64, 64..1280)", d->C);
    PBE_REQUIRE(d->Nk >= 1 && d->Nk <= 16, "pbe_ctx_attention_f16: Nk = %d unsupported (1..16 context tokens)", d->Nk);
    PBE_REQUIRE(d->H >= 1 && (long)d->H * d->Nk <= 128, "pbe_ctx_attention_f16: H * Nk = %ld unsupported (<= 128)", (long)d->H * d->Nk);
    PBE_REQUIRE(d->M > 0 && d->tokens >= 1 && d->M % d->tokens == 0, "pbe_ctx_attention_f16: M = %d must be whole samples of %d tokens", d->M, d->tokens);
    const int HJ = d->H * d->Nk;
    PBE_REQUIRE(d->ldx >= d->C && d->ldy >= d->C && d->ldx % 8 == 0 && d->ldy % 8 == 0, "pbe_ctx_attention_f16: ldx / ldy must cover C and be multiples of 8");
    PBE_REQUIRE(d->kq_rs >= d->C && d->kq_rs % 8 == 0 && d->kq_bs % 8 == 0 && d->kq_bs >= 0, "pbe_ctx_attention_f16: Kq strides (rows of >= C, multiples of 8)");
    PBE_REQUIRE(d->vo_rs >= (HJ + 7) / 8 * 8 && d->vo_rs % 8 == 0 && d->vo_bs % 8 == 0 && d->vo_bs >= 0,
                "pbe_ctx_attention_f16: Vo strides (rows of >= H * Nk rounded up to 8, multiples of 8)");
    PBE_REQUIRE(d->cs_bs >= 0, "pbe_ctx_attention_f16: colsum / kbias batch stride");
    PBE_REQUIRE(d->ln_parts >= 1 && d->ln_stats_ld >= d->M, "pbe_ctx_attention_f16: row statistics need ln_parts >= 1 and ln_stats_ld >= M");
    PBE_REQUIRE(((uintptr_t)d->X & 15) == 0 && ((uintptr_t)d->Y & 15) == 0 && ((uintptr_t)d->Kq & 15) == 0 && ((uintptr_t)d->Vo & 15) == 0 &&
                ((uintptr_t)d->ln_stats & 7) == 0 && ((uintptr_t)d->row_stats_out & 7) == 0, "pbe_ctx_attention_f16: alignment (16 bytes; statistics 8)");
    const int B = d->M / d->tokens, tps = cdiv(d->tokens, CTX_TM);
    PBE_REQUIRE((long)B * tps < (1L << 31), "pbe_ctx_attention_f16: too many workgroups");
    CtxP p;
    p.X = (const h16*)d->X; p.Y = (h16*)d->Y; p.Kq = (const h16*)d->Kq; p.colsum = d->colsum; p.kbias = d->kbias; p.Vo = (const h16*)d->Vo;
    p.bias = d->bias; p.ln_stat = d->ln_stats; p.rstat = d->row_stats_out;
    p.C = d->C; p.tokens = d->tokens; p.H = d->H; p.Nk = d->Nk; p.HJ = HJ; p.NJ = (HJ + 31) / 32; p.tps = tps;
    p.ldx = d->ldx; p.ldy = d->ldy; p.kq_bs = d->kq_bs; p.kq_rs = d->kq_rs; p.vo_bs = d->vo_bs; p.vo_rs = d->vo_rs; p.cs_bs = d->cs_bs;
    p.ln_ld = d->ln_stats_ld; p.ln_parts = d->ln_parts; p.ln_eps = d->ln_eps; p.inv_c = 1.0 / (double)d->C;
    p.log2w = log2w; p.w_bs = w_bs; p.log2rw = log2rw; p.rw_bs = rw_bs; p.rw_rs = rw_rs;
    p.amap = amap; p.am_bs = am_bs; p.am_rs = am_rs; p.am_acc = accumulate ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    pbe_prof_begin(PBE_K_CTXATTN, s);
    const dim3 grid((unsigned)(B * tps));
    if (amap) {
        if (log2rw) hipLaunchKernelGGL((ctx_attn_kernel<true, true>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((ctx_attn_kernel<false, true>), grid, dim3(256), 0, s, p);
    } else if (log2rw) hipLaunchKernelGGL((ctx_attn_kernel<true, false>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((ctx_attn_kernel<false, false>), grid, dim3(256), 0, s, p);
    // a class of its own, accounted in bytes like the norms (memory-bound: 4 HJ FLOP per byte of X at most): X twice (the 2nd from L2 at
    // best), Y, Kq, Vo
    pbe_prof_end(PBE_K_CTXATTN, s, 2.0 * (3.0 * (double)d->M * d->C + 2.0 * (double)B * HJ * d->C));
    PBE_LAUNCH_CHECK("pbe_ctx_attention_f16");
    return PBE_OK;
}

extern "C" int pbe_ctx_attention_f16(const pbe_ctx_attn_desc* d, pbe_stream_t stream) { return ctx_attention_launch(d, nullptr, 0, nullptr, 0, 0, stream); }

// The same launch with exemplar weights: log2w [B, Nk] fp32 (element (b, j) at log2w[b * w_bs + j]) holds log2 of token j's
// non-negative weight, -inf for weight 0.  At least one token per sample must be present (the caller validates the weights).
extern "C" int pbe_ctx_attention_w_f16(const pbe_ctx_attn_desc* d, const float* log2w, int64_t w_bs, pbe_stream_t stream) {
    PBE_REQUIRE(log2w && ((uintptr_t)log2w & 3) == 0 && w_bs >= 0, "pbe_ctx_attention_w_f16: log2w must be a 4-byte aligned pointer, w_bs >= 0");
    return ctx_attention_launch(d, log2w, w_bs, nullptr, 0, 0, stream);
}

// The same launch with a weight per (sample, query row, token): log2rw fp32, element (b, t, j) at log2rw[b * rw_bs + t * rw_rs + j] for
// t < tokens, j < Nk, holds log2 of the effective weight of token j at row t (-inf: absent there; the exemplar weights are already
// multiplied in).  Every row must keep one token of positive weight (the caller's fallback rule sees to it).  The entry is added to
// kbias in fp32 before the LayerNorm fold's fma chain: zeros give the bits of pbe_ctx_attention_f16, log2 w[b, j] on every row those
// of pbe_ctx_attention_w_f16.  Nothing past row tokens - 1 of a sample's table or past column Nk - 1 is read.
extern "C" int pbe_ctx_attention_rw_f16(const pbe_ctx_attn_desc* d, const float* log2rw, int64_t rw_bs, int64_t rw_rs, pbe_stream_t stream) {
    PBE_REQUIRE(log2rw && ((uintptr_t)log2rw & 3) == 0, "pbe_ctx_attention_rw_f16: log2rw must be a 4-byte aligned pointer");
    PBE_REQUIRE(d && rw_rs >= d->Nk && rw_bs >= 0, "pbe_ctx_attention_rw_f16: rw_rs must cover Nk, rw_bs >= 0");
    return ctx_attention_launch(d, nullptr, 0, log2rw, rw_bs, rw_rs, stream);
}

// Any of the three launches above with the attribution map as a side output: amap fp32, element (b, t, j) at amap[b * am_bs + t * am_rs + j]
// for t < tokens, j < Nk, takes (accumulate = 0) or is increased by (accumulate != 0) the mean over the heads of the fp16 softmax
// weights of token j at row t.  log2w / log2rw as in the _w / _rw entries, or NULL; not both.  Y and row_stats_out are those of the
// entry without the map, bit for bit.  Nothing outside t < tokens, j < Nk of a sample's map is touched.
extern "C" int pbe_ctx_attention_map_f16(const pbe_ctx_attn_desc* d, const float* log2w, int64_t w_bs, const float* log2rw, int64_t rw_bs,
                                         int64_t rw_rs, float* amap, int64_t am_bs, int64_t am_rs, int32_t accumulate, pbe_stream_t stream) {
    PBE_REQUIRE(!(log2w && log2rw), "pbe_ctx_attention_map_f16: log2rw replaces log2w: give one of them");
    PBE_REQUIRE(!log2w || (((uintptr_t)log2w & 3) == 0 && w_bs >= 0), "pbe_ctx_attention_map_f16: log2w must be 4-byte aligned, w_bs >= 0");
    PBE_REQUIRE(!log2rw || (((uintptr_t)log2rw & 3) == 0 && d && rw_rs >= d->Nk && rw_bs >= 0),
                "pbe_ctx_attention_map_f16: log2rw must be 4-byte aligned, rw_rs must cover Nk, rw_bs >= 0");
    PBE_REQUIRE(amap && ((uintptr_t)amap & 3) == 0, "pbe_ctx_attention_map_f16: amap must be a 4-byte aligned pointer");
    PBE_REQUIRE(d && am_rs >= d->Nk && am_bs >= 0, "pbe_ctx_attention_map_f16: am_rs must cover Nk, am_bs >= 0");
    return ctx_attention_launch(d, log2w, w_bs, log2rw, rw_bs, rw_rs, stream, amap, am_bs, am_rs, accumulate);
}
