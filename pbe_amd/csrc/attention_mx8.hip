// MX-fp8 attention core, softmax(Q K^T) V with OCP e4m3 operands and one E8M0 (power-of-two) scale per 32 contraction elements,
// for gfx950: both products run v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3, fp32 accumulate, the block scales applied inside
// the matrix core).  The structure is attention.hip's: transposed scores S^T = K Q^T (query on the lane), K / V^T tiles of 64 keys
// staged global -> LDS by LDS-DMA, P kept in registers as the B operand of O^T = V^T P^T, the deferred reference maximum, the
// XCD head map and the softmax denominator from a ones row of V^T.
//
// Operand map of the 32x32x64 e4m3 MFMA (pinned with exact integer data, tests/test_attention_mx8_gpu.py): lane l (r = l & 31,
// h = l >> 5) holds 32 bytes; byte j is contraction index k = 32 (j >> 4) + 16 h + (j & 15) of row r (A) / column r (B), the same
// map for A and B.  The scale VGPR of lane (r, h) (byte 0, op_sel 0) scales k-block h = k >> 5 of that row / column, i.e. the
// FIRST 16 bytes of both half-waves share the scale of half-wave 0, the last 16 bytes that of half-wave 1.
// So a fragment is two 16-byte pieces, bytes [32c + 16h, 32c + 16h + 16) of a row, c = 0, 1.
//
// P as the B operand: register i of the S^T accumulator of 32-key sub-tile s holds K-tile row 4h + (i & 3) + 8 (i >> 2) of that
// sub-tile.  The K tile is staged with rows permuted so that this register is key 32 s + 16 h + i: then the 16 registers of sub-tile
// s are B bytes 16 s .. 16 s + 15 of the lane, i.e. keys 32 s + 16 h + (0..15) in natural order, each 32-key half of the tile is one
// V^T scale block, and the V^T fragment is read in natural key order.
//
// Operand layouts (what pbe_quant_mx8_f16 writes, include/pbe_hip.h):
//   tokens form (Q, K): bytes [B*N][H*DP], DP = D rounded up to 64 (zero padding); scales [B][H][DP/32][NP], NP = N rounded up to 64.
//   V^T form:           bytes [B*H*D][NP] (zero padding past N);            scales [B][H][NP/32][DV], DV = 32 (D / 32 + 1).
// Every staged piece is a whole 16-byte LDS-DMA slot; the scale pads are E8M0 1.0 (127), so the ones row of V^T (row DV - 1, never a
// DMA target) is scaled by 1.
#include "common.h"
#include "../../include/pbe_hip.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// ---- quantiser ---------------------------------------------------------------------------------------------------------------
// (mx8_e4m3 / mx8_scale_exp live in common.h: the GEMM epilogue's MX-fp8 copy-out uses the same code)

struct QuantP {
    const h16* X; unsigned char* Y; unsigned char* S;
    int mode, B, H, N, D;
    long rs;
    float alpha;
    int R, NB, DP, NP, DV;      // scale rows per block column, blocks per row, padded head / token lengths
};

// one thread = one (b, h, block, row) 32-element block; row is the fastest index (scale bytes are written contiguously)
__global__ void __launch_bounds__(256) quant_mx8_kernel(const QuantP p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;      // (32-bit index arithmetic: the host checks the total)
    if (idx >= p.B * p.H * p.NB * p.R) return;
    const int r = idx % p.R;
    int t = idx / p.R;
    const int blk = t % p.NB; t /= p.NB;
    const int h = t % p.H;
    const int b = t / p.H;
    const h16* src = nullptr;
    unsigned char* dst = nullptr;
    int cnt = 0;
    if (p.mode == 0) {                                   // tokens: row = token n, contraction = channel d of head h
        if (r < p.N) {
            src = p.X + ((long)b * p.N + r) * p.rs + (long)h * p.D + 32 * blk;
            dst = p.Y + ((long)b * p.N + r) * ((long)p.H * p.DP) + (long)h * p.DP + 32 * blk;
            cnt = min(max(p.D - 32 * blk, 0), 32);
        }
    } else {                                             // V^T: row = channel d of head h, contraction = token n
        if (r < p.D) {
            src = p.X + ((long)(b * p.H + h) * p.D + r) * p.rs + 32 * blk;
            dst = p.Y + ((long)(b * p.H + h) * p.D + r) * p.NP + 32 * blk;
            cnt = min(max(p.N - 32 * blk, 0), 32);
        }
    }
    float v[32];
    float amax = 0.f;
    if (cnt == 32) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const h16x8 x = *reinterpret_cast<const h16x8*>(src + 8 * c);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[8 * c + e] = (float)x[e] * p.alpha;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 32; ++e) v[e] = e < cnt ? (float)src[e] * p.alpha : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 32; ++e) amax = fmaxf(amax, fabsf(v[e]));
    const int se = mx8_scale_exp(amax);
    if (dst) {
        const float inv = __uint_as_float((unsigned)(254 - se) << 23);                      // 1 / 2^(se - 127), exact
        i32x4 w[2];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            unsigned word = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) word |= mx8_e4m3(v[4 * q + e] * inv) << (8 * e);
            w[q >> 2][q & 3] = (int)word;
        }
        *reinterpret_cast<i32x4*>(dst) = w[0];
        *reinterpret_cast<i32x4*>(dst + 16) = w[1];
    }
    p.S[idx] = (unsigned char)se;
}

extern "C" int pbe_quant_mx8_f16(const void* X, void* Y, void* S, int32_t mode, int32_t B, int32_t H, int32_t N, int32_t D, int64_t rs,
                                 float alpha, pbe_stream_t stream) {
    PBE_REQUIRE(X && Y && S, "pbe_quant_mx8_f16: null operand");
    PBE_REQUIRE(mode == PBE_MX8_TOKENS || mode == PBE_MX8_VT, "pbe_quant_mx8_f16: mode %d unknown", mode);
    PBE_REQUIRE(B > 0 && H > 0 && N > 0 && D > 0 && D % 8 == 0, "pbe_quant_mx8_f16: bad dims (D %% 8 == 0)");
    PBE_REQUIRE(rs % 8 == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)Y & 15) == 0, "pbe_quant_mx8_f16: 16-byte alignment (rs %% 8 == 0)");
    PBE_REQUIRE(mode == PBE_MX8_VT || rs >= (int64_t)H * D, "pbe_quant_mx8_f16: rs < H * D");
    PBE_REQUIRE(mode == PBE_MX8_TOKENS || rs >= (N + 7) / 8 * 8, "pbe_quant_mx8_f16: rs must cover N rounded up to 8");
    QuantP p;
    p.X = (const h16*)X; p.Y = (unsigned char*)Y; p.S = (unsigned char*)S;
    p.mode = mode; p.B = B; p.H = H; p.N = N; p.D = D; p.rs = rs; p.alpha = alpha;
    p.DP = (D + 63) / 64 * 64; p.NP = (N + 63) / 64 * 64; p.DV = (D / 32 + 1) * 32;
    p.NB = mode == PBE_MX8_TOKENS ? p.DP / 32 : p.NP / 32;
    p.R = mode == PBE_MX8_TOKENS ? p.NP : p.DV;
    const long total = (long)B * H * p.NB * p.R;
    PBE_REQUIRE(total < (1L << 31), "pbe_quant_mx8_f16: too many blocks");
    hipStream_t s = (hipStream_t)stream;
    pbe_prof_begin(PBE_K_ELEM, s);
    hipLaunchKernelGGL(quant_mx8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
    pbe_prof_end(PBE_K_ELEM, s, (double)total * 98.0);                                      // 64 B in, 32 B + 1 out, ~1 B pad traffic per block
    PBE_LAUNCH_CHECK("pbe_quant_mx8_f16");
    return PBE_OK;
}

// ---- attention ---------------------------------------------------------------------------------------------------------------
struct AttnMx8P {
    const unsigned char *Q, *Qs, *K, *Ks, *V, *Vs;
    h16* O;
    int B, H, Nq, Nk, D;
    long o_bs, o_rs;
    float scale_log2e;
    int nqb;
};

#define PBE_GLDS16(gsrc, ldst)                                                                     \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc),         \
                                     (__attribute__((address_space(3))) void*)(ldst), 16, 0, 0)

template <int DP>
struct Mx8Tile {
    static constexpr int KT = 64;                       // keys per staged tile
    static constexpr int DV = (DP == 64 ? 40 : DP == 128 ? 80 : 160) / 32 * 32 + 32;   // V^T rows: the head dim + a ones row
    static constexpr int NB = DP / 32;                  // scale blocks per K row
    static constexpr int KR = DP / 16 | 1;              // 16-B slots per K row (odd: conflict-free ds_read_b128)
    static constexpr int VR = KT / 16 | 1;              // slots per V^T row
    static constexpr int KSTR = KR * 16, VSTR = VR * 16;
    static constexpr int KSLOTS = KT * KR, VSLOTS = DV * VR, KSSLOTS = NB * 4, VSSLOTS = 2 * DV / 16;
    static constexpr int VOFF = KSLOTS * 16, KSOFF = VOFF + VSLOTS * 16, VSOFF = KSOFF + KSSLOTS * 16;
    static constexpr int SLOTS = KSLOTS + VSLOTS + KSSLOTS + VSSLOTS;
    static constexpr int NI = (SLOTS + 63) / 64;        // LDS-DMA instructions (64 slots each) per tile
    static constexpr int NPW = (NI + 3) / 4;            // ... per wave
    static constexpr int BUF = NI * 1024;
};

// key held by row R of the K tile (see the header): sub-tile s = R >> 5, accumulator row rho = R & 31 -> key 32 s + 16 h + i with
// h = (rho >> 2) & 1 and register i = (rho & 3) + 4 (rho >> 3)
__device__ __forceinline__ int mx8_key_of_row(int R) {
    const int rho = R & 31;
    return (R & 32) + 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3);
}

#define MX8_THR 8.0f         // deferred maximum: P = exp2(s - m) <= 2^8, inside e4m3's range (448) at scale 1

template <int DP>
__global__ void __launch_bounds__(256, 1) attn_mx8_kernel(const AttnMx8P p) {
    using T = Mx8Tile<DP>;
    constexpr int KT = T::KT, DV = T::DV, NB = T::NB, KSTR = T::KSTR, VSTR = T::VSTR, KR = T::KR, VR = T::VR;
    constexpr int KSLOTS = T::KSLOTS, VSLOTS = T::VSLOTS, KSSLOTS = T::KSSLOTS, SLOTS = T::SLOTS, NPW = T::NPW, BUF = T::BUF;
    constexpr int NDS = DP / 64;          // k-steps of QK^T
    constexpr int NDT = DV / 32;          // 32-row d tiles of O^T
    constexpr bool PREFV = NDT <= 3;      // V^T fragments fetched under the softmax (else just before their MFMA)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h5 = lane >> 5;
    int bh, qblk;
    {   // the query blocks of one (batch, head) on one XCD (attention.hip): its L2 serves the repeated K / V^T sweeps
        const int nq = p.nqb, nbh = p.B * p.H, lin = blockIdx.x;
        if ((nbh & 7) == 0) { const int xcd = lin & 7, j = lin >> 3; qblk = j % nq; bh = (j / nq) * 8 + xcd; }
        else { qblk = lin % nq; bh = lin / nq; }
    }
    const int b = bh / p.H, h = bh - b * p.H;
    const int q = qblk * 128 + wave * 32 + l31;
    const int D = p.D;
    const long HDP = (long)p.H * DP;
    const int NPq = (p.Nq + 63) / 64 * 64, NPk = (p.Nk + 63) / 64 * 64;
    const unsigned char* Kb = p.K + (long)b * p.Nk * HDP + (long)h * DP;
    const unsigned char* Ksb = p.Ks + (long)bh * NB * NPk;
    const unsigned char* Vb = p.V + (long)bh * D * NPk;
    const unsigned char* Vsb = p.Vs + (long)bh * (NPk / 32) * DV;

    // ---- LDS init: zero every tile image (pads, V^T rows D .. DV-2), then the ones row DV-1 (e4m3 1.0 = 0x38) ----
    const i32x4 zero4 = {0, 0, 0, 0};
    for (int i = tid; i < 2 * BUF / 16; i += 256) *reinterpret_cast<i32x4*>(smem + i * 16) = zero4;
    __syncthreads();
    if (tid < 2 * 4) {
        const i32x4 one4 = {0x38383838, 0x38383838, 0x38383838, 0x38383838};
        *reinterpret_cast<i32x4*>(smem + (tid >> 2) * BUF + T::VOFF + (DV - 1) * VSTR + (tid & 3) * 16) = one4;
    }

    // ---- per-lane DMA sources, advanced by a constant per tile ----
    const unsigned char* src[NPW];
    long inc[NPW];
#pragma unroll
    for (int j = 0; j < NPW; ++j) {
        const int slot = (j * 4 + wave) * 64 + lane;
        src[j] = nullptr; inc[j] = 0;
        if (slot < KSLOTS) {
            const int row = slot / KR, c = slot - row * KR;
            if (c < DP / 16) { src[j] = Kb + (long)mx8_key_of_row(row) * HDP + c * 16; inc[j] = KT * HDP; }
        } else if (slot < KSLOTS + VSLOTS) {
            const int sv = slot - KSLOTS, row = sv / VR, c = sv - row * VR;
            if (c < KT / 16 && row < D) { src[j] = Vb + (long)row * NPk + c * 16; inc[j] = KT; }
        } else if (slot < KSLOTS + VSLOTS + KSSLOTS) {
            const int s = slot - KSLOTS - VSLOTS;           // block s >> 2, 16 keys (s & 3)
            src[j] = Ksb + (long)(s >> 2) * NPk + (s & 3) * 16; inc[j] = KT;
        } else if (slot < SLOTS) {
            const int s = slot - KSLOTS - VSLOTS - KSSLOTS;  // 2 key blocks x DV bytes
            src[j] = Vsb + s * 16; inc[j] = 2 * DV;
        }
    }
    const int nt = (p.Nk + KT - 1) / KT;
    const bool ragged = p.Nk % KT != 0;
    auto issue_tile = [&](int t, int buf) {
        unsigned char* dst = smem + buf * BUF + wave * 1024;
        if (t + 1 < nt || !ragged) {
#pragma unroll
            for (int j = 0; j < NPW; ++j) {
                if (src[j]) PBE_GLDS16(src[j], dst + j * 4096);
                src[j] += inc[j];
            }
        } else {                                          // ragged last tile: K rows past Nk re-read key Nk - 1 (their scores are masked)
#pragma unroll
            for (int j = 0; j < NPW; ++j) {
                const int slot = (j * 4 + wave) * 64 + lane;
                const unsigned char* s = src[j];
                if (slot < KSLOTS && s) {
                    const int row = slot / KR, c = slot - row * KR;
                    s = Kb + (long)min(t * KT + mx8_key_of_row(row), p.Nk - 1) * HDP + c * 16;
                }
                if (s) PBE_GLDS16(s, dst + j * 4096);
            }
        }
    };

    // Q fragments (B operand of S^T = K Q^T) and their scales: loaded once
    i32x8 qf[NDS];
    int qs[NDS];
    {
        const bool ok = q < p.Nq;
        const unsigned char* qrow = p.Q + ((long)b * p.Nq + (ok ? q : 0)) * HDP + (long)h * DP;
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds) {
            const i32x4 lo = *reinterpret_cast<const i32x4*>(qrow + 64 * ds + 16 * h5);
            const i32x4 hi = *reinterpret_cast<const i32x4*>(qrow + 64 * ds + 32 + 16 * h5);
#pragma unroll
            for (int w = 0; w < 4; ++w) { qf[ds][w] = ok ? lo[w] : 0; qf[ds][4 + w] = ok ? hi[w] : 0; }
            qs[ds] = ok ? (int)p.Qs[((long)bh * NB + 2 * ds + h5) * NPq + q] : 127;
        }
    }
    const int krow0 = mx8_key_of_row(l31), krow1 = mx8_key_of_row(32 + l31);   // keys of this lane's two A rows (scale lookup)

    f32x16 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY;

    __syncthreads();                                      // init stores done before any DMA lands on them
    issue_tile(0, 0);
    __syncthreads();

    f32x16 sc[2];
    i32x8 kf[2][NDS];
    int ks[2][NDS];
    i32x8 vf[PREFV ? NDT : 1];
    int vs[NDT];
    auto frag = [&](const unsigned char* row) {           // bytes [16h, 16h+16) and [32+16h, ..) of a 64-byte k-step
        const i32x4 lo = *reinterpret_cast<const i32x4*>(row + 16 * h5);
        const i32x4 hi = *reinterpret_cast<const i32x4*>(row + 32 + 16 * h5);
        i32x8 f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { f[w] = lo[w]; f[4 + w] = hi[w]; }
        return f;
    };
    auto load_k = [&](const unsigned char* sk) {
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds) {
            kf[0][ds] = frag(sk + l31 * KSTR + 64 * ds);
            kf[1][ds] = frag(sk + (32 + l31) * KSTR + 64 * ds);
            ks[0][ds] = sk[T::KSOFF + (2 * ds + h5) * 64 + krow0];
            ks[1][ds] = sk[T::KSOFF + (2 * ds + h5) * 64 + krow1];
        }
    };
    auto load_v = [&](const unsigned char* sk) {
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            if constexpr (PREFV) vf[dt] = frag(sk + T::VOFF + (dt * 32 + l31) * VSTR);
            vs[dt] = sk[T::VSOFF + h5 * DV + dt * 32 + l31];
        }
    };

    auto tile = [&](int t, const unsigned char* sk) {
        const int kv0 = t * KT;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[s][r] = 0.f;
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds) {
            sc[0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf[0][ds], qf[ds], sc[0], 0, 0, 0, ks[0][ds], 0, qs[ds]);
            sc[1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf[1][ds], qf[ds], sc[1], 0, 0, 0, ks[1][ds], 0, qs[ds]);
        }
        load_v(sk);                                       // in flight under the softmax
        __builtin_amdgcn_sched_barrier(0);
        // ---- online softmax over this lane's 32 keys (register i of sub-tile s = key kv0 + 32 s + 16 h + i) ----
        if (kv0 + KT > p.Nk) {
            int left = p.Nk - kv0 - 16 * h5;
            asm volatile("" : "+v"(left));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sc[0][r] = (r >= left) ? -INFINITY : sc[0][r];
                sc[1][r] = (r + 32 >= left) ? -INFINITY : sc[1][r];
            }
        }
        float mx = fmaxf(sc[0][0], sc[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(fmaxf(mx, sc[0][r]), sc[1][r]);
        {
            typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
            const unsigned int u = __builtin_bit_cast(unsigned int, mx);
            const u32x2 rr = __builtin_amdgcn_permlane32_swap(u, u, false, false);
            unsigned int r0 = rr[0], r1 = rr[1];
            asm volatile("" : "+v"(r0), "+v"(r1));        // (see attention.hip: the two results must not be folded)
            mx = fmaxf(__builtin_bit_cast(float, r0), __builtin_bit_cast(float, r1));
        }
        const float ms = mx * p.scale_log2e;
        if (__builtin_amdgcn_ballot_w64(ms - m_run > MX8_THR) != 0) {       // (first tile: m_run = -inf)
            const float m_new = fmaxf(m_run, ms);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
        }
        const float neg_m = -m_run;
        i32x8 pb;                                         // P^T as e4m3 bytes: word w = registers 4w .. 4w+3 (s = w >> 2)
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const f32x16& x = sc[w >> 2];
            const int r = 4 * (w & 3);
            const float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(x[r], p.scale_log2e, neg_m));
            const float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(x[r + 1], p.scale_log2e, neg_m));
            const float p2 = __builtin_amdgcn_exp2f(__builtin_fmaf(x[r + 2], p.scale_log2e, neg_m));
            const float p3 = __builtin_amdgcn_exp2f(__builtin_fmaf(x[r + 3], p.scale_log2e, neg_m));
            int v = __builtin_amdgcn_cvt_pk_fp8_f32(p0, p1, 0, false);
            pb[w] = __builtin_amdgcn_cvt_pk_fp8_f32(p2, p3, v, true);
        }
        // ---- O^T += V^T P^T (the ones row DV-1 accumulates the denominator from the same rounded P) ----
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            i32x8 a;
            if constexpr (PREFV) a = vf[dt];
            else a = frag(sk + T::VOFF + (dt * 32 + l31) * VSTR);
            o[dt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, pb, o[dt], 0, 0, 0, vs[dt], 0, 127);
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    load_k(smem);
    for (int t = 0; t < nt; ++t) {
        if (t + 1 < nt) issue_tile(t + 1, (t + 1) & 1);
        tile(t, smem + (t & 1) * BUF);
        __syncthreads();                                  // all waves done with tile t; (vmcnt drained) tile t+1 landed
        if (t + 1 < nt) load_k(smem + ((t + 1) & 1) * BUF);
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- normalise and store O[q, h*D + d] ----
    const float mine = o[NDT - 1][15];                    // O^T row DV-1 (the denominator) lives in register 15 of the upper half-wave
    const float other = __shfl_xor(mine, 32, 64);
    const float inv = 1.0f / (h5 ? mine : other);
    if (q < p.Nq) {
        h16* Ob = p.O + (long)b * p.o_bs + (long)q * p.o_rs + (long)h * D;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d0 = dt * 32 + 8 * g + 4 * h5;
                if (d0 < D) {
                    h16x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = (h16)(o[dt][4 * g + r] * inv);
                    *reinterpret_cast<h16x4*>(Ob + d0) = v;
                }
            }
    }
}

template <int DP>
static void launch_attn_mx8(const AttnMx8P& p, hipStream_t s) {
    constexpr size_t lds = 2 * Mx8Tile<DP>::BUF;
    static_assert(lds <= 160 * 1024, "attention tile exceeds the LDS");
    static std::atomic<uint64_t> attr_done{0};
    pbe_raise_dynamic_lds(attr_done, reinterpret_cast<const void*>(&attn_mx8_kernel<DP>), 160 * 1024);
    AttnMx8P q = p;
    q.nqb = cdiv(p.Nq, 128);
    hipLaunchKernelGGL((attn_mx8_kernel<DP>), dim3((unsigned)(q.nqb * p.B * p.H)), dim3(256), lds, s, q);
}

extern "C" int pbe_attention_mx8(const pbe_attn_mx8_desc* d, pbe_stream_t stream) {
    PBE_REQUIRE(d && d->Q && d->Q_scale && d->K && d->K_scale && d->VT && d->VT_scale && d->O, "pbe_attention_mx8: null operand");
    PBE_REQUIRE(d->B > 0 && d->H > 0 && d->Nq > 0 && d->Nk > 0, "pbe_attention_mx8: bad dims");
    PBE_REQUIRE(d->D == 40 || d->D == 80 || d->D == 160, "pbe_attention_mx8: head dim %d unsupported (40, 80, 160)", d->D);
    PBE_REQUIRE(d->o_rs % 4 == 0 && d->o_bs % 4 == 0 && ((uintptr_t)d->O & 7) == 0, "pbe_attention_mx8: O needs 8-byte aligned rows");
    PBE_REQUIRE(((uintptr_t)d->Q & 15) == 0 && ((uintptr_t)d->K & 15) == 0 && ((uintptr_t)d->VT & 15) == 0 &&
                ((uintptr_t)d->K_scale & 15) == 0 && ((uintptr_t)d->VT_scale & 15) == 0, "pbe_attention_mx8: 16-byte alignment");
    PBE_REQUIRE((long)d->B * d->H * ((d->Nq + 127) / 128) < (1L << 31), "pbe_attention_mx8: too many workgroups");
    AttnMx8P p;
    p.Q = (const unsigned char*)d->Q; p.Qs = (const unsigned char*)d->Q_scale;
    p.K = (const unsigned char*)d->K; p.Ks = (const unsigned char*)d->K_scale;
    p.V = (const unsigned char*)d->VT; p.Vs = (const unsigned char*)d->VT_scale;
    p.O = (h16*)d->O;
    p.B = d->B; p.H = d->H; p.Nq = d->Nq; p.Nk = d->Nk; p.D = d->D;
    p.o_bs = d->o_bs; p.o_rs = d->o_rs;
    p.scale_log2e = d->scale_log2e;
    hipStream_t s = (hipStream_t)stream;
    pbe_prof_begin(PBE_K_ATTN, s);
    if (d->D == 40) launch_attn_mx8<64>(p, s);
    else if (d->D == 80) launch_attn_mx8<128>(p, s);
    else launch_attn_mx8<192>(p, s);
    pbe_prof_end(PBE_K_ATTN, s, 4.0 * d->B * d->H * (double)d->Nq * d->Nk * d->D,
                 (double)d->B * d->H * d->D * (2.0 * d->Nq + 2.0 * d->Nk) * 0.5 + 2.0 * d->B * d->H * d->D * (double)d->Nq);
    PBE_LAUNCH_CHECK("pbe_attention_mx8");
    return PBE_OK;
}
