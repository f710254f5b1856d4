// MX-fp8 copy-out of the implicit-GEMM epilogues (EX_MX forms of igemm_kernel.h, form 2 of igemm_astat.hip): device helpers only.
#pragma once
#include "igemm_params.h"

// ---- MX-fp8 copy-out (EX_MX; also the A-stationary tile's form 2): staged fp16 values -> pbe_quant_mx8_f16's bytes and scales ----
// A block's values are the fp16 values pbe_gemm_f16 would store, times the range's alpha in fp32, then pbe_quant_mx8_f16's arithmetic
// (mx8_scale_exp / mx8_e4m3, common.h) to pbe_quant_mx8_f16's addresses: bit-identical to the two-launch path by construction.
// One block straight from the staged values at src (len in {8, 16, 24, 32}: whole 16-byte chunks; zeros past it, as the quantiser pads):
// the amax in a first pass over the LDS, then the bytes 16 values at a time - 16 live floats instead of 32 (the A-stationary tile's
// epilogue holds its A block and accumulators in registers: the whole-block form spilled 100 bytes per lane there).
__device__ __forceinline__ int mx8_block_lds(const h16* src, int len, float al, unsigned char* dst) {
    typedef int i32x4_ __attribute__((ext_vector_type(4)));
    float amax = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (8 * c < len) {
            const h16x8 x = *reinterpret_cast<const h16x8*>(src + 8 * c);
#pragma unroll
            for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf((float)x[e] * al));
        }
    }
    const int se = mx8_scale_exp(amax);
    const float inv = __uint_as_float((unsigned)(254 - se) << 23);                          // 1 / 2^(se - 127), exact
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        i32x4_ w;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int c = 2 * hf + cc;
            h16x8 x = {};
            if (8 * c < len) x = *reinterpret_cast<const h16x8*>(src + 8 * c);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                unsigned word = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = 8 * c + 4 * q + e < len ? (float)x[4 * q + e] * al : 0.f;
                    word |= mx8_e4m3(v * inv) << (8 * e);
                }
                w[2 * cc + q] = (int)word;
            }
        }
        *reinterpret_cast<i32x4_*>(dst + 16 * hf) = w;
    }
    return se;
}

// the range holding output column n (the last one starting at or left of it), -1: none
__device__ __forceinline__ int mx8_range(const IGemmP& p, int n) {
    int r = -1;
    for (int q = 0; q < p.mx_nr; ++q)
        if (p.mx_c0[q] <= n && (r < 0 || p.mx_c0[q] > p.mx_c0[r])) r = q;
    return r;
}

// V^T scale of block (sample b, channel c of the range, tokens tok .. tok + 31) at (b, h, tok / 32, d).  The last channel of a head also writes
// the head's scale pad rows [D, DV) as 1.0 (pbe_attention_mx8 reads them: pad rows and the ones row): 8 bytes at a time (the scale rows
// are 16-byte aligned, DV % 32 == 0, D % 8 == 0)
__device__ __forceinline__ void mx8_vt_scale(const IGemmP& p, int r, int b, int c, int tok, int se) {
    const int D = p.mx_D, DV = p.mx_DV;
    const int h = c / D, d = c - h * D;
    unsigned char* sp = p.mx_scale[r] + (((long)b * p.mx_H + h) * (p.mx_N >> 5) + (tok >> 5)) * DV;
    sp[d] = (unsigned char)se;
    if (d == D - 1)
        for (int q = D; q < DV; q += 8) *reinterpret_cast<unsigned long long*>(sp + q) = 0x7f7f7f7f7f7f7f7full;
}

// V^T block (sample b, channel c of the range, 32 staged tokens from token tok): bytes row b H D + c, then its scale
__device__ __forceinline__ void mx8_vt_block(const IGemmP& p, int r, const h16* src, int b, int c, int tok) {
    const int se = mx8_block_lds(src, 32, p.mx_alpha[r], p.mx_data[r] + ((long)b * p.mx_H * p.mx_D + c) * p.mx_N + tok);
    mx8_vt_scale(p, r, b, c, tok, se);
}

// The same block over a lane pair (l, l ^ 32) of one wave: half hf = l >> 5 holds tokens 16 hf .. 16 hf + 15, the amax meets over the pair
// (a maximum: exact in any order), each half converts and stores its 16 bytes, the lower lane the scale - every lane of the wave busy where
// a lane per block would leave half of them idle (the A-stationary tile's 32-channel passes)
__device__ __forceinline__ void mx8_vt_block_pair(const IGemmP& p, int r, const h16* src, int b, int c, int tok, int hf) {
    typedef int i32x4_ __attribute__((ext_vector_type(4)));
    const float al = p.mx_alpha[r];
    const h16x8 x[2] = {*reinterpret_cast<const h16x8*>(src + 16 * hf), *reinterpret_cast<const h16x8*>(src + 16 * hf + 8)};
    float amax = 0.f;
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf((float)x[c2][e] * al));
    amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
    const int se = mx8_scale_exp(amax);
    const float inv = __uint_as_float((unsigned)(254 - se) << 23);                          // 1 / 2^(se - 127), exact
    i32x4_ w;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned word = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) word |= mx8_e4m3((float)x[q >> 1][4 * (q & 1) + e] * al * inv) << (8 * e);
        w[q] = (int)word;
    }
    *reinterpret_cast<i32x4_*>(p.mx_data[r] + ((long)b * p.mx_H * p.mx_D + c) * p.mx_N + tok + 16 * hf) = w;
    if (hf == 0) mx8_vt_scale(p, r, b, c, tok, se);
}

// TOKENS blocks of `rows` staged rows (LDS row stride ld halfs, output rows mrow0 ..) x `cols` columns from output column x0, all inside
// range r: block (h, j) = columns h D + 32 j .. + min(32, D - 32 j) of the range; the head's last block also writes the all-padding block
// behind it (DP / 32 - blocks per head <= 1: zero bytes, scale 1.0).  Threads t0, t0 + nt, ... take one (row, block) each, blocks fastest.
__device__ __forceinline__ void mx8_token_blocks(const IGemmP& p, int r, const h16* st, int ld, int rows, int x0, int cols, int mrow0, int t0, int nt) {
    const int D = p.mx_D, Hh = p.mx_H, Nt = p.mx_N, DP = p.mx_DP;
    const int nbh = (D + 31) >> 5, npb = DP >> 5;
    auto nblk = [&](int x) { const int hh = x / D; return hh * nbh + (x - hh * D + 31) / 32; };           // blocks left of column x
    const int c0 = p.mx_c0[r], rel0 = x0 - c0, rel1 = min(x0 + cols, c0 + Hh * D) - c0;
    if (rel1 <= rel0) return;
    const int b0 = nblk(rel0), cnt = nblk(rel1) - b0;
    const float al = p.mx_alpha[r];
    for (int idx = t0; idx < rows * cnt; idx += nt) {
        const int row = idx / cnt, gb = b0 + (idx - row * cnt);
        const int m = mrow0 + row;
        if (m >= p.M) continue;
        const int h = gb / nbh, j = gb - h * nbh, len = min(32, D - 32 * j);
        unsigned char* dst = p.mx_data[r] + (long)m * Hh * DP + h * DP + 32 * j;
        const int se = mx8_block_lds(st + row * ld + (c0 + h * D + 32 * j - x0), len, al, dst);
        const int b = m / Nt, n = m - b * Nt;
        unsigned char* sp = p.mx_scale[r] + (((long)b * Hh + h) * npb + j) * Nt + n;
        sp[0] = (unsigned char)se;
        if (j == nbh - 1 && npb > nbh) {
            typedef int i32x4_ __attribute__((ext_vector_type(4)));
            *reinterpret_cast<i32x4_*>(dst + 32) = (i32x4_){0, 0, 0, 0};
            *reinterpret_cast<i32x4_*>(dst + 48) = (i32x4_){0, 0, 0, 0};
            sp[Nt] = 127;
        }
    }
}
