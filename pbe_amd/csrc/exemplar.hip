// The exemplar cut from a uint8 picture of any size on the device: Pillow's 8-bit resize (Resample.c) in its own integers, so that the
// bytes equal Image.resize's, and the bounding box of a mask.
//   pbe_resample_h_u8   rows first .. last of the picture -> uint8 [last - first, ow, 3]   (the horizontal pass, with mask / fill)
//   pbe_resample_v_u8   uint8 [rows, ow, 3] -> uint8 [oh, ow, 3] (+ normalised fp32 planes) (the vertical pass)
//   pbe_mask_box_i32    mask -> one (ya, yb, xa, xb) per band of rows                        (no atomics; the host reduces the bands)
// The filter tables come from the host (pbe_amd/exemplar.py: Pillow's precompute_coeffs + normalize_coeffs_8bpc in float64): per output
// index (xmin, n) and n coefficients rounded to 22 fractional bits.  A pass gives, per byte,
//   clip((2^21 + sum_x src[xmin + x] * k[x]) >> 22, 0, 255)
// with an int32 accumulator and an arithmetic shift: integer sums do not depend on their order, so tiling the taps changes nothing, and
// there is no float anywhere but the optional planes.  tests/pilref.py restates both passes.
// Nothing here trusts the tables for memory safety: xmin is clamped into the axis, n to ksize, and every tap to the rows / columns
// that exist, so a wrong table gives wrong bytes and never a read outside the operands.
#include "common.h"
#include "u8_norm.h"
#include "../../include/pbe_hip.h"

#define EW_BEGIN(s) pbe_prof_begin(PBE_K_ELEM, s)
#define EW_END(s, bytes, name) \
    pbe_prof_end(PBE_K_ELEM, s, bytes); \
    PBE_LAUNCH_CHECK(name); \
    return PBE_OK

#define RS_MAX_DIM 16384               // picture / output edge: rows * ow * 3 and every index stay below 2^31
#define RS_MAX_KSIZE 98305             // lanczos over a whole 16384 axis: ceil(3 * 16384) * 2 + 1
#define RS_BITS 22
#define RS_TW 64                       // output columns of one workgroup of the horizontal pass
#define RS_THREADS (RS_TW * 3)         // one thread per output column and channel: 3 waves
#define RS_CHUNK 4096                  // source pixels staged per round: 12 KiB of LDS
#define MB_BAND 32                     // rows of one band of pbe_mask_box_i32

__device__ __forceinline__ unsigned char rs_clip8(int acc) { return (unsigned char)min(max(acc >> RS_BITS, 0), 255); }

// ---- the horizontal pass ---------------------------------------------------------------------------------------------------------------
// Workgroup (bx, row): output columns c0 = 64 bx .. of source row first + row.  The columns' taps cover one segment of the source row
// (the bounds rise with the column); it goes through LDS in rounds of RS_CHUNK pixels: whole aligned dwords from HBM, each byte once per
// workgroup, then every thread adds the taps of its column that lie in the round.  With a mask, pixels whose mask byte is < 128 are
// overwritten by `fill` in LDS before the taps read them.  ksize is unbounded: the taps are a loop, the coefficients stay in memory
// (the same ksize * 64 ints for every row: L2).
__global__ void __launch_bounds__(RS_THREADS) resample_h_kernel(const unsigned char* pic, const unsigned char* pic_end, const unsigned char* mask,
                                                                unsigned fill, unsigned char* out, int Ws, int first, int ow, const int* bounds,
                                                                const int* coeffs, int ksize) {
    __shared__ unsigned stage[RS_CHUNK * 3 / 4 + 2];
    const int tid = threadIdx.x, row = blockIdx.y, y = first + row;
    const int c0 = blockIdx.x * RS_TW, tw = min(RS_TW, ow - c0);
    int seg0 = Ws, seg1 = 0;                                         // uniform: every thread walks the tile's bounds (scalar loads)
    for (int c = 0; c < tw; ++c) {
        const int lo = min(max(bounds[2 * (c0 + c)], 0), Ws), n = min(max(bounds[2 * (c0 + c) + 1], 0), ksize);
        seg0 = min(seg0, lo);
        seg1 = max(seg1, min(lo + n, Ws));
    }
    const int col = tid / 3, ch = tid - col * 3;
    const bool active = col < tw;
    int xmin = 0, xend = 0;
    const int* k = coeffs;
    if (active) {
        xmin = min(max(bounds[2 * (c0 + col)], 0), Ws);
        xend = min(xmin + min(max(bounds[2 * (c0 + col) + 1], 0), ksize), Ws);
        k = coeffs + (long)(c0 + col) * ksize;                      // k[x - xmin] is the coefficient of source column x
    }
    int acc = 1 << (RS_BITS - 1);
    const unsigned char* rowp = pic + (long)y * Ws * 3;
    for (int s0 = seg0; s0 < seg1; s0 += RS_CHUNK) {
        const int s1 = min(s0 + RS_CHUNK, seg1);
        const unsigned char* g = rowp + (long)s0 * 3;
        const int head = (int)((uintptr_t)g & 3);
        const unsigned char* a0 = g - head;                          // 4-byte aligned
        const int nwords = (head + (s1 - s0) * 3 + 3) >> 2;
        for (int w = tid; w < nwords; w += RS_THREADS) {
            const unsigned char* p = a0 + 4 * w;
            unsigned v = 0;
            if (p >= pic && p + 4 <= pic_end) v = *(const unsigned*)p;
            else {                                                   // the dword that straddles the picture's first or last byte
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (p + b >= pic && p + b < pic_end) v |= (unsigned)p[b] << (8 * b);
            }
            stage[w] = v;
        }
        __syncthreads();
        unsigned char* sb = (unsigned char*)stage + head;            // sb[(x - s0) * 3 + c]
        if (mask) {
            const unsigned char* mrow = mask + (long)y * Ws + s0;
            for (int p = tid; p < s1 - s0; p += RS_THREADS)
                if (mrow[p] < 128) {
                    sb[p * 3 + 0] = (unsigned char)fill; sb[p * 3 + 1] = (unsigned char)(fill >> 8); sb[p * 3 + 2] = (unsigned char)(fill >> 16);
                }
            __syncthreads();
        }
        const int lo = max(xmin, s0), hi = min(xend, s1);
        for (int x = lo; x < hi; ++x) acc += (int)sb[(x - s0) * 3 + ch] * k[x - xmin];
        __syncthreads();
    }
    if (active) out[((long)row * ow + c0 + col) * 3 + ch] = rs_clip8(acc);
}

extern "C" size_t pbe_resample_workspace_bytes(int32_t rows, int32_t ow) {
    if (rows < 1 || ow < 1 || rows > RS_MAX_DIM || ow > RS_MAX_DIM) return 0;
    return (((size_t)rows * ow * 3) + 15) & ~(size_t)15;
}

static int rs_tables_ok(const int32_t* bounds, const int32_t* coeffs, int32_t ksize) {
    return bounds && coeffs && ((uintptr_t)bounds & 3) == 0 && ((uintptr_t)coeffs & 3) == 0 && ksize >= 1 && ksize <= RS_MAX_KSIZE;
}

extern "C" int pbe_resample_h_u8(const void* picture, const void* mask, const uint8_t* fill3, void* out, int32_t Hs, int32_t Ws, int32_t first,
                                 int32_t last, int32_t ow, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, pbe_stream_t stream) {
    PBE_REQUIRE(picture && out, "pbe_resample_h_u8: null picture or output");
    PBE_REQUIRE(Hs >= 1 && Ws >= 1 && ow >= 1 && Hs <= RS_MAX_DIM && Ws <= RS_MAX_DIM && ow <= RS_MAX_DIM,
                "pbe_resample_h_u8: edges Hs = %d, Ws = %d, ow = %d must lie in 1 .. %d", Hs, Ws, ow, RS_MAX_DIM);
    PBE_REQUIRE(first >= 0 && first < last && last <= Hs, "pbe_resample_h_u8: rows %d .. %d are not inside the %d rows of the picture", first, last, Hs);
    PBE_REQUIRE(rs_tables_ok(bounds, coeffs, ksize), "pbe_resample_h_u8: tables null or not 4-byte aligned, or ksize = %d outside 1 .. %d", ksize, RS_MAX_KSIZE);
    PBE_REQUIRE(!mask || fill3, "pbe_resample_h_u8: a mask needs the three fill bytes");
    hipStream_t s = (hipStream_t)stream;
    const unsigned fill = fill3 ? ((unsigned)fill3[0] | (unsigned)fill3[1] << 8 | (unsigned)fill3[2] << 16) : 0u;
    const unsigned char* pic = (const unsigned char*)picture;
    const int rows = last - first;
    EW_BEGIN(s);
    hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)cdiv(ow, RS_TW), (unsigned)rows), dim3(RS_THREADS), 0, s, pic, pic + (size_t)Hs * Ws * 3,
                       (const unsigned char*)mask, fill, (unsigned char*)out, Ws, first, ow, bounds, coeffs, ksize);
    EW_END(s, (double)rows * (3.0 * Ws + 3.0 * ow), "pbe_resample_h_u8");
}

// ---- the vertical pass -----------------------------------------------------------------------------------------------------------------
// One thread per output byte: workgroup (bx, oy) holds 256 consecutive bytes of output row oy, so every tap is one coalesced read of a
// source row (a source byte serves the output rows whose taps cover it: those re-reads are L2's).  mask (uint8 [rows, ow], may be null)
// composes `fill` as the horizontal pass does - for the launches that read the picture itself because Pillow skips the horizontal pass.
__global__ void __launch_bounds__(256) resample_v_kernel(const unsigned char* src, const unsigned char* mask, unsigned fill, unsigned char* out,
                                                         float* planes, int rows, int ow, int oh, const int* bounds, const int* coeffs, int ksize,
                                                         float m0, float m1, float m2, float s0, float s1, float s2) {
    const int j = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y, pitch = ow * 3;
    if (j >= pitch) return;
    const int x = j / 3, ch = j - x * 3;
    const int ymin = min(max(bounds[2 * oy], 0), rows);
    const int yend = min(ymin + min(max(bounds[2 * oy + 1], 0), ksize), rows);
    const int* k = coeffs + (long)oy * ksize;
    const unsigned char f = (unsigned char)(fill >> (8 * ch));
    int acc = 1 << (RS_BITS - 1);
    for (int y = ymin; y < yend; ++y) {
        unsigned char v = src[(long)y * pitch + j];
        if (mask && mask[(long)y * ow + x] < 128) v = f;
        acc += (int)v * k[y - ymin];
    }
    const unsigned char b = rs_clip8(acc);
    out[(long)oy * pitch + j] = b;
    if (planes) {
        const float mean = ch == 0 ? m0 : (ch == 1 ? m1 : m2), sd = ch == 0 ? s0 : (ch == 1 ? s1 : s2);
        planes[((long)ch * oh + oy) * ow + x] = pbe_u8_norm(b, mean, sd);
    }
}

extern "C" int pbe_resample_v_u8(const void* src, const void* mask, const uint8_t* fill3, void* out, float* planes, int32_t rows, int32_t ow,
                                 int32_t oh, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, const float* mean3, const float* std3,
                                 pbe_stream_t stream) {
    PBE_REQUIRE(src && out, "pbe_resample_v_u8: null source or output");
    PBE_REQUIRE(rows >= 1 && ow >= 1 && oh >= 1 && rows <= RS_MAX_DIM && ow <= RS_MAX_DIM && oh <= RS_MAX_DIM,
                "pbe_resample_v_u8: edges rows = %d, ow = %d, oh = %d must lie in 1 .. %d", rows, ow, oh, RS_MAX_DIM);
    PBE_REQUIRE(rs_tables_ok(bounds, coeffs, ksize), "pbe_resample_v_u8: tables null or not 4-byte aligned, or ksize = %d outside 1 .. %d", ksize, RS_MAX_KSIZE);
    PBE_REQUIRE(!mask || fill3, "pbe_resample_v_u8: a mask needs the three fill bytes");
    PBE_REQUIRE(!planes || (mean3 && std3 && ((uintptr_t)planes & 3) == 0), "pbe_resample_v_u8: the planes need mean and std and 4-byte alignment");
    hipStream_t s = (hipStream_t)stream;
    const unsigned fill = fill3 ? ((unsigned)fill3[0] | (unsigned)fill3[1] << 8 | (unsigned)fill3[2] << 16) : 0u;
    const float m[3] = {planes ? mean3[0] : 0.f, planes ? mean3[1] : 0.f, planes ? mean3[2] : 0.f};
    const float d[3] = {planes ? std3[0] : 1.f, planes ? std3[1] : 1.f, planes ? std3[2] : 1.f};
    EW_BEGIN(s);
    hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)cdiv((long)ow * 3, 256), (unsigned)oh), dim3(256), 0, s, (const unsigned char*)src,
                       (const unsigned char*)mask, fill, (unsigned char*)out, planes, rows, ow, oh, bounds, coeffs, ksize, m[0], m[1], m[2], d[0], d[1], d[2]);
    EW_END(s, 3.0 * ow * ((double)rows + oh) + (planes ? 12.0 * ow * oh : 0.0), "pbe_resample_v_u8");
}

// ---- the bounding box of a mask ----------------------------------------------------------------------------------------------------------
// Workgroup b scans rows 32 b .. 32 b + 31 (thread t the columns t, t + 256, ...: a wave reads 64 consecutive bytes), reduces
// (min y, max y, min x, max x) over the bytes >= 128 through the wave and then LDS, and thread 0 writes row b of the table:
// (ya, yb, xa, xb) inclusive, or four -1 for a band without such a byte.  Every element of the table is written once, by one thread.
__global__ void __launch_bounds__(256) mask_box_kernel(const unsigned char* mask, int* table, int Hs, int Ws) {
    __shared__ int part[4][4];
    const int tid = threadIdx.x, y0 = blockIdx.x * MB_BAND, y1 = min(y0 + MB_BAND, Hs);
    int ya = 0x7fffffff, yb = -1, xa = 0x7fffffff, xb = -1;
    for (int y = y0; y < y1; ++y) {
        const unsigned char* r = mask + (long)y * Ws;
        for (int x = tid; x < Ws; x += 256)
            if (r[x] >= 128) { ya = min(ya, y); yb = max(yb, y); xa = min(xa, x); xb = max(xb, x); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ya = min(ya, __shfl_xor(ya, o, 64)); yb = max(yb, __shfl_xor(yb, o, 64));
        xa = min(xa, __shfl_xor(xa, o, 64)); xb = max(xb, __shfl_xor(xb, o, 64));
    }
    if ((tid & 63) == 0) { part[tid >> 6][0] = ya; part[tid >> 6][1] = yb; part[tid >> 6][2] = xa; part[tid >> 6][3] = xb; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) { ya = min(ya, part[w][0]); yb = max(yb, part[w][1]); xa = min(xa, part[w][2]); xb = max(xb, part[w][3]); }
        const bool empty = yb < 0;
        int* t = table + 4 * blockIdx.x;
        t[0] = empty ? -1 : ya; t[1] = empty ? -1 : yb; t[2] = empty ? -1 : xa; t[3] = empty ? -1 : xb;
    }
}

extern "C" int32_t pbe_mask_box_bands(int32_t Hs) { return Hs >= 1 && Hs <= RS_MAX_DIM ? cdiv(Hs, MB_BAND) : 0; }

extern "C" int pbe_mask_box_i32(const void* mask, int32_t* table, int32_t Hs, int32_t Ws, int32_t bands, pbe_stream_t stream) {
    PBE_REQUIRE(mask && table && ((uintptr_t)table & 3) == 0, "pbe_mask_box_i32: null mask or table, or the table is not 4-byte aligned");
    PBE_REQUIRE(Hs >= 1 && Ws >= 1 && Hs <= RS_MAX_DIM && Ws <= RS_MAX_DIM, "pbe_mask_box_i32: edges Hs = %d, Ws = %d must lie in 1 .. %d", Hs, Ws, RS_MAX_DIM);
    PBE_REQUIRE(bands == pbe_mask_box_bands(Hs), "pbe_mask_box_i32: the table has %d rows, %d rows of the mask need %d", bands, Hs, pbe_mask_box_bands(Hs));
    hipStream_t s = (hipStream_t)stream;
    EW_BEGIN(s);
    hipLaunchKernelGGL(mask_box_kernel, dim3((unsigned)bands), dim3(256), 0, s, (const unsigned char*)mask, table, Hs, Ws);
    EW_END(s, (double)Hs * Ws + 16.0 * bands, "pbe_mask_box_i32");
}
