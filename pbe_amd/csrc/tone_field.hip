// A tone that varies across the pasted window: a low-frequency field of the difference between what the model saw and what it returned.
//   pbe_tone_cells_i32        image (model-normalised) + result ([0, 1]) + sel -> per cell of `cell` x `cell` working pixels n and, per
//                             channel, sum (o - q) over the selected pixels; o and q the two bytes of tone.hip (tone_bytes.h)
//   pbe_tone_field_f32        the cell table -> a dense coarse field in [0, 1] units by a pull-push fill: sums pulled up a 2 x 2 pyramid,
//                             cell means pushed down it, each level blending its own mean in by the evidence it holds
// pbe_paste_window_field_u8 (window.hip) adds the field, sampled bilinearly, to the resampled result before the blend.
// Everything that is added up is an integer, there are no atomics and no float sums, and every output element is written exactly once by
// one thread: the table and the field are the same from run to run.  tests/fieldref.py restates both element for element.
#include "common.h"
#include "tone_bytes.h"
#include "../../include/pbe_hip.h"

#define EW_BEGIN(s) pbe_prof_begin(PBE_K_ELEM, s)
#define EW_END(s, bytes, name) \
    pbe_prof_end(PBE_K_ELEM, s, bytes); \
    PBE_LAUNCH_CHECK(name); \
    return PBE_OK

#define WIN_MAX_DIM 16384              // the edge limit of window.hip
#define TONE_MAX_BATCH 65535           // samples ride on gridDim.z (cells) / gridDim.x (field)
#define FIELD_MAX_CELLS (1 << 20)      // Hc * Wc of pbe_tone_field_f32: one workgroup walks a sample's pyramid
#define FIELD_THREADS 1024             // ... of 16 waves: the walk is a chain of dependent global round trips, so more cells in flight per level

// ---- pbe_tone_cells_i32 ----------------------------------------------------------------------------------------------------------------
// Why nothing overflows: a pixel adds o - q in -255 .. 255, a cell has at most cell^2 <= 4096 pixels, so |sum| <= 255 cell^2 < 2^21 in
// 32 bits - per thread (VEC * cell pixels), across the lanes of a cell and in the table alike.
static_assert(255L * 64 * 64 < (1L << 21), "a cell sum could leave 21 bits");

// grid (ceil(ceil(W / VEC) / 256), Hc, B).  A thread owns VEC neighbouring columns and walks the rows of one cell row: consecutive lanes
// load consecutive vectors of a picture row.  VEC divides CELL and a thread's first column is a multiple of VEC, so its pixels lie in one
// cell, and the CELL / VEC threads of a cell are neighbouring lanes of one wave that start on a multiple of CELL / VEC: a xor-shuffle
// over the offsets below CELL / VEC sums them, and the first of them writes the cell's four numbers.  Lanes past the right edge add 0.
// VEC pixels per load: 4 or 2 only where W is a multiple of it and the three tensors start on 16 / 8 bytes - then H * W is a multiple of
// it as well (the rule of tone_stats_kernel) and every ROW starts aligned, which a table of cells needs on top of it; else VEC = 1.
template <int VEC, int CELL>
__global__ void __launch_bounds__(256) tone_cells_kernel(const float* __restrict__ image, const float* __restrict__ result, const float* __restrict__ sel,
                                                         int* __restrict__ cells, int H, int W, int Hc, int Wc) {
    typedef typename ToneVec<VEC>::type vec_t;
    constexpr int LANES = CELL / VEC;                                // threads per cell: 1 .. 64, a power of two
    const int b = blockIdx.z, cy = blockIdx.y;
    const long HW = (long)H * W;
    const int g = blockIdx.x * 256 + threadIdx.x;                   // the thread's vector within a row
    const int x = g * VEC;
    const float* ip = image + (size_t)b * 3 * HW;
    const float* rp = result + (size_t)b * 3 * HW;
    const float* sp = sel + (size_t)b * HW;
    int acc[4] = {0, 0, 0, 0};
    if (x < W) {                                                    // W is a multiple of VEC wherever VEC > 1: the whole vector lies in the row
        const int ya = cy * CELL, yb = min(ya + CELL, H);           // the bottom cell row may be ragged
#pragma unroll 4
        for (int y = ya; y < yb; ++y) {
            const size_t at = (size_t)y * W + x;
            float s[VEC], xi[3][VEC], r[3][VEC];
            const vec_t sv = *(const vec_t*)(sp + at);
            __builtin_memcpy(s, &sv, sizeof(sv));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const vec_t xv = *(const vec_t*)(ip + (size_t)c * HW + at), rv = *(const vec_t*)(rp + (size_t)c * HW + at);
                __builtin_memcpy(xi[c], &xv, sizeof(xv));
                __builtin_memcpy(r[c], &rv, sizeof(rv));
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (!(s[v] >= 0.5f)) continue;                      // a NaN selects nothing
                acc[0] += 1;
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[1 + c] += (int)tone_byte_image(xi[c][v]) - (int)tone_byte_result(r[c][v]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = LANES >> 1; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    }
    const int cx = x / CELL;
    if ((threadIdx.x & (LANES - 1)) == 0 && cx < Wc) {             // one writer per cell; the right cell column may be ragged
        const size_t plane = (size_t)Hc * Wc;
        int* out = cells + (size_t)b * 4 * plane + (size_t)cy * Wc + cx;
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k * plane] = acc[k];
    }
}

template <int VEC>
static void tone_cells_launch(int cell, dim3 grid, hipStream_t s, const float* image, const float* result, const float* sel, int* cells, int H, int W, int Hc, int Wc) {
    switch (cell) {
        case 4: hipLaunchKernelGGL((tone_cells_kernel<VEC, 4>), grid, dim3(256), 0, s, image, result, sel, cells, H, W, Hc, Wc); break;
        case 8: hipLaunchKernelGGL((tone_cells_kernel<VEC, 8>), grid, dim3(256), 0, s, image, result, sel, cells, H, W, Hc, Wc); break;
        case 16: hipLaunchKernelGGL((tone_cells_kernel<VEC, 16>), grid, dim3(256), 0, s, image, result, sel, cells, H, W, Hc, Wc); break;
        case 32: hipLaunchKernelGGL((tone_cells_kernel<VEC, 32>), grid, dim3(256), 0, s, image, result, sel, cells, H, W, Hc, Wc); break;
        default: hipLaunchKernelGGL((tone_cells_kernel<VEC, 64>), grid, dim3(256), 0, s, image, result, sel, cells, H, W, Hc, Wc); break;
    }
}
static bool tone_cell_ok(int32_t cell) { return cell == 4 || cell == 8 || cell == 16 || cell == 32 || cell == 64; }

extern "C" int pbe_tone_cells_i32(const float* image, const float* result, const float* sel, int32_t* cells, int32_t B, int32_t H, int32_t W, int32_t cell,
                                  pbe_stream_t stream) {
    PBE_REQUIRE(image && result && sel && cells && B > 0 && H > 0 && W > 0, "pbe_tone_cells_i32: bad arguments");
    PBE_REQUIRE(H <= WIN_MAX_DIM && W <= WIN_MAX_DIM, "pbe_tone_cells_i32: an edge above %d", WIN_MAX_DIM);
    PBE_REQUIRE(B <= TONE_MAX_BATCH, "pbe_tone_cells_i32: batch %d above %d", B, TONE_MAX_BATCH);
    PBE_REQUIRE(tone_cell_ok(cell), "pbe_tone_cells_i32: cell %d is not one of 4, 8, 16, 32, 64", cell);
    PBE_REQUIRE(((uintptr_t)cells & 3) == 0, "pbe_tone_cells_i32: cells must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int Hc = (H + cell - 1) / cell, Wc = (W + cell - 1) / cell;
    const uintptr_t bits = (uintptr_t)image | (uintptr_t)result | (uintptr_t)sel;
    const int vec = (W % 4 == 0 && (bits & 15) == 0) ? 4 : (W % 2 == 0 && (bits & 7) == 0) ? 2 : 1;
    const int groups = (W + vec - 1) / vec;
    const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)Hc, (unsigned)B);
    EW_BEGIN(s);
    if (vec == 4) tone_cells_launch<4>(cell, grid, s, image, result, sel, cells, H, W, Hc, Wc);
    else if (vec == 2) tone_cells_launch<2>(cell, grid, s, image, result, sel, cells, H, W, Hc, Wc);
    else tone_cells_launch<1>(cell, grid, s, image, result, sel, cells, H, W, Hc, Wc);
    EW_END(s, 28.0 * (double)B * (double)H * W + 16.0 * (double)B * Hc * Wc, "pbe_tone_cells_i32");
}

// ---- pbe_tone_field_f32 ----------------------------------------------------------------------------------------------------------------
// The pyramid.  Level 0 is the Hc x Wc table; level l + 1 has ceil(Hl / 2) x ceil(Wl / 2) cells; the top is 1 x 1.  A sample's levels
// 1 .. top hold T cells in all.  The workspace keeps, for B samples, first the pulled sums (int64 [B][T cells][4], levels one after the
// other, inside a level four planes n, S0, S1, S2) and then the pushed fields of those levels (fp32 [B][T cells][3] the same way).  Level
// 0 needs no room: its sums are the table and its field is the output.  Every element that is read was written in this launch.
struct FieldLevel {
    int H, W;
    long off;                          // cells of levels 1 .. l - 1
};
__host__ __device__ static inline FieldLevel field_level(int Hc, int Wc, int l) {
    FieldLevel f = {Hc, Wc, 0};
    for (int k = 0; k < l; ++k) {
        if (k > 0) f.off += (long)f.H * f.W;
        f.H = (f.H + 1) >> 1;
        f.W = (f.W + 1) >> 1;
    }
    return f;
}
__host__ __device__ static inline int field_levels(int Hc, int Wc) {          // levels in all, the table included: 1 for a 1 x 1 grid
    int n = 1;
    while (Hc > 1 || Wc > 1) {
        Hc = (Hc + 1) >> 1;
        Wc = (Wc + 1) >> 1;
        ++n;
    }
    return n;
}
static long field_upper_cells(int Hc, int Wc) {                               // T
    const int L = field_levels(Hc, Wc);
    if (L == 1) return 0;
    const FieldLevel top = field_level(Hc, Wc, L - 1);
    return top.off + 1;
}

// m = clamp((float)((double)S / (255.0 (double)n)), -limit, +limit), 0 where n == 0: one rounding from an exact double quotient
__device__ __forceinline__ float field_mean(long long n, long long S, float limit) {
    if (n <= 0) return 0.f;
    const float m = (float)((double)S / (255.0 * (double)n));
    return fminf(fmaxf(m, -limit), limit);
}
// 0.75 a + 0.25 b written so that a constant stays a constant bit for bit
__device__ __forceinline__ float field_mix(float a, float b) { return fmaf(0.25f, b - a, a); }

// grid B, one workgroup per sample.  The levels follow one another with a __syncthreads() between them: a level is written by this
// workgroup's threads to global memory and read by other threads of the same workgroup, which the barrier (and its fence) orders.  The
// pointers into the workspace and the field are not __restrict__ for that reason.
__global__ void __launch_bounds__(FIELD_THREADS) tone_field_kernel(const int* __restrict__ cells, float* field, long long* sums, float* upper, int Hc, int Wc, int L, long T,
                                                         int cap, float limit, int min_pixels) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const long plane0 = (long)Hc * Wc;
    const int* tab = cells + (size_t)b * 4 * plane0;
    float* out = field + (size_t)b * 3 * plane0;
    long long* sm = sums + (size_t)b * 4 * T;
    float* up = upper + (size_t)b * 3 * T;
    // pull
    for (int l = 1; l < L; ++l) {
        const FieldLevel lo = field_level(Hc, Wc, l - 1), hi = field_level(Hc, Wc, l);
        const long nlo = (long)lo.H * lo.W, nhi = (long)hi.H * hi.W;
        for (long e = tid; e < nhi; e += FIELD_THREADS) {
            const int i = (int)(e / hi.W), j = (int)(e - (long)i * hi.W);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                long long t = 0;
#pragma unroll
                for (int di = 0; di < 2; ++di)
#pragma unroll
                    for (int dj = 0; dj < 2; ++dj) {
                        const int ci = 2 * i + di, cj = 2 * j + dj;
                        if (ci >= lo.H || cj >= lo.W) continue;                  // a child outside the grid adds nothing
                        const long at = (long)ci * lo.W + cj;
                        t += l == 1 ? (long long)tab[k * plane0 + at] : sm[4 * lo.off + k * nlo + at];
                    }
                sm[4 * hi.off + k * nhi + e] = t;
            }
        }
        __syncthreads();
    }
    // the whole window's n: too little evidence changes nothing
    const FieldLevel top = field_level(Hc, Wc, L - 1);
    const long long n_all = L == 1 ? (long long)tab[0] : sm[4 * top.off];
    if (n_all <= 0 || n_all < (long long)min_pixels) {                           // the same for every thread of the workgroup
        for (long e = tid; e < 3 * plane0; e += FIELD_THREADS) out[e] = 0.f;
        return;
    }
    // push
    for (int l = L - 1; l >= 0; --l) {
        const FieldLevel me = field_level(Hc, Wc, l), hi = field_level(Hc, Wc, l + 1);
        const long nme = (long)me.H * me.W, nhi = (long)hi.H * hi.W;
        float* dst = l == 0 ? out : up + 3 * me.off;
        const float* par = up + 3 * hi.off;                                      // not read at the top
        for (long e = tid; e < nme; e += FIELD_THREADS) {
            const int i = (int)(e / me.W), j = (int)(e - (long)i * me.W);
            const long long n = l == 0 ? (long long)tab[e] : sm[4 * me.off + e];
            const float w = (float)(n < cap ? (int)n : cap) / (float)cap;
            const int ia = i >> 1, ib = min(max(ia + ((i & 1) ? 1 : -1), 0), hi.H - 1);
            const int ja = j >> 1, jb = min(max(ja + ((j & 1) ? 1 : -1), 0), hi.W - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const long long S = l == 0 ? (long long)tab[(1 + c) * plane0 + e] : sm[4 * me.off + (1 + c) * nme + e];
                const float m = field_mean(n, S, limit);
                float v = m;
                if (l < L - 1) {
                    const float* p = par + c * nhi;
                    const float ra = field_mix(p[(long)ia * hi.W + ja], p[(long)ib * hi.W + ja]);
                    const float rb = field_mix(p[(long)ia * hi.W + jb], p[(long)ib * hi.W + jb]);
                    const float u = field_mix(ra, rb);
                    v = fmaf(w, m - u, u);
                }
                dst[c * nme + e] = v;
            }
        }
        if (l > 0) __syncthreads();
    }
}

static bool field_dims_ok(int32_t B, int32_t Hc, int32_t Wc) {
    return B > 0 && B <= TONE_MAX_BATCH && Hc > 0 && Wc > 0 && Hc <= WIN_MAX_DIM / 4 && Wc <= WIN_MAX_DIM / 4 && (long)Hc * Wc <= FIELD_MAX_CELLS;
}
extern "C" size_t pbe_tone_field_workspace_bytes(int32_t B, int32_t Hc, int32_t Wc) {
    if (!field_dims_ok(B, Hc, Wc)) return 0;
    return (size_t)B * (size_t)field_upper_cells(Hc, Wc) * (4 * sizeof(long long) + 3 * sizeof(float)) + 16;       // never 0 for a valid grid
}
extern "C" int pbe_tone_field_f32(const int32_t* cells, float* field, int32_t B, int32_t Hc, int32_t Wc, int32_t cell, float limit, int32_t min_pixels,
                                  void* workspace, size_t workspace_bytes, pbe_stream_t stream) {
    PBE_REQUIRE(cells && field && workspace && B > 0 && Hc > 0 && Wc > 0, "pbe_tone_field_f32: bad arguments");
    PBE_REQUIRE(B <= TONE_MAX_BATCH, "pbe_tone_field_f32: batch %d above %d", B, TONE_MAX_BATCH);
    PBE_REQUIRE(Hc <= WIN_MAX_DIM / 4 && Wc <= WIN_MAX_DIM / 4, "pbe_tone_field_f32: a grid edge above %d", WIN_MAX_DIM / 4);
    PBE_REQUIRE((long)Hc * Wc <= FIELD_MAX_CELLS, "pbe_tone_field_f32: a grid of %d x %d cells, more than 2^20: one workgroup walks a sample's pyramid - take a larger cell",
                Hc, Wc);
    PBE_REQUIRE(tone_cell_ok(cell), "pbe_tone_field_f32: cell %d is not one of 4, 8, 16, 32, 64", cell);
    PBE_REQUIRE(limit > 0.f && limit <= 3.0e38f, "pbe_tone_field_f32: limit must be finite and > 0");
    PBE_REQUIRE(min_pixels >= 0, "pbe_tone_field_f32: min_pixels %d below 0", min_pixels);
    PBE_REQUIRE(((uintptr_t)workspace & 7) == 0, "pbe_tone_field_f32: the workspace must be 8-byte aligned");
    PBE_REQUIRE(workspace_bytes >= pbe_tone_field_workspace_bytes(B, Hc, Wc), "pbe_tone_field_f32: workspace of %zu bytes, %zu needed", workspace_bytes,
                pbe_tone_field_workspace_bytes(B, Hc, Wc));
    hipStream_t s = (hipStream_t)stream;
    const long T = field_upper_cells(Hc, Wc);
    long long* sums = (long long*)workspace;
    float* upper = (float*)(sums + (size_t)B * 4 * T);
    EW_BEGIN(s);
    hipLaunchKernelGGL(tone_field_kernel, dim3((unsigned)B), dim3(FIELD_THREADS), 0, s, (const int*)cells, field, sums, upper, Hc, Wc, field_levels(Hc, Wc), T, cell * cell, limit,
                       min_pixels);
    EW_END(s, (double)B * (28.0 * (double)Hc * Wc + 88.0 * (double)T), "pbe_tone_field_f32");
}
