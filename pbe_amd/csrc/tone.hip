// Tone statistics of a pasted window: what the model saw against what it returned, on the pixels it was told to keep.
//   pbe_tone_stats_i64        image (model-normalised) + result ([0, 1]) + sel -> per sample and channel n, So, Sq, Soo, Sqq, Soq
// over the selected pixels, o and q the two pictures as BYTES (the grey levels the paste writes).  pbe_amd.window.fit_tone turns the
// table into one affine map per window and channel on the host; pbe_paste_window_tone_u8 (window.hip) applies it.
// Everything that is added is an integer, there are no atomics and no float sums: the table is the same whatever order the blocks ran
// in, and tests/toneref.py restates it element for element.
#include "common.h"
#include "tone_bytes.h"          // tone_byte_image, tone_byte_result, ToneVec: shared with tone_field.hip
#include "../../include/pbe_hip.h"

#define EW_BEGIN(s) pbe_prof_begin(PBE_K_ELEM, s)
#define EW_END(s, bytes, name) \
    pbe_prof_end(PBE_K_ELEM, s, bytes); \
    PBE_LAUNCH_CHECK(name); \
    return PBE_OK

#define WIN_MAX_DIM 16384              // the edge limit of window.hip
#define TONE_MAX_BATCH 65535           // samples ride on gridDim.y
#define TONE_MAX_BLOCKS 256            // blocks per sample: threads stride, so a block sums many pixels before it reduces once
#define TONE_BLOCK_PIXELS 1024         // ... and no block is started for fewer pixels than this (one float4 per thread)
#define TONE_ACC 16                    // n, then per channel So, Sq, Soo, Sqq, Soq

// Why nothing overflows at 16384 x 16384 (2^28 pixels per sample).  A byte is <= 255, so one pixel adds at most 255^2 = 65025 to a sum.
//   per thread, 32 bits:  a thread visits at most ceil(2^28 / (TONE_MAX_BLOCKS * 256)) = 4096 pixels (+ 3 for the vector granule):
//                         4099 * 65025 < 2^29 < 2^31; with fewer blocks a sample has at most blocks * TONE_BLOCK_PIXELS pixels, 4 per thread.
//                         (the general rule: pixels per thread * 65025 must stay below 2^31, i.e. at most 33025 pixels per thread)
//   wave / block, 64 bits: 256 threads * 2^29 < 2^37
//   sample, 64 bits:       the sum of q^2 reaches 2^28 * 65025 < 2^45
static_assert(((long)WIN_MAX_DIM * WIN_MAX_DIM / ((long)TONE_MAX_BLOCKS * 256) + 3) * 65025L < (1L << 31), "a per-thread accumulator could overflow");

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
    return v;
}

// grid (blocks per sample, B).  VEC pixels per load: 4 or 2 only where H * W is a multiple of it and the three tensors start on 16 / 8
// bytes - then every plane base (b * 3 + c) * HW is aligned as well and there is no tail; any other H * W (an odd one leaves the planes
// on 4 bytes) takes VEC = 1, which has no tail either.
template <int VEC>
__global__ void __launch_bounds__(256) tone_stats_kernel(const float* __restrict__ image, const float* __restrict__ result, const float* __restrict__ sel,
                                                         unsigned long long* __restrict__ partial, int HW) {
    typedef typename ToneVec<VEC>::type vec_t;
    const int b = blockIdx.y, nb = gridDim.x;
    const float* ip = image + (size_t)b * 3 * HW;
    const float* rp = result + (size_t)b * 3 * HW;
    const float* sp = sel + (size_t)b * HW;
    unsigned acc[TONE_ACC];
#pragma unroll
    for (int k = 0; k < TONE_ACC; ++k) acc[k] = 0u;
    const int groups = HW / VEC, stride = nb * 256;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += stride) {
        float s[VEC], x[3][VEC], r[3][VEC];
        const vec_t sv = *(const vec_t*)(sp + (size_t)g * VEC);
        __builtin_memcpy(s, &sv, sizeof(sv));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const vec_t xv = *(const vec_t*)(ip + (size_t)c * HW + (size_t)g * VEC), rv = *(const vec_t*)(rp + (size_t)c * HW + (size_t)g * VEC);
            __builtin_memcpy(x[c], &xv, sizeof(xv));
            __builtin_memcpy(r[c], &rv, sizeof(rv));
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            if (!(s[v] >= 0.5f)) continue;                          // a NaN selects nothing
            acc[0] += 1u;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned o = tone_byte_image(x[c][v]), q = tone_byte_result(r[c][v]);
                acc[1 + 5 * c] += o;
                acc[2 + 5 * c] += q;
                acc[3 + 5 * c] += o * o;
                acc[4 + 5 * c] += q * q;
                acc[5 + 5 * c] += o * q;
            }
        }
    }
    __shared__ unsigned long long red[4][TONE_ACC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < TONE_ACC; ++k) {
        const unsigned long long t = wave_sum_u64(acc[k]);
        if (lane == 0) red[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < TONE_ACC)                                     // every block writes its TONE_ACC partials: the workspace needs no clearing
        partial[((size_t)b * nb + blockIdx.x) * TONE_ACC + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// grid B, 4 waves: wave w sums accumulators 4w .. 4w + 3 over the sample's nb block partials (lanes stride over the blocks) in 64 bits and
// writes them; every element of stats[b] is written, n into each of the three rows.
__global__ void __launch_bounds__(256) tone_finalise_kernel(const unsigned long long* __restrict__ partial, long long* __restrict__ stats, int nb) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 4 * wave; k < 4 * wave + 4; ++k) {
        unsigned long long t = 0;
        for (int j = lane; j < nb; j += 64) t += partial[((size_t)b * nb + j) * TONE_ACC + k];
        t = wave_sum_u64(t);
        if (lane != 0) continue;
        long long* row = stats + (size_t)b * 18;
        if (k == 0) {
            row[0] = row[6] = row[12] = (long long)t;
        } else {
            const int c = (k - 1) / 5, j = (k - 1) % 5;
            row[6 * c + 1 + j] = (long long)t;
        }
    }
}

static int tone_blocks(long HW) {
    const long nb = (HW + TONE_BLOCK_PIXELS - 1) / TONE_BLOCK_PIXELS;
    return (int)(nb < TONE_MAX_BLOCKS ? nb : TONE_MAX_BLOCKS);
}
static bool tone_dims_ok(int32_t B, int32_t H, int32_t W) { return B > 0 && B <= TONE_MAX_BATCH && H > 0 && W > 0 && H <= WIN_MAX_DIM && W <= WIN_MAX_DIM; }

extern "C" size_t pbe_tone_stats_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (!tone_dims_ok(B, H, W)) return 0;
    return (size_t)B * (size_t)tone_blocks((long)H * W) * TONE_ACC * sizeof(unsigned long long);
}
extern "C" int pbe_tone_stats_i64(const float* image, const float* result, const float* sel, int64_t* stats, int32_t B, int32_t H, int32_t W,
                                  void* workspace, size_t workspace_bytes, pbe_stream_t stream) {
    PBE_REQUIRE(image && result && sel && stats && workspace && B > 0 && H > 0 && W > 0, "pbe_tone_stats_i64: bad arguments");
    PBE_REQUIRE(H <= WIN_MAX_DIM && W <= WIN_MAX_DIM, "pbe_tone_stats_i64: an edge above %d", WIN_MAX_DIM);
    PBE_REQUIRE(B <= TONE_MAX_BATCH, "pbe_tone_stats_i64: batch %d above %d", B, TONE_MAX_BATCH);
    PBE_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, "pbe_tone_stats_i64: stats and workspace must be 8-byte aligned");
    PBE_REQUIRE(workspace_bytes >= pbe_tone_stats_workspace_bytes(B, H, W), "pbe_tone_stats_i64: workspace of %zu bytes, %zu needed", workspace_bytes,
                pbe_tone_stats_workspace_bytes(B, H, W));
    hipStream_t s = (hipStream_t)stream;
    const long HW = (long)H * W;
    const int nb = tone_blocks(HW);
    const uintptr_t bits = (uintptr_t)image | (uintptr_t)result | (uintptr_t)sel;
    const int vec = (HW % 4 == 0 && (bits & 15) == 0) ? 4 : (HW % 2 == 0 && (bits & 7) == 0) ? 2 : 1;
    unsigned long long* partial = (unsigned long long*)workspace;
    const dim3 grid((unsigned)nb, (unsigned)B);
    EW_BEGIN(s);
    if (vec == 4) hipLaunchKernelGGL(tone_stats_kernel<4>, grid, dim3(256), 0, s, image, result, sel, partial, (int)HW);
    else if (vec == 2) hipLaunchKernelGGL(tone_stats_kernel<2>, grid, dim3(256), 0, s, image, result, sel, partial, (int)HW);
    else hipLaunchKernelGGL(tone_stats_kernel<1>, grid, dim3(256), 0, s, image, result, sel, partial, (int)HW);
    hipLaunchKernelGGL(tone_finalise_kernel, dim3((unsigned)B), dim3(256), 0, s, (const unsigned long long*)partial, (long long*)stats, nb);
    EW_END(s, 28.0 * (double)B * (double)HW, "pbe_tone_stats_i64");
}
