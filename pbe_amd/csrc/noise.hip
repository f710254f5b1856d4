// Noise as a function: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; the Random123 constants) keyed by a per-sample seed.
//   pbe_philox_u32          the raw words
//   pbe_randn_philox_f32    out = a * out + b * z, z standard normal by Box-Muller on the words
// For sample b and element e of its flat array of n:  key = (seed lo32, seed hi32), counter = (q, sub[b], stream lo32, stream hi32) with
// q = e / 4; the call gives x0 .. x3 and elements 4q .. 4q + 3 come from it:
//   u = ((x0 >> 8) + 1) * 2^-24 in (0, 1],  v = (x1 >> 8) * 2^-24 in [0, 1)      both exact in fp32
//   r = sqrtf(-2 logf(u)),  (s, c) = sincospif(2 v)                               the accurate library functions
//   elements 4q, 4q + 1 = r c, r s;  4q + 2, 4q + 3 the same from (x2, x3).
// There is no generator state: an element is a pure function of (seed, sub, stream, e).  It does not depend on B, on the sample's place in
// the batch, on n, or on the alignment of out: one thread owns one counter, normal4() is the only code that computes values, and the
// vector / scalar choice below only decides how the four finished floats are read and stored.  No atomics, no synchronisation, every
// element written exactly once, plain vector stores.  tests/noiseref.py restates all of it in numpy.
#include "common.h"
#include "../../include/pbe_hip.h"

#define EW_BEGIN(s) pbe_prof_begin(PBE_K_ELEM, s)
#define EW_END(s, bytes, name) \
    pbe_prof_end(PBE_K_ELEM, s, bytes); \
    PBE_LAUNCH_CHECK(name); \
    return PBE_OK

#define NOISE_MAX_BATCH 65535              // samples ride on gridDim.y
#define NOISE_MAX_N 0xFFFFFFFCll           // q = e / 4 is one 32-bit counter word, and the grid stays below 2^30 threads per sample

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

struct Words4 { unsigned x[4]; };

__device__ __forceinline__ Words4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const unsigned hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;          // the bump after the last round is dead code
    }
    Words4 w;
    w.x[0] = c0; w.x[1] = c1; w.x[2] = c2; w.x[3] = c3;
    return w;
}

// the sample's words for counter q: seeds / sub are uniform per workgroup (b = blockIdx.y), so these are scalar loads
__device__ __forceinline__ Words4 sample_words(const long long* __restrict__ seeds, const int* __restrict__ sub, int b, unsigned q, unsigned long long stream) {
    const unsigned long long seed = (unsigned long long)seeds[b];
    const unsigned ss = sub ? (unsigned)sub[b] : 0u;
    return philox4x32_10(q, ss, (unsigned)stream, (unsigned)(stream >> 32), (unsigned)seed, (unsigned)(seed >> 32));
}

__device__ __forceinline__ void box_muller(unsigned xa, unsigned xb, float& z0, float& z1) {
    const float u = (float)((xa >> 8) + 1u) * 0x1p-24f;       // <= 2^24: the conversion and the scaling are exact
    const float v = (float)(xb >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u));
    float s, c;
    sincospif(2.0f * v, &s, &c);
    z0 = r * c;
    z1 = r * s;
}

__device__ __forceinline__ void normal4(const Words4& w, float (&z)[4]) {
    box_muller(w.x[0], w.x[1], z[0], z[1]);
    box_muller(w.x[2], w.x[3], z[2], z[3]);
}

// grid (ceil(nq / 256), B), nq = ceil(n / 4): thread q of sample b owns elements 4q .. 4q + 3 of out[b * n ..].  A quad that lies inside n
// and starts on 16 bytes moves as one f32x4 / uint4; any other one (the tail, or a sample base off alignment) as up to four dwords.
template <bool RAW>
__global__ void __launch_bounds__(256) philox_kernel(void* __restrict__ out_, const long long* __restrict__ seeds, const int* __restrict__ sub, long n,
                                                     unsigned long long stream, float a, float bscale) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    const long e0 = 4 * q;
    if (e0 >= n) return;
    const int b = blockIdx.y;
    const Words4 w = sample_words(seeds, sub, b, (unsigned)q, stream);
    const int cnt = n - e0 >= 4 ? 4 : (int)(n - e0);
    if constexpr (RAW) {
        unsigned* o = (unsigned*)out_ + (size_t)b * n + e0;
        if (cnt == 4 && ((uintptr_t)o & 15) == 0) {
            *(uint4*)o = make_uint4(w.x[0], w.x[1], w.x[2], w.x[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) o[k] = w.x[k];
        }
        return;
    }
    float* o = (float*)out_ + (size_t)b * n + e0;
    const bool vec = cnt == 4 && ((uintptr_t)o & 15) == 0;
    float z[4], prev[4] = {0.f, 0.f, 0.f, 0.f}, res[4];
    normal4(w, z);
    if (a != 0.0f) {                                             // uniform: with a == 0 out is never read
        if (vec) {
            const f32x4 p = *(const f32x4*)o;
            prev[0] = p[0]; prev[1] = p[1]; prev[2] = p[2]; prev[3] = p[3];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) prev[k] = o[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) res[k] = __builtin_fmaf(bscale, z[k], a * prev[k]);      // a == 1: the bits of pbe_axpy_f32
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) res[k] = bscale * z[k];
    }
    if (vec) {
        f32x4 r;
        r[0] = res[0]; r[1] = res[1]; r[2] = res[2]; r[3] = res[3];
        *(f32x4*)o = r;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) o[k] = res[k];
    }
}

static int noise_args_ok(const char* name, const void* out, const void* seeds, const void* sub, int32_t B, int64_t n) {
    PBE_REQUIRE(out && seeds && B > 0 && n > 0, "%s: bad arguments", name);
    PBE_REQUIRE(B <= NOISE_MAX_BATCH, "%s: batch %d above %d", name, B, NOISE_MAX_BATCH);
    PBE_REQUIRE(n <= NOISE_MAX_N, "%s: %lld elements per sample above %lld", name, (long long)n, (long long)NOISE_MAX_N);
    PBE_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)seeds & 7) == 0 && ((uintptr_t)sub & 3) == 0, "%s: out / sub must be 4-byte, seeds 8-byte aligned", name);
    return PBE_OK;
}
static dim3 noise_grid(int32_t B, int64_t n) { return dim3((unsigned)(((n + 3) / 4 + 255) / 256), (unsigned)B); }

extern "C" int pbe_philox_u32(uint32_t* out, const int64_t* seeds, const int32_t* sub, int32_t B, int64_t n_words, uint64_t stream_id, pbe_stream_t stream) {
    if (int rc = noise_args_ok("pbe_philox_u32", out, seeds, sub, B, n_words)) return rc;
    hipStream_t s = (hipStream_t)stream;
    EW_BEGIN(s);
    hipLaunchKernelGGL(philox_kernel<true>, noise_grid(B, n_words), dim3(256), 0, s, (void*)out, (const long long*)seeds, (const int*)sub, (long)n_words,
                       (unsigned long long)stream_id, 0.0f, 1.0f);
    EW_END(s, 4.0 * (double)B * (double)n_words, "pbe_philox_u32");
}

extern "C" int pbe_randn_philox_f32(float* out, const int64_t* seeds, const int32_t* sub, int32_t B, int64_t n, uint64_t stream_id, float a, float b,
                                    pbe_stream_t stream) {
    if (int rc = noise_args_ok("pbe_randn_philox_f32", out, seeds, sub, B, n)) return rc;
    hipStream_t s = (hipStream_t)stream;
    EW_BEGIN(s);
    hipLaunchKernelGGL(philox_kernel<false>, noise_grid(B, n), dim3(256), 0, s, (void*)out, (const long long*)seeds, (const int*)sub, (long)n,
                       (unsigned long long)stream_id, a, b);
    EW_END(s, (a != 0.0f ? 8.0 : 4.0) * (double)B * (double)n, "pbe_randn_philox_f32");
}
