// Windowed pre/post-processing: inpaint a region of a uint8 picture of any size and paste it back in place.
//   pbe_window_image_u8_f32   window of the picture -> normalised fp32 planes at the working size (antialiased triangle filter)
//   pbe_window_mask_u8_f32    window of the mask    -> keep plane in {0, 1} at the working size (integer footprint rule, no filter)
//   pbe_feather_alpha_f32     mask + window + r     -> alpha = box_r(dilate_r(hole)) / (2r+1)^2 on the window (separable integer passes)
//   pbe_paste_window_u8       result + alpha        -> the picture's bytes, in place, where alpha > 0
//   pbe_paste_window_tone_u8  the same with res = gain * res + offset per channel before the blend (the tone map of csrc/tone.hip's statistics)
//   pbe_paste_window_field_u8 the same with res += the coarse difference field of csrc/tone_field.hip, sampled bilinearly
// One thread per output pixel (all three channels), 256 threads per block.  No per-thread arrays: filter weights are recomputed per
// tap from integers, so any scale goes (pbe_resize_bilinear_f32 keeps 64 weights in registers and stops at scale 31).  Every fused
// multiply-add is written as fmaf and no other product feeds a sum, so the arithmetic does not depend on -ffp-contract and
// tests/windowref.py restates it op for op.
#include "common.h"
#include "../../include/pbe_hip.h"

#define EW_GRID(n) dim3((unsigned)(((n) + 255) / 256))
#define EW_BEGIN(s) pbe_prof_begin(PBE_K_ELEM, s)
#define EW_END(s, bytes, name) \
    pbe_prof_end(PBE_K_ELEM, s, bytes); \
    PBE_LAUNCH_CHECK(name); \
    return PBE_OK

#define WIN_MAX_DIM 16384              // picture / working-size edge: the resampler's integers and every launch stay below 2^31
#define WIN_MAX_FEATHER 2047           // (2r+1)^2 <= 2^24: the count and its divisor are exact in fp32

// ---- the shared resampler: the filter of ATen's upsample_bilinear2d_aa (what pbe_resize_bilinear_f32 computes) -----------------------
// One axis, n_in -> n_out samples, output index o.  That filter has scale s = n_in / n_out, support sup = max(s, 1), centre
// c = s (o + 0.5), taps lo = max((int)(c - sup + 0.5), 0) .. min((int)(c + sup + 0.5), n_in) - 1 and weights
// max(1 - |j + 0.5 - c| / sup, 0) normalised by their sum.  Multiplied through by den = 2 max(n_in, n_out) everything is an integer:
//   weight_j * den = max(den - |(2j + 1) n_out - (2o + 1) n_in|, 0) = wnum_j,   normalised weight = (float)wnum_j / (float)sum_j wnum_j
// so the tap range and the weights carry no coordinate rounding at any scale or picture size (one conversion and one IEEE division per
// weight), and at n_in = n_out the weights are exactly 1 and 0.  Edges <= 16384 keep every integer below 2^31.
struct AaAxis {
    int lo, n;
    int n_out, cnum, den;          // cnum = (2o + 1) n_in
    float wsum;                    // (float) sum of wnum over the taps
};
__device__ __forceinline__ int aa_wnum(const AaAxis& a, int j) {
    const int d = (2 * (j + a.lo) + 1) * a.n_out - a.cnum;
    return max(a.den - abs(d), 0);
}
__device__ __forceinline__ float aa_weight(const AaAxis& a, int j) { return (float)aa_wnum(a, j) / a.wsum; }
__device__ __forceinline__ AaAxis aa_axis(int o, int n_in, int n_out) {
    AaAxis a;
    a.n_out = n_out;
    a.cnum = (2 * o + 1) * n_in;
    a.den = 2 * max(n_in, n_out);
    a.lo = max((a.cnum - a.den + n_out) / (2 * n_out), 0);            // a negative numerator truncates towards 0: 0 either way
    a.n = min((a.cnum + a.den + n_out) / (2 * n_out), n_in) - a.lo;
    int tw = 0;
    for (int j = 0; j < a.n; ++j) tw += aa_wnum(a, j);
    a.wsum = (float)tw;                                               // > 0: the tap under the centre has wnum >= den / 2
    return a;
}
// out[c] = sum_k wy_k * (sum_j src(lo_y + k, lo_x + j)[c] * wx_j): row sums first, then the column combination, each accumulated in
// tap order with one fmaf per tap (r = fmaf(v, wx, r); acc = fmaf(r, wy, acc)).  Src::load(y, x, v[3]) returns the three channels of one source pixel; taps never leave [0, Hin) x [0, Win).
template <class Src>
__device__ __forceinline__ void aa_resample3(const Src& src, int oy, int ox, int Hin, int Win, int Hout, int Wout, float out[3]) {
    const AaAxis ay = aa_axis(oy, Hin, Hout), ax = aa_axis(ox, Win, Wout);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < ay.n; ++k) {
        const float wy = aa_weight(ay, k);
        float r[3] = {0.f, 0.f, 0.f};
        for (int j = 0; j < ax.n; ++j) {
            const float wx = aa_weight(ax, j);
            float v[3];
            src.load(ay.lo + k, ax.lo + j, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = fmaf(v[c], wx, r[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = fmaf(r[c], wy, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = acc[c];
}

// a window of a uint8 HWC picture as v / 255: lut[b] = (float)b / 255.0f (256 IEEE divisions per block in place of one per tap and channel)
struct SrcU8Window {
    const unsigned char* p;        // the window's first byte
    long pitch;                    // bytes per picture row
    const float* lut;
    __device__ __forceinline__ void load(int y, int x, float v[3]) const {
        const unsigned char* q = p + (long)y * pitch + (long)x * 3;
        v[0] = lut[q[0]]; v[1] = lut[q[1]]; v[2] = lut[q[2]];
    }
};
// fp32 planes [3, H, W]
struct SrcF32Planes {
    const float* p;
    int W;
    long HW;
    __device__ __forceinline__ void load(int y, int x, float v[3]) const {
        const float* q = p + (long)y * W + x;
        v[0] = q[0]; v[1] = q[HW]; v[2] = q[2 * HW];
    }
};

// ---- pbe_window_image_u8_f32 -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) window_image_kernel(const unsigned char* pic, float* dst, int Ws, int y0, int x0, int wh, int ww, int H, int W,
                                                           float m0, float m1, float m2, float s0, float s1, float s2) {
    __shared__ float lut[256];
    lut[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
    const long HW = (long)H * W;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;           // over H * W working pixels
    if (i >= HW) return;
    const int oy = (int)(i / W), ox = (int)(i - (long)oy * W);
    const SrcU8Window src = {pic + ((long)y0 * Ws + x0) * 3, (long)Ws * 3, lut};
    float f[3];
    aa_resample3(src, oy, ox, wh, ww, H, W, f);
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = f[c] - mean[c];                                  // the order of u8_to_planes_kernel: subtract, then an IEEE division
        asm volatile("" : "+v"(v));
        dst[c * HW + i] = v / sd[c];
    }
}
extern "C" int pbe_window_image_u8_f32(const void* picture, float* dst, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t wh, int32_t ww,
                                       int32_t H, int32_t W, const float* mean3, const float* std3, pbe_stream_t stream) {
    PBE_REQUIRE(picture && dst && mean3 && std3 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "pbe_window_image_u8_f32: bad arguments");
    PBE_REQUIRE(Hs <= WIN_MAX_DIM && Ws <= WIN_MAX_DIM && H <= WIN_MAX_DIM && W <= WIN_MAX_DIM, "pbe_window_image_u8_f32: an edge above %d", WIN_MAX_DIM);
    PBE_REQUIRE(y0 >= 0 && x0 >= 0 && wh > 0 && ww > 0 && wh <= Hs - y0 && ww <= Ws - x0,
                "pbe_window_image_u8_f32: window (%d, %d, %d, %d) outside the %d x %d picture", y0, x0, wh, ww, Hs, Ws);
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)H * W;
    EW_BEGIN(s);
    hipLaunchKernelGGL(window_image_kernel, EW_GRID(total), dim3(256), 0, s, (const unsigned char*)picture, dst, Ws, y0, x0, wh, ww, H, W,
                       mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    EW_END(s, 3.0 * (double)wh * ww + 12.0 * (double)total, "pbe_window_image_u8_f32");
}

// ---- pbe_window_mask_u8_f32 ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) window_mask_kernel(const unsigned char* mask, float* dst, int Ws, int y0, int x0, int wh, int ww, int H, int W) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;           // over H * W working pixels
    if (i >= (long)H * W) return;
    const int Y = (int)(i / W), X = (int)(i - (long)Y * W);
    const int ya = (int)(((long)Y * wh) / H), yb = (int)((((long)Y + 1) * wh + H - 1) / H);        // rows ya .. yb-1 of the window
    const int xa = (int)(((long)X * ww) / W), xb = (int)((((long)X + 1) * ww + W - 1) / W);
    bool hole = false;
    for (int y = ya; y < yb && !hole; ++y) {
        const unsigned char* row = mask + (long)(y0 + y) * Ws + x0;
        for (int x = xa; x < xb; ++x) hole |= row[x] >= 128;
    }
    dst[i] = hole ? 0.f : 1.f;
}
extern "C" int pbe_window_mask_u8_f32(const void* mask, float* dst, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t wh, int32_t ww,
                                      int32_t H, int32_t W, pbe_stream_t stream) {
    PBE_REQUIRE(mask && dst && Hs > 0 && Ws > 0 && H > 0 && W > 0, "pbe_window_mask_u8_f32: bad arguments");
    PBE_REQUIRE(Hs <= WIN_MAX_DIM && Ws <= WIN_MAX_DIM && H <= WIN_MAX_DIM && W <= WIN_MAX_DIM, "pbe_window_mask_u8_f32: an edge above %d", WIN_MAX_DIM);
    PBE_REQUIRE(y0 >= 0 && x0 >= 0 && wh > 0 && ww > 0 && wh <= Hs - y0 && ww <= Ws - x0,
                "pbe_window_mask_u8_f32: window (%d, %d, %d, %d) outside the %d x %d picture", y0, x0, wh, ww, Hs, Ws);
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)H * W;
    EW_BEGIN(s);
    hipLaunchKernelGGL(window_mask_kernel, EW_GRID(total), dim3(256), 0, s, (const unsigned char*)mask, dst, Ws, y0, x0, wh, ww, H, W);
    EW_END(s, (double)wh * ww + 4.0 * (double)total, "pbe_window_mask_u8_f32");
}

// ---- pbe_feather_alpha_f32 -------------------------------------------------------------------------------------------------------------
// Four separable passes over rectangles of PICTURE coordinates (clamping a coordinate to the picture = replicate padding):
//   1  any_x  [ya2, yb2) x [xa, xb)   hole byte in columns q-r .. q+r                     ya2 .. yb2 = window rows +- 2r, clipped
//   2  any_y  [ya,  yb)  x [xa, xb)   pass 1 in rows p-r .. p+r      = dilate_r(hole)     ya .. yb, xa .. xb = window +- r, clipped
//   3  sum_x  [ya,  yb)  x window     pass 2 at columns clamp(x + dx), dx = -r .. r       (a clamped column counts once per dx)
//   4  sum_y  window                  pass 3 at rows clamp(y + dy), dy = -r .. r;  alpha = (float)count / (float)(2r+1)^2
// A maximum ignores the duplicates replicate padding makes, so passes 1 and 2 visit each picture pixel once.
struct FeatherGeom {
    int Hs, Ws, y0, x0, wh, ww, r;
    int ya2, yb2, ya, yb, xa, xb;
};
__global__ void __launch_bounds__(256) feather_any_x_kernel(const unsigned char* mask, unsigned char* t1, FeatherGeom g) {
    const int nx = g.xb - g.xa;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)(g.yb2 - g.ya2) * nx) return;
    const int p = g.ya2 + (int)(i / nx), q = g.xa + (int)(i % nx);
    const unsigned char* row = mask + (long)p * g.Ws;
    const int lo = max(q - g.r, 0), hi = min(q + g.r, g.Ws - 1);
    bool any = false;
    for (int x = lo; x <= hi && !any; ++x) any = row[x] >= 128;
    t1[i] = any ? 1 : 0;
}
__global__ void __launch_bounds__(256) feather_any_y_kernel(const unsigned char* t1, unsigned char* t2, FeatherGeom g) {
    const int nx = g.xb - g.xa;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)(g.yb - g.ya) * nx) return;
    const int p = g.ya + (int)(i / nx), qi = (int)(i % nx);
    const int lo = max(p - g.r, 0), hi = min(p + g.r, g.Hs - 1);         // inside [ya2, yb2): p lies within r of the window
    bool any = false;
    for (int y = lo; y <= hi && !any; ++y) any = t1[(long)(y - g.ya2) * nx + qi] != 0;
    t2[i] = any ? 1 : 0;
}
__global__ void __launch_bounds__(256) feather_sum_x_kernel(const unsigned char* t2, unsigned short* t3, FeatherGeom g) {
    const int nx = g.xb - g.xa;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)(g.yb - g.ya) * g.ww) return;
    const int pi = (int)(i / g.ww), x = g.x0 + (int)(i % g.ww);
    const unsigned char* row = t2 + (long)pi * nx;
    int n = 0;
    for (int dx = -g.r; dx <= g.r; ++dx) n += row[min(max(x + dx, 0), g.Ws - 1) - g.xa];        // the clamped column lies in [xa, xb)
    t3[i] = (unsigned short)n;
}
__global__ void __launch_bounds__(256) feather_sum_y_kernel(const unsigned short* t3, float* alpha, FeatherGeom g) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)g.wh * g.ww) return;
    const int y = g.y0 + (int)(i / g.ww), xi = (int)(i % g.ww);
    int n = 0;
    for (int dy = -g.r; dy <= g.r; ++dy) n += t3[(long)(min(max(y + dy, 0), g.Hs - 1) - g.ya) * g.ww + xi];
    const int m = 2 * g.r + 1;
    alpha[i] = (float)n / (float)(m * m);
}
static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
extern "C" size_t pbe_feather_alpha_workspace_bytes(int32_t wh, int32_t ww, int32_t r) {
    if (wh <= 0 || ww <= 0 || r < 0) return 0;
    const size_t h2 = (size_t)wh + 4 * (size_t)r, h1 = (size_t)wh + 2 * (size_t)r, w1 = (size_t)ww + 2 * (size_t)r;
    return up16(h2 * w1) + up16(h1 * w1) + up16(2 * h1 * (size_t)ww);
}
extern "C" int pbe_feather_alpha_f32(const void* mask, float* alpha, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t wh, int32_t ww, int32_t r,
                                     void* workspace, size_t workspace_bytes, pbe_stream_t stream) {
    PBE_REQUIRE(mask && alpha && workspace && Hs > 0 && Ws > 0, "pbe_feather_alpha_f32: bad arguments");
    PBE_REQUIRE(Hs <= WIN_MAX_DIM && Ws <= WIN_MAX_DIM, "pbe_feather_alpha_f32: an edge above %d", WIN_MAX_DIM);
    PBE_REQUIRE(r >= 0 && r <= WIN_MAX_FEATHER, "pbe_feather_alpha_f32: feather radius %d outside 0 .. %d", r, WIN_MAX_FEATHER);
    PBE_REQUIRE(y0 >= 0 && x0 >= 0 && wh > 0 && ww > 0 && wh <= Hs - y0 && ww <= Ws - x0,
                "pbe_feather_alpha_f32: window (%d, %d, %d, %d) outside the %d x %d picture", y0, x0, wh, ww, Hs, Ws);
    PBE_REQUIRE(workspace_bytes >= pbe_feather_alpha_workspace_bytes(wh, ww, r), "pbe_feather_alpha_f32: workspace of %zu bytes, %zu needed", workspace_bytes,
                pbe_feather_alpha_workspace_bytes(wh, ww, r));
    FeatherGeom g = {Hs, Ws, y0, x0, wh, ww, r, 0, 0, 0, 0, 0, 0};
    g.ya2 = max(y0 - 2 * r, 0); g.yb2 = min(y0 + wh + 2 * r, Hs);
    g.ya = max(y0 - r, 0); g.yb = min(y0 + wh + r, Hs);
    g.xa = max(x0 - r, 0); g.xb = min(x0 + ww + r, Ws);
    const long nx = g.xb - g.xa, n1 = (long)(g.yb2 - g.ya2) * nx, n2 = (long)(g.yb - g.ya) * nx, n3 = (long)(g.yb - g.ya) * ww, n4 = (long)wh * ww;
    unsigned char* t1 = (unsigned char*)workspace;                        // the clipped rectangles never exceed the unclipped sizes of workspace_bytes
    unsigned char* t2 = t1 + up16((size_t)n1);
    unsigned short* t3 = (unsigned short*)(t2 + up16((size_t)n2));
    hipStream_t s = (hipStream_t)stream;
    EW_BEGIN(s);
    hipLaunchKernelGGL(feather_any_x_kernel, EW_GRID(n1), dim3(256), 0, s, (const unsigned char*)mask, t1, g);
    hipLaunchKernelGGL(feather_any_y_kernel, EW_GRID(n2), dim3(256), 0, s, t1, t2, g);
    hipLaunchKernelGGL(feather_sum_x_kernel, EW_GRID(n3), dim3(256), 0, s, t2, t3, g);
    hipLaunchKernelGGL(feather_sum_y_kernel, EW_GRID(n4), dim3(256), 0, s, t3, alpha, g);
    EW_END(s, 2.0 * n1 + 2.0 * n2 + 4.0 * n3 + 4.0 * n4, "pbe_feather_alpha_f32");
}

// ---- pbe_paste_window_u8, pbe_paste_window_tone_u8, pbe_paste_window_field_u8 ----------------------------------------------------------
// One body for the three.  PASTE_TONE: the resampled result goes through res = fmaf(gain, res, offset) per channel (the affine map of
// pbe_amd.window.fit_tone) before the blend; fmaf(1, res, 0) = res, so tone (1, 0) gives the plain paste's bytes.  PASTE_FIELD:
// res += the coarse field of csrc/tone_field.hip, sampled bilinearly at the window pixel's centre; a zero field gives the plain paste's
// bytes and a constant field b the bytes of tone (1, b), since fmaf(1, res, b) = res + b.  Nothing else differs.
// paste_window_kernel and paste_window_tone_kernel keep their names and arguments: they compile to what they compiled to before.
enum { PASTE_PLAIN = 0, PASTE_TONE = 1, PASTE_FIELD = 2 };
struct FieldGrid {
    const float* p;                // fp32 [3, Hc, Wc]
    int Hc, Wc;
    float sy, sx;                  // cells per window pixel: (float)((double)H / ((double)wh * cell)), the same in x
};
// one axis of the bilinear sample: the cell coordinate of window pixel o's centre, its two clamped cells and the fraction between them
__device__ __forceinline__ void field_axis(int o, float s, int n, int& a, int& b, float& t) {
    const float c = fmaf((float)o + 0.5f, s, -0.5f);
    const float f = floorf(c);
    const int i = (int)f;
    a = min(max(i, 0), n - 1);
    b = min(max(i + 1, 0), n - 1);
    t = c - f;
}
template <int MODE>
__device__ __forceinline__ void paste_window_body(const float* result, const float* alpha, unsigned char* pic, int Ws, int y0, int x0, int wh, int ww, int H, int W,
                                                  const float (&gain)[3], const float (&offset)[3], const FieldGrid& fg) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;           // over wh * ww window pixels
    if (i >= (long)wh * ww) return;
    const float a = alpha[i];
    if (!(a > 0.f)) return;                                        // alpha == 0 (or NaN): the byte is not written
    const int oy = (int)(i / ww), ox = (int)(i - (long)oy * ww);
    const SrcF32Planes src = {result, W, (long)H * W};
    float res[3];
    aa_resample3(src, oy, ox, H, W, wh, ww, res);
    if (MODE == PASTE_TONE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) res[c] = fmaf(gain[c], res[c], offset[c]);
    }
    if (MODE == PASTE_FIELD) {
        int ya, yb, xa, xb;
        float ty, tx;
        field_axis(oy, fg.sy, fg.Hc, ya, yb, ty);
        field_axis(ox, fg.sx, fg.Wc, xa, xb, tx);
        const long plane = (long)fg.Hc * fg.Wc;
#pragma unroll
        for (int c = 0; c < 3; ++c) {                              // along y in the two columns, then along x
            const float* f = fg.p + c * plane;
            const float aa = f[(long)ya * fg.Wc + xa], ba = f[(long)yb * fg.Wc + xa], ab = f[(long)ya * fg.Wc + xb], bb = f[(long)yb * fg.Wc + xb];
            const float ca = fmaf(ty, ba - aa, aa), cb = fmaf(ty, bb - ab, ab);
            res[c] += fmaf(tx, cb - ca, ca);
        }
    }
    unsigned char* d = pic + ((long)(y0 + oy) * Ws + (x0 + ox)) * 3;
    const float keep = 1.f - a;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float o = (float)d[c] / 255.0f;
        float v = fmaf(a, res[c], keep * o);
        v = fminf(fmaxf(v, 0.f), 1.f);
        d[c] = (unsigned char)rintf(255.0f * v);                   // round half to even
    }
}
__global__ void __launch_bounds__(256) paste_window_kernel(const float* result, const float* alpha, unsigned char* pic, int Ws, int y0, int x0, int wh, int ww,
                                                           int H, int W) {
    const float none[3] = {0.f, 0.f, 0.f};
    paste_window_body<PASTE_PLAIN>(result, alpha, pic, Ws, y0, x0, wh, ww, H, W, none, none, FieldGrid{nullptr, 0, 0, 0.f, 0.f});
}
__global__ void __launch_bounds__(256) paste_window_tone_kernel(const float* result, const float* alpha, unsigned char* pic, int Ws, int y0, int x0, int wh, int ww,
                                                                int H, int W, float g0, float g1, float g2, float b0, float b1, float b2) {
    const float gain[3] = {g0, g1, g2}, offset[3] = {b0, b1, b2};
    paste_window_body<PASTE_TONE>(result, alpha, pic, Ws, y0, x0, wh, ww, H, W, gain, offset, FieldGrid{nullptr, 0, 0, 0.f, 0.f});
}
__global__ void __launch_bounds__(256) paste_window_field_kernel(const float* result, const float* alpha, unsigned char* pic, int Ws, int y0, int x0, int wh, int ww,
                                                                 int H, int W, FieldGrid fg) {
    const float none[3] = {0.f, 0.f, 0.f};
    paste_window_body<PASTE_FIELD>(result, alpha, pic, Ws, y0, x0, wh, ww, H, W, none, none, fg);
}
extern "C" int pbe_paste_window_u8(const float* result, const float* alpha, void* picture, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t wh,
                                   int32_t ww, int32_t H, int32_t W, pbe_stream_t stream) {
    PBE_REQUIRE(result && alpha && picture && Hs > 0 && Ws > 0 && H > 0 && W > 0, "pbe_paste_window_u8: bad arguments");
    PBE_REQUIRE(Hs <= WIN_MAX_DIM && Ws <= WIN_MAX_DIM && H <= WIN_MAX_DIM && W <= WIN_MAX_DIM, "pbe_paste_window_u8: an edge above %d", WIN_MAX_DIM);
    PBE_REQUIRE(y0 >= 0 && x0 >= 0 && wh > 0 && ww > 0 && wh <= Hs - y0 && ww <= Ws - x0,
                "pbe_paste_window_u8: window (%d, %d, %d, %d) outside the %d x %d picture", y0, x0, wh, ww, Hs, Ws);
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)wh * ww;
    EW_BEGIN(s);
    hipLaunchKernelGGL(paste_window_kernel, EW_GRID(total), dim3(256), 0, s, result, alpha, (unsigned char*)picture, Ws, y0, x0, wh, ww, H, W);
    EW_END(s, 12.0 * (double)H * W + 10.0 * (double)total, "pbe_paste_window_u8");
}
extern "C" int pbe_paste_window_tone_u8(const float* result, const float* alpha, void* picture, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t wh,
                                        int32_t ww, int32_t H, int32_t W, const float* gain3, const float* offset3, pbe_stream_t stream) {
    PBE_REQUIRE(result && alpha && picture && gain3 && offset3 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "pbe_paste_window_tone_u8: bad arguments");
    PBE_REQUIRE(Hs <= WIN_MAX_DIM && Ws <= WIN_MAX_DIM && H <= WIN_MAX_DIM && W <= WIN_MAX_DIM, "pbe_paste_window_tone_u8: an edge above %d", WIN_MAX_DIM);
    PBE_REQUIRE(y0 >= 0 && x0 >= 0 && wh > 0 && ww > 0 && wh <= Hs - y0 && ww <= Ws - x0,
                "pbe_paste_window_tone_u8: window (%d, %d, %d, %d) outside the %d x %d picture", y0, x0, wh, ww, Hs, Ws);
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)wh * ww;
    EW_BEGIN(s);
    hipLaunchKernelGGL(paste_window_tone_kernel, EW_GRID(total), dim3(256), 0, s, result, alpha, (unsigned char*)picture, Ws, y0, x0, wh, ww, H, W,
                       gain3[0], gain3[1], gain3[2], offset3[0], offset3[1], offset3[2]);
    EW_END(s, 12.0 * (double)H * W + 10.0 * (double)total, "pbe_paste_window_tone_u8");
}
extern "C" int pbe_paste_window_field_u8(const float* result, const float* alpha, void* picture, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0, int32_t wh,
                                         int32_t ww, int32_t H, int32_t W, const float* field, int32_t Hc, int32_t Wc, int32_t cell, pbe_stream_t stream) {
    PBE_REQUIRE(result && alpha && picture && field && Hs > 0 && Ws > 0 && H > 0 && W > 0, "pbe_paste_window_field_u8: bad arguments");
    PBE_REQUIRE(Hs <= WIN_MAX_DIM && Ws <= WIN_MAX_DIM && H <= WIN_MAX_DIM && W <= WIN_MAX_DIM, "pbe_paste_window_field_u8: an edge above %d", WIN_MAX_DIM);
    PBE_REQUIRE(y0 >= 0 && x0 >= 0 && wh > 0 && ww > 0 && wh <= Hs - y0 && ww <= Ws - x0,
                "pbe_paste_window_field_u8: window (%d, %d, %d, %d) outside the %d x %d picture", y0, x0, wh, ww, Hs, Ws);
    PBE_REQUIRE(cell == 4 || cell == 8 || cell == 16 || cell == 32 || cell == 64, "pbe_paste_window_field_u8: cell %d is not one of 4, 8, 16, 32, 64", cell);
    PBE_REQUIRE(Hc == (H + cell - 1) / cell && Wc == (W + cell - 1) / cell, "pbe_paste_window_field_u8: a field of %d x %d cells for a %d x %d result at cell %d", Hc, Wc,
                H, W, cell);
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)wh * ww;
    const FieldGrid fg = {field, Hc, Wc, (float)((double)H / ((double)wh * cell)), (float)((double)W / ((double)ww * cell))};
    EW_BEGIN(s);
    hipLaunchKernelGGL(paste_window_field_kernel, EW_GRID(total), dim3(256), 0, s, result, alpha, (unsigned char*)picture, Ws, y0, x0, wh, ww, H, W, fg);
    EW_END(s, 12.0 * (double)H * W + 10.0 * (double)total + 12.0 * (double)Hc * Wc, "pbe_paste_window_field_u8");
}
