// The shape of a mask: the exact squared Euclidean distance map of a mask in integers, and what grows, shrinks, closes, opens and boxes a
// hole with it (pbe_amd.ops.mask_grow / mask_close / mask_open / fill_boxes, pbe_amd.window.shape_mask).
//   pbe_mask_dist2_u8_i32    mask -> d2[y, x] = min(min over the set S of (y - y')^2 + (x - x')^2, rmax^2 + 1); S = the hole pixels
//                            (to_hole = 1) or the non-hole pixels (to_hole = 0) INSIDE the picture: the outside belongs to neither set
//   pbe_mask_from_dist2_u8   d2 -> 255 where d2 <= t2 (above = 0) or d2 > t2 (above = 1), else 0
//   pbe_fill_boxes_u8        rows (ya, yb, xa, xb) -> 255 inside any box, else 0
// The map is separable: with g(y, x') = the distance from (y, x') to the nearest set pixel of column x', min over the set of
// dy^2 + dx^2 = min over x' of (x - x')^2 + g(y, x')^2.  Only values <= rmax^2 are told apart, so g is kept as min(g, rmax + 1) in 16 bits
// (a column whose g exceeds rmax cannot give a value <= rmax^2) and x' runs over |x - x'| <= rmax.  Two launches:
//   1  columns  one thread per column and band of rows: a sweep down and a sweep up, each carrying the count of rows since the last set
//               pixel.  A count saturates at rmax + 1, so a sweep that starts rmax + 1 rows outside its band with the saturated count has
//               the true value when it enters the band: bands are independent, and no thread reads what another wrote.
//   2  rows     one workgroup per 256 pixels of a row: g of the segment and rmax columns on each side in LDS (columns outside the picture
//               hold rmax + 1), then every thread takes taps dx = 0, 1, 2 ... on both sides and stops at dx^2 >= best (no later tap can
//               be smaller) or dx > rmax.  A pixel at distance d of the set takes about d taps, a pixel far from it 2 rmax + 1.
// No atomics; every result is a minimum of integers and does not depend on any order.
#include "common.h"
#include "../../include/pbe_hip.h"

#define SHAPE_MAX_DIM 16384            // as csrc/holes.hip
#define SHAPE_MAX_R 2047               // (rmax + 1)^2 + rmax^2 < 2^24: everything fits an int32
#define SHAPE_MAX_BOXES 4096
#define SEG 256                        // pixels of a row per workgroup of the row pass
#define BAND_MIN 64                    // rows per band of the column pass: max(BAND_MIN, 2 (rmax + 1)), so the lead-in is at most half the work

#define SHAPE_BEGIN(s) pbe_prof_begin(PBE_K_ELEM, s)
#define SHAPE_END(s, bytes, name) \
    pbe_prof_end(PBE_K_ELEM, s, bytes); \
    PBE_LAUNCH_CHECK(name); \
    return PBE_OK

// ---- pbe_mask_dist2_u8_i32 -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) dist2_cols_kernel(const unsigned char* mask, unsigned short* g, int Hs, int Ws, int to_hole, int cap, int band) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= Ws) return;
    const int ya = blockIdx.y * band, yb = min(ya + band, Hs);                           // this thread writes rows ya .. yb - 1 of column x
    const unsigned char* m = mask + x;
    unsigned short* gx = g + x;
    int d = cap;                                                                          // rows since the last set pixel, saturated at cap
    for (int y = max(ya - cap, 0); y < yb; ++y) {
        const bool in_set = (m[(long)y * Ws] >= 128) == (to_hole != 0);
        d = in_set ? 0 : min(d + 1, cap);
        if (y >= ya) gx[(long)y * Ws] = (unsigned short)d;
    }
    d = cap;
    for (int y = min(yb + cap, Hs) - 1; y >= ya; --y) {
        const bool in_set = (m[(long)y * Ws] >= 128) == (to_hole != 0);
        d = in_set ? 0 : min(d + 1, cap);
        if (y < yb) gx[(long)y * Ws] = (unsigned short)min((int)gx[(long)y * Ws], d);     // this thread's own store of the sweep down
    }
}
__global__ void __launch_bounds__(SEG) dist2_rows_kernel(const unsigned short* g, int* d2, int Ws, int rmax) {
    __shared__ unsigned short s[SEG + 2 * SHAPE_MAX_R];
    const int x0 = blockIdx.x * SEG, y = blockIdx.y, tx = threadIdx.x;
    const int n = min(SEG, Ws - x0) + 2 * rmax, cap = rmax + 1;
    const unsigned short* row = g + (long)y * Ws;
    for (int i = tx; i < n; i += SEG) {
        const int c = x0 - rmax + i;
        s[i] = c >= 0 && c < Ws ? row[c] : (unsigned short)cap;
    }
    __syncthreads();
    if (x0 + tx >= Ws) return;
    const int c = rmax + tx, sat = rmax * rmax + 1;
    const int g0 = s[c];
    int best = min(g0 * g0, sat);
    for (int dx = 1; dx <= rmax && dx * dx < best; ++dx) {
        const int a = min((int)s[c - dx], (int)s[c + dx]);
        best = min(best, dx * dx + a * a);
    }
    d2[(long)y * Ws + x0 + tx] = best;
}
static int shape_band(int rmax) { return max(BAND_MIN, 2 * (rmax + 1)); }
extern "C" size_t pbe_mask_dist2_workspace_bytes(int32_t Hs, int32_t Ws) {
    if (Hs <= 0 || Ws <= 0 || Hs > SHAPE_MAX_DIM || Ws > SHAPE_MAX_DIM) return 0;
    return sizeof(unsigned short) * (size_t)Hs * (size_t)Ws;                              // g, one 16-bit count per pixel
}
extern "C" int pbe_mask_dist2_u8_i32(const void* mask, int32_t* d2, int32_t Hs, int32_t Ws, int32_t to_hole, int32_t rmax, void* workspace,
                                     size_t workspace_bytes, pbe_stream_t stream) {
    PBE_REQUIRE(mask && d2 && workspace && Hs > 0 && Ws > 0, "pbe_mask_dist2_u8_i32: bad arguments");
    PBE_REQUIRE(Hs <= SHAPE_MAX_DIM && Ws <= SHAPE_MAX_DIM, "pbe_mask_dist2_u8_i32: an edge above %d", SHAPE_MAX_DIM);
    PBE_REQUIRE(to_hole == 0 || to_hole == 1, "pbe_mask_dist2_u8_i32: to_hole %d is neither 0 nor 1", to_hole);
    PBE_REQUIRE(rmax >= 0 && rmax <= SHAPE_MAX_R, "pbe_mask_dist2_u8_i32: rmax %d outside 0 .. %d", rmax, SHAPE_MAX_R);
    PBE_REQUIRE(workspace_bytes >= pbe_mask_dist2_workspace_bytes(Hs, Ws), "pbe_mask_dist2_u8_i32: workspace of %zu bytes, %zu needed", workspace_bytes,
                pbe_mask_dist2_workspace_bytes(Hs, Ws));
    PBE_REQUIRE(((uintptr_t)workspace & 1) == 0, "pbe_mask_dist2_u8_i32: the workspace must be 2-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int band = shape_band(rmax);
    unsigned short* g = (unsigned short*)workspace;
    SHAPE_BEGIN(s);
    hipLaunchKernelGGL(dist2_cols_kernel, dim3((Ws + 255) / 256, (Hs + band - 1) / band), dim3(256), 0, s, (const unsigned char*)mask, g, Hs, Ws, to_hole, rmax + 1,
                       band);
    hipLaunchKernelGGL(dist2_rows_kernel, dim3((Ws + SEG - 1) / SEG, Hs), dim3(SEG), 0, s, (const unsigned short*)g, d2, Ws, rmax);
    SHAPE_END(s, 11.0 * (double)Hs * (double)Ws, "pbe_mask_dist2_u8_i32");
}

// ---- pbe_mask_from_dist2_u8 ------------------------------------------------------------------------------------------------------------
// four pixels per thread: one 16-byte load and one 4-byte store where both planes are aligned for them, else pixel by pixel
__global__ void __launch_bounds__(256) from_dist2_kernel(const int* d2, unsigned char* out, long total, int t2, int above, int wide) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= total) return;
    if (wide && i + 4 <= total) {
        const int4 v = *reinterpret_cast<const int4*>(d2 + i);
        uchar4 o;
        o.x = ((v.x <= t2) != (above != 0)) ? 255 : 0;
        o.y = ((v.y <= t2) != (above != 0)) ? 255 : 0;
        o.z = ((v.z <= t2) != (above != 0)) ? 255 : 0;
        o.w = ((v.w <= t2) != (above != 0)) ? 255 : 0;
        *reinterpret_cast<uchar4*>(out + i) = o;
        return;
    }
    for (long k = i; k < min(i + 4, total); ++k) out[k] = ((d2[k] <= t2) != (above != 0)) ? 255 : 0;
}
extern "C" int pbe_mask_from_dist2_u8(const int32_t* d2, void* out_mask, int32_t Hs, int32_t Ws, int32_t t2, int32_t above, pbe_stream_t stream) {
    PBE_REQUIRE(d2 && out_mask && Hs > 0 && Ws > 0, "pbe_mask_from_dist2_u8: bad arguments");
    PBE_REQUIRE(Hs <= SHAPE_MAX_DIM && Ws <= SHAPE_MAX_DIM, "pbe_mask_from_dist2_u8: an edge above %d", SHAPE_MAX_DIM);
    PBE_REQUIRE(t2 >= 0, "pbe_mask_from_dist2_u8: the threshold t2 = %d is negative", t2);
    PBE_REQUIRE(above == 0 || above == 1, "pbe_mask_from_dist2_u8: above %d is neither 0 nor 1", above);
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)Hs * Ws;
    const int wide = ((uintptr_t)d2 & 15) == 0 && ((uintptr_t)out_mask & 3) == 0;
    SHAPE_BEGIN(s);
    hipLaunchKernelGGL(from_dist2_kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, s, d2, (unsigned char*)out_mask, total, t2, above, wide);
    SHAPE_END(s, 5.0 * (double)total, "pbe_mask_from_dist2_u8");
}

// ---- pbe_fill_boxes_u8 -----------------------------------------------------------------------------------------------------------------
// One workgroup per 64 x 16 tile.  First its four waves list the boxes that meet the tile, 64 boxes per wave and turn: a ballot of the
// lanes whose box meets it, each such lane storing its box number behind the lanes below it (a list per wave, so nothing is shared and
// no atomic is needed).  Then every thread tests its four pixels against the listed boxes only and stops once all four are inside one.
#define BOX_TW 64
#define BOX_TH 16
#define BOX_LIST (SHAPE_MAX_BOXES / 4)   // a wave sees every fourth group of 64 boxes
__global__ void __launch_bounds__(256) fill_boxes_kernel(const int* boxes, int n, unsigned char* out, int Hs, int Ws) {
    __shared__ unsigned short list[4][BOX_LIST];
    __shared__ int count[4];
    const int lane = threadIdx.x, w = threadIdx.y;
    const int tx0 = blockIdx.x * BOX_TW, ty0 = blockIdx.y * BOX_TH;
    const int tx1 = min(tx0 + BOX_TW, Ws) - 1, ty1 = min(ty0 + BOX_TH, Hs) - 1;
    int have = 0;                                                                         // the same in every lane of the wave
    for (int base = w * 64; base < n; base += 256) {
        const int i = base + lane;
        bool meets = false;
        if (i < n) {
            const int* b = boxes + 4 * (long)i;
            meets = b[0] <= ty1 && b[1] >= ty0 && b[2] <= tx1 && b[3] >= tx0;
        }
        const unsigned long long hits = __ballot(meets);
        if (meets) list[w][have + __popcll(hits & ((1ull << lane) - 1ull))] = (unsigned short)i;
        have += __popcll(hits);
    }
    if (lane == 0) count[w] = have;
    __syncthreads();
    const int x = tx0 + lane;
    if (x >= Ws) return;
    unsigned inside = 0;                                                                  // bit r: the pixel of row ty0 + 4 r + w lies in a box
    for (int l = 0; l < 4 && inside != 15u; ++l)
        for (int k = 0; k < count[l] && inside != 15u; ++k) {
            const int* b = boxes + 4 * (long)list[l][k];
            const int ya = b[0], yb = b[1];
            if (x < b[2] || x > b[3]) continue;
            for (int r = 0; r < 4; ++r) {
                const int y = ty0 + 4 * r + w;
                if (y >= ya && y <= yb) inside |= 1u << r;
            }
        }
    for (int r = 0; r < 4; ++r) {
        const int y = ty0 + 4 * r + w;
        if (y < Hs) out[(long)y * Ws + x] = (inside >> r & 1u) ? 255 : 0;
    }
}
extern "C" int pbe_fill_boxes_u8(const int32_t* boxes, int32_t n, void* out_mask, int32_t Hs, int32_t Ws, pbe_stream_t stream) {
    PBE_REQUIRE(out_mask && Hs > 0 && Ws > 0 && (boxes || n == 0), "pbe_fill_boxes_u8: bad arguments");
    PBE_REQUIRE(Hs <= SHAPE_MAX_DIM && Ws <= SHAPE_MAX_DIM, "pbe_fill_boxes_u8: an edge above %d", SHAPE_MAX_DIM);
    PBE_REQUIRE(n >= 0 && n <= SHAPE_MAX_BOXES, "pbe_fill_boxes_u8: %d boxes, 0 .. %d allowed", n, SHAPE_MAX_BOXES);
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        // The rows live on the device and a bad one must be refused before anything is launched: they are read back (at most 64 KiB)
        // on the caller's stream.  This entry point therefore waits for that stream, unlike its neighbours.
        static thread_local int32_t host[4 * SHAPE_MAX_BOXES];
        hipError_t e = hipMemcpyAsync(host, boxes, sizeof(int32_t) * 4 * (size_t)n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return pbe_set_error(PBE_ELAUNCH, "pbe_fill_boxes_u8: reading the boxes back failed: %s", hipGetErrorString(e));
        for (int i = 0; i < n; ++i) {
            const int32_t* b = host + 4 * i;
            PBE_REQUIRE(0 <= b[0] && b[0] <= b[1] && b[1] < Hs && 0 <= b[2] && b[2] <= b[3] && b[3] < Ws,
                        "pbe_fill_boxes_u8: box %d (ya, yb, xa, xb) = (%d, %d, %d, %d) is not a box inside the %d x %d picture", i, b[0], b[1], b[2], b[3], Hs, Ws);
        }
    }
    SHAPE_BEGIN(s);
    hipLaunchKernelGGL(fill_boxes_kernel, dim3((Ws + BOX_TW - 1) / BOX_TW, (Hs + BOX_TH - 1) / BOX_TH), dim3(64, 4), 0, s, boxes, n, (unsigned char*)out_mask, Hs, Ws);
    SHAPE_END(s, (double)Hs * (double)Ws, "pbe_fill_boxes_u8");
}
