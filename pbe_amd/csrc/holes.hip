// Holes of a mask: connected-component labelling on the device and what the per-hole planner (pbe_amd/window.py, plan_holes) needs of it.
//   pbe_mask_components_u8_i32   mask -> labels: -1 off the hole, else the smallest linear index y * Ws + x of the pixel's component
//   pbe_component_boxes_i32      labels -> count and one row (label, ya, yb, xa, xb, area) per component
//   pbe_select_components_u8     labels + an ascending list of labels -> the u8 mask (255 / 0) of those components
// Labelling is a union-find whose parent array IS the label plane: parent[i] <= i always, a root has parent[i] == i, and every link goes
// from a root to a smaller index of the same component, so the root a set ends with is its smallest index whatever the order of the
// atomics.  Three launches:
//   1  tiles    each 64 x 16 tile in LDS: link every hole pixel to its left / upper (and, at 8, upper diagonal) neighbours inside the
//               tile, flatten, write the tile-local root as a picture index (raster order in the tile = raster order in the picture)
//   2  borders  pixels on a tile's first row, first and last column: the same links across the tile border, in global memory
//   3  flatten  every pixel follows its chain to the root
// A link is a lock-free loop: find both roots, atomicMin the larger root's parent to the smaller; when another thread was faster the
// loop goes on from the value the atomic returned, which is smaller.  Every step moves to a smaller index, so it ends; no workgroup waits
// for another.  A find may read a parent that another compute die has since lowered: an old parent is still a member of the same set
// above the root, so the walk only gets longer; what decides is the value atomicMin returns, and that is the word's true one.
#include "common.h"
#include "../../include/pbe_hip.h"

#define HOLES_MAX_DIM 16384            // as csrc/window.hip: Hs * Ws <= 2^28 fits an int32 index
#define HOLES_MAX_WANTED 4096
#define HOLES_MAX_CAPACITY (1 << 20)
#define TILE_W 64                      // one wave per tile row: 64-byte mask reads, 256-byte label writes
#define TILE_H 16

#define HOLES_BEGIN(s) pbe_prof_begin(PBE_K_ELEM, s)
#define HOLES_END(s, bytes, name) \
    pbe_prof_end(PBE_K_ELEM, s, bytes); \
    PBE_LAUNCH_CHECK(name); \
    return PBE_OK

// ---- union-find on an int array in LDS (Agent = false) or global memory (Agent = true) -----------------------------------------------
template <bool Agent>
__device__ __forceinline__ int uf_load(const int* p) {
    return Agent ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool Agent>
__device__ __forceinline__ int uf_find(const int* L, int i) {
    for (int p = uf_load<Agent>(L + i); p != i; p = uf_load<Agent>(L + i)) i = p;        // p < i: the walk descends
    return i;
}
template <bool Agent>
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
    for (;;) {
        a = uf_find<Agent>(L, a);
        b = uf_find<Agent>(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }                                     // a: the larger root, to be linked below b
        const int old = atomicMin(L + a, b);
        if (old == a) return;                                                             // a was still a root: linked
        a = old;                                                                          // somebody linked a first, to old < a: join old and b
    }
}

// ---- pbe_mask_components_u8_i32 --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TILE_W * TILE_H) holes_tile_kernel(const unsigned char* mask, int* labels, int Hs, int Ws, int conn8) {
    __shared__ int s[TILE_W * TILE_H];
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * TILE_W + tx;
    const int x = blockIdx.x * TILE_W + tx, y = blockIdx.y * TILE_H + ty;
    const bool in = x < Ws && y < Hs;
    const bool hole = in && mask[(long)y * Ws + x] >= 128;
    s[t] = hole ? t : -1;
    __syncthreads();
    if (hole) {
        if (tx > 0 && s[t - 1] >= 0) uf_union<false>(s, t, t - 1);
        if (ty > 0) {
            const bool up = s[t - TILE_W] >= 0;
            if (up) uf_union<false>(s, t, t - TILE_W);
            else if (conn8) {                                                             // next to a hole pixel above, the diagonals add nothing
                if (tx > 0 && s[t - TILE_W - 1] >= 0) uf_union<false>(s, t, t - TILE_W - 1);
                if (tx < TILE_W - 1 && s[t - TILE_W + 1] >= 0) uf_union<false>(s, t, t - TILE_W + 1);
            }
        }
    }
    __syncthreads();
    if (!in) return;
    int lab = -1;
    if (hole) {
        const int r = uf_find<false>(s, t);
        lab = (blockIdx.y * TILE_H + r / TILE_W) * Ws + blockIdx.x * TILE_W + r % TILE_W;
    }
    labels[(long)y * Ws + x] = lab;
}
__global__ void __launch_bounds__(256) holes_border_kernel(int* labels, int Hs, int Ws, int conn8) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= Ws || y >= Hs) return;
    const int cx = x % TILE_W;
    const bool top = y % TILE_H == 0 && y > 0, left = cx == 0 && x > 0, right = cx == TILE_W - 1 && x + 1 < Ws;
    if (!top && !left && !(right && conn8 && y > 0)) return;                              // an interior pixel: nothing crosses a border
    const int i = y * Ws + x;
    if (uf_load<true>(labels + i) < 0) return;
    if (left && uf_load<true>(labels + i - 1) >= 0) uf_union<true>(labels, i, i - 1);
    if (y == 0) return;
    const bool up = uf_load<true>(labels + i - Ws) >= 0;
    if (top && up) {
        // the pixel to the left makes the same link when it and the one above it are hole pixels of these two tiles
        const bool dup = cx != 0 && uf_load<true>(labels + i - 1) >= 0 && uf_load<true>(labels + i - Ws - 1) >= 0;
        if (!dup) uf_union<true>(labels, i, i - Ws);
    }
    if (!conn8) return;
    // a diagonal neighbour in the tile of a hole pixel straight above is already joined to it by pass 1
    if (x > 0 && (top || left) && !(up && cx != 0) && uf_load<true>(labels + i - Ws - 1) >= 0) uf_union<true>(labels, i, i - Ws - 1);
    if (x + 1 < Ws && (top || right) && !(up && cx != TILE_W - 1) && uf_load<true>(labels + i - Ws + 1) >= 0) uf_union<true>(labels, i, i - Ws + 1);
}
__global__ void __launch_bounds__(256) holes_flatten_kernel(int* labels, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int l = labels[i];
    if (l < 0) return;
    for (int p = labels[l]; p != l; p = labels[l]) l = p;                                 // a concurrent write stores this same root
    labels[i] = l;
}
extern "C" size_t pbe_mask_components_workspace_bytes(int32_t Hs, int32_t Ws) {
    (void)Hs; (void)Ws;
    return 16;                                                                            // the label plane is the only state; kept for the ABI
}
extern "C" int pbe_mask_components_u8_i32(const void* mask, int32_t* labels, int32_t Hs, int32_t Ws, int32_t connectivity, void* workspace,
                                          size_t workspace_bytes, pbe_stream_t stream) {
    PBE_REQUIRE(mask && labels && workspace && Hs > 0 && Ws > 0, "pbe_mask_components_u8_i32: bad arguments");
    PBE_REQUIRE(Hs <= HOLES_MAX_DIM && Ws <= HOLES_MAX_DIM, "pbe_mask_components_u8_i32: an edge above %d", HOLES_MAX_DIM);
    PBE_REQUIRE(connectivity == 8 || connectivity == 4, "pbe_mask_components_u8_i32: connectivity %d is neither 8 nor 4", connectivity);
    PBE_REQUIRE(workspace_bytes >= pbe_mask_components_workspace_bytes(Hs, Ws), "pbe_mask_components_u8_i32: workspace of %zu bytes, %zu needed",
                workspace_bytes, pbe_mask_components_workspace_bytes(Hs, Ws));
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)Hs * Ws;
    const int c8 = connectivity == 8;
    HOLES_BEGIN(s);
    hipLaunchKernelGGL(holes_tile_kernel, dim3((Ws + TILE_W - 1) / TILE_W, (Hs + TILE_H - 1) / TILE_H), dim3(TILE_W, TILE_H), 0, s,
                       (const unsigned char*)mask, labels, Hs, Ws, c8);
    hipLaunchKernelGGL(holes_border_kernel, dim3((Ws + 63) / 64, (Hs + 3) / 4), dim3(64, 4), 0, s, labels, Hs, Ws, c8);
    hipLaunchKernelGGL(holes_flatten_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, labels, total);
    HOLES_END(s, 13.0 * (double)total, "pbe_mask_components_u8_i32");
}

// ---- pbe_component_boxes_i32 -----------------------------------------------------------------------------------------------------------
// workspace: an open-addressing table label -> row of at least 2 * capacity slots (keys, then rows).  Pass 1 gives every root pixel
// (labels[i] == i) a row number by one atomicAdd on *count and, below capacity, enters it with ya = its own row (the smallest index of a
// component lies in its first row).  In pass 2 a wave walks 16 picture rows of 64 columns.  Per row the lanes that share a label form a
// group: its lowest and highest lane are the group's xa and xb, its population the area.  The wave keeps the sums of ONE label - the
// first it meets - in registers over its 16 rows and adds them to the table once, with four atomics; groups of other labels are added
// row by row.  A hole of a million pixels thus makes about a thousand times fewer atomics than it has pixels.
struct BoxTable {
    int* keys;
    int* rows;
    unsigned mask;
};
__device__ __forceinline__ unsigned box_hash(int label, unsigned mask) { return ((unsigned)label * 2654435761u >> 7) & mask; }
static unsigned box_slots(int capacity) {
    unsigned n = 64;
    while (n < 2u * (unsigned)capacity) n <<= 1;
    return n;
}
__global__ void __launch_bounds__(256) boxes_init_kernel(BoxTable t, int* count) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i <= t.mask) t.keys[i] = -1;
    if (i == 0) *count = 0;
}
__global__ void __launch_bounds__(256) boxes_roots_kernel(const int* labels, int* table, int* count, BoxTable t, int Hs, int Ws, int capacity) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Hs * Ws || labels[i] != (int)i) return;
    const int row = atomicAdd(count, 1);
    if (row >= capacity) return;
    int* r = table + 6 * (long)row;
    r[0] = (int)i; r[1] = (int)(i / Ws); r[2] = -1; r[3] = Ws; r[4] = -1; r[5] = 0;           // ya: the root is the component's first pixel
    for (unsigned h = box_hash((int)i, t.mask);; h = (h + 1) & t.mask)                    // at most capacity entries in >= 2 capacity slots: a free one exists
        if (atomicCAS(t.keys + h, -1, (int)i) == -1) {
            t.rows[h] = row;
            return;
        }
}
// one lane adds (yb, xa, xb, area) of some pixels of component `label` to its row; ya needs no atomic: it is the row of the root pixel
__device__ __forceinline__ void box_flush(int* table, const BoxTable& t, int label, int yb, int xa, int xb, int area) {
    unsigned h = box_hash(label, t.mask), n = 0;                                          // entered by pass 1; the probe is bounded all the same, so
    while (t.keys[h] != label && n <= t.mask) { h = (h + 1) & t.mask; ++n; }              // that a plane that is no label plane cannot hang it
    if (t.keys[h] != label) return;
    int* r = table + 6 * (long)t.rows[h];
    atomicMax(r + 2, yb);
    atomicMin(r + 3, xa); atomicMax(r + 4, xb);
    atomicAdd(r + 5, area);
}
#define BOX_ROWS 16                    // picture rows per wave
__global__ void __launch_bounds__(256) boxes_reduce_kernel(const int* labels, int* table, const int* count, BoxTable t, int Hs, int Ws, int capacity) {
    if (*count > capacity) return;                                                        // the table is unspecified then: leave it
    const int x0 = blockIdx.x * 64, x = x0 + threadIdx.x;
    const int y_begin = (blockIdx.y * 4 + threadIdx.y) * BOX_ROWS, y_end = min(y_begin + BOX_ROWS, Hs);
    int cur = -1, c_yb = 0, c_xa = 0, c_xb = 0, c_area = 0;                               // the label this wave is collecting, the same in every lane
    for (int y = y_begin; y < y_end; ++y) {
        const int lab = x < Ws ? labels[(long)y * Ws + x] : -1;
        unsigned long long todo = __ballot(lab >= 0);
        while (todo) {                                                                    // one turn per distinct label of the row's 64 pixels
            const int first = __ffsll((long long)todo) - 1;
            const int want = __shfl(lab, first);
            const unsigned long long grp = __ballot(lab == want);
            todo &= ~grp;
            const int xa = x0 + first, xb = x0 + 63 - __clzll((long long)grp), n = __popcll(grp);
            if (cur < 0) { cur = want; c_yb = y; c_xa = xa; c_xb = xb; c_area = 0; }
            if (want == cur) {
                c_yb = y; c_xa = min(c_xa, xa); c_xb = max(c_xb, xb); c_area += n;
            } else if (threadIdx.x == 0) {                                                // (no `continue`: the wave meets whole at the next ballot)
                box_flush(table, t, want, y, xa, xb, n);
            }
        }
    }
    if (cur >= 0 && threadIdx.x == 0) box_flush(table, t, cur, c_yb, c_xa, c_xb, c_area);
}
extern "C" size_t pbe_component_boxes_workspace_bytes(int32_t Hs, int32_t Ws, int32_t capacity) {
    if (Hs <= 0 || Ws <= 0 || capacity <= 0 || capacity > HOLES_MAX_CAPACITY) return 0;
    return 2 * sizeof(int) * (size_t)box_slots(capacity);
}
extern "C" int pbe_component_boxes_i32(const int32_t* labels, int32_t* table, int32_t* count, int32_t Hs, int32_t Ws, int32_t capacity, void* workspace,
                                       size_t workspace_bytes, pbe_stream_t stream) {
    PBE_REQUIRE(labels && table && count && workspace && Hs > 0 && Ws > 0, "pbe_component_boxes_i32: bad arguments");
    PBE_REQUIRE(Hs <= HOLES_MAX_DIM && Ws <= HOLES_MAX_DIM, "pbe_component_boxes_i32: an edge above %d", HOLES_MAX_DIM);
    PBE_REQUIRE(capacity >= 1 && capacity <= HOLES_MAX_CAPACITY, "pbe_component_boxes_i32: capacity %d outside 1 .. %d", capacity, HOLES_MAX_CAPACITY);
    PBE_REQUIRE(workspace_bytes >= pbe_component_boxes_workspace_bytes(Hs, Ws, capacity), "pbe_component_boxes_i32: workspace of %zu bytes, %zu needed",
                workspace_bytes, pbe_component_boxes_workspace_bytes(Hs, Ws, capacity));
    const unsigned slots = box_slots(capacity);
    BoxTable t = {(int*)workspace, (int*)workspace + slots, slots - 1};
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)Hs * Ws;
    HOLES_BEGIN(s);
    hipLaunchKernelGGL(boxes_init_kernel, dim3((slots + 255) / 256), dim3(256), 0, s, t, count);
    hipLaunchKernelGGL(boxes_roots_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, labels, table, count, t, Hs, Ws, capacity);
    hipLaunchKernelGGL(boxes_reduce_kernel, dim3((Ws + 63) / 64, (Hs + 4 * BOX_ROWS - 1) / (4 * BOX_ROWS)), dim3(64, 4), 0, s, labels, table, (const int*)count, t, Hs, Ws, capacity);
    HOLES_END(s, 8.0 * (double)total, "pbe_component_boxes_i32");
}

// ---- pbe_select_components_u8 ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) select_components_kernel(const int* labels, const int* wanted, int n, unsigned char* out, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int lab = labels[i];
    bool hit = false;
    if (lab >= 0) {
        int lo = 0, hi = n;                                                               // the first entry >= lab in the ascending list
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (wanted[mid] < lab) lo = mid + 1; else hi = mid;
        }
        hit = lo < n && wanted[lo] == lab;
    }
    out[i] = hit ? 255 : 0;
}
extern "C" int pbe_select_components_u8(const int32_t* labels, const int32_t* wanted, int32_t n_wanted, void* out_mask, int32_t Hs, int32_t Ws,
                                        pbe_stream_t stream) {
    PBE_REQUIRE(labels && out_mask && Hs > 0 && Ws > 0 && (wanted || n_wanted == 0), "pbe_select_components_u8: bad arguments");
    PBE_REQUIRE(Hs <= HOLES_MAX_DIM && Ws <= HOLES_MAX_DIM, "pbe_select_components_u8: an edge above %d", HOLES_MAX_DIM);
    PBE_REQUIRE(n_wanted >= 0 && n_wanted <= HOLES_MAX_WANTED, "pbe_select_components_u8: %d labels wanted, 0 .. %d allowed", n_wanted, HOLES_MAX_WANTED);
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)Hs * Ws;
    HOLES_BEGIN(s);
    hipLaunchKernelGGL(select_components_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, labels, wanted, n_wanted, (unsigned char*)out_mask, total);
    HOLES_END(s, 5.0 * (double)total, "pbe_select_components_u8");
}
