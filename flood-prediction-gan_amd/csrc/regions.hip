// The flood regions of a scene: connected-component labelling, per-component statistics and the sieve
// (floodgan/regions.py; include/floodgan.h: fg_regions_*).  Everything here is integer-exact.
//
// Labelling (fg_regions_label) is union-find over the pixel indices i = y * W + x, three launches whatever the data:
//   1. label_tiles_kernel: one workgroup labels one TH x TW tile in LDS -- every member pixel is united with its
//      left / upper (and, 8-connected, upper diagonal) member neighbours inside the tile -- and writes, per member
//      pixel, the GLOBAL index of its tile-local root into the parent plane (-1 for non-members);
//   2. merge_borders_kernel: one lane per pixel along the tile borders unites the pairs of neighbours that lie in
//      different tiles, on the global parent plane;
//   3. compress_kernel: every member pixel replaces its parent by its root.
// A union always hangs the LARGER root under the smaller index (atomic min), so parent[i] <= i at all times, a
// tree's root is the smallest index of its set, and the final label of a pixel is the smallest index of its
// component -- its first pixel in row-major order -- whatever order the workgroups ran in: the labels are a function of
// the mask alone.
// While workgroups race on the parent plane (launch 2, and the in-place writes of launch 3) every access to it is
// an agent-scope relaxed atomic: a plain load could be served from this CU's L1 or a stale line.  A value read late
// is still a value the word once held, i.e. an ancestor-or-self that is <= the index, which is all the loops
// need.  The kernel boundaries publish each phase to the next; no workgroup ever waits for another.
// Every loop below ends by a strictly decreasing non-negative integer; each states it.
//
// Statistics (fg_regions_stats, fg_regions_table) are two policies of scene_common.hpp's accumulation kernel, which
// holds the loop and its reasons: int32 areas and flags, int64 sums, min / max for the boxes.  An update of the table
// is seven atomic instructions onto one 64-byte row per region.
#include "scene_common.hpp"

namespace {

using namespace fg::scene;

constexpr int TW = 64, TH = 16, TPX = TW * TH;      // a wave reads one 256-byte tile row of a unit-stride source

#define FG_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

// ---- union-find on the global parent plane (agent scope) and on a tile in LDS (workgroup scope)

struct GlobalForest {
    int* parent;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(parent + i, FG_RLX_AGENT); }
    __device__ __forceinline__ int lower(int i, int v) const { return __hip_atomic_fetch_min(parent + i, v, FG_RLX_AGENT); }
};

struct TileForest {
    int* parent;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(parent + i, FG_RLX_WG); }
    __device__ __forceinline__ int lower(int i, int v) const { return __hip_atomic_fetch_min(parent + i, v, FG_RLX_WG); }
};

template <class F>
__device__ __forceinline__ int find_root(const F& f, int x) {
    // variant: x strictly decreases (the step is taken only when 0 <= parent[x] < x)
    for (int p = f.load(x); p >= 0 && p < x; p = f.load(x)) x = p;
    return x;
}

// a and b are members (parent >= 0).  After the call a chain of parents joins them, now or once every unite
// running beside this one has returned.
template <class F>
__device__ __forceinline__ void unite(const F& f, int a, int b) {
    // variant: a + b strictly decreases.  find_root never raises a or b; a failed lower() returns the word's earlier
    // value old with 0 <= old < a (it was not a: a was no root any more) and a takes it.  A lower() that found a
    // linked elsewhere may have cut that link (a -> old became a -> b): going on with (old, b) restores it.
    for (;;) {
        a = find_root(f, a);
        b = find_root(f, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = f.lower(a, b);
        if (old == a || old < 0) return;
        a = old;
    }
}

__global__ void __launch_bounds__(NT) label_tiles_kernel(ClassPlane m, int H, int W, int tiles_x, int conn8,
                                                         int* labels) {
    __shared__ int lab[TPX];
    const TileForest f{lab};
    const int ty0 = (int)(blockIdx.x / tiles_x) * TH, tx0 = (int)(blockIdx.x % tiles_x) * TW;
    for (int i = threadIdx.x; i < TPX; i += NT) {
        const int y = ty0 + i / TW, x = tx0 + i % TW;
        lab[i] = (y < H && x < W && m.member(y, x)) ? i : -1;
    }
    __syncthreads();
    // (a member's word stays >= 0 and a non-member's -1 whatever the unions do: the tests below are stable)
    for (int i = threadIdx.x; i < TPX; i += NT) {
        if (f.load(i) < 0) continue;
        const int ly = i / TW, lx = i % TW;
        if (lx > 0 && f.load(i - 1) >= 0) unite(f, i, i - 1);
        const bool up = ly > 0 && f.load(i - TW) >= 0;
        if (up) unite(f, i, i - TW);
        // with the upper neighbour a member, the upper diagonals are joined to it by their own left / right step
        if (conn8 && ly > 0 && !up) {
            if (lx > 0 && f.load(i - TW - 1) >= 0) unite(f, i, i - TW - 1);
            if (lx < TW - 1 && f.load(i - TW + 1) >= 0) unite(f, i, i - TW + 1);
        }
    }
    __syncthreads();
    // the tile-local root is the tile's first pixel of the set in row-major order, in the tile as in the scene
    for (int i = threadIdx.x; i < TPX; i += NT) {
        const int y = ty0 + i / TW, x = tx0 + i % TW;
        if (y >= H || x >= W) continue;
        int v = -1;
        if (lab[i] >= 0) {
            const int r = find_root(f, i);
            v = (ty0 + r / TW) * W + tx0 + r % TW;
        }
        labels[y * W + x] = v;
    }
}

// nbh = (H - 1) / TH horizontal borders (between rows k TH - 1 and k TH) of W pixels each, then nbv = (W - 1) / TW
// vertical ones of H pixels each: one lane per border pixel unites it with its neighbours across the border
__global__ void __launch_bounds__(NT) merge_borders_kernel(int* labels, int H, int W, int nbh, int nbv, int conn8) {
    const GlobalForest f{labels};
    const long long horiz = (long long)nbh * W, total = horiz + (long long)nbv * H;
    for (long long t = blockIdx.x * (long long)NT + threadIdx.x; t < total; t += (long long)gridDim.x * NT) {
        if (t < horiz) {
            const int y = ((int)(t / W) + 1) * TH, x = (int)(t % W);
            const int p = y * W + x, q = p - W;
            if (f.load(p) < 0) continue;
            const bool up = f.load(q) >= 0;
            if (up) unite(f, p, q);
            // (as in the tile: a member above joins its own row neighbours, here or in the tile's launch)
            if (conn8 && !up) {
                if (x > 0 && f.load(q - 1) >= 0) unite(f, p, q - 1);
                if (x < W - 1 && f.load(q + 1) >= 0) unite(f, p, q + 1);
            }
        } else {
            const long long u = t - horiz;
            const int x = ((int)(u / H) + 1) * TW, y = (int)(u % H);
            const int p = y * W + x, q = p - 1;
            if (f.load(p) < 0) continue;
            if (f.load(q) >= 0) unite(f, p, q);
            if (conn8) {
                if (y > 0 && f.load(q - W) >= 0) unite(f, p, q - W);
                if (y < H - 1 && f.load(q + W) >= 0) unite(f, p, q + W);
            }
        }
    }
}

// in place: a lane that walks through a word another lane has already replaced by its root takes a shortcut
__global__ void __launch_bounds__(NT) compress_kernel(int* labels, long long total) {
    const GlobalForest f{labels};
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int p = f.load((int)i);
        if (p < 0 || p == (int)i) continue;
        __hip_atomic_store(labels + i, find_root(f, p), FG_RLX_AGENT);
    }
}

// ---- statistics: two policies of accumulate_kernel.  Every index that comes out of memory is checked against the
// plane or the table before it is used.

// area[root]: the pixels of the region; border[root]: 1 when one of them lies in the scene's first or last row or column
struct AreaPlanes {
    struct Acc { int root, n, edge; };
    int H, W;
    const int* labels;
    int* area;                  // planes indexed by root
    int* border;
    static __device__ __forceinline__ Acc empty() { return Acc{-1, 0, 0}; }
    __device__ __forceinline__ long long weight(long long) const { return 1; }
    __device__ __forceinline__ void add(Acc& a, int y, int x, long long) const {
        a.n += 1;
        a.edge |= y == 0 || x == 0 || y == H - 1 || x == W - 1;
    }
    static __device__ __forceinline__ void merge(Acc& g, int d) {
        g.n += __shfl_xor(g.n, d);
        g.edge |= __shfl_xor(g.edge, d);
    }
    __device__ __forceinline__ void emit(const Acc& a) const {
        if (a.n <= 0 || (unsigned)a.root >= (unsigned)(H * W)) return;
        __hip_atomic_fetch_add(area + a.root, a.n, FG_RLX_AGENT);
        if (a.edge) __hip_atomic_fetch_or(border + a.root, 1, FG_RLX_AGENT);
    }
};

__device__ __forceinline__ void ll_min(long long* p, long long v) { __hip_atomic_fetch_min(p, v, FG_RLX_AGENT); }
__device__ __forceinline__ void ll_max(long long* p, long long v) { __hip_atomic_fetch_max(p, v, FG_RLX_AGENT); }
__device__ __forceinline__ void ll_add(long long* p, long long v) { __hip_atomic_fetch_add(p, v, FG_RLX_AGENT); }

// table[rank[root]] = {label, area, y0, x0, y1, x1, sum_y, sum_x}
struct BoxTable {
    struct Acc {
        int root, n, y0, x0, y1, x1;
        long long sy, sx;
    };
    int H, W;
    const int* labels;
    const int* rank;            // plane indexed by root
    long long* table;           // [R, 8]
    int R;
    static __device__ __forceinline__ Acc empty() { return Acc{-1, 0, INT_MAX, INT_MAX, -1, -1, 0, 0}; }
    __device__ __forceinline__ long long weight(long long) const { return 1; }
    __device__ __forceinline__ void add(Acc& a, int y, int x, long long) const {
        a.n += 1;
        a.y0 = min(a.y0, y);
        a.x0 = min(a.x0, x);
        a.y1 = max(a.y1, y);
        a.x1 = max(a.x1, x);
        a.sy += y;
        a.sx += x;
    }
    static __device__ __forceinline__ void merge(Acc& g, int d) {
        g.n += __shfl_xor(g.n, d);
        g.y0 = min(g.y0, __shfl_xor(g.y0, d));
        g.x0 = min(g.x0, __shfl_xor(g.x0, d));
        g.y1 = max(g.y1, __shfl_xor(g.y1, d));
        g.x1 = max(g.x1, __shfl_xor(g.x1, d));
        g.sy += __shfl_xor(g.sy, d);
        g.sx += __shfl_xor(g.sx, d);
    }
    __device__ __forceinline__ void emit(const Acc& a) const {
        if (a.n <= 0 || (unsigned)a.root >= (unsigned)(H * W)) return;
        const int r = rank[a.root];
        if ((unsigned)r >= (unsigned)R) return;
        long long* row = table + 8ll * r;
        ll_add(row + 1, a.n);
        ll_min(row + 2, a.y0);
        ll_min(row + 3, a.x0);
        ll_max(row + 4, a.y1);
        ll_max(row + 5, a.x1);
        ll_add(row + 6, a.sy);
        ll_add(row + 7, a.sx);
    }
};

// table[rank[p]] = {p, 0, H, W, -1, -1, 0, 0} at every root p: the neutral row the table launch accumulates into
__global__ void __launch_bounds__(NT) table_init_kernel(BoxTable k) {
    const long long total = (long long)k.H * k.W;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        if (k.labels[i] != (int)i) continue;
        const int r = k.rank[i];
        if ((unsigned)r >= (unsigned)k.R) continue;
        long long* row = k.table + 8ll * r;
        row[0] = i; row[1] = 0; row[2] = k.H; row[3] = k.W; row[4] = -1; row[5] = -1; row[6] = 0; row[7] = 0;
    }
}

// ---- the sieve

__global__ void __launch_bounds__(NT) apply_kernel(const int* labels, const int* area, const int* border, int H, int W,
                                                   int mode, int min_area, float* mask, unsigned long long* counts) {
    const long long total = (long long)H * W;
    int comps = 0, pixels = 0;                          // per wave, on every lane
    for (long long i0 = blockIdx.x * (long long)NT; i0 < total; i0 += (long long)gridDim.x * NT) {
        const long long i = i0 + threadIdx.x;
        bool changed = false, root = false;
        if (i < total) {
            const int lab = labels[i];
            const bool in = (unsigned)lab < (unsigned)total;         // a member whose root indexes the planes
            bool wet;
            if (mode == FG_REGIONS_REMOVE) {                         // labels of the flood class
                changed = in && min_area > 1 && area[lab] < min_area;
                wet = lab >= 0 && !changed;
            } else {                                                 // labels of the dry class
                changed = in && min_area > 0 && area[lab] < min_area && border[lab] == 0;
                wet = lab < 0 || changed;
            }
            root = changed && lab == (int)i;
            mask[i] = wet ? 1.f : 0.f;
        }
        pixels += __popcll(__ballot(changed));
        comps += __popcll(__ballot(root));
    }
    if ((threadIdx.x & 63) == 0 && pixels) {
        atomicAdd(counts, (unsigned long long)comps);
        atomicAdd(counts + 1, (unsigned long long)pixels);
    }
}

}  // namespace

FG_API int fg_regions_label(fg_sview src, int H, int W, int kind, int target, int connectivity, int* labels,
                            hipStream_t stream) {
    const char* who = "fg_regions_label";
    if (!src.ptr || !labels) return fg::fail(FG_ERR_INVALID, "%s: null source or labels", who);
    if (int e = check_scene(who, H, W)) return e;
    if (int e = check_class(who, kind, target)) return e;
    if (connectivity != 4 && connectivity != 8)
        return fg::fail(FG_ERR_INVALID, "%s: connectivity %d (4 or 8)", who, connectivity);
    if (!aligned(src.ptr, 4) || !aligned(labels, 4))
        return fg::fail(FG_ERR_INVALID, "%s: source and labels must be 4-byte aligned", who);
    // the dry class takes the complementary connectivity
    const int conn8 = (connectivity == 8) == (target == 1);
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int nbh = (H - 1) / TH, nbv = (W - 1) / TW;
    const long long total = (long long)H * W, border = (long long)nbh * W + (long long)nbv * H;
    hipLaunchKernelGGL(label_tiles_kernel, dim3((unsigned)(tiles_x * (long long)tiles_y)), dim3(NT), 0, stream,
                       ClassPlane{src.ptr, src.sy, src.sx, kind, target}, H, W, tiles_x, conn8, labels);
    if (border > 0)
        hipLaunchKernelGGL(merge_borders_kernel, dim3(fg::blocks_for(border, NT, 4096)), dim3(NT), 0, stream, labels,
                           H, W, nbh, nbv, conn8);
    hipLaunchKernelGGL(compress_kernel, dim3(fg::blocks_for(total, NT, 4096)), dim3(NT), 0, stream, labels, total);
    return fg::launched("regions_label");
}

FG_API int fg_regions_stats(const int* labels, int H, int W, int* area, int* border, hipStream_t stream) {
    const char* who = "fg_regions_stats";
    if (!labels || !area || !border) return fg::fail(FG_ERR_INVALID, "%s: null labels, area or border plane", who);
    if (int e = check_scene(who, H, W)) return e;
    if (!aligned(labels, 4) || !aligned(area, 4) || !aligned(border, 4))
        return fg::fail(FG_ERR_INVALID, "%s: the planes must be 4-byte aligned", who);
    const size_t bytes = sizeof(int) * (size_t)H * W;
    if (hipMemsetAsync(area, 0, bytes, stream) != hipSuccess || hipMemsetAsync(border, 0, bytes, stream) != hipSuccess)
        return fg::fail(FG_ERR_INVALID, "%s: clearing the planes failed", who);
    launch_accumulate(AreaPlanes{H, W, labels, area, border}, stream);
    return fg::launched("regions_stats");
}

FG_API int fg_regions_table(const int* labels, const int* rank, int H, int W, long long* table, int R,
                            hipStream_t stream) {
    const char* who = "fg_regions_table";
    if (!labels || !rank || !table) return fg::fail(FG_ERR_INVALID, "%s: null labels, rank plane or table", who);
    if (int e = check_scene(who, H, W)) return e;
    if (R <= 0 || R > (long long)H * W)
        return fg::fail(FG_ERR_INVALID, "%s: %d regions in a scene of %d x %d", who, R, H, W);
    if (!aligned(labels, 4) || !aligned(rank, 4) || !aligned(table, 8))
        return fg::fail(FG_ERR_INVALID, "%s: labels and ranks must be 4-byte, the table 8-byte aligned", who);
    const BoxTable k{H, W, labels, rank, table, R};
    hipLaunchKernelGGL(table_init_kernel, dim3(fg::blocks_for((long long)H * W, NT, 4096)), dim3(NT), 0, stream, k);
    launch_accumulate(k, stream);
    return fg::launched("regions_table");
}

FG_API int fg_regions_apply(const int* labels, const int* area, const int* border, int H, int W, int mode,
                            int min_area, float* mask, unsigned long long* counts, hipStream_t stream) {
    const char* who = "fg_regions_apply";
    if (!labels || !mask || !counts) return fg::fail(FG_ERR_INVALID, "%s: null labels, mask or counts", who);
    if (int e = check_scene(who, H, W)) return e;
    if (mode != FG_REGIONS_REMOVE && mode != FG_REGIONS_FILL)
        return fg::fail(FG_ERR_INVALID, "%s: mode %d (FG_REGIONS_REMOVE or FG_REGIONS_FILL)", who, mode);
    if (min_area < 0) return fg::fail(FG_ERR_INVALID, "%s: min_area %d is negative", who, min_area);
    const bool active = mode == FG_REGIONS_REMOVE ? min_area > 1 : min_area > 0;
    if (active && (!area || (mode == FG_REGIONS_FILL && !border)))
        return fg::fail(FG_ERR_INVALID, "%s: min_area %d needs the area plane%s", who, min_area,
                        mode == FG_REGIONS_FILL ? " and the border plane" : "");
    if (!aligned(labels, 4) || !aligned(mask, 4) || !aligned(counts, 8) || (area && !aligned(area, 4)) ||
        (border && !aligned(border, 4)))
        return fg::fail(FG_ERR_INVALID, "%s: planes must be 4-byte, counts 8-byte aligned", who);
    if (hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), stream) != hipSuccess)
        return fg::fail(FG_ERR_INVALID, "%s: clearing the counts failed", who);
    hipLaunchKernelGGL(apply_kernel, dim3(fg::blocks_for((long long)H * W, NT, 4096)), dim3(NT), 0, stream, labels, area,
                       border, H, W, mode, active ? min_area : 0, mask, counts);
    return fg::launched("regions_apply");
}
