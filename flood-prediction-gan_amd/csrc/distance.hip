// Flood depth of a scene: the exact Euclidean nearest-seed (feature) transform, the shore plane, the depth plane and
// the per-region depth table (floodgan/depth.py; include/floodgan.h: fg_nearest_seed, fg_shore, fg_flood_depth,
// fg_depth_table).  The transform and the table are integer-exact; the depth is one fp32 subtraction.
//
// fg_nearest_seed is separable, three launches whatever the data:
//   1. seed_bits_kernel: one lane per (band of 64 rows, column) packs the seed decisions of its 64 pixels into one
//      64-bit word (bit r = row 64 b + r); adjacent lanes are adjacent columns, so a unit-stride source is read
//      coalesced;
//   2. column_kernel: one lane per (band, column) finds the last seed row above its band and the first below it in
//      the words of the other bands of its column, then for each of its 64 rows the nearest seed row of the column
//      from the bits (ties to the SMALLER row), and writes the column plane col[y][x] (that row, or -1 for a column
//      without a seed);
//   3. row_kernel: one workgroup per (row y, segment of CH columns) minimises, per pixel x, the 64-bit key
//      (dist2 << 32 | index) over the columns x' with col[y][x'] = r >= 0, dist2 = (x - x')^2 + (y - r)^2, index =
//      r W + x', searching outward from x (d = 0, 1, 2 ... on both sides) while d^2 <= the best dist2 so far.  The
//      minimum of the key is the minimum distance with ties to the smallest linear index.  The row of column results
//      is staged in LDS in chunks of CH columns; a lane at distance d = k CH + j reads chunks -k and -(k + 1) to its
//      left and k and k + 1 to its right (relative to its segment), so two chunks per side are live and each ring k
//      stages one new chunk per side.  A ring whose four chunks hold no seed at all is skipped.
// The column plane and the band words are read by the launch after the one that wrote them: the kernel boundary
// publishes them, the loads are plain.  No workgroup waits for another and there is no atomic in the transform.
// Every loop is counted: by the rows of a band (64), the bands (ceil(H / 64)), the rings (ceil(W / CH) + 1) or the
// columns of a ring (CH).
//
// fg_depth_table is a policy of scene_common.hpp's accumulation kernel, which holds the loop and its reasons: int64
// add and max only.
#include "scene_common.hpp"

namespace {

using namespace fg::scene;

constexpr int BAND = 64;                            // rows per band word
constexpr int CH = 256;                             // columns per row-pass segment and per staged chunk (= NT)
constexpr int MAX_SIDE = 32768;                     // 2 * 32767^2 < 2^31: every squared distance fits int32
constexpr float Q_CAP = 1048576.0f, Q_SCALE = 1024.0f;

typedef unsigned long long u64;

// bits[b * W + x]: bit r set when pixel (64 b + r, x) is a seed (rows >= H are never set)
__global__ void __launch_bounds__(NT) seed_bits_kernel(ClassPlane s, int H, int W, int nb, u64* bits) {
    const long long total = (long long)nb * W;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int b = (int)(i / W), x = (int)(i % W), y0 = b * BAND;
        u64 w = 0;
#pragma unroll 8
        for (int r = 0; r < BAND; ++r)
            if (y0 + r < H && s.member(y0 + r, x)) w |= 1ull << r;
        bits[i] = w;
    }
}

// col[y * W + x] = the seed row of column x nearest to y, ties to the smaller row; -1 in a column without a seed
__global__ void __launch_bounds__(NT) column_kernel(const u64* bits, int H, int W, int nb, int* col) {
    const long long total = (long long)nb * W;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int b = (int)(i / W), x = (int)(i % W), y0 = b * BAND;
        const u64 w = bits[i];
        int above = -1, below = -1;
        // counted: at most nb - 1 words each way, stopping at the first that holds a seed
        for (int bb = b - 1; bb >= 0; --bb) {
            const u64 v = bits[(long long)bb * W + x];
            if (v) { above = bb * BAND + 63 - __clzll((long long)v); break; }
        }
        for (int bb = b + 1; bb < nb; ++bb) {
            const u64 v = bits[(long long)bb * W + x];
            if (v) { below = bb * BAND + __ffsll((long long)v) - 1; break; }
        }
        for (int r = 0; r < BAND && y0 + r < H; ++r) {
            const int y = y0 + r;
            const u64 lo = w & (~0ull >> (63 - r)), hi = w & (~0ull << r);        // rows <= y, rows >= y of the band
            const int up = lo ? y0 + 63 - __clzll((long long)lo) : above;
            const int dn = hi ? y0 + __ffsll((long long)hi) - 1 : below;
            int best;
            if (up < 0) best = dn;
            else if (dn < 0) best = up;
            else best = (y - up) <= (dn - y) ? up : dn;
            col[(long long)y * W + x] = best;
        }
    }
}

// one workgroup per (row, segment of CH columns); lane t owns pixel x = x0 + t
__global__ void __launch_bounds__(NT) row_kernel(const int* col, int H, int W, int segs, int* nearest, int* dist2) {
    __shared__ int left[2 * CH], right[2 * CH];     // chunks -k, -(k + 1) and k, k + 1 of ring k, by parity
    const int y = (int)(blockIdx.x / segs), x0 = (int)(blockIdx.x % segs) * CH;
    const int t = threadIdx.x, x = x0 + t;
    const int* row = col + (long long)y * W;
    // a value read from the column plane is a row of the scene or "no seed": anything else counts as no seed
    auto fetch = [&](int c) {
        const long long xc = (long long)x0 + (long long)c * CH + t;
        if (xc < 0 || xc >= W) return -1;
        const int r = row[xc];
        return (unsigned)r < (unsigned)H ? r : -1;
    };
    const int own = fetch(0);
    left[t] = right[t] = own;
    int prev_any = __syncthreads_or(own >= 0);
    u64 best = ~0ull;
    // the farthest column of the scene from any pixel of the segment
    const int reach = max(min(x0 + CH - 1, W - 1), W - 1 - x0);
    const int rings = reach / CH + 1;
    // counted: rings <= W / CH + 1
    for (int k = 0; k < rings; ++k) {
        const int p = k & 1, q = p ^ 1;
        const int vl = fetch(-(k + 1)), vr = fetch(k + 1);
        left[q * CH + t] = vl;
        right[q * CH + t] = vr;
        const int new_any = __syncthreads_or(vl >= 0 || vr >= 0);
        if (x < W && (prev_any || new_any)) {
            // counted: CH columns each side; a lane leaves when no farther column can beat or tie its best
            for (int j = 0; j < CH; ++j) {
                const long long d = (long long)k * CH + j;
                if ((u64)(d * d) > (best >> 32)) break;
                const int xl = x - (int)d, xr = x + (int)d;
                if (xl >= 0) {
                    const int o = t - j;
                    const int r = o >= 0 ? left[p * CH + o] : left[q * CH + o + CH];
                    if (r >= 0) {
                        const long long dy = y - r;
                        const u64 key = ((u64)(d * d + dy * dy) << 32) | (unsigned)(r * W + xl);
                        best = key < best ? key : best;
                    }
                }
                if (xr < W) {
                    const int o = t + j;
                    const int r = o < CH ? right[p * CH + o] : right[q * CH + o - CH];
                    if (r >= 0) {
                        const long long dy = y - r;
                        const u64 key = ((u64)(d * d + dy * dy) << 32) | (unsigned)(r * W + xr);
                        best = key < best ? key : best;
                    }
                }
            }
        }
        const long long dn = (long long)(k + 1) * CH;
        const int go = x < W && (u64)(dn * dn) <= (best >> 32);
        // (also the barrier between this ring's reads of parity q's predecessor and the next ring's staging)
        if (!__syncthreads_or(go)) break;
        prev_any = new_any;
    }
    if (x < W) {
        const bool found = best != ~0ull;
        nearest[(long long)y * W + x] = found ? (int)(unsigned)(best & 0xffffffffu) : -1;
        if (dist2) dist2[(long long)y * W + x] = found ? (int)(best >> 32) : -1;
    }
}

__global__ void __launch_bounds__(NT) shore_kernel(const float* mask, int H, int W, float* shore) {
    const long long total = (long long)H * W;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int y = (int)(i / W), x = (int)(i % W);
        bool s = false;
        if (mask[i] > 0.5f) {
            // a neighbour outside the scene is unknown, not dry
            s = (y > 0 && !(mask[i - W] > 0.5f)) || (y < H - 1 && !(mask[i + W] > 0.5f)) ||
                (x > 0 && !(mask[i - 1] > 0.5f)) || (x < W - 1 && !(mask[i + 1] > 0.5f));
        }
        shore[i] = s ? 1.f : 0.f;
    }
}

__global__ void __launch_bounds__(NT) depth_kernel(const float* mask, const float* elev, const int* nearest,
                                                   long long total, float* depth) {
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        float out = 0.f;
        if (mask[i] > 0.5f) {
            const int s = nearest[i];
            if ((unsigned)s < (unsigned)total) {            // the index names a pixel of the scene
                const float d = elev[s] - elev[i];
                out = d > 0.f ? d : 0.f;                    // negative and NaN differences give 0
            }
        }
        depth[i] = out;
    }
}

// ---- the depth table: a policy of accumulate_kernel

// table[rank[root]] = {wet_area, depth_sum_q, depth_max_q} over the pixels whose depth rounds to at least one quantum;
// the quantum is a pixel's weight, so a shallower pixel is left out before its root is looked at
struct DepthTable {
    struct Acc {
        int root, n;
        long long sum, mx;
    };
    int H, W;
    const int* labels;          // null with rank: the whole scene as one region, row 0
    const int* rank;            // plane indexed by root
    const float* depth;
    long long* table;           // [R, 3]
    int R;
    static __device__ __forceinline__ Acc empty() { return Acc{-1, 0, 0, 0}; }
    __device__ __forceinline__ long long weight(long long at) const {
        return (long long)rintf(fminf(depth[at], Q_CAP) * Q_SCALE);
    }
    __device__ __forceinline__ void add(Acc& a, int, int, long long q) const {
        a.n += 1;
        a.sum += q;
        a.mx = max(a.mx, q);
    }
    static __device__ __forceinline__ void merge(Acc& g, int d) {
        g.n += __shfl_xor(g.n, d);
        g.sum += __shfl_xor(g.sum, d);
        g.mx = max(g.mx, __shfl_xor(g.mx, d));
    }
    // every index that comes out of memory is checked against the plane or the table before it is used
    __device__ __forceinline__ void emit(const Acc& a) const {
        if (a.n <= 0 || (unsigned)a.root >= (unsigned)(H * W)) return;
        const int r = rank ? rank[a.root] : 0;
        if ((unsigned)r >= (unsigned)R) return;
        long long* row = table + 3ll * r;
        __hip_atomic_fetch_add(row + 0, (long long)a.n, FG_RLX_AGENT);
        __hip_atomic_fetch_add(row + 1, a.sum, FG_RLX_AGENT);
        __hip_atomic_fetch_max(row + 2, a.mx, FG_RLX_AGENT);
    }
};

inline long long col_bytes(int H, int W) { return ((long long)H * W * 4 + 7) / 8 * 8; }
inline int bands(int H) { return (H + BAND - 1) / BAND; }

}  // namespace

FG_API long long fg_nearest_seed_scratch_bytes(int H, int W) {
    if (H <= 0 || W <= 0 || H > MAX_SIDE || W > MAX_SIDE) return 0;
    return col_bytes(H, W) + (long long)bands(H) * W * 8;
}

FG_API int fg_nearest_seed(fg_sview src, int H, int W, int kind, int target, int* nearest, int* dist2, void* scratch,
                           hipStream_t stream) {
    const char* who = "fg_nearest_seed";
    if (!src.ptr || !nearest || !scratch) return fg::fail(FG_ERR_INVALID, "%s: null source, nearest plane or scratch", who);
    if (H <= 0 || W <= 0 || H > MAX_SIDE || W > MAX_SIDE)
        return fg::fail(FG_ERR_INVALID, "%s: a scene of %d x %d: each side must be 1 .. %d (squared distances are "
                        "int32)", who, H, W, MAX_SIDE);
    if (int e = check_scene(who, H, W)) return e;
    if (int e = check_class(who, kind, target)) return e;
    if (!aligned(src.ptr, 4) || !aligned(nearest, 4) || (dist2 && !aligned(dist2, 4)) || !aligned(scratch, 8))
        return fg::fail(FG_ERR_INVALID, "%s: source and planes must be 4-byte, the scratch 8-byte aligned", who);
    int* col = static_cast<int*>(scratch);
    u64* bits = reinterpret_cast<u64*>(static_cast<char*>(scratch) + col_bytes(H, W));
    const int nb = bands(H), segs = (W + CH - 1) / CH;
    const int grid = fg::blocks_for((long long)nb * W, NT, 1 << 16);
    hipLaunchKernelGGL(seed_bits_kernel, dim3(grid), dim3(NT), 0, stream,
                       ClassPlane{src.ptr, src.sy, src.sx, kind, target}, H, W, nb, bits);
    hipLaunchKernelGGL(column_kernel, dim3(grid), dim3(NT), 0, stream, bits, H, W, nb, col);
    hipLaunchKernelGGL(row_kernel, dim3((unsigned)((long long)H * segs)), dim3(NT), 0, stream, col, H, W, segs, nearest,
                       dist2);
    return fg::launched("nearest_seed");
}

FG_API int fg_shore(const float* mask, int H, int W, float* shore, hipStream_t stream) {
    const char* who = "fg_shore";
    if (!mask || !shore) return fg::fail(FG_ERR_INVALID, "%s: null mask or shore plane", who);
    if (int e = check_scene(who, H, W)) return e;
    if (mask == shore) return fg::fail(FG_ERR_INVALID, "%s: the shore plane must not be the mask", who);
    if (!aligned(mask, 4) || !aligned(shore, 4)) return fg::fail(FG_ERR_INVALID, "%s: planes must be 4-byte aligned", who);
    hipLaunchKernelGGL(shore_kernel, dim3(fg::blocks_for((long long)H * W, NT, 4096)), dim3(NT), 0, stream, mask, H, W,
                       shore);
    return fg::launched("shore");
}

FG_API int fg_flood_depth(const float* mask, const float* elev, const int* nearest, int H, int W, float* depth,
                          hipStream_t stream) {
    const char* who = "fg_flood_depth";
    if (!mask || !elev || !nearest || !depth)
        return fg::fail(FG_ERR_INVALID, "%s: null mask, elevation, nearest plane or depth plane", who);
    if (int e = check_scene(who, H, W)) return e;
    if (depth == elev) return fg::fail(FG_ERR_INVALID, "%s: the depth plane must not be the elevation", who);
    if (!aligned(mask, 4) || !aligned(elev, 4) || !aligned(nearest, 4) || !aligned(depth, 4))
        return fg::fail(FG_ERR_INVALID, "%s: planes must be 4-byte aligned", who);
    hipLaunchKernelGGL(depth_kernel, dim3(fg::blocks_for((long long)H * W, NT, 4096)), dim3(NT), 0, stream, mask, elev,
                       nearest, (long long)H * W, depth);
    return fg::launched("flood_depth");
}

FG_API int fg_depth_table(const int* labels, const int* rank, const float* depth, int H, int W, long long* table,
                          int R, hipStream_t stream) {
    const char* who = "fg_depth_table";
    if (!depth || !table) return fg::fail(FG_ERR_INVALID, "%s: null depth plane or table", who);
    if ((labels == nullptr) != (rank == nullptr))
        return fg::fail(FG_ERR_INVALID, "%s: labels and rank plane come together (both null: the scene as one region)",
                        who);
    if (int e = check_scene(who, H, W)) return e;
    if (R <= 0 || R > (long long)H * W || (!labels && R != 1))
        return fg::fail(FG_ERR_INVALID, "%s: %d regions in a scene of %d x %d%s", who, R, H, W,
                        labels ? "" : " taken as one region");
    if ((labels && !aligned(labels, 4)) || (rank && !aligned(rank, 4)) || !aligned(depth, 4) || !aligned(table, 8))
        return fg::fail(FG_ERR_INVALID, "%s: planes must be 4-byte, the table 8-byte aligned", who);
    if (hipMemsetAsync(table, 0, sizeof(long long) * 3 * (size_t)R, stream) != hipSuccess)
        return fg::fail(FG_ERR_INVALID, "%s: clearing the table failed", who);
    launch_accumulate(DepthTable{H, W, labels, rank, depth, table, R}, stream);
    return fg::launched("depth_table");
}
