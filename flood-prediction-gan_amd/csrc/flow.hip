// Flow routing over a scene's elevation: D8 directions, the flat wave, accumulation / basin / length by pointer
// doubling with scatter, and the per-region flow table (floodgan/flow.py; include/floodgan.h: fg_flow_directions,
// fg_flow_flats, fg_flow_accumulate, fg_flow_region_table).  All of it is integer-exact but for the
// direction's comparison, which is exact in fp64.
//
// Codes k = 0 .. 7: E, SE, S, SW, W, NW, N, NE, (dy, dx) = DY[k], DX[k]; 8 a pit, 255 nodata (a pixel whose elevation
// is not finite).  What lies outside the scene is never a neighbour.
//
// fg_flow_directions: one lane per pixel, the eight neighbours by plain loads.  A wave's lanes are adjacent pixels of
// a row, so each of the nine loads is one coalesced row segment and the three rows a wave touches stay in its CU's
// vector cache for the neighbouring waves; the kernel moves 4 bytes in and 1 byte out per pixel and holds no state
// worth staging.  The steepness key of a drop d = z[p] - z[n] (one fp32 subtraction) is c d d in fp64, c = 2 for a
// cardinal and 1 for a diagonal neighbour: d has 24 significant bits, its square 48, so key and comparison are exact.
//
// fg_flow_flats: `rounds` launches of one gather kernel, each reading the plane the previous one wrote; a round's count
// is reduced over the wave and the workgroup before its one atomic per workgroup, on a grid capped at 2048 workgroups
// (one counter takes an add every few nanoseconds: one per wave made a round of 2048^2 pixels cost 0.2 ms).
//
// fg_flow_accumulate: an initial launch (receivers from the directions), then K = ceil(log2 max(H W, 2)) rounds of
// {copy A, doubling launch}: 2 K + 1 launches and copies.  State per pixel and round: j (the ancestor at distance 2^r,
// or -1), A (data descendants at distance < 2^r), len (min(length, 2^r); -1 on nodata) and b (the ancestor at distance
// len; -1 on nodata).  A
// round reads one set of buffers and writes the other; the only atomics are relaxed agent-scope int32 adds into the
// set being written, which the kernel boundary publishes.  No workgroup waits for another.
//
// fg_flow_region_table is a policy of scene_common.hpp's accumulation kernel: int64 max and add only.
#include <utility>

#include "scene_common.hpp"

namespace {

using namespace fg::scene;

constexpr int MAX_FLAT_ROUNDS = 32768;
constexpr int PIT = 8, NODATA = 255;

__constant__ const int DY[8] = {0, 1, 1, 1, 0, -1, -1, -1};
__constant__ const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1};

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= 3.402823466e38f; }      // false for NaN

__global__ void __launch_bounds__(NT) directions_kernel(const float* elev, int H, int W, unsigned char* dir) {
    const long long total = (long long)H * W;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int y = (int)(i / W), x = (int)(i % W);
        const float z = elev[i];
        int best = NODATA;
        if (finite(z)) {
            best = PIT;
            double key = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int yn = y + DY[k], xn = x + DX[k];
                if (yn < 0 || yn >= H || xn < 0 || xn >= W) continue;
                const float zn = elev[(long long)yn * W + xn];
                if (!finite(zn)) continue;
                const float d = z - zn;
                if (!(d > 0.f)) continue;
                const double s = ((k & 1) ? 1.0 : 2.0) * (double)d * (double)d;
                if (s > key) {                      // strictly: a tie stays with the smaller k
                    key = s;
                    best = k;
                }
            }
        }
        dir[i] = (unsigned char)best;
    }
}

// one round of the wave: a pit takes the direction of its first neighbour (cardinals, then diagonals) of equal
// elevation that is directed in `in`; every other pixel is copied.  *count += the pixels directed here.
__global__ void __launch_bounds__(NT) flats_kernel(const float* elev, int H, int W, const unsigned char* in,
                                                   unsigned char* out, int* count) {
    __shared__ int block_count;
    if (threadIdx.x == 0) block_count = 0;
    __syncthreads();
    const long long total = (long long)H * W;
    int mine = 0;                                   // the pixels this lane directed, over all its tiles
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        int c = in[i];
        if (c == PIT) {
            const int y = (int)(i / W), x = (int)(i % W);
            // the directed neighbours first (bytes only): the inside of a flat has none and reads no elevation
            unsigned open = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int yn = y + DY[k], xn = x + DX[k];
                if (yn >= 0 && yn < H && xn >= 0 && xn < W && in[(long long)yn * W + xn] < 8) open |= 1u << k;
            }
            if (open) {
                const float z = elev[i];
#pragma unroll
                for (int o = 0; o < 8; ++o) {
                    const int k = o < 4 ? 2 * o : 2 * (o - 4) + 1;          // 0, 2, 4, 6, 1, 3, 5, 7
                    if (c == PIT && (open >> k & 1) && elev[(long long)(y + DY[k]) * W + x + DX[k]] == z) c = k;
                }
                mine += c != PIT;
            }
        }
        out[i] = (unsigned char)c;
    }
    // the round's count: summed over the wave, then over the block in LDS, then one atomic per block (the grid is
    // capped, so a round's adds to the one counter stay in the low thousands)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&block_count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && block_count) __hip_atomic_fetch_add(count, block_count, FG_RLX_AGENT);
}

// round 0 of the doubling: the receiver of every pixel from its direction byte.  A byte that is not 0 .. 7, a
// neighbour outside the scene and a neighbour that is nodata all make a pit.
__global__ void __launch_bounds__(NT) receivers_kernel(const unsigned char* dir, int H, int W, int* j, int* A, int* len,
                                                       int* b) {
    const long long total = (long long)H * W;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int c = dir[i];
        int r = -1;
        if (c < 8) {
            const int y = (int)(i / W), x = (int)(i % W);
            const int yn = y + DY[c], xn = x + DX[c];
            if (yn >= 0 && yn < H && xn >= 0 && xn < W) {
                const long long n = (long long)yn * W + xn;
                if (dir[n] != NODATA) r = (int)n;
            }
        }
        const bool data = c != NODATA;
        j[i] = r;
        A[i] = data ? 1 : 0;
        len[i] = r >= 0 ? 1 : (data ? 0 : -1);
        b[i] = r >= 0 ? r : (data ? (int)i : -1);
    }
}

struct FlowState {
    int *j, *A, *len, *b;
};

// one doubling round, `out.A` already a copy of `in.A`: every u with an ancestor q at distance 2^r hands q the
// descendants it has gathered and jumps to q's ancestor.  Indices read from memory are checked before use.
__global__ void __launch_bounds__(NT) doubling_kernel(FlowState in, long long total, FlowState out, int last) {
    for (long long u = blockIdx.x * (long long)NT + threadIdx.x; u < total; u += (long long)gridDim.x * NT) {
        const int q = in.j[u];
        int jn = -1, ln = in.len[u], bn = in.b[u];
        if ((unsigned)q < (unsigned long long)total) {
            const int a = in.A[u];
            if (a != 0) __hip_atomic_fetch_add(out.A + q, a, FG_RLX_AGENT);
            const int jq = in.j[q];
            jn = (unsigned)jq < (unsigned long long)total ? jq : -1;
            ln += in.len[q];
            bn = in.b[q];
        }
        if (!last) out.j[u] = jn;
        out.len[u] = ln;
        out.b[u] = bn;
    }
}

// ---- the flow table: a policy of accumulate_kernel

// table[rank[root]] = {max_accumulation, pit_pixels} over the region's pixels
struct FlowTable {
    struct Acc {
        int root, n;
        long long mx, pits;
    };
    int H, W;
    const int* labels;
    const int* rank;            // plane indexed by root
    const int* acc;
    const unsigned char* dir;
    long long* table;           // [R, 2]
    int R;
    static __device__ __forceinline__ Acc empty() { return Acc{-1, 0, 0, 0}; }
    __device__ __forceinline__ long long weight(long long) const { return 1; }
    __device__ __forceinline__ void add(Acc& a, int y, int x, long long) const {
        const long long at = (long long)y * W + x;
        a.n += 1;
        a.mx = max(a.mx, (long long)acc[at]);
        a.pits += dir[at] == PIT ? 1 : 0;
    }
    static __device__ __forceinline__ void merge(Acc& g, int d) {
        g.n += __shfl_xor(g.n, d);
        g.mx = max(g.mx, __shfl_xor(g.mx, d));
        g.pits += __shfl_xor(g.pits, d);
    }
    // every index that comes out of memory is checked against the plane or the table before it is used
    __device__ __forceinline__ void emit(const Acc& a) const {
        if (a.n <= 0 || (unsigned)a.root >= (unsigned)(H * W)) return;
        const int r = rank[a.root];
        if ((unsigned)r >= (unsigned)R) return;
        long long* row = table + 2ll * r;
        __hip_atomic_fetch_max(row + 0, a.mx, FG_RLX_AGENT);
        if (a.pits) __hip_atomic_fetch_add(row + 1, a.pits, FG_RLX_AGENT);
    }
};

inline long long plane_bytes(int H, int W) { return ((long long)H * W * 4 + 7) / 8 * 8; }

inline int doubling_rounds(long long n) {
    int k = 1;
    while ((1ll << k) < n) ++k;
    return k;
}

}  // namespace

FG_API int fg_flow_rounds(int H, int W) {
    if (H <= 0 || W <= 0 || (long long)H * W > INT_MAX) return 0;
    return doubling_rounds((long long)H * W);
}

FG_API long long fg_flow_scratch_bytes(int H, int W) {
    if (H <= 0 || W <= 0 || (long long)H * W > INT_MAX) return 0;
    return 5 * plane_bytes(H, W);
}

FG_API int fg_flow_directions(const float* elev, int H, int W, unsigned char* dir, hipStream_t stream) {
    const char* who = "fg_flow_directions";
    if (!elev || !dir) return fg::fail(FG_ERR_INVALID, "%s: null elevation or direction plane", who);
    if (int e = check_scene(who, H, W)) return e;
    if (!aligned(elev, 4)) return fg::fail(FG_ERR_INVALID, "%s: the elevation must be 4-byte aligned", who);
    hipLaunchKernelGGL(directions_kernel, dim3(fg::blocks_for((long long)H * W, NT, 1 << 16)), dim3(NT), 0, stream,
                       elev, H, W, dir);
    return fg::launched("flow_directions");
}

FG_API int fg_flow_flats(const float* elev, int H, int W, unsigned char* dir_in, unsigned char* dir_out, int rounds,
                         int* counts, hipStream_t stream) {
    const char* who = "fg_flow_flats";
    if (!elev || !dir_in || !dir_out) return fg::fail(FG_ERR_INVALID, "%s: null elevation or direction plane", who);
    if (int e = check_scene(who, H, W)) return e;
    if (rounds < 0 || rounds > MAX_FLAT_ROUNDS)
        return fg::fail(FG_ERR_INVALID, "%s: %d rounds (0 .. %d)", who, rounds, MAX_FLAT_ROUNDS);
    if (rounds > 0 && !counts) return fg::fail(FG_ERR_INVALID, "%s: null counts for %d rounds", who, rounds);
    if (dir_in == dir_out) return fg::fail(FG_ERR_INVALID, "%s: the two direction planes must be distinct", who);
    if (!aligned(elev, 4) || (counts && !aligned(counts, 4)))
        return fg::fail(FG_ERR_INVALID, "%s: elevation and counts must be 4-byte aligned", who);
    const size_t bytes = (size_t)H * W;
    if (rounds > 0 && hipMemsetAsync(counts, 0, sizeof(int) * (size_t)rounds, stream) != hipSuccess)
        return fg::fail(FG_ERR_INVALID, "%s: clearing the counts failed", who);
    // an odd number of rounds ends in the other plane by itself; an even one starts from a copy there
    unsigned char *a = dir_in, *b = dir_out;
    if (rounds % 2 == 0) {
        if (hipMemcpyAsync(dir_out, dir_in, bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return fg::fail(FG_ERR_INVALID, "%s: copying the direction plane failed", who);
        std::swap(a, b);
    }
    const int grid = fg::blocks_for((long long)H * W, NT, 2048);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(flats_kernel, dim3(grid), dim3(NT), 0, stream, elev, H, W, a, b, counts + r);
        std::swap(a, b);
    }
    return fg::launched("flow_flats");
}

FG_API int fg_flow_accumulate(const unsigned char* dir, int H, int W, int* acc, int* basin, int* length, void* scratch,
                              hipStream_t stream) {
    const char* who = "fg_flow_accumulate";
    if (!dir || !acc || !basin || !length || !scratch)
        return fg::fail(FG_ERR_INVALID, "%s: null direction plane, output or scratch", who);
    if (int e = check_scene(who, H, W)) return e;
    if (acc == basin || acc == length || basin == length)
        return fg::fail(FG_ERR_INVALID, "%s: the three outputs must be distinct", who);
    if (!aligned(acc, 4) || !aligned(basin, 4) || !aligned(length, 4) || !aligned(scratch, 8))
        return fg::fail(FG_ERR_INVALID, "%s: planes must be 4-byte, the scratch 8-byte aligned", who);
    const long long total = (long long)H * W, pb = plane_bytes(H, W);
    char* base = static_cast<char*>(scratch);
    auto take = [&]() { int* p = reinterpret_cast<int*>(base); base += pb; return p; };
    int *j_a = take(), *j_b = take();
    FlowState mine{nullptr, take(), take(), take()}, theirs{nullptr, acc, length, basin};
    const int K = doubling_rounds(total);
    // the buffer a chain of K rounds starts in, so that it ends in the caller's arrays
    FlowState s0 = K % 2 == 0 ? theirs : mine, s1 = K % 2 == 0 ? mine : theirs;
    s0.j = j_a;
    s1.j = j_b;
    const int grid = fg::blocks_for(total, NT, 1 << 16);
    hipLaunchKernelGGL(receivers_kernel, dim3(grid), dim3(NT), 0, stream, dir, H, W, s0.j, s0.A, s0.len, s0.b);
    for (int r = 0; r < K; ++r) {
        if (hipMemcpyAsync(s1.A, s0.A, sizeof(int) * (size_t)total, hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return fg::fail(FG_ERR_INVALID, "%s: copying the accumulation failed", who);
        hipLaunchKernelGGL(doubling_kernel, dim3(grid), dim3(NT), 0, stream, s0, total, s1, (int)(r == K - 1));
        std::swap(s0, s1);
    }
    return fg::launched("flow_accumulate");
}

FG_API int fg_flow_region_table(const int* labels, const int* rank, const int* acc, const unsigned char* dir, int H,
                                int W, long long* table, int R, hipStream_t stream) {
    const char* who = "fg_flow_region_table";
    if (!labels || !rank || !acc || !dir || !table)
        return fg::fail(FG_ERR_INVALID, "%s: null labels, rank, accumulation or direction plane or table", who);
    if (int e = check_scene(who, H, W)) return e;
    if (R <= 0 || R > (long long)H * W)
        return fg::fail(FG_ERR_INVALID, "%s: %d regions in a scene of %d x %d", who, R, H, W);
    if (!aligned(labels, 4) || !aligned(rank, 4) || !aligned(acc, 4) || !aligned(table, 8))
        return fg::fail(FG_ERR_INVALID, "%s: planes must be 4-byte, the table 8-byte aligned", who);
    if (hipMemsetAsync(table, 0, sizeof(long long) * 2 * (size_t)R, stream) != hipSuccess)
        return fg::fail(FG_ERR_INVALID, "%s: clearing the table failed", who);
    launch_accumulate(FlowTable{H, W, labels, rank, acc, dir, table, R}, stream);
    return fg::launched("flow_region_table");
}
