// The outlines of a scene's flood regions: crack extraction, ring ordering by pointer doubling and the corner lists
// (floodgan/outline.py; include/floodgan.h: fg_outline_*).  Everything here is integer-exact and no
// launch holds an atomic: every word of every buffer has one writer per launch.
//
// A crack is a side of a flood pixel (labels >= 0) whose neighbour across it is dry or outside the scene, directed
// with the flood pixel on its left: side 0 top, west; 1 left, south; 2 bottom, east; 3 right, north.  Its key is
// 4 (y W + x) + side; the compact index of a crack is its rank among the cracks in ascending key order, so the
// smallest compact index of a ring is also its smallest key.
//   1. cracks_kernel (fg_outline_cracks): per pixel its 4-bit side mask and its crack count; the caller scans the
//      counts (an inclusive prefix sum) and reads E, the number of cracks, once;
//   2. edges_kernel: per crack its key, its successor's compact index (the crack that starts at its end vertex; at a
//      saddle the right turn with connectivity 8, the left turn with 4), whether its start vertex is a corner of its
//      ring, and its term of the shoelace sum;
//   3. K = ceil(log2 E) rounds of ring_min_kernel: m'[e] = min(m[e], m[j[e]]), j'[e] = j[j[e]]; after round r, m[e] is
//      the minimum over the 2^r cracks from e on, so after K rounds it is the ring's start crack;
//   4. link_kernel cuts every ring in front of its start crack (the crack whose successor is a start crack gets no
//      successor), then K rounds of rank_kernel (Wyllie): every value becomes the sum from its crack to the end of its
//      ring, so the start crack holds the ring's number of cracks, its number of corners and twice its signed area;
//   5. vertices_kernel (fg_outline_vertices): a corner crack writes its start vertex at base[ring] + (corners of the
//      ring - corners from it on).
// Every round reads one buffer set and writes the other; the kernel boundary publishes it, the loads are plain.  No
// workgroup waits for another.  The rounds are counted on the host (K <= 31); the device loops are grid strides.
// Every index read from memory -- an offset, a side mask, a successor, a ring, a base -- is checked against the array
// it indexes before use; a crack whose successor cannot be found points at itself.
#include <utility>

#include "scene_common.hpp"

namespace {

using namespace fg::scene;

constexpr long long MAX_PIXELS = 1ll << 29;         // keys 4 (H W - 1) + 3 fit int32 below it

typedef unsigned char u8;

__device__ __forceinline__ bool wet(const int* labels, int H, int W, int y, int x) {
    return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W && labels[(long long)y * W + x] >= 0;
}

// the direction of travel (hy, hx) of a side and the outward normal (ry, rx) of its pixel: the dry side, on the right
__device__ __forceinline__ void frame(int s, int& hy, int& hx, int& ry, int& rx) {
    hy = (s == 1) - (s == 3);
    hx = (s == 2) - (s == 0);
    ry = (s == 2) - (s == 0);
    rx = (s == 3) - (s == 1);
}

__global__ void __launch_bounds__(NT) cracks_kernel(const int* labels, int H, int W, u8* sides, int* count) {
    const long long total = (long long)H * W;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int y = (int)(i / W), x = (int)(i % W);
        unsigned m = 0;
        if (labels[i] >= 0)
            m = (unsigned)!wet(labels, H, W, y - 1, x) | (unsigned)!wet(labels, H, W, y, x - 1) << 1 |
                (unsigned)!wet(labels, H, W, y + 1, x) << 2 | (unsigned)!wet(labels, H, W, y, x + 1) << 3;
        sides[i] = (u8)m;
        count[i] = __popc(m);
    }
}

struct Edges {
    int *key, *succ, *m, *j, *cnt, *cor;
    long long* area;
    u8* corner;
};

// incl: the inclusive prefix sum of the counts; the cracks of pixel i are incl[i] - popc(sides[i]) .. incl[i] - 1
__global__ void __launch_bounds__(NT) edges_kernel(const int* labels, const u8* sides, const int* incl, int H, int W,
                                                   int conn8, int E, Edges o) {
    const long long total = (long long)H * W;
    for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const unsigned m = sides[i] & 15u;
        if (!m) continue;
        const int n = __popc(m), y = (int)(i / W), x = (int)(i % W);
        const long long off = (long long)incl[i] - n;
        if (off < 0 || off + n > E) continue;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (!(m >> s & 1u)) continue;
            const int e = (int)off + __popc(m & ((1u << s) - 1u));
            int hy, hx, ry, rx;
            frame(s, hy, hx, ry, rx);
            // ahead of the end vertex: a on the flood side, b on the dry side
            const int ay = y + hy, ax = x + hx, by = ay + ry, bx = ax + rx;
            const bool a = wet(labels, H, W, ay, ax), b = wet(labels, H, W, by, bx);
            int qy = y, qx = x, qs = (s + 1) & 3;                       // left turn: the next side of this pixel
            if (b && (a || conn8)) { qy = by; qx = bx; qs = (s + 3) & 3; }      // right turn (the saddle's, at 8)
            else if (a) { qy = ay; qx = ax; qs = s; }                   // straight on
            const long long qi = (long long)qy * W + qx;
            const unsigned mq = sides[qi] & 15u;
            const long long jl = (long long)incl[qi] - __popc(mq) + __popc(mq & ((1u << qs) - 1u));
            const int j = (mq >> qs & 1u) && jl >= 0 && jl < E ? (int)jl : e;
            // behind the start vertex: the arriving crack has this direction only from a flood pixel with a dry one
            // on its right
            const bool straight = wet(labels, H, W, y - hy, x - hx) && !wet(labels, H, W, y - hy + ry, x - hx + rx);
            const long long vy = y + (s >= 2), vx = x + (s == 0 || s == 3);
            o.key[e] = (int)(4 * i + s);
            o.succ[e] = j;
            o.m[e] = e;
            o.j[e] = j;
            o.cnt[e] = 1;
            o.cor[e] = !straight;
            o.corner[e] = (u8)!straight;
            o.area[e] = vx * (vy + hy) - (vx + hx) * vy;
        }
    }
}

__global__ void __launch_bounds__(NT) ring_min_kernel(const int* m, const int* j, int E, int* m2, int* j2) {
    for (long long e = blockIdx.x * (long long)NT + threadIdx.x; e < E; e += (long long)gridDim.x * NT) {
        const int n = j[e];
        if ((unsigned)n < (unsigned)E) {
            m2[e] = min(m[e], m[n]);
            j2[e] = j[n];
        } else {
            m2[e] = m[e];
            j2[e] = n;
        }
    }
}

// nxt[e] = the successor of e, or -1 where the successor is the start crack of its ring
__global__ void __launch_bounds__(NT) link_kernel(const int* succ, const int* ring, int E, int* nxt) {
    for (long long e = blockIdx.x * (long long)NT + threadIdx.x; e < E; e += (long long)gridDim.x * NT) {
        const int n = succ[e];
        nxt[e] = (unsigned)n < (unsigned)E && ring[n] != n ? n : -1;
    }
}

struct Sums {
    int *nxt, *cnt, *cor;
    long long* area;
};

__global__ void __launch_bounds__(NT) rank_kernel(Sums a, int E, Sums b) {
    for (long long e = blockIdx.x * (long long)NT + threadIdx.x; e < E; e += (long long)gridDim.x * NT) {
        const int n = a.nxt[e];
        int cnt = a.cnt[e], cor = a.cor[e], nn = -1;
        long long area = a.area[e];
        if ((unsigned)n < (unsigned)E) {
            cnt += a.cnt[n];
            cor += a.cor[n];
            area += a.area[n];
            nn = a.nxt[n];
        }
        b.nxt[e] = nn;
        b.cnt[e] = cnt;
        b.cor[e] = cor;
        b.area[e] = area;
    }
}

__global__ void __launch_bounds__(NT) vertices_kernel(const int* key, const int* ring, const int* corners,
                                                      const u8* corner, const int* base, int H, int W, int E, int V,
                                                      int* vertices) {
    const long long pixels = (long long)H * W;
    for (long long e = blockIdx.x * (long long)NT + threadIdx.x; e < E; e += (long long)gridDim.x * NT) {
        if (!corner[e]) continue;
        const int r = ring[e], k = key[e];
        if ((unsigned)r >= (unsigned)E || k < 0 || (k >> 2) >= pixels) continue;
        const long long pos = (long long)corners[r] - corners[e], at = (long long)base[r] + pos;
        if (pos < 0 || base[r] < 0 || at >= V) continue;
        const int s = k & 3, i = k >> 2;
        vertices[2 * at] = i / W + (s >= 2);
        vertices[2 * at + 1] = i % W + (s == 0 || s == 3);
    }
}

inline long long pad8(long long bytes) { return (bytes + 7) / 8 * 8; }

inline int rounds(int E) {
    int k = 0;
    while ((1ll << k) < E) ++k;                     // counted: k <= 31
    return k;
}

int check_plane(const char* who, int H, int W) {
    if (int e = check_scene(who, H, W)) return e;
    if ((long long)H * W >= MAX_PIXELS)
        return fg::fail(FG_ERR_INVALID, "%s: a scene of %d x %d = %lld pixels: edge keys are int32, H * W must be below "
                        "2^29", who, H, W, (long long)H * W);
    return 0;
}

}  // namespace

FG_API long long fg_outline_scratch_bytes(int E) {
    if (E <= 0) return 0;
    return 8ll * E + 8 * pad8(4ll * E);
}

FG_API int fg_outline_launches(int E) { return E <= 0 ? 1 : 4 + 2 * rounds(E); }

FG_API int fg_outline_cracks(const int* labels, int H, int W, unsigned char* sides, int* count, hipStream_t stream) {
    const char* who = "fg_outline_cracks";
    if (!labels || !sides || !count) return fg::fail(FG_ERR_INVALID, "%s: null labels, side or count plane", who);
    if (int e = check_plane(who, H, W)) return e;
    if (!aligned(labels, 4) || !aligned(count, 4))
        return fg::fail(FG_ERR_INVALID, "%s: labels and count plane must be 4-byte aligned", who);
    hipLaunchKernelGGL(cracks_kernel, dim3(fg::blocks_for((long long)H * W, NT, 4096)), dim3(NT), 0, stream, labels, H,
                       W, sides, count);
    return fg::launched("outline_cracks");
}

FG_API int fg_outline_rings(const int* labels, const unsigned char* sides, const int* incl, int H, int W,
                            int connectivity, int E, int* key, int* ring, int* edges, int* corners,
                            long long* signed2, unsigned char* corner, void* scratch, hipStream_t stream) {
    const char* who = "fg_outline_rings";
    if (!labels || !sides || !incl || !key || !ring || !edges || !corners || !signed2 || !corner || !scratch)
        return fg::fail(FG_ERR_INVALID, "%s: null plane, output or scratch", who);
    if (int e = check_plane(who, H, W)) return e;
    if (connectivity != 4 && connectivity != 8)
        return fg::fail(FG_ERR_INVALID, "%s: connectivity %d (4 or 8)", who, connectivity);
    if (E <= 0 || E > 4ll * H * W)
        return fg::fail(FG_ERR_INVALID, "%s: %d cracks in a scene of %d x %d (1 .. 4 H W)", who, E, H, W);
    if (!aligned(labels, 4) || !aligned(incl, 4) || !aligned(key, 4) || !aligned(ring, 4) || !aligned(edges, 4) ||
        !aligned(corners, 4) || !aligned(signed2, 8) || !aligned(scratch, 8))
        return fg::fail(FG_ERR_INVALID, "%s: int32 arrays must be 4-byte, signed2 and the scratch 8-byte aligned", who);
    char* base = static_cast<char*>(scratch);
    const long long col = pad8(4ll * E);
    long long* area_x = reinterpret_cast<long long*>(base);
    base += 8ll * E;
    auto take = [&]() { int* p = reinterpret_cast<int*>(base); base += col; return p; };
    int *succ = take(), *j_a = take(), *j_b = take(), *m_x = take(), *n_a = take(), *n_b = take(), *cnt_x = take(),
        *cor_x = take();
    const int K = rounds(E);
    const int grid_px = fg::blocks_for((long long)H * W, NT, 4096), grid = fg::blocks_for(E, NT, 4096);
    // the buffer a chain of K rounds starts in, so that it ends in the caller's array
    const bool out_first = K % 2 == 0;
    int *m0 = out_first ? ring : m_x, *m1 = out_first ? m_x : ring;
    Sums s0{out_first ? n_a : n_b, out_first ? edges : cnt_x, out_first ? corners : cor_x,
            out_first ? signed2 : area_x};
    Sums s1{out_first ? n_b : n_a, out_first ? cnt_x : edges, out_first ? cor_x : corners,
            out_first ? area_x : signed2};
    hipLaunchKernelGGL(edges_kernel, dim3(grid_px), dim3(NT), 0, stream, labels, sides, incl, H, W,
                       (int)(connectivity == 8), E, Edges{key, succ, m0, j_a, s0.cnt, s0.cor, s0.area, corner});
    int *ja = j_a, *jb = j_b;
    for (int r = 0; r < K; ++r) {
        hipLaunchKernelGGL(ring_min_kernel, dim3(grid), dim3(NT), 0, stream, m0, ja, E, m1, jb);
        std::swap(m0, m1);
        std::swap(ja, jb);
    }
    // m0 is `ring` now
    hipLaunchKernelGGL(link_kernel, dim3(grid), dim3(NT), 0, stream, succ, m0, E, s0.nxt);
    for (int r = 0; r < K; ++r) {
        hipLaunchKernelGGL(rank_kernel, dim3(grid), dim3(NT), 0, stream, s0, E, s1);
        std::swap(s0, s1);
    }
    return fg::launched("outline_rings");
}

FG_API int fg_outline_vertices(const int* key, const int* ring, const int* corners, const unsigned char* corner,
                               const int* base, int H, int W, int E, int V, int* vertices, hipStream_t stream) {
    const char* who = "fg_outline_vertices";
    if (!key || !ring || !corners || !corner || !base || !vertices)
        return fg::fail(FG_ERR_INVALID, "%s: null array", who);
    if (int e = check_plane(who, H, W)) return e;
    if (E <= 0 || E > 4ll * H * W || V <= 0 || V > E)
        return fg::fail(FG_ERR_INVALID, "%s: %d cracks and %d vertices in a scene of %d x %d (1 <= V <= E <= 4 H W)",
                        who, E, V, H, W);
    if (!aligned(key, 4) || !aligned(ring, 4) || !aligned(corners, 4) || !aligned(base, 4) || !aligned(vertices, 4))
        return fg::fail(FG_ERR_INVALID, "%s: int32 arrays must be 4-byte aligned", who);
    hipLaunchKernelGGL(vertices_kernel, dim3(fg::blocks_for(E, NT, 4096)), dim3(NT), 0, stream, key, ring, corners,
                       corner, base, H, W, E, V, vertices);
    return fg::launched("outline_vertices");
}
