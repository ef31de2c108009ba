// Scenes larger than a training tile: overlapping windows blended back into one image on the device
// (floodgan/scene.py; include/floodgan.h: fg_mosaic_grid).
//   * fg_mosaic_accumulate: planes[ch, y, x] += w_k(y, x) * window_k[ch, y - y0_k, x - x0_k] for a batch of windows
//     k0 .. k0 + n - 1, read through a strided view (channels-last generator outputs; channel 0 of NHWC logits);
//   * fg_mosaic_finalize: out[ch, y, x] = planes[ch, y, x] / sum_k w_k(y, x), the weight sum recomputed from the grid
//     as an integer (the weight is separable: (sum of w over the covering rows) * (sum over the covering columns)).
// Gather, not scatter: one lane owns a run of four pixels of a scene row, finds the windows of the batch that cover it
// (the starts are ascending and the windows equal in length, so those are an index range per axis: at most three)
// and adds their contributions in ascending window index, each as an fp32 product followed by an fp32 add
// (__fmul_rn / __fadd_rn: nothing the compiler could contract or reassociate).  No atomics, no order left to the
// scheduler: the chain of operations a pixel sees is the ascending list of its windows whatever calls they arrive
// in, so the planes are BIT-IDENTICAL however the windows are split into batches of ascending k0.
// Pure streaming, grid-stride, no LDS.  With planes whose rows are 16-byte aligned (W a multiple of 4) a lane loads
// and stores its run of each plane as 16 bytes; a window row that holds the whole run at unit stride and 16-byte
// alignment is read as 16 bytes too.  Everything else -- the runs at a region's or a window's edge, channels-last
// sources, scenes of odd width -- goes one pixel at a time.
// The device arrays of starts are only ever used to decide WHICH in-bounds element to read: a window is indexed at
// local coordinates checked against [0, tile), the planes at pixels of the scene.
#include <limits.h>

#include "fg_common.hpp"

namespace {

constexpr int NT = 256;

struct Grid {
    const int* ys;
    const int* xs;
    int ny, nx, tile, step, cap;       // step = tile - overlap, cap = max(overlap, 1)
    int H, W;
};

__device__ __forceinline__ int weight1(int u, const Grid& g) { return min(min(u + 1, g.tile - u), g.cap); }

// the windows of one axis (starts s[0 .. n), ascending) that cover coordinate p: indices lo .. hi, empty when lo > hi
__device__ __forceinline__ void covering(const int* s, int n, const Grid& g, int p, int& lo, int& hi) {
    hi = min(p / g.step, n - 1);
    while (hi + 1 < n && s[hi + 1] <= p) ++hi;
    while (hi >= 0 && s[hi] > p) --hi;
    lo = hi + 1;
    while (lo > 0 && s[lo - 1] + g.tile > p) --lo;
}

struct Batch {
    const float* src;
    long long sn, sc, sy, sx;
    int k0, n;
    int ry0, rows;                     // the scene rows the batch touches
    int rx0, rx1;                      // ... and its columns [rx0, rx1)
    int runs;                          // aligned 4-pixel runs per row that meet [rx0, rx1)
    int vec;                           // plane rows take 16-byte accesses
};

template <int C>
__global__ void __launch_bounds__(NT) mosaic_accumulate_kernel(Grid g, Batch b, float* planes) {
    const long long total = (long long)b.rows * b.runs;
    const long long plane = (long long)g.H * g.W;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int y = b.ry0 + (int)(i / b.runs);
        const int xq = (b.rx0 & ~3) + 4 * (int)(i % b.runs);
        const int xa = max(xq, b.rx0), xb = min(xq + 4, b.rx1);        // the run's pixels inside the region
        int ylo, yhi, xlo, xhi, unused;
        covering(g.ys, g.ny, g, y, ylo, yhi);
        covering(g.xs, g.nx, g, xa, xlo, unused);
        covering(g.xs, g.nx, g, xb - 1, unused, xhi);
        float* pp = planes + (long long)y * g.W + xq;
        float acc[C][4];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            if (b.vec) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(pp + ch * plane);
                acc[ch][0] = t[0]; acc[ch][1] = t[1]; acc[ch][2] = t[2]; acc[ch][3] = t[3];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[ch][e] = xq + e >= xa && xq + e < xb ? pp[ch * plane + e] : 0.f;
            }
        }
        unsigned touched = 0;
        for (int iy = ylo; iy <= yhi; ++iy) {
            const int uy = y - g.ys[iy];
            if ((unsigned)uy >= (unsigned)g.tile) continue;
            const int wy = weight1(uy, g);
            for (int ix = xlo; ix <= xhi; ++ix) {
                const long long j = (long long)iy * g.nx + ix - b.k0;             // ascending with (iy, ix)
                if (j < 0 || j >= b.n) continue;
                const int ux0 = xq - g.xs[ix];                                    // local column of the run's first pixel
                const float* sp = b.src + j * b.sn + uy * b.sy;
                if (b.sx == 1 && xa == xq && xb == xq + 4 && ux0 >= 0 && ux0 + 4 <= g.tile) {
                    float w[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) w[e] = (float)(wy * weight1(ux0 + e, g));
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) {
                        const float* s = sp + ch * b.sc + ux0;
                        float v[4];
                        if ((reinterpret_cast<uintptr_t>(s) & 15) == 0) {
                            const f32x4 t = *reinterpret_cast<const f32x4*>(s);
                            v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = s[e];
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[ch][e] = __fadd_rn(acc[ch][e], __fmul_rn(w[e], v[e]));
                    }
                    touched = 15u;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int ux = ux0 + e;
                        if (xq + e < xa || xq + e >= xb || (unsigned)ux >= (unsigned)g.tile) continue;
                        const float w = (float)(wy * weight1(ux, g));
#pragma unroll
                        for (int ch = 0; ch < C; ++ch)
                            acc[ch][e] = __fadd_rn(acc[ch][e], __fmul_rn(w, sp[ch * b.sc + ux * b.sx]));
                        touched |= 1u << e;
                    }
                }
            }
        }
        if (!touched) continue;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            if (b.vec) {
                // (the run's pixels no window of the batch covers are stored back as they were read: this lane is
                // the only one of the launch that owns them)
                f32x4 t;
                t[0] = acc[ch][0]; t[1] = acc[ch][1]; t[2] = acc[ch][2]; t[3] = acc[ch][3];
                *reinterpret_cast<f32x4*>(pp + ch * plane) = t;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (touched & (1u << e)) pp[ch * plane + e] = acc[ch][e];
            }
        }
    }
}

// the weight sum of one axis at coordinate p
__device__ __forceinline__ int weight_sum(const int* s, int n, const Grid& g, int p) {
    int lo, hi, sum = 0;
    covering(s, n, g, p, lo, hi);
    for (int i = lo; i <= hi; ++i) {
        const int u = p - s[i];
        if ((unsigned)u < (unsigned)g.tile) sum += weight1(u, g);
    }
    return sum;
}

template <int C>
__global__ void __launch_bounds__(NT) mosaic_finalize_kernel(Grid g, const float* planes, float* dst, int runs,
                                                             int vec) {
    const long long total = (long long)g.H * runs;
    const long long plane = (long long)g.H * g.W;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(i / runs);
        const int xq = 4 * (int)(i % runs);
        const int wy = weight_sum(g.ys, g.ny, g, y);
        float den[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) den[e] = xq + e < g.W ? (float)(wy * weight_sum(g.xs, g.nx, g, xq + e)) : 1.f;
        const long long at = (long long)y * g.W + xq;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            if (vec) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(planes + ch * plane + at);
                f32x4 o;
                o[0] = __fdiv_rn(t[0], den[0]); o[1] = __fdiv_rn(t[1], den[1]);
                o[2] = __fdiv_rn(t[2], den[2]); o[3] = __fdiv_rn(t[3], den[3]);
                *reinterpret_cast<f32x4*>(dst + ch * plane + at) = o;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (xq + e < g.W) dst[ch * plane + at + e] = __fdiv_rn(planes[ch * plane + at + e], den[e]);
            }
        }
    }
}

// 0, or the error code after recording what is wrong with one axis' starts (host copy)
int check_axis(const char* who, const char* axis, const int* s, int n, int tile, int len) {
    if (s[0] != 0 || s[n - 1] != len - tile)
        return fg::fail(FG_ERR_INVALID, "%s: the %s starts run from %d to %d (a scene of %d needs 0 to %d: a window "
                        "leaves the scene or a pixel is uncovered)", who, axis, s[0], s[n - 1], len, len - tile);
    for (int i = 1; i < n; ++i)
        if (s[i] <= s[i - 1] || s[i] - s[i - 1] > tile)
            return fg::fail(FG_ERR_INVALID, "%s: %s starts %d, %d (index %d): they must ascend in steps of at most "
                            "the tile (%d)", who, axis, s[i - 1], s[i], i, tile);
    return 0;
}

int check_grid(const char* who, const fg_mosaic_grid& g, int c, int H, int W, Grid* out) {
    if (!g.ys || !g.xs || !g.ys_host || !g.xs_host)
        return fg::fail(FG_ERR_INVALID, "%s: null window starts (device and host copies are both required)", who);
    if (g.ny <= 0 || g.nx <= 0 || g.tile <= 0 || H <= 0 || W <= 0)
        return fg::fail(FG_ERR_INVALID, "%s: sizes must be positive (grid %d x %d, tile %d, scene %d x %d)", who, g.ny,
                        g.nx, g.tile, H, W);
    if (c != 1 && c != 3) return fg::fail(FG_ERR_INVALID, "%s: c must be 1 or 3 (got %d)", who, c);
    if (g.overlap < 0 || g.overlap > g.tile / 2 || g.overlap > FG_MOSAIC_MAX_OVERLAP)
        return fg::fail(FG_ERR_INVALID, "%s: overlap %d outside 0 .. min(tile / 2 = %d, %d)", who, g.overlap,
                        g.tile / 2, (int)FG_MOSAIC_MAX_OVERLAP);
    if (g.tile > H || g.tile > W)
        return fg::fail(FG_ERR_INVALID, "%s: tile %d is larger than the %d x %d scene", who, g.tile, H, W);
    if ((long long)g.ny * g.nx > INT_MAX)
        return fg::fail(FG_ERR_INVALID, "%s: a grid of %d x %d windows", who, g.ny, g.nx);
    if (int e = check_axis(who, "row", g.ys_host, g.ny, g.tile, H)) return e;
    if (int e = check_axis(who, "column", g.xs_host, g.nx, g.tile, W)) return e;
    *out = Grid{g.ys, g.xs, g.ny, g.nx, g.tile, g.tile - g.overlap, g.overlap > 1 ? g.overlap : 1, H, W};
    return 0;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

FG_API int fg_mosaic_accumulate(fg_sview src, int n, int c, fg_mosaic_grid grid, int k0, float* planes, int H, int W,
                                hipStream_t stream) {
    const char* who = "fg_mosaic_accumulate";
    if (!src.ptr || !planes) return fg::fail(FG_ERR_INVALID, "%s: null source or planes", who);
    Grid g;
    if (int e = check_grid(who, grid, c, H, W, &g)) return e;
    if (n <= 0 || k0 < 0 || (long long)k0 + n > (long long)g.ny * g.nx)
        return fg::fail(FG_ERR_INVALID, "%s: windows %d .. %lld of a grid of %d x %d", who, k0, (long long)k0 + n - 1,
                        g.ny, g.nx);
    if (reinterpret_cast<uintptr_t>(planes) & 3)
        return fg::fail(FG_ERR_INVALID, "%s: the planes must be 4-byte aligned", who);
    // the scene region the batch touches: whole grid rows, or a span of one
    const int iy0 = k0 / g.nx, iy1 = (k0 + n - 1) / g.nx;
    Batch b{src.ptr, src.sn, src.sc, src.sy, src.sx, k0, n};
    b.ry0 = grid.ys_host[iy0];
    b.rows = grid.ys_host[iy1] + g.tile - b.ry0;
    b.rx0 = iy0 == iy1 ? grid.xs_host[k0 % g.nx] : 0;
    b.rx1 = iy0 == iy1 ? grid.xs_host[(k0 + n - 1) % g.nx] + g.tile : W;
    b.runs = ((b.rx1 + 3) >> 2) - (b.rx0 >> 2);
    b.vec = (W & 3) == 0 && aligned16(planes);
    const int blocks = fg::blocks_for((long long)b.rows * b.runs, NT, 2048);
    if (c == 1) hipLaunchKernelGGL(mosaic_accumulate_kernel<1>, dim3(blocks), dim3(NT), 0, stream, g, b, planes);
    else hipLaunchKernelGGL(mosaic_accumulate_kernel<3>, dim3(blocks), dim3(NT), 0, stream, g, b, planes);
    return fg::launched("mosaic_accumulate");
}

FG_API int fg_mosaic_finalize(const float* planes, int c, fg_mosaic_grid grid, int H, int W, float* dst,
                              hipStream_t stream) {
    const char* who = "fg_mosaic_finalize";
    if (!planes || !dst) return fg::fail(FG_ERR_INVALID, "%s: null planes or destination", who);
    Grid g;
    if (int e = check_grid(who, grid, c, H, W, &g)) return e;
    if ((reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(dst)) & 3)
        return fg::fail(FG_ERR_INVALID, "%s: planes and destination must be 4-byte aligned", who);
    const int runs = (W + 3) >> 2;
    const int vec = (W & 3) == 0 && aligned16(planes) && aligned16(dst);
    const int blocks = fg::blocks_for((long long)H * runs, NT, 2048);
    if (c == 1) hipLaunchKernelGGL(mosaic_finalize_kernel<1>, dim3(blocks), dim3(NT), 0, stream, g, planes, dst, runs, vec);
    else hipLaunchKernelGGL(mosaic_finalize_kernel<3>, dim3(blocks), dim3(NT), 0, stream, g, planes, dst, runs, vec);
    return fg::launched("mosaic_finalize");
}
