// Pictures on the device: fp32 tensors -> RGBA8 panels of a canvas, with the byte rules of the reference's
// plt.imsave calls (models/model.py:505-518, models/segmentation_model.py:207, :227-232; matplotlib 3.10):
//   * fg_render_rgb: channels 0..2 of a strided [n, >=3, h, w] view; FG_RENDER_SIGNED is utils.tensor_to_numpy's
//     clip((x + 1) * 0.5, 0, 1), FG_RENDER_UNIT the segmentation input's clip(x, 0, 1); byte = trunc(v * 255) with
//     the product in fp32 (matplotlib truncates, it does not round), alpha 255, NaN -> byte 0;
//   * fg_render_scalar: channel 0 through a 256-entry RGBA table: FG_SCALAR_UNIT is the colormap rule
//     lut[min(trunc(x * 256), 255)] (x < 0 -> entry 0, NaN -> RGBA 0,0,0,0), FG_SCALAR_THRESHOLD the true mask
//     (x > 0.5 -> entry 255, else 0), FG_SCALAR_LOGIT the predicted mask by fg::flood -- the decision of
//     fg_mask_confusion.
// Every step is a single fp32 operation followed by a clamp or a truncation (__fadd_rn / __fmul_rn): nothing
// the compiler could contract or reassociate.
// Pure streaming, grid-stride, no LDS.  With a unit-stride source and a 16-byte aligned canvas (ptr and row_bytes)
// one lane converts the four pixels of one aligned 16-byte run of a canvas row: it reads 16 contiguous bytes of
// each plane (a wave covers 1 KiB per plane) and issues one 16-byte store.  The partial runs at a panel's left and
// right edge, and every pixel of the other cases (channels-last sources, unaligned canvases), are converted one
// pixel per lane with one 4-byte store each.
#include "fg_common.hpp"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ unsigned q255(float v) {      // v in [0, 1]
    return (unsigned)__fmul_rn(v, 255.f);
}

__device__ __forceinline__ unsigned clip_byte(float x, int mode) {
    if (!(x == x)) return 0u;
    const float v = mode == FG_RENDER_SIGNED ? __fmul_rn(__fadd_rn(x, 1.f), 0.5f) : x;
    return q255(fminf(fmaxf(v, 0.f), 1.f));
}

struct RgbPx {
    const float* p;            // channel 0 of image 0
    long long sc;
    int mode;
    static constexpr int planes = 3;
    __device__ __forceinline__ unsigned px(const float* v) const {
        return clip_byte(v[0], mode) | (clip_byte(v[1], mode) << 8) | (clip_byte(v[2], mode) << 16) | 0xFF000000u;
    }
};

struct ScalarPx {
    const float* p;
    long long sc;              // unused (one plane)
    int mode;
    const unsigned* lut;       // 256 RGBA entries
    static constexpr int planes = 1;
    __device__ __forceinline__ unsigned px(const float* v) const {
        const float x = v[0];
        if (mode == FG_SCALAR_THRESHOLD) return lut[x > 0.5f ? 255 : 0];
        if (mode == FG_SCALAR_LOGIT) return lut[fg::flood(x) ? 255 : 0];
        if (!(x == x)) return 0u;
        const float t = __fmul_rn(x, 256.f);
        return lut[t >= 255.f ? 255 : (t > 0.f ? (int)t : 0)];
    }
};

struct Geo {
    long long sn, sy, sx;
    int n, h, w;
    unsigned char* dst;
    long long row_bytes;
    int row0, col0, step_rows, step_cols;
};

// one lane per pixel
template <class P>
__global__ void __launch_bounds__(NT) render_pixels_kernel(P cv, Geo g) {
    const long long total = (long long)g.n * g.h * g.w;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % g.w);
        const long long r = i / g.w;
        const int y = (int)(r % g.h);
        const int ni = (int)(r / g.h);
        const float* s = cv.p + ni * g.sn + y * g.sy + x * g.sx;
        float v[P::planes];
#pragma unroll
        for (int c = 0; c < P::planes; ++c) v[c] = s[c * cv.sc];
        unsigned char* d = g.dst + (long long)(g.row0 + (long long)ni * g.step_rows + y) * g.row_bytes +
                           4ll * (g.col0 + (long long)ni * g.step_cols + x);
        *reinterpret_cast<unsigned*>(d) = cv.px(v);
    }
}

// one lane per aligned 4-pixel run of a canvas row (sx == 1, canvas 16-byte aligned); qpr = runs a panel row can
// touch at most, (w + 6) / 4
template <class P>
__global__ void __launch_bounds__(NT) render_quads_kernel(P cv, Geo g, int qpr) {
    const long long total = (long long)g.n * g.h * qpr;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(i % qpr);
        const long long r = i / qpr;
        const int y = (int)(r % g.h);
        const int ni = (int)(r / g.h);
        const long long c0 = g.col0 + (long long)ni * g.step_cols;      // the panel's first canvas column
        const int a = (int)(c0 & 3);
        const int x0 = 4 * q - a;                                       // panel column of the run's first pixel
        if (x0 >= g.w) continue;
        const float* s = cv.p + ni * g.sn + y * g.sy;
        unsigned char* d = g.dst + (long long)(g.row0 + (long long)ni * g.step_rows + y) * g.row_bytes + 4ll * c0;
        if (x0 >= 0 && x0 + 4 <= g.w) {
            float v[P::planes][4];
#pragma unroll
            for (int c = 0; c < P::planes; ++c) {
                const float* sp = s + c * cv.sc + x0;
                if ((reinterpret_cast<uintptr_t>(sp) & 15) == 0) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(sp);
                    v[c][0] = t[0]; v[c][1] = t[1]; v[c][2] = t[2]; v[c][3] = t[3];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[c][k] = sp[k];
                }
            }
            uint4 o;
            unsigned* op = reinterpret_cast<unsigned*>(&o);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pv[P::planes];
#pragma unroll
                for (int c = 0; c < P::planes; ++c) pv[c] = v[c][k];
                op[k] = cv.px(pv);
            }
            *reinterpret_cast<uint4*>(d + 4ll * x0) = o;
        } else {
            const int xa = x0 < 0 ? 0 : x0, xb = x0 + 4 < g.w ? x0 + 4 : g.w;
            for (int x = xa; x < xb; ++x) {
                float pv[P::planes];
#pragma unroll
                for (int c = 0; c < P::planes; ++c) pv[c] = s[c * cv.sc + x];
                *reinterpret_cast<unsigned*>(d + 4ll * x) = cv.px(pv);
            }
        }
    }
}

// 0, or the error code after recording why the panels do not fit
int check_canvas(const char* who, const void* src, int n, int h, int w, const fg_canvas& dst, int row0, int col0,
                 int step_rows, int step_cols) {
    if (!src || !dst.ptr) return fg::fail(FG_ERR_INVALID, "%s: null source or canvas", who);
    if (n <= 0 || h <= 0 || w <= 0 || dst.height <= 0 || dst.width <= 0)
        return fg::fail(FG_ERR_INVALID, "%s: sizes must be positive (n %d, h %d, w %d, canvas %d x %d)", who, n, h, w,
                        dst.height, dst.width);
    if (dst.row_bytes < 4ll * dst.width || (reinterpret_cast<uintptr_t>(dst.ptr) & 3) || (dst.row_bytes & 3))
        return fg::fail(FG_ERR_INVALID, "%s: canvas rows of %lld bytes (need >= %lld, 4-byte aligned)", who,
                        dst.row_bytes, 4ll * dst.width);
    // panel positions are linear in the image index: the first and the last bound them all
    for (int i = 0; i < n; i += (n > 1 ? n - 1 : 1)) {
        const long long r = row0 + (long long)i * step_rows, c = col0 + (long long)i * step_cols;
        if (r < 0 || c < 0 || r + h > dst.height || c + w > dst.width)
            return fg::fail(FG_ERR_INVALID, "%s: panel %d (%d x %d at row %lld, col %lld) leaves the %d x %d canvas",
                            who, i, h, w, r, c, dst.height, dst.width);
    }
    return 0;
}

template <class P>
int launch(const char* what, P cv, const fg_sview& src, int n, int h, int w, const fg_canvas& dst, int row0, int col0,
           int step_rows, int step_cols, hipStream_t stream) {
    const Geo g{src.sn, src.sy, src.sx, n, h, w, dst.ptr, dst.row_bytes, row0, col0, step_rows, step_cols};
    const bool quads = src.sx == 1 && (reinterpret_cast<uintptr_t>(dst.ptr) & 15) == 0 && (dst.row_bytes & 15) == 0;
    if (quads) {
        const int qpr = (w + 6) / 4;
        const long long total = (long long)n * h * qpr;
        hipLaunchKernelGGL(render_quads_kernel<P>, dim3(fg::blocks_for(total, NT, 4096)), dim3(NT), 0, stream, cv, g,
                           qpr);
    } else {
        const long long total = (long long)n * h * w;
        hipLaunchKernelGGL(render_pixels_kernel<P>, dim3(fg::blocks_for(total, NT, 4096)), dim3(NT), 0, stream, cv, g);
    }
    return fg::launched(what);
}

}  // namespace

FG_API int fg_render_rgb(fg_sview src, int n, int h, int w, int mode, fg_canvas dst, int row0, int col0,
                         int step_rows, int step_cols, hipStream_t stream) {
    if (int e = check_canvas("fg_render_rgb", src.ptr, n, h, w, dst, row0, col0, step_rows, step_cols)) return e;
    if (mode != FG_RENDER_SIGNED && mode != FG_RENDER_UNIT)
        return fg::fail(FG_ERR_INVALID, "fg_render_rgb: unknown mode %d", mode);
    return launch("render_rgb", RgbPx{src.ptr, src.sc, mode}, src, n, h, w, dst, row0, col0, step_rows, step_cols,
                  stream);
}

FG_API int fg_render_scalar(fg_sview src, int n, int h, int w, int mode, const unsigned char* lut, fg_canvas dst,
                            int row0, int col0, int step_rows, int step_cols, hipStream_t stream) {
    if (int e = check_canvas("fg_render_scalar", src.ptr, n, h, w, dst, row0, col0, step_rows, step_cols)) return e;
    if (mode != FG_SCALAR_UNIT && mode != FG_SCALAR_THRESHOLD && mode != FG_SCALAR_LOGIT)
        return fg::fail(FG_ERR_INVALID, "fg_render_scalar: unknown mode %d", mode);
    if (!lut || (reinterpret_cast<uintptr_t>(lut) & 3))
        return fg::fail(FG_ERR_INVALID, "fg_render_scalar: the colour table must be a 4-byte aligned device pointer");
    return launch("render_scalar", ScalarPx{src.ptr, 0, mode, reinterpret_cast<const unsigned*>(lut)}, src, n,
                  h, w, dst, row0, col0, step_rows, step_cols, stream);
}
