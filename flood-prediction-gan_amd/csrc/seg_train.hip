// Training the flood-segmentation U-Net (models/segmentation_model.py:250-277): the two device passes its
// backward needs beside the conv engine and the BatchNorm kernels.
//
//   * fg_bce_logits: nn.BCEWithLogitsLoss() (mean) over channel 0 of a logits view against a contiguous
//     [N, 1, H, W] target, its gradient (sigmoid(z) - t) * gscale into channel 0 of a gradient view (every other
//     channel and the border written as zero), and train_model's accuracy count
//     #{(sigmoid(z) > 0.5) == (t > 0.5)} -- one pass over the gradient view's padded extent.  sigmoid(z) > 0.5
//     is decided as z > 0 (the fp32 sigmoid of a positive z is > 0.5 down to z ~ 6e-8, of z <= 0 never).
//   * fg_flood_mask_bce: the same pass with the target taken from a second logits view, t = flood(r) ? 1 : 0 (the
//     flood-mask loss of floodgan.segmentation.FloodMaskLoss); its count is the number of agreeing mask pixels,
//     tp + tn of fg_mask_confusion on the same two views.
//   * fg_maxpool2_bwd: the gradient of fg_maxpool2, routed to the FIRST maximum of each 2x2 window in the scan
//     order (0,0), (0,1), (1,0), (1,1) (ATen's rule: a later element wins only when strictly greater, or NaN),
//     recomputed from the saved source; all four positions are written, so no pre-zeroing and no dependence on
//     execution order.
//
// Reductions are two-level and deterministic as in bnorm.hip: fp32 inside a thread, fp64 across the threads of a
// block (LDS tree in a fixed order) and across blocks (a one-block finalize kernel); no floating-point atomics.
#include "fg_common.hpp"

namespace {

constexpr int NT = 256;
constexpr int BCE_BLOCKS_MAX = 1024;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }

// The two targets of the BCE pass: a contiguous [N, 1, H, W] tensor (fg_bce_logits; an element counts as correct when
// (z > 0) == (t > 0.5)), or the flood mask of a second logits view (fg_flood_mask_bce: t = fg::flood(r), the decision
// fg_mask_confusion and the renderer make; correct when fg::flood(z) makes the same one)
struct DenseTarget {
    const float* __restrict__ p;
    __device__ __forceinline__ float operator()(int n, int y, int x, int h, int w) const {
        return p[((size_t)n * h + y) * w + x];
    }
    __device__ __forceinline__ bool agrees(float v, float t) const { return (v > 0.f) == (t > 0.5f); }
};
struct MaskTarget {
    fg_view r;
    __device__ __forceinline__ float operator()(int n, int y, int x, int, int) const {
        return fg::flood(r.ptr[fg::vidx(r, n, y, x)]) ? 1.f : 0.f;
    }
    __device__ __forceinline__ bool agrees(float v, float t) const { return fg::flood(v) == (t != 0.f); }
};

// thread = one pixel of g's padded extent (all of its channel quads); partial[blk] = (loss sum, correct count)
template <class Target>
__global__ void __launch_bounds__(NT) bce_logits_kernel(fg_view z, const Target target, float gscale, fg_view g,
                                                        double* __restrict__ partial) {
    const int hp = g.h + 2 * g.pad, wp = g.w + 2 * g.pad, C4 = g.c_alloc / 4;
    const long long total = (long long)g.n * hp * wp;
    float loss = 0.f;
    unsigned correct = 0;
    for (long long idx = blockIdx.x * (long long)NT + threadIdx.x; idx < total; idx += (long long)gridDim.x * NT) {
        const int xx = (int)(idx % wp) - g.pad;
        const long long r = idx / wp;
        const int yy = (int)(r % hp) - g.pad;
        const int n = (int)(r / hp);
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (xx >= 0 && xx < g.w && yy >= 0 && yy < g.h) {
            const float v = z.ptr[fg::vidx(z, n, yy, xx)];
            const float t = target(n, yy, xx, g.h, g.w);
            const float e = expf(-fabsf(v));                      // in (0, 1]
            loss += fmaxf(v, 0.f) - v * t + log1pf(e);
            // sigmoid(v) and 1 - sigmoid(v), each without cancellation: s - t = s (1 - t) - (1 - s) t
            const float big = 1.f / (1.f + e), small = e / (1.f + e);
            const float s = v >= 0.f ? big : small, s1 = v >= 0.f ? small : big;
            o[0] = (s * (1.f - t) - s1 * t) * gscale;
            correct += target.agrees(v, t);
        }
        float* dst = g.ptr + (size_t)idx * g.c_alloc;
        st4(dst, o);
        for (int q = 1; q < C4; ++q) st4(dst + 4 * q, f32x4{0.f, 0.f, 0.f, 0.f});
    }
    __shared__ double red[NT][2];
    red[threadIdx.x][0] = (double)loss;
    red[threadIdx.x][1] = (double)correct;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            red[threadIdx.x][0] += red[threadIdx.x + s][0];
            red[threadIdx.x][1] += red[threadIdx.x + s][1];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = red[0][0];
        partial[2 * blockIdx.x + 1] = red[0][1];
    }
}

__global__ void __launch_bounds__(NT) bce_finalize_kernel(const double* __restrict__ partial, int blocks,
                                                          double count, float* loss, long long* correct) {
    __shared__ double red[NT][2];
    double a = 0, b = 0;
    for (int k = threadIdx.x; k < blocks; k += NT) {
        a += partial[2 * k];
        b += partial[2 * k + 1];
    }
    red[threadIdx.x][0] = a;
    red[threadIdx.x][1] = b;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            red[threadIdx.x][0] += red[threadIdx.x + s][0];
            red[threadIdx.x][1] += red[threadIdx.x + s][1];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *loss = (float)(red[0][0] / count);
        if (correct) *correct = (long long)(red[0][1] + 0.5);      // exact: counts below 2^53
    }
}

// thread = (window, channel quad) over ceil(h / 2) x ceil(w / 2) windows of src: an odd last row / column is outside
// every pooled window (floor output size) and gets zero
__global__ void __launch_bounds__(NT) maxpool2_bwd_kernel(fg_view src, fg_view g, fg_view dst, unsigned char* choice) {
    const int C4 = src.c_alloc / 4, wh = (src.h + 1) / 2, ww = (src.w + 1) / 2;
    const long long total = (long long)src.n * wh * ww * C4;
    for (long long idx = blockIdx.x * (long long)NT + threadIdx.x; idx < total; idx += (long long)gridDim.x * NT) {
        const int c4 = (int)(idx % C4);
        long long pix = idx / C4;
        const int x = (int)(pix % ww);
        pix /= ww;
        const int y = (int)(pix % wh);
        const int n = (int)(pix / wh);
        const bool full = y < g.h && x < g.w;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        if (!full) {
            for (int k = 0; k < 4; ++k) {
                const int yy = 2 * y + (k >> 1), xx = 2 * x + (k & 1);
                if (yy < src.h && xx < src.w) st4(dst.ptr + fg::vidx(dst, n, yy, xx) + 4 * c4, zero);
            }
            continue;
        }
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = ld4(src.ptr + fg::vidx(src, n, 2 * y + (k >> 1), 2 * x + (k & 1)) + 4 * c4);
        const f32x4 gy = ld4(g.ptr + fg::vidx(g, n, y, x) + 4 * c4);
        int sel[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float m = v[0][e];
            int s = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (v[k][e] > m || v[k][e] != v[k][e]) {
                    m = v[k][e];
                    s = k;
                }
            sel[e] = s;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = sel[e] == k ? gy[e] : 0.f;
            st4(dst.ptr + fg::vidx(dst, n, 2 * y + (k >> 1), 2 * x + (k & 1)) + 4 * c4, o);
        }
        if (choice) {
            // NHWC [n, g.h, g.w, C] bytes
            unsigned* c =
                reinterpret_cast<unsigned*>(choice + (((size_t)n * g.h + y) * g.w + x) * src.c_alloc + 4 * c4);
            *c = (unsigned)sel[0] | (unsigned)sel[1] << 8 | (unsigned)sel[2] << 16 | (unsigned)sel[3] << 24;
        }
    }
}

bool ok_view(const fg_view& v) {
    return v.ptr && v.n > 0 && v.h > 0 && v.w > 0 && v.c_alloc > 0 && v.pad >= 0 && v.c_alloc % 4 == 0 &&
           ((uintptr_t)v.ptr & 15) == 0;
}

}  // namespace

FG_API long long fg_bce_logits_workspace_doubles(void) { return 2 * BCE_BLOCKS_MAX; }

FG_API int fg_bce_logits(fg_view logits, const float* target, float gscale, fg_view grad, float* loss,
                         long long* correct, double* work, hipStream_t stream) {
    if (!ok_view(logits) || !ok_view(grad) || !target || !loss || !work || grad.n != logits.n ||
        grad.h != logits.h || grad.w != logits.w)
        return fg::fail(FG_ERR_INVALID, "fg_bce_logits: bad args (logits %dx%dx%d, gradient %dx%dx%d c %d)", logits.n,
                        logits.h, logits.w, grad.n, grad.h, grad.w, grad.c_alloc);
    const long long total = (long long)grad.n * (grad.h + 2 * grad.pad) * (grad.w + 2 * grad.pad);
    const int blocks = fg::blocks_for(total, NT, BCE_BLOCKS_MAX);
    hipLaunchKernelGGL(bce_logits_kernel<DenseTarget>, dim3(blocks), dim3(NT), 0, stream, logits, DenseTarget{target},
                       gscale, grad, work);
    int e = fg::launched("bce_logits");
    if (e) return e;
    hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(NT), 0, stream, work, blocks,
                       (double)logits.n * logits.h * logits.w, loss, correct);
    return fg::launched("bce_finalize");
}

FG_API int fg_flood_mask_bce(fg_view logits, fg_view ref_logits, float gscale, fg_view grad, void* result, double* work,
                             hipStream_t stream) {
    if (!ok_view(logits) || !ok_view(grad) || !ref_logits.ptr || ref_logits.c_alloc <= 0 || ref_logits.pad < 0 ||
        !result || ((uintptr_t)result & 7) || !work || grad.n != logits.n || grad.h != logits.h ||
        grad.w != logits.w || ref_logits.n != logits.n || ref_logits.h != logits.h || ref_logits.w != logits.w)
        return fg::fail(FG_ERR_INVALID,
                        "fg_flood_mask_bce: bad args (logits %dx%dx%d, reference %dx%dx%d, gradient %dx%dx%d c %d)",
                        logits.n, logits.h, logits.w, ref_logits.n, ref_logits.h, ref_logits.w, grad.n, grad.h, grad.w,
                        grad.c_alloc);
    const long long total = (long long)grad.n * (grad.h + 2 * grad.pad) * (grad.w + 2 * grad.pad);
    const int blocks = fg::blocks_for(total, NT, BCE_BLOCKS_MAX);
    hipLaunchKernelGGL(bce_logits_kernel<MaskTarget>, dim3(blocks), dim3(NT), 0, stream, logits,
                       MaskTarget{ref_logits}, gscale, grad, work);
    int e = fg::launched("flood_mask_bce");
    if (e) return e;
    // result: 16 bytes, the fp32 loss in the low half (its upper word is not written), the int64 count in the high
    hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(NT), 0, stream, work, blocks,
                       (double)logits.n * logits.h * logits.w, reinterpret_cast<float*>(result),
                       reinterpret_cast<long long*>(result) + 1);
    return fg::launched("bce_finalize");
}

FG_API int fg_maxpool2_bwd(fg_view src, fg_view g_pooled, fg_view g_src, unsigned char* choice, hipStream_t stream) {
    if (!ok_view(src) || !ok_view(g_pooled) || !ok_view(g_src) || ((uintptr_t)choice & 3) ||
        g_pooled.c_alloc != src.c_alloc || g_src.c_alloc != src.c_alloc || g_pooled.n != src.n || g_src.n != src.n ||
        g_pooled.h != src.h / 2 || g_pooled.w != src.w / 2 || g_src.h != src.h || g_src.w != src.w ||
        g_pooled.h < 1 || g_pooled.w < 1)
        return fg::fail(FG_ERR_INVALID,
                        "fg_maxpool2_bwd: bad args (source %dx%dx%d c %d, pooled gradient %dx%dx%d c %d)", src.n,
                        src.h, src.w, src.c_alloc, g_pooled.n, g_pooled.h, g_pooled.w, g_pooled.c_alloc);
    const long long total = (long long)src.n * ((src.h + 1) / 2) * ((src.w + 1) / 2) * (src.c_alloc / 4);
    hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(fg::blocks_for(total, NT, 4096)), dim3(NT), 0, stream, src, g_pooled,
                       g_src, choice);
    return fg::launched("maxpool2_bwd");
}
