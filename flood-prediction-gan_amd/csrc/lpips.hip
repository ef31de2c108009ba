// LPIPS (torchmetrics LearnedPerceptualImagePatchSimilarity, net_type="alex") pieces the conv engine has no kernel
// for (models/model.py:404-406 is the reference's call):
//   * fg_lpips_stem: the scaling layer (x - shift) / scale, zero pad 2 (applied AFTER the scaling: a tap outside
//     the image contributes exactly 0), AlexNet's Conv2d(3, 64, 11, stride 4, padding 2), bias and ReLU in one
//     direct fp32 FMA kernel.  K = 363 and 11 taps per axis do not fit the engine's rtab[8] / stab[8].
//   * fg_maxpool3s2: nn.MaxPool2d(3, 2) (floor, no padding) over NHWC interiors into the interior of a
//     destination that may carry the next conv's zero border.
//   * fg_lpips_layer: one tap's distance d_k[i] = mean_{y,x} sum_c w[c] (f0_c / n(f0) - f1_c / n(f1))^2 with
//     n(f) = sqrt(1e-8 + sum_c f_c^2), per image, in one read of both feature vectors.
// The distance is reduced deterministically: fp32 inside a pixel (16 lanes, DPP), fp64 across pixels per 16-lane
// group, groups and blocks combined in a fixed order by a second small launch; no floating-point atomics.
#include "fg_common.hpp"

namespace {

constexpr int NT = 256;

// ---------------------------------------------------------------------------------------------- stem
constexpr int ST_T = 8;                              // output tile edge per block
constexpr int ST_K = 11, ST_S = 4, ST_P = 2;         // kernel, stride, padding
constexpr int ST_C = 3, ST_O = 64;
constexpr int ST_IN = (ST_T - 1) * ST_S + ST_K;      // staged input patch edge (39)
constexpr int ST_Q = (ST_IN + ST_S - 1) / ST_S;      // patch columns per stride phase (10)
// A patch row is stored de-interleaved by column phase (column lx at (lx % 4) * ST_Q + lx / 4): the 8 output
// columns of a wave then read consecutive words for a tap instead of words 4 apart.  Pitch = 2 (mod 8) puts the 4
// output rows of a 32-lane group (4 patch rows apart) on banks 0, 8, 16, 24: no conflicts for ds_read_b32.
constexpr int ST_PITCH = 42;
static_assert(ST_PITCH >= ST_S * ST_Q && ST_PITCH % 8 == 2, "stem patch pitch");

// the scaling layer's constants (lpips ScalingLayer): x' = (x - shift) / scale per RGB channel
__constant__ const float ST_SHIFT[ST_C] = {-0.030f, -0.088f, -0.188f};
__constant__ const float ST_SCALE[ST_C] = {0.458f, 0.448f, 0.450f};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// grid (tiles_x, tiles_y, n): an 8 x 8 tile of output pixels x 64 channels of one image.  Wave q computes
// channels 16q .. 16q + 15 for the tile's 64 pixels (lane = pixel): the weights wt[k][64] (k = (c, r, s)) of a
// tap are wave-uniform, so every input value read from LDS feeds 16 FMAs against scalar operands.
__global__ __launch_bounds__(NT) void lpips_stem_kernel(fg_sview x, int h, int w, const float* __restrict__ wt,
                                                        const float* __restrict__ bias, fg_view y, int img0) {
    __shared__ float patch[ST_C][ST_IN][ST_PITCH];
    const int n = blockIdx.z;
    const int oy0 = blockIdx.y * ST_T, ox0 = blockIdx.x * ST_T;
    const int iy0 = oy0 * ST_S - ST_P, ix0 = ox0 * ST_S - ST_P;
    const float* xp = x.ptr + (long long)n * x.sn;
    for (int i = threadIdx.x; i < ST_C * ST_IN * ST_IN; i += NT) {
        const int c = i / (ST_IN * ST_IN);
        const int rem = i - c * (ST_IN * ST_IN);
        const int ly = rem / ST_IN, lx = rem - ly * ST_IN;
        const int iy = iy0 + ly, ix = ix0 + lx;
        float v = 0.f;                                               // outside the image: the conv's zero padding
        if (iy >= 0 && iy < h && ix >= 0 && ix < w)
            v = (xp[c * x.sc + iy * x.sy + ix * x.sx] - ST_SHIFT[c]) / ST_SCALE[c];
        patch[c][ly][(lx & 3) * ST_Q + (lx >> 2)] = v;
    }
    __syncthreads();
    const int cg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int px = lane & 7, py = lane >> 3;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = bias[cg * 16 + j];
    for (int c = 0; c < ST_C; ++c)
        for (int r = 0; r < ST_K; ++r) {
            const float* row = &patch[c][py * ST_S + r][px];
            const float* wk = wt + (size_t)((c * ST_K + r) * ST_K) * ST_O + cg * 16;
#pragma unroll
            for (int s = 0; s < ST_K; ++s) {
                const float v = row[(s & 3) * ST_Q + (s >> 2)];
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[j] = fmaf(v, wk[s * ST_O + j], acc[j]);
            }
        }
    const int oy = oy0 + py, ox = ox0 + px;
    if (oy < y.h && ox < y.w) {
        float* dst = y.ptr + fg::vidx(y, img0 + n, oy, ox) + cg * 16;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fmaxf(acc[4 * q + j], 0.f);
            st4(dst + 4 * q, o);
        }
    }
}

// ---------------------------------------------------------------------------------------------- pool
__device__ __forceinline__ f32x4 max4(f32x4 a, f32x4 b) {
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaxf(a[j], b[j]);
    return o;
}

// one thread per (output pixel, 4-channel group): consecutive threads read consecutive 16-byte channel vectors
__global__ void maxpool3s2_kernel(fg_view src, fg_view dst) {
    const int C4 = src.c_alloc / 4;
    const long long total = (long long)dst.n * dst.h * dst.w * C4;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        long long pix = idx / C4;
        const int x = (int)(pix % dst.w);
        pix /= dst.w;
        const int y = (int)(pix % dst.h);
        const int n = (int)(pix / dst.h);
        f32x4 m = ld4(src.ptr + fg::vidx(src, n, 2 * y, 2 * x) + 4 * c4);
#pragma unroll
        for (int t = 1; t < 9; ++t) m = max4(m, ld4(src.ptr + fg::vidx(src, n, 2 * y + t / 3, 2 * x + t % 3) + 4 * c4));
        st4(dst.ptr + fg::vidx(dst, n, y, x) + 4 * c4, m);
    }
}

// ---------------------------------------------------------------------------------------------- layer distance
constexpr int LY_LANES = 16;                 // lanes per pixel (one DPP row)
constexpr int LY_PIX = NT / LY_LANES;        // pixels per block per sweep
constexpr int LY_MAX_CHUNKS = 256;
constexpr float LY_EPS = 1e-8f;

int layer_chunks(int h, int w) {
    const long long c = ((long long)h * w + 4 * LY_PIX - 1) / (4 * LY_PIX);
    return (int)(c < 1 ? 1 : c > LY_MAX_CHUNKS ? LY_MAX_CHUNKS : c);
}

// grid (chunks, n); IT = C / 64: lane l of a pixel's 16 holds channels 4 (l + 16 i) .. + 3, i < IT, so each sweep
// of i reads 256 contiguous bytes per pixel.  part[img * chunks + chunk] = sum over the block's pixels.
template <int IT>
__global__ __launch_bounds__(NT) void lpips_layer_kernel(fg_view f0, fg_view f1, const float* __restrict__ wgt,
                                                         double* __restrict__ part) {
    const int img = blockIdx.y, chunks = gridDim.x;
    const int grp = threadIdx.x / LY_LANES, l = threadIdx.x % LY_LANES;
    const int npix = f0.h * f0.w;
    f32x4 wv[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) wv[i] = ld4(wgt + 4 * (l + LY_LANES * i));
    double acc = 0.0;
    for (int base = blockIdx.x * LY_PIX; base < npix; base += chunks * LY_PIX) {     // block-uniform trip count
        const int p = base + grp;
        const bool valid = p < npix;
        f32x4 a[IT], b[IT];
#pragma unroll
        for (int i = 0; i < IT; ++i) a[i] = b[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (valid) {
            const int py = p / f0.w, px = p - py * f0.w;
            const float* pa = f0.ptr + fg::vidx(f0, img, py, px) + 4 * l;
            const float* pb = f1.ptr + fg::vidx(f1, img, py, px) + 4 * l;
#pragma unroll
            for (int i = 0; i < IT; ++i) {
                a[i] = ld4(pa + 4 * LY_LANES * i);
                b[i] = ld4(pb + 4 * LY_LANES * i);
            }
        }
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int i = 0; i < IT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sa = fmaf(a[i][j], a[i][j], sa);
                sb = fmaf(b[i][j], b[i][j], sb);
            }
        const float na = sqrtf(LY_EPS + fg::row_sum16(sa)), nb = sqrtf(LY_EPS + fg::row_sum16(sb));
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < IT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t = a[i][j] / na - b[i][j] / nb;
                d = fmaf(wv[i][j] * t, t, d);
            }
        d = fg::row_sum16(d);
        if (valid) acc += (double)d;
    }
    __shared__ double red[LY_PIX];
    if (l == 0) red[grp] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
        for (int i = 1; i < LY_PIX; ++i) s += red[i];
        part[(size_t)img * chunks + blockIdx.x] = s;
    }
}

// one wave per image: lane l sums chunks l, l + 64, ... in order, the lanes are combined by a fixed xor butterfly
// (the same pairing in every run), then the spatial mean
__global__ __launch_bounds__(64) void lpips_layer_finalize_kernel(int chunks, double inv_count,
                                                                  const double* __restrict__ part, double* out,
                                                                  int accumulate) {
    const int i = blockIdx.x;
    double s = 0.0;
    for (int c = threadIdx.x; c < chunks; c += 64) s += part[(size_t)i * chunks + c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) {
        s *= inv_count;
        out[i] = accumulate ? out[i] + s : s;
    }
}

bool ok_view(const fg_view& v) {
    return v.ptr && v.n > 0 && v.h > 0 && v.w > 0 && v.c_alloc > 0 && v.pad >= 0 && ((uintptr_t)v.ptr & 15) == 0 &&
           v.c_alloc % 4 == 0;
}

template <int IT>
void launch_layer(fg_view f0, fg_view f1, const float* w, int chunks, double* work, hipStream_t stream) {
    hipLaunchKernelGGL(lpips_layer_kernel<IT>, dim3(chunks, f0.n), dim3(NT), 0, stream, f0, f1, w, work);
}

}  // namespace

FG_API int fg_lpips_stem(fg_sview x, int n, int h, int w, const float* wt, const float* bias, fg_view y, int img0,
                         hipStream_t stream) {
    if (!x.ptr || !wt || !bias || n <= 0 || !ok_view(y) || y.c_alloc != ST_O || img0 < 0 ||
        img0 + n > y.n || h + 2 * ST_P < ST_K || w + 2 * ST_P < ST_K || y.h != (h + 2 * ST_P - ST_K) / ST_S + 1 ||
        y.w != (w + 2 * ST_P - ST_K) / ST_S + 1 || ((uintptr_t)wt & 15) != 0)
        return fg::fail(FG_ERR_INVALID, "fg_lpips_stem: bad args (%d images of %dx%d into %dx%dx%d c %d at image %d)",
                        n, h, w, y.n, y.h, y.w, y.c_alloc, img0);
    const dim3 grid((y.w + ST_T - 1) / ST_T, (y.h + ST_T - 1) / ST_T, n);
    hipLaunchKernelGGL(lpips_stem_kernel, grid, dim3(NT), 0, stream, x, h, w, wt, bias, y, img0);
    return fg::launched("lpips_stem");
}

FG_API int fg_maxpool3s2(fg_view src, fg_view dst, hipStream_t stream) {
    if (!ok_view(src) || !ok_view(dst) || dst.c_alloc != src.c_alloc || dst.n != src.n || src.h < 3 || src.w < 3 ||
        dst.h != (src.h - 3) / 2 + 1 || dst.w != (src.w - 3) / 2 + 1)
        return fg::fail(FG_ERR_INVALID, "fg_maxpool3s2: bad args (%dx%dx%d c %d -> %dx%dx%d c %d)", src.n, src.h,
                        src.w, src.c_alloc, dst.n, dst.h, dst.w, dst.c_alloc);
    const long long total = (long long)dst.n * dst.h * dst.w * (dst.c_alloc / 4);
    hipLaunchKernelGGL(maxpool3s2_kernel, dim3(fg::blocks_for(total, NT, 8192)), dim3(NT), 0, stream, src, dst);
    return fg::launched("maxpool3s2");
}

FG_API long long fg_lpips_workspace_doubles(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return (long long)n * layer_chunks(h, w);
}

FG_API int fg_lpips_layer(fg_view f0, fg_view f1, int c, const float* w, double* out, int accumulate, double* work,
                          hipStream_t stream) {
    if (!ok_view(f0) || !ok_view(f1) || !w || !out || !work || f1.n != f0.n || f1.h != f0.h || f1.w != f0.w ||
        c <= 0 || c % 64 != 0 || c > 512 || f0.c_alloc < c || f1.c_alloc < c || ((uintptr_t)w & 15) != 0 ||
        f0.n > 65535)
        return fg::fail(FG_ERR_INVALID, "fg_lpips_layer: bad args (c = %d must be a multiple of 64 up to 512; views "
                        "%dx%dx%d c %d and %dx%dx%d c %d)", c, f0.n, f0.h, f0.w, f0.c_alloc, f1.n, f1.h, f1.w,
                        f1.c_alloc);
    const int chunks = layer_chunks(f0.h, f0.w);
    switch (c / 64) {
        case 1: launch_layer<1>(f0, f1, w, chunks, work, stream); break;
        case 2: launch_layer<2>(f0, f1, w, chunks, work, stream); break;
        case 3: launch_layer<3>(f0, f1, w, chunks, work, stream); break;
        case 4: launch_layer<4>(f0, f1, w, chunks, work, stream); break;
        case 5: launch_layer<5>(f0, f1, w, chunks, work, stream); break;
        case 6: launch_layer<6>(f0, f1, w, chunks, work, stream); break;
        case 7: launch_layer<7>(f0, f1, w, chunks, work, stream); break;
        default: launch_layer<8>(f0, f1, w, chunks, work, stream); break;
    }
    int e = fg::launched("lpips_layer");
    if (e) return e;
    hipLaunchKernelGGL(lpips_layer_finalize_kernel, dim3(f0.n), dim3(64), 0, stream, chunks,
                       1.0 / ((double)f0.h * f0.w), work, out, accumulate);
    return fg::launched("lpips_layer_finalize");
}
