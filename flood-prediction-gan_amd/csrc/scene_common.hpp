// What the scene kernels share (regions.hip, distance.hip): the class decision of a source plane, the entry checks
// and the per-root accumulation kernel behind fg_regions_stats, fg_regions_table and fg_depth_table.
//
// Accumulation.  The result of a table launch is one row per root, built by integer atomics only, so it does not
// depend on the order of arrival.  A lane owns a run of RUN pixels of a row and merges its pixels of equal root into
// one update; the updates a wave is left with at the end of its runs are merged across the wave by root, for the first
// MERGE_ROUNDS roots it holds (the interior of a large region, or the border of two: one or two sets of atomics per 256
// pixels instead of up to 64).  A launch's time is the number of its atomic instructions, which is what the merging is
// for.  What is accumulated is a policy P:
//   P::Acc                     the update: `root` (the pixel index that names the region), `n` (the pixels merged into
//                              it; 0: nothing to emit) and the policy's own fields
//   P::empty()                 the neutral element of every field (root -1, n 0)
//   p.weight(at)               the weight of the member pixel at index `at`; a pixel of weight <= 0 is left out
//   p.add(a, y, x, w)          pixel (y, x) of weight w joins a
//   P::merge(g, d)             one butterfly step: g joins the g of lane ^ d
//   p.emit(a)                  a's atomics; nothing when a.n <= 0 or an index read from memory is out of range
//   p.H, p.W, p.labels         the scene and its int32 labels plane (the root of each member pixel, negative on the
//                              others); a null plane takes the whole scene as one region of root 0
#pragma once
#include <limits.h>

#include "fg_common.hpp"

#define FG_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

namespace fg {
namespace scene {

constexpr int NT = 256;
constexpr int RUN = 4;                              // pixels of a row a lane of the accumulation kernel owns
constexpr int MERGE_ROUNDS = 4;                     // roots per wave whose updates are merged before the atomics

// channel 0 of a source of any strides, and the class of it a launch works on
struct ClassPlane {
    const float* p;
    long long sy, sx;
    int kind, target;
    __device__ __forceinline__ bool member(int y, int x) const {
        const float v = p[y * sy + x * sx];
        const bool wet = kind == FG_SCALAR_LOGIT ? fg::flood(v) : v > 0.5f;
        return wet == (target != 0);
    }
};

// 0, or the error code after recording which of kind / target no ClassPlane takes
inline int check_class(const char* who, int kind, int target) {
    if (kind != FG_SCALAR_THRESHOLD && kind != FG_SCALAR_LOGIT)
        return fg::fail(FG_ERR_INVALID, "%s: kind %d (FG_SCALAR_THRESHOLD or FG_SCALAR_LOGIT)", who, kind);
    if (target != 0 && target != 1) return fg::fail(FG_ERR_INVALID, "%s: target %d (0 dry, 1 flood)", who, target);
    return 0;
}

inline bool aligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// 0, or the error code after recording why an H x W scene cannot be indexed by int32
inline int check_scene(const char* who, int H, int W) {
    if (H <= 0 || W <= 0) return fg::fail(FG_ERR_INVALID, "%s: sizes must be positive (scene %d x %d)", who, H, W);
    if ((long long)H * W > INT_MAX)
        return fg::fail(FG_ERR_INVALID, "%s: a scene of %d x %d = %lld pixels: labels are int32 pixel indices, H * W "
                        "must be below 2^31", who, H, W, (long long)H * W);
    return 0;
}

// vec: W is a multiple of RUN and the labels plane 16-byte aligned, so a run is one 16-byte load
template <class P>
__global__ void __launch_bounds__(NT) accumulate_kernel(P p, int runs, int vec) {
    typedef typename P::Acc Acc;
    const long long total = (long long)p.H * runs;
    // the bound is the same for every lane of a block: the wave-wide steps below see whole waves
    for (long long i0 = blockIdx.x * (long long)NT; i0 < total; i0 += (long long)gridDim.x * NT) {
        const long long i = i0 + threadIdx.x;
        Acc a = P::empty();
        if (i < total) {
            const int y = (int)(i / runs), xq = RUN * (int)(i % runs);
            const long long at = (long long)y * p.W + xq;
            int l[RUN];
            if (!p.labels) {
#pragma unroll
                for (int e = 0; e < RUN; ++e) l[e] = xq + e < p.W ? 0 : -1;
            } else if (vec) {
                const int4 t = *reinterpret_cast<const int4*>(p.labels + at);
                l[0] = t.x; l[1] = t.y; l[2] = t.z; l[3] = t.w;
            } else {
#pragma unroll
                for (int e = 0; e < RUN; ++e) l[e] = xq + e < p.W ? p.labels[at + e] : -1;
            }
#pragma unroll
            for (int e = 0; e < RUN; ++e) {
                if (l[e] < 0) continue;
                const long long w = p.weight(at + e);
                if (w <= 0) continue;
                if (l[e] != a.root) {
                    p.emit(a);
                    a = P::empty();
                    a.root = l[e];
                }
                p.add(a, y, xq + e, w);
            }
        }
        // the updates the wave is left with, merged by root: the first lane that still holds one leads a round, the
        // lanes of its root join it.  MERGE_ROUNDS rounds cover the roots a wave of a smooth mask meets; what a
        // speckled one leaves over goes out lane by lane.
        // variant: `pending` loses at least its lowest set bit every round (the leader is in its own group)
        const int lane = threadIdx.x & 63;
        unsigned long long pending = __ballot(a.n > 0);
        for (int round = 0; pending != 0 && round < MERGE_ROUNDS; ++round) {
            const int leader = __ffsll((long long)pending) - 1;
            const int r0 = __shfl(a.root, leader);
            const bool mine = a.n > 0 && a.root == r0;
            const unsigned long long group = __ballot(mine);
            if (__popcll(group) == 1) {
                if (mine) p.emit(a);
            } else {
                // butterfly over the wave; the lanes outside the group hold the neutral element of each field
                Acc g = mine ? a : P::empty();
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) P::merge(g, d);
                g.root = r0;
                if (lane == leader) p.emit(g);
            }
            if (mine) a.n = 0;
            pending &= ~group;
        }
        p.emit(a);                  // (nothing when a round took it: n is 0)
    }
}

template <class P>
inline void launch_accumulate(const P& p, hipStream_t stream) {
    const int runs = (p.W + RUN - 1) / RUN;
    const int vec = p.W % RUN == 0 && aligned(p.labels, 16);
    hipLaunchKernelGGL(accumulate_kernel<P>, dim3(fg::blocks_for((long long)p.H * runs, NT, 4096)), dim3(NT), 0, stream,
                       p, runs, vec);
}

}  // namespace scene
}  // namespace fg
