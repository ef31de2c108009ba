// The absmax-slot protocol, device side: the only code that knows the layout of a slot.
//
// A slot is FG_AMAX_SHARDS floats (include/floodgan.h).  The maximum over its shards bounds the |values| of the
// operand it belongs to; every consumer derives its power-of-two scale from that maximum (pow2_scale).  A slot only
// ever grows between two host-side resets, by an atomic max on the bit patterns of non-negative floats (uint order =
// float order; NaN sorts high), in one of three ways:
//   raise_block_max  a kernel that measures its output: each block folds its threads' max |v| into one shard;
//   raise_bound      a kernel that knows a bound without measuring: one thread publishes it;
//   (the host)       ops.amax_slot / ops.absmax hand out and measure slots (fg_absmax is raise_block_max too).
// Which shard a block raises is invisible to the consumers: the shards only spread the atomics.
#pragma once
#include "fg_common.hpp"

namespace fg {

static_assert(FG_AMAX_SHARDS == 64, "a wave reads a slot one shard per lane (pow2_scale)");

// the bit pattern of |v|
__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ __forceinline__ unsigned abs_bits(const f32x4& v) {
    return max(max(abs_bits(v[0]), abs_bits(v[1])), max(abs_bits(v[2]), abs_bits(v[3])));
}

// The maximum of one value per thread over a 1-D block of NT threads (NT = 0: blockDim.x threads), valid on thread 0.
// Any multiple of 64 up to 1024 threads.  Precondition: every thread of the block reaches the call (it holds
// barriers).  It may be called any number of times in a kernel: the barrier before the LDS write ends the previous
// call's read.  ONCE drops that barrier for a kernel in which it measurably costs (profiles/amax_slot): such a
// call has an LDS array of its own, so it may stand beside calls of the general form, but only one ONCE call of a
// block size may be reached per kernel.
constexpr bool kOnce = true;
template <int NT = 0, bool ONCE = false>
__device__ __forceinline__ unsigned block_max(unsigned m) {
    static_assert(NT % 64 == 0 && NT <= 1024, "block_max: whole waves, at most 1024 threads");
    constexpr int MAXW = NT ? NT / 64 : 16;
    const int nw = NT ? NT / 64 : (int)(blockDim.x >> 6);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    __shared__ unsigned red[MAXW];
    if (!ONCE) __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < nw; ++i) m = max(m, red[i]);
    return m;
}

// raise shard id % FG_AMAX_SHARDS of a slot to the block's max of m = abs_bits of what each thread wrote
// (block_max's precondition; grids of more than one dimension pass a linear block id)
template <int NT = 0, bool ONCE = false>
__device__ __forceinline__ void raise_block_max(float* slot, unsigned m, int id = blockIdx.x) {
    m = block_max<NT, ONCE>(m);
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(slot) + (id & (FG_AMAX_SHARDS - 1)), m);
}

// raise a slot to a bound >= 0 that the kernel knows without measuring: called by ONE thread of the grid
__device__ __forceinline__ void raise_bound(float* slot, float bound) {
    atomicMax(reinterpret_cast<unsigned*>(slot), __float_as_uint(bound));
}

// the power-of-two scale s = 2^(14-e) of a bound m < 2^e (1 for 0 / non-finite): |v * s| < 2^14
__device__ __forceinline__ float pow2_of(float m) {
    if (!(m > 0.f) || !(m < 3.0e38f)) return 1.f;
    int e;
    frexpf(m, &e);                                        // m < 2^e
    return ldexpf(1.f, 14 - e);
}

// max over an absmax slot's FG_AMAX_SHARDS shards (every lane of the wave gets it)
__device__ __forceinline__ float pow2_scale_max(const float* amax) {
    unsigned b = __float_as_uint(amax[threadIdx.x & (FG_AMAX_SHARDS - 1)]) & 0x7fffffffu;
#pragma unroll
    for (int off = 1; off < FG_AMAX_SHARDS; off <<= 1) b = max(b, (unsigned)__shfl_xor((int)b, off));
    return __uint_as_float(b);
}

// power-of-two operand scale from an absmax slot (max over its FG_AMAX_SHARDS shards, one per
// lane, reduced across the wave): |v * s| < 2^14
__device__ __forceinline__ float pow2_scale(const float* amax) {
    unsigned b = amax ? __float_as_uint(amax[threadIdx.x & (FG_AMAX_SHARDS - 1)]) & 0x7fffffffu : 0u;
#pragma unroll
    for (int off = 1; off < FG_AMAX_SHARDS; off <<= 1) b = max(b, (unsigned)__shfl_xor((int)b, off));
    return pow2_of(__uint_as_float(b));
}

}  // namespace fg
