// cot_reduce.h -- the wave and workgroup reductions of the cotnet_amd HIP kernels (gfx950: 64 lanes per wave), stated once.
//
// Every function adds in an order fixed by its template arguments alone (for the workgroup forms: and by blockDim), so a result is
// equal bit for bit on every run.  Two contracts, told apart by the NAME -- a call site picks one and the emitted exchanges follow:
//   *_sum     the result is valid in lane 0 (thread 0 for the workgroup form) ONLY; the other lanes hold partial sums
//   *_all*    every lane of the wave (segment, workgroup) ends with the same bits
// One definition per name for the whole library: the host build of the kernels links every source into one library, where equal
// inline names merge.
#pragma once
#include "cot_common.h"

namespace cot {

// ---- lane-0 result: the __shfl_down tree, 6 stages ((l, l + 32), then (l, l + 16), ...).  Valid in lane 0 only.
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// ---- all-lanes result: the xor butterfly over aligned segments of SEG consecutive lanes (SEG a power of two, 64 = the wave),
// log2(SEG) stages, offsets SEG/2 down to 1.  Every lane of a segment ends with the segment's total, the same bits in each.
template <int SEG, typename T> __device__ __forceinline__ T seg_allsum(T v) {
#pragma unroll
    for (int o = SEG / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <typename T> __device__ __forceinline__ T wave_allsum(T v) { return seg_allsum<64>(v); }
__device__ __forceinline__ float wave_allmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ unsigned wave_allor(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
// a segment's sum for ONE reader per segment: the tree for a whole wave (valid in lane 0 only), the butterfly below that
template <int SEG> __device__ __forceinline__ float seg_sum(float v) {
    if (SEG == 64) return wave_sum(v);
    return seg_allsum<SEG>(v);
}

// ---- several values at once, all-lanes result.  Each value is summed exactly as by seg_allsum; the two forms differ in how the
// exchanges of different values interleave in the source, which decides how the kernels built on them are scheduled: rewritten as
// per-value calls of seg_allsum they compile to different (and unmeasured) code.
// array form: value by value
template <int NV, int SEG> __device__ __forceinline__ void seg_allsum_n(float (&v)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int o = SEG / 2; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
}
// two values over the wave, stage by stage (the fp64 statistics finalizers)
__device__ __forceinline__ void wave_allsum2(double& a, double& b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
}

// ---- workgroup sums of NV values: wave_sum per wave, lane 0 of wave w stores to smem[k * 16 + w], then the waves' sums are added
// in ascending order.  For both forms: smem holds NV * 16 floats, blockDim <= 1024.
// result in thread 0 only; blockDim a multiple of 64
template <int NV> __device__ __forceinline__ void block_sum(float (&v)[NV], float* smem) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) smem[k * 16 + wave] = v[k];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            float s = 0.f;
            for (int w = 0; w < nw; ++w) s += smem[k * 16 + w];
            v[k] = s;
        }
    }
}
// result in every thread; starts with a barrier, so smem may have been in use up to the call
template <int NV> __device__ __forceinline__ void block_allsum(float (&v)[NV], float* smem) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();  // previous use of smem is over
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) smem[k * 16 + wave] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        float s = 0.f;
        for (int w = 0; w < nw; ++w) s += smem[k * 16 + w];
        v[k] = s;
    }
}

}  // namespace cot
