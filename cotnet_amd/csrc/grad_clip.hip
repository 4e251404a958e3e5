// grad_clip.hip -- the global L2 norm of the gradients in their flat buckets and what the optimizer step makes of it, on the device,
// gfx950: a clip coefficient and a skip flag in one 32-byte block in device memory (cot_clip_state, include/cotnet_amd.h), which
// sgd_flat_kernel's clip form (optim.hip) reads when it runs.
//
// Reference: train.py:269-274 (`loss.backward(); dispatch_clip_grad(...); optimizer.step()`), utils/clip_grad.py:34-35 (mode 'norm' =
// torch.nn.utils.clip_grad_norm_: one norm per parameter tensor, a norm of the norms, one multiply per tensor, and -- for
// error_if_nonfinite or any logging -- a host read).  Here the gradients already lie in a few flat buckets, a step replayed from a HIP
// graph has no host code between its kernels, and the multiply is the `gscale` the SGD kernel applies anyway: what is left is a pure
// read of the buckets (51 MB for CoTNet-50 in bf16) and one tiny kernel.
//
//   grad_sumsq_kernel        HBM-bound.  COT_GRAD_NORM_PARTS workgroups of 256 lanes, ALWAYS: workgroup b, lane t owns the 16-byte
//                            vectors i = b * 256 + t, + PARTS * 256, ... (one sweep of the grid reads PARTS * 4 KB contiguously), four
//                            loads issued before the first is used.  V = 16 / sizeof(T) elements per vector (4 fp32, 8 bf16).
//   grad_clip_finish_kernel  one workgroup: the partials of every bucket in ascending order in fp64 -- 1024 at a time through LDS as
//                            doubles, added by lane 0 in ONE chain while the next 1024 are being loaded (a round that waited for its
//                            own loads cost more than its additions) --, the norm, the coefficient, the counters: lane 0's plain
//                            read-modify-write of the block.  The chain is what the finish costs, a few ns per partial: it is why
//                            COT_GRAD_NORM_PARTS is no larger than the read needs.
//
// No atomics, and nothing depends on timing: the order of additions is a function of n and the constants alone.
//
// The chain.  All terms are >= 0, so the relative error of a sum is bounded by the LONGEST chain of fp32 additions one square passes
// through, d(n, V) (tests/grad_clip_cases.py: chain_length), times 2^-24:
//     rounds = ceil((n / V) / (PARTS * 256))     a lane's sequential adds, one sum per vector slot (the first add, to 0, is counted)
//     + log2(V)                                  the slots, pairwise
//     + 1                                        the tail element (n % V; first lanes of workgroup 0)
//     + 6                                        the wave's exchange stages (cot_reduce.h: wave_allsum)
//     + 3                                        the four waves' sums, added in order by lane 0
// The finish is fp64 and adds nothing at that scale.
#include <float.h>
#include <math.h>

#include "cot_reduce.h"
#include "cot_host.h"

namespace cot {

static_assert(sizeof(cot_clip_state) == 32, "the clip block is 8 x 32-bit words");

constexpr int GC_BLOCK = 256;  // lanes per workgroup (four waves)
constexpr int GC_AHEAD = 4;    // loads of a lane issued before the first is used
constexpr int GC_FIN_BLOCK = 256, GC_FIN_CHUNK = 1024;  // the finish: partials staged per round, by how many lanes

template <typename T, int V> __device__ __forceinline__ void gc_add_squares(float (&acc)[V], const Vec<T, V>& g) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const float x = (float)g.v[k];
        acc[k] += x * x;
    }
}

template <typename T>
__global__ __launch_bounds__(GC_BLOCK) void grad_sumsq_kernel(const T* __restrict__ grad, int64_t n, float* __restrict__ partials) {
    constexpr int V = 16 / (int)sizeof(T);
    __shared__ float s_wave[GC_BLOCK / 64];
    const int64_t nvec = n / V;
    const int64_t stride = (int64_t)gridDim.x * GC_BLOCK;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    int64_t i = (int64_t)blockIdx.x * GC_BLOCK + threadIdx.x;
    for (; i + (GC_AHEAD - 1) * stride < nvec; i += GC_AHEAD * stride) {
        Vec<T, V> g[GC_AHEAD];
#pragma unroll
        for (int a = 0; a < GC_AHEAD; ++a) g[a] = ldv<T, V>(grad + (i + a * stride) * V);
#pragma unroll
        for (int a = 0; a < GC_AHEAD; ++a) gc_add_squares<T, V>(acc, g[a]);  // in ascending order of address, as the loop below
    }
    for (; i < nvec; i += stride) gc_add_squares<T, V>(acc, ldv<T, V>(grad + i * V));
#pragma unroll
    for (int w = 1; w < V; w <<= 1)  // the slots, pairwise: (0 + 1) + (2 + 3), ...
#pragma unroll
        for (int k = 0; k + w < V; k += 2 * w) acc[k] += acc[k + w];
    float s = acc[0];
    // tail (n % V elements): first lanes of workgroup 0
    const int64_t tail0 = nvec * V;
    if (blockIdx.x == 0 && threadIdx.x < n - tail0) {
        const float x = (float)grad[tail0 + threadIdx.x];
        s += x * x;
    }
    s = wave_allsum(s);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = s_wave[0];
#pragma unroll
        for (int w = 1; w < GC_BLOCK / 64; ++w) t += s_wave[w];
        partials[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(GC_FIN_BLOCK) void grad_clip_finish_kernel(const float* __restrict__ partials, int64_t nparts, float max_norm,
                                                                       cot_clip_state* st) {
    __shared__ double s_part[GC_FIN_CHUNK];
    constexpr int PER = GC_FIN_CHUNK / GC_FIN_BLOCK;
    const int lane = threadIdx.x;
    double sum = 0.0;
    float next[PER];  // the chunk after the one lane 0 is adding: its loads are in flight meanwhile
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int64_t p = (int64_t)k * GC_FIN_BLOCK + lane;
        next[k] = p < nparts ? partials[p] : 0.f;
    }
    for (int64_t base = 0; base < nparts; base += GC_FIN_CHUNK) {
#pragma unroll
        for (int k = 0; k < PER; ++k) s_part[k * GC_FIN_BLOCK + lane] = (double)next[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int64_t p = base + GC_FIN_CHUNK + (int64_t)k * GC_FIN_BLOCK + lane;
            next[k] = p < nparts ? partials[p] : 0.f;
        }
        if (lane == 0) {
            const int cnt = nparts - base < GC_FIN_CHUNK ? (int)(nparts - base) : GC_FIN_CHUNK;
#pragma unroll 16
            for (int j = 0; j < cnt; ++j) sum += s_part[j];  // ONE chain, ascending index (not shared with eval_accumulate_kernel's: no prefetch there)
        }
        __syncthreads();
    }
    if (lane == 0) {
        const bool finite = fabs(sum) <= DBL_MAX;  // (false for NaN)
        const float norm = (float)sqrt(sum);
        float scale = 0.f;
        if (finite) {  // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
            const float c = max_norm / (norm + 1e-6f);
            scale = c < 1.f ? c : 1.f;
        }
        st->scale = scale;
        st->total_norm = norm;
        st->skip = finite ? 0 : 1;
        st->steps += 1;
        st->clipped += (finite && scale < 1.f) ? 1 : 0;
        st->skipped += finite ? 0 : 1;
        st->reserved[0] = 0;
        st->reserved[1] = 0;
    }
}

int grad_sumsq(const void* grad, int64_t n, int grad_dtype, float* partials, hipStream_t s) {
    const dim3 grid(COT_GRAD_NORM_PARTS), block(GC_BLOCK);
    if (grad_dtype == COT_F32)
        COT_LAUNCH(grad_sumsq_kernel<float>, grid, block, 0, s, (const float*)grad, n, partials);
    else if (grad_dtype == COT_BF16)
        COT_LAUNCH(grad_sumsq_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)grad, n, partials);
    else
        return set_error(COT_ERR_UNSUPPORTED, "cot_grad_sumsq: gradient dtype %d (float32 / bfloat16)", grad_dtype);
    return check_launch("grad_sumsq_kernel");
}

int grad_clip_finish(const float* partials, int64_t nparts, float max_norm, void* state, hipStream_t s) {
    COT_LAUNCH(grad_clip_finish_kernel, dim3(1), dim3(GC_FIN_BLOCK), 0, s, partials, nparts, max_norm, (cot_clip_state*)state);
    return check_launch("grad_clip_finish_kernel");
}

}  // namespace cot
