// agc.hip -- adaptive gradient clipping (AGC, the NFNet rule) over a flat bucket, unit by unit, on the device, gfx950.
//
// Reference: train.py:269-274 (`loss.backward(); dispatch_clip_grad(..., mode='agc'); optimizer.step()`), utils/clip_grad.py:3-24
// (adaptive_clip_grad: per parameter tensor two unit-wise norms, a clamp, a multiply, a divide and a torch.where that rewrites every
// gradient -- about six launches per tensor).  Here the gradients and the fp32 weights of a bucket lie flat, a table in device memory
// names each unit as (start, len), and ONE launch per bucket reads both operands once and writes only the units that really clip.
//
//   agc_clip_kernel   workgroups of 256 lanes = four waves; ONE WAVE PER UNIT: wave w of the grid takes units w, w + W, ...
//                     (W = 4 * gridDim.x).  A unit of any length is a longer loop of the same wave.  Per operand (V elements per
//                     16 bytes: 4 for fp32, 8 for bf16; the two operands' 16-byte phases differ, each is computed from `start`):
//                       head   (-start) mod V elements up to the first 16-byte boundary (at most len), scalar loads, lane l takes
//                              element l
//                       body   nvec = (len - head) / V aligned 16-byte vectors; lane l takes vectors l + 64 * j, j = 0, 1, ...;
//                              j mod 4 selects one of AGC_AHEAD = 4 accumulator sets (four loads issued before the first is used),
//                              each set one fp32 sum per vector slot, added in ascending j
//                       tail   the remaining < V elements, scalar loads, lane l takes element l
//                     then, per lane: the four sets pairwise per slot ((0 + 1) + (2 + 3)), the V slots pairwise, + the head element's
//                     square, + the tail element's square; then the wave's 64 lanes by wave_allsum's six exchange stages
//                     (cot_reduce.h), which leaves the same bits in every lane.  Lane 0 writes coef[unit].  A unit with coef < 1
//                     re-reads its gradient (L2-resident: the wave read it a moment ago) in the same head / body / tail split and
//                     stores (T)((float)g * coef); a unit with coef == 1 or NaN is not written at all.
//
// No atomics, and nothing depends on timing: which lane adds which square, and in what order, is a function of (start, len, dtype)
// alone -- not of the grid, of the unit's index or of its neighbours.
//
// The chain.  All terms are >= 0, so the relative error of a sum is bounded by the LONGEST chain of fp32 additions one square passes
// through, d(start, len, V) (tests/agc_cases.py: agc_chain_length), times 2^-24.  With head = min(len, (-start) mod V) and
// nvec = (len - head) / V:
//     ceil(nvec / (64 * 4))     a lane's sequential adds into one accumulator (the first add, to 0, is counted)
//     + 2                       the four accumulator sets, pairwise
//     + log2(V)                 the slots, pairwise
//     + 2                       the head element, the tail element
//     + 6                       the wave's exchange stages
// A row of 2048 elements: 1 + 2 + 3 + 2 + 6 = 14 in bf16, 2 + 2 + 2 + 2 + 6 = 14 in fp32.
#include <float.h>
#include <math.h>

#include "cot_reduce.h"
#include "cot_host.h"

namespace cot {

constexpr int AGC_BLOCK = 256;  // lanes per workgroup: four waves, four units at a time
constexpr int AGC_AHEAD = 4;    // accumulator sets = loads of a lane issued before the first is used

// sum of squares of x[0..len) where x = base + start; every lane of the wave returns the same bits
template <typename T> __device__ __forceinline__ float agc_unit_sumsq(const T* __restrict__ base, int64_t start, int64_t len, int lane) {
    constexpr int V = 16 / (int)sizeof(T);
    const T* x = base + start;
    const int64_t to_boundary = (V - (start % V)) % V;
    const int64_t head = to_boundary < len ? to_boundary : len;
    const int64_t nvec = (len - head) / V;
    const int64_t tail0 = head + nvec * V;
    const T* body = x + head;  // 16-byte aligned (the base is)
    float acc[AGC_AHEAD][V];
#pragma unroll
    for (int a = 0; a < AGC_AHEAD; ++a)
#pragma unroll
        for (int k = 0; k < V; ++k) acc[a][k] = 0.f;
    for (int64_t i = lane; i < nvec; i += 64 * AGC_AHEAD) {
        Vec<T, V> v[AGC_AHEAD];
#pragma unroll
        for (int a = 0; a < AGC_AHEAD; ++a) {
            const int64_t j = i + 64 * a;
            if (j < nvec) {
                v[a] = ldv<T, V>(body + j * V);
            } else {  // a zero adds nothing and changes no bit of a sum that is >= 0
#pragma unroll
                for (int k = 0; k < V; ++k) v[a].v[k] = (T)0.f;
            }
        }
#pragma unroll
        for (int a = 0; a < AGC_AHEAD; ++a)
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float f = (float)v[a].v[k];
                acc[a][k] += f * f;
            }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) acc[0][k] = (acc[0][k] + acc[1][k]) + (acc[2][k] + acc[3][k]);
#pragma unroll
    for (int w = 1; w < V; w <<= 1)  // the slots, pairwise: (0 + 1) + (2 + 3), ...
#pragma unroll
        for (int k = 0; k + w < V; k += 2 * w) acc[0][k] += acc[0][k + w];
    float s = acc[0][0];
    if (lane < head) {
        const float f = (float)x[lane];
        s += f * f;
    }
    if (lane < len - tail0) {
        const float f = (float)x[tail0 + lane];
        s += f * f;
    }
    return wave_allsum(s);
}

// g[i] = (T)((float)g[i] * coef) over the unit, in the split of agc_unit_sumsq: every element is read and written by one lane
template <typename T> __device__ __forceinline__ void agc_unit_scale(T* __restrict__ base, int64_t start, int64_t len, float coef, int lane) {
    constexpr int V = 16 / (int)sizeof(T);
    T* x = base + start;
    const int64_t to_boundary = (V - (start % V)) % V;
    const int64_t head = to_boundary < len ? to_boundary : len;
    const int64_t nvec = (len - head) / V;
    const int64_t tail0 = head + nvec * V;
    T* body = x + head;
    for (int64_t j = lane; j < nvec; j += 64) {
        Vec<T, V> v = ldv<T, V>(body + j * V);
#pragma unroll
        for (int k = 0; k < V; ++k) v.v[k] = (T)((float)v.v[k] * coef);
        stv<T, V>(body + j * V, v);
    }
    if (lane < head) x[lane] = (T)((float)x[lane] * coef);
    if (lane < len - tail0) x[tail0 + lane] = (T)((float)x[tail0 + lane] * coef);
}

template <typename T>
__global__ __launch_bounds__(AGC_BLOCK) void agc_clip_kernel(T* __restrict__ grad, const float* __restrict__ weight,
                                                            const int64_t* __restrict__ units, int64_t nunits, float clip_factor, float eps,
                                                            float* __restrict__ coef) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (the same in the whole wave: the table is read once per wave)
    const int64_t nwaves = (int64_t)gridDim.x * (AGC_BLOCK / 64);
    for (int64_t u = (int64_t)blockIdx.x * (AGC_BLOCK / 64) + wave; u < nunits; u += nwaves) {
        const int64_t start = units[2 * u], len = units[2 * u + 1];
        const float sw = agc_unit_sumsq<float>(weight, start, len, lane);
        const float sg = agc_unit_sumsq<T>(grad, start, len, lane);
        float c;
        if (sw <= FLT_MAX && sg <= FLT_MAX) {  // (false for inf and NaN)
            const float max_norm = fmaxf(sqrtf(sw), eps) * clip_factor;
            const float gn = sqrtf(sg);
            c = gn < max_norm ? 1.f : max_norm / fmaxf(gn, 1e-6f);  // utils/clip_grad.py:20-23
        } else {
            c = NAN;  // the marker: an inf, a NaN or squares that overflow fp32 -- the unit's gradient stays as it is
        }
        if (lane == 0) coef[u] = c;
        if (c < 1.f) agc_unit_scale<T>(grad, start, len, c, lane);  // (wave-uniform: every lane holds the same bits)
    }
}

int agc_clip(void* grad, const float* weight, const int64_t* units, int64_t nunits, float clip_factor, float eps, float* coef, int grad_dtype,
             hipStream_t s) {
    const int64_t want = ceil_div64(nunits, AGC_BLOCK / 64);
    const dim3 grid((unsigned)(want < COT_AGC_MAX_GROUPS ? want : COT_AGC_MAX_GROUPS)), block(AGC_BLOCK);
    if (grad_dtype == COT_F32)
        COT_LAUNCH(agc_clip_kernel<float>, grid, block, 0, s, (float*)grad, weight, units, nunits, clip_factor, eps, coef);
    else if (grad_dtype == COT_BF16)
        COT_LAUNCH(agc_clip_kernel<bf16_t>, grid, block, 0, s, (bf16_t*)grad, weight, units, nunits, clip_factor, eps, coef);
    else
        return set_error(COT_ERR_UNSUPPORTED, "cot_agc_clip: gradient dtype %d (float32 / bfloat16)", grad_dtype);
    return check_launch("agc_clip_kernel");
}

}  // namespace cot
