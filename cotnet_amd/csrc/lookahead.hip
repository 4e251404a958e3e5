// lookahead.hip -- Lookahead's slow weights over FLAT parameter buffers, gfx950: cot_lookahead_tick and cot_lookahead_step
// (include/cotnet_amd.h).
//
// Replaces the reference's wrapper (optim/lookahead.py:29-52: a step count per group on the host, and per parameter tensor a subtraction,
// an add_ and a copy_ every k-th step) with one launch per flat bucket behind ONE decision in device memory (cot_lookahead_state), so
// that a HIP graph that recorded the step serves sync and non-sync steps alike.
//
//   lookahead_tick_kernel   one workgroup, once per step (or once per sync_lookahead): lane 0 counts the step and writes what the bucket
//                           kernels are to do -- 0 nothing, 1 adopt (the slow weights are created as a copy of the fast ones, the
//                           reference's lazy buffer, lookahead.py:34-36), 2 interpolate.  A clip block that says skip: only the refused
//                           count moves, and the action is written as 0 so that the last step's decision is not carried out again.
//   lookahead_flat_kernel   HBM-bound, the shape of sgd_flat_kernel (optim.hip): 256 lanes, 16 bytes of fp32 per lane and access, at most
//                           2048 workgroups with a grid-stride loop, the tail (n % 4 elements) on the first lanes of workgroup 0.  Every
//                           lane reads the action ONCE in front of the loop; 0 ends the kernel before it has written anything.  A sync
//                           with bf16 weights and an fp32 master: 4 + 4 B read, 4 + 4 + 2 B written per parameter, once in k steps.
//
// THE ORDER OF OPERATIONS (tests/lookahead_cases.py derives its bound from it).  `fast` is the master, or the fp32 parameters where there
// is none.  All fp32; one rounding per operator unless hipcc contracts the multiply and the add into one FMA (one rounding instead of
// two: never a larger error; with alpha = 0.5 the product is exact and both forms give the same bits).
//   by value:      alpha = (float) of the double given
//   action 1:      slow = fast                          (nothing else is written)
//   action 2:      d = fast - slow
//                  s = slow + alpha * d                 (lookahead.py:38)
//                  slow = s;  fast = s                  (lookahead.py:39)
//                  param = (PT)s                        (round to nearest even; where there is a master)
// No atomics, nothing depends on timing, every element is owned by one lane, the block is only read: equal data give equal bits, eager
// or replayed.
#include "cot_common.h"
#include "cot_host.h"

namespace cot {

static_assert(sizeof(cot_lookahead_state) == 32, "the Lookahead block is 8 x 32-bit words");

__global__ __launch_bounds__(64) void lookahead_tick_kernel(cot_lookahead_state* st, const cot_clip_state* clip, int k, int force) {
    if (threadIdx.x != 0) return;
    if (clip && clip->skip != 0) {  // the step is skipped: it never reaches the optimizer, as behind the reference's scaler
        st->refused += 1;
        st->action = 0;
        return;
    }
    int action;
    if (force) {  // sync_lookahead (lookahead.py:41-43): the count stays
        action = st->born ? 2 : 1;
    } else {
        const int step = st->step + 1;
        st->step = step;
        action = (step % k != 0) ? 0 : (st->born ? 2 : 1);
    }
    st->action = action;
    if (action != 0) {
        st->born = 1;
        st->syncs += 1;
    }
}

__device__ __forceinline__ float lookahead_element(float fast, float slow, float alpha) {
    const float d = fast - slow;
    return slow + alpha * d;
}

template <typename PT, bool HAS_MASTER, int V>
__global__ __launch_bounds__(256) void lookahead_flat_kernel(PT* __restrict__ param, float* __restrict__ master, float* __restrict__ slow,
                                                            int64_t n, float alpha, const cot_lookahead_state* __restrict__ st) {
    const int action = st->action;
    if (action == 0) return;
    float* fast = HAS_MASTER ? master : reinterpret_cast<float*>(param);  // (without a master PT is float)
    const int64_t nvec = n / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        const Vec<float, V> fv = ldv<float, V>(fast + i * V);
        if (action == 1) {
            stv<float, V>(slow + i * V, fv);
            continue;
        }
        const Vec<float, V> sv = ldv<float, V>(slow + i * V);
        Vec<float, V> out;
        Vec<PT, V> work;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            out.v[k] = lookahead_element(fv.v[k], sv.v[k], alpha);
            work.v[k] = (PT)out.v[k];
        }
        stv<float, V>(slow + i * V, out);
        stv<float, V>(fast + i * V, out);
        if (HAS_MASTER) stv<PT, V>(param + i * V, work);
    }
    // tail (n % V elements): first lanes of block 0
    const int64_t tail0 = nvec * V;
    if (blockIdx.x == 0 && threadIdx.x < n - tail0) {
        const int64_t i = tail0 + threadIdx.x;
        if (action == 1) {
            slow[i] = fast[i];
        } else {
            const float s = lookahead_element(fast[i], slow[i], alpha);
            slow[i] = s;
            fast[i] = s;
            if (HAS_MASTER) param[i] = (PT)s;
        }
    }
}

int lookahead_tick(void* state, const void* clip_state, int k, int force, hipStream_t s) {
    COT_LAUNCH(lookahead_tick_kernel, dim3(1), dim3(64), 0, s, (cot_lookahead_state*)state, (const cot_clip_state*)clip_state, k, force);
    return check_launch("lookahead_tick_kernel");
}

template <typename PT, bool HAS_MASTER>
static int launch_lookahead(void* param, void* master, void* slow, int64_t n, float alpha, const cot_lookahead_state* st, hipStream_t s) {
    constexpr int V = 4;  // 16 B of fp32 per lane
    int64_t blocks = ceil_div64(n / V > 0 ? n / V : 1, 256);
    if (blocks > 2048) blocks = 2048;  // grid-stride: 8 blocks per CU
    COT_LAUNCH((lookahead_flat_kernel<PT, HAS_MASTER, V>), dim3((unsigned)blocks), dim3(256), 0, s, (PT*)param, (float*)master, (float*)slow,
               n, alpha, st);
    return check_launch("lookahead_flat_kernel");
}

int lookahead_flat(void* param, void* master, void* slow, int64_t n, double alpha, const cot_lookahead_state* st, int param_dtype,
                   hipStream_t s) {
    // the master rule of sgd_dispatch (optim.hip)
    if (param_dtype == COT_BF16 && master) return launch_lookahead<bf16_t, true>(param, master, slow, n, (float)alpha, st, s);
    if (param_dtype == COT_F32 && !master) return launch_lookahead<float, false>(param, master, slow, n, (float)alpha, st, s);
    return set_error(COT_ERR_UNSUPPORTED, "lookahead: param dtype %d / master %s not supported", param_dtype, master ? "given" : "NULL");
}

}  // namespace cot
