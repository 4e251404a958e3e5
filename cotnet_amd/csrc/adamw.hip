// adamw.hip -- fused Adam / AdamW over FLAT parameter buffers, gfx950: cot_adam_tick and cot_adamw_step (include/cotnet_amd.h).
//
// Replaces the reference's per-tensor steps (optim/optim_factory.py:60-65: `adam` -> torch.optim.Adam, `adamw` -> optim/adamw.py:72-115,
// several elementwise launches per parameter tensor and a step count per parameter on the host) with one launch per flat bucket behind
// ONE step count in device memory (cot_adam_state), so that a HIP graph that recorded the step serves every step.
//
//   adam_tick_kernel   one workgroup, once per step: lane 0 adds 1 to `step` and forms both bias corrections from the INTEGER step in
//                      double, on the betas as the doubles they were given as -- two pow per step, none per element (a per-element
//                      powf would make the streaming kernel VALU-bound).  From the integer, not by multiplying the last value by beta: the block is then a pure function of `step`, and
//                      a block set to step = t - 1 and ticked once equals one ticked t times.  A clip block that says skip: only the
//                      refused count moves.
//   adamw_flat_kernel  HBM-bound, the shape of sgd_flat_kernel (optim.hip): 256 lanes, 16 bytes of fp32 state per lane and access, at
//                      most 2048 workgroups with a grid-stride loop, the tail (n % 4 elements) on the first lanes of workgroup 0.  With
//                      bf16 weights and gradients and an fp32 master: 2 + 4 + 4 + 4 B read, 4 + 4 + 4 + 2 B written per parameter.
//                      Every lane reads the rate, the block's corrections and, where given, the clip block's scale and skip ONCE in
//                      front of the loop; skip != 0 ends the kernel before it has written anything.
//
// THE ORDER OF OPERATIONS (tests/adamw_cases.py derives its bounds from it).  All fp32; each line one rounding per operator unless
// hipcc contracts a multiply and the add that consumes it into one FMA (one rounding instead of two: never a larger error).
//   once per lane:   gs    = gscale                       (no clip block)     or   gscale * clip->scale   (one product)
//                    decay = 1 - lr * wd                  (decoupled only)
//                    a     = lr / bc1                     (IEEE division)
//   by value:        beta1, beta2 = (float) of the doubles given;  omb1 = (float)(1 - beta1), omb2 = (float)(1 - beta2), the subtraction
//                    in double on the host -- torch hands its kernels the same fp32 roundings of the doubles `beta` and `1 - beta`;
//                    1.f - (float)0.999 would be 1.3e-5 off (float)(1 - 0.999)
//   per element:     g = (float)grad * gs
//                    g = g + wd * p                       (decoupled == 0: torch.optim.Adam's L2 form)
//                    p = p * decay                        (decoupled != 0: the reference decays first, adamw.py:72)
//                    m = m * beta1 + omb1 * g
//                    v = v * beta2 + (omb2 * g) * g
//                    d = sqrtf(v) / sqrt_bc2 + eps        (IEEE square root and division)
//                    p = p - a * (m / d)                  (IEEE division)
//                    param = (PT)p                        (round to nearest even)
// No atomics, nothing depends on timing, every element is owned by one lane: equal data give equal bits, eager or replayed.  No
// amsgrad (the reference's factory never sets it).
#include <math.h>

#include "cot_common.h"
#include "cot_host.h"

namespace cot {

static_assert(sizeof(cot_adam_state) == 32, "the Adam block is 8 x 32-bit words");

__global__ __launch_bounds__(64) void adam_tick_kernel(cot_adam_state* st, const cot_clip_state* clip, double beta1, double beta2) {
    if (threadIdx.x != 0) return;
    if (clip && clip->skip != 0) {  // the step is skipped: it never reaches the optimizer, as behind the reference's scaler
        st->refused += 1;
        return;
    }
    const int step = st->step + 1;
    st->step = step;
    st->bc1 = (float)(1.0 - pow(beta1, (double)step));
    st->sqrt_bc2 = (float)sqrt(1.0 - pow(beta2, (double)step));
}

struct AdamArgs {
    float lr;
    const float* lr_dev;  // NULL: `lr`
    const cot_adam_state* st;
    const cot_clip_state* clip;  // NULL: no block
    float beta1, beta2, omb1, omb2;  // (float)beta and (float)(1 - beta), the subtraction in double on the host
    float eps, wd, gscale;
    int decoupled;
};

// what a lane holds across its loop
struct AdamConsts {
    float gs, decay, a, beta1, beta2, omb1, omb2, sqrt_bc2, eps, wd;
    bool decoupled;
};

__device__ __forceinline__ void adam_element(float& p, float& m, float& v, float graw, const AdamConsts& c) {
    float g = graw * c.gs;
    if (c.decoupled)
        p = p * c.decay;
    else
        g = g + c.wd * p;
    m = m * c.beta1 + c.omb1 * g;
    v = v * c.beta2 + (c.omb2 * g) * g;
    const float d = sqrtf(v) / c.sqrt_bc2 + c.eps;
    p = p - c.a * (m / d);
}

template <typename PT, typename GT, bool HAS_MASTER, int V>
__global__ __launch_bounds__(256) void adamw_flat_kernel(PT* __restrict__ param, float* __restrict__ master, float* __restrict__ exp_avg,
                                                        float* __restrict__ exp_avg_sq, const GT* __restrict__ grad, int64_t n,
                                                        AdamArgs args) {
    const float lr = args.lr_dev ? *args.lr_dev : args.lr;
    AdamConsts c;
    c.gs = args.gscale;
    if (args.clip) {
        c.gs *= args.clip->scale;
        if (args.clip->skip != 0) return;
    }
    c.decoupled = args.decoupled != 0;
    c.decay = 1.f - lr * args.wd;
    c.a = lr / args.st->bc1;
    c.beta1 = args.beta1;
    c.beta2 = args.beta2;
    c.omb1 = args.omb1;
    c.omb2 = args.omb2;
    c.sqrt_bc2 = args.st->sqrt_bc2;
    c.eps = args.eps;
    c.wd = args.wd;
    const int64_t nvec = n / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        const Vec<GT, V> gv = ldv<GT, V>(grad + i * V);
        Vec<float, V> mv = ldv<float, V>(exp_avg + i * V);
        Vec<float, V> vv = ldv<float, V>(exp_avg_sq + i * V);
        Vec<float, V> pv;
        if (HAS_MASTER) {
            pv = ldv<float, V>(master + i * V);
        } else {
            const Vec<PT, V> t = ldv<PT, V>(param + i * V);
#pragma unroll
            for (int k = 0; k < V; ++k) pv.v[k] = (float)t.v[k];
        }
        Vec<PT, V> out;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            adam_element(pv.v[k], mv.v[k], vv.v[k], (float)gv.v[k], c);
            out.v[k] = (PT)pv.v[k];
        }
        stv<float, V>(exp_avg + i * V, mv);
        stv<float, V>(exp_avg_sq + i * V, vv);
        if (HAS_MASTER) stv<float, V>(master + i * V, pv);
        stv<PT, V>(param + i * V, out);
    }
    // tail (n % V elements): first lanes of block 0
    const int64_t tail0 = nvec * V;
    if (blockIdx.x == 0 && threadIdx.x < n - tail0) {
        const int64_t i = tail0 + threadIdx.x;
        float p = HAS_MASTER ? master[i] : (float)param[i];
        float m = exp_avg[i], v = exp_avg_sq[i];
        adam_element(p, m, v, (float)grad[i], c);
        exp_avg[i] = m;
        exp_avg_sq[i] = v;
        if (HAS_MASTER) master[i] = p;
        param[i] = (PT)p;
    }
}

int adam_tick(void* adam_state, const void* clip_state, double beta1, double beta2, hipStream_t s) {
    COT_LAUNCH(adam_tick_kernel, dim3(1), dim3(64), 0, s, (cot_adam_state*)adam_state, (const cot_clip_state*)clip_state, beta1, beta2);
    return check_launch("adam_tick_kernel");
}

template <typename PT, typename GT, bool HAS_MASTER>
static int launch_adamw(void* param, void* master, void* exp_avg, void* exp_avg_sq, const void* grad, int64_t n, const AdamArgs& args,
                        hipStream_t s) {
    constexpr int V = 4;  // 16 B of fp32 state per lane
    int64_t blocks = ceil_div64(n / V > 0 ? n / V : 1, 256);
    if (blocks > 2048) blocks = 2048;  // grid-stride: 8 blocks per CU
    COT_LAUNCH((adamw_flat_kernel<PT, GT, HAS_MASTER, V>), dim3((unsigned)blocks), dim3(256), 0, s, (PT*)param, (float*)master,
               (float*)exp_avg, (float*)exp_avg_sq, (const GT*)grad, n, args);
    return check_launch("adamw_flat_kernel");
}

int adamw_flat(void* param, void* master, void* exp_avg, void* exp_avg_sq, const void* grad, int64_t n, float lr, const float* lr_dev,
               const cot_adam_state* st, const cot_clip_state* clip, double beta1, double beta2, float eps, float wd, float gscale,
               int decoupled, int param_dtype, int grad_dtype, hipStream_t s) {
    const AdamArgs args{lr, lr_dev, st, clip, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, wd, gscale, decoupled};
    // the four (param, grad) pairs and the master rule of sgd_dispatch (optim.hip)
    if (param_dtype == COT_BF16 && grad_dtype == COT_BF16 && master)
        return launch_adamw<bf16_t, bf16_t, true>(param, master, exp_avg, exp_avg_sq, grad, n, args, s);
    if (param_dtype == COT_BF16 && grad_dtype == COT_F32 && master)
        return launch_adamw<bf16_t, float, true>(param, master, exp_avg, exp_avg_sq, grad, n, args, s);
    if (param_dtype == COT_F32 && grad_dtype == COT_F32 && !master)
        return launch_adamw<float, float, false>(param, master, exp_avg, exp_avg_sq, grad, n, args, s);
    if (param_dtype == COT_F32 && grad_dtype == COT_BF16 && !master)
        return launch_adamw<float, bf16_t, false>(param, master, exp_avg, exp_avg_sq, grad, n, args, s);
    return set_error(COT_ERR_UNSUPPORTED, "adamw: param dtype %d / grad dtype %d / master %s not supported", param_dtype, grad_dtype,
                     master ? "given" : "NULL");
}

}  // namespace cot
