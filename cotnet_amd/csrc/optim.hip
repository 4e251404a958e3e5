// optim.hip -- fused SGD (momentum / nesterov / weight decay) over FLAT parameter buffers, gfx950.
//
// Replaces the reference's per-tensor optimizer step (optim/optim_factory.py:54-56 -> torch.optim.SGD(nesterov=True),
// one or more elementwise launches per parameter tensor) with one launch per flat bucket:
//     g   = grad * grad_scale + wd * p
//     buf = momentum * buf + g
//     p  -= lr * (nesterov ? g + momentum * buf : buf)
// Low-precision training keeps an fp32 master copy: the kernel reads the bf16 gradient bucket, updates master and
// momentum in fp32 and writes the bf16 working copy the convolutions read -- 2+4+4 B read, 4+4+2 B written per
// parameter, HBM-bound, 16-byte accesses per lane.  Same arithmetic (in fp32) as torch.optim.SGD with dampening 0.
#include <type_traits>

#include "cot_common.h"
#include "cot_host.h"

namespace cot {

// Where the rate comes from is the kernel's last template argument.  LR = float: by value, fixed when the launch is enqueued
// (or recorded into a HIP graph).  LR = const float*: one float in device memory, read when the kernel RUNS -- every lane loads
// it once in front of the loop, the tail uses the same value -- so a graph that recorded the launch steps with whatever the
// float holds at each replay.  The kernel only reads it; the caller writes it, ordered on the stream.
__device__ __forceinline__ float sgd_rate(float lr) { return lr; }
__device__ __forceinline__ float sgd_rate(const float* __restrict__ lr_dev) { return *lr_dev; }

// LR = SgdClipped (cot_sgd_step_clip): the rate from either source, behind the clip block that cot_grad_clip_finish left in device
// memory (grad_clip.hip).  Every lane reads the block's `scale` and `skip` once in front of the loop, next to the rate: skip != 0
// ends the kernel before it has written anything; otherwise the gradient's factor becomes the ONE fp32 product gscale * scale, and
// the expression below is the same.  The other two forms have no block: their sgd_gate is the constant `true`.
struct SgdClipped {
    float lr;
    const float* lr_dev;  // NULL: `lr`
    const cot_clip_state* clip;
};
__device__ __forceinline__ float sgd_rate(const SgdClipped& a) { return a.lr_dev ? *a.lr_dev : a.lr; }
__device__ __forceinline__ bool sgd_gate(float, float&) { return true; }
__device__ __forceinline__ bool sgd_gate(const float*, float&) { return true; }
__device__ __forceinline__ bool sgd_gate(const SgdClipped& a, float& gscale) {
    gscale *= a.clip->scale;
    return a.clip->skip == 0;
}

template <typename PT, typename GT, bool HAS_MASTER, int V, typename LR>
__global__ __launch_bounds__(256) void sgd_flat_kernel(PT* __restrict__ param, float* __restrict__ master,
                                                      float* __restrict__ mom, const GT* __restrict__ grad,
                                                      int64_t n, LR lr_arg, float momentum, float wd, float gscale,
                                                      int nesterov) {
    const float lr = sgd_rate(lr_arg);
    if (!sgd_gate(lr_arg, gscale)) return;
    const int64_t nvec = n / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        const Vec<GT, V> gv = ldv<GT, V>(grad + i * V);
        Vec<float, V> mv = ldv<float, V>(mom + i * V);
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
            const float g = (float)gv.v[k] * gscale + wd * pv.v[k];
            const float b = momentum * mv.v[k] + g;
            mv.v[k] = b;
            pv.v[k] -= lr * (nesterov ? g + momentum * b : b);
            out.v[k] = (PT)pv.v[k];
        }
        stv<float, V>(mom + i * V, mv);
        if (HAS_MASTER) stv<float, V>(master + i * V, pv);
        stv<PT, V>(param + i * V, out);
    }
    // tail (n % V elements): first lanes of block 0
    const int64_t tail0 = nvec * V;
    if (blockIdx.x == 0 && threadIdx.x < n - tail0) {
        const int64_t i = tail0 + threadIdx.x;
        float p = HAS_MASTER ? master[i] : (float)param[i];
        const float g = (float)grad[i] * gscale + wd * p;
        const float b = momentum * mom[i] + g;
        mom[i] = b;
        p -= lr * (nesterov ? g + momentum * b : b);
        if (HAS_MASTER) master[i] = p;
        param[i] = (PT)p;
    }
}

// ema = decay * ema + (1 - decay) * src over a flat buffer (reference: utils/model_ema.py:45-53, ModelEmaV2._update, one
// elementwise op per state_dict tensor); src = the fp32 master copy (or the fp32 parameters), ema fp32
template <typename ST, int V>
__global__ __launch_bounds__(256) void ema_flat_kernel(float* __restrict__ ema, const ST* __restrict__ src, int64_t n,
                                                      float decay) {
    const int64_t nvec = n / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        Vec<float, V> e = ldv<float, V>(ema + i * V);
        const Vec<ST, V> sv = ldv<ST, V>(src + i * V);
#pragma unroll
        for (int k = 0; k < V; ++k) e.v[k] = decay * e.v[k] + (1.f - decay) * (float)sv.v[k];
        stv<float, V>(ema + i * V, e);
    }
    const int64_t tail0 = nvec * V;
    if (blockIdx.x == 0 && threadIdx.x < n - tail0) {
        const int64_t i = tail0 + threadIdx.x;
        ema[i] = decay * ema[i] + (1.f - decay) * (float)src[i];
    }
}

int ema_flat(void* ema, const void* src, int64_t n, float decay, int src_dtype, hipStream_t s) {
    constexpr int V = 4;
    int64_t blocks = ceil_div64(n / V > 0 ? n / V : 1, 256);
    if (blocks > 2048) blocks = 2048;
    if (src_dtype == COT_F32)
        COT_LAUNCH((ema_flat_kernel<float, V>), dim3((unsigned)blocks), dim3(256), 0, s, (float*)ema, (const float*)src, n,
                   decay);
    else if (src_dtype == COT_BF16)
        COT_LAUNCH((ema_flat_kernel<bf16_t, V>), dim3((unsigned)blocks), dim3(256), 0, s, (float*)ema, (const bf16_t*)src, n,
                   decay);
    else
        return set_error(COT_ERR_UNSUPPORTED, "ema: source dtype %d not supported (float32 / bfloat16)", src_dtype);
    return check_launch("ema_flat_kernel");
}

template <typename PT, typename GT, bool HAS_MASTER, typename LR>
static int launch_sgd(void* param, void* master, void* mom, const void* grad, int64_t n, LR lr, float momentum,
                      float wd, float gscale, int nesterov, hipStream_t s) {
    constexpr int V = 4;  // 16 B of fp32 state per lane
    int64_t blocks = ceil_div64(n / V > 0 ? n / V : 1, 256);
    if (blocks > 2048) blocks = 2048;  // grid-stride: 8 blocks per CU
    COT_LAUNCH((sgd_flat_kernel<PT, GT, HAS_MASTER, V, LR>), dim3((unsigned)blocks), dim3(256), 0, s, (PT*)param,
               (float*)master, (float*)mom, (const GT*)grad, n, lr, momentum, wd, gscale, nesterov);
    return check_launch(std::is_same<LR, SgdClipped>::value ? "sgd_flat_kernel<clip>"
                        : std::is_pointer<LR>::value        ? "sgd_flat_kernel<lr_dev>"
                                                            : "sgd_flat_kernel");
}

template <typename LR>  // float (cot_sgd_step), const float* (cot_sgd_step_lr) or SgdClipped (cot_sgd_step_clip)
static int sgd_dispatch(void* param, void* master, void* mom, const void* grad, int64_t n, LR lr, float momentum, float wd,
                        float gscale, int nesterov, int param_dtype, int grad_dtype, hipStream_t s) {
    if (param_dtype == COT_BF16 && grad_dtype == COT_BF16 && master)
        return launch_sgd<bf16_t, bf16_t, true>(param, master, mom, grad, n, lr, momentum, wd, gscale, nesterov, s);
    if (param_dtype == COT_BF16 && grad_dtype == COT_F32 && master)
        return launch_sgd<bf16_t, float, true>(param, master, mom, grad, n, lr, momentum, wd, gscale, nesterov, s);
    if (param_dtype == COT_F32 && grad_dtype == COT_F32 && !master)
        return launch_sgd<float, float, false>(param, master, mom, grad, n, lr, momentum, wd, gscale, nesterov, s);
    if (param_dtype == COT_F32 && grad_dtype == COT_BF16 && !master)
        return launch_sgd<float, bf16_t, false>(param, master, mom, grad, n, lr, momentum, wd, gscale, nesterov, s);
    return set_error(COT_ERR_UNSUPPORTED, "sgd: param dtype %d / grad dtype %d / master %s not supported", param_dtype,
                     grad_dtype, master ? "given" : "NULL");
}

int sgd_flat(void* param, void* master, void* mom, const void* grad, int64_t n, float lr, float momentum, float wd,
             float gscale, int nesterov, int param_dtype, int grad_dtype, hipStream_t s) {
    return sgd_dispatch<float>(param, master, mom, grad, n, lr, momentum, wd, gscale, nesterov, param_dtype, grad_dtype, s);
}

int sgd_flat_lr(void* param, void* master, void* mom, const void* grad, int64_t n, const float* lr_dev, float momentum,
                float wd, float gscale, int nesterov, int param_dtype, int grad_dtype, hipStream_t s) {
    return sgd_dispatch<const float*>(param, master, mom, grad, n, lr_dev, momentum, wd, gscale, nesterov, param_dtype,
                                      grad_dtype, s);
}

int sgd_flat_clip(void* param, void* master, void* mom, const void* grad, int64_t n, float lr, const float* lr_dev,
                  const cot_clip_state* clip, float momentum, float wd, float gscale, int nesterov, int param_dtype, int grad_dtype,
                  hipStream_t s) {
    return sgd_dispatch<SgdClipped>(param, master, mom, grad, n, SgdClipped{lr, lr_dev, clip}, momentum, wd, gscale, nesterov,
                                    param_dtype, grad_dtype, s);
}

}  // namespace cot
