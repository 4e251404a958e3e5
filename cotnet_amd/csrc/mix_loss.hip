// mix_loss.hip -- the per-step arithmetic of the reference's training recipe that is neither the model nor the optimizer, gfx950:
// batch-mode mixup / CutMix folded into the input normalisation, and the soft-target cross entropy against mixed, smoothed targets.
//
// Reference: datasets/mixup.py (FastCollateMixup(mode='batch'), :282-299, runs in the host loader's collate; mixup_target, :22-27, builds
// two dense [N, K] one-hot tensors) and loss/cross_entropy.py:29-36 (SoftTargetCrossEntropy = sum(-target * log_softmax(x))).mean()).
//
// What changes from batch to batch -- mixup or CutMix, lambda, the box -- is NOT a kernel argument: every kernel here reads one 32-byte
// parameter block in device memory (cot_mix_params, include/cotnet_amd.h) when it RUNS, as cot_sgd_step_lr reads its rate, so a HIP
// graph that recorded these launches follows the values the block holds at each replay.  The kernels only read the block.
// The reference's per-sample modes ('elem', 'pair': _mix_elem_collate / _mix_pair_collate, :229-280) are the same kernels reading a
// TABLE: a header `mode 3, R` followed by R records of the block's layout, record n for sample n and its partner N-1-n.  Header or
// table is device data too, so the branch is taken inside the kernels (uniform over the grid), not by choosing a kernel on the host;
// a record is 32 bytes that the lanes of a wave almost always share (one plane is H*W/16 consecutive vectors), served by the cache.
//
//   cot_mix_normalize   = cot_input_normalize on  u = mix(x[i], x[N-1-i]):  1 + 1 B read (1 B in mode 0) + sizeof(T) B written per
//                         element, HBM-bound, 16 pixels per lane (two 16-byte loads, 16-byte stores); the partner is read from the
//                         unmodified uint8 input, which is why no clone of the batch is needed.
//   cot_soft_target_ce_*: latency-bound (N x K logits, 160 KB at the recipe's 80 x 1000 bf16): one wave per row, the row is walked three
//                         times out of the cache (max, sum of exponentials, -sum t * logp), in fp64 from the maximum on; the target is
//                         formed per element from the two labels -- labels are only COMPARED with the column index, never used as
//                         an address.  The mean over rows is a second one-wave launch that adds the row losses in a fixed order:
//                         no atomics, so a replayed step equals the eager one bit for bit.
#include <math.h>

#include "input_norm.h"
#include "cot_reduce.h"
#include "cot_host.h"

namespace cot {

struct MixParams {  // = cot_mix_params
    int mode;       // 0 none, 1 mixup, 2 CutMix; in the header also 3: a table of yl records, one per sample, follows
    float lam, one_minus_lam;
    int yl, yh, xl, xh, reserved;
};
constexpr int MIX_TABLE = 3;
static_assert(sizeof(MixParams) == 32 && sizeof(MixParams) == sizeof(cot_mix_params), "the parameter block is 8 x 32-bit words");

// numpy's `a.astype(float32) * lam + b.astype(float32) * (1 - lam)`, np.rint, .astype(uint8) (mixup.py:296-298): the two products are
// rounded separately, then added; round half to even
__device__ __forceinline__ uint8_t mix_pixel(uint8_t a, uint8_t b, float lam, float oml) {
#pragma clang fp contract(off)
    const float pa = (float)a * lam;
    const float pb = (float)b * oml;
    return (uint8_t)(int)rintf(pa + pb);
}

// the record sample n is mixed by.  Header modes 0-2: the header itself, for every sample.  Table mode: record n of the R that follow the
// header; a sample past the table is not mixed (mode 0, lam 1).  n < N always, so no word beyond 8 * (1 + min(R, N)) is read
template <bool TABLE>
__device__ __forceinline__ MixParams record_of(const MixParams* __restrict__ pb, const MixParams& head, int n) {
    if (!TABLE) return head;
    MixParams r = {0, 1.f, 0.f, 0, 0, 0, 0, 0};
    if (n < head.yl) r = pb[1 + n];  // (head.yl = R)
    return r;
}

template <typename T, bool TABLE>
__device__ __forceinline__ void mix_normalize_body(const uint8_t* __restrict__ x, T* __restrict__ y, const float* __restrict__ mean,
                                                   const float* __restrict__ stdv, const MixParams* __restrict__ pb,
                                                   const MixParams& head, int N, int C, int H, int W) {
    const int HW = H * W;
    const int64_t planes = (int64_t)N * C;
    if (HW % 16 == 0) {
        const int vpp = HW / 16;
        const int64_t nvec = planes * vpp;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t plane = i / vpp;
            const int v = (int)(i - plane * vpp);
            const int n = (int)(plane / C), c = (int)(plane - (int64_t)n * C);
            const float m = mean[c], s = stdv[c];
            const MixParams r = record_of<TABLE>(pb, head, n);
            Vec<uint8_t, 16> a = ldv<uint8_t, 16>(x + i * 16);
            if (r.mode == 1 || r.mode == 2) {  // (any other value: as mode 0)
                const int64_t j = ((int64_t)(N - 1 - n) * C + c) * vpp + v;  // the same 16 pixels of sample N-1-n
                const Vec<uint8_t, 16> b = ldv<uint8_t, 16>(x + j * 16);
                if (r.mode == 1) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) a.v[k] = mix_pixel(a.v[k], b.v[k], r.lam, r.one_minus_lam);
                } else {  // a box edge may fall inside the vector, and the vector may run over the end of an image row
                    int yy = (v * 16) / W, xx = v * 16 - yy * W;
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        if (yy >= r.yl && yy < r.yh && xx >= r.xl && xx < r.xh) a.v[k] = b.v[k];
                        if (++xx == W) { xx = 0; ++yy; }
                    }
                }
            }
            constexpr int OV = 16 / sizeof(T);  // elements per 16-byte store
#pragma unroll
            for (int q = 0; q < 16 / OV; ++q) {
                Vec<T, OV> o;
#pragma unroll
                for (int k = 0; k < OV; ++k) o.v[k] = norm_one<T>(a.v[q * OV + k], m, s);
                stv<T, OV>(y + i * 16 + q * OV, o);
            }
        }
    } else {  // odd image sizes: element-wise
        const int64_t total = planes * HW;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t plane = i / HW;
            const int p = (int)(i - plane * HW);
            const int n = (int)(plane / C), c = (int)(plane - (int64_t)n * C);
            const MixParams r = record_of<TABLE>(pb, head, n);
            uint8_t u = x[i];
            if (r.mode == 1 || r.mode == 2) {
                const uint8_t b = x[((int64_t)(N - 1 - n) * C + c) * HW + p];
                const int yy = p / W, xx = p - yy * W;
                if (r.mode == 1) u = mix_pixel(u, b, r.lam, r.one_minus_lam);
                else if (yy >= r.yl && yy < r.yh && xx >= r.xl && xx < r.xh) u = b;
            }
            y[i] = norm_one<T>(u, mean[c], stdv[c]);
        }
    }
}

// header or table is device data: one kernel, the branch is taken on the header's mode when it runs (uniform over the grid)
template <typename T>
__global__ __launch_bounds__(256) void mix_normalize_kernel(const uint8_t* __restrict__ x, T* __restrict__ y,
                                                           const float* __restrict__ mean, const float* __restrict__ stdv,
                                                           const MixParams* __restrict__ pb, int N, int C, int H, int W) {
    const MixParams head = *pb;
    if (head.mode == MIX_TABLE) mix_normalize_body<T, true>(x, y, mean, stdv, pb, head, N, C, H, W);
    else mix_normalize_body<T, false>(x, y, mean, stdv, pb, head, N, C, H, W);
}

int mix_normalize(const void* x, void* y, const float* mean, const float* stdv, const void* params, int N, int C, int H, int W,
                  int dtype, hipStream_t s) {
    const int64_t planes = (int64_t)N * C;
    const int HW = H * W;
    const int64_t work = HW % 16 == 0 ? planes * (HW / 16) : planes * (int64_t)HW;
    int64_t blocks = ceil_div64(work, 256);
    if (blocks > 4096) blocks = 4096;  // grid-stride, 16 blocks per CU
    const dim3 grid((unsigned)blocks), block(256);
    const uint8_t* xs = (const uint8_t*)x;
    const MixParams* pb = (const MixParams*)params;
    switch (dtype) {
        case COT_F32: COT_LAUNCH((mix_normalize_kernel<float>), grid, block, 0, s, xs, (float*)y, mean, stdv, pb, N, C, H, W); break;
        case COT_BF16: COT_LAUNCH((mix_normalize_kernel<bf16_t>), grid, block, 0, s, xs, (bf16_t*)y, mean, stdv, pb, N, C, H, W); break;
        case COT_F16: COT_LAUNCH((mix_normalize_kernel<f16_t>), grid, block, 0, s, xs, (f16_t*)y, mean, stdv, pb, N, C, H, W); break;
        default: return set_error(COT_ERR_UNSUPPORTED, "cot_mix_normalize: output dtype %d (float32 / bfloat16 / float16)", dtype);
    }
    return check_launch("mix_normalize_kernel");
}

// ---- soft-target cross entropy

// t[n, j] = lam * oh(j, y_n) + (1 - lam) * oh(j, y_{N-1-n}),  oh = on / off  (mixup_target, mixup.py:22-27): fp32 products rounded
// separately, then added, as the reference's fp32 tensors are
struct RowTarget {
    long long y1, y2;
    float on, off, lam, oml;
    __device__ __forceinline__ float val(bool is1, bool is2) const {
#pragma clang fp contract(off)
        const float a = (is1 ? on : off) * lam;
        const float b = (is2 ? on : off) * oml;
        return a + b;
    }
    __device__ __forceinline__ float at(int j) const { return val((long long)j == y1, (long long)j == y2); }
    // sum_j t[j] over the K columns, exactly (the fp32 entries take at most four values; counted, added in double).  It is 1 only up to
    // the entries' fp32 rounding, and the derivative of -sum t*logp is p*sum(t) - t
    __device__ __forceinline__ double sum(int K) const {
        const bool in1 = y1 >= 0 && y1 < K, in2 = y2 >= 0 && y2 < K;
        if (in1 && y1 == y2) return (double)val(true, true) + (double)(K - 1) * (double)val(false, false);
        return (in1 ? (double)val(true, false) : 0.0) + (in2 ? (double)val(false, true) : 0.0) +
               (double)(K - (int)in1 - (int)in2) * (double)val(false, false);
    }
};
__device__ __forceinline__ RowTarget row_target(const long long* __restrict__ labels, const MixParams* __restrict__ pb, int n, int N,
                                                float on, float off) {
    RowTarget t;
    t.y1 = labels[n];
    t.y2 = labels[N - 1 - n];
    t.on = on;
    t.off = off;
    if (pb->mode != MIX_TABLE) {
        t.lam = pb->lam;
        t.oml = pb->one_minus_lam;
    } else if (n < pb->yl) {  // table mode: row n's own record; n < N, so nothing behind record min(R, N) - 1 is read
        t.lam = pb[1 + n].lam;
        t.oml = pb[1 + n].one_minus_lam;
    } else {  // a row past the table: the hard label
        t.lam = 1.f;
        t.oml = 0.f;
    }
    return t;
}

// one wave (= one workgroup) per row.  The probabilities are formed in fp64: the gradient p*sum(t) - t CANCELS wherever a probability
// comes close to its target (every column holds off = smoothing/K, and some of 80 000 probabilities always land within 1e-4 of it), and
// there an fp32 p -- 3e-7 relative from the rounding of log(sum) alone -- is tens of bf16 ulps off in the difference.  So the shifted
// exponentials are summed in fp64 and the row's log-sum-exp is kept for backward in the workspace `row_lse` (fp32 [4N], opaque to the
// caller): row_lse[n] = the row maximum m (exact: a logit), row_lse[N + n] and row_lse[2N + n] = log(sum_j exp(x_j - m)) as a high and a
// low part; row_lse[3N + n] = what the fp32 row_loss[n] lost of the fp64 row loss, for the mean.  N*K fp64 exponentials are nothing
// at these sizes (the kernels are latency-bound).
template <typename T>
__global__ __launch_bounds__(64) void soft_ce_forward_kernel(const T* __restrict__ logits, const long long* __restrict__ labels,
                                                            const MixParams* __restrict__ pb, float* __restrict__ row_loss,
                                                            float* __restrict__ row_lse, int N, int K, float on, float off) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const T* row = logits + (int64_t)n * K;
    const RowTarget t = row_target(labels, pb, n, N, on, off);
    float m = -INFINITY;
    for (int j = lane; j < K; j += 64) m = fmaxf(m, (float)row[j]);
    m = wave_allmax(m);
    double s = 0.0;
    for (int j = lane; j < K; j += 64) s += exp((double)(float)row[j] - (double)m);
    const double l = log(wave_allsum(s));
    double acc = 0.0;
    for (int j = lane; j < K; j += 64) acc += (double)t.at(j) * (((double)(float)row[j] - (double)m) - l);
    acc = wave_allsum(acc);
    if (lane == 0) {
        const float hi = (float)l, loss = (float)-acc;
        row_loss[n] = loss;
        row_lse[n] = m;
        row_lse[N + n] = hi;
        row_lse[2 * N + n] = (float)(l - (double)hi);
        row_lse[3 * N + n] = (float)(-acc - (double)loss);
    }
}

// mean of the row losses: one wave, lane l adds rows l, l + 64, ... in order, then the xor tree -- the same order every time.  The
// rows are added in fp64, each as row_loss[n] + its low part, and the mean is rounded ONCE: the nearest fp32 to the fp64 mean, which no
// fp32 evaluation can be closer to
__global__ __launch_bounds__(64) void row_mean_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_lo,
                                                      float* __restrict__ mean, int N) {
    double s = 0.0;
    for (int n = threadIdx.x; n < N; n += 64) s += (double)row_loss[n] + (double)row_lo[n];
    s = wave_allsum(s);
    if (threadIdx.x == 0) *mean = (float)(s / (double)N);
}

// dlogits[n, j] = g * (exp(logit - lse_n) * sum_j t[n, j] - t[n, j]) / N -- the derivative of the forward's -sum t*logp; sum t is 1 up to the
// fp32 rounding of the entries -- in fp64, rounded once;  g: the upstream gradient of the mean, one float in device memory
template <typename T>
__global__ __launch_bounds__(256) void soft_ce_backward_kernel(const T* __restrict__ logits, const long long* __restrict__ labels,
                                                              const MixParams* __restrict__ pb, const float* __restrict__ row_lse,
                                                              const float* __restrict__ g, T* __restrict__ dlogits, int N, int K,
                                                              float on, float off) {
    const int n = blockIdx.x;
    const int64_t base = (int64_t)n * K;
    const RowTarget t = row_target(labels, pb, n, N, on, off);
    const double m = (double)row_lse[n], l = (double)row_lse[N + n] + (double)row_lse[2 * N + n];
    const double scale = (double)*g / (double)N, st = t.sum(K);
    for (int j = threadIdx.x; j < K; j += 256) {
        const double p = exp(((double)(float)logits[base + j] - m) - l);
        dlogits[base + j] = (T)(float)(scale * (p * st - (double)t.at(j)));
    }
}

// off = smoothing / K, on = 1 - smoothing + off in double, then one rounding to fp32: what torch.full / scatter_ store (mixup.py:23-25)
static void on_off(double smoothing, int K, float* on, float* off) {
    const double o = smoothing / (double)K;
    *off = (float)o;
    *on = (float)(1.0 - smoothing + o);
}

int soft_ce_forward(const void* logits, const void* labels, const void* params, double smoothing, float* row_loss, float* row_lse,
                    float* mean_loss, int N, int K, int dtype, hipStream_t s) {
    float on, off;
    on_off(smoothing, K, &on, &off);
    const dim3 grid((unsigned)N), block(64);
    const long long* lb = (const long long*)labels;
    const MixParams* pb = (const MixParams*)params;
    if (dtype == COT_F32)
        COT_LAUNCH((soft_ce_forward_kernel<float>), grid, block, 0, s, (const float*)logits, lb, pb, row_loss, row_lse, N, K, on, off);
    else if (dtype == COT_BF16)
        COT_LAUNCH((soft_ce_forward_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)logits, lb, pb, row_loss, row_lse, N, K, on, off);
    else
        return set_error(COT_ERR_UNSUPPORTED, "cot_soft_target_ce_forward: logits dtype %d (float32 / bfloat16)", dtype);
    int rc = check_launch("soft_ce_forward_kernel");
    if (rc) return rc;
    COT_LAUNCH(row_mean_kernel, dim3(1), block, 0, s, (const float*)row_loss, (const float*)(row_lse + 3 * (size_t)N), mean_loss, N);
    return check_launch("row_mean_kernel");
}

int soft_ce_backward(const void* logits, const void* labels, const void* params, double smoothing, const float* row_lse,
                     const float* grad_out, void* dlogits, int N, int K, int dtype, hipStream_t s) {
    float on, off;
    on_off(smoothing, K, &on, &off);
    const dim3 grid((unsigned)N), block(256);
    const long long* lb = (const long long*)labels;
    const MixParams* pb = (const MixParams*)params;
    if (dtype == COT_F32)
        COT_LAUNCH((soft_ce_backward_kernel<float>), grid, block, 0, s, (const float*)logits, lb, pb, row_lse, grad_out, (float*)dlogits, N,
                   K, on, off);
    else if (dtype == COT_BF16)
        COT_LAUNCH((soft_ce_backward_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)logits, lb, pb, row_lse, grad_out,
                   (bf16_t*)dlogits, N, K, on, off);
    else
        return set_error(COT_ERR_UNSUPPORTED, "cot_soft_target_ce_backward: logits dtype %d (float32 / bfloat16)", dtype);
    return check_launch("soft_ce_backward_kernel");
}

}  // namespace cot
