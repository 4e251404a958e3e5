// eval_score.hip -- what a validation pass keeps of every batch, on the device, gfx950: top-1 / top-5 hits and the summed negative
// log-likelihood of [N, K] logits against integer labels, ADDED to one 32-byte block in device memory (cot_eval_acc, include/cotnet_amd.h).
//
// Reference: utils/meters.py:12-19 (`accuracy`: topk(5), a transpose, eq, two sums) and evaler/evaler.py:50-52 (one `accuracy` and one
// torch.cuda.synchronize() per batch; utils/meters.py:154-157 adds the counts on the host).  Here a pass is read by the host ONCE, at
// its end: every batch is two launches that leave their result in the block, so the pair can be recorded into a HIP graph behind the
// model's forward and replayed on new logits and labels.
//
//   eval_rows_kernel        latency-bound like cot_soft_target_ce_forward (N x K logits, 256 KB at 128 x 1000 bf16): one wave per row.
//                           Rows of up to 1024 columns are read ONCE, 16 columns per lane held in registers, and the maximum, the
//                           target's rank and the sum of exponentials are all formed from them; longer rows are walked twice out of
//                           the cache.  rank = #{j: x_j > t} + #{j < y: x_j == t} -- the target's place in a stable descending sort --
//                           so no top-k selection is needed at all.  The label is only COMPARED with column indices (the target logit
//                           is picked up by the lane that meets j == y): a label outside [0, K) matches nothing and marks the row
//                           skipped, which is how a padded last batch is expressed.
//   eval_accumulate_kernel  one wave adds the rows' results in ascending row order (64 at a time through LDS, summed by lane 0) and
//                           performs acc += totals as lane 0's plain read-modify-write.  No atomics: equal bits on every run, eager
//                           or replayed; successive calls are ordered by the stream.
//
// The rows' results travel between the two launches in g_eval_rows, a fixed array in device memory that belongs to this file (the entry
// point has no workspace argument, and an allocation could not be made while a stream records).  It holds EVAL_ROWS_CAP rows; a longer
// batch is served in slices of that many rows, one launch pair each, in row order.  Calls on DIFFERENT streams of one device share it
// and must be ordered by the caller.
#include <math.h>

#include "cot_reduce.h"
#include "cot_host.h"

namespace cot {

struct EvalAcc {  // = cot_eval_acc
    long long samples, top1, top5;
    double nll_sum;
};
static_assert(sizeof(EvalAcc) == 32 && sizeof(EvalAcc) == sizeof(cot_eval_acc), "the accumulator block is 4 x 64-bit words");

struct EvalRow {
    double nll;  // fp64 row loss; 0 for a skipped row
    int flags;   // bit 0 valid, bit 1 rank == 0, bit 2 rank < 5
    int pad;
};
constexpr int EVAL_ROWS_CAP = 4096;  // rows per launch pair (64 KB)
constexpr int EVAL_REG = 16;         // columns a lane holds: rows of up to 64 * 16 columns are read once
__device__ EvalRow g_eval_rows[EVAL_ROWS_CAP];

// the order of torch's descending sort: NaN above everything, NaNs equal among themselves
__device__ __forceinline__ bool ev_greater(float a, float b) { return a > b || (a != a && b == b); }
__device__ __forceinline__ bool ev_same(float a, float b) { return a == b || (a != a && b != b); }

template <typename T, bool FITS>
__global__ __launch_bounds__(64) void eval_rows_kernel(const T* __restrict__ logits, const long long* __restrict__ labels,
                                                      int* __restrict__ row_rank, float* __restrict__ row_nll, int K) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const long long y = labels[n];
    if (y < 0 || y >= (long long)K) {  // skipped (wave-uniform)
        if (lane == 0) {
            g_eval_rows[n].nll = 0.0;
            g_eval_rows[n].flags = 0;
            if (row_rank) row_rank[n] = -1;
            if (row_nll) row_nll[n] = 0.0f;
        }
        return;
    }
    const T* row = logits + (int64_t)n * K;
    constexpr int HELD = FITS ? EVAL_REG : 1;
    float v[HELD];
    if (FITS) {
#pragma unroll
        for (int i = 0; i < HELD; ++i) {
            const int j = lane + 64 * i;
            v[i] = j < K ? (float)row[j] : -INFINITY;
        }
    }
    const int steps = FITS ? EVAL_REG : (K + 63) / 64;  // (FITS: a constant, and `unroll 16` below unrolls the loops whole)
    static_assert(EVAL_REG == 16, "the unroll counts below");
#define EV_AT(i, j) (FITS ? v[FITS ? (i) : 0] : (float)row[j])
    // the maximum (NaN aside, as fmaxf leaves it) and the target logit, picked up where the column index meets the label
    float m = -INFINITY;
    unsigned tbits = 0;
#pragma unroll 16
    for (int i = 0; i < steps; ++i) {
        const int j = lane + 64 * i;
        if (j < K) {
            const float x = EV_AT(i, j);
            m = fmaxf(m, x);
            if ((long long)j == y) tbits = __builtin_bit_cast(unsigned, x);
        }
    }
    m = wave_allmax(m);
    const float t = __builtin_bit_cast(float, wave_allor(tbits));  // one lane holds it, the others 0
    int rank = 0;
    double s = 0.0;
#pragma unroll 16
    for (int i = 0; i < steps; ++i) {
        const int j = lane + 64 * i;
        if (j < K) {
            const float x = EV_AT(i, j);
            rank += (ev_greater(x, t) || ((long long)j < y && ev_same(x, t))) ? 1 : 0;
            s += exp((double)x - (double)m);
        }
    }
#undef EV_AT
    rank = wave_allsum(rank);
    const double nll = log(wave_allsum(s)) - ((double)t - (double)m);  // = logsumexp(row) - t
    if (lane == 0) {
        g_eval_rows[n].nll = nll;
        g_eval_rows[n].flags = 1 | (rank == 0 ? 2 : 0) | (rank < 5 ? 4 : 0);
        if (row_rank) row_rank[n] = rank;
        if (row_nll) row_nll[n] = (float)nll;
    }
}

__global__ __launch_bounds__(64) void eval_accumulate_kernel(EvalAcc* acc, int N) {
    __shared__ double s_nll[64];
    __shared__ int s_flags[64];
    const int lane = threadIdx.x;
    long long samples = 0, top1 = 0, top5 = 0;
    double sum = 0.0;
    for (int base = 0; base < N; base += 64) {
        const int n = base + lane;
        s_nll[lane] = n < N ? g_eval_rows[n].nll : 0.0;
        s_flags[lane] = n < N ? g_eval_rows[n].flags : 0;
        __syncthreads();
        if (lane == 0) {
            const int cnt = N - base < 64 ? N - base : 64;
            for (int i = 0; i < cnt; ++i) {  // (not shared with grad_clip_finish_kernel's ordered loop: that one runs under a prefetch)
                const int f = s_flags[i];
                if (f & 1) {
                    samples += 1;
                    top1 += (f >> 1) & 1;
                    top5 += (f >> 2) & 1;
                    sum += s_nll[i];
                }
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        acc->samples += samples;
        acc->top1 += top1;
        acc->top5 += top5;
        acc->nll_sum += sum;
    }
}

template <typename T>
static int eval_score_slice(const T* logits, const long long* labels, EvalAcc* acc, int* row_rank, float* row_nll, int N, int K,
                            hipStream_t s) {
    const dim3 grid((unsigned)N), block(64);
    if (K <= 64 * EVAL_REG)
        COT_LAUNCH((eval_rows_kernel<T, true>), grid, block, 0, s, logits, labels, row_rank, row_nll, K);
    else
        COT_LAUNCH((eval_rows_kernel<T, false>), grid, block, 0, s, logits, labels, row_rank, row_nll, K);
    int rc = check_launch("eval_rows_kernel");
    if (rc) return rc;
    COT_LAUNCH(eval_accumulate_kernel, dim3(1), block, 0, s, acc, N);
    return check_launch("eval_accumulate_kernel");
}

int eval_score(const void* logits, const void* labels, void* acc, int* row_rank, float* row_nll, int N, int K, int dtype, hipStream_t s) {
    for (int n0 = 0; n0 < N; n0 += EVAL_ROWS_CAP) {
        const int cnt = N - n0 < EVAL_ROWS_CAP ? N - n0 : EVAL_ROWS_CAP;
        const long long* lb = (const long long*)labels + n0;
        int* rr = row_rank ? row_rank + n0 : nullptr;
        float* rn = row_nll ? row_nll + n0 : nullptr;
        const int64_t off = (int64_t)n0 * K;
        int rc;
        if (dtype == COT_F32)
            rc = eval_score_slice((const float*)logits + off, lb, (EvalAcc*)acc, rr, rn, cnt, K, s);
        else if (dtype == COT_BF16)
            rc = eval_score_slice((const bf16_t*)logits + off, lb, (EvalAcc*)acc, rr, rn, cnt, K, s);
        else
            return set_error(COT_ERR_UNSUPPORTED, "cot_eval_score: logits dtype %d (float32 / bfloat16)", dtype);
        if (rc) return rc;
    }
    return COT_OK;
}

}  // namespace cot
