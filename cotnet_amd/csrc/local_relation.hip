// local_relation.hip -- LR-Net's local relation (models/lr_net.py:82-96) as fused kernels (producer half).
//
// Semantics (dim = C, G = C/8 heads of 8 CONSECUTIVE q/k channels, 3x3 window t = 3i + j, pad 1):
//   logit[n,g,t,p] = sum_{j<8} q[n,8g+j,p] * (uk[n,8g+j,t,p] + pos[8g+j,t])     (:85-93; uk = 0 outside the image, :75)
//   a              = softmax over t                                              (:94)
//   out[n,c,p]     = sum_t a[n, c mod G, t, p] * v[n, c, p + off_t]  (zero pad)  (:95-96; w.view(B,1,G,9,H,W) => wC = G)
// A padded tap keeps its logit sum_j q*pos and its probability mass; only v is zero there.  The head that weights channel c
// (c mod G) is NOT the head whose q/k channels hold c (c / 8).
//
// One workgroup per (n, head g, tile of TR rows).  The tile's k / v channels (and, backward, gL / q / k) are staged into LDS as
// fp32 rows of W + 2 with the one-pixel halo and the zero padding already in place, so the 3x3 window of every pixel is
// read without a bounds test.  Everything is accumulated in fp32 in a fixed order: results are bit-identical run to run.
//
//   lr_fwd          the nine logits, the softmax and the aggregation in registers; writes out and probs ([N,1,G,9,H,W],
//                   the layout cot_agg_softmax_backward consumes).  The logits never reach HBM.
//   lr_bwd_rel      gq = sum_t gL (uk + pos);  gk[p'] = sum_t gL[p' - off_t] q[p' - off_t] (a gather over gL's halo, no
//                   atomics);  per-workgroup partial sums of gpos[c][t] = sum_p gL q  (one wave butterfly + one LDS pass).
//   lr_gpos_reduce  the partials of each (head, j, t) summed in a fixed order into gpos[C][9].
//   lr_softmax_bwd  gv and gL for the geometries the LDS-staged softmax aggregation backward (agg_nchw.hip) does not take
//                   (its 16-byte plane-stride rule); direct loads, one thread per (n, g, pixel).
// The 7x7 window (K = 7, T = 49, pad 3) has its own plan and kernels in local_relation7.hip; the host functions below route to it.
#include "cot_common.h"
#include "cot_host.h"

namespace cot {

static const char* g_lr_kernel = "";
const char* last_kernel_lr() { return g_lr_kernel; }

constexpr int LR_THREADS = 256;

struct LrPlan {
    bool ok;
    int TR, tiles, nthreads, pitch, prow;  // rows per tile, tiles per plane, threads, LDS row pitch (W + 2), rows per LDS plane
    size_t lds_bytes;
};

// rows per tile: a workgroup of at most 256 threads covers TR whole rows (a lane per pixel; wider rows loop)
static LrPlan lr_plan(int H, int W, int planes) {
    LrPlan p{};
    p.TR = LR_THREADS / W;
    if (p.TR < 1) p.TR = 1;
    if (p.TR > H) p.TR = H;
    p.tiles = (H + p.TR - 1) / p.TR;
    const int px = p.TR * W;
    p.nthreads = px >= LR_THREADS ? LR_THREADS : ((px + 63) / 64) * 64;
    p.pitch = W + 2;
    p.prow = p.TR + 2;
    p.lds_bytes = ((size_t)planes * p.prow * p.pitch + 72 + (size_t)(LR_THREADS / 64) * 72) * sizeof(float);
    p.ok = p.lds_bytes <= 64 * 1024;
    return p;
}

template <typename T, int V> static __device__ __forceinline__ void to_float(const Vec<T, V>& v, float* d) {
#pragma unroll
    for (int i = 0; i < V; ++i) d[i] = (float)v.v[i];
}

// rows r0-1 .. r0+TR of one plane (`src` = the plane's first element) -> LDS rows of `pitch` floats, columns shifted by one;
// rows outside the image and the two padding columns are zero.  W % V == 0 and the plane starts on a V-element boundary,
// so every vector load is aligned and inside the plane.
template <typename T, int V>
static __device__ __forceinline__ void stage_plane(const T* __restrict__ src, float* __restrict__ dst, int r0, int H, int W, int prow,
                                            int pitch) {
    const int vpr = W / V, items = prow * vpr;
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        const int lr = it / vpr, cv = it - lr * vpr;
        const int gr = r0 - 1 + lr;
        float f[V];
        if (gr >= 0 && gr < H) {
            to_float<T, V>(ldv<T, V>(src + (int64_t)gr * W + cv * V), f);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) f[i] = 0.f;
        }
        float* d = dst + lr * pitch + 1 + cv * V;
#pragma unroll
        for (int i = 0; i < V; ++i) d[i] = f[i];
    }
    for (int it = threadIdx.x; it < prow; it += blockDim.x) {
        dst[it * pitch] = 0.f;
        dst[it * pitch + W + 1] = 0.f;
    }
}

template <typename T, int V>
__global__ __launch_bounds__(LR_THREADS) void lr_fwd(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                      const float* __restrict__ pos, T* __restrict__ out, T* __restrict__ probs,
                                                      int C, int G, int H, int W, int TR, int tiles) {
    extern __shared__ __attribute__((aligned(16))) char cot_smem[];
    float* lds = reinterpret_cast<float*>(cot_smem);
    const int prow = TR + 2, pitch = W + 2, psz = prow * pitch;
    float* ks = lds;              // [8][prow][pitch]  k channels 8g + j
    float* vs = lds + 8 * psz;    // [8][prow][pitch]  v channels g + j G
    float* ps = lds + 16 * psz;   // [8][9]            pos[8g + j][t]
    const int tile = blockIdx.x % tiles, ng = blockIdx.x / tiles, g = ng % G, n = ng / G;
    const int r0 = tile * TR;
    const int64_t HW = (int64_t)H * W, img = (int64_t)n * C * HW;
    for (int j = 0; j < 8; ++j) {
        stage_plane<T, V>(k + img + (int64_t)(8 * g + j) * HW, ks + j * psz, r0, H, W, prow, pitch);
        stage_plane<T, V>(v + img + (int64_t)(g + j * G) * HW, vs + j * psz, r0, H, W, prow, pitch);
    }
    for (int i = threadIdx.x; i < 72; i += blockDim.x) ps[i] = pos[(int64_t)g * 72 + i];  // (blocks of 64 threads: 7 x 7 planes)
    __syncthreads();

    const int rows = H - r0 < TR ? H - r0 : TR;
    for (int pi = threadIdx.x; pi < rows * W; pi += blockDim.x) {
        const int lr = pi / W, col = pi - lr * W;
        const int64_t p = (int64_t)(r0 + lr) * W + col;
        float lg[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) lg[t] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float qj = (float)q[img + (int64_t)(8 * g + j) * HW + p];
            const float* kw = ks + j * psz + lr * pitch + col;  // window origin (tap 0) in the padded tile
#pragma unroll
            for (int t = 0; t < 9; ++t) lg[t] += qj * (kw[(t / 3) * pitch + t % 3] + ps[j * 9 + t]);
        }
        float m = lg[0];
#pragma unroll
        for (int t = 1; t < 9; ++t) m = lg[t] > m ? lg[t] : m;
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            lg[t] = expf(lg[t] - m);
            s += lg[t];
        }
        const float inv = 1.f / s;
        T* pp = probs ? probs + ((int64_t)n * G + g) * 9 * HW + p : nullptr;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const T a = (T)(lg[t] * inv);  // rounded once: the aggregation below and the backward use the same value
            lg[t] = (float)a;
            if (pp) pp[t * HW] = a;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float* vw = vs + j * psz + lr * pitch + col;
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) acc += lg[t] * vw[(t / 3) * pitch + t % 3];
            out[img + (int64_t)(g + j * G) * HW + p] = (T)acc;
        }
    }
}

// partials[((g * N + n) * tiles + tile) * 72 + j * 9 + t] = sum over the tile's pixels of gL[n,g,t,p] q[n,8g+j,p]
template <typename T, int V>
__global__ __launch_bounds__(LR_THREADS) void lr_bwd_rel(const T* __restrict__ gl, const T* __restrict__ q,
                                                          const T* __restrict__ k, const float* __restrict__ pos,
                                                          T* __restrict__ gq, T* __restrict__ gk, float* __restrict__ partials,
                                                          int N, int C, int G, int H, int W, int TR, int tiles) {
    extern __shared__ __attribute__((aligned(16))) char cot_smem[];
    float* lds = reinterpret_cast<float*>(cot_smem);
    const int prow = TR + 2, pitch = W + 2, psz = prow * pitch;
    float* ls = lds;              // [9][prow][pitch]  gL taps of head g
    float* qs = lds + 9 * psz;    // [8][prow][pitch]  q channels 8g + j
    float* ks = lds + 17 * psz;   // [8][prow][pitch]  k channels 8g + j
    float* ps = lds + 25 * psz;   // [72]
    float* red = ps + 72;         // [waves][72]
    const int tile = blockIdx.x % tiles, ng = blockIdx.x / tiles, g = ng % G, n = ng / G;
    const int r0 = tile * TR;
    const int64_t HW = (int64_t)H * W, img = (int64_t)n * C * HW;
    const T* glp = gl + ((int64_t)n * G + g) * 9 * HW;
    for (int t = 0; t < 9; ++t) stage_plane<T, V>(glp + t * HW, ls + t * psz, r0, H, W, prow, pitch);
    for (int j = 0; j < 8; ++j) {
        stage_plane<T, V>(q + img + (int64_t)(8 * g + j) * HW, qs + j * psz, r0, H, W, prow, pitch);
        stage_plane<T, V>(k + img + (int64_t)(8 * g + j) * HW, ks + j * psz, r0, H, W, prow, pitch);
    }
    for (int i = threadIdx.x; i < 72; i += blockDim.x) ps[i] = pos[(int64_t)g * 72 + i];  // (blocks of 64 threads: 7 x 7 planes)
    __syncthreads();

    // gpos: each wave folds its lanes' gL q products of one channel (9 taps) by an xor butterfly and lane 0 adds them to the
    // wave's row of `red`; the pixel loop runs the same trip count in every lane (the butterfly needs all 64), masked by `valid`
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int i = 0; i < 72; ++i) red[wave * 72 + i] = 0.f;
    const int rows = H - r0 < TR ? H - r0 : TR;
    for (int base = 0; base < rows * W; base += blockDim.x) {
        const int pi = base + threadIdx.x;
        const bool valid = pi < rows * W;
        const int lr = valid ? pi / W : 0, col = valid ? pi - lr * W : 0;
        const int64_t p = (int64_t)(r0 + lr) * W + col;
        const int ctr = (lr + 1) * pitch + col + 1;  // this pixel in the padded tile
        float gt[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) gt[t] = valid ? ls[t * psz + ctr] : 0.f;
#pragma unroll 2
        for (int j = 0; j < 8; ++j) {
            const float* kw = ks + j * psz + ctr - pitch - 1;  // window origin: p + off_0
            const float* qj = qs + j * psz;
            const float qc = qj[ctr];
            float a_q = 0.f, a_k = 0.f, gp[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int dy = t / 3 - 1, dx = t % 3 - 1;
                a_q += gt[t] * (kw[(t / 3) * pitch + t % 3] + ps[j * 9 + t]);
                const int src = ctr - dy * pitch - dx;  // p - off_t: zero outside the image in both staged planes
                a_k += ls[t * psz + src] * qj[src];
                gp[t] = gt[t] * qc;
            }
            if (valid) {
                gq[img + (int64_t)(8 * g + j) * HW + p] = (T)a_q;
                gk[img + (int64_t)(8 * g + j) * HW + p] = (T)a_k;
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                // cot_reduce.h's wave_allsum, left open-coded: as a call it is unrolled before it is inlined, which reschedules every
                // lr_bwd_rel instance (same arithmetic, 272 assembly lines moved; profiles/reduce_header_isa_diff.log)
                float s = gp[t];
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
                if (lane == 0) red[wave * 72 + j * 9 + t] += s;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 72; i += blockDim.x) {  // the waves in order
        float s = 0.f;
        const int nw = blockDim.x >> 6;
        for (int w = 0; w < nw; ++w) s += red[w * 72 + i];
        partials[(((int64_t)g * N + n) * tiles + tile) * 72 + i] = s;
    }
}

// one workgroup per (g, j*9 + t): strided sums over the N * tiles partial rows, then a fixed LDS tree
__global__ __launch_bounds__(LR_THREADS) void lr_gpos_reduce(const float* __restrict__ partials, float* __restrict__ gpos,
                                                              int rows) {
    __shared__ float sh[LR_THREADS];
    const int g = blockIdx.x / 72, jt = blockIdx.x - g * 72;
    const float* src = partials + (int64_t)g * rows * 72 + jt;
    float s = 0.f;
    for (int r = threadIdx.x; r < rows; r += LR_THREADS) s += src[(int64_t)r * 72];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = LR_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) gpos[blockIdx.x] = sh[0];  // (c = 8g + j: gpos[c * 9 + t] = gpos[g * 72 + j * 9 + t])
}

// gv[n, g + jG, p'] = sum_t a[n,g,t,p' - off_t] gout[n, g + jG, p' - off_t]   (valid p' - off_t only)
// gL[n,g,t,p]       = a_t (gA_t - sum_u a_u gA_u),  gA_t = sum_j gout[n, g + jG, p] v[n, g + jG, p + off_t]
template <typename T>
__global__ __launch_bounds__(LR_THREADS) void lr_softmax_bwd(const T* __restrict__ gout, const T* __restrict__ v,
                                                              const T* __restrict__ probs, T* __restrict__ gv,
                                                              T* __restrict__ gl, int N, int C, int G, int H, int W) {
    const int64_t HW = (int64_t)H * W;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)N * G * HW) return;
    const int64_t p = idx % HW, ng = idx / HW;
    const int g = (int)(ng % G), n = (int)(ng / G);
    const int h = (int)(p / W), w = (int)(p - (int64_t)h * W);
    const int64_t img = (int64_t)n * C * HW;
    const T* pr = probs + ng * 9 * HW;
    float a[9], ga[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        a[t] = (float)pr[t * HW + p];
        ga[t] = 0.f;
    }
    for (int j = 0; j < 8; ++j) {
        const int64_t pl = img + (int64_t)(g + j * G) * HW;
        const float go = (float)gout[pl + p];
        float sv = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            const int hh = h + dy, ww = w + dx;
            const bool in = hh >= 0 && hh < H && ww >= 0 && ww < W;
            ga[t] += in ? go * (float)v[pl + (int64_t)hh * W + ww] : 0.f;
            const int hs = h - dy, ws = w - dx;
            const bool ins = hs >= 0 && hs < H && ws >= 0 && ws < W;
            const int64_t ps = (int64_t)hs * W + ws;
            sv += ins ? (float)pr[t * HW + ps] * (float)gout[pl + ps] : 0.f;
        }
        gv[pl + p] = (T)sv;
    }
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) dot += a[t] * ga[t];
    T* gp = gl + ng * 9 * HW + p;
#pragma unroll
    for (int t = 0; t < 9; ++t) gp[t * HW] = (T)(a[t] * (ga[t] - dot));
}

static inline int lr_vec(int W) { return W % 4 == 0 ? 4 : (W % 2 == 0 ? 2 : 1); }

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool lr_covers(const cot_agg_geom& g) {
    if (g.kh == 7 && g.kw == 7) return lr7_covers(g);  // the 7x7 window: local_relation7.hip, its own plan
    return g.kh == 3 && g.kw == 3 && g.sh == 1 && g.sw == 1 && g.ph == 1 && g.pw == 1 && g.dh == 1 && g.dw == 1 && g.heads == 1 &&
           g.C % 8 == 0 && g.wC * 8 == g.C && lr_plan(g.H, g.W, 25).ok && (int64_t)g.N * g.wC * lr_plan(g.H, g.W, 25).tiles < (1LL << 31);
}

// [glogits: N G 9 HW elements, 256-byte aligned][partials: G N tiles 72 floats]
int64_t lr_workspace_bytes(const cot_agg_geom& g, size_t esize) {
    if (g.kh == 7) return lr7_workspace_bytes(g, esize);
    const LrPlan p = lr_plan(g.H, g.W, 25);
    return (int64_t)(align256((size_t)g.N * g.wC * 9 * g.H * g.W * esize) + (size_t)g.wC * g.N * p.tiles * 72 * sizeof(float));
}

template <typename T>
int lr_forward(const T* q, const T* k, const T* v, const float* pos, T* out, T* probs, const cot_agg_geom& g, hipStream_t s) {
    if (g.kh == 7) {
        const int rc = lr7_forward<T>(q, k, v, pos, out, probs, g, s);
        g_lr_kernel = last_kernel_lr7();
        return rc;
    }
    const LrPlan p = lr_plan(g.H, g.W, 16);
    const int G = g.wC;
    const dim3 grid((unsigned)((int64_t)g.N * G * p.tiles)), block(p.nthreads);
    switch (lr_vec(g.W)) {
        case 4: COT_LAUNCH((lr_fwd<T, 4>), grid, block, p.lds_bytes, s, q, k, v, pos, out, probs, g.C, G, g.H, g.W, p.TR, p.tiles); break;
        case 2: COT_LAUNCH((lr_fwd<T, 2>), grid, block, p.lds_bytes, s, q, k, v, pos, out, probs, g.C, G, g.H, g.W, p.TR, p.tiles); break;
        default: COT_LAUNCH((lr_fwd<T, 1>), grid, block, p.lds_bytes, s, q, k, v, pos, out, probs, g.C, G, g.H, g.W, p.TR, p.tiles);
    }
    g_lr_kernel = "lr_fwd";
    return check_launch(g_lr_kernel);
}

template <typename T>
int lr_backward(const T* gout, const T* q, const T* k, const T* v, const float* pos, const T* probs, T* gq, T* gk, T* gv,
                float* gpos, void* workspace, const cot_agg_geom& g, hipStream_t s) {
    if (g.kh == 7) {
        const int rc = lr7_backward<T>(gout, q, k, v, pos, probs, gq, gk, gv, gpos, workspace, g, s);
        g_lr_kernel = last_kernel_lr7();
        return rc;
    }
    const LrPlan p = lr_plan(g.H, g.W, 25);
    const int G = g.wC;
    const int64_t HW = (int64_t)g.H * g.W;
    T* gl = reinterpret_cast<T*>(workspace);
    float* partials = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + align256((size_t)g.N * G * 9 * HW * sizeof(T)));
    // (a) gv and gL: the LDS-staged softmax aggregation backward where it applies, else the direct kernel
    int rc = agg_softmax_backward_nchw<T>(gout, v, probs, gv, gl, g, s);
    const char* first = "agg_softmax_backward";
    if (rc == COT_ERR_UNSUPPORTED) {
        const int64_t items = (int64_t)g.N * G * HW;
        COT_LAUNCH((lr_softmax_bwd<T>), dim3((unsigned)ceil_div64(items, LR_THREADS)), dim3(LR_THREADS), 0, s, gout, v, probs, gv, gl,
                   g.N, g.C, G, g.H, g.W);
        first = "lr_softmax_bwd";
        rc = check_launch(first);
    }
    if (rc) return rc;
    // (b) gq, gk and the per-workgroup gpos partials
    const dim3 grid((unsigned)((int64_t)g.N * G * p.tiles)), block(p.nthreads);
    switch (lr_vec(g.W)) {
        case 4: COT_LAUNCH((lr_bwd_rel<T, 4>), grid, block, p.lds_bytes, s, gl, q, k, pos, gq, gk, partials, g.N, g.C, G, g.H, g.W, p.TR, p.tiles); break;
        case 2: COT_LAUNCH((lr_bwd_rel<T, 2>), grid, block, p.lds_bytes, s, gl, q, k, pos, gq, gk, partials, g.N, g.C, G, g.H, g.W, p.TR, p.tiles); break;
        default: COT_LAUNCH((lr_bwd_rel<T, 1>), grid, block, p.lds_bytes, s, gl, q, k, pos, gq, gk, partials, g.N, g.C, G, g.H, g.W, p.TR, p.tiles);
    }
    if ((rc = check_launch("lr_bwd_rel"))) return rc;
    // (c) gpos[C][9]
    COT_LAUNCH(lr_gpos_reduce, dim3((unsigned)(G * 72)), dim3(LR_THREADS), 0, s, partials, gpos, g.N * p.tiles);
    g_lr_kernel = first[0] == 'l' ? "lr_softmax_bwd+lr_bwd_rel+lr_gpos_reduce" : "agg_bwd_nchw_k3_lds<softmax>+lr_bwd_rel+lr_gpos_reduce";
    return check_launch("lr_gpos_reduce");
}

#define LR_INSTANTIATE(T)                                                                                                    \
    template int lr_forward<T>(const T*, const T*, const T*, const float*, T*, T*, const cot_agg_geom&, hipStream_t);        \
    template int lr_backward<T>(const T*, const T*, const T*, const T*, const float*, const T*, T*, T*, T*, float*, void*,   \
                                const cot_agg_geom&, hipStream_t);
LR_INSTANTIATE(float)
LR_INSTANTIATE(bf16_t)

}  // namespace cot
