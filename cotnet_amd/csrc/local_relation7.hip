// local_relation7.hip -- LR-Net's local relation at its own 7x7 window (models/lr_net.py:82-96 with kernel_size = 7).
//
// Semantics: the header of local_relation.hip with K = 7, T = 49 taps t = 7i + j (nn.Unfold's order), pad 3:
//   logit[n,g,t,p] = sum_{j<8} q[n,8g+j,p] * (uk[n,8g+j,t,p] + pos[8g+j,t])     uk = 0 outside the image
//   a              = softmax over t
//   out[n,c,p]     = sum_t a[n, c mod G, t, p] * v[n, c, p + off_t]              zero pad
// A padded tap keeps its logit sum_j q*pos and its probability mass; only v is zero there.
//
// One workgroup per (n, head g, tile of TR whole rows), ONE LANE PER PIXEL (TR W <= 256), so a lane's 49 logits / probabilities /
// gA live in registers across the barriers between staging steps.  Planes are staged into LDS as fp32 rows of W + 6 with the
// three-pixel halo and the zero padding in place (vector loads of V elements), so no window read tests a bound.  Every sum is
// fp32 in a fixed order, nothing is atomic: results are bit-identical run to run.
//
//   lr7_fwd          stages the 8 k planes, forms the 49 logits and the softmax in registers, re-stages the same LDS with the
//                    8 v planes, aggregates.  Writes out and probs [N,1,G,49,H,W]; each probability is rounded to storage once
//                    and the aggregation uses the rounded value.
//   lr7_bwd_agg      gv and gL.  gout / v planes (JC channels at a time) stay staged with the full halo; the probabilities are
//                    staged ONE WINDOW ROW (7 taps) AT A TIME, twice: at the tile's own rows (a_t of this pixel, for sum_u a_u
//                    gA_u; last pass only) and at the rows r - dy, where the pixels sit whose tap (dy, .) lands on this tile
//                    (gv is a gather, like gk below).  gA_t = sum_j gout_j v_j[p + off_t] stays in 49 registers;
//                    gL_t = a_t (gA_t - sum_u a_u gA_u)  -> the caller's workspace.
//   lr7_bwd_rel      gq = sum_t gL_t (uk_t + pos_t);  gk[p'] = sum_t gL_t[p' - off_t] q[p' - off_t];  gL staged a window row
//                    at a time the same two ways, q / k planes staged with the full halo.  gpos[c][t] = sum_p gL_t q_c needs
//                    no cross-lane exchange: thread (c, t, part) sums a fixed strided share of the tile's pixels out of LDS and
//                    the parts are added in order -- no wave butterflies (the 3x3 kernel spends 72 per pixel on them).
//   lr7_gpos_reduce  the per-workgroup partials of each (head, j, t) summed in a fixed order into gpos[C][49].
//
// pos is read straight from global memory at workgroup-uniform addresses (scalar loads: it costs no LDS traffic and no LDS space).
//
// LDS: (2 JC planes of (TR + 6)(W + 6) + 14 planes of TR (W + 6) + 256) floats, plane sizes rounded up to odd (the gpos pass
// strides over planes); JC = 8 where that fits the project's 64 KiB per-workgroup cap (every LR-Net-50 stage does: 53 KiB at
// 56 x 56), else 4 (two passes over the window rows; one-row tiles up to W = 224).  The cap is kept: two workgroups per CU.
#include "cot_common.h"
#include "cot_host.h"

namespace cot {

static const char* g_lr7_kernel = "";
const char* last_kernel_lr7() { return g_lr7_kernel; }

constexpr int L7_THREADS = 256;
constexpr int L7_T = 49;           // taps
constexpr int L7_POS = 8 * L7_T;   // pos / gpos floats of one head

struct Lr7Plan {
    bool ok;
    int TR, tiles, nthreads, JC;  // rows per tile, tiles per plane, threads, channels staged per pass of the backward kernels
    size_t lds_fwd, lds_bwd;
};

static size_t lr7_lds_bwd(int TR, int W, int JC) {
    const size_t pszH = ((size_t)(TR + 6) * (W + 6)) | 1, pszR = ((size_t)TR * (W + 6)) | 1;
    return (2 * JC * pszH + 14 * pszR + L7_THREADS) * sizeof(float);
}

static Lr7Plan lr7_plan(int H, int W) {
    Lr7Plan p{};
    if (H < 1 || W < 1 || W > L7_THREADS) return p;  // a lane per pixel, whole rows
    p.TR = L7_THREADS / W;
    if (p.TR > H) p.TR = H;
    p.tiles = (H + p.TR - 1) / p.TR;
    const int px = p.TR * W;
    p.nthreads = ((px + 63) / 64) * 64;
    p.JC = lr7_lds_bwd(p.TR, W, 8) <= 64 * 1024 ? 8 : 4;
    p.lds_bwd = lr7_lds_bwd(p.TR, W, p.JC);
    p.lds_fwd = 8 * (((size_t)(p.TR + 6) * (W + 6)) | 1) * sizeof(float);  // (< lds_bwd at JC = 4)
    p.ok = p.lds_bwd <= 64 * 1024;
    return p;
}

// rows gr0 .. gr0 + nrows - 1 of `nplanes` planes (plane i starts at src + i * sstride and lands at dst + i * dstride) -> LDS rows of
// `pitch` = W + 6 floats, columns shifted by three; rows outside the image and the six padding columns are zero.  One flat loop over
// all the planes' vectors, so every lane has work and its loads are in flight together (a loop per plane leaves most of a workgroup
// idle on a 7-row slice and pays the load latency once per plane).  W % V == 0 and every plane starts on a V-element boundary, so
// each vector load is aligned and inside its plane.
template <typename T, int V>
static __device__ __forceinline__ void l7_stage(const T* __restrict__ src, int64_t sstride, float* __restrict__ dst, int dstride,
                                                int nplanes, int gr0, int nrows, int H, int W, int pitch) {
    const int vpr = W / V, per = nrows * vpr, items = nplanes * per;
#pragma unroll 4
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        const int pl = it / per, r = it - pl * per;
        const int lr = r / vpr, cv = r - lr * vpr;
        const int gr = gr0 + lr;
        float* d = dst + pl * dstride + lr * pitch + 3 + cv * V;
        if (gr >= 0 && gr < H) {
            const Vec<T, V> x = ldv<T, V>(src + pl * sstride + (int64_t)gr * W + cv * V);
#pragma unroll
            for (int i = 0; i < V; ++i) d[i] = (float)x.v[i];
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) d[i] = 0.f;
        }
    }
    for (int it = threadIdx.x; it < nplanes * nrows * 6; it += blockDim.x) {
        const int row = it / 6, c = it - row * 6;  // row = pl * nrows + lr
        const int pl = row / nrows, lr = row - pl * nrows;
        dst[pl * dstride + lr * pitch + (c < 3 ? c : W + c)] = 0.f;
    }
}

template <typename T, int V>
__global__ __launch_bounds__(L7_THREADS) void lr7_fwd(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                       const float* __restrict__ pos, T* __restrict__ out, T* __restrict__ probs,
                                                       int C, int G, int H, int W, int TR, int tiles) {
    extern __shared__ __attribute__((aligned(16))) char cot_smem[];
    float* lds = reinterpret_cast<float*>(cot_smem);
    const int prow = TR + 6, pitch = W + 6, psz = (prow * pitch) | 1;
    float* pl = lds;  // [8][psz]  k channels 8g + j, then v channels g + j G
    const int tile = blockIdx.x % tiles, ng = blockIdx.x / tiles, g = ng % G, n = ng / G;
    const int r0 = tile * TR;
    const int64_t HW = (int64_t)H * W, img = (int64_t)n * C * HW;
    const float* __restrict__ ps = pos + (int64_t)g * L7_POS;  // [8][49]  pos[8g + j][t], workgroup-uniform addresses
    l7_stage<T, V>(k + img + (int64_t)8 * g * HW, HW, pl, psz, 8, r0 - 3, prow, H, W, pitch);
    __syncthreads();

    const int rows = H - r0 < TR ? H - r0 : TR;
    const bool valid = (int)threadIdx.x < rows * W;  // lanes past the tile's pixels only keep the barriers company
    const int lr = valid ? (int)threadIdx.x / W : 0, col = valid ? (int)threadIdx.x - lr * W : 0;
    const int64_t p = (int64_t)(r0 + lr) * W + col;
    const int org = lr * pitch + col;  // window origin (tap 0) in a padded plane
    float lg[L7_T];
#pragma unroll
    for (int t = 0; t < L7_T; ++t) lg[t] = 0.f;
#pragma unroll 2
    for (int j = 0; j < 8; ++j) {
        const float qj = valid ? (float)q[img + (int64_t)(8 * g + j) * HW + p] : 0.f;
        const float* kw = pl + j * psz + org;
#pragma unroll
        for (int t = 0; t < L7_T; ++t) lg[t] += qj * (kw[(t / 7) * pitch + t % 7] + ps[j * L7_T + t]);
    }
    float m = lg[0];
#pragma unroll
    for (int t = 1; t < L7_T; ++t) m = lg[t] > m ? lg[t] : m;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < L7_T; ++t) {
        lg[t] = expf(lg[t] - m);
        s += lg[t];
    }
    const float inv = 1.f / s;
    T* pp = probs && valid ? probs + ((int64_t)n * G + g) * L7_T * HW + p : nullptr;
#pragma unroll
    for (int t = 0; t < L7_T; ++t) {
        const T a = (T)(lg[t] * inv);  // rounded once: the aggregation below and the backward use the same value
        lg[t] = (float)a;
        if (pp) pp[t * HW] = a;
    }
    __syncthreads();  // every lane is done with the k planes
    l7_stage<T, V>(v + img + (int64_t)g * HW, G * HW, pl, psz, 8, r0 - 3, prow, H, W, pitch);
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < 8; ++j) {
        const float* vw = pl + j * psz + org;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < L7_T; ++t) acc += lg[t] * vw[(t / 7) * pitch + t % 7];
        if (valid) out[img + (int64_t)(g + j * G) * HW + p] = (T)acc;
    }
}

// gv[n, g + jG, p'] = sum_t a[n,g,t,p' - off_t] gout[n, g + jG, p' - off_t]   (both staged zero outside the image)
// gL[n,g,t,p]       = a_t (gA_t - sum_u a_u gA_u),  gA_t = sum_j gout[n, g + jG, p] v[n, g + jG, p + off_t]
// The window-row loop stays rolled (one copy of the staging code); a row's seven gA are formed in `ga` and filed into the 49
// registers by a branch on the wave-uniform row index.
template <typename T, int V, int JC>
__global__ __launch_bounds__(L7_THREADS) void lr7_bwd_agg(const T* __restrict__ gout, const T* __restrict__ v,
                                                           const T* __restrict__ probs, T* __restrict__ gv, T* __restrict__ gl,
                                                           int C, int G, int H, int W, int TR, int tiles) {
    extern __shared__ __attribute__((aligned(16))) char cot_smem[];
    float* lds = reinterpret_cast<float*>(cot_smem);
    const int prow = TR + 6, pitch = W + 6, pszH = (prow * pitch) | 1, pszR = (TR * pitch) | 1;
    float* gs = lds;                  // [JC][pszH]  gout channels g + (j0 + jj) G, full halo
    float* vs = gs + JC * pszH;       // [JC][pszH]  v, the same channels
    float* ac = vs + JC * pszH;       // [7][pszR]   a of window row i at the tile's own rows (last pass only)
    float* as = ac + 7 * pszR;        // [7][pszR]   a of window row i at rows r - dy
    const int tile = blockIdx.x % tiles, ng = blockIdx.x / tiles, g = ng % G, n = ng / G;
    const int r0 = tile * TR;
    const int64_t HW = (int64_t)H * W, img = (int64_t)n * C * HW;
    const T* pr = probs + ((int64_t)n * G + g) * L7_T * HW;
    const int rows = H - r0 < TR ? H - r0 : TR;
    const bool valid = (int)threadIdx.x < rows * W;
    const int lr = valid ? (int)threadIdx.x / W : 0, col = valid ? (int)threadIdx.x - lr * W : 0;
    const int64_t p = (int64_t)(r0 + lr) * W + col;
    const int ctr = (lr + 3) * pitch + col + 3;  // this pixel in a full-halo plane
    float gA[L7_T], dot = 0.f;
#pragma unroll
    for (int t = 0; t < L7_T; ++t) gA[t] = 0.f;
#pragma unroll
    for (int j0 = 0; j0 < 8; j0 += JC) {
        const bool last = j0 + JC == 8;  // gA is complete in the last pass: sum_u a_u gA_u is formed there
        // (the barrier that ends the previous pass's last window row covers these writes)
        l7_stage<T, V>(gout + img + (int64_t)(g + j0 * G) * HW, G * HW, gs, pszH, JC, r0 - 3, prow, H, W, pitch);
        l7_stage<T, V>(v + img + (int64_t)(g + j0 * G) * HW, G * HW, vs, pszH, JC, r0 - 3, prow, H, W, pitch);
        float gva[JC];
#pragma unroll
        for (int jj = 0; jj < JC; ++jj) gva[jj] = 0.f;
#pragma unroll 1
        for (int i = 0; i < 7; ++i) {
            if (last) l7_stage<T, V>(pr + (int64_t)7 * i * HW, HW, ac, pszR, 7, r0, TR, H, W, pitch);
            l7_stage<T, V>(pr + (int64_t)7 * i * HW, HW, as, pszR, 7, r0 - (i - 3), TR, H, W, pitch);
            __syncthreads();
            float ga[7];
#pragma unroll
            for (int jx = 0; jx < 7; ++jx) ga[jx] = 0.f;
            const float* aw = as + lr * pitch + col + 6;  // tap (i, jx) comes from pixel (r - dy, c - dx): column c + 3 - dx
#pragma unroll
            for (int jj = 0; jj < JC; ++jj) {
                const float go = gs[jj * pszH + ctr];
                const float* vw = vs + jj * pszH + (lr + i) * pitch + col;
                const float* gw = gs + jj * pszH + (lr + 6 - i) * pitch + col + 6;
#pragma unroll
                for (int jx = 0; jx < 7; ++jx) {
                    ga[jx] += go * vw[jx];
                    gva[jj] += aw[jx * pszR - jx] * gw[-jx];
                }
            }
#pragma unroll
            for (int ii = 0; ii < 7; ++ii)
                if (i == ii) {
#pragma unroll
                    for (int jx = 0; jx < 7; ++jx) {
                        gA[7 * ii + jx] += ga[jx];
                        ga[jx] = gA[7 * ii + jx];
                    }
                }
            if (last) {
#pragma unroll
                for (int jx = 0; jx < 7; ++jx) dot += ac[jx * pszR + lr * pitch + col + 3] * ga[jx];
            }
            __syncthreads();  // before the next window row (or the next pass) overwrites what was just read
        }
        if (valid) {
#pragma unroll
            for (int jj = 0; jj < JC; ++jj) gv[img + (int64_t)(g + (j0 + jj) * G) * HW + p] = (T)gva[jj];
        }
    }
    if (valid) {
        T* gp = gl + ((int64_t)n * G + g) * L7_T * HW + p;
#pragma unroll
        for (int t = 0; t < L7_T; ++t) gp[t * HW] = (T)((float)pr[t * HW + p] * (gA[t] - dot));
    }
}

// partials[((g * N + n) * tiles + tile) * 392 + j * 49 + t] = sum over the tile's pixels of gL[n,g,t,p] q[n,8g+j,p]
template <typename T, int V, int JC>
__global__ __launch_bounds__(L7_THREADS) void lr7_bwd_rel(const T* __restrict__ gl, const T* __restrict__ q,
                                                           const T* __restrict__ k, const float* __restrict__ pos,
                                                           T* __restrict__ gq, T* __restrict__ gk, float* __restrict__ partials,
                                                           int N, int C, int G, int H, int W, int TR, int tiles) {
    extern __shared__ __attribute__((aligned(16))) char cot_smem[];
    float* lds = reinterpret_cast<float*>(cot_smem);
    const int prow = TR + 6, pitch = W + 6, pszH = (prow * pitch) | 1, pszR = (TR * pitch) | 1;
    float* qs = lds;                  // [JC][pszH]  q channels 8g + j0 + jj, full halo
    float* ks = qs + JC * pszH;       // [JC][pszH]  k, the same channels
    float* lc = ks + JC * pszH;       // [7][pszR]   gL of window row i at the tile's own rows
    float* ls = lc + 7 * pszR;        // [7][pszR]   gL of window row i at rows r - dy
    float* red = ls + 7 * pszR;       // [parts][JC * 7]
    const int tile = blockIdx.x % tiles, ng = blockIdx.x / tiles, g = ng % G, n = ng / G;
    const int r0 = tile * TR;
    const int64_t HW = (int64_t)H * W, img = (int64_t)n * C * HW;
    const T* glp = gl + ((int64_t)n * G + g) * L7_T * HW;
    float* part_out = partials + (((int64_t)g * N + n) * tiles + tile) * L7_POS;
    const int rows = H - r0 < TR ? H - r0 : TR;
    const bool valid = (int)threadIdx.x < rows * W;
    const int lr = valid ? (int)threadIdx.x / W : 0, col = valid ? (int)threadIdx.x - lr * W : 0;
    const int64_t p = (int64_t)(r0 + lr) * W + col;
    // the gpos pass: thread (part, o = jj * 7 + jx) sums columns part, part + parts, .. of every row, then the parts in order
    constexpr int OUTS = JC * 7;
    const int parts = (int)blockDim.x / OUTS, o = (int)threadIdx.x % OUTS, part = (int)threadIdx.x / OUTS;
    const int ojj = o / 7, ojx = o - ojj * 7;
    const float* __restrict__ ps = pos + (int64_t)g * L7_POS;  // [8][49]  pos[8g + j][t], workgroup-uniform addresses
#pragma unroll
    for (int j0 = 0; j0 < 8; j0 += JC) {
        // (the barrier that ends the previous pass's last window row covers these writes)
        l7_stage<T, V>(q + img + (int64_t)(8 * g + j0) * HW, HW, qs, pszH, JC, r0 - 3, prow, H, W, pitch);
        l7_stage<T, V>(k + img + (int64_t)(8 * g + j0) * HW, HW, ks, pszH, JC, r0 - 3, prow, H, W, pitch);
        float gqa[JC], gka[JC];
#pragma unroll
        for (int jj = 0; jj < JC; ++jj) gqa[jj] = gka[jj] = 0.f;
#pragma unroll 1
        for (int i = 0; i < 7; ++i) {
            l7_stage<T, V>(glp + (int64_t)7 * i * HW, HW, lc, pszR, 7, r0, TR, H, W, pitch);
            l7_stage<T, V>(glp + (int64_t)7 * i * HW, HW, ls, pszR, 7, r0 - (i - 3), TR, H, W, pitch);
            __syncthreads();
            float gc[7];
#pragma unroll
            for (int jx = 0; jx < 7; ++jx) gc[jx] = lc[jx * pszR + lr * pitch + col + 3];
            const float* lw = ls + lr * pitch + col + 6;  // tap (i, jx) comes from pixel (r - dy, c - dx): column c + 3 - dx
#pragma unroll
            for (int jj = 0; jj < JC; ++jj) {
                const float* kw = ks + jj * pszH + (lr + i) * pitch + col;
                const float* pw = ps + (j0 + jj) * L7_T + 7 * i;
                const float* qw = qs + jj * pszH + (lr + 6 - i) * pitch + col + 6;
#pragma unroll
                for (int jx = 0; jx < 7; ++jx) {
                    gqa[jj] += gc[jx] * (kw[jx] + pw[jx]);
                    gka[jj] += lw[jx * pszR - jx] * qw[-jx];
                }
            }
            if (part < parts) {
                const float* lp = lc + ojx * pszR + 3;
                const float* qp = qs + ojj * pszH + 3 * pitch + 3;
                float s = 0.f;
                for (int r = 0; r < rows; ++r)
                    for (int c = part; c < W; c += parts) s += lp[r * pitch + c] * qp[r * pitch + c];
                red[part * OUTS + o] = s;
            }
            __syncthreads();  // red complete; every lane is done with this window row's gL
            if ((int)threadIdx.x < OUTS) {
                float s = 0.f;
                for (int w = 0; w < parts; ++w) s += red[w * OUTS + o];
                part_out[(j0 + ojj) * L7_T + 7 * i + ojx] = s;
            }
            // (the next red is written only after the next window row's barrier, which these reads precede)
        }
        if (valid) {
#pragma unroll
            for (int jj = 0; jj < JC; ++jj) {
                gq[img + (int64_t)(8 * g + j0 + jj) * HW + p] = (T)gqa[jj];
                gk[img + (int64_t)(8 * g + j0 + jj) * HW + p] = (T)gka[jj];
            }
        }
    }
}

// one workgroup per (g, j*49 + t): strided sums over the N * tiles partial rows, then a fixed LDS tree
__global__ __launch_bounds__(L7_THREADS) void lr7_gpos_reduce(const float* __restrict__ partials, float* __restrict__ gpos,
                                                               int rows) {
    __shared__ float sh[L7_THREADS];
    const int g = blockIdx.x / L7_POS, jt = blockIdx.x - g * L7_POS;
    const float* src = partials + (int64_t)g * rows * L7_POS + jt;
    float s = 0.f;
    for (int r = threadIdx.x; r < rows; r += L7_THREADS) s += src[(int64_t)r * L7_POS];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = L7_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) gpos[blockIdx.x] = sh[0];  // (c = 8g + j: gpos[c * 49 + t] = gpos[g * 392 + j * 49 + t])
}

static inline int lr7_vec(int W) { return W % 4 == 0 ? 4 : (W % 2 == 0 ? 2 : 1); }

static size_t lr7_align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool lr7_covers(const cot_agg_geom& g) {
    if (!(g.kh == 7 && g.kw == 7 && g.sh == 1 && g.sw == 1 && g.ph == 3 && g.pw == 3 && g.dh == 1 && g.dw == 1 && g.heads == 1 &&
          g.C % 8 == 0 && g.wC * 8 == g.C))
        return false;
    const Lr7Plan p = lr7_plan(g.H, g.W);
    return p.ok && (int64_t)g.N * g.wC * p.tiles < (1LL << 31);
}

// [glogits: N G 49 HW elements, 256-byte aligned][partials: G N tiles 392 floats]
int64_t lr7_workspace_bytes(const cot_agg_geom& g, size_t esize) {
    const Lr7Plan p = lr7_plan(g.H, g.W);
    return (int64_t)(lr7_align256((size_t)g.N * g.wC * L7_T * g.H * g.W * esize) + (size_t)g.wC * g.N * p.tiles * L7_POS * sizeof(float));
}

template <typename T>
int lr7_forward(const T* q, const T* k, const T* v, const float* pos, T* out, T* probs, const cot_agg_geom& g, hipStream_t s) {
    const Lr7Plan p = lr7_plan(g.H, g.W);
    const int G = g.wC;
    const dim3 grid((unsigned)((int64_t)g.N * G * p.tiles)), block(p.nthreads);
    switch (lr7_vec(g.W)) {
        case 4: COT_LAUNCH((lr7_fwd<T, 4>), grid, block, p.lds_fwd, s, q, k, v, pos, out, probs, g.C, G, g.H, g.W, p.TR, p.tiles); break;
        case 2: COT_LAUNCH((lr7_fwd<T, 2>), grid, block, p.lds_fwd, s, q, k, v, pos, out, probs, g.C, G, g.H, g.W, p.TR, p.tiles); break;
        default: COT_LAUNCH((lr7_fwd<T, 1>), grid, block, p.lds_fwd, s, q, k, v, pos, out, probs, g.C, G, g.H, g.W, p.TR, p.tiles);
    }
    g_lr7_kernel = "lr7_fwd";
    return check_launch(g_lr7_kernel);
}

#define LR7_BY_VEC_JC(KERNEL, ...)                                                                                      \
    do {                                                                                                                \
        const int vec = lr7_vec(g.W);                                                                                   \
        if (p.JC == 8) {                                                                                                \
            if (vec == 4) COT_LAUNCH((KERNEL<T, 4, 8>), grid, block, p.lds_bwd, s, __VA_ARGS__);                        \
            else if (vec == 2) COT_LAUNCH((KERNEL<T, 2, 8>), grid, block, p.lds_bwd, s, __VA_ARGS__);                   \
            else COT_LAUNCH((KERNEL<T, 1, 8>), grid, block, p.lds_bwd, s, __VA_ARGS__);                                 \
        } else {                                                                                                        \
            if (vec == 4) COT_LAUNCH((KERNEL<T, 4, 4>), grid, block, p.lds_bwd, s, __VA_ARGS__);                        \
            else if (vec == 2) COT_LAUNCH((KERNEL<T, 2, 4>), grid, block, p.lds_bwd, s, __VA_ARGS__);                   \
            else COT_LAUNCH((KERNEL<T, 1, 4>), grid, block, p.lds_bwd, s, __VA_ARGS__);                                 \
        }                                                                                                               \
    } while (0)

template <typename T>
int lr7_backward(const T* gout, const T* q, const T* k, const T* v, const float* pos, const T* probs, T* gq, T* gk, T* gv,
                 float* gpos, void* workspace, const cot_agg_geom& g, hipStream_t s) {
    const Lr7Plan p = lr7_plan(g.H, g.W);
    const int G = g.wC;
    const int64_t HW = (int64_t)g.H * g.W;
    T* gl = reinterpret_cast<T*>(workspace);
    float* partials = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + lr7_align256((size_t)g.N * G * L7_T * HW * sizeof(T)));
    const dim3 grid((unsigned)((int64_t)g.N * G * p.tiles)), block(p.nthreads);
    int rc;
    // (a) gv and gL
    LR7_BY_VEC_JC(lr7_bwd_agg, gout, v, probs, gv, gl, g.C, G, g.H, g.W, p.TR, p.tiles);
    if ((rc = check_launch("lr7_bwd_agg"))) return rc;
    // (b) gq, gk and the per-workgroup gpos partials
    LR7_BY_VEC_JC(lr7_bwd_rel, gl, q, k, pos, gq, gk, partials, g.N, g.C, G, g.H, g.W, p.TR, p.tiles);
    if ((rc = check_launch("lr7_bwd_rel"))) return rc;
    // (c) gpos[C][49]
    COT_LAUNCH(lr7_gpos_reduce, dim3((unsigned)(G * L7_POS)), dim3(L7_THREADS), 0, s, partials, gpos, g.N * p.tiles);
    g_lr7_kernel = "lr7_bwd_agg+lr7_bwd_rel+lr7_gpos_reduce";
    return check_launch("lr7_gpos_reduce");
}

#define LR7_INSTANTIATE(T)                                                                                                   \
    template int lr7_forward<T>(const T*, const T*, const T*, const float*, T*, T*, const cot_agg_geom&, hipStream_t);       \
    template int lr7_backward<T>(const T*, const T*, const T*, const T*, const float*, const T*, T*, T*, T*, float*, void*,  \
                                 const cot_agg_geom&, hipStream_t);
LR7_INSTANTIATE(float)
LR7_INSTANTIATE(bf16_t)

}  // namespace cot
