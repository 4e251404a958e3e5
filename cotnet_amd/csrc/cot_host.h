// cot_host.h -- the host-side interface between the .hip files: every launcher, coverage predicate, workspace-size function,
// last-kernel getter and tuning global that one file defines and another (mostly cot_abi.hip) uses.  Every file includes it, so each
// definition is compiled against its declaration; default arguments are stated here only.  What a tuning global means is told at its
// definition; which cot_set_tuning key sets it, in the table of cot_abi.hip.
#pragma once
#include "cot_common.h"

namespace cot {

// ---- cot_abi.hip
extern unsigned long long* g_debug_stamps;  // DIAGNOSTIC: see cot_debug_stamps

// ---- agg_nchw.hip: aggregation, NCHW (fused softmax / GroupNorm-9 / row-statistics forms included)
const char* last_kernel_nchw();
extern int g_tune[9];
int xchg_mode();
template <typename T> int agg_forward_nchw(const T* x, const T* w, T* out, const cot_agg_geom& g, int Ho, int Wo, hipStream_t s, const char* tname);
template <typename T>
int agg_backward_nchw(const T* gout, const T* x, const T* w, T* gx, T* gw, const cot_agg_geom& g, int Ho, int Wo, hipStream_t s);
int agg_gn9_forward_nchw(const bf16_t* x, const bf16_t* logits, const float* mean, const float* rstd, const bf16_t* gamma, const bf16_t* beta,
                         int gimg, bf16_t* out, const cot_agg_geom& g, hipStream_t s);
int agg_forward_rowstats_nchw(const bf16_t* x, const bf16_t* w, bf16_t* out, float* rowstats, const float* mean, const float* rstd,
                              const bf16_t* gamma, const bf16_t* beta, int gimg, const cot_agg_geom& g, hipStream_t s);
template <typename T> int agg_softmax_forward_nchw(const T* x, const T* logits, T* out, T* probs, const cot_agg_geom& g, hipStream_t s);
template <typename T>
int agg_softmax_backward_nchw(const T* gout, const T* x, const T* probs, T* gx, T* glogits, const cot_agg_geom& g, hipStream_t s);

// ---- agg_dot2.hip: packed-bf16 dot-product backward of the 3x3 aggregation; -1 = geometry not covered
int agg_backward_nchw_dot2(const bf16_t* gout, const bf16_t* x, const bf16_t* w, bf16_t* gx, bf16_t* gw, const cot_agg_geom& g, hipStream_t s);
extern int g_dot2[6];
int agg_gn9_backward_nchw_dot2(const bf16_t* gout, const bf16_t* x, const bf16_t* logits, const float* mean, const float* rstd, const bf16_t* gamma,
                               const bf16_t* beta, int gimg, bf16_t* gx, bf16_t* gw, const cot_agg_geom& g, hipStream_t s);

// ---- agg_nhwc.hip: aggregation, channels-last
const char* last_kernel_nhwc();
template <typename T> int agg_forward_nhwc(const T* x, const T* w, T* out, const cot_agg_geom& g, int Ho, int Wo, int max_vec, hipStream_t s);
template <typename T>
int agg_backward_nhwc(const T* gout, const T* x, const T* w, T* gx, T* gw, const cot_agg_geom& g, int Ho, int Wo, int max_vec, hipStream_t s);

// ---- agg_mix.hip: 3x3 + 5x5 mixed aggregation
extern int g_mix_tune[3];
const char* last_kernel_mix();
template <typename T>
int aggmix_forward(const T* x, const T* w1, const T* w2, T* out, const cot_agg_geom& g, int p2h, int p2w, int Ho, int Wo, hipStream_t s);
template <typename T>
int aggmix_backward_input(const T* gout, const T* w1, const T* w2, T* gx, const cot_agg_geom& g, int p2h, int p2w, int all_heads, int Ho, int Wo,
                          hipStream_t s);
template <typename T>
int aggmix_backward_weight(const T* gout, const T* x, T* gw1, T* gw2, const cot_agg_geom& g, int p2h, int p2w, int Ho, int Wo, hipStream_t s);

// ---- optim.hip: SGD / EMA over flat buffers
int ema_flat(void* ema, const void* src, int64_t n, float decay, int src_dtype, hipStream_t s);
int sgd_flat(void* param, void* master, void* mom, const void* grad, int64_t n, float lr, float momentum, float wd, float gscale, int nesterov,
             int param_dtype, int grad_dtype, hipStream_t s);
int sgd_flat_lr(void* param, void* master, void* mom, const void* grad, int64_t n, const float* lr_dev, float momentum, float wd, float gscale,
                int nesterov, int param_dtype, int grad_dtype, hipStream_t s);
int sgd_flat_clip(void* param, void* master, void* mom, const void* grad, int64_t n, float lr, const float* lr_dev, const cot_clip_state* clip,
                  float momentum, float wd, float gscale, int nesterov, int param_dtype, int grad_dtype, hipStream_t s);

// ---- adamw.hip: Adam / AdamW over flat buffers behind one step count in device memory (arguments validated by cot_abi.hip)
int adam_tick(void* adam_state, const void* clip_state, double beta1, double beta2, hipStream_t s);
int adamw_flat(void* param, void* master, void* exp_avg, void* exp_avg_sq, const void* grad, int64_t n, float lr, const float* lr_dev,
               const cot_adam_state* st, const cot_clip_state* clip, double beta1, double beta2, float eps, float wd, float gscale, int decoupled,
               int param_dtype, int grad_dtype, hipStream_t s);

// ---- lookahead.hip: Lookahead's slow weights over flat buffers behind one decision in device memory (arguments validated by cot_abi.hip)
int lookahead_tick(void* state, const void* clip_state, int k, int force, hipStream_t s);
int lookahead_flat(void* param, void* master, void* slow, int64_t n, double alpha, const cot_lookahead_state* st, int param_dtype,
                   hipStream_t s);

// ---- grad_clip.hip: the gradients' global norm -> clip coefficient / skip flag in a block in device memory (read by sgd_flat_clip)
int grad_sumsq(const void* grad, int64_t n, int grad_dtype, float* partials, hipStream_t s);
int grad_clip_finish(const float* partials, int64_t nparts, float max_norm, void* state, hipStream_t s);

// ---- agc.hip: adaptive gradient clipping, one wave per unit of a flat bucket (arguments validated by cot_agc_clip)
int agc_clip(void* grad, const float* weight, const int64_t* units, int64_t nunits, float clip_factor, float eps, float* coef, int grad_dtype,
             hipStream_t s);

// ---- bn_act.hip: BatchNorm (+ activation, residual); `mask`: ReLU sign mask or NULL; -2 / -3 = geometry not covered / kernel takes no mask
extern int g_bn_fold, g_bn_grid_cap, g_bn_split_target, g_bn_small_m, g_bn_chan, g_bn_chan7, g_bn_chan_rr;
int64_t bn_relu_mask_bytes(int N, int C, int HW, int esize);
int bn_workspace_floats(int N, int C);
template <typename T>
int bn_act_inference(const void* x, const void* res, void* y, const float* gamma, const float* beta, const float* rmean, const float* rvar, int N,
                     int C, int HW, float eps, int act, hipStream_t s);
template <typename T>
int bn_act_forward(const void* x, const void* res, void* y, const float* gamma, const float* beta, float* mean, float* rstd, float* rmean,
                   float* rvar, long long* nbt, float* ws, int N, int C, int HW, float eps, float mom, int act, const float* ps, uint8_t* mask,
                   hipStream_t s);
template <typename T>
int bn_act_backward(const void* dy, const void* x, const void* y, void* dx, void* dres, const float* gamma, const float* beta, const float* mean,
                    const float* rstd, float* dgamma, float* dbeta, float* ws, int N, int C, int HW, int act, const float* ps,
                    const uint8_t* mask, hipStream_t s);
template <typename T>
int bn_batch_stats(const void* x, float* mean, float* rstd, float* rmean, float* rvar, long long* nbt, float* ws, int N, int C, int HW, float eps,
                   float mom, hipStream_t s);
int bn_stats_split(int N, int C);
template <typename T> int bn_stats_sums_launch(const void* x, float* ws, int N, int C, int HW, hipStream_t s);
int bn_tile_stats(const float* part, int N, int C, int HW, float eps, float mom, float* mean, float* rstd, float* rmean, float* rvar, long long* nbt,
                  hipStream_t s);
int bn_rowstats(const float* rows, int N, int C, int H, int W, float eps, float mom, float* mean, float* rstd, float* rmean, float* rvar,
                long long* nbt, hipStream_t s);
int bn_apply_forward(const void* x, const void* res, void* y, const float* gamma, const float* beta, const float* mean, const float* rstd, int N,
                     int C, int HW, int act, uint8_t* mask, hipStream_t s);
int bn_act_lay_covers(int N, int C, int HW);
int bn_act_forward_lay(const void* x, const void* res, void* y, void* y2, const float* gamma, const float* beta, float* mean, float* rstd,
                       float* rmean, float* rvar, long long* nbt, int N, int C, int HW, float eps, float mom, int act, const float* ps, int lay,
                       hipStream_t s);
int bn_act_backward_lay(const void* dy, const void* dy2, const void* x, const void* y, void* dx, void* dres, const float* gamma, const float* beta,
                        const float* mean, const float* rstd, float* dgamma, float* dbeta, int N, int C, int HW, int act, const float* ps, int lay,
                        hipStream_t s);

// ---- radix_tail.hip: radix-2 split-attention tail and SE gate
extern int g_radix_pack7;
template <typename T> int radix_gap(const void* y, const void* k, void* gap, int64_t planes, int HW, hipStream_t s);
template <typename T> int radix_mix(const void* y, const void* k, const void* attn, void* out, int64_t planes, int HW, hipStream_t s);
template <typename T>
int radix_mix_bwd(const void* g, const void* y, const void* k, const void* attn, void* gy, void* gk, void* gattn, int64_t planes, int HW,
                  hipStream_t s);
template <typename T> int se_gap(const void* x, void* gap, int64_t planes, int HW, hipStream_t s);
template <typename T> int se_gate(const void* x, const void* logit, void* out, int64_t planes, int HW, hipStream_t s);
template <typename T> int se_gate_bwd(const void* g, const void* x, const void* logit, void* gx, void* glogit, int64_t planes, int HW, hipStream_t s);
template <typename T> int radix_gap_t(const void* y, const void* k, void* gapT, int N, int C, int HW, int lay, hipStream_t s);
template <typename T>
int radix_mix_logits(const void* y, const void* k, const void* logitsT, void* out, void* attn, int N, int C, int HW, int lay, hipStream_t s);
template <typename T>
int radix_mix_bwd_reduce(const void* g, const void* y, const void* k, const void* attn, void* glogitsT, int N, int C, int HW, int lay, hipStream_t s);
template <typename T>
int radix_mix_bwd_apply(const void* g, const void* attn, const void* ggapT, void* gy, void* gk, int N, int C, int HW, int lay, hipStream_t s);
template <typename T>
int radix_gap_t_bn(const void* a, const void* k, void* gapT, const float* gamma, const float* beta, float* mean, float* rstd, float* rmean,
                   float* rvar, long long* nbt, const float* part, int split, float eps, float mom, int N, int C, int HW, int lay, hipStream_t s);
template <typename T>
int radix_mix_logits_bn(const void* a, const void* k, const void* logitsT, void* out, void* attn, const float* gamma, const float* beta,
                        const float* mean, const float* rstd, int N, int C, int HW, int lay, hipStream_t s);
template <typename T>
int radix_mix_bwd_reduce_bn(const void* g, const void* a, const void* k, const void* attn, void* glogitsT, float* tsum, const float* gamma,
                            const float* beta, const float* mean, const float* rstd, int N, int C, int HW, int lay, hipStream_t s);
template <typename T>
int radix_mix_bwd_apply_bn(const void* g, const void* a, const void* attn, const void* ggapT, const float* tsum, void* ga, void* gk,
                           const float* gamma, const float* beta, const float* mean, const float* rstd, float* dgamma, float* dbeta, int N, int C,
                           int HW, int lay, hipStream_t s);

// ---- conv1x1.hip: first-generation 1x1 convolution kernels and the partial-sum reduce every weight gradient ends with
extern int g_conv1x1_tune[4], g_wgrad_cap_pct;
int conv1x1_wgrad_reduce_launch(const float* part, int S, int M, int J, int has_bias, void* gw, void* gb, hipStream_t stream);
int conv1x1_gemm(const void* x1, const void* x2, int k1, const void* A, const void* bias, void* y1, void* y2, int m1, int N, int K, int M, int HW,
                 int accumulate, int transposed_a, hipStream_t stream);
int conv1x1_wgrad_splits(int N, int M, int J, int HW, int has_bias);
int conv1x1_wgrad(const void* gy, const void* x1, const void* x2, int k1, void* gw, void* gb, float* workspace, int N, int J, int M, int HW,
                  hipStream_t stream);

// ---- conv3x3g.hip: first-generation grouped 3x3 convolution
int64_t conv3x3g_masks_bytes(int H, int W);
int conv3x3g_masks(void* masks, int H, int W, hipStream_t stream);
int conv3x3g_gemm(const void* x, const void* w, void* y, const void* masks, int N, int Cin, int Cout, int G, int H, int W, int mode, int accumulate,
                  hipStream_t stream);
int conv3x3g_wgrad_splits(int N, int Cin, int Cout, int G, int HW);
int conv3x3g_wgrad(const void* gy, const void* x, void* gw, const void* masks, float* ws, int N, int Cin, int Cout, int G, int H, int W,
                   hipStream_t stream);

// ---- group_norm9.hip: GroupNorm, 9 channels per group (gn9f_*: fp32)
extern int g_gn9_pack;
int gn9f_forward(const void* x, const void* gamma, const void* beta, void* y, float* mean, float* rstd, int N, int C, int HW, float eps,
                 hipStream_t stream);
int gn9_stats_finalize(const float* part, float* mean, float* rstd, int N, int C, int HW, float eps, hipStream_t stream);
int gn9_forward(const void* x, const void* gamma, const void* beta, void* y, float* mean, float* rstd, int N, int C, int HW, float eps, int lay,
                hipStream_t stream);
int gn9_backward_params(const float* workspace, void* dgamma, void* dbeta, int N, int C, hipStream_t stream);
int gn9_backward(const void* dy, const void* x, const float* mean, const float* rstd, const void* gamma, void* dx, void* dgamma, void* dbeta,
                 float* workspace, int N, int C, int HW, int lay, hipStream_t stream);
int gn9f_backward(const void* dy, const void* x, const float* mean, const float* rstd, const void* gamma, void* dx, void* dgamma, void* dbeta,
                  float* workspace, int N, int C, int HW, hipStream_t stream);

// ---- pool3x3.hip: poolings and stride-2 subsampling
extern int g_pool_tile;
template <typename T> int subsample2(int bwd, const void* a, void* out, int64_t planes, int H, int W, hipStream_t stream);
template <typename T> int avgpool2x2s2(int bwd, const void* a, void* out, int64_t planes, int H, int W, hipStream_t stream);
template <typename T> int pool3x3s2(int op, const void* a, const void* b, void* out, int64_t planes, int H, int W, hipStream_t stream);

// ---- stem7x7.hip: 7x7 / stride 2 stem, bf16
extern int g_stem_lds;
int stem7x7_splits(int N, int H, int W);
int stem7x7_forward(const void* x, const void* w, void* y, int N, int H, int W, hipStream_t stream);
int stem7x7_wgrad(const void* gy, const void* x, void* gw, float* workspace, int N, int H, int W, hipStream_t stream);

// ---- stem7x7_f32.hip: the same stem in fp32
int stem7x7_f32_forward(const void* x, const void* w, void* y, int N, int H, int W, hipStream_t stream);
int stem7x7_f32_backward_weight(const void* gy, const void* x, void* gw, float* workspace, int S, int N, int H, int W, hipStream_t stream);

// ---- stem3x3.hip: 3x3 / stride 2 stem
int stem3x3s2_splits(int N, int H, int W, int Co);
int stem3x3s2_forward(const void* x, const void* w, void* y, int N, int H, int W, int Co, hipStream_t stream);
int stem3x3s2_wgrad(const void* gy, const void* x, void* gw, float* workspace, int N, int H, int W, int Co, hipStream_t stream);

// ---- input_norm.hip: uint8 images -> normalised tensor
int input_normalize(const void* x, void* y, const float* mean, const float* stdv, int64_t planes, int C, int HW, int dtype, hipStream_t s);

// ---- conv_lds.hip: LDS-tiled 1x1 and grouped 3x3 kernels; -1 = not covered; `pack`: 0 pack and run, 1 pack only, 2 `ws` is packed
extern int g_conv_lds_tune[3], g_wgrad_lds_cap_pct, g_conv3x3_ring, g_conv3x3_res, g_conv3x3_wsingle, g_conv3x3_cols, g_conv3x3_perm;
int transpose_bf16(const void* src, void* dst, int R, int C, int pack, hipStream_t stream);
int conv3x3g_lds_gemm(const void* x, const void* w, void* y, void* ws, int N, int Cin, int Cout, int G, int H, int W, int mode, int accumulate,
                      int pack, hipStream_t stream);
bool conv1x1_wgrad_lds_covers(int N, int HW, int M, int J);
int conv1x1_wgrad_lds_splits(int N, int M, int J, int HW, int has_bias);
int conv1x1_wgrad_lds_run(const void* gy, const void* x1, const void* x2, int k1, void* gw, void* gb, float* workspace, int N, int J, int M, int HW,
                          hipStream_t stream);
bool conv1x1_lds_covers(int K, int k1, bool two_slabs, int HW);
int conv1x1_lds_gemm(const void* x1, const void* x2, int k1, const void* w, int wpacked, const void* bias, void* y1, void* y2, int m1, int N, int K,
                     int M, int HW, int accumulate, hipStream_t stream, int64_t xs = 0, int64_t ys = 0, float* stats = nullptr,
                     const void* acc_src = nullptr, const void* acc_mask = nullptr);

// ---- conv_lds2.hip: third-generation 1x1 forward / data gradient, reached through conv1x1_lds_gemm
extern int g_conv_lds2_tune, g_conv_big_fill, g_conv_big_xswz, g_conv_flat_ns3, g_conv_ablate, g_conv_k_tail;
struct C1LdsArgs;  // conv_lds_common.h
int conv1x1_lds_gemm2(const C1LdsArgs& a0, hipStream_t stream);

// ---- conv_wgrad2.hip: third-generation weight gradients; -1 = geometry not covered
extern int g_wgrad2_tune;
bool conv1x1_wgrad2_covers(int N, int HW, int M, int J, int k1, bool two_slabs);
int conv1x1_wgrad2_splits(int N, int M, int J, int HW, int has_bias);
int conv1x1_wgrad2_run(const void* gy, const void* x1, const void* x2, int k1, void* gw, void* gb, float* workspace, int N, int J, int M, int HW,
                       hipStream_t stream, int sy = 0, int sx = 0);
bool conv3x3g_wgrad2_covers(int N, int Cin, int Cout, int G, int H, int W, int x_guard);
int conv3x3g_wgrad2_splits(int N, int Cin, int Cout, int G, int HW);
int conv3x3g_wgrad2_run(const void* gy, const void* x, void* gw, const void* masks, float* workspace, int N, int Cin, int Cout, int G, int H, int W,
                        int x_guard, hipStream_t stream);

// ---- conv_gen.hip: general grouped convolutions, fp32 or bf16, any channel counts
int convg_forward(const void* x, const void* w, const void* bias, void* y, int N, int Cin, int Cout, int G, int H, int W, int ksize, int accumulate,
                  int dtype, hipStream_t stream);
int convg_backward_data(const void* gy, const void* w, void* gx, int N, int Cin, int Cout, int G, int H, int W, int ksize, int accumulate, int dtype,
                        hipStream_t stream);
int64_t convg_workspace(int N, int Cin, int Cout, int G, int H, int W, int ksize);
int convg_backward_weight(const void* gy, const void* x, void* gw, void* gbias, float* workspace, int N, int Cin, int Cout, int G, int H, int W,
                          int ksize, int dtype, hipStream_t stream);

// ---- conv_tiny.hip: 1x1 convolutions over one image of at most 256 pixels
extern int g_conv_tiny;
bool conv_tiny_covers(int N, int Ci, int Co, int HW);
int conv_tiny_forward(const void* x, const void* w, const void* bias, void* y, int Ci, int Co, int HW, hipStream_t stream);
int conv_tiny_backward_data(const void* gy, const void* w, void* gx, int Ci, int Co, int HW, int accumulate, hipStream_t stream);
int conv_tiny_backward_weight(const void* gy, const void* x, void* gw, void* gb, int Ci, int Co, int HW, hipStream_t stream);

// ---- local_relation.hip: LR-Net's local relation
const char* last_kernel_lr();
bool lr_covers(const cot_agg_geom& g);
int64_t lr_workspace_bytes(const cot_agg_geom& g, size_t esize);
template <typename T> int lr_forward(const T* q, const T* k, const T* v, const float* pos, T* out, T* probs, const cot_agg_geom& g, hipStream_t s);
template <typename T>
int lr_backward(const T* gout, const T* q, const T* k, const T* v, const float* pos, const T* probs, T* gq, T* gk, T* gv, float* gpos,
                void* workspace, const cot_agg_geom& g, hipStream_t s);

// ---- local_relation7.hip: the 7x7 window of the same operation (lr_covers / lr_workspace_bytes / lr_forward / lr_backward route to it)
const char* last_kernel_lr7();
bool lr7_covers(const cot_agg_geom& g);
int64_t lr7_workspace_bytes(const cot_agg_geom& g, size_t esize);
template <typename T> int lr7_forward(const T* q, const T* k, const T* v, const float* pos, T* out, T* probs, const cot_agg_geom& g, hipStream_t s);
template <typename T>
int lr7_backward(const T* gout, const T* q, const T* k, const T* v, const float* pos, const T* probs, T* gq, T* gk, T* gv, float* gpos,
                 void* workspace, const cot_agg_geom& g, hipStream_t s);

// ---- mix_loss.hip: mixup / CutMix input pipeline and soft-target cross entropy
int mix_normalize(const void* x, void* y, const float* mean, const float* stdv, const void* params, int N, int C, int H, int W, int dtype,
                  hipStream_t s);
int soft_ce_forward(const void* logits, const void* labels, const void* params, double smoothing, float* row_loss, float* row_lse, float* mean_loss,
                    int N, int K, int dtype, hipStream_t s);
int soft_ce_backward(const void* logits, const void* labels, const void* params, double smoothing, const float* row_lse, const float* grad_out,
                     void* dlogits, int N, int K, int dtype, hipStream_t s);

// ---- eval_score.hip: top-1 / top-5 / loss of a validation batch, added to an accumulator block in device memory
int eval_score(const void* logits, const void* labels, void* acc, int* row_rank, float* row_nll, int N, int K, int dtype, hipStream_t s);

}  // namespace cot
