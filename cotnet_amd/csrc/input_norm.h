// input_norm.h -- the per-pixel arithmetic of the on-device input pipeline, shared by cot_input_normalize (input_norm.hip) and
// cot_mix_normalize (mix_loss.hip) so that a mixed and an unmixed batch are normalised by ONE definition, bit for bit.
// Arithmetic = the reference's, operation by operation: fp32: IEEE subtract, then IEEE divide (no reciprocal, no FMA
// contraction) -> bit-identical to torch; fp16 (reference `fp16=True`): every intermediate rounded to half as torch's
// half kernels do (fp32 holds a half product / quotient exactly enough that the double rounding is innocuous);
// bf16 (extension for the bf16 model): computed in fp32, rounded once.
#pragma once
#include "cot_common.h"

namespace cot {

template <typename T> __device__ __forceinline__ T norm_one(uint8_t u, float m, float s) {
#pragma clang fp contract(off)
    const float d = (float)u - m;
    return (T)(d / s);
}
template <> __device__ __forceinline__ f16_t norm_one<f16_t>(uint8_t u, float m, float s) {
#pragma clang fp contract(off)
    const f16_t d = (f16_t)((float)u - m);  // m, s are already half-representable (the host rounds them as the reference does)
    return (f16_t)((float)d / s);
}

}  // namespace cot
