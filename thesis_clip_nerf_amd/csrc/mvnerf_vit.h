// Scalar arithmetic of the transformer-block passes (token_linear.hip, attention.hip): the epilogue of the Dense layer,
// the LayerNormalization of one row and the softmax weight.  Plain scalar code for host and device: tests/cpu_vit builds this file with
// the host compiler.  The operand cut, the scale chooser and the three-product rule of the Dense layer are mvnerf_conv.h's, unchanged.
//
//   Dense       y = epi(sum + bias): epi 0 identity, 1 exact-erf gelu, 2 `+ residual`; the bias joins the un-scaled sum first
//   LayerNorm   with ref = the row's first element: mean = ref + (sum_i (x_i - ref)) / C, M2 = sum_i (x_i - mean)^2 about that mean,
//               rstd = 1 / sqrt(M2 / C + eps) (biased variance), out = ((x - mean) * rstd) * gamma + beta.  No raw sum of x or of x^2 is
//               formed: a constant row gives mean == the constant, M2 == 0 and out == beta exactly, and |mean| >> sigma costs nothing.
//               The sums run in the kernel's order (vit_ln_sum): lane l of 64 owns the quads l, l + 64, ... of the row and adds their
//               elements in order, then an xor butterfly over the 64 lanes.
//   softmax     w_j = expf(s_j - max_k s_k), the accurate expf; out = (sum_j w_j v_j) / (sum_j w_j)
#pragma once

#include "mvnerf_conv.h"

namespace mvnerf {

constexpr int kVitEpiBias = 0, kVitEpiGelu = 1, kVitEpiResidual = 2;
constexpr int kVitLnLanes = 64;              // token_linear.hip: one wave per row

// Keras' gelu(approximate=False) = torch's F.gelu: 0.5 x (1 + erf(x / sqrt 2))
MVC_HD float vit_gelu(float x) {
    const float t = x * 0.70710678118654752440f;
    const float e = 1.0f + erff(t);
    const float h = x * 0.5f;
    return h * e;
}

MVC_HD float vit_linear_epi(float sum, bool has_bias, float bias, int epi, float residual) {
    float y = has_bias ? sum + bias : sum;
    if (epi == kVitEpiGelu) y = vit_gelu(y);
    if (epi == kVitEpiResidual) y = y + residual;
    return y;
}

MVC_HD float vit_ln_mean(float ref, float dev_sum, int C) { return ref + dev_sum / (float)C; }

MVC_HD float vit_ln_rstd(float m2, int C, float eps) {
    const float var = m2 / (float)C;
    return 1.0f / sqrtf(var + eps);
}

MVC_HD float vit_ln_apply(float x, float mean, float rstd, float gamma, float beta) {
    float t = x - mean;
    t = t * rstd;
    t = t * gamma;
    return t + beta;
}

// one lane's share of a row sum: term(x_i) over the elements of its quads, in order
template <class Term>
MVC_HD float vit_ln_lane_sum(const float* row, int C, int lane, Term term) {
    float s = 0.0f;
    for (int q = lane; q < C / 4; q += kVitLnLanes)
        for (int e = 0; e < 4; ++e) s = s + term(row[4 * q + e]);
    return s;
}

MVC_HD float vit_softmax_weight(float logit, float row_max) { return expf(logit - row_max); }

}  // namespace mvnerf
