// Scalar arithmetic of the activation gate (act_gate.hip): the gradient of out = act(y) * mul with respect to y, formed
// from what the forward kept - `out` and `mul` - and nothing else.  Plain scalar code for host and device: tests/cpu_act_gate builds
// this file with the host compiler and compares it bit for bit with the NumPy restatement of tests/fusion_bwd_ref.py.
//
//   d = g * mul * act'(y)
//     act(y) > 0                 d = g * mul                         (relu' = elu' = 1)
//     else, relu                 d = 0
//     else, elu (alpha 1)        d = g * (out + mul)                 (elu'(y) = elu(y) + 1, so mul * elu'(y) = out + mul)
//     identity                   d = g * mul
//
// "act(y) > 0" is read from the SIGNS of out and mul - out > 0 with mul > 0, or out < 0 with mul < 0 - never from the product out * mul,
// which underflows to zero for small factors.  An `out` of zero counts as "not positive": for relu that is act(y) == 0 (or a product
// that underflowed, where the gradient is below the smallest float times g as well), for elu out + mul == mul is the right factor at
// y == 0 and where act(y) * mul underflowed.  mul == 0 gives an exact +0, whatever g holds.  No division, one rounding per operation.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MVG_HD __host__ __device__ inline
#else
#define MVG_HD inline
#endif

namespace mvnerf {

constexpr int kActGateIdentity = 0, kActGateRelu = 1, kActGateElu = 2;

// mul: the factor of this element's (image, channel); 1 where the forward had none
MVG_HD float act_gate_one(float g, float out, float mul, int act) {
    if (mul == 0.0f) return 0.0f;
    const bool positive = (out > 0.0f && mul > 0.0f) || (out < 0.0f && mul < 0.0f);
    if (act == kActGateIdentity || positive) return g * mul;
    if (act == kActGateRelu) return 0.0f;
    const float slope = out + mul;
    return g * slope;
}

}  // namespace mvnerf
