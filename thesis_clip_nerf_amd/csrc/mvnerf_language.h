// Per-row scalar math of the losses of LanguageNeRF.train_step (src/lib/lmvnerf/model_v4.py:277-318; the losses train_language.py:40-63
// selects), usable from device code (hipcc, language_ops.hip) and from a host build (gcc, tests/cpu_language) so the same source is checked
// on the CPU.
//
//   landscape_row   one batch element of the landscape loss and its derivative w.r.t. the predicted success (np logits):
//                     kl_divergence  (model_v4.py:283-285 with softmax_before_loss; tf.keras.losses.KLDivergence(reduction=NONE)):
//                                    s = softmax(y); p = clip(s, 1e-7, 1); t = clip(label, 1e-7, 1); loss = sum t log(t / p).
//                                    The clip passes a derivative inside [1e-7, 1] only; the softmax Jacobian s_k (g_k - sum_j g_j s_j) follows.
//                     cross_entropy  (tf.keras.losses.CategoricalCrossentropy(from_logits=True), train_language.py:56-57):
//                                    loss = -sum label log_softmax(y); derivative s_k sum(label) - label_k.  The mean over the batch is
//                                    the caller's.
//   cosine_row      tf.keras.losses.CosineSimilarity(axis=-1) of one row (model_v4.py:300-314): u(l) . u(x) with u(x) = x rsqrt(max(sum x^2,
//                   1e-12)), and its derivative w.r.t. x: (u(l) - u(x) (u(l) . u(x))) / |x| above the clamp, u(l) 1e6 below it (the clamp
//                   passes no derivative there).  The negated mean over the rows is the caller's.
//
// Arithmetic: as mvnerf_pose.h - compiled with -ffp-contract=off, sums in the order written.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define MVL_HD __host__ __device__ __forceinline__
#else
#define MVL_HD static inline
#endif

namespace mvnerf {
namespace language {

constexpr int kLossKL = 0;
constexpr int kLossCrossEntropy = 1;
constexpr float kClipLo = 1e-7f;
constexpr float kCosClamp = 1e-12f;

MVL_HD float clip01(float v) { return fminf(fmaxf(v, kClipLo), 1.0f); }

// y, label: np floats -> the row's loss; g (np floats, write-only: the softmax is formed again where it is needed, so that nothing
// waits for a store) = d loss / d y
MVL_HD float landscape_row(int kind, const float* y, const float* label, int np, float* g) {
    float m = y[0];
    for (int j = 1; j < np; ++j) m = fmaxf(m, y[j]);
    float z = 0.0f;
    for (int j = 0; j < np; ++j) z += expf(y[j] - m);
    float loss = 0.0f;
    if (kind == kLossKL) {
        float dot = 0.0f;                                  // sum_j (d loss / d s_j) s_j
        for (int j = 0; j < np; ++j) {
            const float s = expf(y[j] - m) / z;
            const float p = clip01(s), t = clip01(label[j]);
            loss += t * logf(t / p);
            const float gp = (s >= kClipLo && s <= 1.0f) ? -(t / p) : 0.0f;
            dot += gp * s;
        }
        for (int j = 0; j < np; ++j) {
            const float s = expf(y[j] - m) / z;
            const float p = clip01(s), t = clip01(label[j]);
            const float gp = (s >= kClipLo && s <= 1.0f) ? -(t / p) : 0.0f;
            g[j] = s * (gp - dot);
        }
    } else {
        const float lz = logf(z);
        float tsum = 0.0f;
        for (int j = 0; j < np; ++j) {
            loss -= label[j] * ((y[j] - m) - lz);
            tsum += label[j];
        }
        for (int j = 0; j < np; ++j) g[j] = (expf(y[j] - m) / z) * tsum - label[j];
    }
    return loss;
}

// x, l: d floats (d <= 4) -> u(l) . u(x); g (d floats) = its derivative w.r.t. x
MVL_HD float cosine_row(const float* x, const float* l, int d, float* g) {
    float ssx = 0.0f, ssl = 0.0f;
    for (int i = 0; i < d; ++i) {
        ssx += x[i] * x[i];
        ssl += l[i] * l[i];
    }
    const float nx = 1.0f / sqrtf(fmaxf(ssx, kCosClamp)), nl = 1.0f / sqrtf(fmaxf(ssl, kCosClamp));
    float cosv = 0.0f;
    for (int i = 0; i < d; ++i) cosv += (l[i] * nl) * (x[i] * nx);
    const bool above = ssx >= kCosClamp;
    for (int i = 0; i < d; ++i) {
        const float ul = l[i] * nl;
        g[i] = above ? nx * (ul - (x[i] * nx) * cosv) : ul * nx;
    }
    return cosv;
}

}  // namespace language
}  // namespace mvnerf
