// C entry points over thesis_clip_nerf_amd/csrc/mvnerf_vit.h for tests/test_vit_cpu.py (arrays in, arrays out).  The LayerNormalization
// walks a row in the kernel's order (csrc/token_linear.hip): 64 lanes, lane l owns the quads l, l + 64, ... and adds their elements in
// order, then an xor butterfly over the lanes.
#include "../../thesis_clip_nerf_amd/csrc/mvnerf_vit.h"

using namespace mvnerf;

namespace {

template <class Term>
float row_sum(const float* row, int C, Term term) {
    float lane[kVitLnLanes];
    for (int l = 0; l < kVitLnLanes; ++l) lane[l] = vit_ln_lane_sum(row, C, l, term);
    for (int mask = 1; mask < kVitLnLanes; mask <<= 1) {
        float next[kVitLnLanes];
        for (int l = 0; l < kVitLnLanes; ++l) next[l] = lane[l] + lane[l ^ mask];
        for (int l = 0; l < kVitLnLanes; ++l) lane[l] = next[l];
    }
    return lane[0];
}

}  // namespace

extern "C" {

int vit_cpu_scale_exp(float amax) { return conv_scale_exp(amax); }

void vit_cpu_cut_act(const float* x, long n, int ex, uint16_t* b0, uint16_t* b1) {
    for (long i = 0; i < n; ++i) conv_cut_act(x[i], ex, b0[i], b1[i]);
}

void vit_cpu_cut_weight(const float* w, long n, int ew, uint16_t* a0, uint16_t* a1, uint16_t* a0s) {
    for (long i = 0; i < n; ++i) conv_cut_weight(w[i], ew, a0[i], a1[i], a0s[i]);
}

void vit_cpu_gelu(const float* x, long n, float* out) {
    for (long i = 0; i < n; ++i) out[i] = vit_gelu(x[i]);
}

// sum (rows, N), bias (N) or null, residual (rows, N) or null with epi != 2
void vit_cpu_linear_epi(const float* sum, const float* bias, const float* residual, long rows, int N, int epi, float* out) {
    for (long i = 0; i < rows; ++i)
        for (int c = 0; c < N; ++c)
            out[i * N + c] = vit_linear_epi(sum[i * N + c], bias != nullptr, bias ? bias[c] : 0.0f, epi, residual ? residual[i * N + c] : 0.0f);
}

void vit_cpu_layer_norm(const float* x, const float* gamma, const float* beta, long M, int C, float eps, float* out) {
    for (long i = 0; i < M; ++i) {
        const float* row = x + i * C;
        const float ref = row[0];
        const float mean = vit_ln_mean(ref, row_sum(row, C, [&](float v) { return v - ref; }), C);
        const float rstd = vit_ln_rstd(row_sum(row, C, [&](float v) { return bn_sq_dev(v, mean); }), C, eps);
        for (int c = 0; c < C; ++c) out[i * C + c] = vit_ln_apply(row[c], mean, rstd, gamma[c], beta[c]);
    }
}

// one softmax row: the maximum first, the accurate expf, the sum in order, one quotient per element
void vit_cpu_softmax_row(const float* logits, int n, float* out) {
    float top = logits[0];
    for (int j = 1; j < n; ++j) top = fmaxf(top, logits[j]);
    float total = 0.0f;
    for (int j = 0; j < n; ++j) {
        out[j] = vit_softmax_weight(logits[j], top);
        total = total + out[j];
    }
    for (int j = 0; j < n; ++j) out[j] = out[j] / total;
}

}  // extern "C"
