// C entry points over thesis_clip_nerf_amd/csrc/mvnerf_conv.h for tests/test_conv3x3_cpu.py (arrays in, arrays out).
#include "../../thesis_clip_nerf_amd/csrc/mvnerf_conv.h"

extern "C" {

int conv_cpu_scale_exp(float amax) { return mvnerf::conv_scale_exp(amax); }

int conv_cpu_amax_finite(float amax) { return mvnerf::conv_amax_finite(amax) ? 1 : 0; }

void conv_cpu_cut_weight(const float* w, long n, int ew, uint16_t* a0, uint16_t* a1, uint16_t* a0s) {
    for (long i = 0; i < n; ++i) mvnerf::conv_cut_weight(w[i], ew, a0[i], a1[i], a0s[i]);
}

void conv_cpu_cut_act(const float* x, long n, int ex, uint16_t* b0, uint16_t* b1) {
    for (long i = 0; i < n; ++i) mvnerf::conv_cut_act(x[i], ex, b0[i], b1[i]);
}

void conv_cpu_rn16(const float* x, long n, uint16_t* h, float* back) {
    for (long i = 0; i < n; ++i) {
        h[i] = mvnerf::conv_rn16(x[i]);
        back[i] = mvnerf::conv_f16_f32(h[i]);
    }
}

}  // extern "C"
