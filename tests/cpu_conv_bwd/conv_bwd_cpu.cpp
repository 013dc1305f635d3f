// C entry points over the weight-gradient part of thesis_clip_nerf_amd/csrc/mvnerf_conv.h for tests/test_conv3x3_bwd_cpu.py.
#include "../../thesis_clip_nerf_amd/csrc/mvnerf_conv.h"

extern "C" {

int conv_bwd_cpu_slab_pixels() { return mvnerf::kWgradSlabPixels; }

long conv_bwd_cpu_tiles(int N, int h, int w) { return mvnerf::conv_wgrad_tiles(N, h, w); }

long conv_bwd_cpu_slabs(int N, int h, int w) { return mvnerf::conv_wgrad_slabs(N, h, w); }

void conv_bwd_cpu_act(const float* x, long n, int act, float* out) {
    for (long i = 0; i < n; ++i) out[i] = mvnerf::conv_act_f(x[i], act);
}

void conv_bwd_cpu_cut_x(const float* x, long n, int act_in, int ex, uint16_t* b0, uint16_t* b1) {
    for (long i = 0; i < n; ++i) mvnerf::conv_wgrad_cut_x(x[i], act_in, ex, b0[i], b1[i]);
}

void conv_bwd_cpu_cut_g(const float* g, long n, int eg, uint16_t* a0, uint16_t* a1, uint16_t* a0s) {
    for (long i = 0; i < n; ++i) mvnerf::conv_wgrad_cut_g(g[i], eg, a0[i], a1[i], a0s[i]);
}

float conv_bwd_cpu_finish(double sum, float amax_x, float amax_g) { return mvnerf::conv_wgrad_finish(sum, amax_x, amax_g); }

float conv_bwd_cpu_dbias_finish(double sum, float amax_x, float amax_g) { return mvnerf::conv_dbias_finish(sum, amax_x, amax_g); }

}  // extern "C"
