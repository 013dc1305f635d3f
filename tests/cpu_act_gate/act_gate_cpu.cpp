// C entry point over thesis_clip_nerf_amd/csrc/mvnerf_act_gate.h for tests/test_act_gate_cpu.py (arrays in, arrays out), with the
// indexing of csrc/act_gate.hip: one row of mul per image, one value per channel.
#include "../../thesis_clip_nerf_amd/csrc/mvnerf_act_gate.h"

using namespace mvnerf;

extern "C" {

// g, out, d (N, pixels_per_image, C); mul (N, C) or null (= 1); d may be g
void act_gate_cpu(const float* g, const float* out, const float* mul, int act, int N, long pixels_per_image, int C, float* d) {
    for (int n = 0; n < N; ++n)
        for (long p = 0; p < pixels_per_image; ++p)
            for (int c = 0; c < C; ++c) {
                const long i = ((long)n * pixels_per_image + p) * C + c;
                d[i] = act_gate_one(g[i], out[i], mul ? mul[(long)n * C + c] : 1.0f, act);
            }
}

}  // extern "C"
