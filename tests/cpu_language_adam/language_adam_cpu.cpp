// C entry points over thesis_clip_nerf_amd/csrc/mvnerf_adam.h for tests/test_language_adam_cpu.py (arrays in, arrays out): the rate, the
// per-element update over an array, and the segment map of the flat gradient layout - the source language_opt.hip compiles for the device.
#include "../../thesis_clip_nerf_amd/csrc/mvnerf_adam.h"

using namespace mvnerf::adam;

extern "C" {

float adam_cpu_rate(float lr, float beta1, float beta2, long long t) { return adam_rate(lr, beta1, beta2, t); }

double adam_cpu_power(double beta, long long t) { return power(beta, t); }

// in place on p, m, v
void adam_cpu_update(float* p, const float* g, float* m, float* v, long n, float lr_t, float beta1, float beta2, float eps, float clip) {
    for (long i = 0; i < n; ++i) adam_one(p + i, g[i], m + i, v + i, lr_t, beta1, beta2, eps, clip);
}

int adam_cpu_entries() { return kFlatEntries; }
int adam_cpu_segment_count() { return kSegments; }
long adam_cpu_head_stack() { return kHeadStack; }

// entry e of the layout table: its name, offset and size at n5, variable and number of parts
const char* adam_cpu_entry(int n5, int e, long* offset, long* floats, int* var, int* parts) {
    long at[kFlatEntries + 1];
    flat_offsets(n5, at);
    *offset = at[e];
    *floats = at[e + 1] - at[e];
    *var = kFlat[e].var;
    *parts = kFlat[e].parts;
    return kFlat[e].name;
}

// begin (kSegments + 1), var, part (kSegments)
void adam_cpu_segments(int n5, long* begin, int* var, int* part) { flat_segments(n5, begin, var, part); }

}  // extern "C"
