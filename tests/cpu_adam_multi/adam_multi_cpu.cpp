// C entry points over thesis_clip_nerf_amd/csrc/mvnerf_adam.h for tests/test_adam_multi_cpu.py: the warm-up schedule, the chunk plan, the
// lookup, and a whole multi-tensor step on host arrays that walks the chunks as a kernel's workgroups would (one chunk, one tensor,
// adam_one per element) - the source a HIP pass would compile for the device.
#include "../../thesis_clip_nerf_amd/csrc/mvnerf_adam.h"

using namespace mvnerf::adam;

extern "C" {

long long multi_cpu_chunk() { return kMultiChunk; }

float multi_cpu_warmup_rate(float target, double warm, double after, long long step) { return warmup_rate(target, warm, after, step); }

long long multi_cpu_plan(const long long* n, int count, long long* first_chunk) { return multi_plan(n, count, first_chunk); }

int multi_cpu_find(const long long* first_chunk, int count, long long chunk) { return multi_find(first_chunk, count, chunk); }

// p, m, v (count pointers each), g (count pointers, NULL: left alone), n (count), first_chunk (count + 1); *step read, then advanced
void multi_cpu_step(float* const* p, const float* const* g, float* const* m, float* const* v, const long long* n, const long long* first_chunk,
                    int count, long long* step, float lr, double warm, double after, float beta1, float beta2, float eps, float clip) {
    const float lr_t = adam_rate(warmup_rate(lr, warm, after, *step), beta1, beta2, *step + 1);
    for (long long chunk = 0; chunk < first_chunk[count]; ++chunk) {
        const int t = multi_find(first_chunk, count, chunk);
        if (!g[t]) continue;
        const long long at = (chunk - first_chunk[t]) * kMultiChunk;
        const long long left = n[t] - at, len = left < kMultiChunk ? left : kMultiChunk;
        for (long long i = at; i < at + len; ++i) adam_one(p[t] + i, g[t][i], m[t] + i, v[t] + i, lr_t, beta1, beta2, eps, clip);
    }
    *step = *step + 1;
}

}  // extern "C"
