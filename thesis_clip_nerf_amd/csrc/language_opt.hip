// extern "C" optimiser of the LanguageNeRF training step and the whole step behind one call (include/mvnerf_hip.h):
//
//   mvnerf_language_apply_gradients   clip-by-value + Keras Adam on the 21 read-out variables where they live, one launch over the flat
//                                     index space of `grads`, the rate formed on the device from a step counter, then the counter's bump
//   mvnerf_language_train_step        head gather + mvnerf_language_loss_and_grads + mvnerf_language_apply_gradients
//
// The segment map (flat index -> variable) comes from adam::kFlat (mvnerf_adam.h), the table language_api.hip's layout is made of.  Every
// entry of the layout but the last starts on a multiple of 64 floats, but nothing here relies on it: one float per thread, the segment
// found by comparing against the 21 begin offsets held in the kernel arguments (a chain of selects: no scratch, no indexed argument read).
// The totals are odd (78 529 floats at n5 = 1), so a vector form would need a predicated tail and could not assume that a segment's flat
// offset is 16-byte aligned; at 0.6 - 2.3 MB per moment (n5 = 7, 42) the launch is latency-bound either way.
// No atomics, no allocation, no host synchronisation: the counter is read by every workgroup of the update and written by a one-thread
// launch behind it on the same stream.
#include <hip/hip_runtime.h>

#include "mvnerf_adam.h"
#include "mvnerf_api.h"

namespace {

using mvnerf::aligned4;
using mvnerf::api_fail;
namespace adam = mvnerf::adam;

const char* const kApply = "mvnerf_language_apply_gradients";
const char* const kStep = "mvnerf_language_train_step";

// the 21 variables in flat order: segment s holds the flat indices begin[s] .. begin[s + 1]
struct Segments {
    long begin[adam::kSegments + 1];
    float* ptr[adam::kSegments];
};

struct Hyper {
    float lr, beta1, beta2, eps, clip;
};

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void language_adam_kernel(Segments seg, float* __restrict__ head_w4, float* __restrict__ head_b4,
                                                                  const float* __restrict__ grads, float* __restrict__ m,
                                                                  float* __restrict__ v, const long long* __restrict__ step, Hyper h) {
    __shared__ float rate;
    if (threadIdx.x == 0) rate = adam::adam_rate(h.lr, h.beta1, h.beta2, *step + 1);
    __syncthreads();
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= seg.begin[adam::kSegments]) return;
    float* p = seg.ptr[0];
    long first = 0;
#pragma unroll
    for (int s = 1; s < adam::kSegments; ++s)
        if (i >= seg.begin[s]) { p = seg.ptr[s]; first = seg.begin[s]; }
    p += i - first;
    adam::adam_one(p, grads[i], m + i, v + i, rate, h.beta1, h.beta2, h.eps, h.clip);
    // the stacked images the next forward reads: w4 is the first 4 * 64 * 128 floats of the layout, b4 the 4 * 64 behind them
    constexpr long kW4 = 4L * 64 * 128;
    if (i < kW4) head_w4[i] = *p;
    else if (i < adam::kHeadStack) head_b4[i - kW4] = *p;
}

__global__ void bump_step_kernel(long long* step) { *step = *step + 1; }

struct HeadPtrs {
    const float* w[4];
    const float* b[4];
};
// head_w4 (4, 64, 128) <- head_w[0..3], head_b4 (4, 64) <- head_b[0..3]: what two torch.stack calls did
__global__ __launch_bounds__(kThreads) void gather_heads_kernel(HeadPtrs src, float* __restrict__ head_w4, float* __restrict__ head_b4) {
    constexpr int kW = 64 * 128, kB = 64;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < 4 * kW) {
        const int k = i / kW;
        const float* w = k == 0 ? src.w[0] : k == 1 ? src.w[1] : k == 2 ? src.w[2] : src.w[3];
        head_w4[i] = w[i - k * kW];
    } else if (i < 4 * kW + 4 * kB) {
        const int j = i - 4 * kW, k = j / kB;
        const float* b = k == 0 ? src.b[0] : k == 1 ? src.b[1] : k == 2 ? src.b[2] : src.b[3];
        head_b4[j] = b[j - k * kB];
    }
}

// part k of the variable `var` of adam::kFlat
float* variable(const mvnerf_language_adam* a, int var, int k) {
    switch (var) {
        case adam::kVarHeadW: return a->head_w[k];
        case adam::kVarHeadB: return a->head_b[k];
        case adam::kVarWc: return a->head_wc;
        case adam::kVarBc: return a->head_bc;
        default: return a->tail_w[var];
    }
}

Segments segments(const mvnerf_language_adam* a, int n5) {
    Segments s;
    int var[adam::kSegments], part[adam::kSegments];
    adam::flat_segments(n5, s.begin, var, part);
    for (int k = 0; k < adam::kSegments; ++k) s.ptr[k] = variable(a, var[k], part[k]);
    return s;
}

int validate_adam(const char* who, const mvnerf_language_call* c, const mvnerf_language_adam* a) {
    if (!c) return api_fail(MVNERF_E_ARG, "%s: null call", who);
    if (!a) return api_fail(MVNERF_E_ARG, "%s: null adam", who);
    if (!c->grads) return api_fail(MVNERF_E_ARG, "%s: null pointer (call->grads)", who);
    if (c->n5 <= 0 || c->n5 > 4096) return api_fail(MVNERF_E_ARG, "%s: n5=%d", who, c->n5);
    for (int k = 0; k < 4; ++k) {
        if (!a->head_w[k]) return api_fail(MVNERF_E_ARG, "%s: null pointer (head_w[%d])", who, k);
        if (!a->head_b[k]) return api_fail(MVNERF_E_ARG, "%s: null pointer (head_b[%d])", who, k);
    }
    for (int i = 0; i < 11; ++i)
        if (!a->tail_w[i]) return api_fail(MVNERF_E_ARG, "%s: null pointer (tail_w[%d])", who, i);
    const struct { const void* p; const char* name; } named[] = {{a->head_wc, "head_wc"}, {a->head_bc, "head_bc"}, {a->head_w4, "head_w4"},
                                                                 {a->head_b4, "head_b4"}, {a->m, "m"}, {a->v, "v"}, {a->step, "step"}};
    for (const auto& f : named)
        if (!f.p) return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, f.name);
    if (!(a->lr >= 0.0f)) return api_fail(MVNERF_E_ARG, "%s: lr=%g (>= 0)", who, (double)a->lr);
    if (!(a->beta1 >= 0.0f && a->beta1 < 1.0f)) return api_fail(MVNERF_E_ARG, "%s: beta1=%g (in [0, 1))", who, (double)a->beta1);
    if (!(a->beta2 >= 0.0f && a->beta2 < 1.0f)) return api_fail(MVNERF_E_ARG, "%s: beta2=%g (in [0, 1))", who, (double)a->beta2);
    if (!(a->eps >= 0.0f)) return api_fail(MVNERF_E_ARG, "%s: eps=%g (>= 0)", who, (double)a->eps);
    for (int k = 0; k < 4; ++k) {
        if (!aligned4(a->head_w[k])) return api_fail(MVNERF_E_ALIGN, "%s: head_w[%d] must be 4-byte aligned", who, k);
        if (!aligned4(a->head_b[k])) return api_fail(MVNERF_E_ALIGN, "%s: head_b[%d] must be 4-byte aligned", who, k);
    }
    for (int i = 0; i < 11; ++i)
        if (!aligned4(a->tail_w[i])) return api_fail(MVNERF_E_ALIGN, "%s: tail_w[%d] must be 4-byte aligned", who, i);
    for (const auto& f : named)
        if (f.p != a->step && !aligned4(f.p)) return api_fail(MVNERF_E_ALIGN, "%s: %s must be 4-byte aligned", who, f.name);
    if ((reinterpret_cast<uintptr_t>(a->step) & 7u) != 0) return api_fail(MVNERF_E_ALIGN, "%s: step must be 8-byte aligned", who);
    if (!aligned4(c->grads)) return api_fail(MVNERF_E_ALIGN, "%s: call->grads must be 4-byte aligned", who);
    return 0;
}

int apply(const char* who, const mvnerf_language_call* c, const mvnerf_language_adam* a, hipStream_t st) {
    const Segments seg = segments(a, c->n5);
    const long n = seg.begin[adam::kSegments];
    const Hyper h = {a->lr, a->beta1, a->beta2, a->eps, a->clip};
    hipLaunchKernelGGL(language_adam_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, seg, a->head_w4, a->head_b4,
                       c->grads, a->m, a->v, a->step, h);
    MV_HIP(hipGetLastError(), who);
    hipLaunchKernelGGL(bump_step_kernel, dim3(1), dim3(1), 0, st, a->step);
    MV_HIP(hipGetLastError(), who);
    return 0;
}

}  // namespace

extern "C" {

int mvnerf_language_apply_gradients(const mvnerf_language_call* call, const mvnerf_language_adam* a, mvnerf_stream_t stream) {
    MV_RC(validate_adam(kApply, call, a));
    return apply(kApply, call, a, static_cast<hipStream_t>(stream));
}

int mvnerf_language_train_step(const mvnerf_language_call* call, const mvnerf_language_adam* a, mvnerf_stream_t stream) {
    MV_RC(validate_adam(kStep, call, a));
    MV_RC(mvnerf::language_validate(call));
    const struct { const void *mine, *theirs; const char* name; } same[] = {
        {a->head_w4, call->head_w4, "head_w4"}, {a->head_b4, call->head_b4, "head_b4"}, {a->head_wc, call->head_wc, "head_wc"},
        {a->head_bc, call->head_bc, "head_bc"}};
    for (const auto& f : same)
        if (f.mine != f.theirs) return api_fail(MVNERF_E_ARG, "%s: adam->%s is not call->%s", kStep, f.name, f.name);
    for (int i = 0; i < 11; ++i)
        if (a->tail_w[i] != call->tail_w[i]) return api_fail(MVNERF_E_ARG, "%s: adam->tail_w[%d] is not call->tail_w[%d]", kStep, i, i);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HeadPtrs src;
    for (int k = 0; k < 4; ++k) { src.w[k] = a->head_w[k]; src.b[k] = a->head_b[k]; }
    hipLaunchKernelGGL(gather_heads_kernel, dim3((unsigned)((adam::kHeadStack + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, src, a->head_w4,
                       a->head_b4);
    MV_HIP(hipGetLastError(), kStep);
    MV_RC(mvnerf_language_loss_and_grads(call, stream));
    return apply(kStep, call, a, st);
}

}  // extern "C"
