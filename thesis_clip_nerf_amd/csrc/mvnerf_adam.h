// optimize() of the read-out (src/train_language.py:65-67: tf.keras.optimizers.Adam behind nerf_utils.py:8-12's clip-by-value) as scalar
// code, usable from device code (hipcc, language_opt.hip) and from a host build (gcc, tests/cpu_language_adam), and the one table of the
// flat gradient layout of mvnerf_language_loss_and_grads that language_api.hip and language_opt.hip both read.
//
//   adam_one    clip, m, v, p - lr_t m / (sqrt(v) + eps): train_ops.hip's adam_clip_kernel operation for operation, one rounding each.
//   adam_rate   lr_t = (float)(lr sqrt(1 - beta2^t) / (1 - beta1^t)) in double; beta^t of (double)beta by square-and-multiply from the
//               low bit of t upwards, so that the host build, the device and a NumPy restatement agree on every bit (pow does not promise).
//   kFlat       the 15 entries of `grads` in order (include/mvnerf_hip.h), each with the variable of mvnerf_language_adam it belongs to.
//   warmup_rate nerf_utils.WarmupScheduler / encoders.warmup_lr_lambda at the counter BEFORE its increment, in double, rounded once.
//   multi_plan  the chunk prefix of a list of tensors of uneven length, multi_find the tensor a chunk belongs to (no kernel yet: DESIGN.md 21).
//
// Arithmetic: compiled with -ffp-contract=off and correctly rounded divide / square root, as everything in this directory.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define MVA_HD __host__ __device__ __forceinline__
#define MVA_MEMBER __host__ __device__ __forceinline__
#else
#define MVA_HD static inline
#define MVA_MEMBER inline
#endif

namespace mvnerf {
namespace adam {

// beta^t, t >= 0: r = product of the squares beta^(2^k) at the set bits k of t, lowest bit first
MVA_HD double power(double beta, long long t) {
    double r = 1.0, s = beta;
    while (t > 0) {
        if (t & 1) r = r * s;
        s = s * s;
        t >>= 1;
    }
    return r;
}

// the bias-corrected rate of update t = 1, 2, ... (tf.keras Adam)
MVA_HD float adam_rate(float lr, float beta1, float beta2, long long t) {
    const double up = sqrt(1.0 - power((double)beta2, t));
    const double down = 1.0 - power((double)beta1, t);
    return (float)((double)lr * up / down);
}

// one element: the gradient clipped by value (clip > 0), both moments, the variable
MVA_HD void adam_one(float* p, float g, float* m, float* v, float lr_t, float beta1, float beta2, float eps, float clip) {
    if (clip > 0.0f) g = fminf(fmaxf(g, -clip), clip);
    const float mi = beta1 * *m + (1.0f - beta1) * g;
    const float vi = beta2 * *v + (1.0f - beta2) * g * g;
    *m = mi;
    *v = vi;
    *p = *p - lr_t * mi / (sqrtf(vi) + eps);
}

// The un-corrected rate of the update that finds `step` completed ones (Keras evaluates a schedule at `iterations`, so the first update of
// a warm-up has rate 0): target * step / warm while step <= warm (the product first), target while step <= after, a tenth of it behind.
// warm <= 0: no warm-up; after < 0: the rate never drops.  The bias correction is adam_rate(this, b1, b2, step + 1).
MVA_HD float warmup_rate(float target, double warm, double after, long long step) {
    const double t = (double)target, s = (double)step;
    if (warm > 0.0 && s <= warm) return (float)(t * s / warm);
    if (after < 0.0 || s <= after) return target;
    return (float)(t * 0.1);
}

// ---- many tensors of uneven length behind one launch: tensor t owns the chunks first_chunk[t] .. first_chunk[t + 1] of kMultiChunk
// elements each (the last one partial), a tensor without elements owns none ----
constexpr long long kMultiChunk = 4096;                     // 256 lanes x four 16-byte accesses

// first_chunk (count + 1) <- the prefix of ceil(n / kMultiChunk); returns its last entry, the number of chunks
MVA_HD long long multi_plan(const long long* n, int count, long long* first_chunk) {
    long long at = 0;
    for (int t = 0; t < count; ++t) {
        first_chunk[t] = at;
        if (n[t] > 0) at += (n[t] + kMultiChunk - 1) / kMultiChunk;
    }
    first_chunk[count] = at;
    return at;
}

// the LAST t in 0 .. count - 1 with first(t) <= chunk: of a run of equal entries (tensors without elements, then their successor) the
// one that owns the chunk.  chunk in 0 .. the total - 1; first(0) == 0.  multi_find_by reads the prefix through `first`, so that a
// kernel can search the table it has (an array of structs) with the code the host build tests.
template <class First>
MVA_HD int multi_find_by(First first, int count, long long chunk) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (first(mid) <= chunk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
struct MultiPrefix {
    const long long* first_chunk;
    MVA_MEMBER long long operator()(int t) const { return first_chunk[t]; }
};
MVA_HD int multi_find(const long long* first_chunk, int count, long long chunk) { return multi_find_by(MultiPrefix{first_chunk}, count, chunk); }

// ---- the flat layout of `grads`: head (w4, b4, wc, bc), block_0, block_1 (both weights, then both biases), output_layer ----
// An entry holds fixed + per_k * K floats (K = 64 n5).  var: the index into mvnerf_language_call.tail_w[] / mvnerf_language_adam.tail_w[]
// (the order of mvnerf_grasp_tail_pack, which is NOT the flat order), or one of the head's below; parts: the variables the entry is made
// of, in order and of equal size (w4 and b4 are the four activation_downscale layers).
constexpr int kVarHeadW = -1, kVarHeadB = -2, kVarWc = -3, kVarBc = -4;
struct FlatEntry {
    const char* name;
    long fixed, per_k;
    int var, parts;
};
constexpr int kFlatEntries = 15;
constexpr FlatEntry kFlat[kFlatEntries] = {
    {"w4", 4 * 64 * 128, 0, kVarHeadW, 4}, {"b4", 4 * 64, 0, kVarHeadB, 4}, {"wc", 64 * 256, 0, kVarWc, 1}, {"bc", 64, 0, kVarBc, 1},
    {"w0", 0, 128, 0, 1},  {"b0", 128, 0, 1, 1},   {"w1", 64 * 128, 0, 2, 1}, {"b1", 64, 0, 3, 1},  {"ws", 0, 64, 4, 1},
    {"w0b", 64 * 64, 0, 5, 1}, {"w1b", 64 * 64, 0, 7, 1}, {"b0b", 64, 0, 6, 1}, {"b1b", 64, 0, 8, 1},
    {"w_out", 64, 0, 9, 1}, {"b_out", 1, 0, 10, 1}};
constexpr int kSegments = 21;                               // the variables: 4 + 4 + 2 + 11
constexpr long kHeadStack = 4 * 64 * 128 + 4 * 64;          // floats of w4, b4: the part of the layout mirrored into head_w4 / head_b4

static inline long flat_floats(const FlatEntry& e, int n5) { return e.fixed + e.per_k * 64L * n5; }

// offsets (floats) of the 15 entries, [kFlatEntries] = the total
static inline void flat_offsets(int n5, long* at) {
    at[0] = 0;
    for (int i = 0; i < kFlatEntries; ++i) at[i + 1] = at[i] + flat_floats(kFlat[i], n5);
}

// flat index -> variable: every entry split into its equal parts.  Segment s (of kSegments) holds the flat indices begin[s] .. begin[s + 1]
// and is part part[s] of the variable var[s] (an entry's `var`).
static inline void flat_segments(int n5, long* begin, int* var, int* part) {
    long at[kFlatEntries + 1];
    flat_offsets(n5, at);
    int n = 0;
    for (int e = 0; e < kFlatEntries; ++e) {
        const long each = (at[e + 1] - at[e]) / kFlat[e].parts;
        for (int k = 0; k < kFlat[e].parts; ++k, ++n) {
            begin[n] = at[e] + k * each;
            var[n] = kFlat[e].var;
            part[n] = k;
        }
    }
    begin[n] = at[kFlatEntries];
}

}  // namespace adam
}  // namespace mvnerf
