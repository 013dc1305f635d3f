// "lane = row" building blocks of the GraspReadout kernels (grasp_head.hip, grasp_tail.hip): Y^T = W X^T on v_mfma_f32_32x32x2_f32 with
// A = packed weights from L2 and B = a row's activations held in accumulator order, so that the D registers of one product are the B
// operands of the next.
#pragma once

#include <hip/hip_runtime.h>

#include "mvnerf_mfma.h"

namespace mvnerf {

// Packed weights of one Dense layer (floats): chunk = 1 KiB = [lane][4 k-steps]; a set (KB, NBO) has chunk index ((kb * 4 + t) * NBO + nbo)
// and holds A[i][kk] on lane (i, h), with kk = 32 kb + 8 t + 4 h + e (the accumulator order: register 4 t + e of block kb on lane half h).
//
// acc[nbo] += A^T-product over KB input blocks held in accumulator order.  The A chunks of step (kb, t) + 1 are requested before the
// MFMAs of step (kb, t) are issued and pinned there (the weights come from L2: a round trip is as long as a step's 4 x NBO MFMAs).
template <int KB, int NBO>
__device__ __forceinline__ void dense_blocks(const float* __restrict__ packed, int lane, const f32x16 (&in)[KB], f32x16 (&acc)[NBO]) {
    const f32x4* w = reinterpret_cast<const f32x4*>(packed) + lane;
    f32x4 a[NBO], an[NBO];
#pragma unroll
    for (int nbo = 0; nbo < NBO; ++nbo) a[nbo] = w[nbo * 64];
#pragma unroll
    for (int st = 0; st < KB * 4; ++st) {
        const int kb = st >> 2, t = st & 3;
        if (st + 1 < KB * 4) {
#pragma unroll
            for (int nbo = 0; nbo < NBO; ++nbo) an[nbo] = w[((st + 1) * NBO + nbo) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nbo = 0; nbo < NBO; ++nbo) acc[nbo] = mfma(a[nbo][e], in[kb][4 * t + e], acc[nbo]);
        if (st + 1 < KB * 4) {
#pragma unroll
            for (int nbo = 0; nbo < NBO; ++nbo) a[nbo] = an[nbo];
        }
    }
}

// block nb (32 features) of row `point` of a row-major (N, F) tensor, in accumulator order: lane (j, h) register 4q + c = feature
// 32 nb + 8 q + 4 h + c
__device__ __forceinline__ f32x16 load_block(const float* __restrict__ rows, long point, int F, int nb, int h) {
    const f32x4* p = reinterpret_cast<const f32x4*>(rows + point * F + 32 * nb + 4 * h);
    f32x16 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 t4 = p[2 * q];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[4 * q + c] = t4[c];
    }
    return v;
}

__device__ __forceinline__ void store_block(float* __restrict__ rows, long point, int F, int nb, int h, const f32x16& v) {
    f32x4* p = reinterpret_cast<f32x4*>(rows + point * F + 32 * nb + 4 * h);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 t4 = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
        p[2 * q] = t4;
    }
}

// bias (F floats, plain order) of block nb in accumulator order
__device__ __forceinline__ f32x16 bias_block(const float* __restrict__ bias, int nb, int h) {
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = bias[32 * nb + (r & 3) + 8 * (r >> 2) + 4 * h];
    return v;
}

__device__ __forceinline__ float elu1(float x) { return x > 0.0f ? x : expm1f(x); }
// derivatives of elu in terms of its OUTPUT e = elu(u): elu'(u) = u > 0 ? 1 : e + 1 ; elu''(u) = u > 0 ? 0 : e + 1   (e > 0 <=> u > 0)
__device__ __forceinline__ float delu(float e) { return e > 0.0f ? 1.0f : e + 1.0f; }
__device__ __forceinline__ float ddelu(float e) { return e > 0.0f ? 0.0f : e + 1.0f; }
// elu' in terms of the pre-activation u
__device__ __forceinline__ float delu_pre(float u) { return u > 0.0f ? 1.0f : expf(u); }

}  // namespace mvnerf
