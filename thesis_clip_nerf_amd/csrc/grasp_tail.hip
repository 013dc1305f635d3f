// The per-pose part of GraspReadout (delta_ngf/layers.py:24-28, 39-41; the pre-activation ResNetMLPBlock of mvnerf/layers.py:262-298) with
// frozen weights, as a value pass and a vector-Jacobian pass - what the grasp-pose optimiser runs on the fused head's output
// (DESIGN.md 12).  For M = B * P rows and K = 64 n5:
//
//   x  (M, K)                                         the head's y, a pose's n5 rows of 64 side by side
//   h0 = elu(x) W0^T + b0        (K -> 128)           r0 = elu(h0) W1^T + b1     (128 -> 64)
//   x1 = x Ws^T + r0             (shortcut K -> 64)
//   h1 = elu(x1) W0'^T + b0'     (64 -> 64)           x2 = x1 + elu(h1) W1'^T + b1'
//   s  = relu(x2) . w_out + b_out
//
// Value: one workgroup = 32 rows, three waves x two 32-column blocks of the 192 wide outputs [h0 | x Ws].  A K-slice of 64 (one gripper
// offset) of the 32 rows is staged through LDS with coalesced loads, once as it is and once through elu (so elu costs one evaluation per
// element, not one per consuming wave); every wave reads its B operands from there and streams its A operands (packed weights) from L2.
// Each slice is summed in a fresh accumulator and added to the running total: blocked summation, the rounding of a 64-term sum plus n5
// additions instead of one K-term chain.  The 64 / 128-wide chain then runs on wave 0 with the row's values in accumulator order, as in
// grasp_head.hip.  Nothing is split along K, so nothing has to be combined: the same bits from run to run.
// VJP: one workgroup = 32 rows x a range of offsets; every wave first runs the chain backwards from the stashed pre-activations
// (h0, x1, h1, x2: 320 floats per row) to g_h0 (128) and g_x1 (64) - 256 MFMAs, repeated per wave rather than exchanged - and keeps them
// as B operands; it then produces 64 columns of g_x = (g_h0 W0) . elu'(x) + g_x1 Ws at a time.  Small M spreads the offsets over
// blockIdx.y.  fp32 throughout (the fp32 MFMA multiplies exactly).
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"
#include "mvnerf_blocks.h"
#include "mvnerf_mfma.h"
#include "mvnerf_tail.h"

namespace mvnerf {

namespace {

// the packed buffer's layout, the stash and the staging constants: mvnerf_tail.h
struct TailWeights {
    const float *w0, *b0, *w1, *b1, *ws, *w0b, *b0b, *w1b, *b1b, *w_out, *b_out;
};

__global__ void grasp_tail_pack_kernel(TailWeights w, int n5, float* __restrict__ dst) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long wide = kWide * n5, K = 64L * n5;
    if (idx >= 2 * wide + kSmall) return;
    const int lane = (int)((idx % 256) / 4), e = (int)(idx % 4), i = lane & 31, h = lane >> 5;
    float val;
    if (idx < wide) {                                        // F
        const long chunk = idx / 256;
        const int nb = (int)(chunk % 6), t = (int)((chunk / 6) % 8);
        const long c = chunk / 48, col = 64 * c + 8 * t + 4 * h + e;
        val = nb < 4 ? w.w0[(32 * nb + i) * K + col] : w.ws[(32 * (nb - 4) + i) * K + col];
    } else if (idx < 2 * wide) {                             // V
        const long chunk = (idx - wide) / 256, c = chunk / 48;
        const int q = (int)(chunk % 48), nbo = q & 1, kt = (q & 31) >> 1;
        const long col = 64 * c + 32 * nbo + i;
        const int kk = 8 * kt + 4 * h + e;
        val = q < 32 ? w.w0[kk * K + col] : w.ws[kk * K + col];
    } else {
        const int off = (int)(idx - 2 * wide);
        if (off >= kBias) {
            const int b = off - kBias;
            val = b < kOffB1 ? w.b0[b] : b < kOffB0b ? w.b1[b - kOffB1] : b < kOffB1b ? w.b0b[b - kOffB0b] : b < kOffWout ? w.b1b[b - kOffB1b]
                : b < kOffBout ? w.w_out[b - kOffWout] : (b == kOffBout && w.b_out) ? w.b_out[0] : 0.0f;
        } else {
            // dense_blocks sets: chunk ((kb * 4 + t) * NBO + nbo), kk = 32 kb + 8 t + 4 h + e, o = 32 nbo + i
            const int set = off < kC2 ? 0 : off < kC3 ? 1 : off < kB1 ? 2 : off < kB2 ? 3 : off < kB3 ? 4 : 5;
            const int base = set == 0 ? kC1 : set == 1 ? kC2 : set == 2 ? kC3 : set == 3 ? kB1 : set == 4 ? kB2 : kB3;
            const int nbo_count = set == 5 ? 4 : 2;
            const int chunk = (off - base) / 256, nbo = chunk % nbo_count, kt = chunk / nbo_count;
            const int kk = 8 * kt + 4 * h + e, o = 32 * nbo + i;        // 8 kt = 32 kb + 8 t
            val = set == 0 ? w.w1[o * 128 + kk] : set == 1 ? w.w0b[o * 64 + kk] : set == 2 ? w.w1b[o * 64 + kk]
                : set == 3 ? w.w1b[kk * 64 + o] : set == 4 ? w.w0b[kk * 64 + o] : w.w1[kk * 128 + o];
        }
    }
    dst[idx] = val;
}

// ---- value: x (M, 64 n5) -> success (M) [+ stash (M, 320)] -------------------------------------------------------------------------------
__global__ __launch_bounds__(kFwdThreads) void grasp_tail_fwd_kernel(const float* __restrict__ x, const float* __restrict__ packed, long M, int n5,
                                                                      float* __restrict__ success, float* __restrict__ stash) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 2 * 32 * kXs];          // [buffer][as it is | elu][row][64 (+4)]
    static_assert(2 * 2 * 32 * kXs >= 32 * kPre, "the wide outputs reuse the staging buffers");
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const long row0 = (long)blockIdx.x * 32, K = 64L * n5;
    const float* small = packed + 2 * kWide * n5;
    const float* bias = small + kBias;

    // staging: 32 rows x 16 float4 per slice, thread -> (row, float4) of up to three of them; rows past M read nothing and stage zeros
    f32x4 stg[3];
    auto gload = [&](int c) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int idx = tid + kFwdThreads * s, r = idx >> 4, c4 = idx & 15;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (idx < 512 && row0 + r < M) v = *reinterpret_cast<const f32x4*>(x + (row0 + r) * K + 64L * c + 4 * c4);
            stg[s] = v;
        }
    };
    auto swrite = [&](int buf) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int idx = tid + kFwdThreads * s, r = idx >> 4, c4 = idx & 15;
            if (idx < 512) {
                const f32x4 v = stg[s];
                const f32x4 ev = {elu1(v[0]), elu1(v[1]), elu1(v[2]), elu1(v[3])};
                float* dst = lds + (buf * 2) * 32 * kXs + r * kXs + 4 * c4;
                *reinterpret_cast<f32x4*>(dst) = v;
                *reinterpret_cast<f32x4*>(dst + 32 * kXs) = ev;
            }
        }
    };

    // waves 0, 1: blocks 0..3 = h0 (elu(x) W0^T + b0); wave 2: blocks 4, 5 = x Ws^T
    f32x16 tot[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (wave < 2) tot[k] = bias_block(bias + kOffB0, 2 * wave + k, h);
        else {
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[k][r] = 0.0f;
        }
    }
    const f32x4* wp = reinterpret_cast<const f32x4*>(packed) + lane + (2 * wave) * 64;       // chunk (step * 6 + 2 wave + k) at wp[(step * 6 + k) * 64]
    // the A operands ride kAhead k-steps (of 8 MFMAs) in front of their use in a ring of 8 register pairs: an L2 round trip is longer than
    // one step, and a SIMD holds one or two of these waves
    const int steps = 8 * n5;
    f32x4 ring[8][2];
#pragma unroll
    for (int st = 0; st < kAhead; ++st) {
        if (st < steps) {
            ring[st][0] = wp[st * 6 * 64];
            ring[st][1] = wp[st * 6 * 64 + 64];
        }
    }
    gload(0);
    for (int c = 0; c < n5; ++c) {
        swrite(c & 1);
        __syncthreads();                            // slice c is staged; everyone is done with slice c - 1 (the other buffer is free)
        if (c + 1 < n5) gload(c + 1);
        const float* src = lds + ((c & 1) * 2 + (wave < 2 ? 1 : 0)) * 32 * kXs + j * kXs + 4 * h;
        f32x16 acc[2];
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[k][r] = 0.0f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int step = c * 8 + t;
            if (step + kAhead < steps) {
                ring[(t + kAhead) & 7][0] = wp[(long)(step + kAhead) * 6 * 64];
                ring[(t + kAhead) & 7][1] = wp[(long)(step + kAhead) * 6 * 64 + 64];
            }
            const f32x4 b = *reinterpret_cast<const f32x4*>(src + 8 * t);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0] = mfma(ring[t][0][e], b[e], acc[0]);
                acc[1] = mfma(ring[t][1][e], b[e], acc[1]);
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[k][r] = tot[k][r] + acc[k][r];
    }
    __syncthreads();                                // the staging buffers are free: they now carry the 192 wide outputs to wave 0
#pragma unroll
    for (int k = 0; k < 2; ++k) store_block(lds, j, kPre, 2 * wave + k, h, tot[k]);
    __syncthreads();
    if (wave != 0) return;

    const long row = row0 + j;
    const bool ok = row < M;
    const bool keep = ok && stash != nullptr;
    f32x16 h0[4], x1[2];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        h0[nb] = load_block(lds, j, kPre, nb, h);
        if (keep) store_block(stash + kSH0, row, kTailStash, nb, h, h0[nb]);
#pragma unroll
        for (int r = 0; r < 16; ++r) h0[nb][r] = elu1(h0[nb][r]);
    }
    f32x16 r0[2] = {bias_block(bias + kOffB1, 0, h), bias_block(bias + kOffB1, 1, h)};
    dense_blocks<4, 2>(small + kC1, lane, h0, r0);
    f32x16 e1[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const f32x16 xs = load_block(lds, j, kPre, 4 + nb, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            x1[nb][r] = xs[r] + r0[nb][r];
            e1[nb][r] = elu1(x1[nb][r]);
        }
        if (keep) store_block(stash + kSX1, row, kTailStash, nb, h, x1[nb]);
    }
    f32x16 h1[2] = {bias_block(bias + kOffB0b, 0, h), bias_block(bias + kOffB0b, 1, h)};
    dense_blocks<2, 2>(small + kC2, lane, e1, h1);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        if (keep) store_block(stash + kSH1, row, kTailStash, nb, h, h1[nb]);
#pragma unroll
        for (int r = 0; r < 16; ++r) h1[nb][r] = elu1(h1[nb][r]);
    }
    f32x16 r1[2] = {bias_block(bias + kOffB1b, 0, h), bias_block(bias + kOffB1b, 1, h)};
    dense_blocks<2, 2>(small + kC3, lane, h1, r1);
    float part = 0.0f;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const f32x16 wo = bias_block(bias + kOffWout, nb, h);
        f32x16 x2;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            x2[r] = x1[nb][r] + r1[nb][r];
            part = part + fmaxf(x2[r], 0.0f) * wo[r];
        }
        if (keep) store_block(stash + kSX2, row, kTailStash, nb, h, x2);
    }
    const float other = __shfl_xor(part, 32);       // the row's other 32 features; added lower half first on both lanes
    const float s = (h == 0 ? part + other : other + part) + bias[kOffBout];
    if (ok && h == 0) success[row] = s;
}

// ---- VJP: g_s (M) or NULL (ones), stash -> g_x (M, 64 n5) --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grasp_tail_vjp_kernel(const float* __restrict__ x, const float* __restrict__ g_s,
                                                              const float* __restrict__ stash, const float* __restrict__ packed, long M, int n5,
                                                              float* __restrict__ g_x) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int c0 = (int)blockIdx.y * 4 + wave, c_step = 4 * (int)gridDim.y;
    if (c0 >= n5) return;
    const long row_raw = (long)blockIdx.x * 32 + j, K = 64L * n5;
    const bool ok = row_raw < M;
    const long row = ok ? row_raw : M - 1;          // rows past M repeat the last row and store nothing
    const float* small = packed + 2 * kWide * n5;
    const float* bias = small + kBias;
    const float gs = g_s ? g_s[row] : 1.0f;

    f32x16 g2[2], gx1[2], gh0[4];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const f32x16 x2 = load_block(stash + kSX2, row, kTailStash, nb, h), wo = bias_block(bias + kOffWout, nb, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) g2[nb][r] = x2[r] > 0.0f ? gs * wo[r] : 0.0f;
    }
    {
        f32x16 ge[2], gh1[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) ge[nb][r] = 0.0f;
        dense_blocks<2, 2>(small + kB1, lane, g2, ge);                      // W1'^T g_x2
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f32x16 h1 = load_block(stash + kSH1, row, kTailStash, nb, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                gh1[nb][r] = ge[nb][r] * delu_pre(h1[r]);
                ge[nb][r] = 0.0f;
            }
        }
        dense_blocks<2, 2>(small + kB2, lane, gh1, ge);                     // W0'^T g_h1
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f32x16 x1 = load_block(stash + kSX1, row, kTailStash, nb, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) gx1[nb][r] = g2[nb][r] + ge[nb][r] * delu_pre(x1[r]);
        }
    }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) gh0[nb][r] = 0.0f;
    dense_blocks<2, 4>(small + kB3, lane, gx1, gh0);                        // W1^T g_x1 (g_r0 = g_x1)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const f32x16 h0 = load_block(stash + kSH0, row, kTailStash, nb, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) gh0[nb][r] = gh0[nb][r] * delu_pre(h0[r]);
    }

    // 24 k-steps per offset (16 over g_h0, 8 over g_x1), two chunks each, contiguous in V; the A operands ride kAhead steps in front of
    // their use in a ring of 8 register pairs, across the offsets of this wave
    const f32x4* vw = reinterpret_cast<const f32x4*>(packed + kWide * n5) + lane;
    f32x4 ring[8][2];
#pragma unroll
    for (int st = 0; st < kAhead; ++st) {
        ring[st][0] = vw[((long)c0 * 48 + 2 * st) * 64];
        ring[st][1] = vw[((long)c0 * 48 + 2 * st + 1) * 64];
    }
#pragma unroll 1
    for (int c = c0; c < n5; c += c_step) {
        f32x16 pa[2], pb[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                pa[nb][r] = 0.0f;
                pb[nb][r] = 0.0f;
            }
#pragma unroll
        for (int st = 0; st < 24; ++st) {
            const int nst = st + kAhead;
            if (nst < 24 || c + c_step < n5) {
                const long q = nst < 24 ? (long)c * 48 + 2 * nst : (long)(c + c_step) * 48 + 2 * (nst - 24);
                ring[nst & 7][0] = vw[q * 64];
                ring[nst & 7][1] = vw[(q + 1) * 64];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (st < 16) {                                              // g_h0 W0, columns 64 c ..
                    const float b = gh0[st >> 2][4 * (st & 3) + e];
                    pa[0] = mfma(ring[st & 7][0][e], b, pa[0]);
                    pa[1] = mfma(ring[st & 7][1][e], b, pa[1]);
                } else {                                                    // g_x1 Ws
                    const float b = gx1[(st - 16) >> 2][4 * (st & 3) + e];
                    pb[0] = mfma(ring[st & 7][0][e], b, pb[0]);
                    pb[1] = mfma(ring[st & 7][1][e], b, pb[1]);
                }
            }
        }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f32x16 xb = load_block(x, row, (int)K, 2 * c + nb, h);
            f32x16 out;
#pragma unroll
            for (int r = 0; r < 16; ++r) out[r] = pa[nb][r] * delu_pre(xb[r]) + pb[nb][r];
            if (ok) store_block(g_x, row, (int)K, 2 * c + nb, h, out);
        }
    }
}

}  // namespace

size_t grasp_tail_packed_floats(int n5) { return (size_t)(2 * kWide) * n5 + kSmall; }
size_t grasp_tail_stash_floats() { return (size_t)kTailStash; }

hipError_t launch_grasp_tail_pack(const float* const* w, int n5, float* packed, hipStream_t st) {
    const TailWeights tw = {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10]};
    const size_t n = grasp_tail_packed_floats(n5);
    hipLaunchKernelGGL(grasp_tail_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tw, n5, packed);
    return hipGetLastError();
}

hipError_t launch_grasp_tail_fwd(const float* x, const float* packed, long M, int n5, float* success, float* stash, hipStream_t st) {
    hipLaunchKernelGGL(grasp_tail_fwd_kernel, dim3((unsigned)((M + 31) / 32)), dim3(kFwdThreads), 0, st, x, packed, M, n5, success, stash);
    return hipGetLastError();
}

hipError_t launch_grasp_tail_vjp(const float* x, const float* g_s, const float* stash, const float* packed, long M, int n5, float* g_x,
                                 hipStream_t st) {
    const long tiles = (M + 31) / 32;
    // few row tiles: spread the offsets over blockIdx.y (every workgroup repeats the chain; no sums cross workgroups)
    long gy = 512 / tiles;
    if (gy > (n5 + 3) / 4) gy = (n5 + 3) / 4;
    if (gy < 1) gy = 1;
    hipLaunchKernelGGL(grasp_tail_vjp_kernel, dim3((unsigned)tiles, (unsigned)gy), dim3(256), 0, st, x, g_s, stash, packed, M, n5, g_x);
    return hipGetLastError();
}

}  // namespace mvnerf

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------
extern "C" {

using mvnerf::aligned16;
using mvnerf::aligned4;
using mvnerf::hip_status;
constexpr long kTailMaxRows = 1L << 24;             // row * K stays far inside 63 bits, K itself inside an int

size_t mvnerf_grasp_tail_packed_floats(int n5) { return n5 > 0 && n5 <= 4096 ? mvnerf::grasp_tail_packed_floats(n5) : 0; }

int mvnerf_grasp_tail_pack(const float* w0, const float* b0, const float* w1, const float* b1, const float* ws, const float* w0b, const float* b0b,
                           const float* w1b, const float* b1b, const float* w_out, const float* b_out, int n5, float* packed,
                           mvnerf_stream_t stream) {
    if (!w0 || !b0 || !w1 || !b1 || !ws || !w0b || !b0b || !w1b || !b1b || !w_out || !packed)
        return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_tail_pack: null pointer (only b_out may be NULL)");
    if (n5 <= 0 || n5 > 4096) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_tail_pack: n5=%d", n5);
    if (!aligned16(packed)) return mvnerf::api_fail(MVNERF_E_ALIGN, "mvnerf_grasp_tail_pack: packed must be 16-byte aligned");
    const float* w[11] = {w0, b0, w1, b1, ws, w0b, b0b, w1b, b1b, w_out, b_out};
    return hip_status(mvnerf::launch_grasp_tail_pack(w, n5, packed, static_cast<hipStream_t>(stream)), "mvnerf_grasp_tail_pack");
}

int mvnerf_grasp_tail_fwd(const float* x, const float* packed, long M, int n5, float* success, float* stash, mvnerf_stream_t stream) {
    if (!x || !packed || !success) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_tail_fwd: null pointer (only stash may be NULL)");
    if (M <= 0 || M > kTailMaxRows || n5 <= 0 || n5 > 4096) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_tail_fwd: M=%ld n5=%d", M, n5);
    if (!aligned16(x) || !aligned16(packed) || !aligned16(stash) || !aligned4(success))
        return mvnerf::api_fail(MVNERF_E_ALIGN, "mvnerf_grasp_tail_fwd: x, packed, stash must be 16-byte aligned (success: 4)");
    return hip_status(mvnerf::launch_grasp_tail_fwd(x, packed, M, n5, success, stash, static_cast<hipStream_t>(stream)), "mvnerf_grasp_tail_fwd");
}

int mvnerf_grasp_tail_vjp(const float* x, const float* g_s, const float* stash, const float* packed, long M, int n5, float* g_x,
                          mvnerf_stream_t stream) {
    if (!x || !stash || !packed || !g_x) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_tail_vjp: null pointer (only g_s may be NULL)");
    if (M <= 0 || M > kTailMaxRows || n5 <= 0 || n5 > 4096) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_tail_vjp: M=%ld n5=%d", M, n5);
    if (!aligned16(x) || !aligned16(stash) || !aligned16(packed) || !aligned16(g_x) || !aligned4(g_s))
        return mvnerf::api_fail(MVNERF_E_ALIGN, "mvnerf_grasp_tail_vjp: x, stash, packed, g_x must be 16-byte aligned (g_s: 4)");
    return hip_status(mvnerf::launch_grasp_tail_vjp(x, g_s, stash, packed, M, n5, g_x, static_cast<hipStream_t>(stream)), "mvnerf_grasp_tail_vjp");
}

}  // extern "C"
