// The per-pose part of GraspReadout (grasp_tail.hip has the forward and its frozen-weight VJP) with TRAINABLE weights: the first backward with
// the cotangents the weight gradients are made of, and the derivative of that backward, which the nested tape of LanguageNeRF.train_step
// takes (a loss on d prediction / d pose differentiated with respect to the read-out).  With E = elu, E'(v) = v > 0 ? 1 : e^v,
// E''(v) = v > 0 ? 0 : e^v, H = [x2 > 0] and the forward
//     h0 = E(x) W0^T + b0;  x1 = x Ws^T + E(h0) W1^T + b1;  h1 = E(x1) W0'^T + b0';  x2 = x1 + E(h1) W1'^T + b1';  s = relu(x2) . w_out + b_out
//
// vjp_train: grasp_tail_vjp_kernel's products in its order (g_x has the same bits), and the wave that owns offset 0 of a row tile also writes
//     cot = [g_h0 | g_x1 | g_h1 | g_x2],  act = [E(h0) | E(x1) | E(h1) | g_s relu(x2)];  every wave writes ex = E(x) of its offsets.
// vjp_bwd (phi = <t, g_x>), two launches:
//   chain  (shaped like grasp_tail_fwd_kernel): the wide K -> 192 product on the staged operands (E'(x) . t | t), i.e. dh0 = da0 W0^T and
//          t Ws^T, then on wave 0 the tangent chain forward
//              de0 = E'(h0) . dh0;  dx1 = t Ws^T + de0 W1^T;  da1 = E'(x1) . dx1;  dh1 = da1 W0'^T;  de1 = E'(h1) . dh1;  dx2 = dx1 + de1 W1'^T
//          and the second-order cotangents backward
//              pi_h1 = E''(h1) . dh1 . (g_x2 W1');   pi_x1 = E'(x1) . (pi_h1 W0') + E''(x1) . dx1 . (g_h1 W0');
//              pi_h0 = E'(h0) . (pi_x1 W1) + E''(h0) . dh0 . (g_x1 W1)
//   wide   (shaped like grasp_tail_vjp_kernel): out_x = E'(x) . (pi_h0 W0) + E''(x) . t . (g_h0 W0) + pi_x1 Ws, the two products over W0
//          sharing every A operand.
// No sums cross workgroups; rows past M are clamped to row M - 1 on reads and never stored.  fp32 on v_mfma_f32_32x32x2_f32.
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"
#include "mvnerf_blocks.h"
#include "mvnerf_mfma.h"
#include "mvnerf_tail.h"

namespace mvnerf {

namespace {

constexpr int kCot = 320;                          // g_h0 (128) | g_x1 | g_h1 | g_x2: the stash's column offsets (kSH0 ..)
constexpr int kCot2 = 256, kPH0 = 0, kPX1 = 128, kPH1 = 192;      // pi_h0 (128) | pi_x1 | pi_h1

// E'(u) and E''(u) from one exponential
__device__ __forceinline__ void delu12(float u, float& d1, float& d2) {
    const float ev = expf(u);
    d1 = u > 0.0f ? 1.0f : ev;
    d2 = u > 0.0f ? 0.0f : ev;
}

__device__ __forceinline__ void zero_blocks2(f32x16 (&v)[2]) {
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) v[nb][r] = 0.0f;
}

// ---- first backward: grasp_tail_vjp_kernel + cot, act, ex ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grasp_tail_vjp_train_kernel(const float* __restrict__ x, const float* __restrict__ g_s,
                                                                    const float* __restrict__ stash, const float* __restrict__ packed, long M, int n5,
                                                                    float* __restrict__ g_x, float* __restrict__ cot, float* __restrict__ act,
                                                                    float* __restrict__ ex) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int c0 = (int)blockIdx.y * 4 + wave, c_step = 4 * (int)gridDim.y;
    if (c0 >= n5) return;
    const long row_raw = (long)blockIdx.x * 32 + j, K = 64L * n5;
    const bool ok = row_raw < M;
    const long row = ok ? row_raw : M - 1;          // rows past M repeat the last row and store nothing
    const bool scribe = ok && c0 == 0;              // one wave per row tile writes the chain's buffers
    const float* small = packed + 2 * kWide * n5;
    const float* bias = small + kBias;
    const float gs = g_s ? g_s[row] : 1.0f;

    f32x16 g2[2], gx1[2], gh0[4];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const f32x16 x2 = load_block(stash + kSX2, row, kTailStash, nb, h), wo = bias_block(bias + kOffWout, nb, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) g2[nb][r] = x2[r] > 0.0f ? gs * wo[r] : 0.0f;
        if (scribe) {
            f32x16 a;
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = x2[r] > 0.0f ? gs * x2[r] : 0.0f;
            store_block(cot + kSX2, row, kCot, nb, h, g2[nb]);
            store_block(act + kSX2, row, kCot, nb, h, a);
        }
    }
    {
        f32x16 ge[2], gh1[2];
        zero_blocks2(ge);
        dense_blocks<2, 2>(small + kB1, lane, g2, ge);                      // W1'^T g_x2
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f32x16 h1 = load_block(stash + kSH1, row, kTailStash, nb, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                gh1[nb][r] = ge[nb][r] * delu_pre(h1[r]);
                ge[nb][r] = 0.0f;
            }
            if (scribe) {
                f32x16 a;
#pragma unroll
                for (int r = 0; r < 16; ++r) a[r] = elu1(h1[r]);
                store_block(cot + kSH1, row, kCot, nb, h, gh1[nb]);
                store_block(act + kSH1, row, kCot, nb, h, a);
            }
        }
        dense_blocks<2, 2>(small + kB2, lane, gh1, ge);                     // W0'^T g_h1
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f32x16 x1 = load_block(stash + kSX1, row, kTailStash, nb, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) gx1[nb][r] = g2[nb][r] + ge[nb][r] * delu_pre(x1[r]);
            if (scribe) {
                f32x16 a;
#pragma unroll
                for (int r = 0; r < 16; ++r) a[r] = elu1(x1[r]);
                store_block(cot + kSX1, row, kCot, nb, h, gx1[nb]);
                store_block(act + kSX1, row, kCot, nb, h, a);
            }
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
        if (scribe) {
            f32x16 a;
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = elu1(h0[r]);
            store_block(cot + kSH0, row, kCot, nb, h, gh0[nb]);
            store_block(act + kSH0, row, kCot, nb, h, a);
        }
    }

    // the wide output as in grasp_tail_vjp_kernel: 24 k-steps per offset (16 over g_h0, 8 over g_x1), A operands kAhead steps in front
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
        zero_blocks2(pa);
        zero_blocks2(pb);
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
            f32x16 out, e;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                out[r] = pa[nb][r] * delu_pre(xb[r]) + pb[nb][r];
                e[r] = elu1(xb[r]);
            }
            if (ok) {
                store_block(g_x, row, (int)K, 2 * c + nb, h, out);
                store_block(ex, row, (int)K, 2 * c + nb, h, e);
            }
        }
    }
}

// ---- derivative of the first backward, chain part: dh0 | t Ws^T wide, then tangents forward and second-order cotangents backward on wave 0 ----
__global__ __launch_bounds__(kFwdThreads) void grasp_tail_bwd_chain_kernel(const float* __restrict__ x, const float* __restrict__ t_x,
                                                                            const float* __restrict__ g_s, const float* __restrict__ stash,
                                                                            const float* __restrict__ cot, const float* __restrict__ packed, long M,
                                                                            int n5, float* __restrict__ out_gs, float* __restrict__ cot2,
                                                                            float* __restrict__ tan, float* __restrict__ dex) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 2 * 32 * kXs];          // [buffer][t | E'(x) . t][row][64 (+4)]
    static_assert(2 * 2 * 32 * kXs >= 32 * kPre, "the wide outputs reuse the staging buffers");
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const long row0 = (long)blockIdx.x * 32, K = 64L * n5;
    const float* small = packed + 2 * kWide * n5;
    const float* bias = small + kBias;

    // staging as in grasp_tail_fwd_kernel, of x and t; rows past M read nothing and stage zeros
    f32x4 stx[3], stt[3];
    auto gload = [&](int c) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int idx = tid + kFwdThreads * s, r = idx >> 4, c4 = idx & 15;
            f32x4 vx = {0.0f, 0.0f, 0.0f, 0.0f}, vt = {0.0f, 0.0f, 0.0f, 0.0f};
            if (idx < 512 && row0 + r < M) {
                vx = *reinterpret_cast<const f32x4*>(x + (row0 + r) * K + 64L * c + 4 * c4);
                vt = *reinterpret_cast<const f32x4*>(t_x + (row0 + r) * K + 64L * c + 4 * c4);
            }
            stx[s] = vx;
            stt[s] = vt;
        }
    };
    auto swrite = [&](int buf, int c) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int idx = tid + kFwdThreads * s, r = idx >> 4, c4 = idx & 15;
            if (idx < 512) {
                const f32x4 vx = stx[s], vt = stt[s];
                const f32x4 da = {delu_pre(vx[0]) * vt[0], delu_pre(vx[1]) * vt[1], delu_pre(vx[2]) * vt[2], delu_pre(vx[3]) * vt[3]};
                float* dst = lds + (buf * 2) * 32 * kXs + r * kXs + 4 * c4;
                *reinterpret_cast<f32x4*>(dst) = vt;
                *reinterpret_cast<f32x4*>(dst + 32 * kXs) = da;
                if (row0 + r < M) *reinterpret_cast<f32x4*>(dex + (row0 + r) * K + 64L * c + 4 * c4) = da;       // da0 = E'(x) . t
            }
        }
    };

    // waves 0, 1: blocks 0..3 = dh0 = da0 W0^T; wave 2: blocks 4, 5 = t Ws^T
    f32x16 tot[2];
    zero_blocks2(tot);
    const f32x4* wp = reinterpret_cast<const f32x4*>(packed) + lane + (2 * wave) * 64;
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
        swrite(c & 1, c);
        __syncthreads();                            // slice c is staged; everyone is done with slice c - 1 (the other buffer is free)
        if (c + 1 < n5) gload(c + 1);
        const float* src = lds + ((c & 1) * 2 + (wave < 2 ? 1 : 0)) * 32 * kXs + j * kXs + 4 * h;
        f32x16 acc[2];
        zero_blocks2(acc);
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

    const bool ok = row0 + j < M;
    const long row = ok ? row0 + j : M - 1;         // rows past M repeat the last row and store nothing
    const float gs = g_s ? g_s[row] : 1.0f;

    // tangents forward
    f32x16 dx1[2] = {load_block(lds, j, kPre, 4, h), load_block(lds, j, kPre, 5, h)};        // t Ws^T
    {
        f32x16 de0[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const f32x16 dh0 = load_block(lds, j, kPre, nb, h), h0 = load_block(stash + kSH0, row, kTailStash, nb, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) de0[nb][r] = delu_pre(h0[r]) * dh0[r];
            if (ok) store_block(tan + kSH0, row, kCot, nb, h, de0[nb]);
        }
        dense_blocks<4, 2>(small + kC1, lane, de0, dx1);                    // + de0 W1^T
    }
    f32x16 dh1[2], dx2[2];
    {
        f32x16 da1[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f32x16 x1 = load_block(stash + kSX1, row, kTailStash, nb, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) da1[nb][r] = delu_pre(x1[r]) * dx1[nb][r];
            if (ok) store_block(tan + kSX1, row, kCot, nb, h, da1[nb]);
        }
        zero_blocks2(dh1);
        dense_blocks<2, 2>(small + kC2, lane, da1, dh1);                    // da1 W0'^T
        f32x16 de1[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f32x16 h1 = load_block(stash + kSH1, row, kTailStash, nb, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                de1[nb][r] = delu_pre(h1[r]) * dh1[nb][r];
                dx2[nb][r] = dx1[nb][r];
            }
            if (ok) store_block(tan + kSH1, row, kCot, nb, h, de1[nb]);
        }
        dense_blocks<2, 2>(small + kC3, lane, de1, dx2);                    // dx1 + de1 W1'^T
    }
    float part = 0.0f;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const f32x16 x2 = load_block(stash + kSX2, row, kTailStash, nb, h), wo = bias_block(bias + kOffWout, nb, h);
        f32x16 tg;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float hd = x2[r] > 0.0f ? dx2[nb][r] : 0.0f;
            part = part + hd * wo[r];
            tg[r] = gs * hd;
        }
        if (ok) store_block(tan + kSX2, row, kCot, nb, h, tg);
    }
    const float other = __shfl_xor(part, 32);       // the row's other 32 features; added lower half first on both lanes
    if (ok && h == 0) out_gs[row] = part + other;

    // second-order cotangents backward
    f32x16 ph1[2], px1[2];
    {
        f32x16 gx2[2] = {load_block(cot + kSX2, row, kCot, 0, h), load_block(cot + kSX2, row, kCot, 1, h)}, te1[2];
        zero_blocks2(te1);
        dense_blocks<2, 2>(small + kB1, lane, gx2, te1);                    // g_x2 W1'
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f32x16 h1 = load_block(stash + kSH1, row, kTailStash, nb, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float d1, d2;
                delu12(h1[r], d1, d2);
                ph1[nb][r] = (d2 * dh1[nb][r]) * te1[nb][r];
            }
            if (ok) store_block(cot2 + kPH1, row, kCot2, nb, h, ph1[nb]);
        }
    }
    {
        f32x16 gh1[2] = {load_block(cot + kSH1, row, kCot, 0, h), load_block(cot + kSH1, row, kCot, 1, h)}, ta1[2], u[2];
        zero_blocks2(ta1);
        zero_blocks2(u);
        dense_blocks<2, 2>(small + kB2, lane, gh1, ta1);                    // g_h1 W0'
        dense_blocks<2, 2>(small + kB2, lane, ph1, u);                      // pi_h1 W0'
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f32x16 x1 = load_block(stash + kSX1, row, kTailStash, nb, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float d1, d2;
                delu12(x1[r], d1, d2);
                px1[nb][r] = d1 * u[nb][r] + (d2 * dx1[nb][r]) * ta1[nb][r];
            }
            if (ok) store_block(cot2 + kPX1, row, kCot2, nb, h, px1[nb]);
        }
    }
    {
        f32x16 gx1[2] = {load_block(cot + kSX1, row, kCot, 0, h), load_block(cot + kSX1, row, kCot, 1, h)}, te0[4], v[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                te0[nb][r] = 0.0f;
                v[nb][r] = 0.0f;
            }
        dense_blocks<2, 4>(small + kB3, lane, gx1, te0);                    // g_x1 W1
        dense_blocks<2, 4>(small + kB3, lane, px1, v);                      // pi_x1 W1
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const f32x16 dh0 = load_block(lds, j, kPre, nb, h), h0 = load_block(stash + kSH0, row, kTailStash, nb, h);
            f32x16 ph0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float d1, d2;
                delu12(h0[r], d1, d2);
                ph0[r] = d1 * v[nb][r] + (d2 * dh0[r]) * te0[nb][r];
            }
            if (ok) store_block(cot2 + kPH0, row, kCot2, nb, h, ph0);
        }
    }
}

// ---- derivative of the first backward, wide part: cot, cot2 -> out_x -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void grasp_tail_bwd_wide_kernel(const float* __restrict__ x, const float* __restrict__ t_x,
                                                                   const float* __restrict__ cot, const float* __restrict__ cot2,
                                                                   const float* __restrict__ packed, long M, int n5, float* __restrict__ out_x) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int c0 = (int)blockIdx.y * 4 + wave, c_step = 4 * (int)gridDim.y;
    if (c0 >= n5) return;
    const long row_raw = (long)blockIdx.x * 32 + j, K = 64L * n5;
    const bool ok = row_raw < M;
    const long row = ok ? row_raw : M - 1;          // rows past M repeat the last row and store nothing

    f32x16 ph0[4], gh0[4], px1[2];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        ph0[nb] = load_block(cot2 + kPH0, row, kCot2, nb, h);
        gh0[nb] = load_block(cot + kSH0, row, kCot, nb, h);
    }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) px1[nb] = load_block(cot2 + kPX1, row, kCot2, nb, h);

    // 24 k-steps per offset as in grasp_tail_vjp_kernel; the 16 over W0 feed two accumulations (pi_h0 W0 and g_h0 W0) from one A operand
    const f32x4* vw = reinterpret_cast<const f32x4*>(packed + kWide * n5) + lane;
    f32x4 ring[8][2];
#pragma unroll
    for (int st = 0; st < kAhead; ++st) {
        ring[st][0] = vw[((long)c0 * 48 + 2 * st) * 64];
        ring[st][1] = vw[((long)c0 * 48 + 2 * st + 1) * 64];
    }
#pragma unroll 1
    for (int c = c0; c < n5; c += c_step) {
        f32x16 pa[2], pt[2], pb[2];
        zero_blocks2(pa);
        zero_blocks2(pt);
        zero_blocks2(pb);
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
                if (st < 16) {                                              // pi_h0 W0 and g_h0 W0, columns 64 c ..
                    const float bp = ph0[st >> 2][4 * (st & 3) + e], bg = gh0[st >> 2][4 * (st & 3) + e];
                    pa[0] = mfma(ring[st & 7][0][e], bp, pa[0]);
                    pa[1] = mfma(ring[st & 7][1][e], bp, pa[1]);
                    pt[0] = mfma(ring[st & 7][0][e], bg, pt[0]);
                    pt[1] = mfma(ring[st & 7][1][e], bg, pt[1]);
                } else {                                                    // pi_x1 Ws
                    const float b = px1[(st - 16) >> 2][4 * (st & 3) + e];
                    pb[0] = mfma(ring[st & 7][0][e], b, pb[0]);
                    pb[1] = mfma(ring[st & 7][1][e], b, pb[1]);
                }
            }
        }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f32x16 xb = load_block(x, row, (int)K, 2 * c + nb, h), tb = load_block(t_x, row, (int)K, 2 * c + nb, h);
            f32x16 out;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float d1, d2;
                delu12(xb[r], d1, d2);
                out[r] = d1 * pa[nb][r] + (d2 * tb[r]) * pt[nb][r] + pb[nb][r];
            }
            if (ok) store_block(out_x, row, (int)K, 2 * c + nb, h, out);
        }
    }
}

// few row tiles: spread the offsets over blockIdx.y, as launch_grasp_tail_vjp does (no sums cross workgroups)
dim3 wide_grid(long M, int n5) {
    const long tiles = (M + 31) / 32;
    long gy = 512 / tiles;
    if (gy > (n5 + 3) / 4) gy = (n5 + 3) / 4;
    if (gy < 1) gy = 1;
    return dim3((unsigned)tiles, (unsigned)gy);
}

}  // namespace

hipError_t launch_grasp_tail_vjp_train(const float* x, const float* g_s, const float* stash, const float* packed, long M, int n5, float* g_x,
                                       float* cot, float* act, float* ex, hipStream_t st) {
    hipLaunchKernelGGL(grasp_tail_vjp_train_kernel, wide_grid(M, n5), dim3(256), 0, st, x, g_s, stash, packed, M, n5, g_x, cot, act, ex);
    return hipGetLastError();
}

hipError_t launch_grasp_tail_vjp_bwd(const float* x, const float* t_x, const float* g_s, const float* stash, const float* cot, const float* packed,
                                     long M, int n5, float* out_gs, float* out_x, float* cot2, float* tan, float* dex, hipStream_t st) {
    hipLaunchKernelGGL(grasp_tail_bwd_chain_kernel, dim3((unsigned)((M + 31) / 32)), dim3(kFwdThreads), 0, st, x, t_x, g_s, stash, cot, packed, M, n5,
                       out_gs, cot2, tan, dex);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || out_x == nullptr) return e;
    hipLaunchKernelGGL(grasp_tail_bwd_wide_kernel, wide_grid(M, n5), dim3(256), 0, st, x, t_x, cot, cot2, packed, M, n5, out_x);
    return hipGetLastError();
}

}  // namespace mvnerf

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------
extern "C" {

using mvnerf::aligned16;
using mvnerf::aligned4;
using mvnerf::hip_status;
constexpr long kTrainMaxRows = 1L << 24;            // row * K stays far inside 63 bits, K itself inside an int

int mvnerf_grasp_tail_vjp_train(const float* x, const float* g_s, const float* stash, const float* packed, long M, int n5, float* g_x, float* cot,
                                float* act, float* ex, mvnerf_stream_t stream) {
    if (!x || !stash || !packed || !g_x || !cot || !act || !ex)
        return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_tail_vjp_train: null pointer (only g_s may be NULL)");
    if (M <= 0 || M > kTrainMaxRows || n5 <= 0 || n5 > 4096) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_tail_vjp_train: M=%ld n5=%d", M, n5);
    if (!aligned16(x) || !aligned16(stash) || !aligned16(packed) || !aligned16(g_x) || !aligned16(cot) || !aligned16(act) || !aligned16(ex) ||
        !aligned4(g_s))
        return mvnerf::api_fail(MVNERF_E_ALIGN, "mvnerf_grasp_tail_vjp_train: x, stash, packed, g_x, cot, act, ex must be 16-byte aligned (g_s: 4)");
    return hip_status(mvnerf::launch_grasp_tail_vjp_train(x, g_s, stash, packed, M, n5, g_x, cot, act, ex, static_cast<hipStream_t>(stream)),
                    "mvnerf_grasp_tail_vjp_train");
}

int mvnerf_grasp_tail_vjp_bwd(const float* x, const float* t_x, const float* g_s, const float* stash, const float* cot, const float* packed, long M,
                              int n5, float* out_gs, float* out_x, float* cot2, float* tan, float* dex, mvnerf_stream_t stream) {
    if (!x || !t_x || !stash || !cot || !packed || !out_gs || !cot2 || !tan || !dex)
        return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_tail_vjp_bwd: null pointer (only g_s and out_x may be NULL)");
    if (M <= 0 || M > kTrainMaxRows || n5 <= 0 || n5 > 4096) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_tail_vjp_bwd: M=%ld n5=%d", M, n5);
    if (!aligned16(x) || !aligned16(t_x) || !aligned16(stash) || !aligned16(cot) || !aligned16(packed) || !aligned16(out_x) ||
        !aligned16(cot2) || !aligned16(tan) || !aligned16(dex) || !aligned4(g_s) || !aligned4(out_gs))
        return mvnerf::api_fail(MVNERF_E_ALIGN,
                                "mvnerf_grasp_tail_vjp_bwd: x, t_x, stash, cot, packed, out_x, cot2, tan, dex must be 16-byte aligned (g_s, out_gs: 4)");
    return hip_status(mvnerf::launch_grasp_tail_vjp_bwd(x, t_x, g_s, stash, cot, packed, M, n5, out_gs, out_x, cot2, tan, dex,
                                                      static_cast<hipStream_t>(stream)),
                    "mvnerf_grasp_tail_vjp_bwd");
}

}  // extern "C"
